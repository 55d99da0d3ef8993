"""The maximum-expected-accuracy structure of a pair list (sf_mea_pairs) and of a whole record under a span
(sf_pf_banded_mea, include/scanfold_hip_long.h): the kernel source compiled for the CPU against a Python restatement of the
header's model, which is itself checked against the enumeration of all structures; synthetic lists at every band and partner
count at which the kernels take another path; records whose band is live up to its edge against the oracle's
probabilities; constraints; a block record; the C ABI; whole.pf_mea; the combined driver's --global_mea.  The checks and the
bars are in pf_mea_util.py, shared with test_gpu_pf_mea.py."""
import numpy as np
import pytest

from scanfold_amd import _lib, params
from long_pf_util import forget_cubic_references  # noqa: F401  (an autouse fixture)
from long_util import hairpin_rich
import pf_mea_util as pm
import pf_probs_util as pp

EMUL_LONG = 1500  # nt of the block record the emulation takes (the MI355X takes 70 000)


@pytest.fixture(scope="module")
def emul():
    from emul_engine import emul_engine
    e = emul_engine()
    e.load_params(params.default_params())
    return e


def test_reference_equals_enumeration():
    pm.check_reference_against_enumeration()


def test_empty_tiny_and_full_bands(emul):
    pm.check_empty_and_tiny(emul)


@pytest.mark.parametrize("band", [30, 64, 65, 129, 200, 400])
def test_random_lists(emul, band):
    pm.check_random_band(emul, band)


@pytest.mark.parametrize("n", [63, 64, 65, 300])
def test_many_partners_of_one_position(emul, n):
    pm.check_many_partners(emul, n)


@pytest.mark.parametrize("L", [200, 167])
def test_fifth_and_later_partner_inside_a_chunk(emul, L):
    pm.check_near_partners(emul, L)


def test_all_ties(emul):
    pm.check_all_ties(emul)


def test_degenerate_bands(emul, oracle):
    pm.check_degenerate_bands(emul, oracle)


@pytest.mark.parametrize("L", [63, 64, 65])
def test_whole_triangle_around_a_wave(emul, oracle, L):
    pm.check_whole_triangle(emul, oracle, L)


@pytest.mark.parametrize("kind,S", pp.EDGE_CASES)
def test_live_band(emul, oracle, kind, S):
    pm.check_live_edge(emul, oracle, kind, S)


def test_constraints(emul, oracle):
    pm.check_constraints(emul, oracle)


def test_block_record(emul, oracle):
    pm.check_long_record(emul, oracle, EMUL_LONG, 120, 7, 1000)


def test_c_abi(emul):
    pm.check_abi(emul)


def test_route(emul, monkeypatch):
    pm.check_route(emul, monkeypatch)


def test_cpu_twin_has_no_mea():
    import os
    from oracle import oracle as orc
    orc.build()
    twin = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "libscanfold_cpu.so")
    assert os.path.exists(twin), "oracle.build() did not produce the CPU twin of the C ABI"
    eng = _lib.Engine(device=0, lib_path=twin)
    assert not eng.has_mea_pairs() and not eng.has_pf_banded_mea()
    with pytest.raises(_lib.ScanFoldHipError):
        eng.mea_pairs(4, np.zeros(0, dtype=_lib.PAIR_PROB_DTYPE), np.ones(4))
    with pytest.raises(_lib.ScanFoldHipError):
        eng.pf_banded_mea("ACGU" * 120)
    with pytest.raises(_lib.ScanFoldHipError):
        eng.mea_times()


def test_combined_driver_global_mea(emul, tmp_path, monkeypatch):
    seq = hairpin_rich(np.random.default_rng(150), 240)
    pm.run_global_mea(emul, tmp_path, monkeypatch, seq, 60, ["-w", "40", "-s", "30", "-r", "3", "--type", "mono", "--seed", "2"],
                      0.01, 1.0)


def test_driver_refusals(tmp_path, monkeypatch):
    pm.check_driver_refusals(tmp_path, monkeypatch)
