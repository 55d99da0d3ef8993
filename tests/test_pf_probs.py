"""The base-pair probabilities of a whole record under a span (sf_pf_banded_probs, include/scanfold_hip_long.h): the kernel
source compiled for the CPU against the oracle's bpp matrix (oracle.pf for short records, oracle.pf_cubic in long double at
433 nt): the sparse pair list, the unpaired probabilities and the positional entropies at degenerate bands, around a wave's
64 lanes, on records whose band is live up to its edge and under constraints; what the outputs must satisfy among
themselves; the C ABI; whole.pf_probs; the combined driver's --global_bpp.  The checks and the bars are in
pf_probs_util.py, shared with test_gpu_pf_probs.py."""
import numpy as np
import pytest

from scanfold_amd import _lib, params
from long_pf_util import forget_cubic_references  # noqa: F401  (an autouse fixture)
from long_util import hairpin_rich
import pf_probs_util as pp


@pytest.fixture(scope="module")
def emul():
    from emul_engine import emul_engine
    e = emul_engine()
    e.load_params(params.default_params())
    return e


def test_degenerate_bands(emul, oracle):
    pp.check_degenerate_bands(emul, oracle)


@pytest.mark.parametrize("L", [63, 64, 65])
@pytest.mark.parametrize("wide", [False, True])
def test_whole_triangle_around_a_wave(emul, oracle, L, wide):
    """B = L: rows of 64 and 65 cells; at 65 nt the ballot's second chunk holds one cell"""
    pp.check_whole_triangle(emul, oracle, L, 1000 if wide else L)


@pytest.mark.parametrize("kind,S", pp.EDGE_CASES)
def test_live_band_equals_cubic_reference(emul, oracle, kind, S):
    pp.check_live_edge(emul, oracle, kind, 433, S)


def test_constraints(emul, oracle):
    pp.check_constraints(emul, oracle)


def test_consistency_without_the_oracle(emul, oracle):
    pp.check_consistency(emul, oracle)


def test_classic_outputs_are_pf_banded_and_twice_the_same_bits(emul, oracle):
    pp.check_identity(emul, oracle)


def test_cutoffs_filter_one_list(emul, oracle):
    pp.check_cutoffs(emul, oracle)


def test_c_abi(emul):
    pp.check_abi(emul)


def test_route(emul, monkeypatch):
    pp.check_route(emul, monkeypatch)


def test_cpu_twin_has_no_probabilities():
    import os
    from oracle import oracle as orc
    orc.build()
    twin = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "libscanfold_cpu.so")
    if not os.path.exists(twin):
        pytest.skip("the CPU twin of the C ABI was not built")
    eng = _lib.Engine(device=0, lib_path=twin)
    assert not eng.has_pf_banded_probs()
    with pytest.raises(_lib.ScanFoldHipError):
        eng.pf_banded_probs("ACGU" * 120)
    with pytest.raises(_lib.ScanFoldHipError):
        eng.pf_banded_probs_times()


def test_combined_driver_global_bpp(emul, tmp_path, monkeypatch):
    seq = hairpin_rich(np.random.default_rng(150), 600)
    pp.run_global_bpp(emul, tmp_path, monkeypatch, seq, 150, ["-w", "40", "-s", "30", "-r", "3", "--type", "mono", "--seed", "2"],
                      0.01)


def test_driver_refusals(tmp_path, monkeypatch):
    pp.check_driver_refusals(tmp_path, monkeypatch)
