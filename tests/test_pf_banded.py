"""The partition function under a base-pair span in banded tables (sf_pf_banded, include/scanfold_hip_long.h): the kernel
source compiled for the CPU against the oracle, against oracle.pf_cubic in long double under the span on records whose band
is live up to its edge, against sf_pf_long under the same span, and on records built from blocks whose exact answer the
oracle gives block by block; the C ABI's refusals; the combined driver's --global_ensemble_banded.  The checks and the bar
are in banded_pf_util.py, shared with test_gpu_pf_banded.py.

What runs here is sized for the emulation (every lane a fiber): 433 and 1 200 nt and the short list of spans that
test_banded_fold.py uses.  The heterogeneous record, which no single-scale exterior loop holds, runs here under span 60
(7 140 nt, about ten seconds of fibers); of the records past SF_MAX_LONG the emulation folds a reduced one of 2 000 nt."""
import numpy as np
import pytest

from scanfold_amd import _lib, params
from long_pf_util import forget_cubic_references  # noqa: F401  (an autouse fixture)
from long_util import hairpin_rich
import banded_pf_util as bp


@pytest.fixture(scope="module")
def emul():
    from emul_engine import emul_engine
    e = emul_engine()
    e.load_params(params.default_params())
    return e


def test_degenerate_bands(emul, oracle):
    bp.check_degenerate_bands(emul, oracle)


@pytest.mark.parametrize("kind,L,S", [("random", 433, 30), ("hairpin_rich", 433, 65), ("multiloop_rich", 433, 33),
                                      ("multiloop_rich", 433, 129), ("hairpin_rich", 1200, 64), ("random", 433, 400)])
def test_live_band_equals_cubic_reference(emul, oracle, kind, L, S):
    bp.check_edge_record(emul, oracle, kind, L, S)


@pytest.mark.parametrize("S", [30, 64])
def test_multiloop_closed_at_the_band_edge(emul, oracle, S):
    bp.check_multiloop_edge(emul, oracle, 433, S)


@pytest.mark.parametrize("S", [40, 101])
def test_equal_to_pf_long(emul, S):
    bp.check_equal_to_pf_long(emul, 433, S)


def test_span_not_below_the_length(emul):
    bp.check_span_not_below_length(emul)


def test_span_not_below_the_length_65(emul):
    """one nucleotide past a wave's 64: every row and column of the band table is a whole row or column of the triangle"""
    bp.check_span_not_below_length(emul, 65)


def test_hints(emul):
    bp.check_hints(emul, 433, 101)


def test_twice_bit_for_bit(emul):
    bp.check_twice(emul, 433, 101)


def test_heterogeneous_record(emul, oracle):
    bp.check_heterogeneous(emul, oracle, 60)


def test_block_record_reduced(emul, oracle):
    """2 000 nt under span 60, the last block constrained: the reduced form of the GPU file's 40 000 and 70 000 nt"""
    bp.check_pooled_record(emul, oracle, 2000, 60, 3, constrained=True)


def test_errors(emul):
    bp.check_errors(emul)


def test_cpu_twin_has_no_banded_partition_function():
    import os
    from oracle import oracle as orc
    orc.build()
    twin = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "libscanfold_cpu.so")
    if not os.path.exists(twin):
        pytest.skip("the CPU twin of the C ABI was not built")
    eng = _lib.Engine(device=0, lib_path=twin)
    assert not eng.has_pf_banded()
    with pytest.raises(_lib.ScanFoldHipError):
        eng.pf_banded("ACGU" * 120)


def test_combined_driver_global_ensemble_banded(emul, tmp_path, monkeypatch):
    seq = hairpin_rich(np.random.default_rng(150), 600)
    bp.run_global_ensemble_banded(emul, tmp_path, monkeypatch, seq, 150,
                                  ["-w", "40", "-s", "30", "-r", "3", "--type", "mono", "--seed", "2"])


def test_driver_refusals(tmp_path, monkeypatch):
    bp.check_driver_refusals(tmp_path, monkeypatch)
