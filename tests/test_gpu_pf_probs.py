"""The base-pair probabilities of a whole record under a span (sf_pf_banded_probs) on the MI355X: the checks of
test_pf_probs.py, and what the emulation is too slow for: 1 200 nt over the full grid of spans against oracle.pf_cubic in
long double, randomised and rescaled parameter sets at 433 nt, and block records of 40 000 and 70 000 nt whose list,
unpaired probabilities and entropies the oracle gives block by block (pairs past position 32 767 and past 65 535).  The
checks and the bars are in pf_probs_util.py."""
import pytest

from scanfold_amd import params
from long_pf_util import forget_cubic_references  # noqa: F401  (an autouse fixture)
from test_gpu_long_fold import synthetic_set
import pf_probs_util as pp

pytestmark = pytest.mark.gpu

SPANS = [30, 33, 64, 65, 129, 400]


def test_degenerate_bands(gpu_engine, oracle):
    pp.check_degenerate_bands(gpu_engine, oracle)


@pytest.mark.parametrize("L", [63, 64, 65])
@pytest.mark.parametrize("wide", [False, True])
def test_whole_triangle_around_a_wave(gpu_engine, oracle, L, wide):
    pp.check_whole_triangle(gpu_engine, oracle, L, 1000 if wide else L)


@pytest.mark.parametrize("kind,S", pp.EDGE_CASES)
def test_live_band_equals_cubic_reference(gpu_engine, oracle, kind, S):
    pp.check_live_edge(gpu_engine, oracle, kind, 433, S)


@pytest.mark.parametrize("S", SPANS)
def test_live_band_1200(gpu_engine, oracle, S):
    pp.check_live_edge(gpu_engine, oracle, "hairpin_rich", 1200, S)


def test_other_parameter_sets(gpu_engine, oracle):
    """params.random_params(3), and a set with enthalpies rescaled to 25 C, at 433 nt under span 129"""
    try:
        p = params.random_params(3)
        gpu_engine.load_params(p)
        pp.check_loaded(gpu_engine, oracle, p, 433, 129, 433 + 3)
        p = synthetic_set()
        gpu_engine.load_params(p)
        gpu_engine.set_temperature(25.0)
        pp.check_loaded(gpu_engine, oracle, p.at_temperature(25.0), 433, 129, 433 + 25)
    finally:
        gpu_engine.load_params(params.default_params())


def test_constraints(gpu_engine, oracle):
    pp.check_constraints(gpu_engine, oracle)


def test_consistency_without_the_oracle(gpu_engine, oracle):
    pp.check_consistency(gpu_engine, oracle)


def test_classic_outputs_are_pf_banded_and_twice_the_same_bits(gpu_engine, oracle):
    pp.check_identity(gpu_engine, oracle)


def test_cutoffs_filter_one_list(gpu_engine, oracle):
    pp.check_cutoffs(gpu_engine, oracle)


@pytest.mark.parametrize("L,S,seed,constrained,past", [(40000, 120, 4, True, 32767), (70000, 60, 7, False, 65535)])
def test_block_records_past_the_old_limits(gpu_engine, oracle, L, S, seed, constrained, past):
    pp.check_pooled_record(gpu_engine, oracle, L, S, seed, constrained, past)


def test_c_abi(gpu_engine):
    pp.check_abi(gpu_engine)


def test_route(gpu_engine, monkeypatch):
    pp.check_route(gpu_engine, monkeypatch)
