"""The partition function under a base-pair span in banded tables (sf_pf_banded) on the MI355X: against oracle.pf_cubic in
long double under the span on records whose band is live up to its last diagonal (the full grid of spans), against
sf_pf_long under the same span at 3 000 nt (free, constrained, randomised and rescaled parameter sets, the alphabet of a
record), with four hints, twice for bit-identical results, on the heterogeneous record that no single-scale exterior loop
holds, and past the old length limit on block records of 40 000 and 70 000 nt whose exact answer the oracle gives block by
block (a bracket pair past position 32 767 and past 65 535).  The checks and the bar are in banded_pf_util.py, shared with
the emulation's test_pf_banded.py."""
import pytest

from scanfold_amd import params
from long_pf_util import forget_cubic_references  # noqa: F401  (an autouse fixture)
from test_gpu_long_fold import model_at
import banded_pf_util as bp

pytestmark = pytest.mark.gpu

SPANS = [30, 33, 64, 65, 129, 400]


def test_degenerate_bands(gpu_engine, oracle):
    bp.check_degenerate_bands(gpu_engine, oracle)


@pytest.mark.parametrize("S", SPANS)
@pytest.mark.parametrize("L", [433, 1200])
@pytest.mark.parametrize("kind", ["random", "hairpin_rich", "multiloop_rich"])
def test_live_band_equals_cubic_reference(gpu_engine, oracle, kind, L, S):
    bp.check_edge_record(gpu_engine, oracle, kind, L, S)


@pytest.mark.parametrize("S", SPANS[:-1])
def test_multiloop_closed_at_the_band_edge(gpu_engine, oracle, S):
    """(not under span 400: multiloop_edge_record's closing pair of width 399 has p = 0.45 in the ensemble of that record,
    so its reference would not depend on the band's edge as assert_live_edge demands)"""
    bp.check_multiloop_edge(gpu_engine, oracle, 433, S)


@pytest.mark.parametrize("S", [100, 401, 1000])
def test_equal_to_pf_long(gpu_engine, S):
    bp.check_equal_to_pf_long(gpu_engine, 3000, S)


@pytest.mark.parametrize("S", [100, 401, 1000])
def test_equal_to_pf_long_under_other_parameter_sets(gpu_engine, oracle, S):
    """params.random_params(3), and sets with enthalpies rescaled to 25 C and to 50 C"""
    try:
        gpu_engine.load_params(params.random_params(3))
        bp.check_equal_to_pf_long_loaded(gpu_engine, 3000, S, 3000 + S)
    finally:
        gpu_engine.load_params(params.default_params())
    for T in (25.0, 50.0):
        with model_at(gpu_engine, oracle, T):
            bp.check_equal_to_pf_long_loaded(gpu_engine, 3000, S, 3000 + S)


@pytest.mark.parametrize("S", [100, 401, 1000])
def test_alphabet_equal_to_pf_long(gpu_engine, S):
    bp.check_alphabet(gpu_engine, 3000, S)


def test_span_not_below_the_length(gpu_engine):
    bp.check_span_not_below_length(gpu_engine)


def test_span_not_below_the_length_65(gpu_engine):
    bp.check_span_not_below_length(gpu_engine, 65)


def test_hints(gpu_engine):
    bp.check_hints(gpu_engine, 3000, 401)


def test_twice_bit_for_bit(gpu_engine):
    bp.check_twice(gpu_engine, 3000, 401)


def test_heterogeneous_record(gpu_engine, oracle):
    """ten G/C-only and ten A/U-only blocks of 300 nt under span 100, 7 900 nt"""
    bp.check_heterogeneous(gpu_engine, oracle, 100)


@pytest.mark.parametrize("L,seed,constrained", [(40000, 4, False), (40000, 41, True), (70000, 7, False), (70000, 71, True)])
def test_block_records_past_the_old_limit(gpu_engine, oracle, L, seed, constrained):
    bp.check_pooled_record(gpu_engine, oracle, L, 120, seed, constrained)


def test_errors(gpu_engine):
    bp.check_errors(gpu_engine)
