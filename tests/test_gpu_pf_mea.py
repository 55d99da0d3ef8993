"""The maximum-expected-accuracy structure of a pair list (sf_mea_pairs) and of a whole record under a span
(sf_pf_banded_mea) on the MI355X: the checks of test_pf_mea.py on the device, with the block record at 70 000 nt (pairs
past position 65 535).  The checks and the bars are in pf_mea_util.py."""
import pytest

from long_pf_util import forget_cubic_references  # noqa: F401  (an autouse fixture)
import pf_mea_util as pm
import pf_probs_util as pp

pytestmark = pytest.mark.gpu


def test_empty_tiny_and_full_bands(gpu_engine):
    pm.check_empty_and_tiny(gpu_engine)


@pytest.mark.parametrize("band", [30, 64, 65, 129, 200, 400])
def test_random_lists(gpu_engine, band):
    pm.check_random_band(gpu_engine, band)


@pytest.mark.parametrize("n", [63, 64, 65, 300])
def test_many_partners_of_one_position(gpu_engine, n):
    pm.check_many_partners(gpu_engine, n)


@pytest.mark.parametrize("L", [200, 167])
def test_fifth_and_later_partner_inside_a_chunk(gpu_engine, L):
    pm.check_near_partners(gpu_engine, L)


def test_all_ties(gpu_engine):
    pm.check_all_ties(gpu_engine)


def test_degenerate_bands(gpu_engine, oracle):
    pm.check_degenerate_bands(gpu_engine, oracle)


@pytest.mark.parametrize("L", [63, 64, 65])
def test_whole_triangle_around_a_wave(gpu_engine, oracle, L):
    pm.check_whole_triangle(gpu_engine, oracle, L)


@pytest.mark.parametrize("kind,S", pp.EDGE_CASES)
def test_live_band(gpu_engine, oracle, kind, S):
    pm.check_live_edge(gpu_engine, oracle, kind, S)


def test_constraints(gpu_engine, oracle):
    pm.check_constraints(gpu_engine, oracle)


def test_block_record_past_65535(gpu_engine, oracle):
    pm.check_long_record(gpu_engine, oracle, 70000, 120, 7, 65535)


def test_c_abi(gpu_engine):
    pm.check_abi(gpu_engine)


def test_route(gpu_engine, monkeypatch):
    pm.check_route(gpu_engine, monkeypatch)
