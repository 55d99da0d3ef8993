"""Whole-record constraints through all eight entry points on the MI355X: the checks of tests/whole_hc_util.py on the product
engine.  Records of 57 to 120 nt; every case takes well under a second of device time."""
import pytest

import whole_hc_util as hc

pytestmark = pytest.mark.gpu


def test_edges_of_one_constraint(gpu_engine, oracle):
    hc.check_edges_of_one_constraint(gpu_engine, oracle)


def test_packing_across_rows_and_chunks(gpu_engine):
    hc.check_packing_across_rows_and_chunks(gpu_engine)


def test_refusals(gpu_engine):
    hc.check_refusals(gpu_engine)


def test_a_constraint_of_dots_is_no_constraint(gpu_engine):
    hc.check_a_constraint_of_dots_is_no_constraint(gpu_engine)
