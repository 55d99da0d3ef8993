"""Whole-record constraints through all eight entry points on the CPU emulation build (tests/whole_hc_util.py has the checks
and what they are for; tests/test_gpu_whole_constraints.py runs them on the MI355X).  Here the emulation's launch log also
shows that a refused call launched nothing."""
import pytest

from scanfold_amd import params
import whole_hc_util as hc


@pytest.fixture(scope="module")
def emul():
    from emul_engine import emul_engine
    e = emul_engine()
    e.load_params(params.default_params())
    return e


def launched(eng, call):
    """-> the kernels call() launched, as the emulation logged them"""
    from emul_engine import launch_log
    launch_log(eng)
    call()
    return launch_log(eng)


def test_the_strings():
    hc.check_the_strings()


def test_edges_of_one_constraint(emul, oracle):
    hc.check_edges_of_one_constraint(emul, oracle)


def test_packing_across_rows_and_chunks(emul):
    hc.check_packing_across_rows_and_chunks(emul)


def test_refusals_launch_nothing(emul):
    assert launched(emul, lambda: emul.fold_long(hc.record(57), hc.CONS[57]))  # (the log does see a fold)
    hc.check_refusals(emul, lambda call: launched(emul, call))


def test_a_constraint_of_dots_is_no_constraint(emul):
    hc.check_a_constraint_of_dots_is_no_constraint(emul)
