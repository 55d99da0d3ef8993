"""The narrow MFE kernel's split steps with the publish terms looked up by the helper waves and the fML bases carried
(sf_mfe_fast.hip.h: SF_FAST_HELPER_TERMS, SF_FAST_FBASE_CARRY), on the CPU emulation build: energies, and structures where a
traceback runs, bit-exact against the oracle.  The emulation build runs every fold under the shadow check of the unguarded sizes
(sf_emul_check_absent): what the helpers leave behind the cells of a ring row is marked as written, so a read for an absent loop
size that found it would stop the run; and it stops on a split step whose row has no room for the terms.
The helper's terms run at the widths 100, 117 and 120 only (helper_terms_util.TERMS_WIDTHS says why); the other widths, and the
poison patterns at W = 64, exercise the carried bases next to the parent's term path.
GPU twin: tests/test_gpu_helper_terms.py."""
import numpy as np
import pytest

from scanfold_amd import params
import helper_terms_util as hu
import role_loops_util as ru


@pytest.fixture(scope="module")
def emul():
    from emul_engine import emul_engine
    eng = emul_engine()
    eng.load_params(params.default_params())
    return eng


@pytest.fixture(scope="module")
def orc(default_params):
    from oracle import oracle as o
    o.build()
    o.set_params(default_params)
    o.set_constraint(None, None)
    return o


@pytest.mark.parametrize("W", range(64, 129))
def test_the_terms_fit_behind_the_cells_of_every_split_diagonal(W):
    assert hu.crossing_area_fits(W), W


def test_which_widths_run_the_helper_terms():
    assert tuple(W for W in hu.WIDTHS if hu.runs_helper_terms(W)) == hu.TERMS_WIDTHS
    assert set(hu.TERMS_WIDTHS) & set(hu.POISON_WIDTHS) == {100, 120}


@pytest.mark.parametrize("W", hu.WIDTHS)
def test_uniform_gc_rich_and_n_rows(emul, orc, W):
    arr = hu.rows(W, 64, 32, 32, 6000 + W)  # 128 here, 2 048 on the GPU
    if W in ru.LIST_WIDTHS:
        assert ru.longest_list(arr).max() > 64, W
    assert (emul.mfe_batch(arr) == orc.mfe_batch(arr)).all(), W


@pytest.mark.parametrize("W", hu.WIDTHS)
def test_pairs_in_row_one_and_column_w(emul, orc, W):
    arr = hu.ends_pair_rows(W, 32, 6100 + W)
    assert (emul.mfe_batch(arr) == orc.mfe_batch(arr)).all(), W
    e, db = emul.mfe_trace_batch(arr[:4])
    assert [(db[k], int(e[k])) for k in range(4)] == [orc.mfe(bytes(r).decode()) for r in arr[:4]], W


@pytest.mark.parametrize("W", (64, 120))
def test_traced_rows_among_swept_ones(emul, orc, W):
    ru.check_traced(emul, orc, W, 6, 6200 + W)  # 42 rows, 6 of them traced


@pytest.mark.parametrize("W,span", [(100, 70), (120, 90)])
def test_base_pair_span_below_the_width(emul, orc, W, span):
    """the span ends inside the split phase: the helper's lists thin out to nothing and every later cell publishes "none" """
    assert ru.split_d0(W) < span < W
    arr = hu.rows(W, 48, 8, 8, 6300 + W)
    emul.set_max_bp_span(span)
    orc.set_max_bp_span(span)
    try:
        assert (emul.mfe_batch(arr) == orc.mfe_batch(arr)).all(), W
        e, db = emul.mfe_trace_batch(arr[:4])
        assert [(db[k], int(e[k])) for k in range(4)] == [orc.mfe(bytes(r).decode()) for r in arr[:4]], W
    finally:
        emul.set_max_bp_span(0)
        orc.set_max_bp_span(0)


@pytest.mark.parametrize("W", hu.POISON_WIDTHS)
@pytest.mark.parametrize("pattern", ("1", "2", "3", "4", "5"))
def test_poison_builds(emul, orc, monkeypatch, W, pattern):
    arr = hu.rows(W, 16, 8, 8, 6400 + W)
    ref = orc.mfe_batch(arr)
    monkeypatch.setenv("SCANFOLD_MFE_POISON", pattern)
    assert (emul.mfe_batch(arr) == ref).all(), (W, pattern)
    e, db = emul.mfe_trace_batch(arr[:2])
    assert [(db[k], int(e[k])) for k in range(2)] == [orc.mfe(bytes(r).decode()) for r in arr[:2]], (W, pattern)
