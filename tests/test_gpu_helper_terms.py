"""The narrow MFE kernel's split steps with the publish terms looked up by the helper waves and the fML bases carried
(sf_mfe_fast.hip.h: SF_FAST_HELPER_TERMS, SF_FAST_FBASE_CARRY), product library through the C ABI: energies, and structures where
a traceback runs, bit-exact against the oracle.  The helper's terms run at the widths 100, 117 and 120 only
(helper_terms_util.TERMS_WIDTHS says why); the other widths exercise the carried bases next to the parent's term path.  CPU twin: tests/test_helper_terms_emul.py."""
import numpy as np
import pytest

from scanfold_amd import params
import helper_terms_util as hu
import role_loops_util as ru

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(gpu_engine):
    gpu_engine.load_params(params.default_params())
    gpu_engine.set_kernel_mode(0)
    return gpu_engine


@pytest.fixture(scope="module")
def orc(default_params):
    from oracle import oracle as o
    o.build()
    o.set_params(default_params)
    o.set_constraint(None, None)
    return o


@pytest.mark.parametrize("W", hu.WIDTHS)
def test_uniform_gc_rich_and_n_rows(eng, orc, W):
    arr = hu.rows(W, 1536, 256, 256, 6000 + W)  # 2 048: every workgroup of the persistent grid folds several in a row
    if W in ru.LIST_WIDTHS:
        assert ru.longest_list(arr).max() > 64, W
    assert (eng.mfe_batch(arr) == orc.mfe_batch(arr)).all(), W


@pytest.mark.parametrize("W", hu.WIDTHS)
def test_pairs_in_row_one_and_column_w(eng, orc, W):
    arr = hu.ends_pair_rows(W, 512, 6100 + W)
    assert (eng.mfe_batch(arr) == orc.mfe_batch(arr)).all(), W
    e, db = eng.mfe_trace_batch(arr[:16])
    assert [(db[k], int(e[k])) for k in range(16)] == [orc.mfe(bytes(r).decode()) for r in arr[:16]], W


@pytest.mark.parametrize("W", (64, 120))
def test_traced_rows_among_swept_ones(eng, orc, W):
    ru.check_traced(eng, orc, W, 146, 6200 + W)  # 1 022 rows, 146 of them traced


@pytest.mark.parametrize("W,span", [(100, 70), (120, 90)])
def test_base_pair_span_below_the_width(eng, orc, W, span):
    assert ru.split_d0(W) < span < W
    arr = hu.rows(W, 768, 128, 128, 6300 + W)
    eng.set_max_bp_span(span)
    orc.set_max_bp_span(span)
    try:
        assert (eng.mfe_batch(arr) == orc.mfe_batch(arr)).all(), W
        e, db = eng.mfe_trace_batch(arr[:16])
        assert [(db[k], int(e[k])) for k in range(16)] == [orc.mfe(bytes(r).decode()) for r in arr[:16]], W
    finally:
        eng.set_max_bp_span(0)
        orc.set_max_bp_span(0)


@pytest.mark.parametrize("W", hu.POISON_WIDTHS)
@pytest.mark.parametrize("pattern", ("1", "2", "3", "4", "5"))
def test_poison_builds(eng, orc, monkeypatch, W, pattern):
    arr = hu.rows(W, 384, 64, 64, 6400 + W)
    ref = orc.mfe_batch(arr)
    monkeypatch.setenv("SCANFOLD_MFE_POISON", pattern)
    assert (eng.mfe_batch(arr) == ref).all(), (W, pattern)
    e, db = eng.mfe_trace_batch(arr[:8])
    assert [(db[k], int(e[k])) for k in range(8)] == [orc.mfe(bytes(r).decode()) for r in arr[:8]], (W, pattern)
