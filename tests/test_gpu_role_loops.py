"""The narrow MFE kernel's split steps as one loop per role of a wave (sf_mfe_fast.hip.h, SfRole), product library through the
C ABI: energies and structures bit-exact against the oracle at the widths where a role boundary moves.
CPU twin: tests/test_role_loops_emul.py."""
import numpy as np
import pytest

from scanfold_amd import params
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


@pytest.mark.parametrize("W", ru.WIDTHS)
def test_random_rows(eng, orc, W):
    arr = ru.random_rows(W, 2048, W)
    assert (eng.mfe_batch(arr) == orc.mfe_batch(arr)).all(), W


@pytest.mark.parametrize("W", ru.WIDTHS)
def test_gc_rich_rows_fill_the_list_past_one_wave(eng, orc, W):
    arr = ru.gc_rows(W, 256, 1000 + W)
    if W in ru.LIST_WIDTHS:
        assert ru.longest_list(arr).max() > 64, W
    assert (eng.mfe_batch(arr) == orc.mfe_batch(arr)).all(), W


@pytest.mark.parametrize("W", ru.WIDTHS)
def test_every_seventh_row_traced(eng, orc, W):
    ru.check_traced(eng, orc, W, 293, 2000 + W)  # 2 051 rows


def test_persistent_loop_takes_further_folds(eng, orc):
    """more rows than the persistent grid has workgroups (4 per CU): every workgroup takes further folds from the counter and
    meets the last-fold path; twice, the same energies everywhere"""
    W, n = 120, 6000
    arr = ru.random_rows(W, n, 5120)
    a, b = eng.mfe_batch(arr), eng.mfe_batch(arr)
    assert (a == b).all()
    pick = np.random.default_rng(7).choice(n, 512, replace=False)
    assert (a[pick] == orc.mfe_batch(arr[pick])).all()


@pytest.mark.parametrize("W,pattern", [(64, "1"), (64, "5"), (120, "1"), (120, "5")])
def test_poison_builds(eng, orc, monkeypatch, W, pattern):
    arr = np.concatenate([ru.random_rows(W, 384, 3000 + W), ru.gc_rows(W, 128, 3100 + W)])
    ref = orc.mfe_batch(arr)
    monkeypatch.setenv("SCANFOLD_MFE_POISON", pattern)
    assert (eng.mfe_batch(arr) == ref).all(), (W, pattern)
    e, db = eng.mfe_trace_batch(arr[:16])
    assert [(db[k], int(e[k])) for k in range(16)] == [orc.mfe(bytes(r).decode()) for r in arr[:16]], (W, pattern)


def test_constraint_row_per_fold(eng, orc):
    ru.check_constrained(eng, orc, 100, 256, 4100)
