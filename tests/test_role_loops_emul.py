"""The narrow MFE kernel's split steps as one loop per role of a wave (sf_mfe_fast.hip.h, SfRole), on the CPU emulation build:
energies and structures bit-exact against the oracle at the widths where a role boundary moves.  The emulation's barrier is a
counter over fibers, so a role body with a barrier too few or too many never gets here.  GPU twin: tests/test_gpu_role_loops.py."""
import numpy as np
import pytest

from scanfold_amd import params
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


@pytest.mark.parametrize("W", ru.WIDTHS)
def test_random_rows(emul, orc, W):
    arr = ru.random_rows(W, 256, W)
    assert (emul.mfe_batch(arr) == orc.mfe_batch(arr)).all(), W


@pytest.mark.parametrize("W", ru.WIDTHS)
def test_gc_rich_rows_fill_the_list_past_one_wave(emul, orc, W):
    arr = ru.gc_rows(W, 256, 1000 + W)
    if W in ru.LIST_WIDTHS:
        assert ru.longest_list(arr).max() > 64, W
    assert (emul.mfe_batch(arr) == orc.mfe_batch(arr)).all(), W


@pytest.mark.parametrize("W", ru.WIDTHS)
def test_every_seventh_row_traced(emul, orc, W):
    ru.check_traced(emul, orc, W, 8, 2000 + W)  # 56 rows, 8 of them traced


@pytest.mark.parametrize("W,pattern", [(64, "1"), (64, "5"), (120, "1"), (120, "5")])
def test_poison_builds(emul, orc, monkeypatch, W, pattern):
    arr = np.concatenate([ru.random_rows(W, 24, 3000 + W), ru.gc_rows(W, 24, 3100 + W)])
    ref = orc.mfe_batch(arr)
    monkeypatch.setenv("SCANFOLD_MFE_POISON", pattern)
    assert (emul.mfe_batch(arr) == ref).all(), (W, pattern)
    e, db = emul.mfe_trace_batch(arr[:4])
    assert [(db[k], int(e[k])) for k in range(4)] == [orc.mfe(bytes(r).decode()) for r in arr[:4]], (W, pattern)


def test_constraint_row_per_fold(emul, orc):
    ru.check_constrained(emul, orc, 100, 24, 4100)
