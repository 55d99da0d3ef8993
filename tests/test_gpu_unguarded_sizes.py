"""The narrow MFE kernel's short diagonals without guards (sf_mfe_fast.hip.h, SF_STEP_SHORT_A / B / C), product library through
the C ABI.  4 096 rows per width — four per persistent workgroup on 256 CUs, so a workgroup folds several in a row and what the
previous fold left in the rolling tables is what a wrong read would find; the poly-GC hairpins (out of the int16 range at the
large widths) come first.  CPU twin, with the read-by-read shadow check: tests/test_unguarded_sizes.py."""
import numpy as np
import pytest

from scanfold_amd import params
import unguarded_sizes_util as uu

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


_PRODUCT = {}


def product(eng, W):
    """(rows, energies of the product route) of a width, computed once"""
    if W not in _PRODUCT:
        arr = uu.gpu_rows(W)
        _PRODUCT[W] = (arr, eng.mfe_batch(arr))
    return _PRODUCT[W]


@pytest.mark.parametrize("W", uu.WIDTHS)
def test_energies_exact_kernel_oracle_and_rerun(eng, orc, W):
    arr, e = product(eng, W)
    assert arr.shape == (4096, W) and all(bytes(r) in (bytes(uu.poly_gc(W, 4)), bytes(uu.poly_gc(W, 5))) for r in arr[:8])
    try:
        eng.set_kernel_mode(1)  # the exact int32 kernel
        exact = eng.mfe_batch(arr)
    finally:
        eng.set_kernel_mode(0)
    assert (e == exact).all(), (W, np.nonzero(e != exact)[0][:8])
    pick = np.arange(0, 4096, 16)  # 256 rows spread evenly
    assert (e[pick] == orc.mfe_batch(arr[pick])).all(), W
    assert (eng.mfe_batch(arr) == e).all(), W  # bit for bit, twice


@pytest.mark.parametrize("W", uu.WIDTHS)
def test_structures(eng, orc, W):
    arr, _ = product(eng, W)
    rows = arr[np.arange(0, 4096, 64)]  # 64 rows: a poly-GC one, uniform, GC-rich and all-N ones
    e, db = eng.mfe_trace_batch(rows)
    assert [(db[k], int(e[k])) for k in range(64)] == [orc.mfe(bytes(r).decode()) for r in rows], W


@pytest.mark.parametrize("W", uu.POISON_WIDTHS)
@pytest.mark.parametrize("pattern", ("1", "2", "3", "4", "5"))
def test_poison_patterns_move_nothing(eng, monkeypatch, W, pattern):
    arr, e = product(eng, W)
    monkeypatch.setenv("SCANFOLD_MFE_POISON", pattern)
    assert (eng.mfe_batch(arr) == e).all(), (W, pattern)
