"""The narrow MFE kernel's short diagonals without guards (sf_mfe_fast.hip.h, SF_STEP_SHORT_A / B / C), on the CPU emulation build.

From d0 = 10 on the narrow kernels run the all-sizes cell code on the plain size tables: a loop size that does not exist on a
diagonal is not tested for, it reads ring rows that no diagonal of the fold has written yet and finds the "none" the fold's
prologue put there.  The emulation build keeps a shadow byte per int16 entry of everything that prologue initialises (0 = by
this fold's prologue, 1 = written by a diagonal of this fold, 2 = left over from the fold before) and aborts on any read for an
absent size, by a valid lane, that leaves that span or finds a shadow other than 0 (sf_emul_check_absent).  Every fold below
runs under that check; the emulated device has few workgroups, so all but a handful of a width's folds run one after the
other in the same workgroup, after the poly-GC rows.  GPU twin: tests/test_gpu_unguarded_sizes.py."""
import subprocess
import sys

import numpy as np
import pytest

from scanfold_amd import params
import unguarded_sizes_util as uu


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


_REF = {}


def reference(orc, W):
    """(rows, [(structure, energy)]) of a width, computed once"""
    if W not in _REF:
        arr = uu.cpu_rows(W)
        _REF[W] = (arr, [orc.mfe(bytes(r).decode()) for r in arr])
    return _REF[W]


@pytest.mark.parametrize("W", uu.WIDTHS)
def test_energies_and_structures_under_the_shadow_check(emul, orc, W):
    arr, ref = reference(orc, W)
    assert len(arr) == 48
    emul.set_kernel_mode(0)
    assert emul.mfe_batch(arr).tolist() == [e for _, e in ref], W
    e, db = emul.mfe_trace_batch(arr)
    assert [(db[k], int(e[k])) for k in range(len(arr))] == ref, W


@pytest.mark.parametrize("W", uu.POISON_WIDTHS)
@pytest.mark.parametrize("pattern", ("1", "2", "3", "4", "5"))
def test_poison_patterns_move_nothing(emul, orc, monkeypatch, W, pattern):
    arr, ref = reference(orc, W)
    monkeypatch.setenv("SCANFOLD_MFE_POISON", pattern)
    assert emul.mfe_batch(arr).tolist() == [e for _, e in ref], (W, pattern)
    e, db = emul.mfe_trace_batch(arr[:8])
    assert [(db[k], int(e[k])) for k in range(8)] == ref[:8], (W, pattern)


@pytest.mark.parametrize("W", (36, 120))
def test_constrained_and_shape_rows(emul, orc, W):
    """the constrained instantiations keep the guarded steps: one constraint row and one row of Deigan pseudo-energies per width"""
    from test_constraints import canonical_constraint
    rng = np.random.default_rng(9000 + W)
    seq = bytes(uu.cpu_rows(W)[5]).decode()
    cons = canonical_constraint(rng, seq)
    sc = rng.integers(-60, 40, (1, W)).astype(np.int32)
    try:
        r = emul.fold_constrained([seq], [cons], pf=False)
        orc.set_constraint(cons, None)
        assert (r["structure"][0], int(r["mfe"][0])) == orc.mfe(seq), (W, cons)
        r = emul.fold_constrained([seq], None, sc, pf=False)
        orc.set_constraint(None, sc[0])
        assert (r["structure"][0], int(r["mfe"][0])) == orc.mfe(seq), W
    finally:
        orc.set_constraint(None, None)


@pytest.mark.parametrize("what,message", [(0, "finds an entry a diagonal of this fold has written"),
                                          (1, "outside the rolling tables and their mirror rows")])
def test_the_shadow_check_can_fire(emul, what, message):
    """the checker called directly, in a child process: a read marked "size absent" aimed at an entry marked written, and one aimed
    past the mirror row (W = 120: into the parameter tables) — each aborts with its message"""
    from emul_engine import EMUL_LIB
    code = "import ctypes; ctypes.CDLL(%r).sfemul_absent_check_selftest(120, %d)" % (EMUL_LIB, what)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60)
    assert p.returncode == -6, (p.returncode, p.stderr[-500:])
    assert "sf_mfe_fast (emulation): read for loop size" in p.stderr and message in p.stderr, p.stderr[-500:]
