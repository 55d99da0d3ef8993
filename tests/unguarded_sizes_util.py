"""Shared by tests/test_unguarded_sizes.py and tests/test_gpu_unguarded_sizes.py: the widths and the rows for the narrow MFE
kernel's short diagonals (sf_mfe_fast.hip.h, SF_STEP_SHORT_A / B / C: the all-sizes code without guards from d0 = 10 on)."""
import numpy as np

# 16 the smallest supported width; 17 odd (fML padding parity); 21 a mid-range small width; 35 / 36 / 37 either side of the ring
# size and of the old guarded / unsplit boundary; 40 a full ring; 64 the first width with split steps; 117 / 118 the merged-helper
# switch; 120 its own instantiation, the parameter tables directly behind the mirror row; 128 the largest narrow width
WIDTHS = (16, 17, 21, 35, 36, 37, 40, 64, 117, 118, 120, 128)
POISON_WIDTHS = (36, 64, 120)
_NT = np.frombuffer(b"ACGU", dtype=np.uint8)


def poly_gc(W, loop):
    """a G...C hairpin over the whole width: past 120 kcal/mol — out of the int16 range — at the large widths"""
    h = (W - loop) // 2
    return np.frombuffer(b"G" * h + b"A" * (W - 2 * h) + b"C" * h, dtype=np.uint8)


def mixed_rows(W, n_gc, n_uniform, n_rich, n_all_n, seed):
    """poly-GC hairpins FIRST (every later fold of a workgroup that took one follows it), then uniform rows, rows with
    P(G) = P(C) = 0.4, rows of all N"""
    rng = np.random.default_rng(seed)
    gc = np.stack([poly_gc(W, 4 + (t & 1)) for t in range(n_gc)])
    uni = _NT[rng.integers(0, 4, (n_uniform, W))]
    rich = rng.choice(np.frombuffer(b"GCAU", dtype=np.uint8), size=(n_rich, W), p=(0.4, 0.4, 0.1, 0.1))
    alln = np.full((n_all_n, W), b"N"[0], dtype=np.uint8)
    return np.ascontiguousarray(np.concatenate([gc, uni, rich, alln]))


def cpu_rows(W):
    return mixed_rows(W, 2, 32, 12, 2, 7000 + W)  # 48


def gpu_rows(W):
    # 4 096: poly-GC at 0 .. 7, the other 4 088 in the CPU test's mix 32 : 12 : 2 (88 of each part; the 40 left over are uniform)
    return mixed_rows(W, 8, 32 * 88 + 40, 12 * 88, 2 * 88, 8000 + W)
