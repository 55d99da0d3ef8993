"""Shared by tests/test_helper_terms_emul.py and tests/test_gpu_helper_terms.py: the rows, the widths and the arithmetic of the
crossing area for the narrow MFE kernel's split steps with the publish terms looked up by the helper waves and the fML bases
carried from step to step (sf_mfe_fast.hip.h: SF_FAST_HELPER_TERMS, SF_FAST_FBASE_CARRY)."""
import numpy as np

import role_loops_util as ru

# 64 / 65 the first widths with split steps, even and odd (the carried base's parity term); 100 / 117 the merged generic
# instantiation; 118 / 128 the mirroring helper; 120 its own instantiation.
# Which path a width runs: the carried fML bases at every one of them.  The helper's terms only where a merged-helper
# instantiation has steps in its loop with 32-lane chunks, split_d0 <= d0 < W - 30 (TERMS_WIDTHS): 100 (d0 = 38 .. 68), 117
# (56 .. 86), 120 (58 .. 88).  At 64 / 65 the split phase starts at d0 = 36, past W - 30, and 118 / 128 keep the terms on the main
# waves (the mirroring helper measured slower with them): those widths hold the parent's term path next to the carried bases.
WIDTHS = (64, 65, 100, 117, 118, 120, 128)
TERMS_WIDTHS = (100, 117, 120)
POISON_WIDTHS = (64, 100, 120)


def runs_helper_terms(W):
    """the width's instantiation has the merged helper (SF_HELP_MERGE_MAXW = 118, and W = 120) and split steps before d0 = W - 30"""
    merged = W < 118 or W == 120
    return merged and ru.split_d0(W) < W - 30
_NT = np.frombuffer(b"ACGU", dtype=np.uint8)


def rows(W, n_uniform, n_gc, n_with_n, seed):
    """uniform rows, GC-rich rows (the merged helper's list passes 64 entries: wave 3 hands terms over too), rows in which one
    nucleotide in ten is N (the mismatch and dangle terms of a pair next to an N), the last of them all N"""
    rng = np.random.default_rng(seed)
    uni = _NT[rng.integers(0, 4, (n_uniform, W))]
    rich = ru.gc_rows(W, n_gc, seed + 1)
    withn = rng.choice(np.frombuffer(b"NACGU", dtype=np.uint8), size=(n_with_n, W), p=(0.1, 0.225, 0.225, 0.225, 0.225))
    withn[-1, :] = b"N"[0]
    return np.ascontiguousarray(np.concatenate([uni, rich, withn]))


def crossing_area_fits(W):
    """On every split diagonal d (n = W - d cells) the helper's exterior term of the cell at column x goes to int16 entry 2 n + x of
    the diagonal's row of the interleaved bulge / 1xn table, behind the n words of the cells: the row has W - 4 words."""
    return all(3 * (W - d) <= 2 * (W - 4) for d in range(ru.split_d0(W), W))


def ends_pair_rows(W, n, seed):
    """rows whose first and last nucleotides pair with many partners: cells in row 1 and in column W (the dangle branches of the
    stem and exterior terms) that do pair"""
    arr = _NT[np.random.default_rng(seed).integers(0, 4, (n, W))].copy()
    arr[:, 0] = b"G"[0]
    arr[:, -1] = b"C"[0]
    arr[: n // 2, 1] = b"G"[0]
    arr[: n // 2, -2] = b"U"[0]
    return arr
