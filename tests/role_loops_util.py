"""Shared by tests/test_role_loops_emul.py and tests/test_gpu_role_loops.py: the rows, the widths and the host-side check of
the cell lists for the narrow MFE kernel's split steps (sf_mfe_fast.hip.h: one loop per role of a wave, SfRole)."""
import numpy as np

from scanfold_amd import _lib

# Where a role boundary moves: 64 / 65 the first narrow widths with a split phase (a handful of steps); 100 the merged helper
# with all three chunk-width loops; 117 / 118 either side of SF_HELP_MERGE_MAXW (the instantiation changes); 120 its own
# instantiation (merged helper, lists in the size-table area); 128 the last narrow width.
WIDTHS = (64, 65, 100, 117, 118, 120, 128)
# widths whose instantiation has the merged helper (one list of the pairable cells of d0 and d0 + 1 per step) AND whose first split
# diagonals hold more than 64 cells together: at W = 64 / 65 a split step has at most 28 + 27 cells, 118 and 128 keep no list
LIST_WIDTHS = (100, 117, 120)
SFD_MAXLOOP = 30
PAIRS = {(b"G"[0], b"C"[0]), (b"C"[0], b"G"[0]), (b"G"[0], b"U"[0]), (b"U"[0], b"G"[0]), (b"A"[0], b"U"[0]), (b"U"[0], b"A"[0])}


def split_d0(W):
    """first even diagonal of the split phase of the narrow kernel (NG = 128, centre lane 32), as the kernel derives it"""
    assert 64 <= W <= 128
    offs = ((W + 1) >> 1) - 32
    return (max(SFD_MAXLOOP + 6, 2 * (offs - 1), 2 * (W - offs - 63)) + 1) & ~1


def random_rows(W, n, seed):
    return np.frombuffer(b"ACGU", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, (n, W))]


def gc_rows(W, n, seed):
    """85 % G + C: four of ten cells can pair, so the list of a step's pairable cells passes 64 entries now and then"""
    return np.random.default_rng(seed).choice(np.frombuffer(b"GCAU", dtype=np.uint8), size=(n, W), p=(0.425, 0.425, 0.075, 0.075))


def longest_list(arr):
    """per row: the most pairable cells (i, i + d) on two adjacent diagonals d0, d0 + 1 of a split step — the entries of the
    merged helper's list in that step (entries 64 and up are the sweeper wave's)"""
    n, W = arr.shape
    can = np.zeros((256, 256), dtype=bool)
    for a, b in PAIRS:
        can[a, b] = True
    best = np.zeros(n, dtype=np.int64)
    for d0 in range(split_d0(W), W, 2):
        cnt = can[arr[:, :W - d0], arr[:, d0:]].sum(axis=1)
        if d0 + 1 < W:
            cnt = cnt + can[arr[:, :W - d0 - 1], arr[:, d0 + 1:]].sum(axis=1)
        best = np.maximum(best, cnt)
    return best


def scan_rows(eng, W, n_win, seed, r=6):
    """n_win windows of a random record, side by side, each with r dinucleotide shuffles: the scan traces every (r + 1)-th row
    (a native fold with the sweep at its end) among folds with the trailing sweep -> (record, rows as the device made them)"""
    rng = np.random.default_rng(seed)
    tr = "".join("ACGU"[k] for k in rng.integers(0, 4, W * n_win))
    rows = np.frombuffer(b"NACGU", dtype=np.uint8)[eng.shuffle_windows(tr, W, W, 0, n_win, r, _lib.SHUFFLE_DI, seed)]
    return tr, rows


def check_traced(eng, orc, W, n_win, seed, r=6):
    tr, rows = scan_rows(eng, W, n_win, seed, r)
    res = eng.scan(tr, W, W, 0, n_win, r, _lib.SHUFFLE_DI, seed, flags=_lib.SCAN_NO_PF)
    ref = orc.mfe_batch(rows)
    assert (res["energies"].reshape(-1) == ref).all(), W
    for w in range(n_win):
        assert (res["structure"][w], int(res["energies"][w, 0])) == orc.mfe(tr[w * W:(w + 1) * W]), (W, w)


def check_constrained(eng, orc, W, n, seed):
    """one constraint row per fold (the HC instantiation) against the oracle's constrained fold"""
    from test_constraints import canonical_constraint
    rng = np.random.default_rng(seed)
    seqs = [bytes(a).decode() for a in random_rows(W, n, seed)]
    cons = [canonical_constraint(rng, s) for s in seqs]
    r = eng.fold_constrained(seqs, cons, pf=False)
    try:
        for k in range(n):
            orc.set_constraint(cons[k], None)
            assert (r["structure"][k], int(r["mfe"][k])) == orc.mfe(seqs[k]), (W, k)
    finally:
        orc.set_constraint(None, None)
