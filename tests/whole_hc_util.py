"""The constraint of a whole record on its way to the device, through all eight entry points that take one (fold_long,
fold_long_batch, fold_banded, fold_banded_batch, pf_long, pf_long_batch, pf_banded, pf_banded_probs): the host parses every
constrained row of a chunk into one staging block (hc_parse_host / bind_rows in scanfold_hip.hip, int16 positions in full
tables and int32 in banded ones) and copies it up in one allocation.  Shared by tests/test_whole_constraints.py (the CPU
emulation) and tests/test_gpu_whole_constraints.py (the MI355X).

Records of 57, 90 and 120 nt and span 30 for the banded calls: the smallest shapes at which a row's L + 2 entries, the
offsets between rows and the offsets between chunks can go wrong.  The random bases leave some bracket pairs
non-complementary (type 7), which is intended.  The oracle's answers are computed once a process and shared."""
import numpy as np
import pytest

from scanfold_amd import _lib
from long_pf_util import KEYS, assert_close, oracle_pf
from long_util import rand_seq, with_oracle_constraint
from test_banded_fold import banded_bytes
from test_long_batch import seq_bytes
from test_long_pf_batch import pf_bytes

LENS = (57, 90, 120)
SPAN = 30
WIDTH = 28  # of the outer bracket pairs under SPAN: j - i + 1 <= SPAN, so the oracle's answer is feasible
PF_KEYS = KEYS + ("centroid",)


def record(L, seed=0):
    return rand_seq(np.random.default_rng(1000 * seed + L), L)


def edge_constraint(L, width=None):
    """One string that touches every edge of the parsed arrays.  width None (full tables): '(' at position 1 and ')' at L.
    Under a span: '(' at 1 closing at `width`, and a pair of the same width closing at L.  In both: 'x' at 2 and at L - 1; inside
    the pair that opens at 1 a second pair nested directly, a third beside it, and '<', '|', '>' inside the second."""
    w = width or L
    assert w >= 20 and (width is None or 2 * w <= L)
    c = ["."] * L
    m = 3 + (w - 6) // 2
    for pos, ch in ((1, "("), (w, ")"), (2, "x"), (3, "("), (m, ")"), (m + 2, "("), (w - 2, ")"), (5, "<"), (7, "|"), (m - 2, ">"),
                    (L - 1, "x")):
        assert c[pos - 1] == ".", (L, width, pos)
        c[pos - 1] = ch
    if width:
        assert c[L - w] == "."
        c[L - w], c[L - 1] = "(", ")"
    return "".join(c)


CONS = {L: edge_constraint(L) for L in LENS}              # full tables
CONS_SPAN = {L: edge_constraint(L, WIDTH) for L in LENS}  # banded tables under SPAN

_refs = {}


def reference(oracle, L, span):
    """-> (mfe (energy, structure), pf dict with bpp) of record(L) under its edge constraint from the oracle, span 0 or SPAN"""
    if (L, span) not in _refs:
        s, c = record(L), (CONS_SPAN if span else CONS)[L]
        oracle.set_max_bp_span(span)
        try:
            db, e = with_oracle_constraint(oracle, c, lambda: oracle.mfe(s))
            pf = oracle_pf(oracle, s, c, want_bpp=True)
        finally:
            oracle.set_max_bp_span(0)
        assert abs(e) < 10 ** 6 and np.isfinite(pf["dG"]), (L, span, e, pf["dG"])  # feasible: a finite energy
        _refs[(L, span)] = ((e, db), pf)
    return _refs[(L, span)]


def under_span(engine, span, fn):
    engine.set_max_bp_span(span)
    try:
        return fn()
    finally:
        engine.set_max_bp_span(0)


def check_the_strings():
    for L in LENS:
        for c, w in ((CONS[L], L), (CONS_SPAN[L], WIDTH)):
            assert len(c) == L and c[0] == "(" and c[-1] == ")" and c[1] == "x" and c[-2] == "x", c
            assert set("()x<>|.") == set(c) and c.count("(") == c.count(")") == (3 if w == L else 4), c
            assert c[w - 1] == ")" and c[2] == "(" and c[w - 3] == ")", c


def check_edges_of_one_constraint(engine, oracle):
    """each entry point on each record under its edge constraint against the oracle: MFE == on energy and structure, the
    partition function within long_pf_util.assert_close's bars with equal centroids"""
    seqs = [record(L) for L in LENS]
    # full tables
    cons = [CONS[L] for L in LENS]
    be, bdb = engine.fold_long_batch(seqs, cons, structure=True)
    brows = engine.pf_long_batch(seqs, cons)
    for k, L in enumerate(LENS):
        mfe, pf = reference(oracle, L, 0)
        assert engine.fold_long(seqs[k], cons[k]) == mfe, L
        assert (int(be[k]), bdb[k]) == mfe, L
        assert_close(engine.pf_long(seqs[k], cons[k]), pf, "pf_long %d" % L, pf["bpp"])
        assert_close(brows[k], pf, "pf_long_batch %d" % L, pf["bpp"])
    # banded tables under SPAN

    def banded():
        cons = [CONS_SPAN[L] for L in LENS]
        be, bdb = engine.fold_banded_batch(seqs, cons, structure=True)
        for k, L in enumerate(LENS):
            mfe, pf = reference(oracle, L, SPAN)
            assert engine.fold_banded(seqs[k], cons[k]) == mfe, L
            assert (int(be[k]), bdb[k]) == mfe, L
            assert_close(engine.pf_banded(seqs[k], cons[k]), pf, "pf_banded %d" % L, pf["bpp"])
            assert_close(engine.pf_banded_probs(seqs[k], cons[k]), pf, "pf_banded_probs %d" % L, pf["bpp"])
    under_span(engine, SPAN, banded)


def packed_rows(width=None):
    """-> (sequences, constraints) of the five rows: constraint A on 120 nt, none, all dots on 90 nt, B on 57 nt, A on 120 nt"""
    lens = (120, 57, 90, 57, 120)
    seqs = [record(L, seed=k + 1) for k, L in enumerate(lens)]
    a, b = edge_constraint(120, width), edge_constraint(57, width)
    return seqs, [a, None, "." * 90, b, a]


def check_packing_across_rows_and_chunks(engine):
    """every row of a batch == the single call of that row, in the given order and reversed, in one chunk and under a byte
    budget of two and a half times the largest row's, which cuts the call into chunks with constrained rows past the first"""
    def mfe_rows(batch, seqs, cons):
        e, db = batch(seqs, cons, structure=True)
        return [(int(e[k]), db[k]) for k in range(len(seqs))]

    def pf_rows(seqs, cons):
        return [{key: row[key] for key in PF_KEYS} for row in engine.pf_long_batch(seqs, cons)]

    def run(rows, single, times, row_bytes, seqs, cons):
        want = [single(s, c) for s, c in zip(seqs, cons)]
        for order in (slice(None), slice(None, None, -1)):
            s, c, w = seqs[order], cons[order], want[order]
            assert rows(s, c) == w
            assert times()["chunks"] == 1
            budget = 5 * max(row_bytes(len(x)) for x in s) // 2
            first, total = 0, 0  # the rows of the first chunk: consecutive rows while they fit, always at least one
            while first < len(s) and (first == 0 or total + row_bytes(len(s[first])) <= budget):
                total += row_bytes(len(s[first]))
                first += 1
            assert any(x and set(x) != {"."} for x in c[first:])  # a constrained row in a chunk that starts at s0 > 0
            try:
                engine.set_long_batch_bytes(budget)
                assert rows(s, c) == w
                assert times()["chunks"] >= 2
            finally:
                engine.set_long_batch_bytes(0)

    seqs, cons = packed_rows()
    run(lambda s, c: mfe_rows(engine.fold_long_batch, s, c), engine.fold_long, engine.fold_long_batch_times, seq_bytes, seqs, cons)
    run(pf_rows, engine.pf_long, engine.pf_long_batch_times, pf_bytes, seqs, cons)
    seqs, cons = packed_rows(WIDTH)
    under_span(engine, SPAN, lambda: run(lambda s, c: mfe_rows(engine.fold_banded_batch, s, c), engine.fold_banded,
                                         engine.fold_banded_batch_times, lambda L: banded_bytes(L, SPAN), seqs, cons))


def the_eight(engine, s, c, batch_of=lambda s, c: ([s], [c])):
    """-> [(name, call)]: the eight entry points on record s under constraint c; the batched ones on batch_of(s, c)"""
    rows, cons = batch_of(s, c)
    return [("fold_long", lambda: engine.fold_long(s, c)),
            ("fold_long_batch", lambda: engine.fold_long_batch(rows, cons, structure=True)),
            ("fold_banded", lambda: engine.fold_banded(s, c)),
            ("fold_banded_batch", lambda: engine.fold_banded_batch(rows, cons, structure=True)),
            ("pf_long", lambda: engine.pf_long(s, c)),
            ("pf_long_batch", lambda: engine.pf_long_batch(rows, cons)),
            ("pf_banded", lambda: engine.pf_banded(s, c)),
            ("pf_banded_probs", lambda: engine.pf_banded_probs(s, c))]


def check_refusals(engine, launched=None):
    """an unbalanced row raises in each of the eight calls, in a batch as the last of three rows; launched(call) -> the kernels
    call() launched (the emulation's log): none"""
    L = 57
    s = record(L)

    def last_of_three(s, c):
        return [record(120), record(90), s], [CONS_SPAN[120], None, c]

    def refused():
        for bad in ("(" + "." * (L - 1), ")" + "." * (L - 1)):
            for name, call in the_eight(engine, s, bad, last_of_three):
                def raises():
                    with pytest.raises(_lib.ScanFoldHipError):
                        call()
                log = launched(raises) if launched else raises()
                assert not log, (name, bad[0], log)
    under_span(engine, SPAN, refused)


def check_a_constraint_of_dots_is_no_constraint(engine):
    """a constraint of dots gives the bytes (and the bits) of no constraint at all in all eight calls"""
    def plain(v):
        if isinstance(v, dict):
            return {k: plain(x) for k, x in v.items()}
        if isinstance(v, (tuple, list)):
            return [plain(x) for x in v]
        return v.tolist() if isinstance(v, np.ndarray) else v

    def same():
        for L in LENS:
            s = record(L)
            for (name, dots), (_, none) in zip(the_eight(engine, s, "." * L), the_eight(engine, s, None)):
                assert plain(dots()) == plain(none()), (name, L)
    under_span(engine, SPAN, same)
