"""Checks of the maximum-expected-accuracy (MEA) structure of a pair list (sf_mea_pairs, sf_pf_banded_mea,
include/scanfold_hip_long.h), shared by tests/test_pf_mea.py (the kernel source compiled for the CPU) and
tests/test_gpu_pf_mea.py (the MI355X).

The reference, mea_reference, restates the header's model in Python floats (IEEE doubles; neither CPython nor numpy
contracts a product into a sum): the same expressions associated the same way, the same tie rule.  It is itself checked,
with no engine involved, against the enumeration of every nested structure (check_reference_against_enumeration) on dense
lists of dyadic values, where every sum is exact and the optimum's score must be equal.  Structure and the score's bytes of
the engine are asserted `==` against it on the same list.

Against the oracle's probabilities (check_live_edge, d) the bar follows from the project's PF_TOL: every listed p and every
u is within PF_TOL of the oracle's and a structure has at most L terms, each weighted by 1 (unpaired) or 2 gamma (a pair),
so two scores of one structure differ by at most PF_TOL L max(1, 2 gamma), and the optimum under one set of numbers lies
within twice that of the optimum under the other."""
import ctypes
import os

import numpy as np
import pytest

from scanfold_amd import _lib
from scanfold_amd import scanfold as sfd
from scanfold_amd import whole
from long_pf_util import oracle_pf
from long_util import hairpin_rich, pair_table, rand_seq
from test_banded_fold import marked_record, model
from test_gpu_parity import PF_TOL
import banded_pf_util as bp
import pf_probs_util as pp

GAMMAS = (0.5, 1.0, 4.0)
SHARED = ("dG", "mean_bp_dist", "centroid_dist", "centroid")


# ---- the reference ----

def mea_reference(L, pairs, unpaired, gamma):
    """-> (dot-bracket, score): the header's recurrences and traceback, in Python floats"""
    u = [float(x) for x in unpaired]
    g2 = 2.0 * float(gamma)
    rows = [[] for _ in range(L + 2)]  # rows[i]: (k, w_ik), ascending in k
    B = 1
    for i, j, p in (pairs.tolist() if isinstance(pairs, np.ndarray) else pairs):
        rows[i].append((j, g2 * float(p)))
        B = max(B, 1 + j - i)
    M = [[0.0] * (L + 2) for _ in range(B)]  # M[d][i] = M[i][i + d]

    def m(i, j):
        return 0.0 if j < i else M[j - i][i]

    for d in range(B):
        Md = M[d]
        for i in range(1, L - d + 1):
            j = i + d
            best = u[i - 1] + m(i + 1, j)
            for k, w in rows[i]:
                if k > j:
                    break
                c = (w + m(i + 1, k - 1)) + m(k + 1, j)
                if c > best:
                    best = c
            Md[i] = best
    E = [0.0] * (L + 2)
    for i in range(L, 0, -1):
        best = u[i - 1] + E[i + 1]
        for k, w in rows[i]:
            c = (w + m(i + 1, k - 1)) + E[k + 1]
            if c > best:
                best = c
        E[i] = best
    db = ["."] * L
    stack = [(1, 0)]  # (i, j); j = 0: the suffix from i
    while stack:
        i, j = stack.pop()
        hi = j if j else L
        value = (lambda x: m(x, j)) if j else (lambda x: E[x])
        while i <= hi:
            v = value(i)
            if v == u[i - 1] + value(i + 1):
                i += 1
                continue
            for k, w in rows[i]:
                if k <= hi and (w + m(i + 1, k - 1)) + value(k + 1) == v:
                    break
            else:
                raise AssertionError("the reference's traceback found no candidate at %d" % i)
            db[i - 1], db[k - 1] = "(", ")"
            if k - 1 >= i + 1:
                stack.append((i + 1, k - 1))
            i = k + 1
    return "".join(db), E[1]


def score_under(db, P, unpaired, gamma):
    """the score of the structure db under the upper-triangular matrix P and the unpaired vector, summed in long double"""
    pt = pair_table(db)
    s = np.longdouble(0)
    for k, ch in enumerate(db):
        if ch == ".":
            s += np.longdouble(unpaired[k])
    for a, b in pt.items():
        if a < b:
            s += np.longdouble(2.0 * gamma) * np.longdouble(P[a, b])
    return float(s)


def as_list(rows):
    """[(i, j, p)] in any order -> PAIR_PROB_DTYPE, ascending in (i, j)"""
    out = np.zeros(len(rows), dtype=_lib.PAIR_PROB_DTYPE)
    for t, (i, j, p) in enumerate(sorted(rows)):
        out[t] = (i, j, p)
    return out


def list_of(P, cutoff):
    """the pairs of the upper-triangular matrix P (0-based) with p >= cutoff as a 1-based list"""
    ij = np.argwhere(P >= cutoff)
    return as_list([(int(a) + 1, int(b) + 1, float(P[a, b])) for a, b in ij])


def all_structures(i, j, rows):
    """every nested set of listed pairs on [i, j], each position with at most one partner"""
    if i > j:
        yield []
        return
    yield from all_structures(i + 1, j, rows)
    for k in rows.get(i, ()):
        if k <= j:
            for a in all_structures(i + 1, k - 1, rows):
                for b in all_structures(k + 1, j, rows):
                    yield [(i, k)] + a + b


def check_reference_against_enumeration():
    """dense random lists at L <= 10, every value a multiple of 1/64: all sums are exact, so the reference's score equals
    the best enumerated score, and its structure is a listed, nested one that attains it"""
    n_structures = 0
    for L in range(1, 11):
        for seed in range(6):
            rng = np.random.default_rng(64 * L + seed)
            keep = rng.random((L + 1, L + 1)) < (0.9 if seed % 2 else 0.5)
            rows = [(i, j, int(rng.integers(0, 65)) / 64.0) for i in range(1, L + 1) for j in range(i + 1, L + 1) if keep[i, j]]
            u = rng.integers(0, 65, L) / 64.0
            pairs = as_list(rows)
            by_row = {}
            for i, j, _ in sorted(rows):
                by_row.setdefault(i, []).append(j)
            p_of = {(i, j): p for i, j, p in rows}
            for gamma in GAMMAS:
                best = -1.0
                for s in all_structures(1, L, by_row):
                    n_structures += 1
                    paired = {x for ij in s for x in ij}
                    assert len(paired) == 2 * len(s)
                    sc = sum(u[k - 1] for k in range(1, L + 1) if k not in paired) + sum(2.0 * gamma * p_of[ij] for ij in s)
                    best = max(best, sc)
                db, score = mea_reference(L, pairs, u, gamma)
                assert score == best, (L, seed, gamma, score, best)
                got = sorted((a + 1, b + 1) for a, b in pair_table(db).items() if a < b)
                assert all(ij in p_of for ij in got)
                assert sum(u[k] for k in range(L) if db[k] == ".") + sum(2.0 * gamma * p_of[ij] for ij in got) == best
    print("%d structures enumerated" % n_structures)
    assert n_structures > 10000  # (the enumeration is not a trivial one)


# ---- sf_mea_pairs on synthetic lists ----

def random_list(rng, L, band, per_row=3):
    """up to per_row partners a position within the band, one pair on the band's last diagonal; -> (pairs, unpaired)"""
    rows = {}
    for i in range(1, L):
        hi = min(L, i + band - 1)
        for j in rng.integers(i + 1, hi + 1, int(rng.integers(0, per_row + 1))):
            rows[i, int(j)] = float(rng.random())
    a = int(rng.integers(1, L - band + 2))
    rows[a, a + band - 1] = 0.9
    pairs = as_list([(i, j, p) for (i, j), p in rows.items()])
    assert int((pairs["j"] - pairs["i"]).max()) == band - 1
    return pairs, rng.random(L)


def same(engine, L, pairs, unp, gamma, what=""):
    """engine.mea_pairs == the reference: the structure and the bytes of the score; -> (structure, score)"""
    db, score = engine.mea_pairs(L, pairs, unp, gamma)
    rdb, rscore = mea_reference(L, pairs, unp, gamma)
    t = engine.mea_times()
    B = 1 + int((pairs["j"] - pairs["i"]).max()) if len(pairs) else 1
    print("%s L=%d n=%d gamma=%g: %d pairs, score %.17g; %s" % (what, L, len(pairs), gamma, db.count("("), score, t))
    assert db == rdb, (what, gamma)
    assert np.float64(score).tobytes() == np.float64(rscore).tobytes(), (what, gamma, score, rscore)
    assert t["band"] == B and t["fill_launches"] == B
    assert t["extra_bytes"] == mea_pairs_bytes(L, B, len(pairs))
    return db, score


def mea_bytes(L, n):
    """SF_MEA_BYTES of include/scanfold_hip_long.h"""
    return 8 * n + 9 * L + 8 * (L // 2) + 33


def mea_pairs_bytes(L, B, n):
    """SF_MEA_PAIRS_BYTES"""
    return 8 * L * B + 16 * n + 16 * L + mea_bytes(L, n)


def check_empty_and_tiny(engine):
    none = np.zeros(0, dtype=_lib.PAIR_PROB_DTYPE)
    for L in (1, 2, 5):
        u = np.random.default_rng(L).random(L)
        db, score = same(engine, L, none, u, 1.0, "empty")
        assert db == "." * L
    # B = 2: only (i, i + 1) pairs
    L = 70
    rng = np.random.default_rng(2)
    pairs = as_list([(i, i + 1, float(rng.random())) for i in range(1, L) if rng.random() < 0.7])
    for gamma in GAMMAS:
        db, _ = same(engine, L, pairs, rng.random(L), gamma, "B=2")
    assert "()" in db
    # B = L
    for L in (2, 66):
        rng = np.random.default_rng(L)
        pairs, u = random_list(rng, L, L)
        for gamma in GAMMAS:
            same(engine, L, pairs, u, gamma, "B=L")


def check_random_band(engine, band, L=433):
    rng = np.random.default_rng(band)
    pairs, u = random_list(rng, L, band)
    n_pairs = []
    for gamma in GAMMAS:
        db, _ = same(engine, L, pairs, u, gamma, "band %d" % band)
        n_pairs.append(db.count("("))
    assert 10 < n_pairs[0] < n_pairs[2]  # gamma is a real knob
    a = engine.mea_pairs(L, pairs, u, 1.0)
    b = engine.mea_pairs(L, pairs, u, 1.0)
    assert a[0] == b[0] and np.float64(a[1]).tobytes() == np.float64(b[1]).tobytes()


def check_many_partners(engine, n, L=433):
    """position 7 has n listed partners, the others a few; its last partner is the likely one, nothing listed crosses that
    pair or shares its end, and both ends are unlikely to be unpaired: at every gamma the pair is in the structure, so the
    partner loops of fill, exterior pass and traceback all reach record n of the row"""
    rng = np.random.default_rng(n)
    pairs, u = random_list(rng, L, 40)
    last = 8 + n - 1
    rows = {(int(i), int(j)): float(p) for i, j, p in pairs.tolist() if i > 7 and j != last and not i <= last < j}
    for j in range(8, last):
        rows[7, j] = float(rng.random()) * 0.01
    rows[7, last] = 0.95
    u[6] = u[last - 1] = 0.1
    pairs = as_list([(i, j, p) for (i, j), p in rows.items()])
    assert int((pairs["i"] == 7).sum()) == n and len(pairs) > n + L // 2
    for gamma in GAMMAS:
        db, _ = same(engine, L, pairs, u, gamma, "%d partners" % n)
        assert pair_table(db).get(6) == last - 1  # (0-based)


def check_near_partners(engine, L=200):
    """The exterior pass works on chunks of 64 positions from the record's end (at L = 200: 137..200, 73..136, 9..72, 1..8)
    and keeps a position's first four partners inside its chunk in registers; the rest it reads on the position's turn.
    Position 20 has ten partners, 22, 24 .. 40, all inside its chunk, and the likely one is the seventh (34); nothing else
    listed touches 20..40, so the pair is an exterior one at every gamma and only the loop past the fourth finds it.  At
    L = 167 the chunks are 104..167, 40..103, 1..39: the first four partners of 20 are near, the likely one too, and the
    last (40) lies beyond the chunk."""
    rng = np.random.default_rng(L)
    pairs, u = random_list(rng, L, 30)
    rows = {(int(i), int(j)): float(p) for i, j, p in pairs.tolist() if j < 20 or i > 40}
    for k in range(22, 41, 2):
        rows[20, k] = 0.01
    rows[20, 34] = 0.95
    u[19] = u[33] = 0.05
    pairs = as_list([(i, j, p) for (i, j), p in rows.items()])
    assert [int(j) for j in pairs["j"][pairs["i"] == 20]].index(34) == 6
    for gamma in GAMMAS:
        db, _ = same(engine, L, pairs, u, gamma, "near partners")
        assert pair_table(db).get(19) == 33  # (0-based)


def check_all_ties(engine, L=65):
    """every p = 0.25, every u = 0.5, gamma = 1: every weight is 0.5 and a pair scores what one of its ends scores unpaired,
    so every structure without a pair is optimal, and the tie rule takes the first candidate: all dots"""
    pairs = as_list([(i, j, 0.25) for i in range(1, L + 1) for j in range(i + 1, L + 1)])
    u = np.full(L, 0.5)
    db, score = same(engine, L, pairs, u, 1.0, "all ties")
    assert db == "." * L and score == 0.5 * L
    # and with weights 1.0 (gamma = 2) a pair ties with its two ends unpaired: still the first candidate
    db, score = same(engine, L, pairs, u, 2.0, "all ties, gamma 2")
    assert db == "." * L and score == 0.5 * L
    # u = 0.125: a pair (0.5) beats its two ends unpaired (0.25), so 32 pairs and one unpaired position are optimal.  The
    # suffix from 1 ties with "1 unpaired, then 32 pairs": the first candidate; from 2 on every position pairs, and among
    # its partners (all tie that leave an even stretch) the smallest k wins: the neighbour.
    db, score = same(engine, L, pairs, np.full(L, 0.125), 1.0, "ties among partners")
    assert db == "." + "()" * (L // 2) and score == 0.5 * (L // 2) + 0.125


# ---- sf_pf_banded_mea ----

def check_call(engine, s, cons=None, hint=None, cutoff=0.01, gamma=1.0, what="", probs=None):
    """(a) and (b): pf_banded_mea == the reference on its own list; its shared outputs == pf_banded_probs's; mea_pairs on
    them gives the same; -> the dict.  probs: pf_banded_probs of the same arguments where the caller has it already (with
    pf_banded_times and pf_banded_probs_times after it), else it is run here."""
    got = engine.pf_banded_mea(s, cons, mfe_hint=hint, cutoff=cutoff, gamma=gamma)
    L = len(s)
    t = engine.mea_times()
    rdb, rscore = mea_reference(L, got["pairs"], got["unpaired"], gamma)
    print("%s gamma=%g: MEA %d pairs, centroid %d, score %.17g; %s" % (what, gamma, got["mea"].count("("),
                                                                     got["centroid"].count("("), got["mea_score"], t))
    assert got["mea"] == rdb, what
    assert np.float64(got["mea_score"]).tobytes() == np.float64(rscore).tobytes(), (what, got["mea_score"], rscore)
    assert t["extra_bytes"] == mea_bytes(L, len(got["pairs"]))
    B = 1 + int((got["pairs"]["j"] - got["pairs"]["i"]).max()) if len(got["pairs"]) else 1
    assert t["band"] == B == t["fill_launches"] and B <= engine.pf_banded_times()["band"]
    tb, tp = engine.pf_banded_times(), engine.pf_banded_probs_times()
    if probs is None:
        probs = (engine.pf_banded_probs(s, cons, mfe_hint=hint, cutoff=cutoff), engine.pf_banded_times(),
                 engine.pf_banded_probs_times())
    probs, tb2, tp2 = probs
    assert {k: got[k] for k in SHARED} == {k: probs[k] for k in SHARED} and pp.same_bits(got, probs)
    assert all(tb[k] == tb2[k] for k in ("attempts", "lns", "band", "launches"))
    assert (tp["n_pairs"], tp["extra_bytes"]) == (tp2["n_pairs"], tp2["extra_bytes"])
    db, score = engine.mea_pairs(L, probs["pairs"], probs["unpaired"], gamma)
    assert db == got["mea"] and np.float64(score).tobytes() == np.float64(got["mea_score"]).tobytes()
    return got


def check_degenerate_bands(engine, oracle):
    for L in (1, 4, 5, 6, 57):
        s = rand_seq(np.random.default_rng(100 + L), L)
        for S in sorted({1, 4, 5, 6, max(1, L - 1), L, 3 * L}):
            with model(engine, oracle, S=S):
                got = check_call(engine, s, what="L=%d S=%d" % (L, S))
                if S < 5:  # nothing pairs: every u is exactly 1
                    assert got["mea"] == "." * L and got["mea_score"] == float(L)
                if L == 57 and S >= 57:
                    assert got["mea"].count("(") > 5


def check_whole_triangle(engine, oracle, L):
    """B = L around a wave's 64 lanes; the cutoff low enough that the list reaches the record's corners"""
    s = "G" + rand_seq(np.random.default_rng(L + 7), L - 2) + "C"
    with model(engine, oracle, S=L):
        for gamma in GAMMAS:
            got = check_call(engine, s, cutoff=1e-6, gamma=gamma, what="L=%d S=L" % L)
            assert engine.mea_times()["band"] == L  # the pair (1, L) is listed: the MEA's band is the whole record
        assert got["mea"].count("(") > 5


def edge_pairs(db, B, L):
    pt = [(a + 1, b + 1) for a, b in pair_table(db).items() if a < b]
    return any(j - i == B - 1 for i, j in pt), any(j >= L - 5 for i, j in pt)


def check_live_edge(engine, oracle, kind, S, L=433):
    s, ref = bp.live_edge_record(oracle, kind, L, S)
    P = pp.upper(ref["bpp"])
    what = "%s %d/%d" % (kind, L, S)
    cutoff = pp.settle_cutoff(P, what)
    ref_list = list_of(P, cutoff)
    ref_unp = pp.nucleotide_reference(P)[0]
    B = min(S, L)
    with model(engine, oracle, bp.kind_params(kind), S):
        probs = (engine.pf_banded_probs(s, cutoff=cutoff), engine.pf_banded_times(), engine.pf_banded_probs_times())
    for gamma in GAMMAS:
        odb, oscore = mea_reference(L, ref_list, ref_unp, gamma)
        assert edge_pairs(odb, B, L) == (True, True), (what, gamma)  # (c), on the oracle's list first
        with model(engine, oracle, bp.kind_params(kind), S):
            got = check_call(engine, s, cutoff=cutoff, gamma=gamma, what=what, probs=probs)  # (a), (b)
        assert edge_pairs(got["mea"], B, L) == (True, True), (what, gamma)  # (c)
        # (d) against the oracle's numbers
        tol = PF_TOL * L * max(1.0, 2.0 * gamma)
        mine = score_under(got["mea"], P, ref_unp, gamma)
        print("%s gamma=%g: |score - oracle's| = %.3g, the engine's structure under the oracle's numbers falls short by %.3g "
              "(bar %.3g)" % (what, gamma, abs(got["mea_score"] - oscore), oscore - mine, tol))
        assert abs(got["mea_score"] - oscore) <= tol
        assert mine >= oscore - 2.0 * tol
        have = np.stack([got["pairs"]["i"], got["pairs"]["j"]], axis=1)
        want = np.stack([ref_list["i"], ref_list["j"]], axis=1)
        assert have.shape == want.shape and (have == want).all()


def check_constraints(engine, oracle, L=200, S=60, cutoff=0.01):
    def make(k):
        s, cons = marked_record(L, S, L + S + 1 + 1000 * k)
        oracle.set_max_bp_span(S)
        try:
            ref = oracle_pf(oracle, s, cons, want_bpp=True)
        finally:
            oracle.set_max_bp_span(0)
        return s, cons, pp.upper(ref["bpp"])
    s, cons, P = pp.seeded(make, cutoff)
    assert set("x<>()") <= set(cons)
    xs = [k for k, ch in enumerate(cons) if ch == "x"]
    forced = sorted((a, b) for a, b in pair_table(cons.replace("x", ".").replace("<", ".").replace(">", ".")).items() if a < b)
    assert forced and xs
    for gamma in GAMMAS:
        with model(engine, oracle, S=S):
            got = check_call(engine, s, cons, cutoff=cutoff, gamma=gamma, what="constrained %d/%d" % (L, S))
        assert all(got["mea"][k] == "." for k in xs)
        mine = [(a, b) for a, b in pair_table(got["mea"]).items() if a < b]
        assert len(mine) > 10
        for a, b in forced:
            assert not any((i < a < j < b) or (a < i < b < j) for i, j in mine), (a, b)
    assert all((a, b) in mine for a, b in forced)  # at gamma = 4 the forced pairs (p = 1) are in


def check_long_record(engine, oracle, L, S, seed, past, cutoff=0.01, gamma=1.0):
    """a block record: no listed pair crosses a block and u = 1 on the N between them, so the structure is the blocks'
    reference structures joined by dots, and the score the sum of the blocks' to the error of two summation orders"""
    blocks, _ = pp.pooled_blocks(L, S, seed, False)
    seq = ("N" * S).join(blocks)
    assert len(seq) == L
    with model(engine, oracle, S=S):
        e, _ = engine.fold_banded(seq, structure=False)
        got = engine.pf_banded_mea(seq, mfe_hint=e, cutoff=cutoff, gamma=gamma)
        print("%d nt:" % L, engine.pf_banded_times(), engine.pf_banded_probs_times(), engine.mea_times())
        assert engine.mea_times()["extra_bytes"] == mea_bytes(L, len(got["pairs"]))
    pr, unp = got["pairs"], got["unpaired"]
    done = {}  # the blocks come from a small pool: a block's list repeats bit for bit only where its neighbours do
    want, total, pos, covered = [], 0.0, 0, 0
    for b, blk in enumerate(blocks):
        n = len(blk)
        lo, hi = np.searchsorted(pr["i"], [pos + 1, pos + n + 1])
        covered += hi - lo
        sub = pr[lo:hi].copy()
        assert (sub["j"] <= pos + n).all()  # no listed pair leaves its block
        sub["i"] -= pos
        sub["j"] -= pos
        key = (sub.tobytes(), unp[pos:pos + n].tobytes())
        if key not in done:
            done[key] = mea_reference(n, sub, unp[pos:pos + n], gamma)
        want.append(done[key][0])
        total += done[key][1]
        if b < len(blocks) - 1:
            assert (unp[pos + n:pos + n + S] == 1.0).all()
            total += float(S)
        pos += n + S
    assert covered == len(pr)  # every listed pair starts inside a block
    want = ("." * S).join(want)
    assert got["mea"] == want
    print("score %.17g, the blocks' %.17g" % (got["mea_score"], total))
    assert abs(got["mea_score"] - total) <= 4 * L * 2.0 ** -53 * got["mea_score"]
    mine = [(a, b) for a, b in pair_table(got["mea"]).items() if a < b]
    assert sum(1 for a, b in mine if a > past) > 10


# ---- the C ABI ----

def check_abi(engine):
    lib = engine.lib
    s = b"GGGGGGAAACCCCCCA" * 3 + b"ACGU" * 4  # 64 nt
    L = len(s)
    out = np.frombuffer(b"\x5a" * 32, dtype=np.float64).copy()
    cen = np.frombuffer(b"?" * (L + 1), dtype=np.uint8).copy()
    mea = np.frombuffer(b"!" * (L + 1), dtype=np.uint8).copy()
    unp = np.frombuffer(b"\x5b" * (8 * L), dtype=np.float64).copy()
    ent = np.frombuffer(b"\x5c" * (8 * L), dtype=np.float64).copy()
    n = ctypes.c_size_t(12345)
    a = [out[0:].ctypes.data, out[1:].ctypes.data, cen.ctypes.data, out[2:].ctypes.data, unp.ctypes.data, ent.ctypes.data,
         ctypes.byref(n), mea.ctypes.data, out[3:].ctypes.data]

    def untouched():
        return (out.tobytes() == b"\x5a" * 32 and cen.tobytes() == b"?" * (L + 1) and unp.tobytes() == b"\x5b" * (8 * L)
                and ent.tobytes() == b"\x5c" * (8 * L) and n.value == 12345 and mea.tobytes() == b"!" * (L + 1))

    def listed():
        m = ctypes.c_size_t(0)
        assert lib.sf_pf_probs_pairs(None, 0, ctypes.byref(m)) == 0
        buf = np.zeros(m.value, dtype=_lib.PAIR_PROB_DTYPE)
        assert lib.sf_pf_probs_pairs(buf.ctypes.data, m.value, None) == 0
        return buf

    engine.set_max_bp_span(0)
    assert lib.sf_pf_banded_mea(s, L, None, None, 0.01, 1.0, *a) == -3  # no span set
    with pytest.raises(_lib.ScanFoldHipError):
        engine.pf_banded_mea(s)
    engine.set_max_bp_span(30)
    try:
        first = engine.pf_banded_mea(s, cutoff=0.01, gamma=1.0)
        times = engine.mea_times()
        assert len(first["pairs"]) >= 6 and listed().tobytes() == first["pairs"].tobytes() and first["mea"].count("(") >= 6
        launches = engine.pf_banded_times()["launches"]
        for gamma in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
            assert lib.sf_pf_banded_mea(s, L, None, None, 0.01, gamma, *a) == -3
            with pytest.raises(_lib.ScanFoldHipError):
                engine.pf_banded_mea(s, gamma=gamma)
        for cutoff in (0.0, -1.0, 1.5, float("nan"), float("inf")):
            assert lib.sf_pf_banded_mea(s, L, None, None, cutoff, 1.0, *a) == -3
        assert lib.sf_pf_banded_mea(s, 0, None, None, 0.01, 1.0, *a) == -3
        assert lib.sf_pf_banded_mea(s, _lib.SF_MAX_BANDED + 1, None, None, 0.01, 1.0, *a) == -3
        assert lib.sf_pf_banded_mea(None, L, None, None, 0.01, 1.0, *a) == -3
        assert lib.sf_pf_banded_mea(s, L, b"((((" + b"." * (L - 4), None, 0.01, 1.0, *a) == -9
        assert engine.pf_banded_times()["launches"] == launches and untouched()
        # a failed call leaves the staged list and the figures of the last good one in place
        assert listed().tobytes() == first["pairs"].tobytes() and engine.mea_times() == times
        # every output may be NULL; the list is staged all the same
        assert lib.sf_pf_banded_mea(s, L, None, None, 0.5, 1.0, *([None] * 9)) == 0
        assert untouched()
        half = listed()
        assert half.tobytes() == first["pairs"][first["pairs"]["p"] >= 0.5].tobytes() and 0 < len(half) < len(first["pairs"])
        # all outputs at once
        assert lib.sf_pf_banded_mea(s, L, None, None, 0.01, 1.0, *a) == 0
        assert n.value == len(first["pairs"]) and cen[L] == 0 and mea[L] == 0
        assert bytes(mea[:L]).decode() == first["mea"] and bytes(cen[:L]).decode() == first["centroid"]
        assert unp.tobytes() == first["unpaired"].tobytes() and ent.tobytes() == first["entropy"].tobytes()
        assert [float(x) for x in out] == [first[k] for k in ("dG", "mean_bp_dist", "centroid_dist", "mea_score")]
    finally:
        engine.set_max_bp_span(0)

    # sf_mea_pairs: no span needed
    pairs, u = first["pairs"].copy(), first["unpaired"].copy()
    db = np.frombuffer(b"!" * (L + 1), dtype=np.uint8).copy()
    sc = np.frombuffer(b"\x5a" * 8, dtype=np.float64).copy()
    assert lib.sf_mea_pairs(L, pairs.ctypes.data, len(pairs), u.ctypes.data, 1.0, db.ctypes.data, sc.ctypes.data) == 0
    assert bytes(db[:L]).decode() == first["mea"] and db[L] == 0 and float(sc[0]) == first["mea_score"]
    times = engine.mea_times()
    assert times["extra_bytes"] == mea_pairs_bytes(L, times["band"], len(pairs))
    db[:] = ord("!")
    sc[:] = np.frombuffer(b"\x5a" * 8, dtype=np.float64)

    def bad(L_=L, pr=pairs, n_=None, u_=u, gamma=1.0):
        rc = lib.sf_mea_pairs(L_, None if pr is None else pr.ctypes.data, len(pr) if n_ is None else n_,
                              None if u_ is None else u_.ctypes.data, gamma, db.ctypes.data, sc.ctypes.data)
        assert db.tobytes() == b"!" * (L + 1) and sc.tobytes() == b"\x5a" * 8
        return rc

    def edited(t, **kw):
        pr = pairs.copy()
        for k, v in kw.items():
            pr[k][t] = v
        return pr

    launched = len(launch_names(engine))
    for gamma in (0.0, -2.0, float("nan"), float("inf")):
        assert bad(gamma=gamma) == -3
    assert bad(L_=0) == -3 and bad(L_=_lib.SF_MAX_BANDED + 1) == -3
    assert bad(pr=None, n_=3) == -3 and bad(u_=None) == -3
    swapped = pairs.copy()
    swapped[[2, 3]] = swapped[[3, 2]]
    assert bad(pr=swapped) == -3  # out of order
    assert bad(pr=np.concatenate([pairs[:3], pairs[2:]])) == -3  # a record twice
    assert bad(pr=edited(4, j=pairs["i"][4])) == -3  # i >= j
    assert bad(pr=edited(len(pairs) - 1, j=L + 1)) == -3  # j > L
    assert bad(pr=edited(0, i=0)) == -3
    for p in (-0.5, 1.5, float("nan"), float("inf")):
        assert bad(pr=edited(1, p=p)) == -3
    for v in (-0.5, 1.5, float("nan")):
        u2 = u.copy()
        u2[9] = v
        assert bad(u_=u2) == -3
    assert len(launch_names(engine)) == launched and engine.mea_times() == times
    with pytest.raises(_lib.ScanFoldHipError):
        engine.mea_pairs(L, swapped, u)
    # every output may be NULL; an empty list needs no pointer
    assert lib.sf_mea_pairs(L, pairs.ctypes.data, len(pairs), u.ctypes.data, 1.0, None, None) == 0
    assert lib.sf_mea_pairs(L, None, 0, u.ctypes.data, 1.0, db.ctypes.data, sc.ctypes.data) == 0
    assert bytes(db[:L]) == b"." * L and db[L] == 0


def launch_names(engine):
    """the emulation build's launch log (not cleared), or nothing on a real device: there the failed calls are told from
    sf_mea_times alone"""
    fn = getattr(engine.lib, "sfemul_launch_log", None)
    if fn is None:
        return []
    fn.restype = ctypes.c_char_p
    return fn().decode().split("\n")[:-1]


def check_route(engine, monkeypatch):
    s = "GGGGGGAAACCCCCCA" * 4
    engine.set_max_bp_span(0)
    with pytest.raises(ValueError, match="the banded ensemble needs a base-pair span"):
        whole.pf_mea(engine, s)
    assert whole.ENTRY_POINTS == ("fold_long", "fold_long_batch", "fold_banded", "fold_banded_batch", "pf_long",
                                  "pf_long_batch", "pf_banded")
    engine.set_max_bp_span(40)
    try:
        got = whole.pf_mea(engine, s, None, None, 0.02, 4.0)
        want = engine.pf_banded_mea(s, cutoff=0.02, gamma=4.0)
        assert {k: got[k] for k in SHARED + ("mea", "mea_score")} == {k: want[k] for k in SHARED + ("mea", "mea_score")}
        assert pp.same_bits(got, want) and got["mea"].count("(") > 10
        monkeypatch.setattr(engine, "has_pf_banded_mea", lambda: False)
        with pytest.raises(_lib.ScanFoldHipError, match="sf_pf_banded_mea, which this library"):
            whole.pf_mea(engine, s)
    finally:
        engine.set_max_bp_span(0)


# ---- the combined driver ----

def run_global_mea(engine, tmp_path, monkeypatch, seq, S, scan_args, cutoff, gamma):
    """scanfold.main(... --global_bpp CUTOFF --global_mea GAMMA) beside the run without --global_mea: every file of that run
    is there with the same bytes, and the three new files hold Engine.pf_banded_mea's structures"""
    monkeypatch.setattr(_lib, "_engine", engine)
    engine.set_max_bp_span(0)
    engine.md_span = 0
    params0 = engine.params
    files = {}
    for tag, extra in (("bpp", []), ("mea", ["--global_mea", repr(gamma)])):
        d = tmp_path / tag
        d.mkdir()
        monkeypatch.chdir(d)
        (d / "in.fa").write_text(">recE\n" + seq + "\n")
        assert sfd.main(["in.fa"] + scan_args + ["--name", "ge", "--dont_extract", "--global_refold", "--global_span", str(S),
                                                 "--global_ensemble_banded", "--global_bpp", repr(cutoff)] + extra) == 0
        assert engine.max_bp_span == 0 and engine.md_span == 0 and engine.params is params0
        files[tag] = {f: (d / f).read_bytes() for f in sorted(os.listdir(d))}
    new = sorted(set(files["mea"]) - set(files["bpp"]))
    base = [f[:-len(".out")] for f in files["bpp"] if f.endswith(".out")][0]
    assert new == sorted(base + ".global_refold." + tag + ".mea.dbn" for tag in ("full", "-1", "-2"))
    assert {f: files["mea"][f] for f in files["bpp"]} == files["bpp"]
    assert (base + ".global_refold.full.bpp.txt") in files["bpp"]
    d = tmp_path / "mea"
    engine.set_max_bp_span(S)
    try:
        for tag in ("full", "-1", "-2"):
            cons = None
            if tag != "full":
                cons = (d / (base + ".ScanFold." + tag + ".dbn")).read_text().split("\n")[2]
                cons = cons + "." * (len(seq) - len(cons))
            e, _ = engine.fold_banded(seq, cons, structure=False)
            r = engine.pf_banded_mea(seq, cons, mfe_hint=e, cutoff=cutoff, gamma=gamma)
            assert r["mea"].count("(") > 20
            want = ">ge %s MEA gamma=%g cutoff=%g span=%d score=%.2f\n%s\n%s\n" % (tag, gamma, cutoff, S, r["mea_score"], seq,
                                                                                 r["mea"])
            assert files["mea"][base + ".global_refold." + tag + ".mea.dbn"].decode() == want
    finally:
        engine.set_max_bp_span(0)


def check_driver_refusals(tmp_path, monkeypatch):
    """--global_mea without --global_bpp, with a gamma that is not finite or not positive, or with --lri: refused before
    anything is scanned or written"""
    monkeypatch.chdir(tmp_path)
    (tmp_path / "r.fa").write_text(">r\n" + "ACGU" * 100 + "\n")
    scan = ["r.fa", "-w", "120", "-s", "100", "-r", "3"]
    bpp = ["--global_refold", "--global_span", "150", "--global_ensemble_banded", "--global_bpp", "0.01"]
    for extra in (["--global_mea", "1"],
                  ["--global_refold", "--global_span", "150", "--global_ensemble_banded", "--global_mea", "1"],
                  bpp + ["--global_mea", "0"], bpp + ["--global_mea", "-1"], bpp + ["--global_mea", "nan"],
                  bpp + ["--global_mea", "inf"],
                  bpp + ["--global_mea", "1", "--lri"]):
        with pytest.raises(ValueError, match="--global_mea"):
            sfd.main(scan + extra)
    assert os.listdir(tmp_path) == ["r.fa"]
