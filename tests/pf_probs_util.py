"""Checks of the base-pair probabilities of a whole record under a span (sf_pf_banded_probs, include/scanfold_hip_long.h),
shared by tests/test_pf_probs.py (the kernel source compiled for the CPU) and tests/test_gpu_pf_probs.py (the MI355X).

Reference: the oracle's bpp matrix, oracle.pf(want_bpp=True) under span and constraint for short records and for the blocks
of block records, oracle.pf_cubic in long double (long_pf_util.cubic_reference; its matrix comes back in doubles) at 433 and
1 200 nt.  unpaired and entropy are formed from the matrix in numpy, the sums in long double.

Bars.  |p - p_ref| <= PF_TOL (1e-8, the project's bar; p <= 1) for every listed pair and for unpaired; the set of listed
pairs equals {p_ref >= cutoff} exactly; the list is strictly ascending in (i, j).  Every check first asserts on the reference
alone that no probability lies within CUTOFF_GAP = 1e-6 of the cutoff, as banded_pf_util.nothing_to_excuse does for 0.5, so
nothing is ever excused: a record made from a seed takes the construction's next seed instead (seeded), and a record that
another module chose (live_edge_record's) takes the next cutoff of CUTOFF_LADDER (settle_cutoff), both looking at the
reference only.

The entropy's bar is not PF_TOL by decree: p log2 p has an unbounded slope at 0.  It is ten times the largest difference
between two references that the code under test plays no part in, the entropy from oracle.pf in double and from
oracle.pf_cubic in long double, on the 433-nt records of the wave-edge cases (EDGE_CASES under their spans; measure_entropy_bar
prints it): measured 2.4e-13 bits (the five records gave 2.1e-14, 4.8e-14, 5.8e-14, 4.2e-14 and 2.3e-13), ten times which is
below PF_TOL, so the bar is PF_TOL = 1e-8 bits."""
import ctypes
import os

import numpy as np
import pytest

from scanfold_amd import _lib, params
from scanfold_amd import scanfold as sfd
from scanfold_amd import whole
from long_pf_util import KEYS, cubic_reference, oracle_pf
from long_util import block_constraint, hairpin_rich, pair_table, rand_seq
from test_banded_fold import marked_record, model
from test_gpu_parity import PF_TOL
import banded_pf_util as bp

CUTOFF_GAP = 1e-6
CUTOFF_LADDER = (0.01, 0.013, 0.017, 0.023)
MEASURED_ENTROPY_GAP = 2.4e-13  # bits, between the two references (measure_entropy_bar)
ENTROPY_TOL = max(10 * MEASURED_ENTROPY_GAP, PF_TOL)
EDGE_CASES = [("random", 30), ("hairpin_rich", 64), ("hairpin_rich", 65), ("multiloop_rich", 129), ("random", 400)]  # at 433 nt
CLASSIC = KEYS + ("centroid",)


# ---- the reference ----

def upper(bpp):
    """the oracle's 1-based square matrix -> (L, L) with p(i, j) at [i - 1, j - 1], i < j, and 0 elsewhere"""
    return np.triu(np.maximum(bpp, bpp.T)[1:, 1:], 1)


def nucleotide_reference(P):
    """-> (unpaired, entropy in bits) of the upper-triangular matrix P, summed in long double"""
    Q = (P + P.T).astype(np.longdouble)
    unp = np.clip(1 - Q.sum(axis=1), 0, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = np.where(Q > 0, Q * np.log2(Q), 0).sum(axis=1)
        ent = -h - np.where(unp > 0, unp * np.log2(unp), 0)
    return unp.astype(np.float64), ent.astype(np.float64)


def clear_of(P, cutoff, what=""):
    """no probability of the reference within CUTOFF_GAP of the cutoff"""
    gap = float(np.abs(P[P > 0] - cutoff).min()) if (P > 0).any() else 1.0
    print("%s closest probability to the cutoff %g: |p - cutoff| = %.3g" % (what, cutoff, gap))
    return gap > CUTOFF_GAP


def settle_cutoff(P, what=""):
    for cutoff in CUTOFF_LADDER:
        if clear_of(P, cutoff, what):
            return cutoff
    raise AssertionError("every cutoff of the ladder has a reference probability within %g: %s" % (CUTOFF_GAP, what))


def seeded(make, cutoff, tries=8):
    """make(k) -> (anything, P) for k = 0, 1, ...: the first whose reference is clear of the cutoff"""
    for k in range(tries):
        out = make(k)
        if clear_of(out[-1], cutoff):
            return out
    raise AssertionError("no seed gave a reference clear of the cutoff %g" % cutoff)


# ---- the bar ----

def check_list_shape(pairs, L):
    assert pairs.dtype == _lib.PAIR_PROB_DTYPE and pairs.dtype.itemsize == 16
    i, j = pairs["i"].astype(np.int64), pairs["j"].astype(np.int64)
    assert ((1 <= i) & (i < j) & (j <= L)).all()
    key = i * (L + 1) + j
    assert (np.diff(key) > 0).all(), "the list is not strictly ascending in (i, j)"


def check_against(got, P, unp_ref, ent_ref, cutoff, what=""):
    """got: Engine.pf_banded_probs's dict; P: upper(reference); prints each figure before it asserts"""
    L = P.shape[0]
    pairs = got["pairs"]
    check_list_shape(pairs, L)
    assert got["unpaired"].shape == got["entropy"].shape == (L,)
    assert got["unpaired"].dtype == got["entropy"].dtype == np.float64
    want = np.argwhere(P >= cutoff)  # (row-major: ascending in (i, j))
    have = np.stack([pairs["i"] - 1, pairs["j"] - 1], axis=1).astype(np.int64) if len(pairs) else np.zeros((0, 2), np.int64)
    print("%s listed %d pairs, the reference has %d at p >= %g" % (what, len(have), len(want), cutoff))
    assert have.shape == want.shape and (have == want).all(), (what, len(have), len(want))
    dp = float(np.abs(pairs["p"] - P[have[:, 0], have[:, 1]]).max()) if len(pairs) else 0.0
    du = float(np.abs(got["unpaired"] - unp_ref).max())
    de = float(np.abs(got["entropy"] - ent_ref).max())
    print("%s max |p - ref| = %.3g, max |unpaired - ref| = %.3g (bar %.3g); max |entropy - ref| = %.3g bits (bar %.3g)"
          % (what, dp, du, PF_TOL, de, ENTROPY_TOL))
    assert np.isfinite(got["unpaired"]).all() and np.isfinite(got["entropy"]).all()
    assert dp <= PF_TOL and du <= PF_TOL, (what, dp, du)
    assert de <= ENTROPY_TOL, (what, de)
    assert (got["unpaired"] >= 0).all() and (got["unpaired"] <= 1).all()


def same_bits(a, b):
    return all(a[k].tobytes() == b[k].tobytes() and a[k].dtype == b[k].dtype for k in ("unpaired", "entropy", "pairs"))


def classic(r):
    return {k: r[k] for k in CLASSIC}


# ---- degenerate bands, wave edges ----

def check_degenerate_bands(engine, oracle, cutoff=0.01):
    for L in (1, 4, 5, 6, 57):
        for S in sorted({1, 4, 5, 6, max(1, L - 1), L, 3 * L}):
            with model(engine, oracle, S=S):
                def make(k):
                    s = rand_seq(np.random.default_rng(100 + L + 1000 * k), L)
                    return s, upper(oracle.pf(s, want_bpp=True)["bpp"])
                s, P = seeded(make, cutoff)
                got = engine.pf_banded_probs(s, cutoff=cutoff)
                check_against(got, P, *nucleotide_reference(P), cutoff, "L=%d S=%d" % (L, S))
                assert classic(got) == engine.pf_banded(s)
                if S < 5:  # a pair needs three unpaired bases inside: nothing pairs
                    assert len(got["pairs"]) == 0
                    assert got["unpaired"].tobytes() == np.ones(L).tobytes()
                    assert got["entropy"].tobytes() == np.zeros(L).tobytes()
                if L == 57 and S >= 57:
                    assert len(got["pairs"]) > 20


def check_whole_triangle(engine, oracle, L, S, cutoff=0.01):
    """S >= L (B = L): the unrestricted probabilities; rows of L - 1 cells at most around a wave's 64"""
    with model(engine, oracle, S=S):
        def make(k):
            s = "G" + rand_seq(np.random.default_rng(L + 7 + 1000 * k), L - 2) + "C"
            return s, upper(oracle.pf(s, want_bpp=True)["bpp"])
        s, P = seeded(make, cutoff)
        assert P[0, L - 1] > 1e-30  # the first row is live in its last cell (at 65 nt the only one of the ballot's second chunk)
        got = engine.pf_banded_probs(s, cutoff=1e-30)
        j_of_1 = got["pairs"]["j"][got["pairs"]["i"] == 1]
        assert j_of_1.max() == L  # that last cell is listed
        check_against(engine.pf_banded_probs(s, cutoff=cutoff), P, *nucleotide_reference(P), cutoff, "L=%d S=%d" % (L, S))


def check_live_edge(engine, oracle, kind, L, S):
    """live_edge_record's record: the reference itself has p > 0.5 on the band's last diagonal and in the last 6 nt"""
    s, ref = bp.live_edge_record(oracle, kind, L, S)
    bp.assert_live_edge(ref, L, S)
    P = upper(ref["bpp"])
    cutoff = settle_cutoff(P, "%s %d/%d" % (kind, L, S))
    with model(engine, oracle, bp.kind_params(kind), S):
        got = engine.pf_banded_probs(s, cutoff=cutoff)
    check_against(got, P, *nucleotide_reference(P), cutoff, "%s %d/%d" % (kind, L, S))
    d = got["pairs"]["j"] - got["pairs"]["i"]
    assert d.max() == min(S, L) - 1 and got["pairs"]["j"].max() >= L - 6  # the list reaches both edges
    return got


def check_loaded(engine, oracle, pset, L, S, seed, cutoff=0.01):
    """a random record under the parameter set pset (resident on the engine already) against the cubic reference"""
    def make(k):
        s = rand_seq(np.random.default_rng(seed + 1000 * k), L)
        return s, upper(cubic_reference(oracle, s, pset, span=S)["bpp"])
    s, P = seeded(make, cutoff)
    engine.set_max_bp_span(S)
    try:
        got = engine.pf_banded_probs(s, cutoff=cutoff)
    finally:
        engine.set_max_bp_span(0)
    assert len(got["pairs"]) > L // 4
    check_against(got, P, *nucleotide_reference(P), cutoff, "seed %d, %d/%d" % (seed, L, S))


def measure_entropy_bar(oracle, L=433):
    """the largest difference between the entropies of the two references on the wave-edge records; prints each"""
    worst = 0.0
    for kind, S in EDGE_CASES:
        s, ref = bp.live_edge_record(oracle, kind, L, S)
        p = bp.kind_params(kind)
        oracle.set_max_bp_span(S)
        if p is not None:
            oracle.set_params(p)
        try:
            dbl = oracle.pf(s, want_bpp=True)
        finally:
            oracle.set_max_bp_span(0)
            oracle.set_params(params.default_params())
        e_long = nucleotide_reference(upper(ref["bpp"]))[1]
        e_dbl = nucleotide_reference(upper(dbl["bpp"]))[1]
        gap = float(np.abs(e_long - e_dbl).max())
        print("%s %d/%d: max |entropy(pf, double) - entropy(pf_cubic, long double)| = %.3g bits" % (kind, L, S, gap))
        worst = max(worst, gap)
    return worst


# ---- constraints ----

def check_constraints(engine, oracle, L=200, S=60, cutoff=0.01):
    def make(k):
        s, cons = marked_record(L, S, L + S + 1 + 1000 * k)
        oracle.set_max_bp_span(S)
        try:
            ref = oracle_pf(oracle, s, cons, want_bpp=True)
        finally:
            oracle.set_max_bp_span(0)
        return s, cons, upper(ref["bpp"])
    s, cons, P = seeded(make, cutoff)
    assert set("x<>()") <= set(cons)
    with model(engine, oracle, S=S):
        got = engine.pf_banded_probs(s, cons, cutoff=cutoff)
        assert classic(got) == engine.pf_banded(s, cons)
    check_against(got, P, *nucleotide_reference(P), cutoff, "constrained %d/%d" % (L, S))
    xs = np.array([k for k, ch in enumerate(cons) if ch == "x"])
    assert (got["unpaired"][xs] == 1.0).all()  # exactly
    i, j = got["pairs"]["i"] - 1, got["pairs"]["j"] - 1
    assert not np.isin(i, xs).any() and not np.isin(j, xs).any()
    forced = sorted((a, b) for a, b in pair_table(cons.replace("x", ".").replace("<", ".").replace(">", ".")).items() if a < b)
    assert forced
    listed = {(int(a), int(b)): float(p) for a, b, p in zip(i, j, got["pairs"]["p"])}
    for a, b in forced:
        crossing = ((i < a) & (a < j) & (j < b)) | ((a < i) & (i < b) & (b < j))
        assert not crossing.any(), (a, b)
        print("forced pair (%d, %d): p = %.17g, the oracle's %.17g" % (a + 1, b + 1, listed.get((a, b), 0.0), P[a, b]))
        assert P[a, b] >= cutoff and abs(listed[a, b] - P[a, b]) <= PF_TOL


# ---- consistency without the oracle, identity, cutoffs ----

def check_consistency(engine, oracle, L=433, S=65):
    s, _ = bp.live_edge_record(oracle, "hairpin_rich", L, S)
    engine.set_max_bp_span(S)
    try:
        got = engine.pf_banded_probs(s, cutoff=1e-30)
    finally:
        engine.set_max_bp_span(0)
    pr = got["pairs"]
    check_list_shape(pr, L)
    p = pr["p"]
    mbd = 2.0 * float((p * (1.0 - p)).sum())
    print("2 sum p (1 - p) over %d pairs = %.15g, mean_bp_dist = %.15g" % (len(p), mbd, got["mean_bp_dist"]))
    assert abs(mbd - got["mean_bp_dist"]) <= PF_TOL * max(1.0, abs(got["mean_bp_dist"]))
    db = ["."] * L
    for i, j in zip(pr["i"][p > 0.5], pr["j"][p > 0.5]):
        db[i - 1], db[j - 1] = "(", ")"
    assert "".join(db) == got["centroid"] and got["centroid"].count("(") > 5
    paired = np.zeros(L)
    np.add.at(paired, pr["i"] - 1, p)
    np.add.at(paired, pr["j"] - 1, p)
    worst = float(np.abs(got["unpaired"] + paired - 1.0).max())
    print("max |unpaired + sum of the listed p - 1| = %.3g" % worst)
    assert worst <= 1e-12


def check_identity(engine, oracle, L=433, S=65):
    """the four classic outputs are pf_banded's bit for bit, with and without constraint and hint; two calls, the same bytes"""
    s, _ = bp.live_edge_record(oracle, "hairpin_rich", L, S)
    s2, cons = marked_record(L, S, L + S + 1)
    engine.set_max_bp_span(S)
    try:
        e, _ = engine.fold_banded(s, structure=False)
        for seq, c, hint in ((s, None, None), (s, None, e), (s2, cons, None)):
            a = engine.pf_banded_probs(seq, c, mfe_hint=hint)
            t = engine.pf_banded_times()
            assert classic(a) == engine.pf_banded(seq, c, mfe_hint=hint)
            t2 = engine.pf_banded_times()
            assert (t["attempts"], t["lns"], t["band"], t["launches"]) == (t2["attempts"], t2["lns"], t2["band"], t2["launches"])
            b = engine.pf_banded_probs(seq, c, mfe_hint=hint)
            assert classic(a) == classic(b) and same_bits(a, b)
            assert len(a["pairs"]) > L // 4
            x = engine.pf_banded_probs_times()
            assert x["n_pairs"] == len(a["pairs"]) and x["extra_bytes"] == 28 * L + 16 * len(a["pairs"]) and x["extract_ms"] > 0
    finally:
        engine.set_max_bp_span(0)


def check_cutoffs(engine, oracle, L=433, S=65):
    """0.5, 0.01 and 1e-5 on one record: each list is the finest one filtered by p >= cutoff, the same p bits; 1.0 is legal"""
    s, _ = bp.live_edge_record(oracle, "hairpin_rich", L, S)
    engine.set_max_bp_span(S)
    try:
        fine = engine.pf_banded_probs(s, cutoff=1e-5)
        assert len(fine["pairs"]) <= L * int(1 / 1e-5) // 2
        last = len(fine["pairs"]) + 1
        for cutoff in (0.01, 0.5, 1.0):
            got = engine.pf_banded_probs(s, cutoff=cutoff)
            keep = fine["pairs"][fine["pairs"]["p"] >= cutoff]
            assert got["pairs"].tobytes() == keep.tobytes()
            assert len(keep) < last and len(keep) <= L * int(1 / cutoff) // 2
            last = len(keep)
            assert got["unpaired"].tobytes() == fine["unpaired"].tobytes() and got["entropy"].tobytes() == fine["entropy"].tobytes()
        assert last < 40  # (p = 1 to the last bit is rare)
    finally:
        engine.set_max_bp_span(0)


# ---- records built from blocks ----

_blocks = {}  # (flanked sequence, constraint, S) -> upper(bpp) of the block, computed once per session


def block_matrix(oracle, seq, cons, S):
    key = (seq, cons, S)
    if key not in _blocks:
        _blocks[key] = upper(oracle_pf(oracle, seq, cons, want_bpp=True)["bpp"])
    return _blocks[key]


def pooled_blocks(L, S, seed, constrained, lo=150, hi=250, pool=12):
    """banded_pf_util.pooled_record's construction, keeping the blocks: -> (blocks, last_cons or None)"""
    rng = np.random.default_rng(seed)
    seqs = [hairpin_rich(rng, int(n)) for n in rng.integers(lo, hi + 1, pool)]
    blocks, n = [], 0
    while True:
        blk = seqs[int(rng.integers(0, pool))]
        rest = L - n
        if rest - len(blk) - S < 2 * lo + S:
            a = (rest - S) // 2
            blocks += [hairpin_rich(rng, a), hairpin_rich(rng, rest - S - a)]
            break
        blocks.append(blk)
        n += len(blk) + S
    last_cons = None
    if constrained:
        blocks[-1], last_cons = block_constraint(blocks[-1], rng, S, close_at_end=True)
    return blocks, last_cons


def pooled_reference(oracle, blocks, last_cons, S, cutoff):
    """blocks joined by S N fold independently under max_bp_span = S: -> (seq, cons, pairs (i, j, p) 1-based, unpaired,
    entropy, clear) from the blocks' oracle matrices shifted to their offsets; clear: no block probability near the cutoff"""
    seq = ("N" * S).join(blocks)
    L = len(seq)
    unp, ent = np.ones(L), np.zeros(L)
    rows, clear, pos = [], True, 0
    oracle.set_max_bp_span(S)
    try:
        for b, blk in enumerate(blocks):
            left = "N" if b > 0 else ""
            right = "N" if b < len(blocks) - 1 else ""
            bc = "." * len(left) + last_cons if last_cons is not None and b == len(blocks) - 1 else None
            P = block_matrix(oracle, left + blk + right, bc, S)
            clear = clear and bool((np.abs(P[P > 0] - cutoff) > CUTOFF_GAP).all())
            u, h = nucleotide_reference(P)
            n0 = len(left)
            assert P[:n0].sum() == 0 and P[:, n0 + len(blk):].sum() == 0  # (the flanking N pair with nothing)
            unp[pos:pos + len(blk)] = u[n0:n0 + len(blk)]
            ent[pos:pos + len(blk)] = h[n0:n0 + len(blk)]
            ij = np.argwhere(P >= cutoff)
            rows.append(np.column_stack([ij[:, 0] - n0 + pos + 1, ij[:, 1] - n0 + pos + 1, P[ij[:, 0], ij[:, 1]]]))
            pos += len(blk) + S
    finally:
        oracle.set_max_bp_span(0)
    cons = None if last_cons is None else "." * (L - len(last_cons)) + last_cons
    return seq, cons, np.concatenate(rows), unp, ent, clear


def check_pooled_record(engine, oracle, L, S, seed, constrained, past, cutoff=0.01):
    """a block record of L nt with listed pairs past position `past`"""
    for k in range(8):
        blocks, last_cons = pooled_blocks(L, S, seed + 1000 * k, constrained)
        seq, cons, want, unp, ent, clear = pooled_reference(oracle, blocks, last_cons, S, cutoff)
        if clear:
            break
    assert clear and len(seq) == L
    with model(engine, oracle, S=S):
        e, _ = engine.fold_banded(seq, cons, structure=False)
        got = engine.pf_banded_probs(seq, cons, mfe_hint=e, cutoff=cutoff)
        print("%d nt:" % L, engine.pf_banded_times(), engine.pf_banded_probs_times())
    pr = got["pairs"]
    check_list_shape(pr, L)
    assert len(pr) == len(want), (len(pr), len(want))
    assert (pr["i"] == want[:, 0]).all() and (pr["j"] == want[:, 1]).all()
    assert pr["j"].max() > past and (pr["i"] > past).sum() > 10
    dp = float(np.abs(pr["p"] - want[:, 2]).max())
    du = float(np.abs(got["unpaired"] - unp).max())
    de = float(np.abs(got["entropy"] - ent).max())
    print("%d pairs; max |p - ref| = %.3g, |unpaired - ref| = %.3g, |entropy - ref| = %.3g" % (len(pr), dp, du, de))
    assert dp <= PF_TOL and du <= PF_TOL and de <= ENTROPY_TOL
    if constrained:
        xs = np.array([k for k, ch in enumerate(cons) if ch == "x"])
        assert (got["unpaired"][xs] == 1.0).all()


# ---- the C ABI ----

def check_abi(engine):
    lib = engine.lib
    s = b"GGGGGGAAACCCCCCA" * 3 + b"ACGU" * 4  # 64 nt
    L = len(s)
    out = np.frombuffer(b"\x5a" * 24, dtype=np.float64).copy()
    cen = np.frombuffer(b"?" * (L + 1), dtype=np.uint8).copy()
    unp = np.frombuffer(b"\x5b" * (8 * L), dtype=np.float64).copy()
    ent = np.frombuffer(b"\x5c" * (8 * L), dtype=np.float64).copy()
    n = ctypes.c_size_t(12345)
    a = [out[0:].ctypes.data, out[1:].ctypes.data, cen.ctypes.data, out[2:].ctypes.data, unp.ctypes.data, ent.ctypes.data,
         ctypes.byref(n)]

    def untouched():
        return (out.tobytes() == b"\x5a" * 24 and cen.tobytes() == b"?" * (L + 1) and unp.tobytes() == b"\x5b" * (8 * L)
                and ent.tobytes() == b"\x5c" * (8 * L) and n.value == 12345)

    def listed():
        m = ctypes.c_size_t(0)
        assert lib.sf_pf_probs_pairs(None, 0, ctypes.byref(m)) == 0
        buf = np.zeros(m.value, dtype=_lib.PAIR_PROB_DTYPE)
        assert lib.sf_pf_probs_pairs(buf.ctypes.data, m.value, None) == 0
        return buf

    engine.set_max_bp_span(0)
    assert lib.sf_pf_banded_probs(s, L, None, None, 0.01, *a) == -3  # no span set
    with pytest.raises(_lib.ScanFoldHipError):
        engine.pf_banded_probs(s)
    engine.set_max_bp_span(30)
    try:
        first = engine.pf_banded_probs(s, cutoff=0.01)  # a list to be left in place
        assert len(first["pairs"]) >= 6 and listed().tobytes() == first["pairs"].tobytes()
        launches = engine.pf_banded_times()["launches"]
        for bad in (0.0, -1.0, 1.5, float("nan"), float("inf")):
            assert lib.sf_pf_banded_probs(s, L, None, None, bad, *a) == -3
            with pytest.raises(_lib.ScanFoldHipError):
                engine.pf_banded_probs(s, cutoff=bad)
        assert engine.pf_banded_times()["launches"] == launches and untouched()
        assert lib.sf_pf_banded_probs(s, 0, None, None, 0.01, *a) == -3
        assert lib.sf_pf_banded_probs(s, _lib.SF_MAX_BANDED + 1, None, None, 0.01, *a) == -3
        assert lib.sf_pf_banded_probs(None, L, None, None, 0.01, *a) == -3
        assert lib.sf_pf_banded_probs(s, L, b"((((" + b"." * (L - 4), None, 0.01, *a) == -9
        assert engine.pf_banded_times()["launches"] == launches and untouched()
        # the absurd hint of banded_pf_util.check_errors: SF_ERR_RANGE after every attempt, nothing written
        absurd = np.array([2000000000], dtype=np.int32)
        assert lib.sf_pf_banded_probs(s, L, None, absurd.ctypes.data, 0.01, *a) == -11
        t = engine.pf_banded_times()
        assert t["attempts"] == bp.MAX_ATTEMPTS and t["launches"] == bp.MAX_ATTEMPTS * 30, t
        assert untouched()
        # a failed call leaves the list of the last successful one in place
        assert listed().tobytes() == first["pairs"].tobytes()
        assert engine.pf_banded_probs_times()["n_pairs"] == len(first["pairs"])
        # every output may be NULL; the list is staged all the same
        assert lib.sf_pf_banded_probs(s, L, None, None, 0.5, None, None, None, None, None, None, None) == 0
        assert untouched()
        half = listed()
        assert half.tobytes() == first["pairs"][first["pairs"]["p"] >= 0.5].tobytes() and 0 < len(half) < len(first["pairs"])
        # cap < n: the first cap records, and n all the same; cap > 0 without a buffer is refused
        buf = np.zeros(len(half), dtype=_lib.PAIR_PROB_DTYPE)
        m = ctypes.c_size_t(0)
        assert lib.sf_pf_probs_pairs(buf.ctypes.data, 2, ctypes.byref(m)) == 0
        assert m.value == len(half) and buf[:2].tobytes() == half[:2].tobytes() and not buf[2:].tobytes().strip(b"\0")
        assert lib.sf_pf_probs_pairs(None, 2, ctypes.byref(m)) == -3
        assert lib.sf_pf_probs_pairs(buf.ctypes.data, len(half) + 5, ctypes.byref(m)) == 0 and buf.tobytes() == half.tobytes()
        # all outputs at once
        assert lib.sf_pf_banded_probs(s, L, None, None, 0.01, *a) == 0
        assert n.value == len(first["pairs"]) and cen[L] == 0 and set(bytes(cen[:L])) <= set(b"().")
        assert unp.tobytes() == first["unpaired"].tobytes() and ent.tobytes() == first["entropy"].tobytes()
        assert [float(out[0]), float(out[1]), float(out[2])] == [first[k] for k in KEYS]
    finally:
        engine.set_max_bp_span(0)


def check_route(engine, monkeypatch):
    """whole.pf_probs: the banded policy, a clear error without a span and on a library without the symbol"""
    s = "GGGGGGAAACCCCCCA" * 4
    engine.set_max_bp_span(0)
    with pytest.raises(ValueError, match="the banded ensemble needs a base-pair span"):
        whole.pf_probs(engine, s)
    engine.set_max_bp_span(40)
    try:
        got = whole.pf_probs(engine, s, None, None, 0.02)
        want = engine.pf_banded_probs(s, cutoff=0.02)
        assert classic(got) == classic(want) and same_bits(got, want)
        monkeypatch.setattr(engine, "has_pf_banded_probs", lambda: False)
        with pytest.raises(_lib.ScanFoldHipError, match="sf_pf_banded_probs, which this library"):
            whole.pf_probs(engine, s)
    finally:
        engine.set_max_bp_span(0)


# ---- the combined driver ----

def run_global_bpp(engine, tmp_path, monkeypatch, seq, S, scan_args, cutoff):
    """scanfold.main(... --global_ensemble_banded --global_bpp CUTOFF) beside the run without --global_bpp: every file of
    that run is there with the same bytes, and the six new files hold Engine.pf_banded_probs's lists and entropies"""
    monkeypatch.setattr(_lib, "_engine", engine)
    engine.set_max_bp_span(0)
    engine.md_span = 0
    params0 = engine.params
    files = {}
    for tag, extra in (("plain", []), ("bpp", ["--global_bpp", repr(cutoff)])):
        d = tmp_path / tag
        d.mkdir()
        monkeypatch.chdir(d)
        (d / "in.fa").write_text(">recE\n" + seq + "\n")
        assert sfd.main(["in.fa"] + scan_args + ["--name", "ge", "--dont_extract", "--global_refold", "--global_span", str(S),
                                                 "--global_ensemble_banded"] + extra) == 0
        assert engine.max_bp_span == 0 and engine.md_span == 0 and engine.params is params0
        files[tag] = {f: (d / f).read_bytes() for f in sorted(os.listdir(d))}
    new = sorted(set(files["bpp"]) - set(files["plain"]))
    base = [f[:-len(".out")] for f in files["plain"] if f.endswith(".out")][0]
    assert new == sorted(base + ".global_refold." + tag + tail for tag in ("full", "-1", "-2") for tail in (".bpp.txt", ".entropy.wig"))
    assert {f: files["bpp"][f] for f in files["plain"]} == files["plain"]  # the ensemble file among them
    assert (base + ".AllDBN-global_refold.ensemble.txt") in files["plain"]
    d = tmp_path / "bpp"
    engine.set_max_bp_span(S)
    try:
        for tag in ("full", "-1", "-2"):
            cons = None
            if tag != "full":
                cons = (d / (base + ".ScanFold." + tag + ".dbn")).read_text().split("\n")[2]
                cons = cons + "." * (len(seq) - len(cons))
            e, _ = engine.fold_banded(seq, cons, structure=False)
            r = engine.pf_banded_probs(seq, cons, mfe_hint=e, cutoff=cutoff)
            assert len(r["pairs"]) > 20
            want = "i\tj\tp span=%d\n" % S + "".join("%d\t%d\t%.6g\n" % (i, j, p) for i, j, p in r["pairs"].tolist())
            assert files["bpp"][base + ".global_refold." + tag + ".bpp.txt"].decode() == want
            wig = "fixedStep chrom=ge start=1 step=1 span=1\n" + "".join("%f\n" % v for v in r["entropy"])
            assert files["bpp"][base + ".global_refold." + tag + ".entropy.wig"].decode() == wig
    finally:
        engine.set_max_bp_span(0)


def check_driver_refusals(tmp_path, monkeypatch):
    """--global_bpp without --global_ensemble_banded, with a cutoff outside (0, 1], or with --lri: refused before anything
    is scanned or written"""
    monkeypatch.chdir(tmp_path)
    (tmp_path / "r.fa").write_text(">r\n" + "ACGU" * 100 + "\n")
    scan = ["r.fa", "-w", "120", "-s", "100", "-r", "3"]
    banded = ["--global_refold", "--global_span", "150", "--global_ensemble_banded"]
    for extra in (["--global_bpp", "0.01"],
                  ["--global_refold", "--global_span", "150", "--global_bpp", "0.01"],
                  ["--global_refold", "--global_ensemble", "--global_bpp", "0.01"],
                  banded + ["--global_bpp", "0"], banded + ["--global_bpp", "-0.5"], banded + ["--global_bpp", "1.5"],
                  banded + ["--global_bpp", "nan"],
                  banded + ["--global_bpp", "0.01", "--lri"]):
        with pytest.raises(ValueError, match="--global_bpp"):
            sfd.main(scan + extra)
    assert os.listdir(tmp_path) == ["r.fa"]
