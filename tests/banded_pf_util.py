"""Checks of the partition function under a span in banded tables (sf_pf_banded, include/scanfold_hip_long.h), shared by
tests/test_pf_banded.py (the kernel source compiled for the CPU) and tests/test_gpu_pf_banded.py (the MI355X).

The bar is long_pf_util.assert_close: PF_TOL = 1e-8 relative on dG, mean_bp_dist and centroid_dist, equal centroids apart
from at most MAX_EXCUSED threshold pairs.  Every check first asserts on its reference that there is nothing to excuse (no
probability within 1e-6 of 0.5) wherever the reference has probabilities; where it has none (Engine.pf_long, sums over
blocks) assert_close gets no matrix and so excuses nothing.

References: oracle.pf under the span for the degenerate bands; oracle.pf_cubic in long double under the span
(long_pf_util.cubic_reference) for records whose band is live up to its edge (test_banded_fold.edge_record and
multiloop_edge_record: the reference's own probabilities must put a pair on the band's last diagonal and one at the
record's end, and live_edge_record takes the construction's next seeds where edge_record's record, chosen by its MFE
structure, has that pair at p < 0.5); Engine.pf_long under the same span; and, for records no triangle holds, blocks
joined by runs of S N, which fold independently under max_bp_span = S (long_pf_util's module text): dG, mean_bp_dist and
centroid_dist are the sums of the blocks' oracle values and the centroid is the blocks' centroids joined by dots.
pooled_record draws its blocks from a small pool and caches each block's oracle.pf by sequence, so a record of 70 000 nt
costs a dozen oracle folds."""
import ctypes
import os

import numpy as np
import pytest

from scanfold_amd import _lib, params
from scanfold_amd import scanfold as sfd
from long_pf_util import KEYS, assert_close, cubic_reference, oracle_pf
from long_util import COMP, block_constraint, hairpin_rich, multiloop_rich, rand_seq, short_hairpin_params
from test_banded_fold import edge_record, marked_record, model, multiloop_edge_record, multiloop_params

KT37 = 0.61632  # kcal/mol at 37 C: ln Z = -dG / kT
MAX_ATTEMPTS = 6  # SF_PFLONG_MAX_ATTEMPTS


def banded_pf_bytes(L, S):
    """SF_PF_BANDED_BYTES of include/scanfold_hip_long.h: seven FP64 band tables and the documented linear term"""
    B = min(S, L)
    return 56 * L * B + 35 * L + 24 * B + 65677


def nothing_to_excuse(bpp, what=""):
    gap = float(np.abs(bpp - 0.5).min())
    print("%s closest probability to 0.5: |p - 0.5| = %.3g" % (what, gap))
    assert gap > 1e-6, (what, gap)


def check_band(engine, L, S):
    t = engine.pf_banded_times()
    assert t["band"] == min(S, L), (t, L, S)
    assert 1 <= t["attempts"] <= MAX_ATTEMPTS, t
    return t


# ---- degenerate bands ----

def check_degenerate_bands(engine, oracle):
    for L in (1, 4, 5, 6, 57):
        s = rand_seq(np.random.default_rng(100 + L), L)
        for S in sorted({1, 4, 5, 6, max(1, L - 1), L, 3 * L}):
            with model(engine, oracle, S=S):
                ref = oracle.pf(s, want_bpp=True)
                nothing_to_excuse(ref["bpp"], "L=%d S=%d" % (L, S))
                got = engine.pf_banded(s)
                assert_close(got, ref, "L=%d S=%d" % (L, S), ref["bpp"])
                check_band(engine, L, S)
                if S < 5:  # a pair needs three unpaired bases inside: nothing pairs
                    assert got["dG"] == 0 and got["centroid"] == "." * L, (L, S, got)


# ---- a band that is live up to its edge, against the cubic reference in long double ----

def assert_live_edge(ref, L, S):
    """the reference itself depends on the band's last diagonal and on the record's end, and on nothing past the band"""
    bpp = ref["bpp"]
    P = np.maximum(bpp, bpp.T)[1:L + 1, 1:L + 1]
    edge = float(np.diagonal(P, S - 1).max()) if S - 1 < L else 0.0
    end = float(np.triu(P)[:, L - 6:].max())
    print("p on the band's last diagonal: %.4f; closing in the last 6 nt: %.4f" % (edge, end))
    assert edge > 0.5, edge
    assert end > 0.5, end
    assert S >= L or float(np.triu(P, S).max()) == 0.0
    nothing_to_excuse(bpp)


def kind_params(kind):
    return short_hairpin_params() if kind == "multiloop_rich" else None


_LIVE = {}  # (kind, L, S) -> the sequence live_edge_record settled on, found once per session


def planted_edge_candidates(kind, L, S):
    """test_banded_fold.edge_record's construction under the seeds after the ones it tries itself: a `kind` record with a
    G/C helix whose outer pair is S - 1 wide and a hairpin closing 3 nt before the record's end"""
    fill = {"random": rand_seq, "hairpin_rich": hairpin_rich, "multiloop_rich": multiloop_rich}[kind]
    for seed in range(16, 32):
        rng = np.random.default_rng(1000 * S + L + 100000 * seed)
        s = fill(rng, L)
        n = min(12, (S - 8) // 2)
        a = max(3, min(L // 5, L - S - 25))
        mid = s[a + n + 4:a + S - n - 4]
        s = s[:a - 3] + "AAA" + "G" * n + "AAAA" + mid + "AAAA" + "C" * n + "AAA" + s[a + S + 3:]
        st = rand_seq(rng, 8, "GC")
        s = s[:L - 22] + st + "GAAA" + st[::-1].translate(COMP) + "AA"
        assert len(s) == L
        yield s


def live_edge_record(oracle, kind, L, S):
    """-> (seq, ref): edge_record(kind, L, S) and its cubic reference under span S where that reference is live at the
    band's edge in the ensemble too (assert_live_edge: the MFE structure's edge pair can have p < 0.5); else the first of
    planted_edge_candidates whose reference is.  The search looks at the reference only."""
    p = kind_params(kind) or params.default_params()
    if (kind, L, S) in _LIVE:
        s = _LIVE[kind, L, S]
        return s, cubic_reference(oracle, s, p, span=S)

    def candidates():
        yield edge_record(oracle, kind, L, S)[0]
        yield from planted_edge_candidates(kind, L, S)

    for s in candidates():
        ref = cubic_reference(oracle, s, p, span=S)
        try:
            assert_live_edge(ref, L, S)
        except AssertionError:
            continue
        _LIVE[kind, L, S] = s
        return s, ref
    raise AssertionError("no seed gave a record whose ensemble reaches the band's last diagonal: %r" % ((kind, L, S),))


def check_edge_record(engine, oracle, kind, L, S):
    s, ref = live_edge_record(oracle, kind, L, S)
    p = kind_params(kind)
    assert_live_edge(ref, L, S)
    with model(engine, oracle, p, S):
        assert_close(engine.pf_banded(s), ref, "%s %d/%d" % (kind, L, S), ref["bpp"])
        check_band(engine, L, S)


def check_multiloop_edge(engine, oracle, L, S):
    s, _, _ = multiloop_edge_record(oracle, L, S)
    p = multiloop_params()
    ref = cubic_reference(oracle, s, p, span=S)
    assert_live_edge(ref, L, S)
    with model(engine, oracle, p, S):
        assert_close(engine.pf_banded(s), ref, "multiloop edge %d/%d" % (L, S), ref["bpp"])
        check_band(engine, L, S)


# ---- against pf_long under the same span ----

def check_equal_to_pf_long(engine, L, S):
    """free and constrained ('< > x ( )': marked_record) ensembles of an L-nt record under span S"""
    engine.set_max_bp_span(S)
    try:
        s = rand_seq(np.random.default_rng(L + S), L)
        ref = engine.pf_long(s)
        assert ref["centroid"].count("(") > L // 20
        assert_close(engine.pf_banded(s), ref, "free %d/%d" % (L, S))
        check_band(engine, L, S)
        s2, cons = marked_record(L, S, L + S + 1)
        assert set("x<>()") <= set(cons)
        ref = engine.pf_long(s2, cons)
        got = engine.pf_banded(s2, cons)
        assert_close(got, ref, "constrained %d/%d" % (L, S))
        assert all(got["centroid"][k] == "." for k, ch in enumerate(cons) if ch == "x")
    finally:
        engine.set_max_bp_span(0)


def check_equal_to_pf_long_loaded(engine, L, S, seed):
    """under whatever parameter set is resident"""
    s = rand_seq(np.random.default_rng(seed), L)
    engine.set_max_bp_span(S)
    try:
        assert_close(engine.pf_banded(s), engine.pf_long(s), "seed %d, %d/%d" % (seed, L, S))
    finally:
        engine.set_max_bp_span(0)


def alphabet_record(L, seed):
    """-> (raw, codes): runs of N, lowercase and T; and the same record as code bytes 0..4"""
    rng = np.random.default_rng(seed)
    s = rand_seq(rng, L)
    for k in rng.choice(L - 100, 8, replace=False):
        n = int(rng.integers(3, 40))
        s = s[:k] + "N" * n + s[k + n:]
    raw = "".join((ch if ch != "U" or rng.random() < 0.5 else "T") for ch in s)
    raw = "".join((ch.lower() if rng.random() < 0.3 else ch) for ch in raw)
    assert len(raw) == L and set(raw) == set("ACGUTNacgutn")
    return raw, bytes("NACGU".index(ch) for ch in raw.upper().replace("T", "U"))


def check_alphabet(engine, L, S):
    raw, codes = alphabet_record(L, S)
    engine.set_max_bp_span(S)
    try:
        ref = engine.pf_long(raw)
        a, b = engine.pf_banded(raw), engine.pf_banded(codes)
        assert_close(a, ref, "alphabet %d/%d" % (L, S))
        assert a == b
    finally:
        engine.set_max_bp_span(0)


def check_span_not_below_length(engine, L=433):
    """S >= L (B = L: the whole triangle in banded storage) against pf_long without a span"""
    s = rand_seq(np.random.default_rng(L), L)
    engine.set_max_bp_span(0)
    ref = engine.pf_long(s)
    try:
        for S in (L, 1000):
            engine.set_max_bp_span(S)
            assert_close(engine.pf_banded(s), ref, "S=%d >= L=%d" % (S, L))
            check_band(engine, L, S)
    finally:
        engine.set_max_bp_span(0)


# ---- hints, determinism ----

def check_hints(engine, L, S):
    """no hint, the MFE, 0 and three times the MFE: the same ensemble to the bar, within the attempts"""
    s = rand_seq(np.random.default_rng(7 * L + S), L)
    engine.set_max_bp_span(S)
    try:
        e, _ = engine.fold_banded(s, structure=False)
        assert e < 0
        ref = engine.pf_long(s, mfe_hint=e) if L <= _lib.SF_MAX_LONG else None
        first = None
        for hint in (None, e, 0, 3 * e):
            got = engine.pf_banded(s, mfe_hint=hint)
            t = check_band(engine, L, S)
            print("hint %s:" % hint, t)
            assert t["launches"] >= t["attempts"] * min(S, L)
            first = first or got
            assert_close(got, first, "hint %s against no hint" % hint)
            if ref is not None:
                assert_close(got, ref, "hint %s against pf_long" % hint)
    finally:
        engine.set_max_bp_span(0)


def check_twice(engine, L, S):
    s = rand_seq(np.random.default_rng(L - S), L)
    engine.set_max_bp_span(S)
    try:
        a = engine.pf_banded(s)
        b = engine.pf_banded(s)
        assert a == b  # bit-identical doubles and strings
        assert a["centroid"].count("(") > L // 20
    finally:
        engine.set_max_bp_span(0)


# ---- records built from blocks ----

_blocks = {}  # (flanked sequence, constraint, S) -> oracle.pf of the block, computed once per session


def block_pf(oracle, seq, cons, S):
    """oracle.pf of one flanked block under span S (set by the caller), cached by sequence"""
    key = (seq, cons, S)
    if key not in _blocks:
        r = oracle_pf(oracle, seq, cons, want_bpp=True)
        nothing_to_excuse(r["bpp"], "block of %d nt" % len(seq))
        _blocks[key] = {k: r[k] for k in KEYS + ("centroid",)}
    return _blocks[key]


def joined_record(oracle, blocks, S, last_cons=None):
    """-> (seq, cons, ref, lnz): the blocks joined by S N; ref = the record's exact dict under max_bp_span = S from the
    oracle's folds of the blocks, each with one flanking N on each inner side; lnz[b] = ln Z of block b.  last_cons: a
    constraint for the last block (the record's constraint is dots before it), else cons is None."""
    seq = ("N" * S).join(blocks)
    ref = dict(dG=0.0, mean_bp_dist=0.0, centroid_dist=0.0)
    cens, lnz = [], []
    oracle.set_max_bp_span(S)
    try:
        for b, blk in enumerate(blocks):
            left = "N" if b > 0 else ""
            right = "N" if b < len(blocks) - 1 else ""
            bc = None
            if last_cons is not None and b == len(blocks) - 1:
                bc = "." * len(left) + last_cons
            r = block_pf(oracle, left + blk + right, bc, S)
            for key in KEYS:
                ref[key] += r[key]
            cens.append(r["centroid"][len(left):len(left) + len(blk)])
            lnz.append(-r["dG"] / KT37)
    finally:
        oracle.set_max_bp_span(0)
    ref["centroid"] = ("." * S).join(cens)
    assert len(ref["centroid"]) == len(seq)
    cons = None if last_cons is None else "." * (len(seq) - len(last_cons)) + last_cons
    return seq, cons, ref, lnz


def heterogeneous_record(oracle, S, n_each=10, block=300, pool=3, seed=5):
    """n_each G/C-only blocks followed by n_each A/U-only blocks of `block` nt, drawn from `pool` sequences of each kind"""
    rng = np.random.default_rng(seed)
    gc = [rand_seq(rng, block, "GC") for _ in range(pool)]
    au = [rand_seq(rng, block, "AU") for _ in range(pool)]
    blocks = [gc[k % pool] for k in range(n_each)] + [au[k % pool] for k in range(n_each)]
    return joined_record(oracle, blocks, S) + ([len(b) for b in blocks],)


def single_scale_excess(lens, lnz, S):
    """min over lns of max_j |c(j) - j lns|, c(j) the running ln Z at the block boundaries j: how far the best single
    per-nucleotide scale leaves q5 from 1 somewhere along the record (in e-folds); a lower bound (the grid's step times
    the record's length is taken off)"""
    js, cs, j, c = [0], [0.0], 0, 0.0
    for b, (n, z) in enumerate(zip(lens, lnz)):
        js.append(j)   # the block's first nucleotide: ln Z as after the block before
        cs.append(c)
        j += n
        c += z
        js.append(j)
        cs.append(c)
        j += S
    js, cs = np.array(js, dtype=float), np.array(cs)
    grid = np.linspace(0.0, 3.0, 30001)
    worst = np.abs(cs[None, :] - grid[:, None] * js[None, :]).max(axis=1)
    return float(worst.min()) - 1e-4 * js.max()


def check_heterogeneous(engine, oracle, S):
    """the record a single-scale exterior loop cannot hold: the exact blockwise sums and the joined centroids"""
    seq, _, ref, lnz, lens = heterogeneous_record(oracle, S)
    excess = single_scale_excess(lens, lnz, S)
    print("%d nt; ln Z = %.1f; the best single scale is off by e^%.0f somewhere" % (len(seq), sum(lnz), excess))
    assert excess > 750, excess
    with model(engine, oracle, S=S):
        got = engine.pf_banded(seq)
        print(engine.pf_banded_times())
        assert_close(got, ref, "heterogeneous")
        check_band(engine, len(seq), S)


def pooled_record(oracle, L, S, seed, lo=150, hi=250, pool=12, constrained=False):
    """-> (seq, cons, ref): a record of exactly L nt of hairpin_rich blocks of lo..hi nt (the last two a little longer
    where the length demands it) drawn from `pool` sequences, joined by S N.  constrained: the last block carries 'x < >'
    marks and a bracket pair that closes within its last 6 nt (long_util.block_constraint), and its reference comes from
    oracle_pf under that constraint."""
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
        assert set("x()") <= set(last_cons)
    seq, cons, ref, _ = joined_record(oracle, blocks, S, last_cons)
    assert len(seq) == L
    return seq, cons, ref


def check_pooled_record(engine, oracle, L, S, seed, constrained):
    seq, cons, ref = pooled_record(oracle, L, S, seed, constrained=constrained)
    if constrained:  # the bracket pair's partners lie at the record's end
        assert cons.rfind(")") >= L - 7 and cons.rfind("(") >= L - S - 1
    with model(engine, oracle, S=S):
        e, _ = engine.fold_banded(seq, cons, structure=False)
        got = engine.pf_banded(seq, cons, mfe_hint=e)
        print("%d nt:" % L, engine.pf_banded_times())
        assert_close(got, ref, "%d nt, S=%d" % (L, S))
        check_band(engine, L, S)
        assert engine.pf_banded_bytes(L, S) == banded_pf_bytes(L, S)


# ---- the C ABI ----

def check_errors(engine):
    lib = engine.lib
    s = b"ACGU" * 10
    out = np.frombuffer(b"\x5a" * 24, dtype=np.float64).copy()
    cen = np.frombuffer(b"?" * 41, dtype=np.uint8).copy()
    a = [out[0:].ctypes.data, out[1:].ctypes.data, cen.ctypes.data, out[2:].ctypes.data]

    def untouched():
        return out.tobytes() == b"\x5a" * 24 and cen.tobytes() == b"?" * 41

    engine.set_max_bp_span(0)
    assert lib.sf_pf_banded(s, 40, None, None, *a) == -3  # no span set
    with pytest.raises(_lib.ScanFoldHipError):
        engine.pf_banded("ACGU" * 10)
    engine.set_max_bp_span(20)
    try:
        assert lib.sf_pf_banded(s, 0, None, None, *a) == -3
        assert lib.sf_pf_banded(s, _lib.SF_MAX_BANDED + 1, None, None, *a) == -3  # (the length argument only)
        assert lib.sf_pf_banded(None, 40, None, None, *a) == -3
        assert lib.sf_pf_banded(s, 40, b"((((" + b"." * 36, None, *a) == -9
        assert lib.sf_pf_banded(s, 40, b"))" + b"." * 36 + b"((", None, *a) == -9
        n = ctypes.c_size_t(5)
        assert lib.sf_pf_banded_bytes(0, 20, ctypes.byref(n)) == -3
        assert lib.sf_pf_banded_bytes(_lib.SF_MAX_BANDED + 1, 20, ctypes.byref(n)) == -3
        assert lib.sf_pf_banded_bytes(40, 0, ctypes.byref(n)) == -3
        assert lib.sf_pf_banded_bytes(40, 20, None) == -3
        assert n.value == 5
        for L, S in ((40, 20), (40, 400), (29903, 600), (_lib.SF_MAX_BANDED, 600)):
            assert engine.pf_banded_bytes(L, S) == banded_pf_bytes(L, S)
        # an unbalanced row at 40 000 nt, its stray bracket past position 32 767: refused before any launch
        L = 40000
        seq = rand_seq(np.random.default_rng(40), L).encode()
        cons = bytearray(b"." * L)
        cons[100], cons[110], cons[39000] = ord("("), ord(")"), ord("(")
        launches = engine.pf_banded_times()["launches"]
        big = ctypes.create_string_buffer(b"#" * L, L + 1)
        assert lib.sf_pf_banded(seq, L, bytes(cons), None, a[0], a[1], ctypes.addressof(big), a[3]) == -9
        assert engine.pf_banded_times()["launches"] == launches
        assert untouched() and big.raw == b"#" * L + b"\0"
        # a hint so far off (ln s = -8e5 per nucleotide) that six steps of 700 / B do not bring the tables back into FP64:
        # SF_ERR_RANGE, every attempt used and reported, no output written
        absurd = np.array([2000000000], dtype=np.int32)
        assert lib.sf_pf_banded(s, 40, None, absurd.ctypes.data, *a) == -11
        t = engine.pf_banded_times()
        assert t["attempts"] == MAX_ATTEMPTS and t["band"] == 20 and t["launches"] == MAX_ATTEMPTS * 20, t
        assert untouched()
        assert lib.sf_pf_banded(s, 40, None, None, None, None, None, None) == 0  # every output may be NULL
        assert untouched()
        assert lib.sf_pf_banded(s, 40, None, None, *a) == 0
        assert np.isfinite(out).all() and cen[40] == 0 and set(bytes(cen[:40])) <= set(b"().")
    finally:
        engine.set_max_bp_span(0)


# ---- the combined driver ----

def run_global_ensemble_banded(engine, tmp_path, monkeypatch, seq, S, scan_args):
    """scanfold.main(... --global_refold --global_span S --global_ensemble_banded) on one record: the ensemble file holds
    three records whose numbers are Engine.pf_banded's (each fold's MFE as hint), formatted as --global_ensemble formats
    them with " span=S" on the header lines, and the engine's state is as before."""
    monkeypatch.setattr(_lib, "_engine", engine)
    monkeypatch.chdir(tmp_path)
    (tmp_path / "in.fa").write_text(">recE\n" + seq + "\n")
    engine.set_max_bp_span(0)
    engine.md_span = 0
    params0 = engine.params
    assert sfd.main(["in.fa"] + scan_args + ["--name", "ge", "--dont_extract", "--global_refold", "--global_span", str(S),
                                             "--global_ensemble_banded"]) == 0
    assert engine.max_bp_span == 0 and engine.md_span == 0 and engine.params is params0
    base = [f[:-len(".out")] for f in os.listdir(tmp_path) if f.endswith(".out")][0]
    want = ""
    engine.set_max_bp_span(S)
    try:
        for label, tag in (("Global Full", None), ("Refolded with -1 constraints", "-1"), ("Refolded with -2 constraints", "-2")):
            cons = None
            if tag:
                cons = (tmp_path / (base + ".ScanFold." + tag + ".dbn")).read_text().split("\n")[2]
                cons = cons + "." * (len(seq) - len(cons))
            e, _ = engine.fold_banded(seq, cons, structure=False)
            r = engine.pf_banded(seq, cons, mfe_hint=e)
            want += (">ge\t%s ensemble dG=%.2f ED=%.2f centroid distance=%.2f span=%d\n%s\n%s\n"
                     % (label, r["dG"], r["mean_bp_dist"], r["centroid_dist"], S, seq, r["centroid"]))
    finally:
        engine.set_max_bp_span(0)
    assert (tmp_path / (base + ".AllDBN-global_refold.ensemble.txt")).read_text() == want
    assert want.count("(") > 0


def check_driver_refusals(tmp_path, monkeypatch):
    """--global_ensemble_banded without --global_span or --global_refold, or together with --global_ensemble: refused
    before anything is scanned or written"""
    monkeypatch.chdir(tmp_path)
    (tmp_path / "r.fa").write_text(">r\n" + "ACGU" * 100 + "\n")
    scan = ["r.fa", "-w", "120", "-s", "100", "-r", "3"]
    for extra in (["--global_refold", "--global_ensemble_banded"],
                  ["--global_span", "150", "--global_ensemble_banded"],
                  ["--global_ensemble_banded"],
                  ["--global_refold", "--global_span", "150", "--global_ensemble", "--global_ensemble_banded"]):
        with pytest.raises(ValueError, match="--global_"):
            sfd.main(scan + extra)
    assert os.listdir(tmp_path) == ["r.fa"]
