"""Whole-record folds under a base-pair span in banded tables (sf_fold_banded, include/scanfold_hip_long.h): the kernel source
compiled for the CPU against the oracle and against sf_fold_long under the same span, always with == on energy and structure;
the RNA facade's routing rule and the combined driver's --global_span.

What runs here is sized for the emulation (every lane a fiber): records of 433 and 1 200 nt and a short list of spans, the
whole file under a minute.  The full list of spans, the 3 000-nt comparisons with sf_fold_long and the records of 40 000 and
70 000 nt (bracket partners past 32 767 and 65 535) run on the GPU in test_gpu_banded_fold.py, which shares this file's
helpers; of the records past the old limit the emulation folds only a reduced one of 2 000 nt, because 40 000 nt under span
150 are six million cells, about two minutes of fibers.

Records whose band is live up to its edge come from `edge_record`: the oracle's own fold of the record must contain a pair
of exactly j - i = S - 1 (the band's last diagonal) and a pair closing within the record's last 6 nt (the band cut by the
record's end), else the next seed is taken; `multiloop_edge_record` does the same for a multiloop closed by a pair of width
S - 1, under a parameter set that rewards multiloops.  The search looks at the oracle only."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

from scanfold_amd import _lib, params
from scanfold_amd import RNA
from scanfold_amd import scanfold as sfd
from long_util import (COMP, block_constraint, formed_type7, hairpin_rich, multiloop_rich, pair_table, rand_seq,
                       separated_record, short_hairpin_params, with_oracle_constraint)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILLS = {"random": (rand_seq, False), "hairpin_rich": (hairpin_rich, False), "multiloop_rich": (multiloop_rich, True)}


@pytest.fixture(scope="module")
def emul():
    from emul_engine import emul_engine
    e = emul_engine()
    e.load_params(params.default_params())
    return e


@contextlib.contextmanager
def model(engine, oracle, p=None, S=0):
    """parameter set p (None: the default) and base-pair span S resident on the engine and in the oracle"""
    try:
        if p is not None:
            oracle.set_params(p)
            engine.load_params(p)
        engine.set_max_bp_span(S)
        oracle.set_max_bp_span(S)
        yield
    finally:
        engine.set_max_bp_span(0)
        oracle.set_max_bp_span(0)
        if p is not None:
            engine.load_params(params.default_params())
            oracle.set_params(params.default_params())


def hairpin(rng, n):
    st = rand_seq(rng, n, "GC")
    return st + "GAAA" + st[::-1].translate(COMP)


def branches(pt, i, j):
    """the number of stems directly inside the pair (i, j) of the pair table pt"""
    n, k = 0, i + 1
    while k < j:
        if pt.get(k, -1) > k:
            n += 1
            k = pt[k] + 1
        else:
            k += 1
    return n


def multiloop_params():
    """short_hairpin_params with multiloops rewarded, so that a lone pair closes one"""
    p = short_hairpin_params()
    p.rec["MLclosing"] = -800
    p.rec["MLintern"][:] = -100
    return p


_RECORDS = {}  # (kind, L, S) -> (seq, db, e): the oracle's fold under span S, computed once per session


def edge_record(oracle, kind, L, S):
    """-> (seq, db, e): a `kind` record of L nt with a G/C helix planted so that its outer pair is S - 1 wide, and a hairpin
    closing 3 nt before the record's end; the oracle's fold under span S (and the kind's parameter set) forms a pair of width
    exactly S - 1 and a pair within the last 6 nt."""
    key = (kind, L, S)
    if key in _RECORDS:
        return _RECORDS[key]
    fill, short = FILLS[kind]
    oracle.set_params(short_hairpin_params() if short else params.default_params())
    oracle.set_max_bp_span(S)
    try:
        for seed in range(16):
            rng = np.random.default_rng(1000 * S + L + 100000 * seed)
            s = fill(rng, L)
            n = min(12, (S - 8) // 2)
            a = max(3, min(L // 5, L - S - 25))
            mid = s[a + n + 4:a + S - n - 4]
            s = s[:a - 3] + "AAA" + "G" * n + "AAAA" + mid + "AAAA" + "C" * n + "AAA" + s[a + S + 3:]
            s = s[:L - 22] + hairpin(rng, 8) + "AA"
            assert len(s) == L
            db, e = oracle.mfe(s)
            pt = pair_table(db)
            if any(j - i == S - 1 for i, j in pt.items()) and any(j > i and j >= L - 6 for i, j in pt.items()):
                _RECORDS[key] = (s, db, e)
                return _RECORDS[key]
    finally:
        oracle.set_max_bp_span(0)
        oracle.set_params(params.default_params())
    raise AssertionError("no seed gave a record whose oracle fold reaches the band's last diagonal: %r" % (key,))


def multiloop_edge_record(oracle, L, S):
    """-> (seq, db, e) under multiloop_params and span S: the oracle's fold has a multiloop closed by a pair of width S - 1"""
    key = ("multiloop_edge", L, S)
    if key in _RECORDS:
        return _RECORDS[key]
    oracle.set_params(multiloop_params())
    oracle.set_max_bp_span(S)
    try:
        for seed in range(16):
            rng = np.random.default_rng(7000 * S + L + 100000 * seed)
            s = rand_seq(rng, L)
            inner = ""
            for h, (x, y) in zip(((S - 4) // 2, S - 4 - (S - 4) // 2), ("GC", "CG")):
                n = min(10, (h - 4) // 2)
                inner += "A" + x * n + "A" * (h - 2 * n) + y * n
            a = max(3, min(L // 5 + seed, L - S - 3))
            s = s[:a - 3] + "AAAG" + inner + "CAAA" + s[a + S + 3:]
            assert len(s) == L
            db, e = oracle.mfe(s)
            pt = pair_table(db)
            if any(j - i == S - 1 and branches(pt, i, j) >= 2 for i, j in pt.items()):
                _RECORDS[key] = (s, db, e)
                return _RECORDS[key]
    finally:
        oracle.set_max_bp_span(0)
        oracle.set_params(params.default_params())
    raise AssertionError("no seed gave a multiloop closed at the band's edge: %r" % (key,))


# ---- checks shared with test_gpu_banded_fold.py ----

def check_degenerate_bands(engine, oracle):
    for L in (1, 4, 5, 6, 57):
        s = rand_seq(np.random.default_rng(100 + L), L)
        for S in sorted({1, 4, 5, 6, max(1, L - 1), L, 3 * L}):
            with model(engine, oracle, S=S):
                db, e = oracle.mfe(s)
                assert engine.fold_banded(s) == (e, db), (L, S)
                assert engine.fold_banded(s, structure=False) == (e, None), (L, S)
                t = engine.fold_banded_times()
                assert t["band"] == min(S, L) and t["fill_launches"] <= t["band"]
                if S < 5:  # a pair needs three unpaired bases inside: nothing pairs
                    assert (e, db) == (0, "." * L)


def check_edge_record(engine, oracle, kind, L, S):
    s, db, e = edge_record(oracle, kind, L, S)
    with model(engine, oracle, short_hairpin_params() if FILLS[kind][1] else None, S):
        assert engine.fold_banded(s) == (e, db)
        t = engine.fold_banded_times()
        assert t["band"] == min(S, L) and t["fill_launches"] <= t["band"]


def check_multiloop_edge(engine, oracle, L, S):
    s, db, e = multiloop_edge_record(oracle, L, S)
    with model(engine, oracle, multiloop_params(), S):
        assert engine.fold_banded(s) == (e, db)


def marked_record(L, S, seed):
    """-> (seq, cons): a random record with 'x < >' marks and a type-7 bracket pair of width S - 1 around a planted helix"""
    rng = np.random.default_rng(seed)
    return block_constraint(rand_seq(rng, L), rng, S)


def check_equal_to_fold_long(engine, L, S):
    """free and constrained folds of an L-nt record under span S: fold_banded == fold_long, byte for byte"""
    engine.set_max_bp_span(S)
    try:
        s = rand_seq(np.random.default_rng(L + S), L)
        ref = engine.fold_long(s)
        assert ref[1].count("(") > L // 10
        assert engine.fold_banded(s) == ref
        assert engine.fold_banded(s, structure=False) == (ref[0], None)
        assert engine.fold_banded_times()["trace_ms"] == 0
        for seed in range(8):  # (a record on which fold_long, the reference, forms the type-7 pair)
            s2, cons = marked_record(L, S, L + S + 1 + 1000 * seed)
            assert set("x<>()") <= set(cons)
            ref = engine.fold_long(s2, cons)
            t7 = formed_type7(s2, cons, ref[1])
            if t7:
                break
        assert t7 and all(j - i == S - 1 for i, j in t7)  # the type-7 pair lies on the band's last diagonal
        assert engine.fold_banded(s2, cons) == ref
    finally:
        engine.set_max_bp_span(0)


def check_errors(engine):
    lib = engine.lib
    s = b"ACGU" * 10
    e = ctypes.c_int32(77)
    buf = ctypes.create_string_buffer(b"#" * 40, 41)
    args = (ctypes.addressof(e), ctypes.addressof(buf))
    engine.set_max_bp_span(0)
    assert lib.sf_fold_banded(s, 40, None, *args) == -3  # no span set
    with pytest.raises(_lib.ScanFoldHipError):
        engine.fold_banded("ACGU" * 10)
    engine.set_max_bp_span(20)
    try:
        assert lib.sf_fold_banded(s, 0, None, *args) == -3
        assert lib.sf_fold_banded(s, _lib.SF_MAX_BANDED + 1, None, *args) == -3  # (the length argument only)
        assert lib.sf_fold_banded(None, 40, None, *args) == -3
        assert lib.sf_fold_banded(s, 40, b"((((" + b"." * 36, *args) == -9
        assert lib.sf_fold_banded(s, 40, b"))" + b"." * 36 + b"((", *args) == -9
        n = ctypes.c_size_t(5)
        assert lib.sf_fold_banded_bytes(0, 20, ctypes.byref(n)) == -3
        assert lib.sf_fold_banded_bytes(_lib.SF_MAX_BANDED + 1, 20, ctypes.byref(n)) == -3
        assert lib.sf_fold_banded_bytes(40, 0, ctypes.byref(n)) == -3
        assert n.value == 5
        assert engine.fold_banded_bytes(_lib.SF_MAX_BANDED, 600) == banded_bytes(_lib.SF_MAX_BANDED, 600)
        # an unbalanced row at 40 000 nt, its stray bracket past position 32 767: refused before any launch
        L = 40000
        seq = rand_seq(np.random.default_rng(40), L).encode()
        cons = bytearray(b"." * L)
        cons[100], cons[110], cons[39000] = ord("("), ord(")"), ord("(")
        big = ctypes.create_string_buffer(b"#" * L, L + 1)
        assert lib.sf_fold_banded(seq, L, bytes(cons), ctypes.addressof(e), ctypes.addressof(big)) == -9
        assert e.value == 77 and buf.raw == b"#" * 40 + b"\0" and big.raw == b"#" * L + b"\0"  # outputs untouched
        assert lib.sf_fold_banded(s, 40, None, None, None) == 0  # every output may be NULL
    finally:
        engine.set_max_bp_span(0)


def banded_bytes(L, S):
    """SF_BANDED_BYTES of include/scanfold_hip_long.h: three int32 band tables and the documented linear term"""
    B = min(S, L)
    return 12 * L * B + 75 * L + 4 * B + 153


def blockwise_fold(oracle, seq, cons, lens, S):
    """the exact fold under span S of a separated_record of block lengths `lens` (N separators of S bases) with a constraint
    whose bracket pairs stay inside the blocks: the blocks' oracle folds joined as separated_record joins them"""
    e, dbs, pos = 0, [], 0
    oracle.set_max_bp_span(S)
    try:
        for b, n in enumerate(lens):
            left, right = int(b > 0), int(b < len(lens) - 1)
            bs = seq[pos - left:pos + n + right]
            bc = "x" * left + cons[pos:pos + n] + "x" * right
            db, eb = with_oracle_constraint(oracle, bc, lambda: oracle.mfe(bs))
            e += eb
            dbs.append(db[left:len(db) - right])
            pos += n + S
    finally:
        oracle.set_max_bp_span(0)
    return e, ("." * S).join(dbs)


def run_global_span(engine, oracle, tmp_path, monkeypatch, seq, S, scan_args, expected):
    """scanfold.main(... --global_refold --global_span S) on one record; expected(cons) -> (e_dcal, db) of the record under
    the constraint line cons (None: free).  The three records are compared, and the engine's state must be as before."""
    monkeypatch.setattr(_lib, "_engine", engine)
    monkeypatch.chdir(tmp_path)
    (tmp_path / "in.fa").write_text(">recS\n" + seq + "\n")
    engine.set_max_bp_span(0)
    engine.md_span = 0
    params0 = engine.params
    assert sfd.main(["in.fa"] + scan_args + ["--name", "gs", "--dont_extract", "--global_refold", "--global_span", str(S)]) == 0
    assert engine.max_bp_span == 0 and engine.md_span == 0 and engine.params is params0
    base = [f[:-len(".out")] for f in os.listdir(tmp_path) if f.endswith(".out")][0]
    want = ""
    for label, tag in (("Global Full", None), ("Refolded with -1 constraints", "-1"), ("Refolded with -2 constraints", "-2")):
        cons = None
        if tag:
            cons = (tmp_path / (base + ".ScanFold." + tag + ".dbn")).read_text().split("\n")[2]
            cons = cons + "." * (len(seq) - len(cons))
        e, db = expected(cons)
        want += ">gs\t%s MFE=%s span=%d\n%s\n%s\n" % (label, str(RNA._f32(e)), S, seq, db)
    assert (tmp_path / (base + ".AllDBN-global_refold.txt")).read_text() == want


def check_refused_flag_combinations(tmp_path, monkeypatch):
    """--global_ensemble / --global_zscore with --global_span on a record past SF_MAX_LONG: refused before anything is scanned"""
    monkeypatch.chdir(tmp_path)
    (tmp_path / "big.fa").write_text(">big\n" + "ACGU" * (_lib.SF_MAX_LONG // 4 + 1) + "\n")
    args = ["big.fa", "-w", "120", "-s", "100", "-r", "3", "--global_refold", "--global_span", "150"]
    for extra in ("--global_ensemble", "--global_zscore"):
        with pytest.raises(ValueError, match="--global_span"):
            sfd.main(args + [extra])
    with pytest.raises(ValueError, match="--global_span"):
        sfd.main(["big.fa", "--global_span", "150"])  # needs --global_refold
    assert [f for f in os.listdir(tmp_path)] == ["big.fa"]


# ---- on the emulation ----

def test_degenerate_bands(emul, oracle):
    check_degenerate_bands(emul, oracle)


@pytest.mark.parametrize("kind,L,S", [("random", 433, 30), ("hairpin_rich", 433, 65), ("multiloop_rich", 433, 33),
                                      ("multiloop_rich", 433, 129), ("hairpin_rich", 1200, 64), ("random", 433, 400)])
def test_live_band_equals_oracle(emul, oracle, kind, L, S):
    check_edge_record(emul, oracle, kind, L, S)


@pytest.mark.parametrize("S", [30, 64])
def test_multiloop_closed_at_the_band_edge(emul, oracle, S):
    check_multiloop_edge(emul, oracle, 433, S)


@pytest.mark.parametrize("S", [40, 101])
def test_equal_to_fold_long(emul, S):
    check_equal_to_fold_long(emul, 433, S)


def test_separated_record_reduced(emul, oracle):
    """2 000 nt, span 60, 'x' separators, marks and type-7 pairs in the first and the last block, the pair (1, L) the span
    forbids: the reduced form of the GPU file's records of 40 000 and 70 000 nt"""
    S = 60
    seq, cons, e, db = separated_record(oracle, [150, 200, 180, 170, 160, 190, 150, 140, 180, 60], "x", S, 11,
                                        cons_blocks=(0, 9), outer_pair=True)
    assert len(seq) == 2120 and formed_type7(seq, cons, db)
    with model(emul, oracle, S=S):
        assert emul.fold_banded(seq, cons) == (e, db)
        t = emul.fold_banded_times()
        assert t["band"] == S and t["fill_launches"] <= S
        assert emul.fold_banded_bytes(len(seq), S) == banded_bytes(len(seq), S)


def test_errors(emul):
    check_errors(emul)


def test_cpu_twin_has_no_banded_fold():
    twin = os.path.join(ROOT, "oracle", "libscanfold_cpu.so")
    from oracle import oracle as orc
    orc.build()
    if not os.path.exists(twin):
        pytest.skip("the CPU twin of the C ABI was not built")
    eng = _lib.Engine(device=0, lib_path=twin)
    assert not eng.has_fold_banded()
    with pytest.raises(_lib.ScanFoldHipError):
        eng.fold_banded("ACGU" * 120)


def check_facade_routing(engine, monkeypatch, L, S_banded, S_long):
    """4 span <= len(seq): fold_banded, the same bytes as fold_long; a wider span stays on fold_long"""
    monkeypatch.setattr(_lib, "_engine", engine)
    rng = np.random.default_rng(L)
    s, cons = block_constraint(rand_seq(rng, L), rng, S_banded)
    try:
        for S, banded in ((S_banded, True), (S_long, False)):
            engine.set_max_bp_span(7)
            engine.fold_banded("ACGUACGUACGU")  # (band = 7: only another banded fold changes it)
            m = RNA.md()
            m.max_bp_span = S
            fc = RNA.fold_compound(s, m)
            fc.hc_add_from_db(cons)
            got = fc.mfe()
            assert engine.fold_banded_times()["band"] == (S if banded else 7)
            e, db = engine.fold_long(s, cons)
            assert got == (db, RNA._f32(e))
    finally:
        engine.set_max_bp_span(0)
        engine.md_span = 0


def test_rna_facade_routes_by_span(emul, monkeypatch):
    check_facade_routing(emul, monkeypatch, 433, 100, 120)
    s = "ACGU" * 9000  # past SF_MAX_LONG without a span: refused with a clear message, nothing folded
    monkeypatch.setattr(_lib, "_engine", emul)
    with pytest.raises(ValueError, match="max_bp_span"):
        RNA.fold_compound(s).mfe()


def test_combined_driver_global_span(emul, oracle, tmp_path, monkeypatch):
    rng = np.random.default_rng(150)
    seq = hairpin_rich(rng, 600)
    S = 150

    def expected(cons):
        oracle.set_max_bp_span(S)
        try:
            db, e = with_oracle_constraint(oracle, cons, lambda: oracle.mfe(seq))
        finally:
            oracle.set_max_bp_span(0)
        return e, db

    run_global_span(emul, oracle, tmp_path, monkeypatch, seq, S, ["-w", "40", "-s", "30", "-r", "3", "--type", "mono",
                                                                  "--seed", "2"], expected)


def test_refused_flag_combinations(tmp_path, monkeypatch):
    check_refused_flag_combinations(tmp_path, monkeypatch)
