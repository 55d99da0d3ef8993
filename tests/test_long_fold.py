"""Whole-record folds past the window limit (sf_fold_long, include/scanfold_hip_long.h): the kernel source compiled for the
CPU against the oracle, the RNA facade's routing of long sequences, and the combined driver's --global_refold
(ScanFold.py:1509-1547)."""
import contextlib
import ctypes
import os
import random

import numpy as np
import pytest

from scanfold_amd import _lib, params
from scanfold_amd import RNA
from scanfold_amd import scanfold as sfd
from long_util import (PAIRS, formed_type7, hairpin_record, multiloop_rich, rand_seq, separated_record, short_hairpin_params,
                       with_oracle_constraint)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emul():
    from emul_engine import emul_engine
    e = emul_engine()
    e.load_params(params.default_params())
    return e


def planted_stem(rng, L, n_stem=12, loop_at=None):
    """a random sequence whose first and last n_stem bases form a perfect helix around the rest"""
    s = rand_seq(rng, n_stem)
    comp = s[::-1].translate(str.maketrans("ACGU", "UGCA"))
    return s + rand_seq(rng, L - 2 * n_stem) + comp


@pytest.mark.parametrize("L", [1, 4, 57, 401, 433])
def test_unconstrained_equals_oracle(emul, oracle, L):
    s = rand_seq(np.random.default_rng(100 + L), L)
    db, e = oracle.mfe(s)
    assert emul.fold_long(s) == (e, db)


def test_planted_long_range_stem(emul, oracle):
    s = planted_stem(np.random.default_rng(7), 420)
    db, e = oracle.mfe(s)
    assert emul.fold_long(s) == (e, db)
    assert db.startswith("((((") and db.endswith("))))")  # the stem spans the whole record


def constraint_string(s, rng):
    """'( ) < > x .' with one bracket pair of non-complementary bases (type 7) and one of complementary ones inside it"""
    L = len(s)
    c = ["."] * L
    for k in rng.choice(L, max(4, L // 10), replace=False):
        c[k] = "<>x"[k % 3]
    a = next(i for i in range(2, L // 4) if (s[i], s[L - 1 - i]) not in PAIRS)  # type 7
    c[a], c[L - 1 - a] = "(", ")"
    b, j = next((i, j) for i in range(a + 3, L // 2) for j in range(i + 10, min(i + 40, L - 2 - a)) if (s[i], s[j]) in PAIRS)
    c[b], c[j] = "(", ")"
    return "".join(c)


@pytest.mark.parametrize("L", [120, 433])
def test_constrained_equals_oracle(emul, oracle, L):
    rng = np.random.default_rng(30 + L)
    s = rand_seq(rng, L)
    cons = constraint_string(s, rng)
    db, e = with_oracle_constraint(oracle, cons, lambda: oracle.mfe(s))
    assert emul.fold_long(s, cons) == (e, db)
    for k, ch in enumerate(cons):
        if ch == "x":
            assert db[k] == "."


def test_span_equals_oracle(emul, oracle):
    s = planted_stem(np.random.default_rng(5), 433)
    emul.set_max_bp_span(150)
    oracle.set_max_bp_span(150)
    try:
        db, e = oracle.mfe(s)
        assert emul.fold_long(s) == (e, db)
    finally:
        emul.set_max_bp_span(0)
        oracle.set_max_bp_span(0)


@contextlib.contextmanager
def params_in(oracle, engine, p):
    oracle.set_params(p)
    engine.load_params(p)
    try:
        yield
    finally:
        oracle.set_params(params.default_params())
        engine.load_params(params.default_params())


@pytest.mark.parametrize("kind", ["N", "x"])
@pytest.mark.parametrize("short_hairpins", [False, True])
def test_separated_blocks_fold_as_the_whole_record(oracle, kind, short_hairpins):
    """The premise of long_util.separated_record, proved on every run: the oracle's fold of the whole record equals the sum
    of its block folds in energy and their join in structure, for both separator kinds, with bracket pairs (one of them
    type 7), '<' / '>' / 'x' marks inside blocks and, for 'x' separators, the bracket pair (1, L) the span forbids; with the
    default set and with multiloop-rich blocks under short_hairpin_params."""
    S = 60
    cons_blocks, outer = ((1, 4), False) if kind == "N" else ((0, 2, 4), True)
    if short_hairpins:
        oracle.set_params(short_hairpin_params())
    try:
        seq, cons, e, db = separated_record(oracle, [180, 250, 200, 190, 230], kind, S, 41, cons_blocks=cons_blocks,
                                            outer_pair=outer, fill=multiloop_rich if short_hairpins else rand_seq)
        assert len(seq) == 1290 and cons and set("()<>x") <= set(cons)
        assert formed_type7(seq, cons, db)
        oracle.set_max_bp_span(S)
        try:
            assert with_oracle_constraint(oracle, cons, lambda: oracle.mfe(seq)) == (db, e)
        finally:
            oracle.set_max_bp_span(0)
    finally:
        oracle.set_params(params.default_params())


def test_separated_record_on_the_emulated_kernel(emul, oracle):
    """sf_fold_long (CPU build) on separated records of 410 nt: three blocks, span 40, N separators without a constraint and
    'x' separators with bracket pairs, marks and the forbidden pair (1, L).  The blocks are multiloop_rich under
    short_hairpin_params, so the multiloop splits need their first and last k."""
    S = 40
    emul.set_max_bp_span(S)
    try:
        with params_in(oracle, emul, short_hairpin_params()):
            seq, cons, e, db = separated_record(oracle, [110, 120, 100], "N", S, 3, fill=multiloop_rich)
            assert cons is None and "N" * S in seq
            assert emul.fold_long(seq) == (e, db)
            seq, cons, e, db = separated_record(oracle, [110, 120, 100], "x", S, 4, cons_blocks=(0, 2), outer_pair=True,
                                                fill=multiloop_rich)
            assert formed_type7(seq, cons, db)
            assert emul.fold_long(seq, cons) == (e, db)
    finally:
        emul.set_max_bp_span(0)


@pytest.mark.parametrize("s", [401, 402, 403])
def test_hairpin_at_the_end_of_the_window_table(emul, oracle, s):
    """A hairpin of size s closed by a bracketed G-C stem: 401 is the last size of the resident model's table (hp_init), 402
    the first one the kernel reads from the host-built table of the call."""
    seq, cons, db = hairpin_record(np.random.default_rng(s), s, flank=5)
    assert len(seq) <= 433
    odb, e = with_oracle_constraint(oracle, cons, lambda: oracle.mfe(seq))
    assert odb == db
    assert emul.fold_long(seq, cons) == (e, db)


def test_bad_arguments(emul):
    lib = emul.lib
    s = b"ACGU" * 10
    e = ctypes.c_int32()
    buf = ctypes.create_string_buffer(41)
    assert lib.sf_fold_long(s, 40, b"((((" + b"." * 36, ctypes.addressof(e), ctypes.addressof(buf)) == -9
    assert lib.sf_fold_long(s, 40, b"))" + b"." * 36 + b"((", ctypes.addressof(e), ctypes.addressof(buf)) == -9
    assert lib.sf_fold_long(s, 0, None, ctypes.addressof(e), ctypes.addressof(buf)) == -3
    assert lib.sf_fold_long(s, 32768, None, ctypes.addressof(e), ctypes.addressof(buf)) == -3
    assert lib.sf_fold_long(None, 40, None, ctypes.addressof(e), ctypes.addressof(buf)) == -3
    with pytest.raises(_lib.ScanFoldHipError):
        emul.fold_long("")
    # energy only: no structure buffer
    assert lib.sf_fold_long(s, 40, None, ctypes.addressof(e), None) == 0


@pytest.mark.parametrize("L", [5, 57, 200])
def test_short_sequences_equal_the_window_entry_points(emul, L):
    rng = np.random.default_rng(60 + L)
    s = rand_seq(rng, L)
    e, db = emul.mfe_trace_batch([s])
    assert emul.fold_long(s) == (int(e[0]), db[0])
    cons = "." * L if L < 20 else constraint_string(s, rng)
    r = emul.fold_constrained([s], [cons], pf=False)
    assert emul.fold_long(s, cons) == (int(r["mfe"][0]), r["structure"][0])


def test_rna_facade_routes_long_sequences(emul, oracle, monkeypatch):
    monkeypatch.setattr(_lib, "_engine", emul)
    rng = np.random.default_rng(9)
    s = rand_seq(rng, 433)
    db, e = oracle.mfe(s)
    assert RNA.fold_compound(s).mfe() == (db, RNA._f32(e))
    cons = constraint_string(s, rng)
    db2, e2 = with_oracle_constraint(oracle, cons, lambda: oracle.mfe(s))
    fc = RNA.fold_compound(s, RNA.md())
    fc.hc_add_from_db(cons)
    assert fc.mfe() == (db2, RNA._f32(e2))
    for call in ("pf", "centroid", "mean_bp_distance"):
        with pytest.raises(NotImplementedError):
            getattr(RNA.fold_compound(s), call)()
    fc = RNA.fold_compound(s)
    fc.sc_add_SHAPE_deigan([0.5] * (len(s) + 1), 0.8, -0.2)
    with pytest.raises(NotImplementedError):
        fc.mfe()


def test_cpu_twin_engine_loads_and_refuses_long_folds():
    twin = os.path.join(ROOT, "oracle", "libscanfold_cpu.so")
    from oracle import oracle as orc
    orc.build()
    if not os.path.exists(twin):
        pytest.skip("the CPU twin of the C ABI was not built")
    eng = _lib.Engine(device=0, lib_path=twin)
    assert not eng.has_fold_long()
    with pytest.raises(_lib.ScanFoldHipError):
        eng.fold_long("ACGU" * 120)


def expected_refold(oracle, seq, name, dbn1, dbn2):
    out = ""
    db, e = oracle.mfe(seq)
    out += ">" + name + "\tGlobal Full MFE=" + str(RNA._f32(e)) + "\n" + seq + "\n" + db + "\n"
    for tag, cons in (("-1", dbn1), ("-2", dbn2)):
        cons = cons + "." * (len(seq) - len(cons))  # (the dbn files stop at the last window's end)
        db, e = with_oracle_constraint(oracle, cons, lambda: oracle.mfe(seq))
        out += ">" + name + "\tRefolded with " + tag + " constraints MFE=" + str(RNA._f32(e)) + "\n" + seq + "\n" + db + "\n"
    return out


def test_combined_driver_global_refold(emul, oracle, tmp_path, monkeypatch):
    monkeypatch.setattr(_lib, "_engine", emul)
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(12)
    seq = planted_stem(rng, 430, n_stem=10).replace("U", "T")
    (tmp_path / "in.fa").write_text(">rec1 x\n" + seq + "\n")
    args = ["in.fa", "-w", "40", "-s", "30", "-r", "3", "--type", "mono", "--seed", "2", "--name", "myrna", "--dont_extract"]
    assert sfd.main(args + ["--global_refold"]) == 0
    base = "rec1.win_40.stp_30.rnd_3.shfl_mono"
    tseq = seq.replace("T", "U")
    lines = {tag: (tmp_path / (base + ".ScanFold." + tag + ".dbn")).read_text() for tag in ("no_filter", "-1", "-2")}
    dbn1, dbn2 = (lines[t].split("\n")[2] for t in ("-1", "-2"))
    assert len(dbn1) == len(tseq) and len(dbn2) == len(tseq)
    got = (tmp_path / (base + ".AllDBN-global_refold.txt")).read_text()
    assert got == expected_refold(oracle, tseq, "myrna", dbn1, dbn2)
    assert (tmp_path / (base + ".AllDBN.txt")).read_text() == lines["no_filter"] + lines["-1"] + lines["-2"]
    assert sfd.build_parser().parse_args(["x.fa", "--dbn_file_path", "g.txt"]).dbn_file_path == "g.txt"
    # refused before the scan where no dbn files are made
    os.remove(base + ".out")
    for extra in (["-c", "0"], ["--dont_fold"]):
        with pytest.raises(ValueError):
            sfd.main(args + ["--global_refold"] + extra)
        assert not os.path.exists(base + ".out")


def test_global_refold_leaves_every_other_output_unchanged(emul, tmp_path, monkeypatch):
    """A two-record FASTA with --span, with and without --global_refold: apart from the two refold files every output file is
    byte-identical (the refold folds without the span; the motif refolds and the second record must still have it)."""
    monkeypatch.setattr(_lib, "_engine", emul)
    rng = np.random.default_rng(21)
    hp = lambda stem, loop: stem + loop + stem[::-1].translate(str.maketrans("ACGU", "UGCA"))  # noqa: E731
    # record 0: strong hairpins (motifs to extract and refold), 102 nt so that the last window (step 10) ends at 100;
    # record 1: a helix whose pairs span more than 25 nt (what --span 25 forbids in its scan)
    recs = ["".join(rand_seq(rng, 12) + hp("GGGCGCCAC", "GAAA") for _ in range(3)),
            rand_seq(rng, 40) + hp("GCGGCC", rand_seq(rng, 24)) + rand_seq(rng, 60)]
    fasta = "".join(">r%d\n%s\n" % (k, s) for k, s in enumerate(recs))
    args = ["in.fa", "-w", "40", "-s", "10", "-r", "6", "--type", "mono", "--seed", "1", "--span", "25"]
    outs = {}
    try:
        for flag in ([], ["--global_refold"]):
            d = tmp_path / ("refold" if flag else "plain")
            d.mkdir()
            (d / "in.fa").write_text(fasta)
            monkeypatch.chdir(d)
            random.seed(4)  # (the motif shuffles draw from Python's generator, unseeded upstream)
            assert sfd.main(args + flag) == 0
            outs[bool(flag)] = {f: (d / f).read_bytes() for f in os.listdir(d)}
        assert emul.max_bp_span == 25
    finally:
        emul.set_max_bp_span(0)
        emul.md_span = 0
    plain, refold = outs[False], outs[True]
    extra = sorted(set(refold) - set(plain))
    assert extra == sorted("r%d.win_40.stp_10.rnd_6.shfl_mono.%s" % (k, f) for k in (0, 1)
                           for f in ("AllDBN-global_refold.txt", "AllDBN.txt"))
    assert plain["r0.win_40.stp_10.rnd_6.shfl_mono.ExtractedStructures.gff3"].strip()  # motifs were refolded
    lines = refold["r0.win_40.stp_10.rnd_6.shfl_mono.AllDBN-global_refold.txt"].decode().split("\n")
    assert lines[1] == recs[0] and len(lines[5]) == len(recs[0])  # the whole record, past the last window
    for f in plain:
        assert refold[f] == plain[f], f


# ---- sf_fold_long and a batch of one row: dots as a constraint, NULL outputs, L = 1 (run again on the GPU in test_gpu_long_fold.py) ----

def check_a_constraint_of_dots_is_no_constraint(engine):
    """a constraint of dots folds like no constraint at all (a batch does not even set up the arrays for such a row)"""
    for L in (57, 433):
        s = rand_seq(np.random.default_rng(100 + L), L)
        assert engine.fold_long(s, "." * L) == engine.fold_long(s), L
        e, db = engine.fold_long_batch([s], ["." * L], structure=True)  # a batch of one row: the same bytes
        assert (int(e[0]), db[0]) == engine.fold_long(s), L


def check_energy_only_and_null_outputs(engine):
    s = b"ACGU" * 10
    assert engine.lib.sf_fold_long(s, 40, None, None, None) == 0  # mfe_dcal_out may be NULL too
    assert engine.fold_long_times()[2] == 0                       # no traceback, no traceback time


def check_the_shortest_records(engine, oracle):
    """L = 1: no diagonal past d = 0"""
    for L in (1, 4):
        s = rand_seq(np.random.default_rng(100 + L), L)
        db, e = oracle.mfe(s)
        assert engine.fold_long(s) == (e, db), L
        assert engine.fold_long(s, structure=False) == (e, None), L
        eb, dbb = engine.fold_long_batch([s], structure=True)
        assert (int(eb[0]), dbb[0]) == (e, db), L


def test_a_constraint_of_dots_is_no_constraint(emul):
    check_a_constraint_of_dots_is_no_constraint(emul)


def test_energy_only_and_null_outputs(emul):
    check_energy_only_and_null_outputs(emul)


def test_the_shortest_records(emul, oracle):
    check_the_shortest_records(emul, oracle)
