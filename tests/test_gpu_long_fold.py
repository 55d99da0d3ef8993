"""Whole-record folds on the MI355X (sf_fold_long) against the oracle: byte-identical structures and energies up to ~3 kb
(the oracle's O(L^3) CPU time is the limit), the window entry points at short lengths, a 29 903-nt record (where 32-bit
table offsets would overflow) checked with the O(L) loop evaluator, and span-separated records of 29 903 and SF_MAX_LONG nt
whose exact answer the oracle gives block by block (long_util.separated_record).  Also hairpins past the window table, rescaled
temperature sets, switches between the two resident parameter slots and the alphabet of a record, at lengths past SF_MAX_W."""
import contextlib
import os

import numpy as np
import pytest

from scanfold_amd import _lib, params
from scanfold_amd import scanfold as sfd
from conftest import random_seqs
from long_util import (formed_type7, hairpin_record, hairpin_rich, lengths_summing_to, multiloop_rich, separated_record,
                       short_hairpin_params, with_oracle_constraint)
from test_gpu_parity import PF_TOL
import test_long_fold
from test_long_fold import constraint_string, expected_refold, planted_stem, rand_seq

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("L", [401, 777, 1024, 2048, 3001])
def test_unconstrained_equals_oracle(gpu_engine, oracle, L):
    s = rand_seq(np.random.default_rng(200 + L), L)
    db, e = oracle.mfe(s)
    assert gpu_engine.fold_long(s) == (e, db)


@pytest.mark.parametrize("seed", [1, 2])
def test_stems_spanning_1500_nt(gpu_engine, oracle, seed):
    rng = np.random.default_rng(seed)
    s = rand_seq(rng, 100) + planted_stem(rng, 1500, n_stem=14) + rand_seq(rng, 60)
    db, e = oracle.mfe(s)
    assert gpu_engine.fold_long(s) == (e, db)


def test_constrained_equals_oracle(gpu_engine, oracle):
    rng = np.random.default_rng(15)
    s = rand_seq(rng, 1500)
    cons = constraint_string(s, rng)
    assert "<" in cons and ">" in cons and "x" in cons
    db, e = with_oracle_constraint(oracle, cons, lambda: oracle.mfe(s))
    assert gpu_engine.fold_long(s, cons) == (e, db)


def test_span_equals_oracle(gpu_engine, oracle):
    s = planted_stem(np.random.default_rng(20), 2000)
    gpu_engine.set_max_bp_span(200)
    oracle.set_max_bp_span(200)
    try:
        db, e = oracle.mfe(s)
        assert gpu_engine.fold_long(s) == (e, db)
    finally:
        gpu_engine.set_max_bp_span(0)
        oracle.set_max_bp_span(0)


def test_randomised_parameter_set(gpu_engine, oracle):
    p = params.random_params(3)
    try:
        oracle.set_params(p)
        gpu_engine.load_params(p)
        s = rand_seq(np.random.default_rng(6), 600)
        db, e = oracle.mfe(s)
        assert gpu_engine.fold_long(s) == (e, db)
    finally:
        gpu_engine.load_params(params.default_params())
        oracle.set_params(params.default_params())


@pytest.mark.parametrize("L", [1, 5, 120, 200, 400])
def test_short_sequences_equal_the_window_entry_points(gpu_engine, L):
    rng = np.random.default_rng(300 + L)
    s = rand_seq(rng, L)
    e, db = gpu_engine.mfe_trace_batch([s])
    assert gpu_engine.fold_long(s) == (int(e[0]), db[0])
    cons = "." * L if L < 20 else constraint_string(s, rng)
    r = gpu_engine.fold_constrained([s], [cons], pf=False)
    assert gpu_engine.fold_long(s, cons) == (int(r["mfe"][0]), r["structure"][0])


def viral_like(L, seed=29903):
    """seeded record of a coronavirus's length with hairpins planted every ~300 nt"""
    rng = np.random.default_rng(seed)
    out = []
    while sum(map(len, out)) < L:
        stem = rand_seq(rng, int(rng.integers(6, 12)))
        out.append(rand_seq(rng, int(rng.integers(150, 400))) + stem + "GAAA" + stem[::-1].translate(str.maketrans("ACGU", "UGCA")))
    return "".join(out)[:L]


def balanced(db):
    depth = 0
    for ch in db:
        depth += ch == "("
        depth -= ch == ")"
        if depth < 0:
            return False
    return depth == 0


def test_whole_genome_length(gpu_engine, oracle):
    L = 29903
    s = viral_like(L)
    e, db = gpu_engine.fold_long(s)
    assert len(db) == L and balanced(db) and set(db) <= set("().")
    assert oracle.eval_structure(s, db) == e
    assert e < -500 * 100  # a 30-kb record folds to several thousand kcal/mol... at least to -500
    # constrained: 'x' / '<' / '>' marks and a bracket pair across the whole record
    rng = np.random.default_rng(4)
    cons = ["."] * L
    for k in rng.choice(L, 3000, replace=False):
        cons[k] = "<>x"[k % 3]
    a, b = next((a, b) for a in range(5, 50) for b in range(L - 6, L - 50, -1) if s[a] + s[b] in ("GC", "CG", "AU", "UA"))
    cons[a], cons[b] = "(", ")"
    cons = "".join(cons)
    e2, db2 = gpu_engine.fold_long(s, cons)
    assert len(db2) == L and balanced(db2)
    for k, ch in enumerate(cons):
        if ch == "x":
            assert db2[k] == "."
    pt, stack = {}, []
    for k, ch in enumerate(db2):
        if ch == "(":
            stack.append(k)
        elif ch == ")":
            o = stack.pop()
            pt[o], pt[k] = k, o
    for k, ch in enumerate(cons):
        if ch == "<" and k in pt:
            assert pt[k] > k
        if ch == ">" and k in pt:
            assert pt[k] < k
    assert pt.get(a, b) == b and pt.get(b, a) == a  # the bracketed positions pair with each other or not at all
    oracle.set_constraint(cons)
    try:
        assert oracle.eval_structure(s, db2) == e2
    finally:
        oracle.set_constraint(None)
    assert gpu_engine.fold_long(s, cons) == (e2, db2)  # deterministic


def test_combined_driver_global_refold_2kb(gpu_engine, oracle, tmp_path, monkeypatch):
    monkeypatch.setattr(_lib, "_engine", gpu_engine)
    monkeypatch.chdir(tmp_path)
    seq = viral_like(2000, seed=8)
    (tmp_path / "in.fa").write_text(">rec2\n" + seq + "\n")
    assert sfd.main(["in.fa", "-w", "120", "-s", "10", "-r", "10", "--type", "di", "--name", "g2", "--dont_extract",
                     "--global_refold"]) == 0
    base = "rec2.win_120.stp_10.rnd_10.shfl_di"
    dbn1, dbn2 = ((tmp_path / (base + ".ScanFold." + t + ".dbn")).read_text().split("\n")[2] for t in ("-1", "-2"))
    got = (tmp_path / (base + ".AllDBN-global_refold.txt")).read_text()
    assert got == expected_refold(oracle, seq, "g2", dbn1, dbn2)
    assert os.path.exists(tmp_path / (base + ".AllDBN.txt"))


def assert_windows_equal_oracle(engine, oracle):
    """64 windows of 120 nt through the window kernels, at the bars of test_gpu_parity's traceback / partition-function test"""
    arr = random_seqs(np.random.default_rng(120), 64, 120)
    e, db = engine.mfe_trace_batch(arr)
    r = engine.pf_batch(arr)
    for k in range(len(arr)):
        s = bytes(arr[k]).decode()
        odb, oe = oracle.mfe(s)
        assert (db[k], int(e[k])) == (odb, oe)
        assert oracle.eval_structure(s, db[k]) == oe
        o = oracle.pf(s)
        assert o["centroid"] == r["centroid"][k]
        assert abs(o["dG"] - r["dG"][k]) < PF_TOL
        assert abs(o["mean_bp_dist"] - r["mean_bp_dist"][k]) < PF_TOL
        assert abs(o["centroid_dist"] - r["centroid_dist"][k]) < PF_TOL


@contextlib.contextmanager
def span(engine, oracle, S):
    engine.set_max_bp_span(S)
    oracle.set_max_bp_span(S)
    try:
        yield
    finally:
        engine.set_max_bp_span(0)
        oracle.set_max_bp_span(0)


def test_genome_length_separated_by_n_runs(gpu_engine, oracle):
    """29 903 nt: hairpin-rich blocks of 400..800 nt between runs of 200 N, span 200.  The fill still covers the whole
    triangle, so c, fML and fMLt are written past 2^31 bytes and the cells within the span are read back there.  Then the
    window kernels, to show that the long fold left no state behind."""
    L, S = 29903, 200
    lens = lengths_summing_to(np.random.default_rng(L), L, S, 400, 800)
    seq, cons, e, db = separated_record(oracle, lens, "N", S, L, fill=hairpin_rich)
    assert len(seq) == L and cons is None
    with span(gpu_engine, oracle, S):
        assert gpu_engine.fold_long(seq) == (e, db)
    assert_windows_equal_oracle(gpu_engine, oracle)


def test_max_length_separated_by_x_runs(gpu_engine, oracle):
    """SF_MAX_LONG nt: multiloop-rich blocks under short_hairpin_params (splits that need their first and last k) between
    runs of 200 bases marked 'x', span 200, with bracket pairs and marks in the first, a middle and the last block (the last
    block's type-7 pair closes at 32 760 or later) and the bracket pair (1, L) that the span forbids, which puts the int16
    bracket partners and enclosing pairs of the constraint at their limit."""
    L, S = _lib.SF_MAX_LONG, 200
    p = short_hairpin_params()
    try:
        oracle.set_params(p)
        gpu_engine.load_params(p)
        lens = lengths_summing_to(np.random.default_rng(L), L, S, 400, 800)
        seq, cons, e, db = separated_record(oracle, lens, "x", S, 5, cons_blocks=(0, len(lens) // 2, len(lens) - 1),
                                            outer_pair=True, fill=multiloop_rich)
        assert len(seq) == L and cons[0] == "(" and cons[-1] == ")"
        t7 = formed_type7(seq, cons, db)
        assert len(t7) >= 2 and any(j + 1 >= L - 7 for _, j in t7)  # (the last block's forms)
        with span(gpu_engine, oracle, S):
            assert gpu_engine.fold_long(seq, cons) == (e, db)
    finally:
        gpu_engine.load_params(params.default_params())
        oracle.set_params(params.default_params())


def synthetic_set():
    base = params.default_params()
    from par_util import par_text, synthetic_enthalpies
    return params.parse_par_text(par_text(base.rec, synthetic_enthalpies(base.rec, 5)), source="synthetic.par")


@contextlib.contextmanager
def model_at(engine, oracle, T):
    """the default set at 37 C, else a set with enthalpies rescaled to T, resident on the engine and in the oracle"""
    if T == 37.0:
        yield
        return
    pset = synthetic_set()
    try:
        engine.load_params(pset)
        engine.set_temperature(T)
        oracle.set_params(pset.at_temperature(T))
        yield
    finally:
        engine.load_params(params.default_params())
        oracle.set_params(params.default_params())


@pytest.mark.parametrize("T", [37.0, 25.0, 50.0])
def test_hairpins_past_the_window_table(gpu_engine, oracle, T):
    """A hairpin of size s closed by a bracketed G-C stem.  Up to SF_MAX_W + 1 = 401 the kernel reads the resident model's
    hp_init, past it the table the call builds on the host: against the oracle's fold up to 1 000, and the known structure
    with the loop evaluator's energy at 5 000 and 20 000."""
    with model_at(gpu_engine, oracle, T):
        for s in (399, 400, 401, 402, 403, 1000, 5000, 20000):
            seq, cons, db = hairpin_record(np.random.default_rng(s), s)
            if s <= 1000:
                odb, e = with_oracle_constraint(oracle, cons, lambda: oracle.mfe(seq))
                assert odb == db
            else:
                e = with_oracle_constraint(oracle, cons, lambda: oracle.eval_structure(seq, db))
            assert gpu_engine.fold_long(seq, cons) == (e, db), (s, T)


@pytest.mark.parametrize("T", [25.0, 50.0])
def test_rescaled_temperature_equals_oracle(gpu_engine, oracle, T):
    s = rand_seq(np.random.default_rng(int(T)), 1200)
    with model_at(gpu_engine, oracle, T):
        db, e = oracle.mfe(s)
        assert gpu_engine.fold_long(s) == (e, db)


def test_switching_parameter_slots(gpu_engine, oracle):
    """The engine keeps two parameter sets resident and switches between them; the long fold builds its hairpin table from
    the current one and must see the span patched into whichever slot becomes current."""
    rng = np.random.default_rng(31)
    s = rand_seq(rng, 1200)
    a, b = params.default_params(), params.random_params(3)

    def check(p, S):
        oracle.set_params(p)
        oracle.set_max_bp_span(S)
        db, e = oracle.mfe(s)
        assert gpu_engine.fold_long(s) == (e, db)

    try:
        gpu_engine.load_params(a)
        gpu_engine.set_max_bp_span(150)
        gpu_engine.load_params(b)
        check(b, 150)
        gpu_engine.set_max_bp_span(120)  # patches b's slot only
        check(b, 120)
        # a's slot still holds span 150, set while it was current: switching to it must patch it to the span now in force
        # (120), so 120 is the right expectation here, not 150
        gpu_engine.load_params(a)
        check(a, 120)
    finally:
        gpu_engine.set_max_bp_span(0)
        gpu_engine.load_params(params.default_params())
        oracle.set_max_bp_span(0)
        oracle.set_params(params.default_params())


def test_alphabet_and_energy_only_call(gpu_engine, oracle):
    """A 1.5-kb record with runs of N, lowercase and T, the same record as codes 0..4, and the call without traceback"""
    rng = np.random.default_rng(1500)
    s = rand_seq(rng, 1500)
    for k in rng.choice(1400, 6, replace=False):
        n = int(rng.integers(3, 40))
        s = s[:k] + "N" * n + s[k + n:]
    raw = "".join((ch if ch != "U" or rng.random() < 0.5 else "T") for ch in s)
    raw = "".join((ch.lower() if rng.random() < 0.3 else ch) for ch in raw)
    assert len(raw) == 1500 and set(raw) == set("ACGUTNacgutn")
    norm = raw.upper().replace("T", "U")
    codes = bytes("NACGU".index(ch) for ch in norm)
    db, e = oracle.mfe(norm)
    assert gpu_engine.fold_long(raw) == (e, db)
    assert gpu_engine.fold_long(codes) == (e, db)
    assert gpu_engine.fold_long(raw, structure=False) == (e, None)
    assert gpu_engine.fold_long_times()[2] == 0


# ---- the single call beside the batch: test_long_fold's checks at the product's lane budgets ----

def test_a_constraint_of_dots_is_no_constraint(gpu_engine):
    test_long_fold.check_a_constraint_of_dots_is_no_constraint(gpu_engine)


def test_energy_only_and_null_outputs(gpu_engine):
    test_long_fold.check_energy_only_and_null_outputs(gpu_engine)


def test_the_shortest_records(gpu_engine, oracle):
    test_long_fold.check_the_shortest_records(gpu_engine, oracle)
