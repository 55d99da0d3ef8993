"""Whole-record folds on the MI355X (sf_fold_long) against the oracle: byte-identical structures and energies up to ~3 kb
(the oracle's O(L^3) CPU time is the limit), the window entry points at short lengths, and a 29 903-nt record (where 32-bit
table offsets would overflow) checked with the O(L) loop evaluator."""
import os

import numpy as np
import pytest

from scanfold_amd import _lib, params
from scanfold_amd import scanfold as sfd
from test_long_fold import constraint_string, expected_refold, planted_stem, rand_seq, with_oracle_constraint

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
