"""Many whole-record folds at once on the MI355X (sf_fold_long_batch) against the oracle, byte for byte: ragged batches across
the window limit, a z-score-shaped batch (a record and its shuffles) also against sf_fold_long row by row, the widest lane
groups (G = 64 past d = 2 048, late diagonals with fewer cells than a workgroup holds), chunking by the byte budget, the
resident model's state (span, randomised tables, 25 C, the alphabet), constraint rows, and what sits on it in Python:
functions.energies / rna_folder past 400 nt and the combined driver's --global_zscore."""
import os
import random

import numpy as np
import pytest

from scanfold_amd import _lib, functions, params
from scanfold_amd import scanfold as sfd
from long_util import rand_seq, with_oracle_constraint
from test_gpu_long_fold import model_at, span
import test_long_batch
from test_long_batch import expected_zscore_file, seq_bytes
from test_long_fold import constraint_string, planted_stem

pytestmark = pytest.mark.gpu


def assert_batch_equals_oracle(engine, oracle, seqs, cons=None):
    e, db = engine.fold_long_batch(seqs, cons, structure=True)
    assert e.dtype == np.int32 and len(e) == len(db) == len(seqs)
    for k, s in enumerate(seqs):
        c = None if cons is None else cons[k]
        s = s.upper().replace("T", "U")
        odb, oe = oracle.mfe(s) if c is None else with_oracle_constraint(oracle, c, lambda: oracle.mfe(s))
        assert (int(e[k]), db[k]) == (oe, odb), (k, len(s))
    return e, db


def test_ragged_batch_equals_oracle(gpu_engine, oracle):
    seqs = [rand_seq(np.random.default_rng(900 + L), L) for L in (1, 4, 57, 400, 401, 433, 640, 777)]
    e, _ = assert_batch_equals_oracle(gpu_engine, oracle, seqs)
    assert gpu_engine.fold_long_batch_times()["chunks"] == 1
    assert (gpu_engine.fold_long_batch(seqs[::-1]) == e[::-1]).all()  # energies only, the rows in another order
    assert gpu_engine.fold_long_batch_times()["trace_ms"] == 0


def test_zscore_shaped_batch(gpu_engine, oracle):
    """one 600-nt sequence and 20 dinucleotide shuffles of it, energies only: the oracle's, and sf_fold_long's per row"""
    seq = rand_seq(np.random.default_rng(600), 600)
    state = random.getstate()
    random.seed(600)
    rows = [seq] + functions.scramble(seq, 20, "di")
    random.setstate(state)
    assert len(set(rows)) == 21
    e = gpu_engine.fold_long_batch(rows)
    assert [int(v) for v in e] == [oracle.mfe(s)[1] for s in rows]
    assert [int(v) for v in e] == [gpu_engine.fold_long(s, structure=False)[0] for s in rows]


def test_widest_lane_groups(gpu_engine, oracle):
    """long_group reaches 64 lanes per cell only past d = 2 048; the last diagonals of the 2 112- and 2 050-nt rows have
    fewer cells than a workgroup holds, and the 1 300-nt row has none there.  The stems over the whole records make the
    cells of those diagonals count."""
    seqs = [planted_stem(np.random.default_rng(2112), 2112), planted_stem(np.random.default_rng(2050), 2050),
            rand_seq(np.random.default_rng(1300), 1300)]
    _, db = assert_batch_equals_oracle(gpu_engine, oracle, seqs)
    for k in (0, 1):
        assert db[k].startswith("((((") and db[k].endswith("))))")


def test_chunking_by_the_byte_budget(gpu_engine):
    seqs = [rand_seq(np.random.default_rng(450 + k), 450) for k in range(5)]
    whole_e, whole_db = gpu_engine.fold_long_batch(seqs, structure=True)
    assert gpu_engine.fold_long_batch_times()["chunks"] == 1
    try:
        gpu_engine.set_long_batch_bytes(2 * seq_bytes(450))
        e, db = gpu_engine.fold_long_batch(seqs, structure=True)
        assert gpu_engine.fold_long_batch_times()["chunks"] == 3
        assert (e == whole_e).all() and db == whole_db
    finally:
        gpu_engine.set_long_batch_bytes(0)
    for k in (0, 4):
        assert gpu_engine.fold_long(seqs[k]) == (int(whole_e[k]), whole_db[k])


def test_span_across_a_planted_stem(gpu_engine, oracle):
    seqs = [planted_stem(np.random.default_rng(21), 600), planted_stem(np.random.default_rng(22), 450)]
    with span(gpu_engine, oracle, 150):
        assert_batch_equals_oracle(gpu_engine, oracle, seqs)
    assert oracle.mfe(seqs[0])[0].startswith("((((")  # (without the span the stem over the record forms)


def test_randomised_parameter_set(gpu_engine, oracle):
    p = params.random_params(3)
    try:
        oracle.set_params(p)
        gpu_engine.load_params(p)
        assert_batch_equals_oracle(gpu_engine, oracle, [rand_seq(np.random.default_rng(6 + L), L) for L in (600, 450, 512)])
    finally:
        gpu_engine.load_params(params.default_params())
        oracle.set_params(params.default_params())


def test_rescaled_temperature(gpu_engine, oracle):
    with model_at(gpu_engine, oracle, 25.0):
        assert_batch_equals_oracle(gpu_engine, oracle, [rand_seq(np.random.default_rng(25 + L), L) for L in (450, 555)])


def test_alphabet(gpu_engine, oracle):
    """runs of N, lowercase and T, in a batch with a plain row"""
    rng = np.random.default_rng(500)
    s = rand_seq(rng, 500)
    for k in rng.choice(440, 4, replace=False):
        n = int(rng.integers(3, 40))
        s = s[:k] + "N" * n + s[k + n:]
    raw = "".join((ch if ch != "U" or rng.random() < 0.5 else "T") for ch in s)
    raw = "".join((ch.lower() if rng.random() < 0.3 else ch) for ch in raw)
    assert len(raw) == 500 and set(raw) == set("ACGUTNacgutn")
    e, db = gpu_engine.fold_long_batch([raw, rand_seq(rng, 450)], structure=True)
    odb, oe = oracle.mfe(raw.upper().replace("T", "U"))
    assert (int(e[0]), db[0]) == (oe, odb)


def test_constraint_rows_at_1100_nt(gpu_engine, oracle):
    rng = np.random.default_rng(1100)
    seqs = [rand_seq(rng, 1100) for _ in range(3)]
    cons = constraint_string(seqs[0], rng)
    assert set("()<>x") <= set(cons)
    e, db = gpu_engine.fold_long_batch(seqs, [cons, "." * 1100, None], structure=True)
    assert (int(e[0]), db[0]) == with_oracle_constraint(oracle, cons, lambda: oracle.mfe(seqs[0]))[::-1]
    for k in (1, 2):
        assert (int(e[k]), db[k]) == oracle.mfe(seqs[k])[::-1]
    with pytest.raises(_lib.ScanFoldHipError):
        gpu_engine.fold_long_batch(seqs, [cons, None, "(" + "." * 1099])


def test_energies_and_rna_folder_past_the_window_limit(gpu_engine, oracle, monkeypatch):
    monkeypatch.setattr(_lib, "_engine", gpu_engine)
    rng = np.random.default_rng(45)
    seqs = [rand_seq(rng, 120), rand_seq(rng, 450), "", rand_seq(rng, 120), rand_seq(rng, 401), rand_seq(rng, 120),
            rand_seq(rng, 450)]
    want = [0.0 if not s else float(np.float32(oracle.mfe(s)[1] / 100)) for s in seqs]
    assert functions.energies(seqs) == want
    s500 = rand_seq(rng, 500)
    assert functions.rna_folder((s500, 37, "rnafold")) == float(np.float32(oracle.mfe(s500)[1] / 100))


def test_combined_driver_global_zscore(gpu_engine, oracle, tmp_path, monkeypatch):
    monkeypatch.setattr(_lib, "_engine", gpu_engine)
    seq = planted_stem(np.random.default_rng(16), 450, n_stem=10)
    args = ["in.fa", "-w", "60", "-s", "40", "-r", "6", "--type", "di", "--seed", "5", "--name", "whole", "--span", "50",
            "--dont_extract"]
    outs = {}
    try:
        for flag in ([], ["--global_zscore"]):
            d = tmp_path / ("z" if flag else "plain")
            d.mkdir()
            (d / "in.fa").write_text(">rec1\n" + seq + "\n")
            monkeypatch.chdir(d)
            random.seed(98)
            state = random.getstate()
            assert sfd.main(args + flag) == 0
            assert random.getstate() == state
            assert gpu_engine.max_bp_span == 50 and gpu_engine.params.temperature == 37.0
            outs[bool(flag)] = {f: (d / f).read_bytes() for f in os.listdir(d)}
    finally:
        gpu_engine.set_max_bp_span(0)
        gpu_engine.md_span = 0
    base = "rec1.win_60.stp_40.rnd_6.shfl_di"
    plain, z = outs[False], outs[True]
    assert sorted(set(z) - set(plain)) == [base + ".global_zscore.txt"]
    for f in plain:
        assert z[f] == plain[f], f
    assert z[base + ".global_zscore.txt"].decode() == expected_zscore_file(oracle, seq, "whole", 6, "di", 5)


# ---- the single call beside the batch: test_long_batch's checks at the product's lane budgets ----

def test_a_single_call_is_one_chunk_under_any_byte_budget(gpu_engine):
    test_long_batch.check_a_single_call_is_one_chunk_under_any_byte_budget(gpu_engine)


def test_the_two_time_records_stay_apart(gpu_engine):
    test_long_batch.check_the_two_time_records_stay_apart(gpu_engine)
