"""Many whole-record folds under a base-pair span at once (sf_fold_banded_batch) on the MI355X: the checks of
test_banded_batch.py over the full list of spans at 433 and 1 200 nt, the ragged call at spans 64 and 401 with a 3 000-nt row
and under other parameter sets, a record and its shuffles against a loop of sf_fold_banded, rows of 40 000 nt (bracket
partners past 32 767) against the oracle's block-wise answer, the promises of the four MFE entry points' one host driver, and
the combined driver's --global_zscore_span at 450 and at 40 000 nt.  Always == on energy and structure."""
import os
import random

import numpy as np
import pytest

from scanfold_amd import _lib, functions, params
from scanfold_amd import scanfold as sfd
from long_util import formed_type7, hairpin_rich, lengths_summing_to, rand_seq, separated_record
import test_banded_batch as tbb
import test_banded_fold as tb
from test_gpu_long_fold import model_at

pytestmark = pytest.mark.gpu

SPANS = [30, 33, 64, 65, 129, 400]
_PAST = {}  # the separated records of 40 000 nt, built once per session (the oracle folds ~130 blocks for each)


def record_40000(oracle, constrained):
    """-> (block lengths, seq, cons, e, db) under span 150: the records of test_gpu_banded_fold.py"""
    if constrained not in _PAST:
        L, S = 40000, 150
        if constrained:
            lens = lengths_summing_to(np.random.default_rng(L), L, S, 150, 400)
            nb = len(lens)
            rec = separated_record(oracle, lens, "N", S, 43, cons_blocks=(0, nb // 2, nb - 1))
        else:
            lens = lengths_summing_to(np.random.default_rng(4), L, S, 150, 400)
            rec = separated_record(oracle, lens, "N", S, 44, fill=hairpin_rich)
        assert len(rec[0]) == L and (rec[1] is not None) == constrained
        _PAST[constrained] = (lens,) + rec
    return _PAST[constrained]


@pytest.mark.parametrize("S", SPANS)
@pytest.mark.parametrize("L", [433, 1200])
def test_live_bands_equal_oracle(gpu_engine, oracle, L, S):
    tbb.check_oracle_rows(gpu_engine, oracle, L, S, both_models=(L == 433))


@pytest.mark.parametrize("S", [64, 401])
def test_ragged_call_equals_fold_banded(gpu_engine, S):
    tbb.check_ragged(gpu_engine, S, tbb.RAGGED + ([3000] if S == 401 else []))


@pytest.mark.parametrize("S", [64, 401])
def test_ragged_call_under_other_parameter_sets(gpu_engine, oracle, S):
    """params.random_params(3), and a set with enthalpies rescaled to 25 C"""
    try:
        gpu_engine.load_params(params.random_params(3))
        tbb.check_ragged(gpu_engine, S, default_model=False)
    finally:
        gpu_engine.load_params(params.default_params())
    with model_at(gpu_engine, oracle, 25.0):
        tbb.check_ragged(gpu_engine, S, default_model=False)


def test_a_record_and_its_shuffles(gpu_engine):
    """the z-score's batch: 21 rows of 1 200 nt against a loop of fold_banded"""
    s = hairpin_rich(np.random.default_rng(1200), 1200)
    state = random.getstate()
    random.seed(7)
    rows = [s] + functions.scramble(s, 20, "di")
    random.setstate(state)
    gpu_engine.set_max_bp_span(150)
    try:
        ref = [gpu_engine.fold_banded(x) for x in rows]
        e, db = gpu_engine.fold_banded_batch(rows, structure=True)
        assert [(int(e[k]), db[k]) for k in range(21)] == ref
        assert len(set(ref)) > 15
        t = gpu_engine.fold_banded_batch_times()
        assert t["chunks"] == 1 and t["fill_launches"] == 150
        assert [int(v) for v in gpu_engine.fold_banded_batch(rows)] == [r[0] for r in ref]
    finally:
        gpu_engine.set_max_bp_span(0)


def test_rows_past_the_old_limit(gpu_engine, oracle):
    """two rows of 40 000 nt under span 150, one with constraints in its first, middle and last block and one without, a
    500-nt row between them: the oracle's block-wise answers, in one chunk and in three"""
    S = 150
    _, s1, c1, e1, d1 = record_40000(oracle, True)
    _, s2, c2, e2, d2 = record_40000(oracle, False)
    assert any(j + 1 >= len(s1) - 7 for _, j in formed_type7(s1, c1, d1))  # int32 partners at the record's end
    mid = rand_seq(np.random.default_rng(500), 500)
    with tb.model(gpu_engine, oracle, S=S):
        dm, em = oracle.mfe(mid)
        want = [(e1, d1), (em, dm), (e2, d2)]
        e, db = gpu_engine.fold_banded_batch([s1, mid, s2], [c1, None, None], structure=True)
        assert [(int(e[k]), db[k]) for k in range(3)] == want
        t = gpu_engine.fold_banded_batch_times()
        assert t["chunks"] == 1 and t["fill_launches"] == S
        try:
            gpu_engine.set_long_batch_bytes(tb.banded_bytes(40000, S))
            e, db = gpu_engine.fold_banded_batch([s1, mid, s2], [c1, None, None], structure=True)
            assert [(int(e[k]), db[k]) for k in range(3)] == want
            t = gpu_engine.fold_banded_batch_times()
            assert t["chunks"] == 3 and t["fill_launches"] == 3 * S
        finally:
            gpu_engine.set_long_batch_bytes(0)


def test_errors(gpu_engine):
    tbb.check_errors(gpu_engine)


def test_single_call_is_one_chunk_under_any_budget(gpu_engine):
    tbb.check_single_is_one_chunk(gpu_engine)


def test_time_records_stay_apart(gpu_engine):
    tbb.check_time_records_stay_apart(gpu_engine)


def test_dots_and_one_row_batches(gpu_engine, oracle):
    tbb.check_dots_and_one_row_batches(gpu_engine, oracle)


def test_combined_driver_global_zscore_span(gpu_engine, oracle, tmp_path, monkeypatch):
    tbb.check_driver_zscore_span(gpu_engine, oracle, tmp_path, monkeypatch)


def test_global_zscore_span_refusals(tmp_path, monkeypatch):
    tbb.check_driver_refusals(tmp_path, monkeypatch)


def test_combined_driver_global_zscore_span_40000_nt(gpu_engine, oracle, tmp_path, monkeypatch):
    """past SF_MAX_LONG, where --global_zscore cannot go: the file against fold_banded's energies and zscore_function (the
    oracle's unblocked fold of 40 000 nt is too slow; fold_banded on this record is checked against its block-wise answer)"""
    S = 150
    _, seq, cons, e, db = record_40000(oracle, False)
    assert len(seq) > _lib.SF_MAX_LONG
    monkeypatch.setattr(_lib, "_engine", gpu_engine)
    monkeypatch.chdir(tmp_path)
    (tmp_path / "in.fa").write_text(">rec4\n" + seq + "\n")
    gpu_engine.set_max_bp_span(0)
    params0 = gpu_engine.params
    assert sfd.main(["in.fa", "-w", "120", "-s", "120", "-r", "3", "--type", "mono", "--seed", "3", "--global_zscore_span",
                     str(S), "--dont_fold"]) == 0
    assert gpu_engine.max_bp_span == 0 and gpu_engine.params is params0
    base = "rec4.win_120.stp_120.rnd_3.shfl_mono"
    assert sorted(os.listdir(tmp_path)) == sorted(["in.fa", base + ".out", base + ".global_zscore.txt"])
    gpu_engine.set_max_bp_span(S)
    try:
        assert gpu_engine.fold_banded(seq, structure=False)[0] == e
        want = tbb.expected_zscore_span_file(lambda s: gpu_engine.fold_banded(s, structure=False)[0], seq, "UserInput", 3,
                                             "mono", 3, S)
    finally:
        gpu_engine.set_max_bp_span(0)
    assert (tmp_path / (base + ".global_zscore.txt")).read_text() == want
