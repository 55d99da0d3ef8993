"""Whole-record folds under a base-pair span in banded tables (sf_fold_banded) on the MI355X: against the oracle on records
whose band is live up to its last diagonal, against sf_fold_long under the same span at 3 000 nt (free, constrained, type-7
pair on the band's edge, randomised and rescaled parameter sets, the alphabet of a record, energy only), and past the old
length limit on span-separated records of 40 000 and 70 000 nt whose exact answer the oracle gives block by block
(long_util.separated_record; bracket partners past 32 767 and past 65 535).  Always == on energy and structure.  Helpers and
the checks shared with the emulation are in test_banded_fold.py."""
import numpy as np
import pytest

from scanfold_amd import _lib, params
from long_util import formed_type7, hairpin_rich, lengths_summing_to, rand_seq, separated_record
import test_banded_fold as tb
from test_gpu_long_fold import model_at

pytestmark = pytest.mark.gpu

SPANS = [30, 33, 64, 65, 129, 400]


def test_degenerate_bands(gpu_engine, oracle):
    tb.check_degenerate_bands(gpu_engine, oracle)


@pytest.mark.parametrize("S", SPANS)
@pytest.mark.parametrize("L", [433, 1200])
@pytest.mark.parametrize("kind", ["random", "hairpin_rich", "multiloop_rich"])
def test_live_band_equals_oracle(gpu_engine, oracle, kind, L, S):
    tb.check_edge_record(gpu_engine, oracle, kind, L, S)


@pytest.mark.parametrize("S", SPANS)
def test_multiloop_closed_at_the_band_edge(gpu_engine, oracle, S):
    tb.check_multiloop_edge(gpu_engine, oracle, 433, S)


@pytest.mark.parametrize("S", [100, 401, 1000])
def test_equal_to_fold_long(gpu_engine, S):
    tb.check_equal_to_fold_long(gpu_engine, 3000, S)


@pytest.mark.parametrize("S", [100, 401, 1000])
def test_equal_to_fold_long_under_other_parameter_sets(gpu_engine, oracle, S):
    """params.random_params(3), and a set with enthalpies rescaled to 25 C"""
    s = rand_seq(np.random.default_rng(3000 + S), 3000)
    try:
        gpu_engine.load_params(params.random_params(3))
        gpu_engine.set_max_bp_span(S)
        assert gpu_engine.fold_banded(s) == gpu_engine.fold_long(s)
    finally:
        gpu_engine.set_max_bp_span(0)
        gpu_engine.load_params(params.default_params())
    with model_at(gpu_engine, oracle, 25.0):
        try:
            gpu_engine.set_max_bp_span(S)
            assert gpu_engine.fold_banded(s) == gpu_engine.fold_long(s)
        finally:
            gpu_engine.set_max_bp_span(0)


@pytest.mark.parametrize("S", [100, 401, 1000])
def test_alphabet_equal_to_fold_long(gpu_engine, S):
    """runs of N, lowercase, T, and the same record as code bytes 0..4"""
    rng = np.random.default_rng(S)
    s = rand_seq(rng, 3000)
    for k in rng.choice(2900, 8, replace=False):
        n = int(rng.integers(3, 40))
        s = s[:k] + "N" * n + s[k + n:]
    raw = "".join((ch if ch != "U" or rng.random() < 0.5 else "T") for ch in s)
    raw = "".join((ch.lower() if rng.random() < 0.3 else ch) for ch in raw)
    assert len(raw) == 3000 and set(raw) == set("ACGUTNacgutn")
    codes = bytes("NACGU".index(ch) for ch in raw.upper().replace("T", "U"))
    gpu_engine.set_max_bp_span(S)
    try:
        ref = gpu_engine.fold_long(raw)
        assert gpu_engine.fold_banded(raw) == ref
        assert gpu_engine.fold_banded(codes) == ref
    finally:
        gpu_engine.set_max_bp_span(0)


def past_the_limit(gpu_engine, oracle, L, kind, seed, outer_pair):
    S = 150
    lens = lengths_summing_to(np.random.default_rng(L), L, S, 150, 400)
    nb = len(lens)
    seq, cons, e, db = separated_record(oracle, lens, kind, S, seed, cons_blocks=(0, nb // 2, nb - 1), outer_pair=outer_pair)
    assert len(seq) == L
    t7 = formed_type7(seq, cons, db)
    assert any(j + 1 >= L - 7 for _, j in t7)  # the last block's type-7 pair forms: int32 partners at the record's end
    with tb.model(gpu_engine, oracle, S=S):
        assert gpu_engine.fold_banded(seq, cons) == (e, db)
        t = gpu_engine.fold_banded_times()
        assert t["band"] == S and t["fill_launches"] <= t["band"]
        assert gpu_engine.fold_banded_bytes(L, S) == tb.banded_bytes(L, S)


@pytest.mark.parametrize("L,kind,seed,outer_pair", [(40000, "N", 43, False), (40000, "x", 41, True), (70000, "N", 70, False),
                                                    (70000, "x", 71, False)])
def test_separated_records_past_the_old_limit(gpu_engine, oracle, L, kind, seed, outer_pair):
    """seeds on which the oracle's fold of the last block forms its type-7 pair"""
    past_the_limit(gpu_engine, oracle, L, kind, seed, outer_pair)


def test_70000_nt_without_a_constraint(gpu_engine, oracle):
    L, S = 70000, 150
    lens = lengths_summing_to(np.random.default_rng(7), L, S, 150, 400)
    seq, cons, e, db = separated_record(oracle, lens, "N", S, 70, fill=hairpin_rich)
    assert len(seq) == L and cons is None
    with tb.model(gpu_engine, oracle, S=S):
        assert gpu_engine.fold_banded(seq) == (e, db)
        assert gpu_engine.fold_banded(seq, structure=False) == (e, None)
        t = gpu_engine.fold_banded_times()
        assert t["band"] == S and t["fill_launches"] <= S and t["trace_ms"] == 0


def test_errors(gpu_engine):
    tb.check_errors(gpu_engine)


def test_rna_facade_routes_by_span(gpu_engine, monkeypatch):
    """1 700 nt: md.max_bp_span = 400 folds through fold_banded (band == 400), 500 stays on fold_long; the same bytes"""
    tb.check_facade_routing(gpu_engine, monkeypatch, 1700, 400, 500)


def test_combined_driver_global_span_40000_nt(gpu_engine, oracle, tmp_path, monkeypatch):
    L, S = 40000, 150
    lens = lengths_summing_to(np.random.default_rng(4), L, S, 150, 400)
    seq, cons, e, db = separated_record(oracle, lens, "N", S, 44, fill=hairpin_rich)
    assert cons is None and len(seq) == L > _lib.SF_MAX_LONG

    def expected(c):
        return (e, db) if c is None else tb.blockwise_fold(oracle, seq, c, lens, S)

    tb.run_global_span(gpu_engine, oracle, tmp_path, monkeypatch, seq, S,
                       ["-w", "120", "-s", "60", "-r", "5", "--type", "mono", "--seed", "3"], expected)


def test_refused_flag_combinations(tmp_path, monkeypatch):
    tb.check_refused_flag_combinations(tmp_path, monkeypatch)
