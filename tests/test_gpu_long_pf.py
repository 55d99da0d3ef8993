"""The whole-record partition function on the MI355X (sf_pf_long) at the default lane budget: against the oracle up to 520 nt
(its outside pass is O(n^4)), against the window entry points at short lengths, against block-built records whose exact
answer the oracle gives block by block (long_pf_util.block_record) at ~9 kb, twice for bit-identical results, and one
29 903-nt record whose tables pass 2^31 bytes.  Then the window kernels, to show that no state was left behind."""
import numpy as np
import pytest

from scanfold_amd import params
import pf_util
from long_pf_util import KEYS, assert_close, block_record, gc_only, oracle_pf
from long_util import hairpin_rich, rand_seq
from test_gpu_long_fold import assert_windows_equal_oracle, balanced, span, viral_like
from test_long_fold import constraint_string, params_in, planted_stem

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("L", [401, 433, 520])
def test_unconstrained_equals_oracle(gpu_engine, oracle, L):
    s = rand_seq(np.random.default_rng(100 + L), L)
    ref = oracle.pf(s, want_bpp=True)
    assert_close(gpu_engine.pf_long(s), ref, "L=%d" % L, ref["bpp"])


@pytest.mark.parametrize("L", [120, 400])
def test_short_sequences_equal_the_window_entry_points(gpu_engine, L):
    rng = np.random.default_rng(60 + L)
    s = rand_seq(rng, L)
    assert_close(gpu_engine.pf_long(s), pf_util.row(gpu_engine.pf_batch([s]), 0), "pf_batch %d" % L)
    cons = constraint_string(s, rng)
    r = gpu_engine.fold_constrained([s], [cons], mfe=False)
    assert_close(gpu_engine.pf_long(s, cons), pf_util.row(r, 0), "fold_constrained %d" % L)


def test_constrained_equals_oracle(gpu_engine, oracle):
    rng = np.random.default_rng(30 + 433)
    s = rand_seq(rng, 433)
    cons = constraint_string(s, rng)
    ref = oracle_pf(oracle, s, cons, want_bpp=True)
    assert_close(gpu_engine.pf_long(s, cons), ref, "constrained", ref["bpp"])


def test_span_equals_oracle(gpu_engine, oracle):
    s = planted_stem(np.random.default_rng(5), 433)
    with span(gpu_engine, oracle, 150):
        ref = oracle.pf(s, want_bpp=True)
        assert_close(gpu_engine.pf_long(s), ref, "span 150", ref["bpp"])


def test_randomised_parameter_set(gpu_engine, oracle):
    with params_in(oracle, gpu_engine, params.random_params(3)):
        s = rand_seq(np.random.default_rng(6), 433)
        ref = oracle.pf(s, want_bpp=True)
        assert_close(gpu_engine.pf_long(s), ref, "random_params(3)", ref["bpp"])


def test_rescaled_temperature_set(gpu_engine, oracle):
    p = pf_util.cold()
    try:
        orc = pf_util.use(p)
        gpu_engine.load_params(p)
        s = rand_seq(np.random.default_rng(25), 433)
        ref = orc.pf(s, want_bpp=True)
        assert_close(gpu_engine.pf_long(s), ref, "25 C", ref["bpp"])
    finally:
        pf_util.use(params.default_params())
        gpu_engine.load_params(params.default_params())


def test_scaling_is_exercised(gpu_engine, oracle):
    s = gc_only()
    assert not oracle.pf_unscaled(s)["lnZ"] <= 709.0
    ref = oracle.pf(s, want_bpp=True)
    assert_close(gpu_engine.pf_long(s), ref, "GC 480", ref["bpp"])
    assert gpu_engine.pf_long_times()["lns"] > 0


def test_nine_kb_block_record_twice(gpu_engine, oracle):
    """25 hairpin_rich blocks of 220..330 nt joined by 150 N under span 150 (~9 kb, ln Z ~ 3 000): more than one wave of
    workgroups per diagonal.  The sums of the blocks' oracle values, and two runs bit for bit."""
    rng = np.random.default_rng(25)
    lens = [int(k) for k in rng.integers(220, 331, 25)]
    seq, ref, _ = block_record(oracle, lens, 150, 18, hairpin_rich)
    assert 8500 <= len(seq) <= 11000 and -ref["dG"] / 0.61632 > 2000
    with span(gpu_engine, oracle, 150):
        a = gpu_engine.pf_long(seq)
        print("9 kb:", gpu_engine.pf_long_times())
        b = gpu_engine.pf_long(seq)
    assert_close(a, ref, "25 blocks")
    assert a == b  # bit-identical doubles and strings
    assert_windows_equal_oracle(gpu_engine, oracle)


def test_whole_genome_length(gpu_engine, oracle):
    """29 903 nt: viral_like blocks of 220..330 nt between runs of 200 N under span 200.  The tables pass 2^31 bytes (25 GB
    in all).  Finite outputs, a balanced centroid, and dG <= MFE record-wide.  The block-sum identity on the first and last
    three blocks is checked through the only per-block quantity sf_pf_long returns, the centroid: that stretch of the
    record's centroid equals the oracle's centroid of the block folded alone (the last blocks' cells lie past 2^31 bytes
    in every table).  The repository has no marker for slow tests; this one takes as long as the O(L^3) inside pass at that
    length (DESIGN.md 4.4.1 has the measured time)."""
    L, S = 29903, 200
    rng = np.random.default_rng(L)
    lens, n = [], 0
    while True:
        k = int(rng.integers(220, 331))
        if L - n - k < 220 + S:
            lens.append(L - n)
            break
        lens.append(k)
        n += k + S
    blocks = [viral_like(k, seed=1000 + b) for b, k in enumerate(lens)]
    seq = ("N" * S).join(blocks)
    assert len(seq) == L
    with span(gpu_engine, oracle, S):
        e, _ = gpu_engine.fold_long(seq, structure=False)
        r = gpu_engine.pf_long(seq, mfe_hint=e)
        print("29 903:", gpu_engine.pf_long_times(), r["dG"], e)
        assert all(np.isfinite(r[k]) for k in KEYS)
        assert len(r["centroid"]) == L and balanced(r["centroid"]) and set(r["centroid"]) <= set("().")
        assert r["dG"] <= e * 0.01
        starts = np.concatenate([[0], np.cumsum([k + S for k in lens[:-1]])])
        for b in (0, 1, 2, len(lens) - 3, len(lens) - 2, len(lens) - 1):
            left, right = ("N" if b > 0 else ""), ("N" if b < len(lens) - 1 else "")
            o = oracle.pf(left + blocks[b] + right)
            cen = o["centroid"][len(left):len(left) + lens[b]]
            assert r["centroid"][starts[b]:starts[b] + lens[b]] == cen, b
    assert_windows_equal_oracle(gpu_engine, oracle)
