"""The whole-record partition function on the MI355X (sf_pf_long) at the default lane budget: against the oracle up to 520 nt
(its outside pass is O(n^4)), against oracle.pf_cubic in long double without a span at 777 to 2 112 nt (the lengths that
reach 16, 32 and 64 lanes per cell), against the window entry points at short lengths, against block-built records whose exact
answer the oracle gives block by block (long_pf_util.block_record) at ~9 kb, twice for bit-identical results, and one
29 903-nt record whose tables pass 2^31 bytes.  Then the window kernels, to show that no state was left behind."""
import numpy as np
import pytest

from scanfold_amd import params
import pf_util
from long_pf_util import (KEYS, assert_carries_weight, assert_close, block_record, cubic_reference, forget_cubic_references,
                          gc_only, nested_record, oracle_pf)  # (forget_cubic_references: an autouse fixture)
from long_util import hairpin_record, hairpin_rich, pair_table, rand_seq
from test_gpu_long_fold import assert_windows_equal_oracle, balanced, model_at, span, synthetic_set, viral_like
import test_long_pf
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


# ---- whole records past 520 nt without a span, against oracle.pf_cubic in long double (long_pf_util.cubic_reference) ----
# The lane-group sizes below are those of a 256-CU device (pfl_group: G doubles while 32 G <= max(64, d) and 2 G cells fit
# the budget of 262 144 lanes): 16 lanes per cell from d = 512, 32 from d = 1 024, 64 from d = 2 048.

def nested_case(oracle, L, seed):
    """nested_record(L, seed) with its reference under the default set, proven on the CPU to depend on the long diagonals"""
    seq, outer, branches = nested_record(np.random.default_rng(seed), L)
    ref = cubic_reference(oracle, seq, params.default_params())
    assert_carries_weight(ref, outer, branches, L)
    return seq, ref, outer


@pytest.mark.parametrize("L,seed", [(777, 1), (1100, 3), (1100, 5)])
def test_nested_record_equals_cubic_reference(gpu_engine, oracle, L, seed):
    """777 nt: 16 lanes per cell on 265 diagonals; 1 100 nt: 32 lanes on 76 diagonals."""
    seq, ref, _ = nested_case(oracle, L, seed)
    assert_close(gpu_engine.pf_long(seq), ref, "nested %d/%d" % (L, seed), ref["bpp"])
    print("nested %d:" % L, gpu_engine.pf_long_times())


def test_nested_record_of_2112_nt_twice(gpu_engine, oracle):
    """64 lanes per cell on the top 64 diagonals, which have 1..64 cells: the last block of those launches is partly groups
    without a cell.  Two runs bit for bit."""
    seq, ref, _ = nested_case(oracle, 2112, 1)
    a = gpu_engine.pf_long(seq)
    print("nested 2112:", gpu_engine.pf_long_times())
    b = gpu_engine.pf_long(seq)
    assert_close(a, ref, "nested 2112", ref["bpp"])
    assert a == b


def test_stem_spanning_1500_nt(gpu_engine, oracle):
    """the whole-record fold suite's record (test_gpu_long_fold.test_stems_spanning_1500_nt), for the partition function"""
    rng = np.random.default_rng(1)
    s = rand_seq(rng, 100) + planted_stem(rng, 1500, n_stem=14) + rand_seq(rng, 60)
    ref = cubic_reference(oracle, s, params.default_params())
    assert ref["centroid"][100] == "(" and ref["centroid"][1599] == ")"
    assert_close(gpu_engine.pf_long(s), ref, "stem over 1500", ref["bpp"])


def test_constrained_nested_record(gpu_engine, oracle):
    seq, _, _ = nested_case(oracle, 1100, 3)
    cons = constraint_string(seq, np.random.default_rng(33))
    assert set("x<>()") <= set(cons)
    ref = cubic_reference(oracle, seq, params.default_params(), cons=cons)
    got = gpu_engine.pf_long(seq, cons)
    assert_close(got, ref, "constrained 1100", ref["bpp"])
    assert all(got["centroid"][k] == "." for k, ch in enumerate(cons) if ch == "x")


def test_span_that_cuts_through_live_cells(gpu_engine, oracle):
    seq, free, outer = nested_case(oracle, 1100, 3)
    ref = cubic_reference(oracle, seq, params.default_params(), span=400)
    pt = pair_table(ref["centroid"])
    assert all(pt.get(i) != j for i, j in outer) and all(abs(j - i) < 400 for i, j in pt.items())  # the outer stem is gone
    assert ref["centroid"] != free["centroid"]
    with span(gpu_engine, oracle, 400):
        assert_close(gpu_engine.pf_long(seq), ref, "span 400", ref["bpp"])


def test_nested_record_under_random_parameters(gpu_engine, oracle):
    seq, _, _ = nested_record(np.random.default_rng(3), 1100)
    p = params.random_params(3)
    ref = cubic_reference(oracle, seq, p)
    with params_in(oracle, gpu_engine, p):
        assert_close(gpu_engine.pf_long(seq), ref, "random_params(3) 1100", ref["bpp"])


def set_at(T):
    return params.default_params() if T == 37.0 else synthetic_set().at_temperature(T)


@pytest.mark.parametrize("T", [25.0, 50.0])
def test_nested_record_at_rescaled_temperatures(gpu_engine, oracle, T):
    seq, _, _ = nested_record(np.random.default_rng(3), 1100)
    ref = cubic_reference(oracle, seq, set_at(T))
    with model_at(gpu_engine, oracle, T):
        assert_close(gpu_engine.pf_long(seq), ref, "%g C 1100" % T, ref["bpp"])


@pytest.mark.parametrize("T", [37.0, 25.0, 50.0])
def test_hairpins_past_the_window_table(gpu_engine, oracle, T):
    """hairpin_record at loop sizes around SF_MAX_W + 1 = 401, where the kernel changes from the resident hairpin table to
    the one the call builds on the host from lxc, hairpin[30] and kT of the current slot, and at 1 000.  The reference
    forms the closing pair, so the loop's weight is in every output; up to 403 the O(n^4) oracle.pf gives a second opinion."""
    p = set_at(T)
    with model_at(gpu_engine, oracle, T):
        for s in (399, 400, 401, 402, 403, 1000):
            seq, cons, db = hairpin_record(np.random.default_rng(s), s)
            ref = cubic_reference(oracle, seq, p, cons=cons)
            assert ref["centroid"][34] == "(" and ref["centroid"][35 + s] == ")", (s, T)  # the pair that closes the loop
            got = gpu_engine.pf_long(seq, cons)
            assert_close(got, ref, "hairpin %d at %g C" % (s, T), ref["bpp"])
            if s <= 403:
                second = oracle_pf(oracle, seq, cons, want_bpp=True)
                assert_close(got, second, "hairpin %d at %g C, oracle.pf" % (s, T), second["bpp"])


def test_switching_parameter_slots(gpu_engine, oracle):
    """The loads and span changes of test_gpu_long_fold.test_switching_parameter_slots: sf_pf_long takes kT, MLbase and
    hairpin[30] from the host copy of the current slot.  Then without a span, back on the first set."""
    seq, _, _ = nested_case(oracle, 777, 1)
    a, b = params.default_params(), params.random_params(3)

    def check(p, S):
        ref = cubic_reference(oracle, seq, p, span=S)
        assert_close(gpu_engine.pf_long(seq), ref, "slot of %s, span %d" % ("a" if p is a else "b", S), ref["bpp"])

    try:
        gpu_engine.load_params(a)
        gpu_engine.set_max_bp_span(150)
        gpu_engine.load_params(b)
        check(b, 150)
        gpu_engine.set_max_bp_span(120)
        check(b, 120)
        gpu_engine.load_params(a)
        check(a, 120)
        gpu_engine.set_max_bp_span(0)
        gpu_engine.load_params(b)
        check(b, 0)
        gpu_engine.load_params(a)
        check(a, 0)
    finally:
        gpu_engine.set_max_bp_span(0)
        gpu_engine.load_params(params.default_params())


def test_alphabet(gpu_engine, oracle):
    """A nested record of 1 100 nt with runs of N, lowercase and T, as text and as codes 0..4"""
    rng = np.random.default_rng(1100)
    s, _, _ = nested_record(rng, 1100)
    for k in rng.choice(np.arange(40, 1000), 6, replace=False):
        n = int(rng.integers(3, 40))
        s = s[:k] + "N" * n + s[k + n:]
    raw = "".join((ch if ch != "U" or rng.random() < 0.5 else "T") for ch in s)
    raw = "".join((ch.lower() if rng.random() < 0.3 else ch) for ch in raw)
    assert len(raw) == 1100 and set(raw) == set("ACGUTNacgutn")
    norm = raw.upper().replace("T", "U")
    codes = bytes("NACGU".index(ch) for ch in norm)
    ref = cubic_reference(oracle, norm, params.default_params())
    a, b = gpu_engine.pf_long(raw), gpu_engine.pf_long(codes)
    assert_close(a, ref, "alphabet", ref["bpp"])
    assert a == b


def test_mfe_hint(gpu_engine, oracle):
    """Whatever scale the first attempt starts from, the result meets the same reference within six attempts; the true
    MFE needs one."""
    seq, ref, _ = nested_case(oracle, 1100, 3)
    e, _ = gpu_engine.fold_long(seq, structure=False)
    assert e < 0
    for hint in (None, e, 0, 3 * e):
        assert_close(gpu_engine.pf_long(seq, mfe_hint=hint), ref, "hint %s" % hint, ref["bpp"])
        t = gpu_engine.pf_long_times()
        print("hint %s:" % hint, t)
        assert 1 <= t["attempts"] <= 6
        if hint == e:
            assert t["attempts"] == 1
    assert_windows_equal_oracle(gpu_engine, oracle)


# ---- the single call beside the batch: test_long_pf's checks at the product's lane budgets ----

def test_a_constraint_of_dots_is_no_constraint(gpu_engine):
    test_long_pf.check_a_constraint_of_dots_is_no_constraint(gpu_engine)


def test_the_shortest_records(gpu_engine, oracle):
    test_long_pf.check_the_shortest_records(gpu_engine, oracle)


def test_failure_leaves_the_callers_buffers_alone(gpu_engine):
    test_long_pf.check_failure_leaves_the_callers_buffers_alone(gpu_engine)


def test_one_row_is_the_batchs_row_with_a_retry(gpu_engine):
    test_long_pf.check_one_row_is_the_batchs_row_with_a_retry(gpu_engine)
