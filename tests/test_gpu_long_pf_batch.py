"""Many whole-record partition functions at once on the MI355X (sf_pf_long_batch) at the product's lane budgets: against the
oracle (oracle.pf up to 520 nt, oracle.pf_cubic in long double past it) under long_pf_util.assert_close, and with `==` on
floats and strings against sf_pf_long row by row — ragged batches in both orders, nested records at the lengths that reach
16, 32 and 64 lanes per cell (those of a 256-CU device) beside shorter rows, chunking by the byte budget,
per-row scales and retries, constraint rows, the resident model's state, and the combined driver's --global_ensemble."""
import os

import numpy as np
import pytest

from scanfold_amd import _lib, params
from scanfold_amd import scanfold as sfd
import pf_util
from long_pf_util import (KEYS, assert_carries_weight, assert_close, cubic_reference, forget_cubic_references, gc_only,
                          nested_record, oracle_pf)  # (forget_cubic_references: an autouse fixture)
from long_util import rand_seq
from test_gpu_long_fold import span
from test_long_fold import constraint_string, params_in, planted_stem
import test_long_pf_batch
from test_long_pf_batch import pf_bytes, single

pytestmark = pytest.mark.gpu


def nested_case(oracle, L, seed):
    """nested_record(L, seed) with its reference under the default set, proven on the CPU to depend on the long diagonals"""
    seq, outer, branches = nested_record(np.random.default_rng(seed), L)
    ref = cubic_reference(oracle, seq, params.default_params())
    assert_carries_weight(ref, outer, branches, L)
    return seq, ref


def constrained_nested_record(oracle):
    """the 1 100-nt constrained nested record of test_gpu_long_pf.test_constrained_nested_record"""
    seq, _, _ = nested_record(np.random.default_rng(3), 1100)
    cons = constraint_string(seq, np.random.default_rng(33))
    assert set("x<>()") <= set(cons)
    return seq, cons


def test_ragged_batch(gpu_engine, oracle):
    seqs = [rand_seq(np.random.default_rng(100 + L), L) for L in (1, 4, 57, 401, 433, 520)]
    rows = gpu_engine.pf_long_batch(seqs)
    t = gpu_engine.pf_long_batch_times()
    assert (t["chunks"], t["inside_passes"]) == (1, 1)
    for s, r in zip(seqs, rows):
        ref = oracle.pf(s, want_bpp=True)
        assert_close(r, ref, "L=%d" % len(s), ref["bpp"])
        assert single(r) == gpu_engine.pf_long(s), len(s)
        ts = gpu_engine.pf_long_times()
        assert (r["attempts"], r["lns"]) == (ts["attempts"], ts["lns"]), len(s)
    assert gpu_engine.pf_long_batch(seqs[::-1]) == rows[::-1]


def test_nested_records_beside_a_short_row(gpu_engine, oracle):
    """777 nt: 16 lanes per cell from d = 512; 1 100 nt: 32 lanes from d = 1 024; the 433-nt row has left by then.  Scales
    from the MFEs of fold_long_batch."""
    a, ref_a = nested_case(oracle, 777, 1)
    b, ref_b = nested_case(oracle, 1100, 3)
    c = rand_seq(np.random.default_rng(100 + 433), 433)
    seqs = [a, b, c]
    hints = [int(v) for v in gpu_engine.fold_long_batch(seqs)]
    rows = gpu_engine.pf_long_batch(seqs, mfe_hints=hints)
    print(gpu_engine.pf_long_batch_times(), [(r["attempts"], r["lns"]) for r in rows])
    assert_close(rows[0], ref_a, "nested 777", ref_a["bpp"])
    assert_close(rows[1], ref_b, "nested 1100", ref_b["bpp"])
    ref_c = oracle.pf(c, want_bpp=True)
    assert_close(rows[2], ref_c, "random 433", ref_c["bpp"])
    for s, h, r in zip(seqs, hints, rows):
        assert single(r) == gpu_engine.pf_long(s, mfe_hint=h), len(s)


def test_widest_lane_groups_twice(gpu_engine, oracle):
    """2 112 nt beside 1 100 nt: 64 lanes per cell on the top 64 diagonals, where only the first row is alive and its
    launches end in groups without a cell.  Two runs bit for bit."""
    a, ref_a = nested_case(oracle, 2112, 1)
    b, ref_b = nested_case(oracle, 1100, 3)
    rows = gpu_engine.pf_long_batch([a, b])
    print(gpu_engine.pf_long_batch_times(), [(r["attempts"], r["lns"]) for r in rows])
    again = gpu_engine.pf_long_batch([a, b])
    assert_close(rows[0], ref_a, "nested 2112", ref_a["bpp"])
    assert_close(rows[1], ref_b, "nested 1100", ref_b["bpp"])
    assert rows == again
    assert single(rows[0]) == gpu_engine.pf_long(a)


def test_chunking_by_the_byte_budget(gpu_engine, oracle):
    seqs = [rand_seq(np.random.default_rng(450 + k), 450) for k in range(5)]
    whole = gpu_engine.pf_long_batch(seqs)
    assert gpu_engine.pf_long_batch_times()["chunks"] == 1
    for s, r in zip(seqs, whole):
        ref = oracle.pf(s, want_bpp=True)
        assert_close(r, ref, "450", ref["bpp"])
    try:
        gpu_engine.set_long_batch_bytes(2 * pf_bytes(450))
        assert gpu_engine.pf_long_batch(seqs) == whole
        t = gpu_engine.pf_long_batch_times()
        assert (t["chunks"], t["inside_passes"]) == (3, 3)
    finally:
        gpu_engine.set_long_batch_bytes(0)
    assert gpu_engine.pf_long_batch(seqs) == whole
    assert gpu_engine.pf_long_batch_times()["chunks"] == 1  # the default budget is back


def test_every_row_has_its_own_scale(gpu_engine, oracle):
    gc = gc_only()
    s = rand_seq(np.random.default_rng(100 + 433), 433)
    e, _ = gpu_engine.fold_long(s, structure=False)
    rows = gpu_engine.pf_long_batch([gc, s], mfe_hints=[None, e])
    t = gpu_engine.pf_long_batch_times()
    a = gpu_engine.pf_long(gc)
    ta = gpu_engine.pf_long_times()
    b = gpu_engine.pf_long(s, mfe_hint=e)
    tb = gpu_engine.pf_long_times()
    print("G/C row:", ta, "random row:", tb, "batch:", t)
    assert (rows[0]["attempts"], rows[0]["lns"]) == (ta["attempts"], ta["lns"])
    assert rows[1]["attempts"] == 1 and rows[1]["lns"] == tb["lns"]
    assert t["inside_passes"] == ta["attempts"] and t["chunks"] == 1
    assert single(rows[0]) == a and single(rows[1]) == b
    for x, r in ((gc, rows[0]), (s, rows[1])):
        ref = oracle.pf(x, want_bpp=True)
        assert_close(r, ref, "scales %d" % len(x), ref["bpp"])


def test_a_row_that_repeats_leaves_the_others_alone(gpu_engine, oracle):
    """test_long_pf_batch's case: a hint thirty times the MFE puts ln Z_s ~ -29 ln Z, far below the range; the rows beside
    it are in range at once and wait."""
    rng = np.random.default_rng(77)
    seqs = [rand_seq(rng, 150), rand_seq(rng, 120), rand_seq(rng, 57)]
    e = [int(v) for v in gpu_engine.fold_long_batch(seqs)]
    hints = [30 * e[0], e[1], None]
    for order in ((0, 1, 2), (1, 2, 0)):
        rows = gpu_engine.pf_long_batch([seqs[k] for k in order], mfe_hints=[hints[k] for k in order])
        t = gpu_engine.pf_long_batch_times()
        got = {k: rows[pos] for pos, k in enumerate(order)}
        assert got[0]["attempts"] > 1 and got[1]["attempts"] == 1 and got[2]["attempts"] == 1
        assert t["inside_passes"] == got[0]["attempts"] and t["chunks"] == 1
        for k in range(3):
            assert single(got[k]) == gpu_engine.pf_long(seqs[k], mfe_hint=hints[k]), (order, k)
            ts = gpu_engine.pf_long_times()
            assert (got[k]["attempts"], got[k]["lns"]) == (ts["attempts"], ts["lns"]), (order, k)
    for k in range(3):
        ref = oracle.pf(seqs[k], want_bpp=True)
        assert_close(got[k], ref, "retry batch %d" % k, ref["bpp"])


def test_constraint_rows(gpu_engine, oracle):
    big, big_cons = constrained_nested_record(oracle)
    rng = np.random.default_rng(30 + 433)
    s = rand_seq(rng, 433)
    cons = constraint_string(s, rng)
    t, u = rand_seq(rng, 120), rand_seq(rng, 57)
    seqs, cc = [s, big, t, u], [cons, big_cons, "." * 120, None]
    rows = gpu_engine.pf_long_batch(seqs, cc)
    ref = cubic_reference(oracle, big, params.default_params(), cons=big_cons)
    assert_close(rows[1], ref, "constrained 1100", ref["bpp"])
    for k in (0, 2, 3):
        r = oracle_pf(oracle, seqs[k], None if k else cons, want_bpp=True)
        assert_close(rows[k], r, "constraint rows %d" % k, r["bpp"])
    for k in (0, 1):
        assert all(rows[k]["centroid"][x] == "." for x, ch in enumerate(cc[k]) if ch == "x")
        assert single(rows[k]) == gpu_engine.pf_long(seqs[k], cc[k])
    # an unbalanced row fails the call and nothing is written to the outputs
    with pytest.raises(_lib.ScanFoldHipError):
        gpu_engine.pf_long_batch([s, t, u], [cons, None, "((" + "." * 55])
    n, ld = 3, 433
    arr = np.zeros((n, ld), dtype=np.uint8)
    cb = np.full((n, ld), ord("."), dtype=np.uint8)
    for k, x in enumerate((s, t, u)):
        arr[k, :len(x)] = np.frombuffer(x.encode(), dtype=np.uint8)
    cb[0] = np.frombuffer(cons.encode(), dtype=np.uint8)
    cb[2, 50:53] = np.frombuffer(b".))", dtype=np.uint8)
    lens = np.array([433, 120, 57], dtype=np.int32)
    out = np.full(n * _lib.PF_LONG_ROW_DTYPE.itemsize, 0x5a, dtype=np.uint8)
    cen = np.full((n, ld + 1), ord("?"), dtype=np.uint8)
    rc = gpu_engine.lib.sf_pf_long_batch(arr.ctypes.data, n, ld, lens.ctypes.data, cb.ctypes.data, None, out.ctypes.data,
                                         cen.ctypes.data)
    assert rc == -9
    assert (out == 0x5a).all() and (cen == ord("?")).all()


def model_state_batch(engine, orc, oracle, pset, seqs, what, S=0):
    """two rows of 433 nt against orc.pf and the constrained 1 100-nt nested record against cubic_reference, under the model
    resident on `engine`; the first and the last row also equal pf_long"""
    big, big_cons = constrained_nested_record(oracle)
    rows = engine.pf_long_batch(seqs + [big], [None, None, big_cons])
    for s, r in zip(seqs, rows):
        ref = orc.pf(s, want_bpp=True)
        assert_close(r, ref, "%s, %d" % (what, len(s)), ref["bpp"])
    ref = cubic_reference(oracle, big, pset, cons=big_cons, span=S)
    assert_close(rows[2], ref, "%s, constrained 1100" % what, ref["bpp"])
    assert single(rows[0]) == engine.pf_long(seqs[0])
    assert single(rows[2]) == engine.pf_long(big, big_cons)


def test_span(gpu_engine, oracle):
    seqs = [planted_stem(np.random.default_rng(5), 433), rand_seq(np.random.default_rng(433), 433)]
    with span(gpu_engine, oracle, 150):
        model_state_batch(gpu_engine, oracle, oracle, params.default_params(), seqs, "span 150", S=150)


def test_randomised_parameter_set(gpu_engine, oracle):
    seqs = [rand_seq(np.random.default_rng(6), 433), rand_seq(np.random.default_rng(433), 433)]
    p = params.random_params(3)
    with params_in(oracle, gpu_engine, p):
        model_state_batch(gpu_engine, oracle, oracle, p, seqs, "random_params(3)")


def test_rescaled_temperature_set(gpu_engine, oracle):
    p = pf_util.cold()
    assert p.temperature == 25.0
    seqs = [rand_seq(np.random.default_rng(25), 433), rand_seq(np.random.default_rng(433), 433)]
    try:
        orc = pf_util.use(p)
        gpu_engine.load_params(p)
        model_state_batch(gpu_engine, orc, oracle, p, seqs, "25 C")
    finally:
        pf_util.use(params.default_params())
        gpu_engine.load_params(params.default_params())


def test_combined_driver_global_ensemble(gpu_engine, tmp_path, monkeypatch):
    monkeypatch.setattr(_lib, "_engine", gpu_engine)
    monkeypatch.chdir(tmp_path)
    seq = planted_stem(np.random.default_rng(12), 600, n_stem=10)
    (tmp_path / "in.fa").write_text(">rec1 x\n" + seq + "\n")
    calls = []
    real = gpu_engine.pf_long_batch
    monkeypatch.setattr(gpu_engine, "pf_long_batch", lambda rows, *a, **kw: (calls.append(len(rows)), real(rows, *a, **kw))[1])
    assert sfd.main(["in.fa", "-w", "40", "-s", "30", "-r", "3", "--type", "mono", "--seed", "2", "--name", "myrna",
                     "--dont_extract", "--global_refold", "--global_ensemble"]) == 0
    assert calls == [3]
    base = "rec1.win_40.stp_30.rnd_3.shfl_mono"
    lines = (tmp_path / (base + ".AllDBN-global_refold.ensemble.txt")).read_text().split("\n")
    assert len(lines) == 10 and lines[9] == ""
    cons = [None] + [(tmp_path / (base + ".ScanFold." + t + ".dbn")).read_text().split("\n")[2] for t in ("-1", "-2")]
    for k, c in enumerate(cons):
        c = None if c is None else c + "." * (len(seq) - len(c))
        r = gpu_engine.pf_long(seq, c, mfe_hint=gpu_engine.fold_long(seq, c, structure=False)[0])
        head, s, cen = lines[3 * k:3 * k + 3]
        assert head.startswith(">myrna\t") and s == seq and cen == r["centroid"]
        assert head.endswith("ensemble dG=%.2f ED=%.2f centroid distance=%.2f" % (r["dG"], r["mean_bp_dist"], r["centroid_dist"]))


# ---- the single call beside the batch: test_long_pf_batch's checks at the product's lane budgets ----

def test_a_single_call_is_one_chunk_under_any_byte_budget(gpu_engine):
    test_long_pf_batch.check_a_single_call_is_one_chunk_under_any_byte_budget(gpu_engine)


def test_the_two_time_records_stay_apart(gpu_engine):
    test_long_pf_batch.check_the_two_time_records_stay_apart(gpu_engine)


def test_row_state_survives_a_retry_in_the_one_row_case(gpu_engine, oracle):
    test_long_pf_batch.check_row_state_survives_a_retry_in_the_one_row_case(gpu_engine, oracle)
