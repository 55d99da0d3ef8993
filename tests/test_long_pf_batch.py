"""Many whole-record partition functions at once (sf_pf_long_batch, include/scanfold_hip_long.h) on the CPU build of the
kernel sources: ragged batches against the oracle and, with `==` on floats and strings, against sf_pf_long row by row; the
order of the rows and the chunking; per-row scales and their retries; constraint rows; model state; bad arguments; and
ScanFold.py's --global_ensemble on the batch.

Every expected value comes from the oracle (oracle.pf up to 520 nt, long_pf_util.cubic_reference past it) under
long_pf_util.assert_close.  The emulation pays per lane (a single 600-nt row takes seconds), so rows stay small; its lane
budgets are the small ones of the SF_EMUL build (SF_PFLONG_LANES_PER_CU, SF_PFLONGB_LANES_PER_CU), the GPU tests run the
product's."""
import ctypes
import os

import numpy as np
import pytest

from scanfold_amd import _lib, params
from scanfold_amd import scanfold as sfd
import pf_util
from long_pf_util import (KEYS, assert_carries_weight, assert_close, cubic_reference, forget_cubic_references, gc_only,
                          nested_record, oracle_pf)  # (forget_cubic_references: an autouse fixture)
from long_util import rand_seq
from test_long_fold import constraint_string, params_in, planted_stem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = [1, 4, 57, 401, 433]


def pf_bytes(L):
    """what the library counts for one row of a chunk (SF_PFLONG_BYTES, include/scanfold_hip_long.h)"""
    return 56 * (L * (L + 1) // 2) + 60 * L


def single(row):
    """the keys pf_long returns, out of one row of pf_long_batch"""
    return {k: row[k] for k in KEYS + ("centroid",)}


@pytest.fixture(scope="module")
def emul():
    from emul_engine import emul_engine
    e = emul_engine()
    e.load_params(params.default_params())
    assert e.has_pf_long_batch()
    return e


@pytest.fixture(scope="module")
def ragged(emul):
    """(sequences, rows) of the ragged batch, computed once"""
    seqs = [rand_seq(np.random.default_rng(100 + L), L) for L in RAGGED]
    rows = emul.pf_long_batch(seqs)
    t = emul.pf_long_batch_times()
    assert (t["chunks"], t["inside_passes"]) == (1, 1) and t["inside_ms"] >= 0 and t["outside_ms"] >= 0
    return seqs, rows


def test_ragged_batch_equals_oracle(oracle, ragged):
    seqs, rows = ragged
    assert len(rows) == len(seqs)
    for s, r in zip(seqs, rows):
        ref = oracle.pf(s, want_bpp=True)
        assert_close(r, ref, "L=%d" % len(s), ref["bpp"])
        assert set(r) == set(KEYS) | {"centroid", "lns", "attempts"}


def test_ragged_batch_equals_pf_long_row_by_row(emul, ragged):
    seqs, rows = ragged
    for s, r in zip(seqs, rows):
        assert single(r) == emul.pf_long(s), len(s)
        t = emul.pf_long_times()
        assert (r["attempts"], r["lns"]) == (t["attempts"], t["lns"]), len(s)


def test_reversed_batch_equals_row_for_row(emul, ragged):
    seqs, rows = ragged
    assert emul.pf_long_batch(seqs[::-1]) == rows[::-1]


def test_nested_record_beside_a_short_row(emul, oracle):
    """600 nt with live long diagonals beside 200 nt: for two thirds of the launches only the first row has cells"""
    seq, outer, branches = nested_record(np.random.default_rng(2), 600)
    ref = cubic_reference(oracle, seq, params.default_params())
    assert_carries_weight(ref, outer, branches, 600)
    short = rand_seq(np.random.default_rng(200), 200)
    rows = emul.pf_long_batch([seq, short])
    assert_close(rows[0], ref, "nested 600", ref["bpp"])
    ref2 = oracle.pf(short, want_bpp=True)
    assert_close(rows[1], ref2, "random 200", ref2["bpp"])
    assert single(rows[0]) == emul.pf_long(seq)
    assert single(rows[1]) == emul.pf_long(short)


def test_chunking_by_the_byte_budget(emul, oracle):
    seqs = [rand_seq(np.random.default_rng(150 + k), 150) for k in range(4)]
    whole = emul.pf_long_batch(seqs)
    assert emul.pf_long_batch_times()["chunks"] == 1
    for s, r in zip(seqs, whole):
        ref = oracle.pf(s, want_bpp=True)
        assert_close(r, ref, "150", ref["bpp"])
    try:
        emul.set_long_batch_bytes(2 * pf_bytes(150))
        assert emul.pf_long_batch(seqs) == whole
        t = emul.pf_long_batch_times()
        assert (t["chunks"], t["inside_passes"]) == (2, 2)
        emul.set_long_batch_bytes(pf_bytes(150) - 1)  # below one row: every chunk still holds one
        assert emul.pf_long_batch(seqs) == whole
        assert emul.pf_long_batch_times()["chunks"] == 4
    finally:
        emul.set_long_batch_bytes(0)
    assert emul.pf_long_batch(seqs) == whole
    assert emul.pf_long_batch_times()["chunks"] == 1  # the default budget is back


def test_every_row_has_its_own_scale(emul, oracle):
    """A G/C-only row without a hint (ln Z ~ 742: only the scale keeps it in range) beside a random row scaled from its MFE:
    each row has the scale and the attempts pf_long has for it alone."""
    gc = gc_only()
    s = rand_seq(np.random.default_rng(100 + 433), 433)
    e, _ = emul.fold_long(s, structure=False)
    rows = emul.pf_long_batch([gc, s], mfe_hints=[None, e])
    t = emul.pf_long_batch_times()
    a = emul.pf_long(gc)
    ta = emul.pf_long_times()
    b = emul.pf_long(s, mfe_hint=e)
    tb = emul.pf_long_times()
    print("G/C row:", ta, "random row:", tb, "batch:", t)
    assert (rows[0]["attempts"], rows[0]["lns"]) == (ta["attempts"], ta["lns"])
    assert rows[1]["attempts"] == 1 and rows[1]["lns"] == tb["lns"]
    assert t["inside_passes"] == ta["attempts"] and t["chunks"] == 1
    assert single(rows[0]) == a and single(rows[1]) == b
    for x, r in ((gc, rows[0]), (s, rows[1])):
        ref = oracle.pf(x, want_bpp=True)
        assert_close(r, ref, "scales %d" % len(x), ref["bpp"])


def test_a_row_that_repeats_leaves_the_others_alone(emul, oracle):
    """A 150-nt row whose hint is thirty times its MFE starts with ln Z_s ~ -29 ln Z, far below the range, and repeats the
    inside pass; the rows beside it are in range at once, wait, and keep their tables, scales and attempts."""
    rng = np.random.default_rng(77)
    seqs = [rand_seq(rng, 150), rand_seq(rng, 120), rand_seq(rng, 57)]
    e = [int(v) for v in emul.fold_long_batch(seqs)]
    assert e[0] < -1000
    hints = [30 * e[0], e[1], None]
    for order in ((0, 1, 2), (1, 2, 0)):
        rows = emul.pf_long_batch([seqs[k] for k in order], mfe_hints=[hints[k] for k in order])
        t = emul.pf_long_batch_times()
        got = {k: rows[pos] for pos, k in enumerate(order)}
        print(t, [r["attempts"] for r in rows])
        assert got[0]["attempts"] > 1 and got[1]["attempts"] == 1 and got[2]["attempts"] == 1
        assert t["inside_passes"] == got[0]["attempts"] and t["chunks"] == 1
        for k in range(3):
            assert single(got[k]) == emul.pf_long(seqs[k], mfe_hint=hints[k]), (order, k)
            ts = emul.pf_long_times()
            assert (got[k]["attempts"], got[k]["lns"]) == (ts["attempts"], ts["lns"]), (order, k)
    for k in range(3):
        ref = oracle.pf(seqs[k], want_bpp=True)
        assert_close(got[k], ref, "retry batch %d" % k, ref["bpp"])


def test_constraint_rows(emul, oracle):
    rng = np.random.default_rng(30 + 433)
    s = rand_seq(rng, 433)
    cons = constraint_string(s, rng)
    assert set("x<>()") <= set(cons)
    t, u = rand_seq(rng, 120), rand_seq(rng, 57)
    rows = emul.pf_long_batch([s, t, u], [cons, "." * 120, None])
    for x, c, r in ((s, cons, rows[0]), (t, None, rows[1]), (u, None, rows[2])):
        ref = oracle_pf(oracle, x, c, want_bpp=True)
        assert_close(r, ref, "constraint rows %d" % len(x), ref["bpp"])
    assert all(rows[0]["centroid"][k] == "." for k, ch in enumerate(cons) if ch == "x")
    assert single(rows[0]) == emul.pf_long(s, cons)
    # an unbalanced row fails the call and nothing is written to the outputs
    with pytest.raises(_lib.ScanFoldHipError):
        emul.pf_long_batch([s, t, u], [cons, None, "((" + "." * 55])
    n, ld = 3, 433
    arr = np.zeros((n, ld), dtype=np.uint8)
    cc = np.full((n, ld), ord("."), dtype=np.uint8)
    for k, x in enumerate((s, t, u)):
        arr[k, :len(x)] = np.frombuffer(x.encode(), dtype=np.uint8)
    cc[0] = np.frombuffer(cons.encode(), dtype=np.uint8)
    cc[2, 50:53] = np.frombuffer(b".))", dtype=np.uint8)
    lens = np.array([433, 120, 57], dtype=np.int32)
    out = np.full(n * _lib.PF_LONG_ROW_DTYPE.itemsize, 0x5a, dtype=np.uint8)
    cen = np.full((n, ld + 1), ord("?"), dtype=np.uint8)
    rc = emul.lib.sf_pf_long_batch(arr.ctypes.data, n, ld, lens.ctypes.data, cc.ctypes.data, None, out.ctypes.data, cen.ctypes.data)
    assert rc == -9
    assert (out == 0x5a).all() and (cen == ord("?")).all()


def test_span(emul, oracle):
    seqs = [planted_stem(np.random.default_rng(5), 433), rand_seq(np.random.default_rng(57), 57)]
    emul.set_max_bp_span(150)
    oracle.set_max_bp_span(150)
    try:
        rows = emul.pf_long_batch(seqs)
        for s, r in zip(seqs, rows):
            ref = oracle.pf(s, want_bpp=True)
            assert_close(r, ref, "span 150, %d" % len(s), ref["bpp"])
        assert single(rows[0]) == emul.pf_long(seqs[0])
    finally:
        emul.set_max_bp_span(0)
        oracle.set_max_bp_span(0)


def test_randomised_parameter_set(emul, oracle):
    seqs = [rand_seq(np.random.default_rng(57), 57), rand_seq(np.random.default_rng(6), 433)]
    with params_in(oracle, emul, params.random_params(3)):
        rows = emul.pf_long_batch(seqs)
        for s, r in zip(seqs, rows):
            ref = oracle.pf(s, want_bpp=True)
            assert_close(r, ref, "random_params(3), %d" % len(s), ref["bpp"])
        assert single(rows[1]) == emul.pf_long(seqs[1])


def test_rescaled_temperature_set(emul, oracle):
    p = pf_util.cold()
    assert p.temperature == 25.0
    seqs = [rand_seq(np.random.default_rng(25), 420), rand_seq(np.random.default_rng(57), 57)]
    try:
        orc = pf_util.use(p)
        emul.load_params(p)
        rows = emul.pf_long_batch(seqs)
        for s, r in zip(seqs, rows):
            ref = orc.pf(s, want_bpp=True)
            assert_close(r, ref, "25 C, %d" % len(s), ref["bpp"])
        assert single(rows[0]) == emul.pf_long(seqs[0])
    finally:
        pf_util.use(params.default_params())
        emul.load_params(params.default_params())


def test_bad_arguments_and_empty_batch(emul):
    lib = emul.lib
    arr = np.frombuffer(b"ACGU" * 20, dtype=np.uint8).reshape(2, 40).copy()
    out = np.zeros(2, dtype=_lib.PF_LONG_ROW_DTYPE)
    out["attempts"] = 777
    cen = np.full((2, 41), ord("?"), dtype=np.uint8)

    def call(seqs, n, ld, lens, o=out.ctypes.data, c=cen.ctypes.data, hints=None):
        ln = None if lens is None else np.array(lens, dtype=np.int32)
        h = None if hints is None else np.array(hints, dtype=np.int32)
        return lib.sf_pf_long_batch(seqs, n, ld, None if ln is None else ln.ctypes.data, None,
                                    None if h is None else h.ctypes.data, o, c)

    a = arr.ctypes.data
    assert call(a, 0, 40, [40, 40]) == 0
    assert call(None, 0, 0, None, None, None) == 0
    assert call(a, -1, 40, [40, 40]) == -3
    assert call(a, 2, 40, [40, 0]) == -3         # a length below 1
    assert call(a, 2, 40, [40, 41]) == -3        # a length above ld
    assert call(a, 2, 40000, [40, _lib.SF_MAX_LONG + 1]) == -3
    assert call(None, 2, 40, [40, 40]) == -3
    assert call(a, 2, 40, None) == -3
    assert (out["attempts"] == 777).all() and (cen == ord("?")).all()
    assert call(a, 2, 40, [40, 17], None, None) == 0  # every output is optional
    assert call(a, 2, 40, [40, 17], out.ctypes.data, None) == 0 and (out["attempts"] == 1).all() and (cen == ord("?")).all()
    first = out.copy()
    assert call(a, 2, 40, [40, 17], None, cen.ctypes.data) == 0
    assert bytes(cen[1, 17:18]) == b"\0" and bytes(cen[0, 40:41]) == b"\0" and set(bytes(cen[1, :17])) <= set(b"().")
    # a row without a hint among hinted ones takes the default scale
    assert call(a, 2, 40, [40, 17], hints=[_lib.SF_PF_LONG_NO_HINT, _lib.SF_PF_LONG_NO_HINT]) == 0
    assert out.tobytes() == first.tobytes()
    assert np.isfinite([out[k][f] for k in range(2) for f in ("ens_dG", "mean_bp_dist", "centroid_dist", "lns")]).all()
    with pytest.raises(_lib.ScanFoldHipError):
        emul.pf_long_batch(["ACGU", ""])
    with pytest.raises(ValueError):
        emul.pf_long_batch(["ACGU"], ["..."])
    with pytest.raises(ValueError):
        emul.pf_long_batch(["ACGU"], mfe_hints=[1, 2])
    assert emul.pf_long_batch([]) == []
    t = emul.pf_long_batch_times()
    assert (t["chunks"], t["inside_passes"]) == (0, 0)


def test_cpu_twin_engine_has_no_pf_long_batch():
    twin = os.path.join(ROOT, "oracle", "libscanfold_cpu.so")
    from oracle import oracle as orc
    orc.build()
    if not os.path.exists(twin):
        pytest.skip("the CPU twin of the C ABI was not built")
    eng = _lib.Engine(device=0, lib_path=twin)
    assert not eng.has_pf_long_batch()
    with pytest.raises(_lib.ScanFoldHipError, match="sf_pf_long_batch"):
        eng.pf_long_batch(["ACGU" * 120])
    with pytest.raises(_lib.ScanFoldHipError, match="sf_pf_long_batch"):
        eng.pf_long_batch_times()


def test_global_ensemble_runs_on_the_batch(emul, tmp_path, monkeypatch):
    """The driver's three ensembles of a record past SF_MAX_W come from ONE pf_long_batch call, and the files are byte for
    byte those of the loop over pf_long, which a library without the entry point still takes."""
    monkeypatch.setattr(_lib, "_engine", emul)
    monkeypatch.chdir(tmp_path)
    seq = planted_stem(np.random.default_rng(12), 433, n_stem=10)
    (tmp_path / "in.fa").write_text(">rec1 x\n" + seq + "\n")
    calls = []
    real = emul.pf_long_batch
    monkeypatch.setattr(emul, "pf_long_batch", lambda rows, *a, **kw: (calls.append(len(rows)), real(rows, *a, **kw))[1])
    assert sfd.main(["in.fa", "-w", "40", "-s", "30", "-r", "3", "--type", "mono", "--seed", "2", "--name", "myrna",
                     "--dont_extract", "--global_refold", "--global_ensemble"]) == 0
    assert calls == [3]
    base = "rec1.win_40.stp_30.rnd_3.shfl_mono"
    lines = (tmp_path / (base + ".AllDBN-global_refold.ensemble.txt")).read_text().split("\n")
    assert len(lines) == 10 and lines[9] == "" and lines[1] == seq
    # the same stage again as a library without the entry point runs it
    monkeypatch.setattr(emul, "has_pf_long_batch", lambda: False)
    sfd.global_refold(seq, "myrna", base, 37, "loop.txt", ensemble=True)
    assert calls == [3]
    for a, b in ((".AllDBN-global_refold.ensemble.txt", ".loop.ensemble.txt"), (".AllDBN-global_refold.txt", ".loop.txt")):
        assert (tmp_path / (base + a)).read_bytes() == (tmp_path / (base + b)).read_bytes(), a


# ---- what a single call must not share with a batch (byte budget, time records), and a retry in a batch of one row (run again on the GPU in test_gpu_long_pf_batch.py) ----

def check_a_single_call_is_one_chunk_under_any_byte_budget(engine):
    s = rand_seq(np.random.default_rng(100 + 433), 433)
    rows = [rand_seq(np.random.default_rng(100 + 57), 57)] * 5
    whole = engine.pf_long(s)
    try:
        engine.set_long_batch_bytes(1)
        assert engine.pf_long(s) == whole
        engine.pf_long_batch(rows)
        assert engine.pf_long_batch_times()["chunks"] == 5  # the setting itself still works
    finally:
        engine.set_long_batch_bytes(0)


def check_the_two_time_records_stay_apart(engine):
    a, b, c = (rand_seq(np.random.default_rng(100 + L), L) for L in (57, 120, 150))
    engine.pf_long_batch([a, b])
    batch = engine.pf_long_batch_times()
    engine.pf_long(c)
    assert engine.pf_long_batch_times() == batch
    single_times = engine.pf_long_times()
    assert set(single_times) == {"inside_ms", "outside_ms", "attempts", "lns"}
    engine.pf_long_batch([b, c, a])
    assert engine.pf_long_times() == single_times


def check_row_state_survives_a_retry_in_the_one_row_case(engine, oracle):
    """the repeating row of test_a_row_that_repeats_leaves_the_others_alone, alone and as a batch of one row: the same retries"""
    s = rand_seq(np.random.default_rng(77), 150)
    e, _ = engine.fold_long(s, structure=False)
    assert e < -1000
    got = engine.pf_long(s, mfe_hint=30 * e)
    t = engine.pf_long_times()
    assert t["attempts"] > 1
    row, = engine.pf_long_batch([s], mfe_hints=[30 * e])
    assert (t["attempts"], t["lns"]) == (row["attempts"], row["lns"])
    assert got == single(row)
    assert_close(got, engine.pf_long(s, mfe_hint=e), "wrong hint against the true one")
    assert engine.pf_long_times()["attempts"] == 1
    ref = oracle.pf(s, want_bpp=True)
    assert_close(got, ref, "wrong hint against the oracle", ref["bpp"])


def test_a_single_call_is_one_chunk_under_any_byte_budget(emul):
    check_a_single_call_is_one_chunk_under_any_byte_budget(emul)


def test_the_two_time_records_stay_apart(emul):
    check_the_two_time_records_stay_apart(emul)


def test_row_state_survives_a_retry_in_the_one_row_case(emul, oracle):
    check_row_state_survives_a_retry_in_the_one_row_case(emul, oracle)
