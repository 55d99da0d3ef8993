"""Many whole-record folds at once (sf_fold_long_batch, include/scanfold_hip_long.h) on the CPU build of the kernel sources:
ragged batches against the oracle and against sf_fold_long row by row, chunking by the byte budget, constraint rows, bad
arguments, functions.energies past the window limit and the combined driver's --global_zscore.  Every expected value comes
from oracle.mfe.  The emulated device has two compute units and a small lane budget (SF_LONGB_LANES_PER_CU under SF_EMUL),
so these batches run with the lane groups of a cell cut down, the chunking test's small ones with long_group's own."""
import os
import random
import statistics

import numpy as np
import pytest

from scanfold_amd import _lib, functions, params
from scanfold_amd import scanfold as sfd
from long_util import rand_seq, with_oracle_constraint
from test_long_fold import constraint_string, planted_stem

RAGGED = [1, 4, 57, 401, 433]


@pytest.fixture(scope="module")
def emul():
    from emul_engine import emul_engine
    e = emul_engine()
    e.load_params(params.default_params())
    return e


@pytest.fixture(scope="module")
def ragged(emul):
    """(sequences, energies, structures) of the ragged batch, folded once"""
    seqs = [rand_seq(np.random.default_rng(100 + L), L) for L in RAGGED]
    e, db = emul.fold_long_batch(seqs, structure=True)
    assert e.dtype == np.int32 and e.shape == (len(seqs),)
    return seqs, [int(v) for v in e], db


def test_ragged_batch_equals_oracle(emul, oracle, ragged):
    seqs, e, db = ragged
    for k, s in enumerate(seqs):
        odb, oe = oracle.mfe(s)
        assert (e[k], db[k]) == (oe, odb), len(s)
    assert emul.fold_long_batch_times()["chunks"] >= 1


def test_ragged_batch_equals_fold_long_row_by_row(emul, ragged):
    seqs, e, db = ragged
    for k, s in enumerate(seqs):
        assert emul.fold_long(s) == (e[k], db[k]), len(s)
    # energies only, in another order: the same numbers, no traceback time
    order = [3, 0, 4, 2, 1]
    e2 = emul.fold_long_batch([seqs[k] for k in order])
    assert [int(v) for v in e2] == [e[k] for k in order]
    assert emul.fold_long_batch_times()["trace_ms"] == 0


def seq_bytes(L):
    """what the library counts for one sequence of a chunk (include/scanfold_hip_long.h)"""
    return 12 * (L * (L + 1) // 2) + 80 * L


def test_chunking_by_the_byte_budget(emul, oracle):
    lens = [33, 120, 57, 88, 101]
    seqs = [rand_seq(np.random.default_rng(700 + L), L) for L in lens]
    whole_e, whole_db = emul.fold_long_batch(seqs, structure=True)
    assert emul.fold_long_batch_times()["chunks"] == 1
    for k, s in enumerate(seqs):
        odb, oe = oracle.mfe(s)
        assert (int(whole_e[k]), whole_db[k]) == (oe, odb)
    try:
        # any two consecutive sequences fit, no three do: (33, 120) (57, 88) (101)
        budget = max(seq_bytes(a) + seq_bytes(b) for a, b in zip(lens, lens[1:]))
        assert all(seq_bytes(a) + seq_bytes(b) + seq_bytes(c) > budget for a, b, c in zip(lens, lens[1:], lens[2:]))
        emul.set_long_batch_bytes(budget)
        e, db = emul.fold_long_batch(seqs, structure=True)
        assert emul.fold_long_batch_times()["chunks"] == 3
        assert (e == whole_e).all() and db == whole_db
        emul.set_long_batch_bytes(seq_bytes(min(lens)) - 1)  # below one sequence: every chunk still holds one
        e, db = emul.fold_long_batch(seqs, structure=True)
        assert emul.fold_long_batch_times()["chunks"] == 5
        assert (e == whole_e).all() and db == whole_db
    finally:
        emul.set_long_batch_bytes(0)
    assert (emul.fold_long_batch(seqs) == whole_e).all()
    assert emul.fold_long_batch_times()["chunks"] == 1  # the default budget is back


def test_constraint_rows(emul, oracle):
    rng = np.random.default_rng(30 + 433)
    s = rand_seq(rng, 433)
    cons = constraint_string(s, rng)  # a type-7 bracket pair, '<', '>', 'x'
    assert set("()<>x") <= set(cons)
    t, u = rand_seq(rng, 120), rand_seq(rng, 57)
    e, db = emul.fold_long_batch([s, t, u], [cons, "." * 120, None], structure=True)
    assert (int(e[0]), db[0]) == with_oracle_constraint(oracle, cons, lambda: oracle.mfe(s))[::-1]
    for k, x in ((1, t), (2, u)):
        assert (int(e[k]), db[k]) == oracle.mfe(x)[::-1]
    for k, ch in enumerate(cons):
        if ch == "x":
            assert db[0][k] == "."
    # an unbalanced row fails the call and nothing is written to the outputs
    with pytest.raises(_lib.ScanFoldHipError):
        emul.fold_long_batch([s, t, u], [cons, None, "((" + "." * 55])
    n, ld = 3, 433
    arr = np.zeros((n, ld), dtype=np.uint8)
    cc = np.full((n, ld), ord("."), dtype=np.uint8)
    for k, x in enumerate((s, t, u)):
        arr[k, :len(x)] = np.frombuffer(x.encode(), dtype=np.uint8)
    cc[0] = np.frombuffer(cons.encode(), dtype=np.uint8)
    cc[2, 50:53] = np.frombuffer(b".))", dtype=np.uint8)
    lens = np.array([433, 120, 57], dtype=np.int32)
    out = np.full(n, 12345, dtype=np.int32)
    dbuf = np.full((n, ld + 1), ord("?"), dtype=np.uint8)
    rc = emul.lib.sf_fold_long_batch(arr.ctypes.data, n, ld, lens.ctypes.data, cc.ctypes.data, out.ctypes.data, dbuf.ctypes.data)
    assert rc == -9
    assert (out == 12345).all() and (dbuf == ord("?")).all()


def test_bad_arguments_and_empty_batch(emul):
    lib = emul.lib
    arr = np.frombuffer(b"ACGU" * 20, dtype=np.uint8).reshape(2, 40).copy()
    out = np.full(2, 777, dtype=np.int32)
    dbuf = np.zeros((2, 41), dtype=np.uint8)

    def call(seqs, n, ld, lens, e):
        ln = None if lens is None else np.array(lens, dtype=np.int32)
        return lib.sf_fold_long_batch(seqs, n, ld, None if ln is None else ln.ctypes.data, None, e, dbuf.ctypes.data)

    a, o = arr.ctypes.data, out.ctypes.data
    assert call(a, 0, 40, [40, 40], o) == 0
    assert call(None, 0, 0, None, None) == 0
    assert call(a, -1, 40, [40, 40], o) == -3
    assert call(a, 2, 40, [40, 0], o) == -3       # a length below 1
    assert call(a, 2, 40, [40, 41], o) == -3      # a length above ld
    assert call(a, 2, 40000, [40, 32768], o) == -3  # a length above SF_MAX_LONG
    assert call(None, 2, 40, [40, 40], o) == -3
    assert call(a, 2, 40, None, o) == -3
    assert call(a, 2, 40, [40, 40], None) == -3
    assert (out == 777).all()
    dbuf[:] = ord("?")
    assert call(a, 2, 40, [40, 17], o) == 0 and (out != 777).all()
    assert bytes(dbuf[1, 17:18]) == b"\0"
    with pytest.raises(_lib.ScanFoldHipError):
        emul.fold_long_batch(["ACGU", ""])
    with pytest.raises(ValueError):
        emul.fold_long_batch(["ACGU"], ["..."])
    e = emul.fold_long_batch([])
    assert e.shape == (0,) and e.dtype == np.int32
    assert emul.fold_long_batch([], structure=True)[1] == []
    assert emul.fold_long_batch_times()["chunks"] == 0


def test_cpu_twin_has_no_batched_long_fold(monkeypatch):
    twin = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "libscanfold_cpu.so")
    from oracle import oracle as orc
    orc.build()
    if not os.path.exists(twin):
        pytest.skip("the CPU twin of the C ABI was not built")
    eng = _lib.Engine(device=0, lib_path=twin)
    assert not eng.has_fold_long_batch()
    with pytest.raises(_lib.ScanFoldHipError, match="sf_fold_long_batch"):
        eng.fold_long_batch(["ACGU" * 120])
    monkeypatch.setattr(_lib, "_engine", eng)
    with pytest.raises(_lib.ScanFoldHipError, match="sf_fold_long_batch"):
        functions.energies(["ACGU" * 120])
    assert functions.energies(["ACGU" * 30]) == [float(np.float32(int(eng.mfe_batch(["ACGU" * 30])[0]) / 100))]


def test_energies_routes_long_sequences(emul, oracle, monkeypatch):
    """Fails without the feature: on the parent commit energies() hands a 433-nt row to sf_mfe_batch, which refuses it."""
    monkeypatch.setattr(_lib, "_engine", emul)
    rng = np.random.default_rng(44)
    seqs = [""] + [rand_seq(rng, 120) for _ in range(3)] + [rand_seq(rng, 433) for _ in range(2)] + [rand_seq(rng, 401)]
    seqs = [seqs[k] for k in (1, 4, 0, 2, 6, 3, 5)]  # lengths 120 433 0 120 401 120 433
    calls = []
    real = emul.fold_long_batch
    monkeypatch.setattr(emul, "fold_long_batch", lambda rows, *a, **kw: (calls.append([len(r) for r in rows]), real(rows, *a, **kw))[1])
    got = functions.energies(seqs)
    assert calls == [[433, 401, 433]]  # ONE batched call for every long sequence, in order
    want = [0.0 if not s else float(np.float32(oracle.mfe(s)[1] / 100)) for s in seqs]
    assert got == want
    assert functions.rna_folder((seqs[4], 37, "rnafold")) == want[4]


def expected_zscore_file(oracle, seq, name, r, kind, seed):
    """<outname>.global_zscore.txt from the generator draws of --seed and the oracle's folds"""
    state = random.getstate()
    random.seed(seed)
    shuffles = functions.scramble(seq, r, kind)
    random.setstate(state)
    assert len(set(shuffles)) == r
    E = [float(np.float32(oracle.mfe(s)[1] / 100)) for s in [seq] + shuffles]
    row = [name, str(len(seq)), "37", str(r), kind] + [str(round(x, 2)) for x in (
        E[0], statistics.mean(E[1:]), statistics.stdev(E[1:]), functions.zscore_function(E, r), functions.pvalue_function(E, r))]
    return sfd.GLOBAL_ZSCORE_HEADER + "\t".join(row) + "\n"


def test_combined_driver_global_zscore(emul, oracle, tmp_path, monkeypatch):
    monkeypatch.setattr(_lib, "_engine", emul)
    seq = planted_stem(np.random.default_rng(13), 420, n_stem=10)
    args = ["in.fa", "-w", "40", "-s", "40", "-r", "6", "--type", "di", "--seed", "5", "--name", "whole", "--span", "50",
            "--dont_extract"]
    outs = {}
    try:
        for flag in ([], ["--global_zscore"]):
            d = tmp_path / ("z" if flag else "plain")
            d.mkdir()
            (d / "in.fa").write_text(">rec1\n" + seq.replace("U", "T") + "\n")
            monkeypatch.chdir(d)
            random.seed(99)
            state = random.getstate()
            assert sfd.main(args + flag) == 0
            assert random.getstate() == state
            assert emul.max_bp_span == 50 and emul.params.temperature == 37.0
            outs[bool(flag)] = {f: (d / f).read_bytes() for f in os.listdir(d)}
    finally:
        emul.set_max_bp_span(0)
        emul.md_span = 0
    base = "rec1.win_40.stp_40.rnd_6.shfl_di"
    plain, z = outs[False], outs[True]
    assert sorted(set(z) - set(plain)) == [base + ".global_zscore.txt"]
    assert len(plain) > 5
    for f in plain:
        assert z[f] == plain[f], f
    db = oracle.mfe(seq)[0]
    assert db.startswith("((((") and db.endswith("))))")  # (no span in the whole-record model: the stem over the record forms)
    assert z[base + ".global_zscore.txt"].decode() == expected_zscore_file(oracle, seq, "whole", 6, "di", 5)


def test_global_zscore_of_a_scan_only_run(emul, oracle, tmp_path, monkeypatch):
    """--dont_fold: the file is written all the same (a 130-nt record: the window entry point folds it)"""
    monkeypatch.setattr(_lib, "_engine", emul)
    monkeypatch.chdir(tmp_path)
    seq = rand_seq(np.random.default_rng(14), 130)
    (tmp_path / "in.fa").write_text(">rec2\n" + seq + "\n")
    assert sfd.main(["in.fa", "-w", "60", "-s", "40", "-r", "5", "--type", "mono", "--seed", "3", "--global_zscore",
                     "--dont_fold"]) == 0
    base = "rec2.win_60.stp_40.rnd_5.shfl_mono"
    assert sorted(os.listdir(tmp_path)) == sorted(["in.fa", base + ".out", base + ".global_zscore.txt"])
    assert (tmp_path / (base + ".global_zscore.txt")).read_text() == expected_zscore_file(oracle, seq, "UserInput", 5, "mono", 3)
    with pytest.raises(ValueError):
        sfd.main(["in.fa", "--global_zscore", "--lri"])


def test_global_zscore_refuses_a_record_past_the_limit_before_the_scan(emul, tmp_path, monkeypatch):
    monkeypatch.setattr(_lib, "_engine", emul)
    monkeypatch.chdir(tmp_path)
    (tmp_path / "in.fa").write_text(">ok\n" + "ACGU" * 20 + "\n>big\n" + "A" * (_lib.SF_MAX_LONG + 1) + "\n")
    with pytest.raises(ValueError, match="global_zscore"):
        sfd.main(["in.fa", "-w", "40", "-s", "20", "-r", "3", "--global_zscore"])
    assert os.listdir(tmp_path) == ["in.fa"]


# ---- what a single call must not share with a batch: the byte budget, the time records (run again on the GPU in test_gpu_long_batch.py) ----

def check_a_single_call_is_one_chunk_under_any_byte_budget(engine):
    s = rand_seq(np.random.default_rng(100 + 433), 433)
    rows = [rand_seq(np.random.default_rng(100 + 57), 57)] * 5
    whole = engine.fold_long(s)
    try:
        engine.set_long_batch_bytes(1)
        assert engine.fold_long(s) == whole
        engine.fold_long_batch(rows)
        assert engine.fold_long_batch_times()["chunks"] == 5  # the setting itself still works
    finally:
        engine.set_long_batch_bytes(0)


def check_the_two_time_records_stay_apart(engine):
    a, b, c = (rand_seq(np.random.default_rng(100 + L), L) for L in (57, 120, 150))
    engine.fold_long_batch([a, b], structure=True)
    batch = engine.fold_long_batch_times()
    engine.fold_long(c)
    assert engine.fold_long_batch_times() == batch
    single = engine.fold_long_times()
    engine.fold_long_batch([b, c, a], structure=True)
    assert engine.fold_long_times() == single


def test_a_single_call_is_one_chunk_under_any_byte_budget(emul):
    check_a_single_call_is_one_chunk_under_any_byte_budget(emul)


def test_the_two_time_records_stay_apart(emul):
    check_the_two_time_records_stay_apart(emul)
