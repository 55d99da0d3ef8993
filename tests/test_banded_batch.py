"""Many whole-record folds under a base-pair span at once (sf_fold_banded_batch, include/scanfold_hip_long.h) on the CPU build of
the kernel sources: against the oracle on records whose band is live up to its last diagonal, against sf_fold_banded row by
row in a ragged call (rows shorter than the band, rows that drop out of early diagonals, constraints, a type-7 pair), in
reversed order, chunked by the byte budget and energies only, always with == on energy and structure; bad arguments; what the
one host driver of the four MFE entry points promises (a single call is one chunk under any budget, the four time records stay
apart, dots are no constraint and a one-row batch is the single call); and the combined driver's --global_zscore_span.

The checks are shared with test_gpu_banded_batch.py, which runs them on the MI355X over more spans, longer rows, other
parameter sets and records past 32 767 nt.  Record builders and the `model` context come from test_banded_fold.py."""
import os
import random
import statistics

import numpy as np
import pytest

from scanfold_amd import _lib, functions, params
from scanfold_amd import scanfold as sfd
from long_util import formed_type7, hairpin_rich, rand_seq
import test_banded_fold as tb

RAGGED = [1, 4, 5, 63, 64, 65, 200, 433, 700]


@pytest.fixture(scope="module")
def emul():
    from emul_engine import emul_engine
    e = emul_engine()
    e.load_params(params.default_params())
    return e


# ---- checks shared with test_gpu_banded_batch.py ----

def check_oracle_rows(engine, oracle, L, S, both_models=True):
    """One call per model under span S: two edge_records of L nt (their band live on its last diagonal and cut by the record's
    end) and a 433-nt multiloop_edge_record; every row must be the oracle's fold under the call's model.  The records' own
    folds (made when they were searched) serve where the model is theirs, a fresh oracle fold elsewhere."""
    a, b = tb.edge_record(oracle, "random", L, S), tb.edge_record(oracle, "hairpin_rich", L, S)
    m = tb.multiloop_edge_record(oracle, 433, S)
    rows = [a[0], m[0], b[0]]
    for p in ([None, tb.multiloop_params()] if both_models else [None]):
        with tb.model(engine, oracle, p, S):
            want = []
            for rec in (a, m, b):
                own = (rec is m) == (p is not None)  # the record was searched under this model
                want.append((rec[2], rec[1]) if own else oracle.mfe(rec[0])[::-1])
            e, db = engine.fold_banded_batch(rows, structure=True)
            assert e.dtype == np.int32 and e.shape == (3,)
            assert [(int(e[k]), db[k]) for k in range(3)] == want, (L, S, p is not None)
            t = engine.fold_banded_batch_times()
            assert t["chunks"] == 1 and t["fill_launches"] == min(S, max(L, 433))


def marked_rows(engine, L, S, formed=True):
    """-> [(seq, cons)] * 2 under the resident span S: a record whose fold_banded forms the constraint's type-7 pair (on the
    band's last diagonal; formed=False: the first record, whatever its fold), and another sequence under the same 'x < >' marks
    without the brackets"""
    for seed in range(8 if formed else 1):
        s, cons = tb.marked_record(L, S, L + S + 1 + 1000 * seed)
        t7 = formed_type7(s, cons, engine.fold_banded(s, cons)[1])
        if t7:
            break
    assert not formed or (t7 and all(j - i == S - 1 for i, j in t7))
    assert set("x<>()") <= set(cons)
    marks = cons.replace("(", ".").replace(")", ".")
    return [(s, cons), (rand_seq(np.random.default_rng(L + S), L), marks)]


def predicted_chunks(lens, S, budget):
    """the chunking rule of include/scanfold_hip_long.h: consecutive rows while their SF_BANDED_BYTES fit the budget, always at
    least one -> [[lengths of a chunk]]"""
    out, cur, used = [], [], 0
    for L in lens:
        b = tb.banded_bytes(L, S)
        if cur and used + b > budget:
            out.append(cur)
            cur, used = [], 0
        cur.append(L)
        used += b
    return out + [cur]


def check_ragged(engine, S, lens=RAGGED, default_model=True):
    """rows of `lens`, plus a row with a formed type-7 pair, a row of marks and a row of dots only, in one call under span S
    and the resident parameter set: equal to fold_banded row by row; the same bytes in reversed order, in chunks of one or two
    rows and with energies only; chunk and launch counts as the chunking rule predicts.  default_model=False (another
    parameter set is resident): what the rows fold into is not looked at, only that both entry points agree"""
    engine.set_max_bp_span(S)
    try:
        seqs = [rand_seq(np.random.default_rng(100 + L), L) for L in lens]
        cons = [None] * len(seqs)
        cons[lens.index(200)] = "." * 200
        for s, c in marked_rows(engine, 700, S, formed=default_model):
            seqs.append(s)
            cons.append(c)
        n = len(seqs)
        all_lens = [len(s) for s in seqs]
        ref = [engine.fold_banded(s, c) for s, c in zip(seqs, cons)]
        assert not default_model or sum(db.count("(") for _, db in ref) > sum(all_lens) // 10

        def run(order, structure=True):
            got = engine.fold_banded_batch([seqs[k] for k in order], [cons[k] for k in order], structure=structure)
            e, db = got if structure else (got, [None] * n)
            back = {k: (int(e[x]), db[x]) for x, k in enumerate(order)}
            return [back[k] for k in range(n)]

        order = list(range(n))
        assert run(order) == ref
        t = engine.fold_banded_batch_times()
        assert t["chunks"] == 1 and t["fill_launches"] == min(S, max(all_lens)) and t["trace_ms"] > 0
        assert run(order[::-1]) == ref
        assert run(order, structure=False) == [(e, None) for e, _ in ref]
        assert engine.fold_banded_batch_times()["trace_ms"] == 0
        try:
            budget = tb.banded_bytes(1, S) + tb.banded_bytes(4, S)  # rows 1 and 4 share a chunk, every other row is alone
            for o in (order, order[::-1]):
                engine.set_long_batch_bytes(budget)
                chunks = predicted_chunks([all_lens[k] for k in o], S, budget)
                assert {len(c) for c in chunks} == {1, 2}
                assert run(o) == ref
                t = engine.fold_banded_batch_times()
                assert t["chunks"] == len(chunks) == n - 1
                assert t["fill_launches"] == sum(min(S, max(c)) for c in chunks)
        finally:
            engine.set_long_batch_bytes(0)
        assert run(order) == ref
        assert engine.fold_banded_batch_times()["chunks"] == 1  # the default budget is back
    finally:
        engine.set_max_bp_span(0)


def check_errors(engine):
    lib = engine.lib
    n, ld = 3, 40
    arr = np.frombuffer(b"ACGU" * 30, dtype=np.uint8).reshape(n, ld).copy()
    out = np.full(n, 777, dtype=np.int32)
    dbuf = np.full((n, ld + 1), ord("?"), dtype=np.uint8)

    def call(seqs, m, lens, e, cons=None, db=dbuf):
        ln = None if lens is None else np.array(lens, dtype=np.int32)
        return lib.sf_fold_banded_batch(seqs, m, ld, None if ln is None else ln.ctypes.data,
                                        None if cons is None else cons.ctypes.data, e, None if db is None else db.ctypes.data)

    a, o = arr.ctypes.data, out.ctypes.data
    engine.set_max_bp_span(0)
    assert call(a, n, [40, 40, 40], o) == -3  # no span set
    with pytest.raises(_lib.ScanFoldHipError):
        engine.fold_banded_batch(["ACGU" * 10])
    engine.set_max_bp_span(20)
    try:
        assert call(a, 0, [40, 40, 40], o) == 0  # n == 0
        assert call(None, 0, None, None) == 0
        assert call(a, -1, [40, 40, 40], o) == -3
        assert call(a, n, [40, 0, 40], o) == -3   # a length of 0
        assert call(a, n, [40, 40, 41], o) == -3  # a length greater than ld
        assert call(None, n, [40, 40, 40], o) == -3
        assert call(a, n, None, o) == -3
        assert call(a, n, [40, 40, 40], None) == -3
        cc = np.full((n, ld), ord("."), dtype=np.uint8)
        cc[0, 2], cc[0, 13] = ord("("), ord(")")
        cc[2, 20:23] = np.frombuffer(b".))", dtype=np.uint8)  # unbalanced brackets in the last row
        assert call(a, n, [40, 40, 40], o, cc) == -9
        assert (out == 777).all() and (dbuf == ord("?")).all()  # no output was written by any refused call
        with pytest.raises(_lib.ScanFoldHipError):
            engine.fold_banded_batch(["ACGU" * 10, "ACGU"], [None, "(..."])
        with pytest.raises(_lib.ScanFoldHipError):
            engine.fold_banded_batch(["ACGU", ""])
        with pytest.raises(ValueError):
            engine.fold_banded_batch(["ACGU"], ["..."])
        cc[2, 20:23] = np.frombuffer(b"...", dtype=np.uint8)
        assert call(a, n, [40, 17, 40], o, cc) == 0 and (out != 777).all()
        assert bytes(dbuf[1, 17:19]) == b"\0?" and bytes(dbuf[0, 40:]) == b"\0"
        assert call(a, n, [40, 17, 40], o, cc, db=None) == 0  # energies only
        e = engine.fold_banded_batch([])
        assert e.shape == (0,) and e.dtype == np.int32
        assert engine.fold_banded_batch([], structure=True)[1] == []
        t = engine.fold_banded_batch_times()
        assert t["chunks"] == 0 and t["fill_launches"] == 0
    finally:
        engine.set_max_bp_span(0)


DRIVER_SPAN = 40  # the span of the checks below, which hold the four MFE entry points to what their one host driver promises


def driver_rows():
    """seeded rows of 57, 120, 150 and 433 nt"""
    return [rand_seq(np.random.default_rng(100 + L), L) for L in (57, 120, 150, 433)]


def check_single_is_one_chunk(engine):
    """fold_banded is one chunk under any byte budget: the 433-nt row folds to the same tuple under a budget of one byte,
    under which a batch of five 57-nt rows runs as five chunks"""
    s = driver_rows()[3]
    engine.set_max_bp_span(DRIVER_SPAN)
    try:
        ref = engine.fold_banded(s)
        try:
            engine.set_long_batch_bytes(1)
            assert engine.fold_banded(s) == ref
            rows = [rand_seq(np.random.default_rng(k), 57) for k in range(5)]
            engine.fold_banded_batch(rows)
            assert engine.fold_banded_batch_times()["chunks"] == 5
        finally:
            engine.set_long_batch_bytes(0)
    finally:
        engine.set_max_bp_span(0)


def check_time_records_stay_apart(engine):
    """every entry point's time record is left alone by the other family's calls and by its own family's other call"""
    rows = driver_rows()
    engine.set_max_bp_span(DRIVER_SPAN)
    try:
        engine.fold_banded_batch(rows, structure=True)
        t = engine.fold_banded_batch_times()
        assert t["chunks"] == 1 and t["fill_launches"] == DRIVER_SPAN
        engine.fold_banded(rows[3])
        t_single = engine.fold_banded_times()
        assert t_single["band"] == DRIVER_SPAN and t_single["fill_launches"] == DRIVER_SPAN
        engine.fold_long(rows[2])
        assert engine.fold_banded_batch_times() == t  # after a fold_banded and a fold_long
        engine.fold_long_batch(rows, structure=True)
        t_long, t_long_batch = engine.fold_long_times(), engine.fold_long_batch_times()
        engine.fold_banded_batch(rows, structure=True)
        assert engine.fold_banded_times() == t_single  # after a fold_long_batch and a fold_banded_batch
        engine.fold_banded(rows[1])
        assert engine.fold_long_times() == t_long  # after both banded calls
        assert engine.fold_long_batch_times() == t_long_batch
    finally:
        engine.set_max_bp_span(0)


def check_dots_and_one_row_batches(engine, oracle):
    """a constraint of dots is no constraint for fold_banded, and a batch of that one row, with dots and with the structure,
    gives the single call's energy and string; rows of 1 and 4 nt give the oracle's under the span"""
    with tb.model(engine, oracle, None, DRIVER_SPAN):
        for s in driver_rows() + [rand_seq(np.random.default_rng(100 + L), L) for L in (1, 4)]:
            L = len(s)
            ref = engine.fold_banded(s)
            if L <= 4:
                assert ref == oracle.mfe(s)[::-1]
            assert engine.fold_banded(s, "." * L) == ref
            e, db = engine.fold_banded_batch([s], ["." * L], structure=True)
            assert e.shape == (1,) and (int(e[0]), db[0]) == ref


def expected_zscore_span_file(energy_dcal, seq, name, r, kind, seed, span):
    """<outname>.global_zscore.txt of --global_zscore_span from the generator draws of --seed and energy_dcal(sequence), the
    fold under the span: GLOBAL_ZSCORE_HEADER's columns and a trailing Span"""
    state = random.getstate()
    random.seed(seed)
    shuffles = functions.scramble(seq, r, kind)
    random.setstate(state)
    assert len(set(shuffles)) == r
    E = [float(np.float32(energy_dcal(s) / 100)) for s in [seq] + shuffles]
    row = [name, str(len(seq)), "37", str(r), kind] + [str(round(x, 2)) for x in (
        E[0], statistics.mean(E[1:]), statistics.stdev(E[1:]), functions.zscore_function(E, r), functions.pvalue_function(E, r))]
    assert sfd.GLOBAL_ZSCORE_HEADER.endswith("P-value\n")
    return sfd.GLOBAL_ZSCORE_HEADER[:-1] + "\tSpan\n" + "\t".join(row + [str(span)]) + "\n"


def check_driver_zscore_span(engine, oracle, tmp_path, monkeypatch):
    """a 450-nt record, -r 5 --type di --seed 3, span 60: the file from the oracle's folds under that span; every other output
    of the run byte-identical with and without the flag; the engine's state and the generator's as they were"""
    monkeypatch.setattr(_lib, "_engine", engine)
    S = 60
    seq = hairpin_rich(np.random.default_rng(450), 450)
    args = ["in.fa", "-w", "40", "-s", "40", "-r", "5", "--type", "di", "--seed", "3", "--name", "whole", "--span", "50",
            "--dont_extract"]
    outs = {}
    try:
        for flag in ([], ["--global_zscore_span", str(S)]):
            d = tmp_path / ("z" if flag else "plain")
            d.mkdir()
            (d / "in.fa").write_text(">rec1\n" + seq.replace("U", "T") + "\n")
            monkeypatch.chdir(d)
            random.seed(99)
            state = random.getstate()
            params0 = engine.params
            assert sfd.main(args + flag) == 0
            assert random.getstate() == state
            assert engine.max_bp_span == 50 and engine.params is params0 and engine.params.temperature == 37.0
            outs[bool(flag)] = {f: (d / f).read_bytes() for f in os.listdir(d)}
    finally:
        engine.set_max_bp_span(0)
        engine.md_span = 0
    base = "rec1.win_40.stp_40.rnd_5.shfl_di"
    plain, z = outs[False], outs[True]
    assert sorted(set(z) - set(plain)) == [base + ".global_zscore.txt"]
    assert len(plain) > 5
    for f in plain:
        assert z[f] == plain[f], f
    oracle.set_max_bp_span(S)
    try:
        want = expected_zscore_span_file(lambda s: oracle.mfe(s)[1], seq, "whole", 5, "di", 3, S)
        spanned = oracle.mfe(seq)[1]
    finally:
        oracle.set_max_bp_span(0)
    assert spanned != oracle.mfe(seq)[1]  # (the span binds on this record: the file is not --global_zscore's)
    assert z[base + ".global_zscore.txt"].decode() == want


def check_driver_refusals(tmp_path, monkeypatch):
    """--global_zscore_span with --global_zscore, with --lri, with N < 1 and on a record past SF_MAX_BANDED: refused before
    anything is scanned"""
    monkeypatch.chdir(tmp_path)
    (tmp_path / "in.fa").write_text(">ok\n" + "ACGU" * 40 + "\n")
    base = ["in.fa", "-w", "40", "-s", "20", "-r", "3"]
    with pytest.raises(ValueError, match="same file"):
        sfd.main(base + ["--global_zscore_span", "60", "--global_zscore"])
    with pytest.raises(ValueError, match="--lri"):
        sfd.main(base + ["--global_zscore_span", "60", "--lri"])
    for bad in ("0", "-5"):
        with pytest.raises(ValueError, match="global_zscore_span"):
            sfd.main(base + ["--global_zscore_span", bad])
    (tmp_path / "big.fa").write_text(">ok\n" + "ACGU" * 20 + "\n>big\n" + "A" * (_lib.SF_MAX_BANDED + 1) + "\n")
    with pytest.raises(ValueError, match="global_zscore_span"):
        sfd.main(["big.fa"] + base[1:] + ["--global_zscore_span", "60"])
    assert sorted(os.listdir(tmp_path)) == ["big.fa", "in.fa"]


# ---- on the emulation ----

@pytest.mark.parametrize("S", [30, 65])
def test_live_bands_equal_oracle(emul, oracle, S):
    check_oracle_rows(emul, oracle, 433, S)


def test_ragged_call_equals_fold_banded(emul):
    check_ragged(emul, 64)


def test_errors(emul):
    check_errors(emul)


def test_single_call_is_one_chunk_under_any_budget(emul):
    check_single_is_one_chunk(emul)


def test_time_records_stay_apart(emul):
    check_time_records_stay_apart(emul)


def test_dots_and_one_row_batches(emul, oracle):
    check_dots_and_one_row_batches(emul, oracle)


def test_combined_driver_global_zscore_span(emul, oracle, tmp_path, monkeypatch):
    check_driver_zscore_span(emul, oracle, tmp_path, monkeypatch)


def test_global_zscore_span_refusals(tmp_path, monkeypatch):
    check_driver_refusals(tmp_path, monkeypatch)


def test_global_zscore_span_of_a_scan_only_run(emul, oracle, tmp_path, monkeypatch):
    """--dont_fold, no --global_refold and no --global_span: the file is written all the same"""
    monkeypatch.setattr(_lib, "_engine", emul)
    monkeypatch.chdir(tmp_path)
    seq = rand_seq(np.random.default_rng(15), 130)
    (tmp_path / "in.fa").write_text(">rec2\n" + seq + "\n")
    assert sfd.main(["in.fa", "-w", "60", "-s", "40", "-r", "5", "--type", "mono", "--seed", "3", "--global_zscore_span", "25",
                     "--dont_fold"]) == 0
    base = "rec2.win_60.stp_40.rnd_5.shfl_mono"
    assert sorted(os.listdir(tmp_path)) == sorted(["in.fa", base + ".out", base + ".global_zscore.txt"])
    oracle.set_max_bp_span(25)
    try:
        want = expected_zscore_span_file(lambda s: oracle.mfe(s)[1], seq, "UserInput", 5, "mono", 3, 25)
    finally:
        oracle.set_max_bp_span(0)
    assert (tmp_path / (base + ".global_zscore.txt")).read_text() == want
    assert emul.max_bp_span == 0


def test_cpu_twin_has_no_banded_batch():
    twin = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "libscanfold_cpu.so")
    from oracle import oracle as orc
    orc.build()
    if not os.path.exists(twin):
        pytest.skip("the CPU twin of the C ABI was not built")
    eng = _lib.Engine(device=0, lib_path=twin)
    assert not eng.has_fold_banded_batch()
    with pytest.raises(_lib.ScanFoldHipError, match="sf_fold_banded_batch"):
        eng.fold_banded_batch(["ACGU" * 120])
