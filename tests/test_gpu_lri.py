"""Duplex folds and the LRI scan on the device, against tests/duplex_ref, at sizes the emulation is too slow for.  Exact."""
import os

import numpy as np
import pytest

import duplex_util as du
from scanfold_amd import _lib, params
from test_lri import CODES, dense_as_dict, expected_lri_file, planted, rseq

pytestmark = pytest.mark.gpu


@pytest.fixture()
def eng(gpu_engine):
    gpu_engine.load_params(params.default_params())
    du.set_params(gpu_engine.params)
    return gpu_engine


def test_dense_scan_600(eng):
    seq = rseq(np.random.default_rng(600), 600)
    got = dense_as_dict(eng.lri_scan(seq, 20, 1, 0, dense=True))
    assert got == du.dense_reference(seq, 20, 1) and len(got) > 300000


def test_compacted_scan_4000_and_backgrounds(eng):
    seq = planted(4000, 7, au=0.7)  # A+U rich: few chance duplexes below -25 kcal/mol beside the planted ones
    ref = du.dense_reference(seq, 20, 1)
    want = sorted((j, k) + v for (j, k), v in ref.items() if v[0] != du.NONE and v[0] < -2500)
    assert 3 <= len(want) <= 400
    hits = eng.lri_scan(seq, 20, 1, -2500)
    assert [tuple(int(x) for x in h) for h in hits] == want
    with pytest.raises(_lib.ScanFoldHipError, match="max_hits"):
        eng.lri_scan(seq, 20, 1, -2500, max_hits=2)
    for kind in (_lib.SHUFFLE_MONO, _lib.SHUFFLE_DI):
        en, r1, r2 = eng.lri_background(seq, 20, hits["j_win"], hits["k_win"], 100, kind, 3, rows=True)
        n = len(hits) * 101
        l1 = [min(20, len(seq) - int(j)) for j in hits["j_win"] for _ in range(101)]
        s1 = [bytes(CODES[row[:l1[x]]]).decode() for x, row in enumerate(r1.reshape(n, 20))]
        s2 = [bytes(CODES[row]).decode() for row in r2.reshape(n, 20)]
        e, _, _, _ = du.batch(s1, s2, structures=False)
        assert (en.reshape(-1) == e).all()
        assert (eng.lri_background(seq, 20, hits["j_win"][::-1], hits["k_win"][::-1], 100, kind, 3) == en[::-1]).all()


def test_duplex_batch_10000(eng):
    rng = np.random.default_rng(8)
    s1 = [rseq(rng, int(rng.integers(1, 65)), ("ACGU", "GC", "ACGUN")[k % 3]) for k in range(10000)]
    s2 = [rseq(rng, int(rng.integers(1, 65)), ("ACGU", "GC", "GU")[k % 3]) for k in range(10000)]
    got = eng.duplex_batch(s1, s2)
    e, ri, rj, st = du.batch(s1, s2)
    assert (got["energy"] == e).all() and (got["i"] == ri).all() and (got["j"] == rj).all() and got["structure"] == st


def test_random_tables(eng):
    p0 = eng.params
    try:
        p = params.random_params(17)
        eng.load_params(p)
        du.set_params(p)
        seq = rseq(np.random.default_rng(1), 300)
        assert dense_as_dict(eng.lri_scan(seq, 20, 1, 0, dense=True)) == du.dense_reference(seq, 20, 1)
        assert dense_as_dict(eng.lri_scan(seq, 40, 1, 0, dense=True)) == du.dense_reference(seq, 40, 1)  # device-memory tables
    finally:
        eng.load_params(p0)


def test_cli_writes_lri_out(eng, tmp_path, monkeypatch):
    from scanfold_amd import scanfold
    monkeypatch.setattr(_lib, "_engine", eng)
    monkeypatch.chdir(tmp_path)
    seq = planted(1500, 7, au=0.7)
    with open("x.fa", "w") as f:
        f.write(">rec\n" + seq + "\n")
    assert scanfold.main(["x.fa", "--lri", "-r", "100", "--type", "di", "--seed", "2"]) == 0
    want, n_hits = expected_lri_file(eng, seq, 20, 1, -25, 100, _lib.SHUFFLE_DI, 2)
    assert n_hits >= 3
    assert open("rec.win_120.stp_1.rnd_100.shfl_di.LRI.out").readlines() == want
