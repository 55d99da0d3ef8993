"""Duplex folds and the LRI scan on the CPU emulation of the kernel sources, against tests/duplex_ref; the host side of
--lri against tests/golden/lri_cases.json; the driver end to end.  Every comparison is exact."""
import json
import os

import numpy as np
import pytest

import duplex_util as du
from scanfold_amd import _lib, lri, params
from emul.emul_engine import emul_engine

HERE = os.path.dirname(os.path.abspath(__file__))
CODES = np.frombuffer(b"NACGU", dtype=np.uint8)


def dinuc(s):
    import collections
    return collections.Counter(s[x:x + 2] for x in range(len(s) - 1))


def rseq(rng, n, al="ACGU"):
    return "".join(al[k] for k in rng.integers(0, len(al), n))


_ENGINE = []


def engine_with(p):
    """THE emulated engine (one library, one resident model) and the reference, both switched to the tables `p`: every test
    sets the two itself, so no test depends on what another one left loaded"""
    if not _ENGINE:
        _ENGINE.append(emul_engine(p))
    _ENGINE[0].load_params(p)
    du.set_params(p)
    return _ENGINE[0]


@pytest.fixture(params=[None, 3], ids=["default tables", "random tables"])
def eng(request):
    return engine_with(params.default_params() if request.param is None else params.random_params(request.param))


def test_duplex_batch_equals_reference(eng):
    rng = np.random.default_rng(2)
    s1 = [rseq(rng, int(rng.integers(1, _lib.SF_DUPLEX_MAX_LEN + 1)), ("ACGU", "GC", "ACGUN")[k % 3]) for k in range(150)]
    s2 = [rseq(rng, int(rng.integers(1, _lib.SF_DUPLEX_MAX_LEN + 1)), ("ACGU", "GC", "GU")[k % 3]) for k in range(150)]
    s1 += ["G" * 64, "A", "AAAA", ""]
    s2 += ["C" * 64, "U", "CCCC", "ACGU"]
    got = eng.duplex_batch(s1, s2)
    e, ri, rj, st = du.batch(s1, s2)
    assert (got["energy"] == e).all() and (got["i"] == ri).all() and (got["j"] == rj).all()
    assert got["structure"] == st
    assert got["energy"][-1] == _lib.SF_DUPLEX_NONE and got["structure"][-2:] == ["&", "&"]


def dense_as_dict(d):
    nj, nk = d["energy"].shape
    return {(a, b): (int(d["energy"][a, b]), int(d["i"][a, b]), int(d["j"][a, b]))
            for a in range(nj) for b in range(nk) if d["energy"][a, b] != _lib.SF_DUPLEX_SKIPPED}


@pytest.mark.parametrize("L,kmer,step", [(45, 5, 1), (200, 5, 3), (90, 20, 1), (200, 20, 3), (120, 33, 1), (150, 33, 3),
                                         (61, 20, 1), (19, 20, 1), (20, 20, 1), (47, 20, 3)])
def test_dense_scan_equals_reference_loops(eng, L, kmer, step):
    seq = rseq(np.random.default_rng(L * 100 + kmer), L)
    d = eng.lri_scan(seq, kmer, step, 0, dense=True)
    got = {(a * step, b * step): v for (a, b), v in dense_as_dict(d).items()}
    ref = du.dense_reference(seq, kmer, step)
    assert set(got) == set(du.reference_loops(L, kmer, step))
    assert got == ref
    if L >= kmer and (L - kmer + 1) % step == 0:
        assert any(j == L - kmer + 1 for j, _ in ref) or L < 2 * kmer + 5  # the short last strand 1 is scanned


def test_compacted_scan_is_the_filtered_dense_scan(eng):
    seq = rseq(np.random.default_rng(9), 140, "GC")
    ref = du.dense_reference(seq, 20, 1)
    cutoff = sorted(v[0] for v in ref.values())[len(ref) // 20]
    want = sorted((j, k) + v for (j, k), v in ref.items() if v[0] < cutoff)
    assert 3 <= len(want) < len(ref)
    hits = eng.lri_scan(seq, 20, 1, cutoff)
    assert [tuple(int(x) for x in h) for h in hits] == want
    with pytest.raises(_lib.ScanFoldHipError, match="max_hits"):
        eng.lri_scan(seq, 20, 1, cutoff, max_hits=len(want) - 1)
    # the status, and nothing written
    buf = np.full(len(want) - 1, 77, dtype=_lib.LRI_HIT_DTYPE)
    import ctypes
    n = ctypes.c_int64(0)
    s = np.frombuffer(seq.encode(), dtype=np.uint8)
    rc = eng.lib.sf_lri_scan(s.ctypes.data, len(s), 20, 1, int(cutoff), len(buf), buf.ctypes.data, ctypes.byref(n), None, None, None)
    assert rc == _lib.SF_ERR_DUPLEX_HITS and n.value == len(want) and (buf["energy"] == 77).all()
    assert len(eng.lri_scan(seq, 20, 1, cutoff, max_hits=len(want))) == len(want)


@pytest.mark.parametrize("kind", [_lib.SHUFFLE_MONO, _lib.SHUFFLE_DI])
def test_backgrounds(eng, kind):
    rng = np.random.default_rng(4)
    seq = rseq(rng, 100)
    kmer, r = 20, 12
    jw = np.array([0, 50, 81, 30], dtype=np.int32)  # 81 = L - kmer + 1: the short strand 1
    kw = np.array([40, 3, 10, 80], dtype=np.int32)
    en, r1, r2 = eng.lri_background(seq, kmer, jw, kw, r, kind, 11, rows=True)
    for h in range(len(jw)):
        frag, dup = seq[jw[h]:jw[h] + kmer], seq[kw[h]:kw[h] + kmer]
        n1 = len(frag)
        assert bytes(CODES[r2[h, 0]]).decode() == dup
        rows1 = [bytes(CODES[r1[h, x, :n1]]).decode() for x in range(r + 1)]
        rows2 = [bytes(CODES[r2[h, x]]).decode() for x in range(r + 1)]
        assert all(sorted(x) == sorted(frag) for x in rows1) and (r1[h, :, n1:] == 0).all()
        assert len(set(rows1)) > r // 2 and rows1[0] != frag  # element 0's strand 1 is shuffled too
        for x in rows2[1:]:
            if kind == _lib.SHUFFLE_MONO:
                assert sorted(x) == sorted(dup)
            else:
                assert dinuc(x) == dinuc(dup)
                assert x[0] == dup[0] and x[-1] == dup[-1]
        assert len(set(rows2[1:])) > r // 2
        e, _, _, _ = du.batch(rows1, rows2, structures=False)
        assert (en[h] == e).all()
    # a hit's row does not depend on the batch it is in
    order = [2, 0, 3, 1]
    assert (eng.lri_background(seq, kmer, jw[order], kw[order], r, kind, 11) == en[order]).all()
    assert (eng.lri_background(seq, kmer, jw[1:2], kw[1:2], r, kind, 11) == en[1:2]).all()
    assert (eng.lri_background(seq, kmer, jw, kw, r, kind, 12) != en).any()


def test_facade_and_twin_error(eng, monkeypatch):
    from scanfold_amd import RNA
    monkeypatch.setattr(_lib, "_engine", eng)
    d = RNA.duplexfold("GGGGAAAC", "GUUUCCCC")
    e, ri, rj, st = du.fold("GGGGAAAC", "GUUUCCCC")
    assert (d.energy, d.structure, d.i, d.j) == (float(np.float32(e) / np.float32(100)), st, ri, rj)
    none = RNA.duplexfold("AAAA", "CCCC")
    assert none.structure == "&" and none.energy == float(np.float32(10000000) / np.float32(100))

    class NoDuplex:
        _name = "twin"

        def __getattr__(self, name):
            raise AttributeError(name)
    twin = object.__new__(_lib.Engine)
    twin.lib = NoDuplex()
    assert not twin.has_duplex()
    for call in (lambda: twin.duplex_batch(["A"], ["U"]), lambda: twin.lri_scan("ACGU" * 20, 20, 1, 0),
                 lambda: twin.lri_background("ACGU" * 20, 20, [0], [40], 2, 0, 0)):
        with pytest.raises(_lib.ScanFoldHipError, match="no duplex entry points"):
            call()


def test_cpu_twin_library_has_no_duplex():
    import subprocess
    root = os.path.dirname(HERE)
    subprocess.check_call(["make", "-C", os.path.join(root, "oracle"), "-s"])
    lib = _lib.load_library(os.path.join(root, "oracle", "libscanfold_cpu.so"))
    e = object.__new__(_lib.Engine)
    e.lib = lib
    assert not e.has_duplex()
    with pytest.raises(_lib.ScanFoldHipError, match="no duplex entry points"):
        e.duplex_batch(["A"], ["U"])


def test_host_records_against_golden():
    with open(os.path.join(HERE, "golden", "lri_cases.json")) as f:
        cases = json.load(f)
    kinds = set()
    for c in cases:
        rec = lri.hit_record(c["frag"], c["dup_frag"], c["j_win"], c["k_win"], c["energy_dcal"], c["i"], c["j"], c["structure"])
        rec["cofold_zscore"] = c["cofold_zscore"]
        kept = rec["cofold_zscore"] < 10  # ScanFold.py:822: the row and its pairs exist only below 10
        assert (lri.lri_row(rec) if kept else "") == c["row"], c["name"]
        assert ([list(p) for p in lri.lri_pairs(rec)] if kept else []) == c["pairs"], c["name"]
        kinds.add(c["name"].split(":")[0])
    assert {"downstream", "upstream", "bulge", "strand ends"} <= kinds


def planted(L, seed, n_plant=3, kmer=20, au=0.5):
    """a random record (A+U fraction `au`) with reverse complements of n_plant of its own k-mers planted far downstream"""
    rng = np.random.default_rng(seed)
    s = ["ACGU"[k] for k in rng.choice(4, L, p=[au / 2, (1 - au) / 2, (1 - au) / 2, au / 2])]
    comp = str.maketrans("ACGU", "UGCA")
    for x in range(n_plant):
        a = 10 + x * (L // (2 * n_plant))
        b = L - 40 - x * (L // (2 * n_plant))
        s[b:b + kmer] = "".join(s[a:a + kmer]).translate(comp)[::-1]
    return "".join(s)


def expected_lri_file(eng, seq, kmer, step, cutoff, r, kind, seed):
    """.LRI.out computed from REFERENCE energies: the reference's loops and folds, and the reference's energies of the rows
    the engine shuffled"""
    from scanfold_amd import functions as sff
    out = [lri.HEADER]
    ref = du.dense_reference(seq, kmer, step)
    hit_keys = [k for k in du.reference_loops(len(seq), kmer, step) if ref[k][0] != du.NONE and ref[k][0] < cutoff * 100]
    if not hit_keys:
        return out, 0
    _, r1, r2 = eng.lri_background(seq, kmer, [k[0] for k in hit_keys], [k[1] for k in hit_keys], r, kind, seed, rows=True)
    for h, (jw, kw) in enumerate(hit_keys):
        frag, dup = seq[jw:jw + kmer], seq[kw:kw + kmer]
        e, ri, rj, st = du.fold(frag, dup)
        rec = lri.hit_record(frag, dup, jw, kw, e, ri, rj, st)
        en, _, _, _ = du.batch([bytes(CODES[row[:len(frag)]]).decode() for row in r1[h]],
                               [bytes(CODES[row]).decode() for row in r2[h]], structures=False)
        rec["cofold_zscore"] = round(sff.zscore_function(lri.energy_list(en), r), 2)
        if rec["cofold_zscore"] < 10:
            out.append(lri.lri_row(rec))
    return out, len(hit_keys)


@pytest.mark.parametrize("kind", ["mono", "di"])
def test_driver_end_to_end(tmp_path, monkeypatch, kind):
    from scanfold_amd import scanfold
    e = engine_with(params.default_params())
    monkeypatch.setattr(_lib, "_engine", e)
    monkeypatch.chdir(tmp_path)
    seq = planted(150, 21, n_plant=2, kmer=12)
    with open("x.fa", "w") as f:
        f.write(">rec\n" + seq + "\n")
    assert scanfold.main(["x.fa", "--lri", "--kmer", "12", "--kmer_step_size", "2", "--lri_cutoff", "-9", "-r", "10",
                          "--type", kind, "--seed", "5"]) == 0
    name = "rec.win_120.stp_1.rnd_10.shfl_%s.LRI.out" % kind
    assert os.listdir(".") == ["x.fa", name] or sorted(os.listdir(".")) == sorted(["x.fa", name])
    want, n_hits = expected_lri_file(e, seq, 12, 2, -9, 10, _lib.SHUFFLE_DI if kind == "di" else _lib.SHUFFLE_MONO, 5)
    assert n_hits >= 1
    assert open(name).readlines() == want
    # without --lri nothing of this is touched: the flag defaults parse and the window path is the one taken
    a = scanfold.build_parser().parse_args(["x.fa"])
    assert (a.lri, a.kmer, a.kmer_step_size, a.lri_cutoff) == (False, 20, 1, -25)


def test_driver_refuses_what_it_cannot_scan(tmp_path, monkeypatch):
    """before anything is scanned: a k-mer the duplex kernels cannot fold, a step of 0, more than one process"""
    from scanfold_amd import scanfold
    e = engine_with(params.default_params())
    monkeypatch.setattr(_lib, "_engine", e)
    monkeypatch.setattr(e, "lri_scan", lambda *a, **k: pytest.fail("the scan was started"))
    monkeypatch.chdir(tmp_path)
    with open("x.fa", "w") as f:
        f.write(">rec\n" + "ACGU" * 100 + "\n")
    for bad in (["--kmer", str(_lib.SF_DUPLEX_MAX_LEN + 1)], ["--kmer", "1"], ["--kmer_step_size", "0"]):
        with pytest.raises(ValueError, match="--kmer"):
            scanfold.main(["x.fa", "--lri"] + bad)
    with pytest.raises(ValueError, match="--kmer"):
        lri.lri_scan("ACGU" * 100, kmer=65, engine=e)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one GPU"):
        scanfold.main(["x.fa", "--lri"])
    assert os.listdir(".") == ["x.fa"]
    # the library refuses the same k-mers itself
    s = np.frombuffer(b"ACGU" * 100, dtype=np.uint8)
    import ctypes
    n = ctypes.c_int64(0)
    for kmer in (1, _lib.SF_DUPLEX_MAX_LEN + 1, 100):
        assert e.lib.sf_lri_scan(s.ctypes.data, len(s), kmer, 1, 0, 0, None, ctypes.byref(n), None, None, None) == -3


def test_vienna_duplexfold_opportunistic(tmp_path):
    """ViennaRNA's own RNA.duplexfold, where `import RNA` works, against the library (the emulated engine) and against the
    reference, under ViennaRNA's OWN compiled-in parameters: ViennaRNA writes them to a .par file, params.load_par reads it
    (as tests/test_vienna_opportunistic.py does for the folds), so the comparison tests the algorithm and not the shipped
    reconstructed table.  Skips only when the module is absent; parity is unpinned until it has run somewhere."""
    import conftest
    try:
        import RNA
    except Exception as e:
        conftest.SUMMARY_LINES.append("VIENNA duplexfold: absent (import RNA -> %s: %s); parity with RNA.duplexfold unpinned"
                                      % (type(e).__name__, e))
        pytest.skip("ViennaRNA (import RNA) is not installed: duplexfold parity stays unpinned")
    par = str(tmp_path / "vienna_compiled_in.par")
    if hasattr(RNA, "params_save"):
        RNA.params_save(par)
    else:
        RNA.write_parameter_file(par)
    eng = engine_with(params.load_par(par))
    rng = np.random.default_rng(0)
    s1 = [rseq(rng, 20, ("ACGU", "GC", "ACGUN")[k % 3]) for k in range(300)]
    s2 = [rseq(rng, 20, ("ACGU", "GC", "GU")[k % 3]) for k in range(300)]
    s1 += [rseq(rng, int(rng.integers(1, 65))) for _ in range(200)]
    s2 += [rseq(rng, int(rng.integers(1, 65))) for _ in range(200)]
    got = eng.duplex_batch(s1, s2)
    bad = []
    for x, (a, b) in enumerate(zip(s1, s2)):
        e, ri, rj, st = du.fold(a, b)
        lib_rec = (int(got["energy"][x]), int(got["i"][x]), int(got["j"][x]), got["structure"][x])
        if e == du.NONE:  # upstream leaves its minimum at INF there; what it puts into the record is not compared
            ok = lib_rec == (e, ri, rj, st)
        else:
            d = RNA.duplexfold(a, b)
            ok = (int(round(d.energy * 100)), d.i, d.j, d.structure) == (e, ri, rj, st) == lib_rec
        if not ok:
            bad.append((a, b))
    conftest.SUMMARY_LINES.append("VIENNA duplexfold: ran (ViennaRNA %s, %d pairs under its own parameters: %d differ)"
                                  % (getattr(RNA, "__version__", "unknown"), len(s1), len(bad)))
    assert not bad, bad[:10]
