"""The whole-record partition function (sf_pf_long, include/scanfold_hip_long.h): the kernel source compiled for the CPU
against the oracle's McCaskill fold and against the window entry points, its scaling, its additivity over span-separated
blocks past FP64's range, and its way up: Engine.pf_long, functions.rna_refold, ScanFold.py's --global_ensemble.

The emulation pays per lane, so its build has a small lane budget per compute unit (SF_PFLONG_LANES_PER_CU under SF_EMUL);
the GPU tests run the product's."""
import ctypes
import os

import numpy as np
import pytest

from scanfold_amd import _lib, params
from scanfold_amd import RNA
from scanfold_amd import functions as sff
from scanfold_amd import scanfold as sfd
import pf_util
from long_pf_util import (KEYS, assert_carries_weight, assert_close, block_record, cubic_reference, forget_cubic_references,
                          gc_only, nested_record, oracle_pf)  # (forget_cubic_references: an autouse fixture)
from long_util import hairpin_rich, rand_seq
from test_long_fold import constraint_string, params_in, planted_stem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emul():
    from emul_engine import emul_engine
    e = emul_engine()
    e.load_params(params.default_params())
    assert e.has_pf_long()
    return e


@pytest.mark.parametrize("L", [1, 4, 57, 401, 433])
def test_unconstrained_equals_oracle(emul, oracle, L):
    s = rand_seq(np.random.default_rng(100 + L), L)
    ref = oracle.pf(s, want_bpp=True)
    assert_close(emul.pf_long(s), ref, "L=%d" % L, ref["bpp"])


@pytest.mark.parametrize("L", [120, 400])
def test_short_sequences_equal_the_window_entry_points(emul, L):
    rng = np.random.default_rng(60 + L)
    s = rand_seq(rng, L)
    assert_close(emul.pf_long(s), pf_util.row(emul.pf_batch([s]), 0), "pf_batch %d" % L)
    cons = constraint_string(s, rng)
    r = emul.fold_constrained([s], [cons], mfe=False)
    assert_close(emul.pf_long(s, cons), pf_util.row(r, 0), "fold_constrained %d" % L)


def test_constrained_equals_oracle(emul, oracle):
    rng = np.random.default_rng(30 + 433)
    s = rand_seq(rng, 433)
    cons = constraint_string(s, rng)
    assert set("x<>()") <= set(cons)
    ref = oracle_pf(oracle, s, cons, want_bpp=True)
    got = emul.pf_long(s, cons)
    assert_close(got, ref, "constrained", ref["bpp"])
    for k, ch in enumerate(cons):
        if ch == "x":
            assert got["centroid"][k] == "."


def test_span_equals_oracle(emul, oracle):
    s = planted_stem(np.random.default_rng(5), 433)
    emul.set_max_bp_span(150)
    oracle.set_max_bp_span(150)
    try:
        ref = oracle.pf(s, want_bpp=True)
        assert_close(emul.pf_long(s), ref, "span 150", ref["bpp"])
    finally:
        emul.set_max_bp_span(0)
        oracle.set_max_bp_span(0)


def test_randomised_parameter_set(emul, oracle):
    with params_in(oracle, emul, params.random_params(3)):
        s = rand_seq(np.random.default_rng(6), 433)
        ref = oracle.pf(s, want_bpp=True)
        assert_close(emul.pf_long(s), ref, "random_params(3)", ref["bpp"])


def test_rescaled_temperature_set(emul, oracle):
    p = pf_util.cold()
    assert p.temperature == 25.0
    try:
        orc = pf_util.use(p)
        emul.load_params(p)
        s = rand_seq(np.random.default_rng(25), 420)
        ref = orc.pf(s, want_bpp=True)
        assert_close(emul.pf_long(s), ref, "25 C", ref["bpp"])
    finally:
        pf_util.use(params.default_params())
        emul.load_params(params.default_params())


def test_scaling_is_exercised(emul, oracle):
    s = gc_only()
    lz = oracle.pf_unscaled(s)["lnZ"]
    assert not lz <= 709.0, lz  # the unscaled fold is out of FP64's range
    ref = oracle.pf(s, want_bpp=True)
    assert abs(ref["dG"] - (-457.34)) < 0.005
    assert_close(emul.pf_long(s), ref, "GC 480", ref["bpp"])
    t = emul.pf_long_times()
    assert t["lns"] > 0 and 1 <= t["attempts"] <= 6
    e, _ = emul.fold_long(s, structure=False)
    assert_close(emul.pf_long(s, mfe_hint=e), ref, "GC 480 with the MFE", ref["bpp"])
    assert emul.pf_long_times()["attempts"] == 1


def test_additivity_past_the_range(emul, oracle):
    """Nine hairpin_rich blocks of 220..330 nt joined by 150 N under span 150 (~3.6 kb, ln Z ~ 1 100): dG, mean_bp_dist and
    centroid_dist are the sums of the blocks' oracle values, the centroid their centroids joined by dots."""
    rng = np.random.default_rng(9)
    lens = [int(k) for k in rng.integers(220, 331, 9)]
    seq, ref, _ = block_record(oracle, lens, 150, 17, hairpin_rich)
    assert 3400 <= len(seq) <= 4200
    assert -ref["dG"] / 0.61632 > 709
    emul.set_max_bp_span(150)
    try:
        assert_close(emul.pf_long(seq), ref, "nine blocks")
    finally:
        emul.set_max_bp_span(0)


def test_rna_refold(emul, oracle, tmp_path, monkeypatch):
    monkeypatch.setattr(_lib, "_engine", emul)
    rng = np.random.default_rng(44)
    s = rand_seq(rng, 433)
    cons = constraint_string(s, rng)
    f = tmp_path / "cons.txt"
    f.write_text(s + "\n" + cons + "\n")
    oracle.set_constraint(cons)
    try:
        db, e = oracle.mfe(s)
        ref = oracle.pf(s)
    finally:
        oracle.set_constraint(None)
    structure, centroid, mfe, ed = sff.rna_refold(s, 37, str(f))
    assert (structure, centroid, mfe) == (db, ref["centroid"], RNA._f32(e))
    assert ed == round(ref["mean_bp_dist"], 2)
    # a short sequence goes through the window entry points
    s2, c2 = s[:90], "." * 90
    (tmp_path / "c2.txt").write_text(s2 + "\n" + c2 + "\n")
    db2, e2 = oracle.mfe(s2)
    r2 = oracle.pf(s2)
    assert sff.rna_refold(s2, 37, str(tmp_path / "c2.txt")) == (db2, r2["centroid"], RNA._f32(e2), round(r2["mean_bp_dist"], 2))


def test_global_ensemble_needs_global_refold(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    (tmp_path / "in.fa").write_text(">r\n" + "ACGU" * 30 + "\n")
    with pytest.raises(ValueError):
        sfd.main(["in.fa", "-w", "40", "-s", "30", "-r", "3", "--global_ensemble"])
    assert os.listdir(tmp_path) == ["in.fa"]  # refused before scanning


def test_combined_driver_global_ensemble(emul, tmp_path, monkeypatch):
    monkeypatch.setattr(_lib, "_engine", emul)
    seq = planted_stem(np.random.default_rng(12), 600, n_stem=10)
    args = ["in.fa", "-w", "40", "-s", "30", "-r", "3", "--type", "mono", "--seed", "2", "--name", "myrna", "--dont_extract",
            "--global_refold"]
    base = "rec1.win_40.stp_30.rnd_3.shfl_mono"
    outs = {}
    for flag in ([], ["--global_ensemble"]):
        d = tmp_path / ("ens" if flag else "plain")
        d.mkdir()
        (d / "in.fa").write_text(">rec1 x\n" + seq + "\n")
        monkeypatch.chdir(d)
        assert sfd.main(args + flag) == 0
        outs[bool(flag)] = {f: (d / f).read_bytes() for f in os.listdir(d)}
    extra = set(outs[True]) - set(outs[False])
    assert extra == {base + ".AllDBN-global_refold.ensemble.txt"}
    for f in outs[False]:
        assert outs[True][f] == outs[False][f], f  # AllDBN-global_refold.txt among them, byte for byte
    lines = outs[True][base + ".AllDBN-global_refold.ensemble.txt"].decode().split("\n")
    assert len(lines) == 10 and lines[9] == ""
    cons = [None] + [outs[True][base + ".ScanFold." + t + ".dbn"].decode().split("\n")[2] for t in ("-1", "-2")]
    for k, c in enumerate(cons):
        c = None if c is None else c + "." * (len(seq) - len(c))
        r = emul.pf_long(seq, c)
        head, s, cen = lines[3 * k:3 * k + 3]
        assert head.startswith(">myrna\t") and s == seq and cen == r["centroid"]
        assert head.endswith("ensemble dG=%.2f ED=%.2f centroid distance=%.2f" % (r["dG"], r["mean_bp_dist"], r["centroid_dist"]))


def test_global_ensemble_of_a_short_record(emul, tmp_path, monkeypatch):
    """A record of at most SF_MAX_W nt: the three ensembles come from the window entry point (fold_constrained)."""
    monkeypatch.setattr(_lib, "_engine", emul)
    monkeypatch.chdir(tmp_path)
    seq = planted_stem(np.random.default_rng(13), 130, n_stem=8)
    (tmp_path / "in.fa").write_text(">rec1\n" + seq + "\n")
    assert sfd.main(["in.fa", "-w", "40", "-s", "30", "-r", "3", "--type", "mono", "--seed", "2", "--name", "short",
                     "--dont_extract", "--global_refold", "--global_ensemble"]) == 0
    base = "rec1.win_40.stp_30.rnd_3.shfl_mono"
    lines = (tmp_path / (base + ".AllDBN-global_refold.ensemble.txt")).read_text().split("\n")
    assert len(lines) == 10 and lines[9] == ""
    cons = [None] + [(tmp_path / (base + ".ScanFold." + t + ".dbn")).read_text().split("\n")[2] for t in ("-1", "-2")]
    for k, c in enumerate(cons):
        c = "." * len(seq) if c is None else c + "." * (len(seq) - len(c))
        r = pf_util.row(emul.fold_constrained([seq], [c], mfe=False), 0)
        head, s, cen = lines[3 * k:3 * k + 3]
        assert head.startswith(">short\t") and s == seq and cen == r["centroid"]
        assert head.endswith("ensemble dG=%.2f ED=%.2f centroid distance=%.2f" % (r["dG"], r["mean_bp_dist"], r["centroid_dist"]))
        assert_close(emul.pf_long(seq, c), r, "short record %d" % k)


def test_cpu_twin_engine_has_no_pf_long():
    twin = os.path.join(ROOT, "oracle", "libscanfold_cpu.so")
    from oracle import oracle as orc
    orc.build()
    if not os.path.exists(twin):
        pytest.skip("the CPU twin of the C ABI was not built")
    eng = _lib.Engine(device=0, lib_path=twin)
    assert not eng.has_pf_long()
    with pytest.raises(_lib.ScanFoldHipError, match="sf_pf_long"):
        eng.pf_long("ACGU" * 120)
    with pytest.raises(_lib.ScanFoldHipError):
        eng.pf_long_times()


def test_rna_facade_still_refuses(emul, monkeypatch):
    monkeypatch.setattr(_lib, "_engine", emul)
    s = rand_seq(np.random.default_rng(9), 433)
    for call in ("pf", "centroid", "mean_bp_distance"):
        with pytest.raises(NotImplementedError, match="pf_long"):
            getattr(RNA.fold_compound(s), call)()


def test_bad_arguments(emul):
    lib = emul.lib
    s = b"ACGU" * 10
    out = (ctypes.c_double * 3)()
    buf = ctypes.create_string_buffer(41)
    a = [ctypes.addressof(out), ctypes.addressof(out) + 8, ctypes.addressof(buf), ctypes.addressof(out) + 16]
    assert lib.sf_pf_long(s, 0, None, None, *a) == -3
    assert lib.sf_pf_long(s, _lib.SF_MAX_LONG + 1, None, None, *a) == -3
    assert lib.sf_pf_long(None, 40, None, None, *a) == -3
    assert lib.sf_pf_long(s, 40, b"((((" + b"." * 36, None, *a) == -9
    assert lib.sf_strerror(-11).decode().startswith("partition function left the FP64 range")
    with pytest.raises(_lib.ScanFoldHipError):
        emul.pf_long("")
    assert lib.sf_pf_long(s, 40, None, None, None, None, None, None) == 0  # every output is optional
    assert lib.sf_pf_long(s, 40, None, None, *a) == 0 and all(np.isfinite(v) for v in out) and len(buf.value) == 40
    assert set(KEYS) | {"centroid"} == set(emul.pf_long("ACGU" * 10))


def test_unspanned_nested_record(emul, oracle):
    """600 nt without a span, against oracle.pf_cubic in long double: under the emulation's lane budget a group walks several
    cells per launch, here with live data on the long diagonals (the block records above leave them dead)."""
    seq, outer, branches = nested_record(np.random.default_rng(2), 600)
    ref = cubic_reference(oracle, seq, params.default_params())
    assert_carries_weight(ref, outer, branches, 600)
    assert_close(emul.pf_long(seq), ref, "nested 600", ref["bpp"])


# ---- sf_pf_long and a batch of one row: dots as a constraint, L = 1 (run again on the GPU in test_gpu_long_pf.py) ----

def check_a_constraint_of_dots_is_no_constraint(engine):
    """a constraint of dots gives the bits of no constraint at all (a batch does not even set up the arrays for such a row):
    `==` on floats and strings, with and without the MFE as a hint"""
    for L in (57, 433):
        s = rand_seq(np.random.default_rng(100 + L), L)
        e, _ = engine.fold_long(s, structure=False)
        assert engine.pf_long(s, "." * L) == engine.pf_long(s), L
        assert engine.pf_long(s, "." * L, mfe_hint=e) == engine.pf_long(s, mfe_hint=e), L
        row, = engine.pf_long_batch([s], ["." * L], mfe_hints=[e])  # a batch of one row: the same bits
        assert {k: row[k] for k in KEYS + ("centroid",)} == engine.pf_long(s, mfe_hint=e), L


def check_the_shortest_records(engine, oracle):
    """L = 1: no diagonal past d = 0, and no outside launch at all"""
    for L in (1, 4):
        s = rand_seq(np.random.default_rng(100 + L), L)
        ref = oracle.pf(s, want_bpp=True)
        assert_close(engine.pf_long(s), ref, "L=%d" % L, ref["bpp"])
        assert engine.pf_long_times()["attempts"] == 1
        row, = engine.pf_long_batch([s])
        assert {k: row[k] for k in KEYS + ("centroid",)} == engine.pf_long(s), L


def check_failure_leaves_the_callers_buffers_alone(engine):
    """unbalanced brackets end sf_pf_long with SF_ERR_CONSTRAINT and not one byte of the caller's four buffers written; the
    same call without the constraint fills them"""
    s = b"ACGU" * 10
    out = np.frombuffer(b"\x5a" * 24, dtype=np.float64).copy()
    cen = np.frombuffer(b"?" * 41, dtype=np.uint8).copy()
    a = [out[0:].ctypes.data, out[1:].ctypes.data, cen.ctypes.data, out[2:].ctypes.data]
    assert engine.lib.sf_pf_long(s, 40, b"((((" + b"." * 36, None, *a) == -9
    assert out.tobytes() == b"\x5a" * 24 and cen.tobytes() == b"?" * 41
    assert engine.lib.sf_pf_long(s, 40, None, None, *a) == 0
    assert np.isfinite(out).all() and cen[40] == 0 and set(bytes(cen[:40])) <= set(b"().")


def check_one_row_is_the_batchs_row_with_a_retry(engine):
    """the 150-nt row of test_long_pf_batch.test_a_row_that_repeats_leaves_the_others_alone, whose hint is thirty times its
    MFE, folded alone: the single launches repeat the inside pass in the shared loop and end on the bits, the attempts and
    the scale of the batch of that one row"""
    s = rand_seq(np.random.default_rng(77), 150)
    e, _ = engine.fold_long(s, structure=False)
    assert e < -1000
    h = 30 * e
    got = engine.pf_long(s, mfe_hint=h)
    t = engine.pf_long_times()
    assert t["attempts"] > 1
    row, = engine.pf_long_batch([s], mfe_hints=[h])
    assert {k: row[k] for k in KEYS + ("centroid",)} == got
    assert (row["attempts"], row["lns"]) == (t["attempts"], t["lns"])


def test_a_constraint_of_dots_is_no_constraint(emul):
    check_a_constraint_of_dots_is_no_constraint(emul)


def test_failure_leaves_the_callers_buffers_alone(emul):
    check_failure_leaves_the_callers_buffers_alone(emul)


def test_one_row_is_the_batchs_row_with_a_retry(emul):
    check_one_row_is_the_batchs_row_with_a_retry(emul)


def test_the_shortest_records(emul, oracle):
    check_the_shortest_records(emul, oracle)
