"""Partition functions at the edge of FP64's range (CPU: the oracle, the CPU twin, the emulation build of the kernels).

Z passes DBL_MAX once the ensemble free energy passes kT ln(DBL_MAX) (~437 kcal/mol at 37 C); the outside pass
overflows some 10 kcal/mol earlier.  Every FP64 engine folds unscaled and redoes a fold whose ln Z passes 600 with a
per-nucleotide scale.  The reference is the oracle built with long double accumulators, unscaled (pf_util)."""
import math

import numpy as np
import pytest

from scanfold_amd import params

import pf_util as pu
from pf_util import hp

KT37 = (37 + 273.15) * 1.98717 / 1000.0


def rseq(rng, n, p=None):
    return "".join("ACGU"[k] for k in rng.choice(4, n, p=p))


# ---------------------------------------------------------------- the reference's premise
def test_long_reference_equals_the_double_oracle_in_range():
    """Where FP64 is far from its limits the long-double build gives the double oracle's answer (V3 / twin inputs)."""
    dflt = params.default_params()
    orc = pu.use(dflt)
    rng = np.random.default_rng(3)
    seqs = [rseq(rng, int(rng.integers(8, 18))) for _ in range(30)]
    seqs += [rseq(rng, W) for W in (16, 30, 61, 120, 200)]
    for s in seqs:
        a, b = orc.pf(s), orc.pf(s, precision="long")
        assert abs(a["dG"] - b["dG"]) <= 1e-12 * max(1.0, abs(b["dG"])), s
        assert abs(a["mean_bp_dist"] - b["mean_bp_dist"]) <= 1e-12 * max(1.0, b["mean_bp_dist"]), s
        assert a["centroid"] == b["centroid"], s


@pytest.mark.parametrize("n", [14, 16, 18])
def test_long_reference_equals_long_enumeration_past_double_range(n):
    """Under stacks x 40 the Boltzmann sum of these short sequences is past DBL_MAX: the double enumeration returns
    inf, while the long-double PF equals the long-double enumeration (ensemble energy and pair probabilities).  A
    reference built with double accumulators fails here through the overflow itself."""
    p = pu.amplified(40)
    orc = pu.use(p)
    rng = np.random.default_rng(n)
    for s in (hp(n), pu.gc_rich(rng, n, 0.95)):
        _, Z, _, _ = orc.brute(s)
        if s == hp(n):
            assert math.isinf(Z), (s, Z)
        e = orc.brute(s, want_bpp=True, precision="long")
        r = orc.pf(s, want_bpp=True, precision="long")
        assert np.isfinite(r["dG"]) and abs(r["dG"] - e["dG"]) <= 1e-9 * abs(e["dG"]), (s, r["dG"], e["dG"])
        assert np.abs(r["bpp"] - e["bpp"]).max() < 1e-9, s
        if math.isinf(Z):
            assert -e["dG"] / KT37 > 709.8, s  # ln Z past ln(DBL_MAX)


# ---------------------------------------------------------------- the FP64 oracle, scaled
@pytest.mark.parametrize("W", [300, 306, 308, 310, 340, 400])
def test_double_oracle_is_scaled_past_the_threshold(W):
    """hp(W) on the shipped table: both sides of the flag threshold (ln Z = 600 near W = 256) and of true overflow
    (W >= 310; the outside pass already at 308)."""
    dflt = params.default_params()
    orc = pu.use(dflt)
    s = hp(W)
    ref = pu.reference(s, dflt)
    pu.assert_matches(orc.pf(s), ref, W)
    raw = orc.pf_unscaled(s)
    if W >= 308:  # what the scale-free fold would have returned
        assert not (np.isfinite(raw["dG"]) and np.isfinite(raw["mean_bp_dist"])), (W, raw)


def test_double_oracle_amplified_and_cold_tables():
    rng = np.random.default_rng(5)
    amp = pu.amplified(4)
    orc = pu.use(amp)
    for W in (40, 64, 92, 120):
        for s in (hp(W), pu.gc_rich(rng, W)):
            pu.assert_matches(orc.pf(s), pu.reference(s, amp), W)
    cold = pu.cold()
    orc = pu.use(cold)
    for W in (256, 280):
        s = hp(W)
        assert not orc.pf_unscaled(s)["lnZ"] <= 600  # past the threshold at 25 C
        pu.assert_matches(orc.pf(s), pu.reference(s, cold), W)


# ---------------------------------------------------------------- the CPU twin
@pytest.fixture(scope="module")
def cpu_engine():
    from scanfold_amd import _lib
    from test_cpu_twin_abi import CPU_LIB
    from oracle import oracle as orc
    orc.build()
    return _lib.Engine(device=0, lib_path=CPU_LIB)


def test_cpu_twin_through_the_c_abi(cpu_engine):
    """libscanfold_cpu.so: pf_batch, fold_constrained (all '.', and bracket pairs) and sf_scan on folds past the range."""
    dflt = params.default_params()
    cpu_engine.load_params(dflt)
    seqs = [hp(340), pu.gc_rich(np.random.default_rng(9), 340, 0.4)]
    r = cpu_engine.pf_batch(seqs)
    refs = [pu.reference(s, dflt) for s in seqs]
    for k in range(2):
        pu.assert_matches(pu.row(r, k), refs[k], k)
    cons = ["." * 340] * 2
    r = cpu_engine.fold_constrained(seqs, cons, mfe=False)
    for k in range(2):
        pu.assert_matches(pu.row(r, k), refs[k], k)
    c = "((" + "." * 330 + "))......"
    r = cpu_engine.fold_constrained([hp(340)], [c], mfe=False)
    pu.assert_matches(pu.row(r, 0), pu.reference(hp(340), dflt, cons=c), "cons")
    tr = "AU" + hp(340) + "UA"
    res = cpu_engine.scan(tr, 340, 2, 0, 3, 1, 1, 7)
    for w in range(3):
        ref = pu.reference(tr[2 * w:2 * w + 340], dflt)
        pu.assert_matches(dict(dG=res["ens_dG"][w], mean_bp_dist=res["ens_div"][w], centroid=res["centroid"][w]), ref, w)


def test_cpu_twin_baseline_engine_is_scaled():
    """sf_cpu_twin.c's own PF (bench.py's CPU baseline)."""
    dflt = params.default_params()
    orc = pu.use(dflt)
    rows = np.frombuffer((hp(310) + hp(310)[::-1]).encode(), dtype=np.uint8).reshape(2, 310)
    out = orc.twin_scan_windows(rows, 1, 1)
    ref = pu.reference(hp(310), dflt)
    pu.assert_matches(dict(mean_bp_dist=out["ens_div"][0], centroid=out["centroid"][0]), ref)


# ---------------------------------------------------------------- the kernels (emulation build)
@pytest.fixture(scope="module")
def emul():
    from emul_engine import emul_engine
    return emul_engine()


def _emul_rows(W, mode):
    """Rows per batch so that the last one runs in workgroup 0 right after the flagged row 0.  The emulation has two
    CUs: LDS kernel (W <= 120) grid 2, device-table kernel grid 8 (W <= 128) or 4, generic kernel grid 8."""
    if mode == 1 or W > 256:
        return 9
    if W <= 120:
        return 3
    return 9 if W <= 128 else 5


def _mixed(W, n, rng):
    """Two flagged folds (hp(W) and its reverse), then n - 2 AU-rich unflagged ones."""
    return [hp(W), hp(W)[::-1]] + [pu.low_gc(rng, W) for _ in range(n - 2)]


@pytest.mark.parametrize("mode", [0, 1])
def test_emul_kernel_families_amplified(emul, mode):
    """Stacks x flag_factor(W): the LDS kernel (63, 64, 65, 92, 120), the device-table kernel (121, 256), its
    constrained instantiation (250) and the generic kernel (257, 400; kernel mode 1: every width).  Each batch is longer
    than the kernel's grid, so that workgroup 0 folds an unflagged row right after an overflowed one; every unflagged
    row is bit-identical to the same row folded alone, every flagged one equals the reference."""
    emul.set_kernel_mode(mode)
    try:
        rng = np.random.default_rng(40 + mode)
        for W in (63, 64, 65, 92, 120, 121, 256, 257, 400):
            if mode == 1 and W in (92, 256, 257, 400):
                continue
            p = pu.amplified(pu.flag_factor(W))
            emul.load_params(p)
            seqs = _mixed(W, _emul_rows(W, mode), rng) if W < 400 else _mixed(W, 3, rng)
            pu.assert_flagged(seqs[:3], p, [True, True, False])
            r = emul.pf_batch(seqs)
            last = len(seqs) - 1
            alone = emul.pf_batch([seqs[last]])
            for key in ("dG", "mean_bp_dist", "centroid_dist"):
                assert r[key][last] == alone[key][0], (W, key)
            assert r["centroid"][last] == alone["centroid"][0]
            for k in (0, 1):
                pu.assert_matches(pu.row(r, k), pu.reference(seqs[k], p), (W, k))
            assert np.isfinite(r["dG"]).all() and np.isfinite(r["mean_bp_dist"]).all()
        if mode == 0:  # the constrained device-table instantiation (grid 4)
            W = 250
            p = pu.amplified(4)
            emul.load_params(p)
            seqs = _mixed(W, 5, rng)
            r = emul.fold_constrained(seqs, ["." * W] * 5, mfe=False)
            alone = emul.fold_constrained([seqs[4]], ["." * W], mfe=False)
            assert r["dG"][4] == alone["dG"][0] and r["mean_bp_dist"][4] == alone["mean_bp_dist"][0]
            for k in (0, 1):
                pu.assert_matches(pu.row(r, k), pu.reference(seqs[k], p), ("hc", k))
    finally:
        emul.set_kernel_mode(0)
        emul.load_params(params.default_params())


@pytest.mark.parametrize("W", [64, 120])
def test_emul_flagged_window_inside_a_shared_run(emul, W):
    """sf_scan step 1: consecutive windows share their inside tables.  The window that holds the whole hairpin is
    flagged, its neighbours are not: every window equals its stand-alone fold and the reference."""
    p, tr, centre = pu.shared_run_case(W)
    emul.load_params(p)
    try:
        nwin = len(tr) - W + 1
        res = emul.scan(tr, W, 1, 0, nwin, 1, 1, 5)
        alone = emul.pf_batch([tr[w:w + W] for w in range(nwin)])
        for w in range(nwin):
            assert res["centroid"][w] == alone["centroid"][w], w
            assert abs(res["ens_dG"][w] - alone["dG"][w]) <= 1e-9 and abs(res["ens_div"][w] - alone["mean_bp_dist"][w]) <= 1e-9, w
            ref = pu.reference(tr[w:w + W], p)
            pu.assert_matches(dict(dG=res["ens_dG"][w], mean_bp_dist=res["ens_div"][w], centroid=res["centroid"][w]), ref, w)
    finally:
        emul.load_params(params.default_params())


def test_emul_overflowed_window_inside_a_shared_run(emul):
    """sf_scan, step 16 at W = 64 (shared inside tables, runs of three windows under the emulation's two CUs): window 1
    holds the whole hairpin and overflows FP64 outright; window 2 resumes from its tables.  Every window equals its
    stand-alone fold and the reference."""
    W, step = 64, 16
    p = pu.amplified(pu.flag_factor(W))
    tr = "A" * step + hp(W) + "A" * (3 * step)
    nwin = (len(tr) - W) // step + 1
    orc = pu.use(p)
    assert not np.isfinite(orc.pf_unscaled(tr[step:step + W])["lnZ"])
    emul.load_params(p)
    try:
        res = emul.scan(tr, W, step, 0, nwin, 1, 1, 5)
        alone = emul.pf_batch([tr[w * step:w * step + W] for w in range(nwin)])
        for w in range(nwin):
            s = tr[w * step:w * step + W]
            assert res["centroid"][w] == alone["centroid"][w], w
            assert abs(res["ens_dG"][w] - alone["dG"][w]) <= 1e-9 and abs(res["ens_div"][w] - alone["mean_bp_dist"][w]) <= 1e-9, w
            pu.assert_matches(dict(dG=res["ens_dG"][w], mean_bp_dist=res["ens_div"][w], centroid=res["centroid"][w]),
                              pu.reference(s, p), w)
    finally:
        emul.load_params(params.default_params())


def test_scan_command_line_on_the_cpu_twin_past_the_range(tmp_path):
    """The TSV writer at W = 340 over a GC-hairpin record (libscanfold_cpu.so behind the CLI): no `nan` anywhere, and the
    ED and centroid columns equal the reference rounded as the writer rounds (round(x, 2))."""
    import os
    import subprocess
    import sys
    from test_cpu_twin_abi import CPU_LIB, ROOT
    W, step = 340, 5
    seq = "AUAUA" + hp(W) + "UAUAU"
    fa = tmp_path / "gc.fa"
    fa.write_text(">gc GC hairpin record\n" + seq + "\n")
    out = tmp_path / "gc.tsv"
    p = subprocess.run([sys.executable, "-m", "scanfold_amd.scan", "-i", str(fa), "-w", str(W), "-s", str(step), "-r", "2",
                        "-type", "mono", "--seed", "7", "-o", str(out)], cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, SCANFOLD_LIB_PATH=CPU_LIB, SCANFOLD_DEVICE="0"), timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    text = out.read_text()
    assert "nan" not in text.lower() and "inf" not in text.lower()
    rows = [ln.split("\t") for ln in text.split("\n")[1:] if ln]
    assert len(rows) == (len(seq) - W) // step + 1
    dflt = params.default_params()
    for row in rows:
        i = int(row[0]) - 1
        ref = pu.reference(seq[i:i + W], dflt)
        assert row[6] == str(round(ref["mean_bp_dist"], 2)), (i, row[6], ref["mean_bp_dist"])
        assert row[9] == ref["centroid"], i
