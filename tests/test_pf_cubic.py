"""oracle.pf_cubic, the O(n^3) whole-record reference (sfo_pf_cubic: outside tables for qm and qm1), against the O(n^4)
oracle.pf it stands in for past ~520 nt, in both precisions, and against the enumeration of every structure at <= 18 nt.

The bar is the project's PF_TOL, relative as in long_pf_util.assert_close, on dG, mean_bp_dist and centroid_dist, absolute
on every pair probability; centroids are equal outright."""
import numpy as np
import pytest

from scanfold_amd import params
import pf_util
from long_pf_util import KEYS, gc_only
from long_util import pair_table, rand_seq
from test_gpu_parity import PF_TOL
from test_long_fold import constraint_string, planted_stem

PRECISIONS = ("double", "long")
worst = {}  # the largest differences seen, printed as they grow


def note(key, v):
    worst[key] = max(worst.get(key, 0.0), float(v))
    print("largest so far: " + ", ".join("%s %.3g" % kv for kv in sorted(worst.items())))


def both(orc, s, cons=None, span=0, what=""):
    """pf_cubic against pf on s in both precisions, under the parameter set resident in orc's two libraries"""
    for prec in PRECISIONS:
        orc.set_constraint(cons, precision=prec)
        orc.set_max_bp_span(span, precision=prec)
        try:
            ref = orc.pf(s, want_bpp=True, precision=prec)
            got = orc.pf_cubic(s, want_bpp=True, precision=prec)
        finally:
            orc.set_constraint(None, precision=prec)
            orc.set_max_bp_span(0, precision=prec)
        for key in KEYS:
            d = abs(got[key] - ref[key])
            print("%s %s %s cubic=%.15g pf=%.15g diff=%.3g" % (what, prec, key, got[key], ref[key], d))
            assert np.isfinite(got[key]) and d <= PF_TOL * max(1.0, abs(ref[key])), (what, prec, key, got[key], ref[key])
            note(key + " (relative)", d / max(1.0, abs(ref[key])))
        d = float(np.abs(got["bpp"] - ref["bpp"]).max())
        assert d <= PF_TOL, (what, prec, d)
        note("bpp", d)
        assert got["centroid"] == ref["centroid"], (what, prec)
    return got


@pytest.fixture()
def orc(oracle):
    yield pf_util.use(params.default_params())
    pf_util.use(params.default_params())


@pytest.mark.parametrize("L", [1, 4, 5, 57, 120, 257, 400])
def test_default_tables(orc, L):
    both(orc, rand_seq(np.random.default_rng(700 + L), L), what="L=%d" % L)


@pytest.mark.parametrize("L", [57, 257])
def test_randomised_parameter_set(orc, L):
    pf_util.use(params.random_params(3))
    both(orc, rand_seq(np.random.default_rng(3 + L), L), what="random_params(3) L=%d" % L)


def test_rescaled_temperature_set(orc):
    pf_util.use(pf_util.cold())
    both(orc, rand_seq(np.random.default_rng(25), 257), what="25 C")


def test_span_on_a_planted_stem(orc):
    s = planted_stem(np.random.default_rng(5), 257)
    free = both(orc, s, what="planted stem")
    cut = both(orc, s, span=50, what="planted stem, span 50")
    assert free["centroid"].startswith("((((") and free["centroid"].endswith("))))")
    assert all(j - i < 50 for i, j in pair_table(cut["centroid"]).items())  # the span removes the stem


@pytest.mark.parametrize("L", [120, 257])
def test_constraint(orc, L):
    rng = np.random.default_rng(30 + L)
    s = rand_seq(rng, L)
    cons = constraint_string(s, rng)
    assert set("x<>()") <= set(cons)
    both(orc, s, cons=cons, what="constrained L=%d" % L)


def test_past_the_range_of_double(orc):
    s = gc_only()
    assert not orc.pf_unscaled(s)["lnZ"] <= 709.0  # the FP64 build has to scale
    both(orc, s, what="GC 480")


def test_run_of_60_n(orc):
    rng = np.random.default_rng(60)
    both(orc, rand_seq(rng, 100) + "N" * 60 + rand_seq(rng, 97), what="60 N")


@pytest.mark.parametrize("case", ["default", "random_params", "cold", "constraint", "span", "N run"])
def test_against_the_enumeration(orc, case):
    """Every structure of a sequence of <= 18 nt, summed in long double (oracle.brute), as test_oracle.py does for pf."""
    rng = np.random.default_rng(len(case))
    if case == "random_params":
        pf_util.use(params.random_params(3))
    if case == "cold":
        pf_util.use(pf_util.cold())
    for L in (8, 13, 16, 18):
        s = rand_seq(rng, L, "GC" if L == 16 else "ACGU")
        if case == "N run":
            s = s[:L // 2] + "NN" + s[L // 2 + 2:]
        cons = None
        if case == "constraint":
            cons = "".join(rng.choice(list("..<>x"), L))
            a = int(rng.integers(0, L - 7))
            cons = cons[:a] + "(" + cons[a + 1:a + 7] + ")" + cons[a + 8:]
        S = 9 if case == "span" else 0
        for prec in PRECISIONS:
            orc.set_constraint(cons, precision=prec)
            orc.set_max_bp_span(S, precision=prec)
        try:
            ref = orc.brute(s, want_bpp=True, precision="long")
            for prec in PRECISIONS:
                got = orc.pf_cubic(s, want_bpp=True, precision=prec)
                d, dp = abs(got["dG"] - ref["dG"]), float(np.abs(got["bpp"] - ref["bpp"]).max())
                print("%s L=%d %s dG diff=%.3g bpp diff=%.3g" % (case, L, prec, d, dp))
                assert d <= PF_TOL and dp <= PF_TOL, (case, L, prec, d, dp)
                note("dG vs enumeration", d)
                note("bpp vs enumeration", dp)
        finally:
            for prec in PRECISIONS:
                orc.set_constraint(None, precision=prec)
                orc.set_max_bp_span(0, precision=prec)
