"""Helpers shared by the whole-record partition-function tests (tests/test_long_pf.py on the CPU emulation,
tests/test_gpu_long_pf.py on the GPU).

The bar is the project's PF_TOL made relative: |got - ref| <= PF_TOL * max(1, |ref|) for dG, mean_bp_dist and centroid_dist
(a 3-kb record's dG is in the thousands; FP64 carries 16 digits whatever the magnitude), and equal centroids except at
pairs whose oracle probability lies within 1e-9 of the 0.5 threshold, at most MAX_EXCUSED positions of them.

The outside pass of oracle.pf is O(n^4).  Whole records past ~520 nt without a span are checked against oracle.pf_cubic in
long double (cubic_reference), whose O(n^3) outside pass tests/test_pf_cubic.py proves against oracle.pf; nested_record
builds inputs whose long diagonals carry weight.  Longer records are built from blocks oracle.pf can still answer: under
max_bp_span = S, blocks joined by runs of S N fold independently (long_util.separated_record shows it for the MFE), so Z is
the product of the blocks' Z — dG, mean_bp_dist and centroid_dist are the sums of the blocks' — and the centroid is the
blocks' centroids joined by dots.  Each block is folded with one flanking N on each inner side, which a stem's exterior
term reads."""
import numpy as np
import pytest

from scanfold_amd import params
from long_util import COMP, hairpin_rich, pair_table, rand_seq
from test_gpu_parity import PF_TOL

MAX_EXCUSED = 2
KEYS = ("dG", "mean_bp_dist", "centroid_dist")


def assert_close(got, ref, what="", bpp=None):
    """got: one pf_long result; ref: dict(dG, mean_bp_dist, centroid_dist, centroid); bpp: the oracle's pair probabilities
    (1-based square matrix) where the centroid may be excused at |p - 0.5| <= 1e-9.  Prints each figure before asserting."""
    for key in KEYS:
        v, r = float(got[key]), float(ref[key])
        print("%s %s got=%.15g ref=%.15g diff=%.3g bar=%.3g" % (what, key, v, r, abs(v - r), PF_TOL * max(1.0, abs(r))))
        assert np.isfinite(v), (what, key, v)
        assert abs(v - r) <= PF_TOL * max(1.0, abs(r)), (what, key, v, r)
    g, c = got["centroid"], ref["centroid"]
    assert len(g) == len(c), (what, len(g), len(c))
    diff = [k for k in range(len(c)) if g[k] != c[k]]
    if diff:
        assert bpp is not None and len(diff) <= MAX_EXCUSED, (what, diff[:10])
        for k in diff:  # a differing position must belong to a pair on the threshold
            near = np.abs(np.maximum(bpp[k + 1, :], bpp[:, k + 1]) - 0.5) <= 1e-9
            assert near.any(), (what, k)


def oracle_pf(oracle, seq, cons=None, want_bpp=False):
    oracle.set_constraint(cons)
    try:
        return oracle.pf(seq, want_bpp=want_bpp)
    finally:
        oracle.set_constraint(None)


def block_record(oracle, block_lens, S, seed, fill):
    """-> (seq, ref, blocks): blocks of the given lengths from fill(rng, n) joined by S N; ref = the record's exact
    dict(dG, mean_bp_dist, centroid_dist, centroid, lnZ_over_kT) under max_bp_span = S from the oracle's folds of the blocks;
    blocks = [(start, length, block ref)]."""
    rng = np.random.default_rng(seed)
    blocks = [fill(rng, n) for n in block_lens]
    seq = ("N" * S).join(blocks)
    ref = dict(dG=0.0, mean_bp_dist=0.0, centroid_dist=0.0)
    cens, out, pos = [], [], 0
    oracle.set_max_bp_span(S)
    try:
        for b, blk in enumerate(blocks):
            left = "N" if b > 0 else ""
            right = "N" if b < len(blocks) - 1 else ""
            r = oracle.pf(left + blk + right)
            cen = r["centroid"][len(left):len(left) + len(blk)]
            for key in KEYS:
                ref[key] += r[key]
            cens.append(cen)
            out.append((pos, len(blk), dict(r, centroid=cen)))
            pos += len(blk) + S
    finally:
        oracle.set_max_bp_span(0)
    ref["centroid"] = ("." * S).join(cens)
    assert len(ref["centroid"]) == len(seq)
    return seq, ref, out


def gc_only(L=480):
    """the G/C-only sequence whose unscaled partition function leaves FP64's range (ln Z ~ 742)"""
    return rand_seq(np.random.default_rng(2), L, "GC")


def nested_record(rng, L):
    """-> (seq, outer, branches): a record of exactly L nt whose top diagonals are live.  A G/C stem of 12 pairs joins its two
    ends and closes a multiloop of three branches, each a hairpin_rich stretch of about L/3 closed by a G/C stem of 10 pairs,
    with two A between the stems.  outer and branches[k] list the planted pairs (0-based, outermost first)."""
    def helix(n):
        a = rand_seq(rng, n, "GC")
        return a, a[::-1].translate(COMP)
    room = L - 2 * 12 - 4 * 2 - 3 * 2 * 10
    lens = [room // 3, room // 3, room - 2 * (room // 3)]
    o5, o3 = helix(12)
    seq, branches = o5, []
    for m in lens:
        b5, b3 = helix(10)
        start = len(seq) + 2
        seq += "AA" + b5 + hairpin_rich(rng, m) + b3
        branches.append([(start + k, len(seq) - 1 - k) for k in range(10)])
    seq += "AA" + o3
    assert len(seq) == L
    return seq, [(k, L - 1 - k) for k in range(12)], branches


_cubic = {}


@pytest.fixture(scope="module", autouse=True)
def forget_cubic_references():
    """A module that imports this fixture drops its references when its last test has run: each keeps a whole bpp matrix
    (36 MB at 2 112 nt), which no later module reads."""
    yield
    _cubic.clear()


def cubic_reference(oracle, seq, paramset, cons=None, span=0):
    """oracle.pf_cubic(seq, want_bpp=True, precision="long") under paramset, constraint and span, computed once per module run:
    dict(dG, mean_bp_dist, centroid_dist, centroid, bpp).  The long-double library keeps its own tables, span and constraint;
    they are set for the call, and the default set, no constraint and no span are put back."""
    key = (seq, paramset.blob(), cons, span)
    if key not in _cubic:
        oracle.set_params(paramset, L=oracle.lib_long())
        oracle.set_constraint(cons, precision="long")
        oracle.set_max_bp_span(span, precision="long")
        try:
            _cubic[key] = oracle.pf_cubic(seq, want_bpp=True, precision="long")
        finally:
            oracle.set_constraint(None, precision="long")
            oracle.set_max_bp_span(0, precision="long")
            oracle.set_params(params.default_params(), L=oracle.lib_long())
    return _cubic[key]


def assert_carries_weight(ref, outer, branches, L):
    """The reference of a nested_record must itself depend on the long diagonals: the outermost planted pair is likelier than
    not, the centroid holds a pair spanning all but 40 nt and a planted pair of every branch, and no probability lies within
    1e-6 of the centroid's threshold, so that assert_close has nothing to excuse."""
    bpp, pt = ref["bpp"], pair_table(ref["centroid"])
    assert bpp[outer[0][0] + 1, outer[0][1] + 1] > 0.5, bpp[outer[0][0] + 1, outer[0][1] + 1]
    assert any(j - i >= L - 40 for i, j in pt.items())
    for b, pairs in enumerate(branches):
        assert any(pt.get(i) == j for i, j in pairs), b
    gap = float(np.abs(bpp - 0.5).min())
    print("closest probability to 0.5: |p - 0.5| = %.3g" % gap)
    assert gap > 1e-6, gap
