"""Helpers shared by the whole-record partition-function tests (tests/test_long_pf.py on the CPU emulation,
tests/test_gpu_long_pf.py on the GPU).

The bar is the project's PF_TOL made relative: |got - ref| <= PF_TOL * max(1, |ref|) for dG, mean_bp_dist and centroid_dist
(a 3-kb record's dG is in the thousands; FP64 carries 16 digits whatever the magnitude), and equal centroids except at
pairs whose oracle probability lies within 1e-9 of the 0.5 threshold, at most MAX_EXCUSED positions of them.

The oracle's outside pass is O(n^4), so records past ~520 nt are built from blocks it can still answer: under
max_bp_span = S, blocks joined by runs of S N fold independently (long_util.separated_record shows it for the MFE), so Z is
the product of the blocks' Z — dG, mean_bp_dist and centroid_dist are the sums of the blocks' — and the centroid is the
blocks' centroids joined by dots.  Each block is folded with one flanking N on each inner side, which a stem's exterior
term reads."""
import numpy as np

from long_util import rand_seq
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
