"""Partition functions at the edge of FP64's range on the MI355X (-m gpu): the kernels' flag and the scaled redo
against the long-double reference (pf_util).  See test_pf_range.py for the CPU side."""
import numpy as np
import pytest

from scanfold_amd import params

import pf_util as pu
from pf_util import hp

pytestmark = pytest.mark.gpu


@pytest.fixture()
def eng(gpu_engine):
    yield gpu_engine
    gpu_engine.set_kernel_mode(0)
    gpu_engine.load_params(params.default_params())


def _check_batch(r, seqs, p, what):
    for k, s in enumerate(seqs):
        pu.assert_matches(pu.row(r, k), pu.reference(s, p), (what, k))


def test_gpu_hairpins_300_to_400(eng):
    """hp(W), W in 300..400, on the shipped table through pf_batch, fold_constrained and sf_scan's native windows."""
    dflt = params.default_params()
    eng.load_params(dflt)
    for W in (300, 308, 310, 340, 400):
        seqs = [hp(W), hp(W)[::-1]]
        _check_batch(eng.pf_batch(seqs), seqs, dflt, ("pf_batch", W))
        _check_batch(eng.fold_constrained(seqs, ["." * W] * 2, mfe=False), seqs, dflt, ("fold_constrained", W))
    tr = "AU" + hp(340) + "UA"
    res = eng.scan(tr, 340, 2, 0, 3, 1, 1, 7)
    for w in range(3):
        pu.assert_matches(dict(dG=res["ens_dG"][w], mean_bp_dist=res["ens_div"][w], centroid=res["centroid"][w]),
                          pu.reference(tr[2 * w:2 * w + 340], dflt), ("scan", w))


@pytest.mark.parametrize("mode", [0, 1])
def test_gpu_kernel_families_amplified_and_cold(eng, mode):
    """Stacks x flag_factor(W) and 25 C with synthetic enthalpies: every kernel family and the constrained
    instantiations, in both kernel modes.  The unflagged fold of each batch is bit-identical to the same row alone."""
    eng.set_kernel_mode(mode)
    rng = np.random.default_rng(70 + mode)
    for W in (63, 64, 65, 120, 121, 256, 257, 400):
        amp = pu.amplified(pu.flag_factor(W))
        eng.load_params(amp)
        seqs = [hp(W), pu.low_gc(rng, W)]
        pu.assert_flagged(seqs, amp, [True, False])
        r = eng.pf_batch(seqs)
        alone = eng.pf_batch([seqs[1]])
        for key in ("dG", "mean_bp_dist", "centroid_dist"):
            assert r[key][1] == alone[key][0], (W, key)
        pu.assert_matches(pu.row(r, 0), pu.reference(seqs[0], amp), ("amp", W))
    for W in (64, 120, 250):  # constrained: the LDS HC instantiation at 64 and 120, the device-table one at 250
        amp = pu.amplified(pu.flag_factor(W))
        eng.load_params(amp)
        seqs = [hp(W)]
        _check_batch(eng.fold_constrained(seqs, ["." * W], mfe=False), seqs, amp, ("hc", W))
    cold = pu.cold()
    eng.load_params(cold)
    for W in (256, 280):  # the device-table kernel, the generic one
        seqs = [hp(W)]
        pu.assert_flagged(seqs, cold, [True])
        _check_batch(eng.pf_batch(seqs), seqs, cold, ("cold", W))


@pytest.mark.parametrize("mode,W,n", [(0, 120, 2200), (1, 120, 2200), (0, 257, 1100)])
def test_gpu_mixed_batch_larger_than_the_grid(eng, mode, W, n):
    """More rows than resident workgroups (LDS kernel: one per CU; generic kernel: four per CU), so that workgroups fold
    unflagged rows after flagged ones: the unflagged rows are bit-identical to the same rows without the flagged ones."""
    eng.set_kernel_mode(mode)
    amp = pu.amplified(pu.flag_factor(W))
    eng.load_params(amp)
    rng = np.random.default_rng(5)
    seqs = [pu.low_gc(rng, W) for _ in range(n)]
    flagged = sorted(set(rng.integers(0, n, 12).tolist()))
    for k in flagged:
        seqs[k] = hp(W)
    unflagged = [k for k in range(n) if k not in flagged]
    pu.assert_flagged([hp(W)] + [seqs[k] for k in unflagged[:3]], amp, [True, False, False, False])
    r = eng.pf_batch(seqs)
    alone = eng.pf_batch([seqs[k] for k in unflagged])  # the same rows without the flagged ones
    for key in ("dG", "mean_bp_dist", "centroid_dist"):
        assert np.array_equal(r[key][unflagged], alone[key]), key
    ref_hp = pu.reference(hp(W), amp)
    for k in flagged:
        pu.assert_matches(pu.row(r, k), ref_hp, k)
    assert np.isfinite(r["dG"]).all() and np.isfinite(r["mean_bp_dist"]).all()
    orc = pu.use(amp)
    for k in range(0, n, 197):
        if k not in flagged:
            pu.assert_matches(pu.row(r, k), orc.pf(seqs[k]), k)


@pytest.mark.parametrize("W", [64, 120])
def test_gpu_flagged_window_inside_a_shared_run(eng, W):
    """sf_scan step 1 over > 256 windows (shared inside tables): the window holding the whole hairpin is flagged, its
    neighbours are not; every window equals its stand-alone fold, and the reference near the hairpin."""
    p, core, centre = pu.shared_run_case(W)
    rng = np.random.default_rng(W)
    pre = "".join("AU"[k] for k in rng.integers(0, 2, 300))
    tr = pre + core + pre[::-1]
    eng.load_params(p)
    nwin = len(tr) - W + 1
    res = eng.scan(tr, W, 1, 0, nwin, 1, 1, 5)
    alone = eng.pf_batch([tr[w:w + W] for w in range(nwin)])
    for w in range(nwin):
        assert res["centroid"][w] == alone["centroid"][w], w
        assert abs(res["ens_dG"][w] - alone["dG"][w]) <= 1e-9 and abs(res["ens_div"][w] - alone["mean_bp_dist"][w]) <= 1e-9, w
    for w in range(len(pre) + centre - 2, len(pre) + centre + 3):
        pu.assert_matches(dict(dG=res["ens_dG"][w], mean_bp_dist=res["ens_div"][w], centroid=res["centroid"][w]),
                          pu.reference(tr[w:w + W], p), w)


def test_gpu_device_pointer_path_equals_host_path(eng):
    """sf_scan_dev through torch tensors: the flag list stays on the device; same answer as the host path."""
    import torch
    dflt = params.default_params()
    eng.load_params(dflt)
    tr = "AU" + hp(340) + "UA"
    W, step, n_win, r = 340, 2, 3, 1
    host = eng.scan(tr, W, step, 0, n_win, r, 1, 7)
    dev = torch.device("cuda:0")
    d_tr = torch.tensor(list(tr.encode()), dtype=torch.uint8, device=dev)
    en = torch.zeros(n_win * (r + 1), dtype=torch.int32, device=dev)
    db = torch.zeros(n_win * (W + 1), dtype=torch.uint8, device=dev)
    cen = torch.zeros(n_win * (W + 1), dtype=torch.uint8, device=dev)
    div = torch.zeros(n_win, dtype=torch.float64, device=dev)
    dG = torch.zeros(n_win, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev)
    eng.scan_dev(d_tr.data_ptr(), len(tr), W, step, 0, n_win, r, 1, 7, 0, en.data_ptr(), db.data_ptr(), cen.data_ptr(),
                 div.data_ptr(), dG.data_ptr(), st.cuda_stream)
    torch.cuda.synchronize(dev)
    assert np.array_equal(dG.cpu().numpy(), host["ens_dG"]) and np.array_equal(div.cpu().numpy(), host["ens_div"])
    c = cen.cpu().numpy().reshape(n_win, W + 1)
    assert [bytes(x[:W]).decode() for x in c] == host["centroid"]
    assert np.isfinite(host["ens_dG"]).all()
