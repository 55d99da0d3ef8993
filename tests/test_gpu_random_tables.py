"""The random-table matrix of tests/test_random_tables.py on the MI355X (-m gpu): every MFE instantiation in both kernel modes,
tracebacks, the three partition-function families, constrained folds, max_bp_span, a scan with shuffles over more than 256
windows (shared inside tables), a rescaled temperature, the int16 magnitude boundary, per-type MLintern and a whole-record
fold of 2 000 nt.  MFE batches are larger than the resident grid (four workgroups per CU at W <= 128, two above), so that folds
are handed out dynamically and workgroups fold several sequences in a row."""
import numpy as np
import pytest

from scanfold_amd import params
import pf_util as pu
from conftest import random_seqs
from par_util import SF_FAST_MAXPARAM, boundary_params, plant_specials
from test_random_tables import W_MFE, W_PF, W_TRACE, mlintern_table, rescaled_table, seqs_for, table

pytestmark = pytest.mark.gpu


@pytest.fixture()
def eng(gpu_engine):
    yield gpu_engine
    gpu_engine.set_kernel_mode(0)
    gpu_engine.set_max_bp_span(0)
    gpu_engine.load_params(params.default_params())


@pytest.fixture()
def orc():
    from oracle import oracle as o
    o.build()
    yield o
    o.set_max_bp_span(0)
    o.set_constraint(None, None)
    o.set_params(params.default_params())


def use(eng, orc, p):
    orc.set_params(p)
    eng.load_params(p)


def batch(W):
    return 2500 if W <= 128 else 1200


def check_mfe_both_modes(eng, arr, ref, what):
    try:
        for mode in (0, 1):
            eng.set_kernel_mode(mode)
            got = eng.mfe_batch(arr)
            assert (got == ref).all(), (what, mode, int((got != ref).sum()), len(ref))
    finally:
        eng.set_kernel_mode(0)


def check_sample(eng, orc, arr, what, n=24, pf=True):
    """traceback (and partition function) of every len(arr)/n-th row against the oracle"""
    e, db = eng.mfe_trace_batch(arr)
    assert (e == orc.mfe_batch(arr)).all(), what
    r = eng.pf_batch(arr) if pf else None
    for k in range(0, len(arr), max(1, len(arr) // n)):
        s = bytes(arr[k]).decode()
        assert (db[k], e[k]) == orc.mfe(s), (what, k)
        if pf:
            pu.assert_matches(pu.row(r, k), orc.pf(s), (what, k))


@pytest.mark.parametrize("W", W_MFE)
def test_gpu_mfe_every_instantiation_both_kernel_modes(eng, orc, W):
    for seed in (2 * W, 2 * W + 1):
        p = table(seed)
        use(eng, orc, p)
        arr = seqs_for(p, W, batch(W), seed)
        check_mfe_both_modes(eng, arr, orc.mfe_batch(arr), (W, seed))


@pytest.mark.parametrize("W", W_TRACE)
def test_gpu_traceback(eng, orc, W):
    for seed in (2 * W, 2 * W + 1):
        p = table(seed)
        use(eng, orc, p)
        check_sample(eng, orc, seqs_for(p, W, 512, seed), (W, seed), pf=False)


@pytest.mark.parametrize("W", W_PF)
def test_gpu_partition_function_every_family(eng, orc, W):
    p = table(3 * W)
    use(eng, orc, p)
    arr = seqs_for(p, W, 256, W)
    r = eng.pf_batch(arr)
    assert np.isfinite(r["dG"]).all()
    for k in range(0, len(arr), 16):
        pu.assert_matches(pu.row(r, k), orc.pf(bytes(arr[k]).decode()), (W, k))


@pytest.mark.parametrize("W", [64, 120, 250])
def test_gpu_fold_constrained(eng, orc, W):
    from test_constraints import canonical_constraint
    p = table(6 * W)
    use(eng, orc, p)
    rng = np.random.default_rng(W)
    seqs = [bytes(a).decode() for a in seqs_for(p, W, 300, W)]
    cons = [canonical_constraint(rng, s) for s in seqs]
    r = eng.fold_constrained(seqs, cons)
    for k in range(0, len(seqs), 15):
        orc.set_constraint(cons[k], None)
        assert (r["structure"][k], r["mfe"][k]) == orc.mfe(seqs[k]), (W, k)
        pu.assert_matches(pu.row(r, k), orc.pf(seqs[k]), (W, k))
        orc.set_constraint(None, None)


@pytest.mark.parametrize("W,span", [(120, 50), (200, 70)])
def test_gpu_max_bp_span(eng, orc, W, span):
    p = table(8 * W)
    use(eng, orc, p)
    arr = seqs_for(p, W, batch(W), W)
    try:
        orc.set_max_bp_span(span)
        eng.set_max_bp_span(span)
        check_mfe_both_modes(eng, arr, orc.mfe_batch(arr), W)
        check_sample(eng, orc, arr[:256], W, n=12)
    finally:
        eng.set_max_bp_span(0)
        orc.set_max_bp_span(0)


def test_gpu_scan_with_shuffles_and_shared_inside_tables(eng, orc):
    """sf_scan, step 1 over 400 windows (shared inside tables), four dinucleotide shuffles per window."""
    p = table(10)
    use(eng, orc, p)
    rng = np.random.default_rng(10)
    W, nwin, r = 120, 400, 4
    L = W + nwin - 1
    tr = bytes(plant_specials(rng, random_seqs(rng, 1, L), p, per_row=40)[0]).decode()
    res = eng.scan(tr, W, 1, 0, nwin, r, 1, 17)
    rows = np.frombuffer(b"NACGU", dtype=np.uint8)[eng.shuffle_windows(tr, W, 1, 0, nwin, r, 1, 17)]
    assert (res["energies"].reshape(-1) == orc.mfe_batch(rows)).all()
    for w in range(0, nwin, 13):
        s = tr[w:w + W]
        assert orc.mfe(s)[0] == res["structure"][w], w
        pu.assert_matches(dict(dG=res["ens_dG"][w], mean_bp_dist=res["ens_div"][w], centroid=res["centroid"][w]), orc.pf(s), w)


@pytest.mark.parametrize("seed", [11, 12])
def test_gpu_rescaled_temperature_with_random_enthalpies(eng, orc, seed):
    p = rescaled_table(seed, 50.0)
    use(eng, orc, p)
    for W in (90, 200):
        arr = seqs_for(p, W, batch(W), W)
        check_mfe_both_modes(eng, arr, orc.mfe_batch(arr), W)
        check_sample(eng, orc, arr[:256], W, n=8)


@pytest.mark.parametrize("top", [SF_FAST_MAXPARAM, SF_FAST_MAXPARAM + 1])
def test_gpu_magnitude_boundary_of_the_int16_kernel(eng, orc, top):
    p = boundary_params(13, top)
    use(eng, orc, p)
    for W in (90, 120, 200):
        arr = seqs_for(p, W, batch(W), W)
        check_mfe_both_modes(eng, arr, orc.mfe_batch(arr), (W, top))
        check_sample(eng, orc, arr[:256], (W, top), n=8, pf=False)


def test_gpu_mlintern_of_every_pair_type(eng, orc):
    use(eng, orc, mlintern_table())
    rng = np.random.default_rng(60)
    for W in (60, 120, 200, 300):
        arr = random_seqs(rng, batch(W), W)
        check_mfe_both_modes(eng, arr, orc.mfe_batch(arr), W)
        check_sample(eng, orc, arr[:256], W, n=8, pf=False)


def test_gpu_fold_long_under_a_full_random_table(eng, orc):
    p = table(2000)
    use(eng, orc, p)
    rng = np.random.default_rng(2000)
    s = bytes(plant_specials(rng, random_seqs(rng, 1, 2000), p, per_row=60)[0]).decode()
    db, e = orc.mfe(s)
    assert eng.fold_long(s) == (e, db)
