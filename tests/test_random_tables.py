"""Every kernel family under fully randomised energy tables (par_util.random_params_full), on the CPU emulation build of the
kernel sources (tests/emul), against the oracle.

The shipped table is smooth and nearly symmetric: a kernel that reads the wrong entry of a table can still get the right answer
on it.  Here every field the model reads is random — loop-size tables, ninio, MLintern per pair type, MLbase / TerminalAU of
either sign, dangles, mismatches, special hairpins (planted in the sequences; table lengths on both sides of the MFE kernel's
blocks of eight keys) — at the widths where the MFE kernel changes instantiation, in both kernel modes, and at the magnitude
boundary of the int16 kernel.  The first tests pin the oracle itself to the independent Python model under the same tables.
The GPU twin of this file is tests/test_gpu_random_tables.py."""
import math
import re

import numpy as np
import pytest

from scanfold_amd import params
import pf_util as pu
import py_model
from conftest import random_seqs
from par_util import (SF_FAST_MAXPARAM, SPECIAL_COUNTS, boundary_params, max_finite_entry, plant_specials, random_enthalpies,
                      random_params_full)

W_MFE = (20, 40, 64, 90, 117, 118, 120, 121, 128, 129, 160, 199, 200, 201, 256, 257, 300)
W_TRACE = (40, 90, 120, 128, 160, 200, 256, 300)
W_PF = (90, 160, 280)  # sf_pf_lds_kernel, sf_pf_fast_kernel, sf_pf_kernel
MULTI = re.compile(r"\([^()]*\([^()]*\)[^()]*\(")  # a pair that closes a multiloop


def table(seed):
    """random_params_full(seed).  Odd seeds keep MLintern per pair type, which sends every width to the int32 kernel
    (sf_fast_build_params), with MLclosing = -200 so that multiloops, where MLintern[type] counts, win often.  Even seeds take
    ONE MLintern for every type (-100 .. 49) and MLclosing 100 .. 499, so that W <= 256 runs on the int16 kernel within its range."""
    p = random_params_full(seed)
    r = p.rec
    if seed % 2:
        r["MLclosing"] = -200
    else:
        r["MLintern"] = int(r["MLintern"][1]) % 150 - 100
        r["MLclosing"] = int(r["MLclosing"]) % 400 + 100
    return p


def seqs_for(p, W, n, seed):
    """n random W-mers (uint8 ASCII) with special hairpins of p planted in them."""
    rng = np.random.default_rng([seed, W])
    return plant_specials(rng, random_seqs(rng, n, W), p, per_row=max(2, W // 30))


def pair_table(db):
    pt, stack = [0] * (len(db) + 2), []
    for k, ch in enumerate(db, 1):
        if ch == "(":
            stack.append(k)
        elif ch == ")":
            a = stack.pop()
            pt[a], pt[k] = k, a
    return pt


@pytest.fixture(scope="module")
def emul():
    from emul_engine import emul_engine
    e = emul_engine()
    yield e
    e.set_kernel_mode(0)
    e.set_max_bp_span(0)
    e.load_params(params.default_params())


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


def check_mfe_both_modes(eng, arr, ref, what):
    try:
        for mode in (0, 1):
            eng.set_kernel_mode(mode)
            got = eng.mfe_batch(arr)
            assert (got == ref).all(), (what, mode, int((got != ref).sum()), len(ref))
    finally:
        eng.set_kernel_mode(0)


def check_trace_and_pf(eng, orc, arr, what, pf=True):
    e, db = eng.mfe_trace_batch(arr)
    r = eng.pf_batch(arr) if pf else None
    for k in range(len(arr)):
        s = bytes(arr[k]).decode()
        assert (db[k], e[k]) == orc.mfe(s), (what, k)
        if pf:
            pu.assert_matches(pu.row(r, k), orc.pf(s), (what, k))


# ---------------------------------------------------------------- the generator
def test_full_random_tables_are_what_they_claim():
    dflt = params.default_params().rec
    seen_counts, signs = set(), set()
    for seed in range(12):
        p = random_params_full(seed)
        r, base = p.rec, params.random_params(seed).rec
        assert (r["stack"] == r["stack"].T).all()
        assert (r["int11"] == r["int11"].transpose(1, 0, 3, 2)).all()
        assert (r["int22"] == r["int22"].transpose(1, 0, 4, 5, 2, 3)).all()
        for f in ("int11", "int21", "int22"):  # random_params' own draws are kept, its stacks halved
            assert (r[f] == base[f]).all(), f
        assert (r["stack"] == base["stack"] // 2).all()
        assert max_finite_entry(r) <= SF_FAST_MAXPARAM
        assert len(set(r["MLintern"][1:8].tolist())) > 1
        for f in ("hairpin", "bulge", "internal_loop", "dangle5", "mismatchM"):
            assert not (r[f] == dflt[f]).all(), f
        for f in ("hairpin", "bulge", "internal_loop"):  # loop sizes that cannot exist stay INF
            assert (r[f][dflt[f] >= params.INF] == params.INF).all(), f
        for fseq, fn, ln in (("tetra_seq", "n_tetra", 6), ("tri_seq", "n_tri", 5), ("hexa_seq", "n_hexa", 8)):
            assert int(r[fn]) in SPECIAL_COUNTS
            seen_counts.add(int(r[fn]))
            keys = [bytes(s).decode() for s in r[fseq]]
            assert len(set(keys)) == params.MAX_SPECIAL and all(len(s) == ln for s in keys)
            assert all((s[0], s[-1]) in py_model.PAIR for s in keys)
        signs.add((int(r["MLbase"]) < 0, int(r["TerminalAU"]) < 0))
        again = random_params_full(seed).rec
        assert all(np.array_equal(r[f], again[f]) for f in r.dtype.names)
    assert {1, 7, 9} <= seen_counts and len(signs) >= 3, (seen_counts, signs)
    assert max_finite_entry(boundary_params(3).rec) == SF_FAST_MAXPARAM
    assert max_finite_entry(boundary_params(3, SF_FAST_MAXPARAM + 1).rec) == SF_FAST_MAXPARAM + 1


# ---------------------------------------------------------------- the model, pinned first
def test_oracle_structures_evaluate_to_their_energy_in_the_python_model(orc):
    """Under 12 full-random tables the oracle's MFE structure, re-evaluated by tests/py_model.py (which shares no code with
    it), gives the oracle's energy: the oracle honours every randomised field, MLintern per pair type included."""
    rng = np.random.default_rng(40)
    n_multi, classes = 0, set()
    for seed in range(12):
        p = table(seed)
        orc.set_params(p)
        model = py_model.Model(p, 37.0, "mfe")
        for _ in range(10):
            s = bytes(plant_specials(rng, random_seqs(rng, 1, int(rng.integers(14, 33))), p)[0]).decode()
            db, e = orc.mfe(s)
            assert int(round(model.energy(s, pair_table(db)))) == e, (seed, s, db, e)
            n_multi += bool(MULTI.search(db))
        classes |= model.seen
    assert n_multi >= 10, n_multi
    assert {"multiloop", "special hairpin 3", "special hairpin 4", "special hairpin 6"} <= classes, sorted(classes)


def test_oracle_partition_function_equals_enumeration(orc):
    """Short sequences under 10 full-random tables: the oracle's partition function equals its exhaustive enumeration
    (ensemble energy, pair probabilities, MFE) and the Python model's own enumeration (ensemble energy, mean base-pair
    distance, MFE)."""
    rng = np.random.default_rng(41)
    kT = py_model.GASCONST * (37.0 + py_model.K0) / 1000.0
    for seed in range(10):
        p = table(seed)
        orc.set_params(p)
        for t in range(6):
            s = bytes(plant_specials(rng, random_seqs(rng, 1, int(rng.integers(10, 17))), p, per_row=1)[0]).decode()
            be, Z, bpp, _ = orc.brute(s, True)
            r = orc.pf(s, True)
            assert abs(-math.log(Z) * kT - r["dG"]) < 1e-9, (seed, s)
            assert np.abs(bpp - r["bpp"]).max() < 1e-9, (seed, s)
            assert be == orc.mfe(s)[1], (seed, s)
            if t < 2:
                dg, dist, _, mfe, _, _ = py_model.ensemble(p, s, 37.0)
                assert abs(dg - r["dG"]) < 1e-9 * max(1.0, abs(dg)) and abs(dist - r["mean_bp_dist"]) < 1e-9, (seed, s)
                assert mfe == be, (seed, s)


# ---------------------------------------------------------------- the kernels
@pytest.mark.parametrize("W", W_MFE)
def test_mfe_every_instantiation_both_kernel_modes(emul, orc, W):
    for seed in (2 * W, 2 * W + 1):
        p = table(seed)
        use(emul, orc, p)
        arr = seqs_for(p, W, 6 if W <= 128 else 3, seed)
        ref = orc.mfe_batch(arr)
        if seed % 2 == 0:  # the int16 kernel's table: every fold inside its range, none takes the overflow way
            assert (ref > -11000).all(), ref
        check_mfe_both_modes(emul, arr, ref, (W, seed))


@pytest.mark.parametrize("W", W_TRACE)
def test_traceback(emul, orc, W):
    for seed in (2 * W, 2 * W + 1):
        p = table(seed)
        use(emul, orc, p)
        check_trace_and_pf(emul, orc, seqs_for(p, W, 3, seed), (W, seed), pf=False)


@pytest.mark.parametrize("W", W_PF)
def test_partition_function_every_family(emul, orc, W):
    p = table(3 * W)
    use(emul, orc, p)
    arr = seqs_for(p, W, 2, W)
    r = emul.pf_batch(arr)
    for k in range(len(arr)):
        pu.assert_matches(pu.row(r, k), orc.pf(bytes(arr[k]).decode()), (W, k))


@pytest.mark.parametrize("W", [64, 120, 250])
def test_fold_constrained(emul, orc, W):
    """sf_fold_constrained: the LDS hard-constraint instantiations at 64 / 120; at 250 the last width of the constrained LDS
    MFE kernel and the device-table partition function."""
    from test_constraints import canonical_constraint
    p = table(6 * W)
    use(emul, orc, p)
    rng = np.random.default_rng(W)
    seqs = [bytes(a).decode() for a in seqs_for(p, W, 2, W)]
    cons = [canonical_constraint(rng, s) for s in seqs]
    r = emul.fold_constrained(seqs, cons)
    for k, (s, c) in enumerate(zip(seqs, cons)):
        orc.set_constraint(c, None)
        assert (r["structure"][k], r["mfe"][k]) == orc.mfe(s), (W, k)
        pu.assert_matches(pu.row(r, k), orc.pf(s), (W, k))
        orc.set_constraint(None, None)


@pytest.mark.parametrize("W,span", [(120, 50), (200, 70)])
def test_max_bp_span(emul, orc, W, span):
    p = table(8 * W)
    use(emul, orc, p)
    arr = seqs_for(p, W, 3, W)
    try:
        orc.set_max_bp_span(span)
        emul.set_max_bp_span(span)
        check_mfe_both_modes(emul, arr, orc.mfe_batch(arr), W)
        check_trace_and_pf(emul, orc, arr[:2], W)
    finally:
        emul.set_max_bp_span(0)
        orc.set_max_bp_span(0)


def test_scan_with_shuffles_and_shared_inside_tables(emul, orc):
    """sf_scan with step 1 (consecutive native windows share their inside tables) and two dinucleotide shuffles per window."""
    p = table(10)
    use(emul, orc, p)
    rng = np.random.default_rng(10)
    W, L, r = 64, 100, 2
    tr = bytes(plant_specials(rng, random_seqs(rng, 1, L), p, per_row=6)[0]).decode()
    nwin = L - W + 1
    res = emul.scan(tr, W, 1, 0, nwin, r, 1, 17)
    rows = np.frombuffer(b"NACGU", dtype=np.uint8)[emul.shuffle_windows(tr, W, 1, 0, nwin, r, 1, 17)]
    assert (res["energies"].reshape(-1) == orc.mfe_batch(rows)).all()
    for w in range(nwin):
        s = tr[w:w + W]
        assert orc.mfe(s)[0] == res["structure"][w], w
        pu.assert_matches(dict(dG=res["ens_dG"][w], mean_bp_dist=res["ens_div"][w], centroid=res["centroid"][w]), orc.pf(s), w)


def rescaled_table(seed, T):
    """table(seed) with random enthalpies, rescaled to T through ParamSet.at_temperature: MLintern stays one value for every
    pair type on even seeds (the int16 kernel), per type on odd ones."""
    base = table(seed)
    dH = random_enthalpies(base.rec, seed)
    if seed % 2 == 0:
        dH["MLintern"] = dH["MLintern"][1]
    p = params.ParamSet(base.rec.copy(), base.source, dH).at_temperature(T)
    assert (len(set(p.rec["MLintern"][1:8].tolist())) > 1) == bool(seed % 2)
    return p


@pytest.mark.parametrize("seed", [11, 12])
def test_rescaled_temperature_with_random_enthalpies(emul, orc, seed):
    p = rescaled_table(seed, 50.0)
    use(emul, orc, p)
    for W in (90, 200):
        arr = seqs_for(p, W, 3, W)
        check_mfe_both_modes(emul, arr, orc.mfe_batch(arr), W)
        check_trace_and_pf(emul, orc, arr[:2], W)


@pytest.mark.parametrize("top", [SF_FAST_MAXPARAM, SF_FAST_MAXPARAM + 1])
def test_magnitude_boundary_of_the_int16_kernel(emul, orc, top):
    """Entries at exactly +SF_FAST_MAXPARAM (the int16 kernel) and one entry past it (the int32 kernel at every width) on
    ninio / max_ninio, internal_loop, mismatchI and the hairpin sizes: exact MFE and traceback."""
    p = boundary_params(13, top)
    assert max_finite_entry(p.rec) == top
    use(emul, orc, p)
    for W in (90, 120, 200):
        arr = seqs_for(p, W, 4, W)
        check_mfe_both_modes(emul, arr, orc.mfe_batch(arr), (W, top))
        check_trace_and_pf(emul, orc, arr[:2], (W, top), pf=False)


def mlintern_table():
    """The shipped table with MLintern 0 / -90 (CG, GC) / -300 (every other type) and MLclosing = -200."""
    p = params.default_params()
    p.rec["MLintern"] = [0, -90, -90, -300, -300, -300, -300, -300]
    p.rec["MLclosing"] = -200
    return p


def test_mlintern_of_every_pair_type(emul, orc):
    """The int16 kernel once added MLintern[1] for every pair type (multiloop closing term, stems, traceback) while every other
    kernel used MLintern[type]."""
    p = mlintern_table()
    use(emul, orc, p)
    rng = np.random.default_rng(60)
    for W in (60, 120, 200, 300):
        arr = random_seqs(rng, 8, W)
        check_mfe_both_modes(emul, arr, orc.mfe_batch(arr), W)
        check_trace_and_pf(emul, orc, arr[:3], W, pf=False)
