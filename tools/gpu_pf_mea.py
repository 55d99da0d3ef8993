"""The maximum-expected-accuracy structure of a whole record under a span (sf_pf_banded_mea) against sf_pf_banded_probs
alone, on one GPU.

Points: the seeded random records of tools/gpu_pf_probs.py (4 000 and 10 000 nt under spans 120 and 600; 29 903, 100 000
and 500 000 nt under span 600), each with its MFE (fold_banded's) as hint, cutoff 0.01, gamma 1.  One warm-up of each path,
then three rounds alternating pf_banded_probs with pf_banded_mea in the same process; the host clock around the synchronous
calls, median (min..max); of the mea call also sf_mea_times: the device-event times of fill, exterior pass and traceback,
the band of the list, and the device bytes on top of the probs call's against SF_MEA_BYTES(L, n).  Printed per point: the
ratio pf_banded_mea / pf_banded_probs of the wall medians and the three phases' share of the call.
In every round the outputs the two paths share are compared for equality, and mea and mea_score with the warm-up's; after
the rounds mea_pairs on the returned list must give the same structure and score, and a gamma sweep (--gammas) of mea_pairs
is timed: what a further gamma costs once the partition function has been paid for.

--parent-lib PATH: sf_pf_banded_probs of another build of the library (the parent commit's) alternated with this tree's in
the same rounds at the same points: wall medians and their ratio, and the results compared for equality.

    python tools/gpu_pf_mea.py [--points 4000:120,4000:600,10000:120,10000:600,29903:600,100000:600,500000:600]
                               [--rounds 3] [--cutoff 0.01] [--gamma 1] [--gammas 0.5,1,4] [--parent-lib PATH]
                               [--json out.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

POINTS = "4000:120,4000:600,10000:120,10000:600,29903:600,100000:600,500000:600"
CLASSIC = ("dG", "mean_bp_dist", "centroid_dist", "centroid")
ARRAYS = ("unpaired", "entropy", "pairs")
PHASES = ("fill_ms", "ext_ms", "trace_ms")


def seeded(L):
    return "".join("ACGU"[k] for k in np.random.default_rng(L).integers(0, 4, L))


def mmm(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def fmt(m):
    return "%.1f (%.1f..%.1f)" % (m["median"], m["min"], m["max"])


def timed(call):
    t0 = time.perf_counter()
    r = call()
    return r, (time.perf_counter() - t0) * 1e3


def shared_equal(a, b):
    return all(a[k] == b[k] for k in CLASSIC) and all(a[k].tobytes() == b[k].tobytes() for k in ARRAYS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default=POINTS)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cutoff", type=float, default=0.01)
    ap.add_argument("--gamma", type=float, default=1.0)
    ap.add_argument("--gammas", default="0.5,1,4")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from scanfold_amd import _lib
    eng = _lib.get_engine(0)
    parent = None
    if args.parent_lib:
        parent = _lib.Engine(device=0, lib_path=args.parent_lib)
        parent.load_params(eng.params)
    out = dict(device=eng.device_name(), rounds=args.rounds, cutoff=args.cutoff, gamma=args.gamma, points=[])
    print("device:", out["device"])
    ok = True
    for point in args.points.split(","):
        L, S = (int(x) for x in point.split(":"))
        s = seeded(L)
        eng.set_max_bp_span(S)
        e, _ = eng.fold_banded(s, structure=False)
        ref = eng.pf_banded_probs(s, mfe_hint=e, cutoff=args.cutoff)  # warm-up of each path
        first = eng.pf_banded_mea(s, mfe_hint=e, cutoff=args.cutoff, gamma=args.gamma)
        same = shared_equal(first, ref)
        if parent:
            parent.set_max_bp_span(S)
            same = same and shared_equal(parent.pf_banded_probs(s, mfe_hint=e, cutoff=args.cutoff), ref)
        rows = {"probs": [], "mea": [], "parent": []}
        m = eng.mea_times()  # the warm-up's; every round replaces it
        for _ in range(max(1, args.rounds)):
            r, wall = timed(lambda: eng.pf_banded_probs(s, mfe_hint=e, cutoff=args.cutoff))
            rows["probs"].append((wall, 0.0, 0.0, 0.0))
            same = same and shared_equal(r, ref)
            r, wall = timed(lambda: eng.pf_banded_mea(s, mfe_hint=e, cutoff=args.cutoff, gamma=args.gamma))
            m = eng.mea_times()
            rows["mea"].append((wall,) + tuple(m[k] for k in PHASES))
            same = same and shared_equal(r, ref) and r["mea"] == first["mea"] and r["mea_score"] == first["mea_score"]
            if parent:
                r, wall = timed(lambda: parent.pf_banded_probs(s, mfe_hint=e, cutoff=args.cutoff))
                rows["parent"].append((wall, 0.0, 0.0, 0.0))
                same = same and shared_equal(r, ref)
        n = len(ref["pairs"])
        formula = 8 * n + 9 * L + 8 * (L // 2) + 33  # SF_MEA_BYTES(L, n)
        rec = dict(L=L, span=S, band=eng.pf_banded_times()["band"], list_band=m["band"], fill_launches=m["fill_launches"],
                   mfe_dcal=e, agree=None, n_pairs=n, extra_bytes=m["extra_bytes"], formula_bytes=formula,
                   mea_pairs=first["mea"].count("("), centroid_pairs=first["centroid"].count("("), mea_score=first["mea_score"])
        same = same and m["extra_bytes"] == formula
        for path in rows:
            if rows[path]:
                a = np.array(rows[path])
                rec[path] = {k: mmm(a[:, c].tolist()) for c, k in enumerate(("wall_ms",) + PHASES)}
        rec["mea_over_probs"] = rec["mea"]["wall_ms"]["median"] / rec["probs"]["wall_ms"]["median"]
        phases = sum(rec["mea"][k]["median"] for k in PHASES)
        rec["phases_share_of_call"] = phases / rec["mea"]["wall_ms"]["median"]
        if parent:
            rec["probs_over_parent"] = rec["probs"]["wall_ms"]["median"] / rec["parent"]["wall_ms"]["median"]
        # the same structure from the list alone, and what a further gamma costs
        sweep = {}
        for gamma in [float(x) for x in args.gammas.split(",")]:
            (db, score), wall = timed(lambda: eng.mea_pairs(L, ref["pairs"], ref["unpaired"], gamma))
            t = eng.mea_times()
            sweep["%g" % gamma] = dict(wall_ms=wall, pairs=db.count("("), score=score, **{k: t[k] for k in PHASES})
            if gamma == args.gamma:
                same = same and db == first["mea"] and score == first["mea_score"]
        rec["gamma_sweep"] = sweep
        rec["agree"] = bool(same)
        ok = ok and same
        out["points"].append(rec)
        print("L=%d span=%d agree=%s  list %d pairs, band %d; MEA %d pairs (centroid %d); extra %d bytes (formula %d)"
              % (L, S, same, n, m["band"], rec["mea_pairs"], rec["centroid_pairs"], m["extra_bytes"], formula))
        print("  pf_banded_probs  wall %s ms" % fmt(rec["probs"]["wall_ms"]))
        print("  pf_banded_mea    wall %s ms  fill %s  exterior %s  traceback %s ms = %.2f %% of the call;  mea / probs = %.4f"
              % (fmt(rec["mea"]["wall_ms"]), fmt(rec["mea"]["fill_ms"]), fmt(rec["mea"]["ext_ms"]), fmt(rec["mea"]["trace_ms"]),
                 100.0 * rec["phases_share_of_call"], rec["mea_over_probs"]))
        if parent:
            print("  parent pf_banded_probs wall %s ms;  this tree / parent = %.4f"
                  % (fmt(rec["parent"]["wall_ms"]), rec["probs_over_parent"]))
        print("  mea_pairs sweep: " + "; ".join("gamma %s: %d pairs, %.1f ms" % (g, v["pairs"], v["wall_ms"])
                                                 for g, v in sweep.items()))
        sys.stdout.flush()
    eng.set_max_bp_span(0)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
