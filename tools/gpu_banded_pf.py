"""Banded partition function (sf_pf_banded) against sf_pf_long under the same base-pair span, on one GPU.

Compared points: seeded random records of 4 000 and 10 000 nt under spans 120 and 600, each with its MFE (fold_banded's) as
hint.  One warm-up of each path, then three rounds alternating pf_banded with pf_long in the same process; the host clock
around the synchronous calls and both calls' device-event splits (inside / outside); median (min..max).  The two paths'
results are compared in every round to the tests' bar (1e-8 relative on dG, mean_bp_dist and centroid_dist, equal
centroids).  The claim checked and printed per point: the banded path's slowest round is faster than pf_long's fastest.

Then pf_banded alone at 29 903, 100 000 and 500 000 nt under span 600: times, attempts, launches, bytes allocated.

    python tools/gpu_banded_pf.py [--lengths 4000,10000] [--spans 120,600] [--alone 29903,100000,500000] [--rounds 3]
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

TOL = 1e-8
KEYS = ("dG", "mean_bp_dist", "centroid_dist")


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


def close(a, b):
    return a["centroid"] == b["centroid"] and all(np.isfinite(a[k]) and abs(a[k] - b[k]) <= TOL * max(1.0, abs(b[k]))
                                                   for k in KEYS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", default="4000,10000")
    ap.add_argument("--spans", default="120,600")
    ap.add_argument("--alone", default="29903,100000,500000")
    ap.add_argument("--alone-span", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    ints = lambda s: [int(x) for x in s.split(",") if x]  # noqa: E731
    from scanfold_amd import _lib
    eng = _lib.get_engine(0)
    out = dict(device=eng.device_name(), rounds=args.rounds, compared=[], alone=[])
    print("device:", out["device"])
    ok = True
    for L in ints(args.lengths):
        s = seeded(L)
        for S in ints(args.spans):
            eng.set_max_bp_span(S)
            e, _ = eng.fold_banded(s, structure=False)
            ref = eng.pf_long(s, mfe_hint=e)  # warm-up of each path
            same = close(eng.pf_banded(s, mfe_hint=e), ref)
            rows = {"banded": [], "long": []}
            for _ in range(args.rounds):
                r, wall = timed(lambda: eng.pf_banded(s, mfe_hint=e))
                t = eng.pf_banded_times()
                rows["banded"].append((wall, t["inside_ms"], t["outside_ms"], t["attempts"]))
                same = same and close(r, ref)
                r, wall = timed(lambda: eng.pf_long(s, mfe_hint=e))
                t = eng.pf_long_times()
                rows["long"].append((wall, t["inside_ms"], t["outside_ms"], t["attempts"]))
                same = same and r == ref
            t = eng.pf_banded_times()
            rec = dict(L=L, span=S, mfe_dcal=e, dG=ref["dG"], dG_banded=r["dG"], agree=bool(same), band=t["band"],
                       launches=t["launches"], lns=t["lns"], bytes=eng.pf_banded_bytes(L, S),
                       long_table_bytes=56 * (L * (L + 1) // 2))
            for path in rows:
                a = np.array(rows[path])
                rec[path] = {k: mmm(a[:, c].tolist()) for c, k in enumerate(("wall_ms", "inside_ms", "outside_ms", "attempts"))}
            rec["claim_holds"] = rec["banded"]["wall_ms"]["max"] < rec["long"]["wall_ms"]["min"]
            rec["ratio_median"] = rec["long"]["wall_ms"]["median"] / rec["banded"]["wall_ms"]["median"]
            ok = ok and same and rec["claim_holds"]
            out["compared"].append(rec)
            print("L=%d span=%d agree=%s band=%d launches=%d bytes=%d" % (L, S, same, rec["band"], rec["launches"], rec["bytes"]))
            for path in ("banded", "long"):
                print("  %-7s wall %s  inside %s  outside %s ms  attempts %s" % ((path,) + tuple(
                    fmt(rec[path][k]) for k in ("wall_ms", "inside_ms", "outside_ms", "attempts"))))
            print("  pf_long / pf_banded = %.1fx (medians); slowest banded < fastest long: %s"
                  % (rec["ratio_median"], rec["claim_holds"]), flush=True)
    for L in ints(args.alone):
        S = args.alone_span
        s = seeded(L)
        eng.set_max_bp_span(S)
        e, _ = eng.fold_banded(s, structure=False)
        r, wall = timed(lambda: eng.pf_banded(s, mfe_hint=e))
        t = eng.pf_banded_times()
        rec = dict(L=L, span=S, mfe_dcal=e, dG=r["dG"], mean_bp_dist=r["mean_bp_dist"], centroid_dist=r["centroid_dist"],
                   pairs=r["centroid"].count("("), wall_ms=wall, bytes=eng.pf_banded_bytes(L, S), **t)
        ok = ok and all(np.isfinite(r[k]) for k in KEYS) and r["dG"] <= e * 0.01
        out["alone"].append(rec)
        print("alone L=%d span=%d: wall %.1f inside %.1f outside %.1f ms; attempts %d, launches %d, lns %.4f; %d bytes; "
              "dG %.2f (mfe %.2f), %d centroid pairs" % (L, S, wall, t["inside_ms"], t["outside_ms"], t["attempts"],
                                                         t["launches"], t["lns"], rec["bytes"], r["dG"], e * 0.01,
                                                         rec["pairs"]), flush=True)
    eng.set_max_bp_span(0)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
