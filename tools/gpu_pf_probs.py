"""Base-pair probabilities of a whole record under a span (sf_pf_banded_probs) against sf_pf_banded alone, on one GPU.

Points: the seeded random records of tools/gpu_banded_pf.py (4 000 and 10 000 nt under spans 120 and 600; 29 903, 100 000
and 500 000 nt under span 600), each with its MFE (fold_banded's) as hint.  One warm-up of each path, then three rounds
alternating pf_banded with pf_banded_probs (cutoff 0.01) in the same process; the host clock around the synchronous calls,
median (min..max); of the probs call also the extraction's device-event time, the length of the list and the device bytes
on top of pf_banded's.  Printed per point: the ratio pf_banded_probs / pf_banded of the wall medians, and the extraction's
achieved bytes per second against the table bytes it must read (ob and qb, 16 L B bytes together, four times: the
per-nucleotide pass by rows and again by column blocks, the count, and the writing pass).
In every round the four classic outputs of the two paths are compared for equality and the three arrays with the warm-up's.

--parent-lib PATH: sf_pf_banded of another build of the library (the parent commit's) alternated with this tree's in the
same rounds at the same points: wall medians and their ratio, and the results compared for equality.

    python tools/gpu_pf_probs.py [--points 4000:120,4000:600,10000:120,10000:600,29903:600,100000:600,500000:600]
                                 [--rounds 3] [--cutoff 0.01] [--parent-lib PATH] [--json out.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default=POINTS)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cutoff", type=float, default=0.01)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from scanfold_amd import _lib
    eng = _lib.get_engine(0)
    parent = None
    if args.parent_lib:
        parent = _lib.Engine(device=0, lib_path=args.parent_lib)
        parent.load_params(eng.params)
    out = dict(device=eng.device_name(), rounds=args.rounds, cutoff=args.cutoff, points=[])
    print("device:", out["device"])
    ok = True
    for point in args.points.split(","):
        L, S = (int(x) for x in point.split(":"))
        s = seeded(L)
        eng.set_max_bp_span(S)
        e, _ = eng.fold_banded(s, structure=False)
        ref = eng.pf_banded(s, mfe_hint=e)  # warm-up of each path
        first = eng.pf_banded_probs(s, mfe_hint=e, cutoff=args.cutoff)
        same = all(first[k] == ref[k] for k in CLASSIC)
        if parent:
            parent.set_max_bp_span(S)
            same = same and parent.pf_banded(s, mfe_hint=e) == ref
        rows = {"banded": [], "probs": [], "parent": []}
        for _ in range(args.rounds):
            r, wall = timed(lambda: eng.pf_banded(s, mfe_hint=e))
            t = eng.pf_banded_times()
            rows["banded"].append((wall, t["inside_ms"], t["outside_ms"], 0.0))
            same = same and r == ref
            r, wall = timed(lambda: eng.pf_banded_probs(s, mfe_hint=e, cutoff=args.cutoff))
            t, x = eng.pf_banded_times(), eng.pf_banded_probs_times()
            rows["probs"].append((wall, t["inside_ms"], t["outside_ms"], x["extract_ms"]))
            same = same and all(r[k] == ref[k] for k in CLASSIC)
            same = same and all(r[k].tobytes() == first[k].tobytes() for k in ("unpaired", "entropy", "pairs"))
            if parent:
                r, wall = timed(lambda: parent.pf_banded(s, mfe_hint=e))
                t = parent.pf_banded_times()
                rows["parent"].append((wall, t["inside_ms"], t["outside_ms"], 0.0))
                same = same and r == ref
        t = eng.pf_banded_times()
        B = t["band"]
        rec = dict(L=L, span=S, band=B, mfe_dcal=e, dG=ref["dG"], agree=bool(same), attempts=t["attempts"],
                   bytes=eng.pf_banded_bytes(L, S), n_pairs=x["n_pairs"], extra_bytes=x["extra_bytes"],
                   pairs_bound=L * int(1 / args.cutoff) // 2, mean_entropy_bits=float(first["entropy"].mean()),
                   mean_unpaired=float(first["unpaired"].mean()))
        for path in rows:
            if rows[path]:
                a = np.array(rows[path])
                rec[path] = {k: mmm(a[:, c].tolist()) for c, k in enumerate(("wall_ms", "inside_ms", "outside_ms", "extract_ms"))}
        rec["probs_over_banded"] = rec["probs"]["wall_ms"]["median"] / rec["banded"]["wall_ms"]["median"]
        rec["table_bytes_read"] = 4 * 16 * L * B
        rec["extract_GBps"] = rec["table_bytes_read"] / (rec["probs"]["extract_ms"]["median"] * 1e-3) / 1e9
        if parent:
            rec["banded_over_parent"] = rec["banded"]["wall_ms"]["median"] / rec["parent"]["wall_ms"]["median"]
        ok = ok and same
        out["points"].append(rec)
        print("L=%d span=%d agree=%s attempts=%d bytes=%d  list %d pairs (bound %d), extra %d bytes"
              % (L, S, same, rec["attempts"], rec["bytes"], rec["n_pairs"], rec["pairs_bound"], rec["extra_bytes"]))
        print("  pf_banded        wall %s ms" % fmt(rec["banded"]["wall_ms"]))
        print("  pf_banded_probs  wall %s ms  extraction %s ms = %.0f GB/s of %d table bytes;  probs / banded = %.4f"
              % (fmt(rec["probs"]["wall_ms"]), fmt(rec["probs"]["extract_ms"]), rec["extract_GBps"], rec["table_bytes_read"],
                 rec["probs_over_banded"]))
        if parent:
            print("  parent pf_banded wall %s ms;  this tree / parent = %.4f"
                  % (fmt(rec["parent"]["wall_ms"]), rec["banded_over_parent"]))
        sys.stdout.flush()
    eng.set_max_bp_span(0)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
