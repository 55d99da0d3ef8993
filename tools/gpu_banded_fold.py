"""Banded whole-record fold (sf_fold_banded) against sf_fold_long under the same base-pair span, on one GPU.

Compared points: seeded random records of 4 000, 10 000 and 29 903 nt under spans 120 and 600, with structure.  One warm-up
of each path, then three rounds alternating fold_banded with fold_long in the same process; the host clock around the
synchronous calls and both calls' device-event splits (fill / f5 / traceback); median (min..max).  Energies and structures of
the two paths are compared with == in every round.  The claim checked and printed per point: the banded path's slowest round
is faster than fold_long's fastest.

Then fold_banded alone at 100 000 and 500 000 nt under span 600: times, f5 ms per nucleotide, bytes allocated.

    python tools/gpu_banded_fold.py [--lengths 4000,10000,29903] [--spans 120,600] [--alone 100000,500000] [--rounds 3]
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
    ap.add_argument("--lengths", default="4000,10000,29903")
    ap.add_argument("--spans", default="120,600")
    ap.add_argument("--alone", default="100000,500000")
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
            ref = eng.fold_banded(s)  # warm-up of each path
            same = ref == eng.fold_long(s)
            rows = {"banded": [], "long": []}
            for _ in range(args.rounds):
                r, wall = timed(lambda: eng.fold_banded(s))
                t = eng.fold_banded_times()
                rows["banded"].append((wall, t["fill_ms"], t["f5_ms"], t["trace_ms"]))
                same = same and r == ref
                r, wall = timed(lambda: eng.fold_long(s))
                rows["long"].append((wall,) + tuple(eng.fold_long_times()))
                same = same and r == ref
            t = eng.fold_banded_times()
            rec = dict(L=L, span=S, mfe_dcal=ref[0], identical=bool(same), band=t["band"], fill_launches=t["fill_launches"],
                       bytes=eng.fold_banded_bytes(L, S), long_table_bytes=12 * (L * (L + 1) // 2))
            for path in rows:
                a = np.array(rows[path])
                rec[path] = {k: mmm(a[:, c].tolist()) for c, k in enumerate(("wall_ms", "fill_ms", "f5_ms", "trace_ms"))}
            rec["claim_holds"] = rec["banded"]["wall_ms"]["max"] < rec["long"]["wall_ms"]["min"]
            rec["ratio_median"] = rec["long"]["wall_ms"]["median"] / rec["banded"]["wall_ms"]["median"]
            ok = ok and same and rec["claim_holds"]
            out["compared"].append(rec)
            print("L=%d span=%d identical=%s band=%d launches=%d bytes=%d" % (L, S, same, rec["band"], rec["fill_launches"],
                                                                              rec["bytes"]))
            for path in ("banded", "long"):
                print("  %-7s wall %s  fill %s  f5 %s  trace %s ms" % ((path,) + tuple(
                    fmt(rec[path][k]) for k in ("wall_ms", "fill_ms", "f5_ms", "trace_ms"))))
            print("  fold_long / fold_banded = %.1fx (medians); slowest banded < fastest long: %s"
                  % (rec["ratio_median"], rec["claim_holds"]), flush=True)
    for L in ints(args.alone):
        S = args.alone_span
        s = seeded(L)
        eng.set_max_bp_span(S)
        (e, db), wall = timed(lambda: eng.fold_banded(s))
        t = eng.fold_banded_times()
        rec = dict(L=L, span=S, mfe_dcal=e, pairs=db.count("("), wall_ms=wall, bytes=eng.fold_banded_bytes(L, S),
                   f5_ms_per_nt=t["f5_ms"] / L, **t)
        out["alone"].append(rec)
        print("alone L=%d span=%d: wall %.1f fill %.1f f5 %.1f trace %.1f ms; f5 %.5f ms/nt; %d bytes; mfe %d dcal, %d pairs"
              % (L, S, wall, t["fill_ms"], t["f5_ms"], t["trace_ms"], rec["f5_ms_per_nt"], rec["bytes"], e, rec["pairs"]),
              flush=True)
    eng.set_max_bp_span(0)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
