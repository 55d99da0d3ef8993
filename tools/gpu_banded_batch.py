"""Batched banded whole-record fold (sf_fold_banded_batch) against a loop of sf_fold_banded calls, on one GPU.

The workload is the whole-record z-score under a span: one seeded random record and 100 dinucleotide shuffles of it, energies
only.  Measured points: records of 2 000, 10 000 and 29 903 nt under spans 120 and 600.  One warm-up of each path, then three
rounds alternating ONE fold_banded_batch of the 101 rows with a loop of 101 fold_banded calls in the same process; the host
clock around the synchronous calls; median (min..max).  Both paths' device-event splits (fill / f5; the loop's summed over its
101 calls), the batch's chunk and launch counts, the bytes of the batch's tables, and whether the 101 energies of the two
paths were equal in every round.  The conditions checked and printed per point: the batch's median time does not exceed the
loop's, and (at 2 000 nt, where the single call is launch-bound) the batch's slowest round is faster than the loop's fastest.

    python tools/gpu_banded_batch.py [--lengths 2000,10000,29903] [--spans 120,600] [--shuffles 100] [--rounds 3]
                                     [--json out.json]
"""
import argparse
import json
import os
import random
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
    ap.add_argument("--lengths", default="2000,10000,29903")
    ap.add_argument("--spans", default="120,600")
    ap.add_argument("--shuffles", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--strict-below", type=int, default=2001,
                    help="records shorter than this must also have the batch's slowest round under the loop's fastest")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    ints = lambda s: [int(x) for x in s.split(",") if x]  # noqa: E731
    from scanfold_amd import _lib, functions
    eng = _lib.get_engine(0)
    out = dict(device=eng.device_name(), rounds=args.rounds, shuffles=args.shuffles, points=[])
    print("device:", out["device"])
    ok = True

    def loop(rows):
        """-> (energies, summed fill ms, summed f5 ms) of one fold_banded call per row"""
        e, fill, f5 = [], 0.0, 0.0
        for s in rows:
            e.append(eng.fold_banded(s, structure=False)[0])
            t = eng.fold_banded_times()
            fill += t["fill_ms"]
            f5 += t["f5_ms"]
        return e, fill, f5

    for L in ints(args.lengths):
        s = seeded(L)
        random.seed(L)
        rows = [s] + functions.scramble(s, args.shuffles, "di")
        for S in ints(args.spans):
            eng.set_max_bp_span(S)
            ref = [int(v) for v in eng.fold_banded_batch(rows)]  # warm-up of each path
            same = ref == loop(rows)[0]
            t_rows = {"batch": [], "loop": []}
            for _ in range(args.rounds):
                e, wall = timed(lambda: eng.fold_banded_batch(rows))
                t = eng.fold_banded_batch_times()
                t_rows["batch"].append((wall, t["fill_ms"], t["f5_ms"]))
                same = same and [int(v) for v in e] == ref
                (e, fill, f5), wall = timed(lambda: loop(rows))
                t_rows["loop"].append((wall, fill, f5))
                same = same and e == ref
            t = eng.fold_banded_batch_times()
            rec = dict(L=L, span=S, rows=len(rows), mfe_dcal=ref[0], identical=bool(same), chunks=t["chunks"],
                       fill_launches=t["fill_launches"], loop_fill_launches=len(rows) * min(S, L),
                       bytes=len(rows) * eng.fold_banded_bytes(L, S))
            for path in t_rows:
                a = np.array(t_rows[path])
                rec[path] = {k: mmm(a[:, c].tolist()) for c, k in enumerate(("wall_ms", "fill_ms", "f5_ms"))}
            rec["median_holds"] = rec["batch"]["wall_ms"]["median"] <= rec["loop"]["wall_ms"]["median"]
            rec["strict"] = L < args.strict_below
            rec["strict_holds"] = rec["batch"]["wall_ms"]["max"] < rec["loop"]["wall_ms"]["min"]
            rec["ratio_median"] = rec["loop"]["wall_ms"]["median"] / rec["batch"]["wall_ms"]["median"]
            rec["f5_ratio_median"] = rec["loop"]["f5_ms"]["median"] / rec["batch"]["f5_ms"]["median"]
            ok = ok and same and rec["median_holds"] and (rec["strict_holds"] or not rec["strict"])
            out["points"].append(rec)
            print("L=%d span=%d rows=%d identical=%s chunks=%d launches=%d (loop: %d) bytes=%d"
                  % (L, S, len(rows), same, rec["chunks"], rec["fill_launches"], rec["loop_fill_launches"], rec["bytes"]))
            for path in ("batch", "loop"):
                print("  %-5s wall %s  fill %s  f5 %s ms" % ((path,) + tuple(fmt(rec[path][k])
                                                                              for k in ("wall_ms", "fill_ms", "f5_ms"))))
            print("  loop / batch = %.2fx wall, %.2fx f5 (medians); median batch <= median loop: %s; slowest batch < fastest "
                  "loop: %s%s" % (rec["ratio_median"], rec["f5_ratio_median"], rec["median_holds"], rec["strict_holds"],
                                  " (required here)" if rec["strict"] else ""), flush=True)
    eng.set_max_bp_span(0)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
