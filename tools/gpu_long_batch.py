"""Batched whole-record folds (sf_fold_long_batch) against a loop of sf_fold_long calls on one GPU: the z-score workload of a
record past the window limit, one seeded sequence and 100 dinucleotide shuffles of it (n = 101), energies only, at
L = 500, 1 000, 2 000 and 4 000.

Per length: one warm-up of each path, then `--repeats` timed rounds that alternate one fold_long_batch with 101 fold_long
calls in the same process.  Times are a host clock around the synchronous calls; for the batch also the device-event times
of fill / f5 from fold_long_batch_times(), for the loop the sum of fold_long_times().  Energies of both paths must agree.
Writes the table to stdout and everything to a JSON file.

    python tools/gpu_long_batch.py [--lengths 500,1000,2000,4000] [--n 101] [--repeats 3] [--json long_batch.json]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def rows_for(L, n):
    from scanfold_amd import functions
    seq = "".join("ACGU"[k] for k in np.random.default_rng(L).integers(0, 4, L))
    state = random.getstate()
    random.seed(L)
    rows = [seq] + functions.scramble(seq, n - 1, "di")
    random.setstate(state)
    return rows


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), all=xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", default="500,1000,2000,4000")
    ap.add_argument("--n", type=int, default=101)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default="long_batch.json")
    ap.add_argument("--batch-only", action="store_true", help="skip the loop of fold_long calls (for a kernel trace)")
    args = ap.parse_args()
    from scanfold_amd import _lib
    eng = _lib.get_engine(0)
    print("device:", eng.device_name())
    result = dict(device=eng.device_name(), n=args.n, repeats=args.repeats, shapes=[])
    print("%6s %4s %7s %12s %12s %12s %12s %8s %10s %10s" % ("L", "n", "chunks", "batch_ms", "batch_fill", "batch_f5",
                                                            "loop_ms", "ratio", "batch f/s", "loop f/s"))
    for L in [int(x) for x in args.lengths.split(",")]:
        rows = rows_for(L, args.n)
        e_batch = eng.fold_long_batch(rows)  # warm-up of both paths
        if not args.batch_only:
            eng.fold_long(rows[0], structure=False)
        batch_ms, loop_ms, fill_ms, f5_ms, loop_dev_ms = [], [], [], [], []
        chunks = 0
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            e_batch = eng.fold_long_batch(rows)
            batch_ms.append((time.perf_counter() - t0) * 1e3)
            t = eng.fold_long_batch_times()
            fill_ms.append(t["fill_ms"])
            f5_ms.append(t["f5_ms"])
            chunks = t["chunks"]
            if args.batch_only:
                continue
            t0 = time.perf_counter()
            dev = 0.0
            e_loop = []
            for s in rows:
                e_loop.append(eng.fold_long(s, structure=False)[0])
                dev += sum(eng.fold_long_times())
            loop_ms.append((time.perf_counter() - t0) * 1e3)
            loop_dev_ms.append(dev)
            if [int(v) for v in e_batch] != e_loop:
                raise SystemExit("L = %d: the batch and the loop disagree" % L)
        shape = dict(L=L, n=args.n, chunks=chunks, batch_wall_ms=spread(batch_ms), batch_fill_ms=spread(fill_ms),
                     batch_f5_ms=spread(f5_ms), batch_folds_per_s=args.n / (statistics.median(batch_ms) * 1e-3),
                     mfe_dcal_native=int(e_batch[0]))
        if not args.batch_only:
            shape.update(loop_wall_ms=spread(loop_ms), loop_device_ms=spread(loop_dev_ms),
                         loop_folds_per_s=args.n / (statistics.median(loop_ms) * 1e-3),
                         ratio_loop_over_batch=statistics.median(loop_ms) / statistics.median(batch_ms))
        result["shapes"].append(shape)
        print("%6d %4d %7d %12.1f %12.1f %12.1f %12s %8s %10.1f %10s" % (
            L, args.n, chunks, statistics.median(batch_ms), statistics.median(fill_ms), statistics.median(f5_ms),
            "-" if args.batch_only else "%.1f" % statistics.median(loop_ms),
            "-" if args.batch_only else "%.2f" % shape["ratio_loop_over_batch"], shape["batch_folds_per_s"],
            "-" if args.batch_only else "%.1f" % shape["loop_folds_per_s"]), flush=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
