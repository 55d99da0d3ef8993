"""Batched whole-record partition functions (sf_pf_long_batch) against a loop of sf_pf_long calls on one GPU, in three shapes:

  ensemble   n = 3 at 1 100 nt: one nested record (tests/long_pf_util.nested_record) unconstrained and under two constraint
             rows, scaled from the three MFEs — what --global_ensemble runs;
  windows    n = 32 at 600 nt and at 1 000 nt: overlapping windows of one seeded record, scaled from their MFEs — what a
             window scan past 400 nt would run;
  long       n = 8 at 2 112 nt: seeded records, scaled from their MFEs.

Per case: one warm-up of each path, then `--repeats` timed rounds that alternate one pf_long_batch with n pf_long calls on the
same rows, constraints and hints in the same process.  Times are a host clock around the synchronous calls; for the batch
also the device-event times of the inside and outside passes from pf_long_batch_times(), for the loop the sums of
pf_long_times().  Every row of the batch must equal the loop's (`==` on floats and strings).  Prints median (min..max) and
writes everything to a JSON file.

    python tools/gpu_long_pf_batch.py [--cases ensemble,windows600,windows1000,long] [--repeats 3] [--json pf_long_batch.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def rand_seq(rng, L):
    return "".join("ACGU"[k] for k in rng.integers(0, 4, L))


def pair_constraint(db, keep):
    """every keep-th pair of a dot-bracket structure as a constraint row"""
    out, stack, n = ["."] * len(db), [], 0
    for k, ch in enumerate(db):
        if ch == "(":
            stack.append(k)
        elif ch == ")":
            i = stack.pop()
            if n % keep == 0:
                out[i], out[k] = "(", ")"
            n += 1
    return "".join(out)


def case_rows(eng, name):
    """-> (sequences, constraints or None, MFE hints)"""
    if name == "ensemble":
        from long_pf_util import nested_record
        seq, _, _ = nested_record(np.random.default_rng(3), 1100)
        _, db = eng.fold_long(seq)
        cons = [None, pair_constraint(db, 2), pair_constraint(db, 5)]
        seqs = [seq] * 3
    elif name.startswith("windows"):
        W = int(name[len("windows"):])
        rec = rand_seq(np.random.default_rng(W), W + 31 * 10)
        seqs, cons = [rec[10 * k:10 * k + W] for k in range(32)], None
    elif name == "long":
        seqs, cons = [rand_seq(np.random.default_rng(2112 + k), 2112) for k in range(8)], None
    else:
        raise SystemExit("unknown case " + name)
    hints = [int(v) for v in eng.fold_long_batch(seqs, cons)]
    return seqs, cons, hints


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), all=xs)


def fmt(s):
    return "%.1f (%.1f..%.1f)" % (s["median"], s["min"], s["max"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="ensemble,windows600,windows1000,long")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default="pf_long_batch.json")
    args = ap.parse_args()
    from scanfold_amd import _lib
    eng = _lib.get_engine(0)
    print("device:", eng.device_name())
    result = dict(device=eng.device_name(), repeats=args.repeats, cases=[])
    for name in args.cases.split(","):
        seqs, cons, hints = case_rows(eng, name)
        n = len(seqs)

        def loop():
            dev_in = dev_out = 0.0
            rows = []
            for k in range(n):
                rows.append(eng.pf_long(seqs[k], None if cons is None else cons[k], mfe_hint=hints[k]))
                t = eng.pf_long_times()
                dev_in += t["inside_ms"]
                dev_out += t["outside_ms"]
            return rows, dev_in, dev_out

        eng.pf_long_batch(seqs, cons, hints)  # warm-up of both paths
        loop()
        batch_ms, loop_ms, b_in, b_out, l_in, l_out = [], [], [], [], [], []
        info = {}
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            rows = eng.pf_long_batch(seqs, cons, hints)
            batch_ms.append((time.perf_counter() - t0) * 1e3)
            info = eng.pf_long_batch_times()
            b_in.append(info["inside_ms"])
            b_out.append(info["outside_ms"])
            t0 = time.perf_counter()
            single, di, do = loop()
            loop_ms.append((time.perf_counter() - t0) * 1e3)
            l_in.append(di)
            l_out.append(do)
            if [{k: r[k] for k in single[0]} for r in rows] != single:
                raise SystemExit("%s: the batch and the loop disagree" % name)
        case = dict(case=name, n=n, L=len(seqs[0]), chunks=info["chunks"], inside_passes=info["inside_passes"],
                    attempts=[r["attempts"] for r in rows], batch_wall_ms=spread(batch_ms), batch_inside_ms=spread(b_in),
                    batch_outside_ms=spread(b_out), loop_wall_ms=spread(loop_ms), loop_inside_ms=spread(l_in),
                    loop_outside_ms=spread(l_out), ratio_loop_over_batch=statistics.median(loop_ms) / statistics.median(batch_ms),
                    slowest_batch_beats_fastest_loop=max(batch_ms) < min(loop_ms), dG=[r["dG"] for r in rows])
        result["cases"].append(case)
        print("%-12s n=%2d L=%4d chunks=%d passes=%d  batch %s ms [inside %s, outside %s]  loop %s ms [inside %s, outside %s]  "
              "loop/batch %.2f  slowest batch < fastest loop: %s"
              % (name, n, case["L"], case["chunks"], case["inside_passes"], fmt(case["batch_wall_ms"]),
                 fmt(case["batch_inside_ms"]), fmt(case["batch_outside_ms"]), fmt(case["loop_wall_ms"]),
                 fmt(case["loop_inside_ms"]), fmt(case["loop_outside_ms"]), case["ratio_loop_over_batch"],
                 case["slowest_batch_beats_fastest_loop"]), flush=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
