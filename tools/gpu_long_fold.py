"""Whole-record fold (sf_fold_long) timing on one GPU: seeded sequences at L = 1 000, 4 000, 10 000 and 29 903, one warm-up,
then the device-event times of the fill (one launch per diagonal), the exterior loop f5 and the traceback.

Split terms = sum over the cells (i, j) of the multiloop split length max(0, j - i - 7) (the O(L^3) part of the fill).
The byte bound is two int32 loads per split term (row i of fML, row j of its transpose) against the fill time: what the fill
would need if every term came from memory.  The oracle's CPU time at L = 2 000 is printed for context.

    python tools/gpu_long_fold.py [--lengths 1000,4000,10000,29903] [--no-oracle]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def split_terms(L):
    d = np.arange(L, dtype=np.float64)
    return float(np.sum((L - d) * np.maximum(0.0, d - 7)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", default="1000,4000,10000,29903")
    ap.add_argument("--no-oracle", action="store_true")
    args = ap.parse_args()
    from scanfold_amd import _lib
    eng = _lib.get_engine(0)
    print("device:", eng.device_name())
    rng = np.random.default_rng(29903)
    warm = "".join("ACGU"[k] for k in rng.integers(0, 4, 1000))
    eng.fold_long(warm)
    print("%7s %10s %9s %9s %9s %10s %12s %12s %10s" % ("L", "mfe_dcal", "fill_ms", "f5_ms", "trace_ms", "wall_ms",
                                                        "terms", "terms/s", "GB/s@2ld"))
    for L in [int(x) for x in args.lengths.split(",")]:
        s = "".join("ACGU"[k] for k in np.random.default_rng(L).integers(0, 4, L))
        t0 = time.perf_counter()
        e, db = eng.fold_long(s)
        wall = (time.perf_counter() - t0) * 1e3
        fill, f5, tr = eng.fold_long_times()
        terms = split_terms(L)
        print("%7d %10d %9.1f %9.1f %9.1f %10.1f %12.3e %12.3e %10.1f" % (
            L, e, fill, f5, tr, wall, terms, terms / (fill * 1e-3), terms * 8 / (fill * 1e-3) / 1e9), flush=True)
    if not args.no_oracle:
        from oracle import oracle
        from scanfold_amd import params
        oracle.build()
        oracle.set_params(params.default_params())
        s = "".join("ACGU"[k] for k in np.random.default_rng(2000).integers(0, 4, 2000))
        t0 = time.perf_counter()
        db, e = oracle.mfe(s)
        t_cpu = time.perf_counter() - t0
        t0 = time.perf_counter()
        e2, db2 = eng.fold_long(s)
        t_gpu = time.perf_counter() - t0
        print("L=2000: oracle (CPU, one thread) %.2f s, GPU %.3f s, identical=%s" % (t_cpu, t_gpu, (e, db) == (e2, db2)))


if __name__ == "__main__":
    main()
