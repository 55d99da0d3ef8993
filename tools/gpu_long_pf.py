"""Whole-record partition function (sf_pf_long) timing on one GPU: seeded sequences at L = 1 000, 4 000, 10 000 and 29 903,
one warm-up, then per length the MFE (sf_fold_long, whose energy sets the scale) and the device-event times of the inside
passes and of the outside pass, the number of attempts, the final per-nucleotide scale and the device-memory footprint.
One process; each length is a step of its own, printed as it finishes.

    python tools/gpu_long_pf.py [--lengths 1000,4000,10000,29903] [--no-hint]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def footprint_bytes(L):
    return 56 * L * (L + 1) // 2 + 60 * L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", default="1000,4000,10000,29903")
    ap.add_argument("--no-hint", action="store_true", help="start from the fixed per-nucleotide scale, not from the MFE")
    args = ap.parse_args()
    from scanfold_amd import _lib
    eng = _lib.get_engine(0)
    print("device:", eng.device_name())
    warm = "".join("ACGU"[k] for k in np.random.default_rng(29903).integers(0, 4, 1000))
    eng.pf_long(warm)
    print("%7s %10s %12s %10s %11s %11s %8s %8s %10s %9s" % ("L", "mfe_dcal", "dG", "fill_ms", "inside_ms", "outside_ms",
                                                             "attempts", "lns", "wall_ms", "GB"))
    for L in [int(x) for x in args.lengths.split(",")]:
        s = "".join("ACGU"[k] for k in np.random.default_rng(L).integers(0, 4, L))
        e, _ = eng.fold_long(s, structure=False)
        fill = eng.fold_long_times()[0]
        t0 = time.perf_counter()
        r = eng.pf_long(s, mfe_hint=None if args.no_hint else e)
        wall = (time.perf_counter() - t0) * 1e3
        t = eng.pf_long_times()
        print("%7d %10d %12.2f %10.1f %11.1f %11.1f %8d %8.4f %10.1f %9.2f" % (
            L, e, r["dG"], fill, t["inside_ms"], t["outside_ms"], t["attempts"], t["lns"], wall, footprint_bytes(L) / 1e9),
            flush=True)


if __name__ == "__main__":
    main()
