"""Measure the long-range-interaction scan (Engine.lri_scan) on the seeded 30-kb cfg3 record.

Prints: duplexes/s of the all-pairs scan by device events (a warm-up on a short record, --repeats timed runs, median), the time of the
hits' backgrounds, the wall time of scanfold_amd.lri.lri_scan end to end, the scan time at k = 10 / 20 / 40, and the
yardstick — tests/duplex_ref (the plain-C restatement of the model) on --threads CPU threads over a subsample of j_win
rows, scaled to the whole scan.  One JSON line at the end.

    python tools/gpu_lri.py [--L 30000] [--kmer 20] [--repeats 3] [--threads 16] [--cpu-rows 4] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def record(L, seed=3):
    rng = np.random.default_rng(seed)  # bench.py's cfg3 record: i.i.d. over ACGU, seed 3
    return "".join("ACGU"[k] for k in rng.integers(0, 4, L))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=30000)
    ap.add_argument("--kmer", type=int, default=20)
    ap.add_argument("--step", type=int, default=1)
    ap.add_argument("--cutoff", type=int, default=-25)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup-L", type=int, default=3000)
    ap.add_argument("--no-end-to-end", action="store_true", help="skip lri.lri_scan end to end (one more whole scan)")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cpu-rows", type=int, default=4)
    ap.add_argument("--sweep", type=str, default="10,20,40")
    ap.add_argument("--sweep-L", type=int, default=8000)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()

    from scanfold_amd import _lib, lri
    import duplex_util as du
    eng = _lib.get_engine()
    du.set_params(eng.params)
    seq = record(a.L)
    res = dict(device=eng.device_name(), L=a.L, kmer=a.kmer, step=a.step, cutoff=a.cutoff)

    res["argv"] = sys.argv[1:]
    # warm-up on a short record (code object load, first launch); the timed runs scan the whole record
    eng.lri_scan(record(min(a.L, a.warmup_L)), a.kmer, a.step, a.cutoff * 100)
    times = []
    for rep in range(a.repeats):
        hits = eng.lri_scan(seq, a.kmer, a.step, a.cutoff * 100)
        ms, nd = eng.lri_scan_time()
        times.append(ms)
        print("scan run %d: %.1f ms, %d duplexes, %d hits" % (rep, ms, nd, len(hits)), flush=True)
    ms = statistics.median(times)
    res.update(scan_ms=ms, scan_ms_all=times, duplexes=nd, hits=len(hits), gpu_duplexes_per_s=nd / (ms / 1e3))

    t = time.perf_counter()
    eng.lri_background(seq, a.kmer, hits["j_win"], hits["k_win"], 100, _lib.SHUFFLE_MONO, 0)
    res["background_s_r100"] = time.perf_counter() - t
    if not a.no_end_to_end:
        t = time.perf_counter()
        recs = lri.lri_scan(seq, a.kmer, a.step, a.cutoff, 100, "mono", eng, 0)
        res["end_to_end_s"] = time.perf_counter() - t
        res["rows_written"] = len(recs)

    # CPU yardstick: a few whole j_win rows spread over the record
    nj, nk = eng.lri_grid(a.L, a.kmer, a.step)
    rows = sorted(set(int(x) for x in np.linspace(0, nj - 1, a.cpu_rows)))
    pl = [(j * a.step, k * a.step) for j in rows for k in range(nk)
          if (k * a.step + 3) < (j * a.step - a.kmer) or k * a.step > (j * a.step + a.kmer + 3)]
    jw, kw = [p[0] for p in pl], [p[1] for p in pl]
    du.pairs(seq, a.kmer, jw[:1000], kw[:1000], threads=a.threads)  # warm-up
    t = time.perf_counter()
    e, _, _ = du.pairs(seq, a.kmer, jw, kw, threads=a.threads)
    dt = time.perf_counter() - t
    res.update(cpu_threads=a.threads, cpu_sample_duplexes=len(pl), cpu_duplexes_per_s=len(pl) / dt,
               cpu_scan_s_scaled=nd / (len(pl) / dt), speedup=(nd / (ms / 1e3)) / (len(pl) / dt))
    # the sampled rows agree with the GPU's hits
    want = sorted((jw[x], kw[x], int(e[x])) for x in range(len(pl)) if e[x] < a.cutoff * 100)
    got = sorted((int(h["j_win"]), int(h["k_win"]), int(h["energy"])) for h in hits if int(h["j_win"]) in set(jw))
    res["sample_rows_agree"] = want == got

    sweep = {}
    sseq = record(a.sweep_L)
    for k in [int(x) for x in a.sweep.split(",") if x]:
        eng.lri_scan(sseq, k, 1, a.cutoff * 100)
        eng.lri_scan(sseq, k, 1, a.cutoff * 100)
        m, n = eng.lri_scan_time()
        sweep[str(k)] = dict(ms=m, duplexes=n, duplexes_per_s=n / (m / 1e3))
        print("k = %d on %d nt: %.1f ms, %.3g duplexes/s" % (k, a.sweep_L, m, n / (m / 1e3)), flush=True)
    res["k_sweep"] = dict(L=a.sweep_L, by_k=sweep)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
