#!/usr/bin/env python3
"""Cost of mcx_samples_rank_summary on the C3 store (65 536 chains x 16-D, 500 + 1000) against mcx_samples_summary on the
same store in the same process: one warm call of each, then --reps timed ones (wall clock around the whole call; both
calls wait for their own results), and the stages of the rank summary with HIP events (mcx_debug_rank_summary_times): key
extraction, every sort pass, rank look-up and transform, the summary passes of each of the four transformed stores.

  python tools/rank_summary_bench.py [--out profiles/rank_summary_c3.txt] [--reps 3] [--np 16] [--nc 65536] [--nsamp 1000]
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/rank_summary_bench.py --out ''`."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import mcpar_amd as M  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_summary_c3.txt"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--np", type=int, default=16)
    ap.add_argument("--nc", type=int, default=65536)
    ap.add_argument("--nsamp", type=int, default=1000)
    a = ap.parse_args()
    d, n, nburn, nsamp = a.np, a.nc, 500, a.nsamp
    M.load().mcx_set_device(0)
    vl, keep = M.make_vlfunc(M.VL_ROSENBROCK1, d)
    eg = M.Engine(d, n, pl=1.0)
    g = np.arange(n, dtype=np.float64)[:, None]
    i = np.arange(d, dtype=np.float64)[None, :]
    eg.run(nsamp, nburn, (0.5 * np.sin(0.37 * (g * d + i))).astype(np.float32), vl)
    eg.synchronize()
    probs = (0.05, 0.5, 0.95)
    basic = eg.summary(probs)  # warm
    rank = eg.rank_summary()   # warm
    t_basic, t_rank, parts = [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        eg.summary(probs)
        t1 = time.perf_counter()
        eg.rank_summary()
        t2 = time.perf_counter()
        t_basic.append((t1 - t0) * 1e3)
        t_rank.append((t2 - t1) * 1e3)
        parts.append(eg.rank_summary_times())
    p = np.array(parts).min(axis=0)
    N = nsamp * n
    ncol = d + 1
    keys = N * ncol
    store = keys * 4
    fmt = lambda v: " ".join("%.2f" % x for x in v)  # noqa: E731
    lines = ["mcx_samples_rank_summary on the C3 store: %d chains x %d-D, %d + %d, %.2f GB of rows, %.3g keys per transform"
             % (n, d, nburn, nsamp, store / 1e9, keys),
             "device: %s" % (M.device_info()[0],),
             "mcx_samples_summary, probs (0.05, 0.5, 0.95), %d after one warm-up: %s ms (wall)" % (a.reps, fmt(t_basic)),
             "mcx_samples_rank_summary, %d after one warm-up: %s ms (wall)" % (a.reps, fmt(t_rank)),
             "ratio of the best of each: %.2f" % (min(t_rank) / min(t_basic)),
             "stages (HIP events, best of %d; ms):" % a.reps,
             "  thresholds (moments + order statistics):                 %8.2f" % p[18]]
    for s, name in ((0, "values"), (1, "folded")):
        o = 7 * s
        sort = p[o + 1:o + 5]
        lines += ["  %s: key extraction                                   %8.2f  (%.2f TB/s of rows and keys)"
                  % (name, p[o], 2 * store / p[o] / 1e9),
                  "  %s: sort passes (count, scan, scatter each)   %s  = %.2f  (%.2f TB/s at 12 B per key and pass)"
                  % (name, fmt(sort), sort.sum(), 12.0 * keys * 4 / sort.sum() / 1e9),
                  "  %s: rank look-up and transform                       %8.2f" % (name, p[o + 5]),
                  "  %s: summary passes of the transformed store          %8.2f" % (name, p[o + 6])]
    lines += ["  x <= q05: indicator %.2f, summary passes %.2f" % (p[14], p[15]),
              "  x <= q95: indicator %.2f, summary passes %.2f" % (p[16], p[17]),
              "  whole call %.2f; the four summary runs %.2f, the sorts %.2f, keys + look-ups %.2f"
              % (p[19], p[6] + p[13] + p[15] + p[17], p[1:5].sum() + p[8:12].sum(), p[0] + p[5] + p[7] + p[12]),
              "largest rhat %.4f (basic %.4f); smallest ess_bulk %.0f, ess_tail %.0f (basic ess %.0f)"
              % (np.nanmax(rank["rhat"]), np.nanmax(basic["rhat"]), np.nanmin(rank["ess_bulk"]), np.nanmin(rank["ess_tail"]),
                 np.nanmin(basic["ess"]))]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
