#!/usr/bin/env python3
"""Cost of comparing two stores on the C3 run (65 536 chains x 16-D, 500 + 1000): the first against the
second 500 kept steps, one warm call, then --reps timed -- every stage with HIP events (mcx_debug_compare_times) -- against the
four sort passes of section 11 on one of the halves in the same process (mcx_debug_rank_summary_times), the yardstick: a
comparison sorts both sides once, so its two sorts should cost two yardsticks, and the merge sweeps well under one sort pass.

  python tools/compare_bench.py [--out profiles/compare_c3.txt] [--reps 3] [--np 16] [--nc 65536]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import mcpar_amd as M  # noqa: E402
from mcpar_amd import engine as E  # noqa: E402

STAGES = ("the two sides' summaries", "k_cmp_keys of A", "sort of A (4 passes)", "k_cmp_keys of B", "sort of B (4 passes)",
          "k_cmp_bounds (both sides)", "k_cmp_sweep, self = A", "k_cmp_sweep, self = B", "k_cmp_reduce", "whole call")


def device_line():
    name, cu, mem = M.device_info()
    name = name.strip()
    if name.startswith("("):
        name = name.strip("()") + " (the runtime reports no device name)"
    return "device: %s, %d CUs, %.0f GB" % (name, cu, mem / 1e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compare_c3.txt"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--np", type=int, default=16)
    ap.add_argument("--nc", type=int, default=65536)
    a = ap.parse_args()
    d, n, nburn, nsamp = a.np, a.nc, 500, 1000
    half = nsamp // 2
    M.load().mcx_set_device(0)
    vl, keep = M.make_vlfunc(M.VL_ROSENBROCK1, d)
    eg = M.Engine(d, n, pl=1.0)
    g = np.arange(n, dtype=np.float64)[:, None]
    i = np.arange(d, dtype=np.float64)[None, :]
    eg.run(nsamp, nburn, (0.5 * np.sin(0.37 * (g * d + i))).astype(np.float32), vl)
    eg.synchronize()
    N = half * n
    geo = E.debug_compare_geometry(N, N, d + 1)
    lines = ["compare of the C3 store's halves: %d chains x %d-D, %d + %d, steps [0, %d) against [%d, %d): N = %d values per column "
             "and side, %d columns, %.2f GB of keys per side" % (n, d, nburn, nsamp, half, half, nsamp, N, d + 1, 4.0 * N * (d + 1) / 1e9),
             device_line(),
             "geometry: %d + %d sweep tiles of %d keys per column, windows of at most %d keys in LDS (%d B a workgroup), %d columns at "
             "a time, %.1f MB of scratch per column" % (geo["tiles_a"], geo["tiles_b"], geo["tile_keys"], geo["window_lds_keys"],
                                                        geo["lds_bytes"], geo["group_cols"], geo["scratch_bytes_per_col"] / 1e6)]
    eg.rank_summary_times(0, half)  # warm
    rs = np.array([eg.rank_summary_times(0, half) for _ in range(a.reps)])
    sort = rs[:, 1:5].sum(axis=1)
    yard = sort.min()
    lines.append("section 11's four sort passes of one half, the yardstick: %s ms; best %.3f ms = %.2f TB/s at 12 B per key and pass"
                 % (" ".join("%.3f" % v for v in sort), yard, 4 * 12.0 * N * (d + 1) / yard / 1e9))
    eg.compare_times(0, half, half, half)  # warm
    t = np.array([eg.compare_times(0, half, half, half) for _ in range(a.reps)])
    lines.append("Engine.compare(0, %d, %d, %d), HIP events:" % (half, half, half))
    for k, name in enumerate(STAGES):
        best = t[:, k].min()
        lines.append("  %-28s %s ms; best %.3f ms = %.2f x the yardstick" % (name + ":", " ".join("%.3f" % v for v in t[:, k]), best, best / yard))
    merge = t[:, 5:9].sum(axis=1).min()
    lines.append("  bounds + both sweeps + reduce: best %.3f ms = %.2f of one sort pass" % (merge, merge / (yard / 4)))
    r = eg.compare(0, half, half, half)
    lines.append("what it says of the run's halves: ks %s" % " ".join("%.4f" % v for v in r["ks"]))
    lines.append("  ks_neff %s" % " ".join("%.0f" % v for v in r["ks_neff"]))
    lines.append("  ks_p %s" % " ".join("%.3g" % v for v in r["ks_p"]))
    lines.append("  z_mean %s" % " ".join("%.2f" % v for v in r["z_mean"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
