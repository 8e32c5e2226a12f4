#!/usr/bin/env python3
"""Cost of the interval estimates of a store on the C3 run (65 536 chains x 16-D, 500 + 1000): one mass
(0.9) and three probabilities (0.05, 0.5, 0.95); one warm call, then --reps timed -- every stage with HIP events
(mcx_debug_intervals_times) -- against mcx_samples_rank_summary over the same range in the same process
(mcx_debug_rank_summary_times), the yardstick: it sorts every column twice and runs the summary's mixing passes four times.

The model, stated before the measurement: the 1 + nprobs mixing runs are the summary's autocovariance passes each, on this unmixed
store some 130 ms a run (profiles/summary_c3.txt), and dominate; a transform sweep reads and writes the store once; the keys and
the four sort passes are section 11's (4 + 4 x 12 B per key); k_hdi_windows reads (1 + nmass) x 4 B per key; k_hdi_reduce and
k_iv_pick touch a few kilobytes.

  python tools/intervals_bench.py [--out profiles/intervals_c3.txt] [--reps 3] [--np 16] [--nc 65536]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import mcpar_amd as M  # noqa: E402
from mcpar_amd import engine as E  # noqa: E402

HDI, PROBS = (0.9,), (0.05, 0.5, 0.95)
STAGES = ("summary_spread", "k_iv_transform x 4", "summary_mixing x 4", "k_iv_keys", "sort pass 0", "sort pass 1", "sort pass 2",
          "sort pass 3", "k_hdi_windows", "k_hdi_reduce", "k_iv_pick", "whole intervals call")


def device_line():
    name, cu, mem = M.device_info()
    name = name.strip()
    if name.startswith("("):
        name = name.strip("()") + " (the runtime reports no device name)"
    return "device: %s, %d CUs, %.0f GB" % (name, cu, mem / 1e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intervals_c3.txt"))
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
    N, ncol = nsamp * n, d + 1
    geo = E.debug_intervals_geometry(nsamp, n, d, len(HDI), len(PROBS))
    store_bytes = 4.0 * N * ncol
    lines = ["intervals of the C3 store: %d chains x %d-D, %d + %d: N = %d values in each of %d columns, %.2f GB; masses %s, "
             "probabilities %s" % (n, d, nburn, nsamp, N, ncol, store_bytes / 1e9, HDI, PROBS), device_line(),
             "geometry: %d window tiles of %d starts and %d sort tiles a column; a slab of %d (w, i) pairs a column; %d transforms; "
             "up to %d columns sorted at a time; %.2f GB of transformed store, then %.1f MB of scratch a column"
             % (geo["window_tiles"], geo["window_tile"], geo["sort_tiles"], geo["slab_entries"], geo["transforms"], geo["group_cols"],
                geo["store_scratch_bytes"] / 1e9, geo["scratch_bytes_per_col"] / 1e6)]
    eg.rank_summary_times(0, nsamp)  # warm
    ys = np.array([eg.rank_summary_times(0, nsamp)[19] for _ in range(a.reps)])
    yard = ys.min()
    lines.append("mcx_samples_rank_summary over the same range, the yardstick: %s ms; best %.2f ms" % (" ".join("%.2f" % v for v in ys), yard))
    eg.intervals_times(HDI, PROBS, 0, nsamp)  # warm
    t = np.array([eg.intervals_times(HDI, PROBS, 0, nsamp) for _ in range(a.reps)])
    gbs = {3: 8.0 * N * ncol, 8: (1 + len(HDI)) * 4.0 * N * ncol}
    for k in range(4, 8):
        gbs[k] = 12.0 * N * ncol
    gbs[1] = 2.0 * store_bytes * (1 + len(PROBS))
    lines.append("Engine.intervals(hdi=%s, probs=%s), HIP events:" % (HDI, PROBS))
    for k, name in enumerate(STAGES):
        best = t[:, k].min()
        s = "  %-22s %s ms; best %.3f ms = %.3f x the yardstick" % (name + ":", " ".join("%.3f" % v for v in t[:, k]), best, best / yard)
        if k in gbs:
            s += "; %.2f TB/s of its model's bytes" % (gbs[k] / best / 1e9)
        lines.append(s)
    r = eg.intervals(HDI, PROBS)
    lines.append("what it says of the run (a column a line: mean sd mcse_sd ess_sd | hdi90 | q05 q50 q95 | mcse_q | ess_q):")
    for c in range(ncol):
        q = r["quantiles"]
        lines.append("  %-3s %8.4f %7.4f %.2g %6.0f | %8.4f %8.4f | %s | %s | %s"
                     % ("p%d" % c if c < d else "LL", r["mean"][c], r["sd"][c], r["mcse_sd"][c], r["ess_sd"][c], r["hdi"]["lo"][c, 0],
                        r["hdi"]["hi"][c, 0], " ".join("%8.4f" % v for v in q["q"][c]), " ".join("%.2g" % v for v in q["mcse_q"][c]),
                        " ".join("%.0f" % v for v in q["ess_q"][c])))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
