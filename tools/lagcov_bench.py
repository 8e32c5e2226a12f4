#!/usr/bin/env python3
"""Cost of the lagged covariance of a store on the C3 run (65 536 chains x 16-D, 500 + 1000): one warm
call, then --reps timed -- every stage with HIP events (mcx_debug_lagcov_times) -- with max_lag 64 and with every lag, against
mcx_samples_covariance's k_cov_tiles over the same range in the same process (mcx_debug_covariance_times), the yardstick: one
lag of the same contraction.  numpy on the copied rows of a sub-range (every 64th step would change the lags: the first
sub = nsamp // 64 steps are taken, 15 of 1000) is timed for min(sub, 65) lags and scaled by nsamp // sub (66) and to 65 lags, and is
marked as scaled.

The model, stated before the measurement: a window of W = 8 lags reads the rows once from HBM (about 0.9 ms, the column-sum
sweep) and the partners of its 8 lags from the caches, and issues 8 MFMAs per four rows (about 0.45 ms a lag at the nominal fp64
matrix rate); a lag should land within 1.5 x k_cov_tiles.

  python tools/lagcov_bench.py [--out profiles/lagcov_c3.txt] [--reps 3] [--np 16] [--nc 65536]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import mcpar_amd as M  # noqa: E402
from mcpar_amd import engine as E  # noqa: E402

STAGES = ("column sums", "lag 0 sweep", "window sweeps", "reducers", "whole lagcov call")


def device_line():
    name, cu, mem = M.device_info()
    name = name.strip()
    if name.startswith("("):
        name = name.strip("()") + " (the runtime reports no device name)"
    return "device: %s, %d CUs, %.0f GB" % (name, cu, mem / 1e9)


def numpy_lags(rows, T, nc, nlags):
    x = rows.astype(np.float64).reshape(T, nc, -1)
    c = x - x.reshape(T * nc, -1).sum(axis=0) / (T * nc)
    return [c[:T - t].reshape(-1, c.shape[2]).T @ c[t:].reshape(-1, c.shape[2]) / (T * nc) for t in range(nlags)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lagcov_c3.txt"))
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
    store_bytes = 4.0 * N * ncol
    geo = E.debug_lagcov_geometry(nsamp, n, d, nsamp)
    lines = ["lagged covariance of the C3 store: %d chains x %d-D, %d + %d: N = %d rows of %d columns, %.2f GB"
             % (n, d, nburn, nsamp, N, ncol, store_bytes / 1e9), device_line(),
             "geometry: windows of %d lags; %d units of %d rows over %d workgroups; %d tile(s), %d pair(s) a lag; %d partial sums a lag "
             "and workgroup; %.1f MB of scratch" % (geo["window_lags"], geo["units"], geo["rows_per_iteration"], geo["workgroups"],
                                                    geo["tiles"], geo["pairs"], geo["slab_rows"], geo["scratch_bytes"] / 1e6)]
    eg.covariance_times(0, nsamp)  # warm
    ys = np.array([eg.covariance_times(0, nsamp) for _ in range(a.reps)])
    yard, sums = ys[:, 1].min(), ys[:, 0].min()
    lines.append("mcx_samples_covariance over the same range: column-sum sweep best %.3f ms; k_cov_tiles, the yardstick: %s ms; best "
                 "%.3f ms" % (sums, " ".join("%.3f" % v for v in ys[:, 1]), yard))
    for max_lag in (64, None):
        eg.lagcov_times(max_lag=max_lag)  # warm
        runs = [eg.lagcov_times(max_lag=max_lag) for _ in range(a.reps)]
        t, lags = np.array([r[0] for r in runs]), runs[0][1]
        windows = E.debug_lagcov_geometry(nsamp, n, d, lags)["windows"]
        lines.append("Engine.lagcov(max_lag=%s): %d lags computed in 1 + %d sweeps, HIP events:" % (max_lag, lags, windows))
        for k, name in enumerate(STAGES):
            lines.append("  %-18s %s ms; best %.3f ms" % (name + ":", " ".join("%.3f" % v for v in t[:, k]), t[:, k].min()))
        per_lag = t[:, 2].min() / max(lags - 1, 1)
        lines.append("  a lag of the window sweeps: %.3f ms = %.2f x k_cov_tiles (expected: within 1.5 x); a window: %.3f ms = %.2f x the "
                     "column-sum sweep plus %d lags at %.3f ms" % (per_lag, per_lag / yard, t[:, 2].min() / max(windows, 1),
                                                                   t[:, 2].min() / max(windows, 1) / sums, geo["window_lags"], per_lag))
        r = eg.lagcov(max_lag=max_lag)
        lines.append("  what it says of the run: p %d, s %d, k_used %d, lags_used %d, flags %d, mess %.1f of N = %d (%.3g), smallest and "
                     "largest per-column ess %.1f %.1f" % (r["p"], r["s"], r["k_used"], r["lags_used"], r["flags"], r["mess"], N,
                                                           r["mess"] / N, np.nanmin(r["ess"]), np.nanmax(r["ess"])))
    # numpy on copied rows, a 1/64 sub-range, the lags of the first call
    sub = max(nsamp // 64, 4)
    t0 = time.perf_counter()
    rows = eg.samples_range(0, sub)
    t1 = time.perf_counter()
    nl = min(sub, 65)
    numpy_lags(rows, sub, n, nl)
    t2 = time.perf_counter()
    lines.append("numpy, float64, on the copied rows of the first %d steps (1/%d of the range), %d lags: copy %.1f ms, lags %.1f ms; SCALED "
                 "by %d to the whole range: copy %.0f ms, 65 lags %.0f ms" % (sub, nsamp // sub, nl, 1e3 * (t1 - t0), 1e3 * (t2 - t1),
                                                                              nsamp // sub, 1e3 * (t1 - t0) * (nsamp // sub),
                                                                              1e3 * (t2 - t1) * (nsamp // sub) * 65 / nl))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
