#!/usr/bin/env python3
"""Cost of the profile likelihoods on the C3 store (65 536 chains x 16-D, 500 + 1000): one warm call, then three timed -- the
sweep k_profile_bins with HIP events, the statistics passes, the host grids and finish and the whole call by the wall clock
(mcx_debug_profile_times); the pair call's code and key sweeps, k_profile_pairs and k_profile_at (mcx_debug_profile2d_times) --
against the column-sum sweep k_sum_moments (mcx_debug_covariance_times) and the density sweep k_density_bins
(mcx_debug_density_times) of the same process, and against numpy on copied rows of a sub-range, scaled up.

  python tools/profile_bench.py [--out profiles/profile_c3.txt] [--reps 3] [--np 16] [--nc 65536]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import mcpar_amd as M  # noqa: E402

STAGES1 = ("statistics passes (wall)", "k_profile_bins (HIP events)", "host grids and finish (wall)", "whole call (wall)")
STAGES2 = ("statistics passes (wall)", "k_profile_codes + k_profile_keys", "k_profile_pairs", "k_profile_at", "host grids and finish (wall)",
           "whole call (wall)")


def device_line():
    name, cu, mem = M.device_info()
    name = name.strip()
    if name.startswith("("):
        name = name.strip("()") + " (the runtime reports no device name)"
    return "device: %s, %d CUs, %.0f GB" % (name, cu, mem / 1e9)


def report(lines, what, times, reps, stages):
    times()  # warm
    t = np.array([times() for _ in range(reps)])
    lines.append(what)
    for k, name in enumerate(stages):
        lines.append("  %-34s %s ms; best %.3f ms" % (name + ":", " ".join("%.3f" % v for v in t[:, k]), t[:, k].min()))
    return t.min(axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "profile_c3.txt"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--np", type=int, default=16)
    ap.add_argument("--nc", type=int, default=65536)
    a = ap.parse_args()
    d, n, nburn, nsamp = a.np, a.nc, 500, 1000
    M.load().mcx_set_device(0)
    vl, keep = M.make_vlfunc(M.VL_ROSENBROCK1, d)
    eg = M.Engine(d, n, pl=1.0)
    g = np.arange(n, dtype=np.float64)[:, None]
    i = np.arange(d, dtype=np.float64)[None, :]
    eg.run(nsamp, nburn, (0.5 * np.sin(0.37 * (g * d + i))).astype(np.float32), vl)
    eg.synchronize()
    N = nsamp * n
    rbytes = 4.0 * N * (d + 1)
    lines = ["profile likelihoods of the C3 store: %d chains x %d-D, %d + %d, N = %d rows, %.2f GB of rows" % (n, d, nburn, nsamp, N, rbytes / 1e9),
             device_line()]
    eg.covariance_times()  # warm
    mom = min(eg.covariance_times()[0] for _ in range(a.reps))
    lines.append("column-sum sweep (k_sum_moments), the yardstick: best %.3f ms = %.2f TB/s read" % (mom, rbytes / mom / 1e9))
    eg.density_times()  # warm
    dens = min(eg.density_times()[1] for _ in range(a.reps))
    lines.append("density sweep (k_density_bins, n = 512, all %d columns): best %.3f ms = %.2f x the yardstick" % (d + 1, dens, dens / mom))
    for nb in (64, 512):
        b = report(lines, "Engine.profile_likelihood(n = %d), %d columns:" % (nb, d), lambda: eg.profile_likelihood_times(n=nb), a.reps, STAGES1)
        lines.append("  the sweep: %.2f TB/s read; %.2f x the yardstick; %.2f x k_density_bins" % (rbytes / b[1] / 1e9, b[1] / mom, b[1] / dens))
    pairs = [(0, 1), (2, 3), (0, 15), (7, 8)]
    for gg in (32, 64):
        b = report(lines, "Engine.profile_likelihood2d(g = %d), %d pairs:" % (gg, len(pairs)),
                   lambda: eg.profile_likelihood2d_times(g=gg, pairs=pairs), a.reps, STAGES2)
        lines.append("  the pair sweep: %.3f ms a pair, %.2f TB/s of codes and keys" % (b[2] / len(pairs), 10.0 * N * len(pairs) / b[2] / 1e9))
    # numpy on copied rows of a sub-range, scaled up
    import profile_ref as R
    sub = 4
    t0 = time.perf_counter()
    rows = eg.samples_range(0, sub)
    t_copy = time.perf_counter() - t0
    t0 = time.perf_counter()
    K = R.row_keys(rows[:, d])
    for c in range(d):
        gr = R.grid_of(rows[:, c], 64)
        R.max_keys(R.bins_of(rows[:, c], 64, *gr), K, 64)
    t_np = time.perf_counter() - t0
    lines.append("numpy on %d copied steps (%d rows): copy %.3f s, keys and bins of %d columns %.3f s; scaled to %d steps: %.1f s + %.1f s"
                 % (sub, sub * n, t_copy, d, t_np, nsamp, t_copy * nsamp / sub, t_np * nsamp / sub))
    got = eg.profile_likelihood(n=64)
    assert np.all(got["nbinned"] == N) and np.all(got["flags"] == 0)
    lm, _ = eg.maxlike()
    assert np.float32(got["lhat"][0]) == np.float32(lm)
    lines.append("lhat = %.6g at row %d; the 68.27 %% intervals of p0, p1: [%.4f, %.4f] [%.4f, %.4f] (hull [%.4f, %.4f] [%.4f, %.4f])"
                 % (got["lhat"][0], got["row_hat"][0], got["intervals"]["lo"][0, 0], got["intervals"]["hi"][0, 0], got["intervals"]["lo"][1, 0],
                    got["intervals"]["hi"][1, 0], got["intervals"]["lo_hull"][0, 0], got["intervals"]["hi_hull"][0, 0],
                    got["intervals"]["lo_hull"][1, 0], got["intervals"]["hi_hull"][1, 0]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
