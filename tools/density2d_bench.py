#!/usr/bin/env python3
"""Cost of a pair density call on the C3 store (65 536 chains x 16-D, 500 + 1000): all 136 pairs at g = 64 and at g = 32, and
one pair alone.  Per case one warm call, then three timed -- the three kernels with HIP events, the statistics passes, the
host grids and finish and the whole call by the wall clock (mcx_debug_density2d_times) -- against the column-sum sweep
k_sum_moments of the same process (mcx_debug_covariance_times), which reads the same rows once.  DESIGN.md section 15 holds
the model the last lines compare the pair sweep with.

  python tools/density2d_bench.py [--out profiles/density2d_c3.txt] [--reps 3] [--np 16] [--nc 65536]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import mcpar_amd as M  # noqa: E402
from density_bench import device_line  # noqa: E402

STAGES = ("statistics passes (wall)", "k_density2d_codes (HIP events)", "k_density2d_pairs (HIP events)",
          "k_density2d_reduce (HIP events)", "host grids and finish (wall)", "whole call (wall)")
# section 15's model of the pair sweep: the code columns of a pair are read once per pair at the rate the yardstick reads the
# store (they come from L2 / MALL where the pairs of a chunk run together, so this is the floor of the model, not its guess),
# and a CU retires one 64-lane ds_add_u64 per LDS_CLK clocks
LDS_CLK, CLOCK_GHZ = 8.0, 2.4


def model_ms(N, npairs, cus, yard_tbs):
    read_ms = npairs * 2 * 4.0 * N / yard_tbs / 1e9
    lds_ms = npairs * 2.0 * N / 64.0 / cus * LDS_CLK / CLOCK_GHZ / 1e6
    return read_ms, lds_ms


def report(lines, what, times, reps, yardstick, N, npairs, cus, yard_tbs):
    times()  # warm
    t = np.array([times() for _ in range(reps)])
    lines.append(what)
    for k, name in enumerate(STAGES):
        best = t[:, k].min()
        tail = "; %.2f x the yardstick" % (best / yardstick) if 1 <= k <= 3 else ""
        lines.append("  %-34s %s ms; best %.3f ms%s" % (name + ":", " ".join("%.3f" % v for v in t[:, k]), best, tail))
    best = t[:, 2].min()
    read_ms, lds_ms = model_ms(N, npairs, cus, yard_tbs)
    lines.append("  the pair sweep: %.2f G rows x pairs / s, %.2f TB/s of codes; the model: %.3f ms of code reads, %.3f ms of LDS "
                 "adds, the larger %.3f ms -- measured / model = %.2f"
                 % (npairs * N / best / 1e6, npairs * 8.0 * N / best / 1e9, read_ms, lds_ms, max(read_ms, lds_ms),
                    best / max(read_ms, lds_ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density2d_c3.txt"))
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
    ncol = d + 1
    npairs = ncol * (ncol - 1) // 2
    cus = M.device_info()[1]
    lines = ["pair densities of the C3 store: %d chains x %d-D, %d + %d, N = %d rows, %.2f GB of rows, %d pairs"
             % (n, d, nburn, nsamp, N, rbytes / 1e9, npairs),
             device_line()]
    eg.covariance_times()  # warm
    mom = [eg.covariance_times()[0] for _ in range(a.reps)]
    yard = min(mom)
    yard_tbs = rbytes / yard / 1e9
    lines.append("column-sum sweep (k_sum_moments), the yardstick: %s ms; best %.3f ms = %.2f TB/s read"
                 % (" ".join("%.3f" % v for v in mom), yard, yard_tbs))
    for G in (64, 32):
        report(lines, "Engine.density2d(g = %d), all %d pairs:" % (G, npairs), lambda: eg.density2d_times(g=G), a.reps, yard, N,
               npairs, cus, yard_tbs)
    report(lines, "Engine.density2d(g = 64, pairs = [(0, 1)]):", lambda: eg.density2d_times(g=64, pairs=[(0, 1)]), a.reps, yard, N, 1,
           cus, yard_tbs)
    one = eg.density2d(g=64, pairs=[(0, 1), (1, 0), (15, 16)])
    assert np.all(one["nbinned"] == N) and np.all(one["flags"] == 0)
    assert one["z"][1].tobytes() == np.ascontiguousarray(one["z"][0].T).tobytes()
    lines.append("check: nbinned = N for (0, 1), (1, 0), (15, 16); z of (1, 0) is the transpose of (0, 1)'s")
    # the sum of z over the nodes times the cell: 1 where the nodes resolve the kernel (delta <= h), above 1 where they do not
    for adjust in (1.0, 8.0):
        r = eg.density2d(g=64, pairs=[(0, 1)], adjust=adjust)
        delta = [np.diff(r["axes"][c])[0] for c in (0, 1)]
        lines.append("  adjust = %g: delta / h = %.2f, %.2f for p0, p1; sum of z x cell over the nodes of (p0, p1) = %.4f"
                     % (adjust, delta[0] / r["bw"][0], delta[1] / r["bw"][1], r["z"][0].sum() * delta[0] * delta[1]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
