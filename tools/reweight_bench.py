#!/usr/bin/env python3
"""Cost of importance weights on a store on the C3 run (65 536 chains x 16-D, 500 + 1000): the power
posterior L^0.5 (MCX_WEIGHT_LL, scale -0.5), three probabilities, and 10^6 resampled rows; one warm call, then --reps timed --
every stage with HIP events (mcx_debug_reweight_times) -- against k_sum_moments over the same range in the same process
(mcx_debug_covariance_times' first stage), the yardstick: one read of the store.

The model, stated before the measurement: k_rw_max and k_rw_q move 4 to 8 B per row (well under a tenth of a yardstick for 17
columns); the two moment passes and the four histogram passes are one read of the store plus q each (two and four yardsticks);
the sort is section 11's 12 B per key and pass for one column (about 0.7 yardsticks for four passes); the draw is bound by its
gather (10^6 rows of 68 B: microseconds, next to the walk of a scan tile per draw).

  python tools/reweight_bench.py [--out profiles/reweight_c3.txt] [--reps 3] [--np 16] [--nc 65536] [--draws 1000000]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import mcpar_amd as M  # noqa: E402
from mcpar_amd import engine as E  # noqa: E402

# (name, the model in yardsticks for the C3 shape -- None: no model of its own)
STAGES = (("k_rw_max + reducer", "4 B/row"), ("k_rw_q + scan", "8 B/row"), ("k_rw_moments x 2", "2 reads of the store + q"),
          ("k_rw_hist x 4 + host walks", "4 reads of the store + q"), ("sort of q (4 passes)", "12 B per key and pass"),
          ("k_rw_draw", "the gather"), ("whole reweight call", None), ("whole resample call", None))


def device_line():
    name, cu, mem = M.device_info()
    name = name.strip()
    if name.startswith("("):
        name = name.strip("()") + " (the runtime reports no device name)"
    return "device: %s, %d CUs, %.0f GB" % (name, cu, mem / 1e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reweight_c3.txt"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--np", type=int, default=16)
    ap.add_argument("--nc", type=int, default=65536)
    ap.add_argument("--nsamp", type=int, default=1000)
    ap.add_argument("--draws", type=int, default=1000000)
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
    nc_out = 1000 if a.draws % 1000 == 0 else 1
    geo = E.debug_reweight_geometry(N, ncol, 3, a.draws)
    store_bytes = 4.0 * N * ncol
    lines = ["reweight of the C3 store to L^0.5: %d chains x %d-D, %d + %d: N = %d rows of %d columns, %.2f GB; 3 probabilities, "
             "%d resampled rows" % (n, d, nburn, nsamp, N, ncol, store_bytes / 1e9, a.draws), device_line(),
             "geometry: %d scan tiles of %d rows; histogram launches of up to %d prefixes on tiles %d columns wide, %d B of LDS a "
             "workgroup (budget %d B of bins); tail of %d weights, %d sort tiles; %d draw workgroups; %.1f MB of per-call scratch"
             % (geo["scan_tiles"], geo["scan_tile_rows"], geo["hist_prefixes"], geo["hist_tile_cols"], geo["hist_lds_bytes"],
                geo["hist_lds_budget"], geo["tail_m"], geo["sort_tiles"], geo["draw_workgroups"], geo["scratch_bytes"] / 1e6)]
    eg.covariance_times(0, nsamp)  # warm
    ys = np.array([eg.covariance_times(0, nsamp)[0] for _ in range(a.reps)])
    yard = ys.min()
    lines.append("k_sum_moments over the same range, the yardstick: %s ms; best %.3f ms = %.2f TB/s for one read of the store"
                 % (" ".join("%.3f" % v for v in ys), yard, store_bytes / yard / 1e9))
    model = (4.0 * N / store_bytes, 8.0 * N / store_bytes, 2.0 * (1.0 + 1.0 / ncol), 4.0 * (1.0 + 1.0 / ncol), 4 * 12.0 * N / store_bytes, None,
             None, None)
    w = E.weights_loglike(0.5 - 1.0)
    args = dict(probs=(0.05, 0.5, 0.95), nsteps_out=a.draws // nc_out, nc_out=nc_out, seed=1)
    eg.reweight_times(w, **args)  # warm
    t = np.array([eg.reweight_times(w, **args) for _ in range(a.reps)])
    lines.append("Engine.reweight(weights_loglike(-0.5)) and Engine.resample(%d x %d), HIP events:" % (a.draws // nc_out, nc_out))
    for k, (name, what) in enumerate(STAGES):
        best = t[:, k].min()
        s = "  %-28s %s ms; best %.3f ms = %.2f x the yardstick" % (name + ":", " ".join("%.3f" % v for v in t[:, k]), best, best / yard)
        if model[k] is not None:
            s += "; model (%s) %.2f x: %.1f times its model" % (what, model[k], best / yard / model[k])
        lines.append(s)
    r = eg.reweight(w)
    lines.append("what it says of the run: ess_kish %.0f of %d rows, log_mean_w %.4f, khat %.3f (tail of %d), %d rows of weight zero"
                 % (r["ess_kish"], r["n"], r["log_mean_w"], r["khat"], r["tail_m"], r["nzero"]))
    lines.append("  mean %s" % " ".join("%.4f" % v for v in r["cols"]["mean"]))
    lines.append("  sd   %s" % " ".join("%.4f" % v for v in r["cols"]["sd"]))
    lines.append("  mcse %s" % " ".join("%.2g" % v for v in r["cols"]["mcse_mean"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
