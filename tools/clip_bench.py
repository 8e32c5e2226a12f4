#!/usr/bin/env python3
"""Cost of a tail clip on the C3 store (65 536 chains x 16-D, 500 + 1000), spec (0.01, 0.99, ll_hi = 0): one warm call, then
three timed -- the mark sweep, the scan and the scatter sweep with HIP events, the thresholds (the summary's quantile
passes) and the whole call by the wall clock (mcx_debug_clip_times) -- against the column-sum sweep k_sum_moments of the same
process (mcx_debug_covariance_times), which reads the same rows once.  The model: mark reads 4 N (np + 1) bytes, the
yardstick's time; scatter reads them again and writes K (4 (np + 1) + 8) bytes; the scan is negligible.

  python tools/clip_bench.py [--out profiles/clip_c3.txt] [--reps 3] [--np 16] [--nc 65536]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import mcpar_amd as M  # noqa: E402

STAGES = ("thresholds (wall)", "k_clip_mark (HIP events)", "k_clip_scan (HIP events)", "k_clip_scatter (HIP events)", "whole call (wall)")


def device_line():
    """name (architecture), CUs, memory -- the runtime of some boxes reports an empty name: the architecture string then"""
    name, cu, mem = M.device_info()
    name = name.strip()
    if name.startswith("("):
        name = name.strip("()") + " (the runtime reports no device name)"
    return "device: %s, %d CUs, %.0f GB" % (name, cu, mem / 1e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_c3.txt"))
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
    lines = ["clip of the C3 store: %d chains x %d-D, %d + %d, N = %d rows, %.2f GB of rows, spec (0.01, 0.99, ll_hi = 0)"
             % (n, d, nburn, nsamp, N, rbytes / 1e9),
             device_line()]
    eg.covariance_times()  # warm
    mom = [eg.covariance_times()[0] for _ in range(a.reps)]
    yard = min(mom)
    lines.append("column-sum sweep (k_sum_moments), the yardstick: %s ms; best %.3f ms = %.2f TB/s read"
                 % (" ".join("%.3f" % v for v in mom), yard, rbytes / yard / 1e9))
    eg.clip_times()  # warm
    t = np.array([eg.clip_times() for _ in range(a.reps)])
    lines.append("Engine.clip() of the run's store:")
    for k, name in enumerate(STAGES):
        lines.append("  %-30s %s ms; best %.3f ms" % (name + ":", " ".join("%.3f" % v for v in t[:, k]), t[:, k].min()))
    co = eg.clip(count_only=True)
    K = co.nrows
    assert co.nsource == N and not co.report["flags"].any()
    wbytes = K * (4.0 * (d + 1) + 8.0)
    mark, scan, scat = t[:, 1].min(), t[:, 2].min(), t[:, 3].min()
    model = yard * (2.0 * rbytes + wbytes) / rbytes  # the bytes of mark and scatter at the yardstick's own rate
    lines.append("  kept K = %d of N = %d rows (%.4f); the scatter writes %.2f GB" % (K, N, K / N, wbytes / 1e9))
    lines.append("  mark: %.2f TB/s read, %.2f x the yardstick; scatter: %.2f TB/s read and written, %.2f x the yardstick"
                 % (rbytes / mark / 1e9, mark / yard, (rbytes + wbytes) / scat / 1e9, scat / yard))
    lines.append("  mark + scatter: %.3f ms, the model's bytes at the yardstick's rate: %.3f ms, ratio %.2f; scan %.3f ms"
                 % (mark + scat, model, (mark + scat) / model, scan))
    lines.append("  tails: nbelow %s" % " ".join(str(v) for v in co.report["nbelow"]))
    lines.append("         nabove %s" % " ".join(str(v) for v in co.report["nabove"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
