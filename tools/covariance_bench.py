#!/usr/bin/env python3
"""Cost of mcx_samples_covariance on the C3 store (65 536 chains x 16-D, 500 + 1000): one warm call, then three timed --
the whole call with HIP events on the engine's stream and the wall clock, and the device passes by themselves
(mcx_debug_covariance_times): the covariance sweep against the column-sum sweep mcx_samples_summary shares, both of which
read the rows exactly once.

  python tools/covariance_bench.py [--out profiles/covariance_c3.txt] [--reps 3] [--np 16] [--nc 65536]
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/covariance_bench.py --out ''`."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import mcpar_amd as M  # noqa: E402
from mcpar_amd import engine as E  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covariance_c3.txt"))
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
    hip = C.CDLL("libamdhip64.so.7")
    st, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(st)) == 0
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    eg.set_option(E.OPT_STREAM, st.value)
    c = eg.covariance()  # warm
    gpu, wall, parts = [], [], []
    ms = C.c_float()
    for _ in range(a.reps):
        hip.hipEventRecord(e0, st)
        t0 = time.perf_counter()
        eg.covariance()
        t1 = time.perf_counter()
        hip.hipEventRecord(e1, st)
        assert hip.hipEventSynchronize(e1) == 0
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        gpu.append(ms.value)
        wall.append((t1 - t0) * 1e3)
        parts.append(eg.covariance_times())
    parts = np.array(parts)
    xbytes = nsamp * n * d * 4
    lbytes = nsamp * n * 4
    tiles = (d + 15) // 16
    pairs = tiles * (tiles + 1) // 2
    flop = 2.0 * 16 * 16 * pairs * nsamp * n
    mom, cov, red = parts.min(axis=0)
    corr = c["corr"][:d, :d] - np.eye(d)
    lines = ["mcx_samples_covariance on the C3 store: %d chains x %d-D, %d + %d, %.2f GB of rows"
             % (n, d, nburn, nsamp, (xbytes + lbytes) / 1e9),
             "device: %s" % (M.device_info()[0],),
             "whole call, %d after one warm-up: %s ms (HIP events), %s ms (wall)"
             % (a.reps, " ".join("%.2f" % v for v in gpu), " ".join("%.2f" % v for v in wall)),
             "column-sum sweep (k_sum_moments, shared with mcx_samples_summary): %s ms; best %.3f ms = %.2f TB/s"
             % (" ".join("%.3f" % v for v in parts[:, 0]), mom, (xbytes + lbytes) / mom / 1e9),
             "covariance sweep (k_cov_tiles, %d tile pair%s): %s ms; best %.3f ms = %.2f TB/s of rows, %.1f Tflop/s fp64 on the matrix cores"
             % (pairs, "" if pairs == 1 else "s", " ".join("%.3f" % v for v in parts[:, 1]), cov, (xbytes + lbytes) / cov / 1e9,
                flop / cov / 1e9),
             "reducer of its partials (k_sum_rows): best %.3f ms" % red,
             "covariance sweep / column-sum sweep: %.2f" % (cov / mom),
             "largest |correlation| between two parameters: %.4f; sd of p0, p%d: %.4f %.4f"
             % (np.abs(corr).max(), d - 1, np.sqrt(c["cov"][0, 0]), np.sqrt(c["cov"][d - 1, d - 1]))]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
