#!/usr/bin/env python3
"""Cost of mcx_samples_summary on the C3 store (65 536 chains x 16-D, 500 + 1000): one warm call, then the median of
10 timed with HIP events (on the engine's stream) and the wall clock; the 32-lag autocovariance windows the columns
needed; once, the host route it replaces (mcx_samples_copy of the store + the float64 numpy restatement).

  python tools/summary_bench.py [--out profiles/summary_c3.txt] [--no-host] [--reps 10]
Per-pass kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/summary_bench.py --no-host`."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import mcpar_amd as M  # noqa: E402
from mcpar_amd import engine as E  # noqa: E402
import summary_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "summary_c3.txt"))
    ap.add_argument("--no-host", action="store_true", help="skip the host route")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    d, n, nburn, nsamp = 16, 65536, 500, 1000
    probs = (0.01, 0.5, 0.99)
    M.load().mcx_set_device(0)
    vl, keep = M.make_vlfunc(M.VL_ROSENBROCK1, d)
    eg = M.Engine(d, n, pl=1.0)
    g = np.arange(n, dtype=np.float64)[:, None]
    i = np.arange(d, dtype=np.float64)[None, :]
    eg.run(nsamp, nburn, (0.5 * np.sin(0.37 * (g * d + i))).astype(np.float32), vl)
    eg.synchronize()
    # HIP events on a stream of our own, through the HIP runtime libmcx.so itself uses
    hip = C.CDLL("libamdhip64.so.7")
    st, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(st)) == 0
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    eg.set_option(E.OPT_STREAM, st.value)
    s = eg.summary(probs)  # warm
    gpu, wall = [], []
    ms = C.c_float()
    for _ in range(a.reps):
        hip.hipEventRecord(e0, st)
        t0 = time.perf_counter()
        eg.summary(probs)
        t1 = time.perf_counter()
        hip.hipEventRecord(e1, st)
        assert hip.hipEventSynchronize(e1) == 0
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        gpu.append(ms.value)
        wall.append((t1 - t0) * 1e3)
    nwin = eg.summary_windows()
    gbytes = nsamp * n * (d + 1) * 4 / 1e9
    lines = ["mcx_samples_summary on the C3 store: %d chains x %d-D, %d + %d, %.2f GB of rows, probs %s"
             % (n, d, nburn, nsamp, gbytes, probs),
             "device: %s" % (M.device_info()[0],),
             "summary: median of %d: %.2f ms (HIP events), %.2f ms (wall); min %.2f / %.2f ms"
             % (a.reps, np.median(gpu), np.median(wall), min(gpu), min(wall)),
             "lag windows of 32 computed (all columns together): %d" % nwin,
             "ess_lag per column (p0..p15, LL): %s" % " ".join(str(int(v)) for v in s["ess_lag"]),
             "rhat per column: %s" % " ".join("%.4f" % v for v in s["rhat"]),
             "ess per column: %s" % " ".join("%.0f" % v for v in s["ess"])]
    if not a.no_host:
        t0 = time.perf_counter()
        rows = eg.samples
        t1 = time.perf_counter()
        x = rows.reshape(nsamp, n, d + 1)
        for c in range(d + 1):
            R.restate_column(np.ascontiguousarray(x[:, :, c]), probs)
        t2 = time.perf_counter()
        lines.append("host route: mcx_samples_copy %.2f s + numpy restatement of %d columns %.2f s = %.2f s"
                     % (t1 - t0, d + 1, t2 - t1, t2 - t0))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
