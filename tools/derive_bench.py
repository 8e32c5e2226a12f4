#!/usr/bin/env python3
"""Cost of the derive sweep and of bootstrap draws on the C3 store (65 536 chains x 16-D, 500 + 1000): one warm call, then
three timed with HIP events -- the sweep alone (mcx_debug_derive_times) for MCX_DERIVE_LINEAR with nout = 1 and nout = 16,
against the column-sum sweep k_sum_moments of the same process (mcx_debug_covariance_times), which reads the same rows once
and writes next to nothing; and 10^6 draws from the same store (the whole mcx_samples_draw call, copy to the host included).

  python tools/derive_bench.py [--out profiles/derive_c3.txt] [--reps 3] [--np 16] [--nc 65536]"""
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


def device_line():
    """name (architecture), CUs, memory -- the runtime of some boxes reports an empty name: the architecture string then"""
    name, cu, mem = M.device_info()
    name = name.strip()
    if name.startswith("("):
        name = name.strip("()") + " (the runtime reports no device name)"
    return "device: %s, %d CUs, %.0f GB" % (name, cu, mem / 1e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "derive_c3.txt"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--np", type=int, default=16)
    ap.add_argument("--nc", type=int, default=65536)
    ap.add_argument("--ndraw", type=int, default=1000000)
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
    lines = ["derive sweep and draws on the C3 store: %d chains x %d-D, %d + %d, N = %d rows, %.2f GB of rows"
             % (n, d, nburn, nsamp, N, rbytes / 1e9),
             device_line()]
    eg.covariance_times()  # warm
    mom = [eg.covariance_times()[0] for _ in range(a.reps)]
    lines.append("column-sum sweep (k_sum_moments), the yardstick: %s ms; best %.3f ms = %.2f TB/s read"
                 % (" ".join("%.3f" % v for v in mom), min(mom), rbytes / min(mom) / 1e9))
    rng = np.random.default_rng(12)
    for nout in (1, 16):
        spec = M.derive_linear(rng.standard_normal((nout, d)), rng.standard_normal(nout))
        eg.derive_times(spec)  # warm
        t = [eg.derive_times(spec) for _ in range(a.reps)]
        wbytes = 4.0 * N * (nout + 1)
        lines.append("derive sweep, LINEAR nout = %d (reads %.2f GB, writes %.2f GB): %s ms; best %.3f ms = %.2f TB/s moved; "
                     "%.2f x the yardstick" % (nout, rbytes / 1e9, wbytes / 1e9, " ".join("%.3f" % v for v in t), min(t),
                                               (rbytes + wbytes) / min(t) / 1e9, min(t) / min(mom)))
        t0 = time.perf_counter()
        st = eg.derive(spec)
        t1 = time.perf_counter()
        st.close()
        lines.append("  the whole mcx_samples_derive call (allocation, sweep, wait): %.2f ms (wall)" % ((t1 - t0) * 1e3))
    hip = C.CDLL("libamdhip64.so.7")
    stream, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    eg.set_option(E.OPT_STREAM, stream.value)
    eg.draw(a.ndraw, 1)  # warm
    gpu, wall = [], []
    ms = C.c_float()
    for r in range(a.reps):
        hip.hipEventRecord(e0, stream)
        t0 = time.perf_counter()
        rows, index = eg.draw(a.ndraw, 2 + r)
        t1 = time.perf_counter()
        hip.hipEventRecord(e1, stream)
        assert hip.hipEventSynchronize(e1) == 0
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        gpu.append(ms.value)
        wall.append((t1 - t0) * 1e3)
    assert index.min() >= 0 and index.max() < N
    # the rows are the rows of the index, at both ends and on either side of the boundary of the 64 MiB chunks
    edge = (64 << 20) // (4 * (d + 1))
    for k in sorted({0, a.ndraw - 1, min(edge - 1, a.ndraw - 1), min(edge, a.ndraw - 1)}):
        step, chain = divmod(int(index[k]), n)
        assert rows[k].tobytes() == eg.samples_range(step, 1)[chain].tobytes(), k
    lines.append("%d draws (mcx_samples_draw: gather on the device, %.0f MB of rows and indices to the host): %s ms (HIP events), "
                 "%s ms (wall)" % (a.ndraw, a.ndraw * (4.0 * (d + 1) + 8) / 1e6, " ".join("%.2f" % v for v in gpu),
                                   " ".join("%.2f" % v for v in wall)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
