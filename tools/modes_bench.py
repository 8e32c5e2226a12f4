#!/usr/bin/env python3
"""Cost of the modes of a store on the C3 run (65 536 chains x 16-D, 500 + 1000): one warm call, then
--reps timed, every stage with HIP events (mcx_debug_modes_times).  One assign pass (max_iter = 1) at K = 2, 8, 32 with given
centres, against mcx_samples_covariance's column-sum sweep k_sum_moments over the same range in the same process
(mcx_debug_covariance_times), the yardstick: one read of the store.  The table pass, a whole call at K = 8 with the seeding,
the chain and step sweeps, the rows of a mode, and numpy on copied rows of a sub-range (scaled, and marked as scaled).

The model, stated before the measurement: a pass reads the store once (the yardstick's time) and issues 3 K p fp64 vector
operations a row without fused multiply-add; it should take max(bytes / yardstick rate, 3 K p N / fp64 vector rate).  The fp64
vector rate is what tools/ubench (built from tools/ubench.hip) measures for its dist_f64 group at 8 wavefronts per SIMD when the
binary is there; else the model's second term is not computed and the line says so.

  python tools/modes_bench.py [--out profiles/modes_c3.txt] [--reps 3] [--np 16] [--nc 65536] [--nsamp 1000]"""
import argparse
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import mcpar_amd as M  # noqa: E402
from mcpar_amd import engine as E  # noqa: E402

STAGES = ("scale (summary passes)", "seed sample and seeding", "assign passes", "their reducers", "table pass and reducer")


def device_line():
    name, cu, mem = M.device_info()
    name = name.strip()
    if name.startswith("("):
        name = name.strip("()") + " (the runtime reports no device name)"
    return "device: %s, %d CUs, %.0f GB" % (name, cu, mem / 1e9), cu


def fp64_rate(cus):
    """(lane operations per second of the dist_f64 group at 8 wavefronts per SIMD, the line of the microbenchmark) or (None, why)"""
    exe = os.path.join(ROOT, "tools", "ubench")
    if not os.path.exists(exe):
        return None, "tools/ubench is not built (hipcc --offload-arch=gfx950 -O2 -o tools/ubench tools/ubench.hip)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        return None, "tools/ubench failed: " + (r.stdout + r.stderr).strip()[-200:]
    block = r.stdout.split("== 8 wave(s) per SIMD")[-1]
    m = re.search(r"dist_f64\s+([0-9.]+) ns/wave-instr/SIMD", block)
    if not m:
        return None, "tools/ubench printed no dist_f64 line"
    ns = float(m.group(1))
    return 64.0 * 4 * cus / (ns * 1e-9), "tools/ubench, 8 wavefronts per SIMD: dist_f64 %.3f ns per wave-instruction per SIMD" % ns


def numpy_pass(rows, c, s):
    u = rows[:, :-1].astype(np.float64) * s
    d = np.stack([((u - ck) ** 2).sum(1) for ck in c], 1)
    lab = d.argmin(1)
    return np.stack([u[lab == k].sum(0) for k in range(len(c))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modes_c3.txt"))
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
    dev, cus = device_line()
    lines = ["modes of the C3 store: %d chains x %d-D, %d + %d: N = %d rows of %d columns, %.2f GB" % (n, d, nburn, nsamp, N, ncol, store_bytes / 1e9),
             dev]
    eg.covariance_times(0, nsamp)  # warm
    ys = np.array([eg.covariance_times(0, nsamp) for _ in range(a.reps)])
    yard = ys[:, 0].min()
    lines.append("k_sum_moments over the same range, the yardstick: %s ms; best %.3f ms = %.2f TB/s"
                 % (" ".join("%.3f" % v for v in ys[:, 0]), yard, store_bytes / yard / 1e9))
    rate, how = fp64_rate(cus)
    lines.append("fp64 vector rate: " + (how if rate is None else "%s = %.2f T lane operations/s on %d CUs" % (how, rate / 1e12, cus)))
    first = eg.samples_range(0, 1)[:, :d].astype(np.float64)
    for K in (2, 8, 32):
        geo = E.debug_modes_geometry(d, nsamp, n, K)
        centres = first[np.linspace(0, n - 1, K).astype(int)]
        eg.modes_times(K, centres=centres, max_iter=1, scale=False)  # warm
        t = np.array([eg.modes_times(K, centres=centres, max_iter=1, scale=False)[0] for _ in range(a.reps)])
        best = t[:, 2].min()
        ops = 3.0 * K * d * N
        model = "not computed" if rate is None else "max(%.3f, %.3f) = %.3f ms" % (yard, 1e3 * ops / rate, max(yard, 1e3 * ops / rate))
        lines.append("one assign pass, K = %d (%d workgroups of %d-row tiles, %d centre block(s), %.1f KB of LDS, %.1f MB of scratch):"
                     % (K, geo["workgroups"], geo["rows_per_tile"], geo["centre_blocks"], geo["assign_lds_bytes"] / 1e3, geo["scratch_bytes"] / 1e6))
        lines.append("  k_modes_assign %s ms; best %.3f ms = %.2f x the yardstick; model %s%s; reducer best %.3f ms; table pass best %.3f ms = "
                     "%.2f x the yardstick" % (" ".join("%.3f" % v for v in t[:, 2]), best, best / yard, model,
                                              "" if rate is None else ", measured / model %.2f" % (best / max(yard, 1e3 * ops / rate)),
                                              t[:, 3].min(), t[:, 4].min(), t[:, 4].min() / yard))
    K = 8
    eg.modes_times(K, seed=1)  # warm
    runs = [eg.modes_times(K, seed=1) for _ in range(a.reps)]
    t, res = np.array([r[0] for r in runs]), runs[0][1]
    lines.append("Engine.modes(%d, seed=1), the whole call with the scale and the seeding: %d passes, flags %d" % (K, res["iters"], res["flags"]))
    for k, name in enumerate(STAGES):
        lines.append("  %-26s %s ms; best %.3f ms" % (name + ":", " ".join("%.3f" % v for v in t[:, k]), t[:, k].min()))
    lines.append("  %-26s %s ms; best %.3f ms" % ("whole call (wall clock):", " ".join("%.3f" % v for v in t[:, 7]), t[:, 7].min()))
    m = eg.modes(K, seed=1)
    tt = []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        ct = m.chain_table()
        tt.append(1e3 * (time.perf_counter() - t0))
    lines.append("Modes.chain_table() (k_modes_chains, k_modes_steps and the copies, wall clock): %s ms; best %.3f ms"
                 % (" ".join("%.3f" % v for v in tt[1:]), min(tt[1:])))
    big = int(np.argmax(m.table["n"]))
    tt = []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        rs = m.rows(big)
        tt.append(1e3 * (time.perf_counter() - t0))
        kept = rs.nrows
        rs.close()
    lines.append("Modes.rows(%d) (k_modes_mark, scan, scatter of %d rows, wall clock): %s ms; best %.3f ms"
                 % (big, kept, " ".join("%.3f" % v for v in tt[1:]), min(tt[1:])))
    lines.append("  what it says of the run: n %s; hops in all %d over %d chains; weights %s"
                 % (m.table["n"].tolist(), int(ct["hops"].sum()), n, " ".join("%.4f" % w for w in m.table["weight"])))
    # numpy on copied rows, a 1/64 sub-range
    sub = max(nsamp // 64, 4)
    t0 = time.perf_counter()
    rows = eg.samples_range(0, sub)
    t1 = time.perf_counter()
    numpy_pass(rows, m.centres_scaled, m.scale)
    t2 = time.perf_counter()
    lines.append("numpy, float64, one pass at K = %d on the copied rows of the first %d steps (1/%d of the range): copy %.1f ms, pass %.1f ms; "
                 "SCALED by %d to the whole range: copy %.0f ms, pass %.0f ms"
                 % (K, sub, nsamp // sub, 1e3 * (t1 - t0), 1e3 * (t2 - t1), nsamp // sub, 1e3 * (t1 - t0) * (nsamp // sub),
                    1e3 * (t2 - t1) * (nsamp // sub)))
    m.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
