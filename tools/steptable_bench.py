#!/usr/bin/env python3
"""Cost of the step table on the C3 store (65 536 chains x 16-D, 500 + 1000): one warm call, then three timed -- the moments
sweep, the select sweep and the row sweep with HIP events and the whole call by the wall clock (mcx_debug_step_table_times) --
against the column-sum sweep k_sum_moments of the same process (mcx_debug_covariance_times), which reads the same rows once.
The bytes a sweep must read: the moments sweep the rows twice (the sum, then the centred sums and the extremes), the select
sweep four times (one radix digit each), the row sweep twice (step t and step t - 1).  Then the host route on a short range:
copy the rows, numpy's mean, std, min, max and quantiles per step, and the row comparison.  Last, the settle rule on the
table (host, wall clock) and what it says of the C3 run.

  python tools/steptable_bench.py [--out profiles/steptable_c3.txt] [--reps 3] [--np 16] [--nc 65536] [--host-steps 20]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import mcpar_amd as M  # noqa: E402
from mcpar_amd import engine as E  # noqa: E402

PROBS = (0.05, 0.5, 0.95)
STAGES = (("k_step_moments (HIP events)", 2.0), ("k_step_select (HIP events)", 4.0), ("k_step_rows + reduce (HIP events)", 2.0),
          ("whole call (wall)", 0.0))


def device_line():
    """name (architecture), CUs, memory -- the runtime of some boxes reports an empty name: the architecture string then"""
    name, cu, mem = M.device_info()
    name = name.strip()
    if name.startswith("("):
        name = name.strip("()") + " (the runtime reports no device name)"
    return "device: %s, %d CUs, %.0f GB" % (name, cu, mem / 1e9)


def host_route(eg, first, nsteps, n, d):
    """what the table costs today: the rows to the host, then numpy per step"""
    t0 = time.perf_counter()
    a = eg.samples_range(first, nsteps).reshape(nsteps, n, d + 1)
    t1 = time.perf_counter()
    x = a.astype(np.float64)
    out = dict(mean=x.mean(axis=1), sd=x.std(axis=1, ddof=1), min=a.min(axis=1), max=a.max(axis=1),
               q=np.quantile(x, PROBS, axis=1), moved=(a.view(np.uint32)[1:] != a.view(np.uint32)[:-1]).any(axis=2).sum(axis=1),
               ll=a[:, :, d].argmax(axis=1))
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "steptable_c3.txt"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--np", type=int, default=16)
    ap.add_argument("--nc", type=int, default=65536)
    ap.add_argument("--host-steps", type=int, default=20)
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
    geo = E.debug_steptable_geometry(d, nsamp, n, len(PROBS))
    lines = ["step table of the C3 store: %d chains x %d-D, %d + %d, N = %d rows, %.2f GB of rows, %.2f MB a step; probs %s"
             % (n, d, nburn, nsamp, N, rbytes / 1e9, rbytes / nsamp / 1e6, " ".join("%g" % p for p in PROBS)),
             device_line(),
             "geometry: moments %d workgroups of tiles of %d columns, %d B of LDS; select %d workgroups of tiles of %d columns x %d "
             "slots, %d B of LDS (%d workgroups to a CU's 160 KiB); rows %d workgroups, %d lanes a chain, %d chunks a step"
             % (geo["moments_workgroups"], geo["moments_tile_cols"], geo["moments_lds_bytes"], geo["select_workgroups"],
                geo["select_tile_cols"], geo["select_slots"], geo["select_lds_bytes"], 163840 // max(geo["select_lds_bytes"], 1),
                geo["rows_workgroups"], geo["rows_lanes_per_chain"], geo["rows_chunks"])]
    eg.covariance_times()  # warm
    mom = [eg.covariance_times()[0] for _ in range(a.reps)]
    yard = min(mom)
    lines.append("column-sum sweep (k_sum_moments), the yardstick: %s ms; best %.3f ms = %.2f TB/s read"
                 % (" ".join("%.3f" % v for v in mom), yard, rbytes / yard / 1e9))
    eg.step_table_times(probs=PROBS)  # warm
    t = np.array([eg.step_table_times(probs=PROBS) for _ in range(a.reps)])
    lines.append("Engine.step_table() of the run's store, %d steps:" % nsamp)
    for k, (name, reads) in enumerate(STAGES):
        best = t[:, k].min()
        tail = " = %.2f TB/s of the rows, which it must read once (it loads them %g times: %.2f TB/s of loads), %.2f x the yardstick" \
            % (rbytes / best / 1e9, reads, reads * rbytes / best / 1e9, best / yard) if reads else ", %.2f x the yardstick" % (best / yard)
        lines.append("  %-36s %s ms; best %.3f ms%s" % (name + ":", " ".join("%.3f" % v for v in t[:, k]), best, tail))
    t0 = np.array([eg.step_table_times(probs=()) for _ in range(a.reps)])
    lines.append("  without quantiles (nprobs = 0, no select launch), whole call (wall): %s ms" % " ".join("%.3f" % v for v in t0[:, 3]))
    # the host route on a short range, and the device on the same range
    hs = min(a.host_steps, nsamp)
    first = nsamp - hs
    cp, npy, host = host_route(eg, first, hs, n, d)
    eg.step_table_times(first, hs, PROBS)  # warm
    dev = min(eg.step_table_times(first, hs, PROBS)[3] for _ in range(a.reps))
    tab = eg.step_table(first, hs, PROBS)
    agree = np.allclose(tab["mean"], host["mean"], rtol=1e-9, atol=1e-12) and np.allclose(tab["sd"], host["sd"], rtol=1e-9) and \
        np.allclose(tab["quantiles"], np.moveaxis(host["q"], 0, 2), rtol=1e-9, atol=1e-12) and \
        np.array_equal(tab["moved"][1:], host["moved"]) and np.array_equal(tab["min"], host["min"]) and np.array_equal(tab["max"], host["max"])
    lines.append("host route on the last %d steps (%.1f MB of rows): copy %.1f ms + numpy %.1f ms = %.1f ms; the device's whole call on "
                 "the same range %.3f ms (%.0f x); the two tables agree: %s"
                 % (hs, 4.0 * hs * n * (d + 1) / 1e6, cp, npy, cp + npy, dev, (cp + npy) / dev, "yes" if agree else "NO"))
    lines.append("  the host route scaled to %d steps: %.1f s (not run)" % (nsamp, (cp + npy) * nsamp / hs / 1e3))
    # the rule, and what the table says of the run
    table = eg.step_table(probs=PROBS)
    tk = []
    for _ in range(a.reps):
        t1 = time.perf_counter()
        settled, cols = E.settle_steps(table)
        tk.append((time.perf_counter() - t1) * 1e3)
    lines.append("settle_steps(tol 0.1, 0.1, ref 0.5), host: %s ms; %s" % (" ".join("%.3f" % v for v in tk),
                 "settled at step %d of %d" % (settled, nsamp) if settled >= 0 else "not settled"))
    lines.append("  last step out of band per column: %s" % " ".join("%d" % v for v in cols["last_out"]))
    lines.append("  largest |mean_t - m_ref| / s_ref per column: %s" % " ".join("%.3f" % v for v in cols["max_dev_mean"]))
    lines.append("  largest |sd_t - s_ref| / s_ref per column:   %s" % " ".join("%.3f" % v for v in cols["max_dev_sd"]))
    mv = table["moved"][1:]
    lines.append("  moved per step (of %d chains): min %d, median %d, max %d; first 5 steps %s; last 5 steps %s"
                 % (n, mv.min(), int(np.median(mv)), mv.max(), " ".join("%d" % v for v in mv[:5]), " ".join("%d" % v for v in mv[-5:])))
    lines.append("  log L: step mean %.4g at step 0, %.4g at step %d; largest log L of the run %.6g at step %d, chain %d"
                 % (table["mean"][0, d], table["mean"][-1, d], nsamp - 1, table["ll_max"].max(), int(table["ll_max"].argmax()),
                    int(table["ll_max_chain"][table["ll_max"].argmax()])))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
