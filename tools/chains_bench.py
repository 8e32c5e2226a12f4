#!/usr/bin/env python3
"""Cost of the chain table and of a store of chosen chains on the C3 store (65 536 chains x 16-D, 500 + 1000): one warm call,
then three timed -- the series sweep and the row sweep with HIP events and the whole table call by the wall clock
(mcx_debug_chain_table_times), the host rule (keep_chains, wall clock) and the selection of the chains it keeps (the whole
Engine.select_chains call by the wall clock: allocation, the gather sweep, the synchronise) -- against the column-sum sweep
k_sum_moments of the same process (mcx_debug_covariance_times), which reads the same rows once.  The bytes: the series sweep
reads the rows twice (the sum, then the centred sums), the row sweep once; the gather reads and writes the kept rows.

  python tools/chains_bench.py [--out profiles/chains_c3.txt] [--reps 3] [--np 16] [--nc 65536]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import mcpar_amd as M  # noqa: E402
from mcpar_amd import engine as E  # noqa: E402

STAGES = ("k_chain_series (HIP events)", "k_chain_rows (HIP events)", "whole call (wall)")


def device_line():
    """name (architecture), CUs, memory -- the runtime of some boxes reports an empty name: the architecture string then"""
    name, cu, mem = M.device_info()
    name = name.strip()
    if name.startswith("("):
        name = name.strip("()") + " (the runtime reports no device name)"
    return "device: %s, %d CUs, %.0f GB" % (name, cu, mem / 1e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chains_c3.txt"))
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
    lines = ["chain table of the C3 store: %d chains x %d-D, %d + %d, N = %d rows, %.2f GB of rows" % (n, d, nburn, nsamp, N, rbytes / 1e9),
             device_line()]
    eg.covariance_times()  # warm
    mom = [eg.covariance_times()[0] for _ in range(a.reps)]
    yard = min(mom)
    lines.append("column-sum sweep (k_sum_moments), the yardstick: %s ms; best %.3f ms = %.2f TB/s read"
                 % (" ".join("%.3f" % v for v in mom), yard, rbytes / yard / 1e9))
    eg.chain_table_times()  # warm
    t = np.array([eg.chain_table_times() for _ in range(a.reps)])
    lines.append("Engine.chain_table() of the run's store:")
    for k, name in enumerate(STAGES):
        lines.append("  %-30s %s ms; best %.3f ms" % (name + ":", " ".join("%.3f" % v for v in t[:, k]), t[:, k].min()))
    ser, row, whole = t[:, 0].min(), t[:, 1].min(), t[:, 2].min()
    lines.append("  series: %.2f TB/s over two reads, %.2f x the yardstick; rows: %.2f TB/s read, %.2f x the yardstick; whole call %.2f x"
                 % (2.0 * rbytes / ser / 1e9, ser / yard, rbytes / row / 1e9, row / yard, whole / yard))
    table = eg.chain_table()
    tk = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        reasons, centre, kept = E.keep_chains(table, z=5.0, min_moves=1)
        tk.append((time.perf_counter() - t0) * 1e3)
    lines.append("keep_chains(z = 5, min_moves = 1), host: %s ms; kept %d of %d chains (non-finite %d, stuck %d, outlier %d)"
                 % (" ".join("%.3f" % v for v in tk), kept.size, n, int((reasons & 1 != 0).sum()), int((reasons & 2 != 0).sum()),
                    int((reasons & 4 != 0).sum())))
    lines.append("  moves per chain over %d steps: min %d, median %d, max %d; longest stay: median %d, max %d"
                 % (nsamp, table["moves"].min(), int(np.median(table["moves"])), table["moves"].max(),
                    int(np.median(table["longest_stay"])), table["longest_stay"].max()))
    eg.select_chains(kept).close()  # warm
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        st = eg.select_chains(kept)
        ts.append((time.perf_counter() - t0) * 1e3)
        st.close()
    sel = min(ts)
    sbytes = 2.0 * 4.0 * nsamp * kept.size * (d + 1)
    lines.append("Engine.select_chains(kept), whole call (wall): %s ms; best %.3f ms = %.2f TB/s read and written, %.2f x the yardstick"
                 % (" ".join("%.3f" % v for v in ts), sel, sbytes / sel / 1e9, sel / yard))
    s_all, st = eg.summary(), eg.select_chains(kept)
    s_kept = st.summary()
    st.close()
    lines.append("split R-hat, all chains:  %s" % " ".join("%.3f" % v for v in s_all["rhat"]))
    lines.append("split R-hat, kept chains: %s" % " ".join("%.3f" % v for v in s_kept["rhat"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
