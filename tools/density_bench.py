#!/usr/bin/env python3
"""Cost of a density call on the C3 store (65 536 chains x 16-D, 500 + 1000): one warm call, then three timed -- the binning
sweep k_density_bins with HIP events, the statistics passes, the host grid and finish and the whole call by the wall clock
(mcx_debug_density_times) -- against the column-sum sweep k_sum_moments of the same process (mcx_debug_covariance_times),
which reads the same rows once.  Then the same on a second store of the same shape whose first column is constant (a
derived store: d0 = 3, d1 .. d15 = the parameters), the contended case: every value of that column lands in one slot.

  python tools/density_bench.py [--out profiles/density_c3.txt] [--reps 3] [--np 16] [--nc 65536]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import mcpar_amd as M  # noqa: E402

STAGES = ("statistics passes (wall)", "k_density_bins (HIP events)", "host grid and finish (wall)", "whole call (wall)")


def device_line():
    """name (architecture), CUs, memory -- the runtime of some boxes reports an empty name: the architecture string then"""
    name, cu, mem = M.device_info()
    name = name.strip()
    if name.startswith("("):
        name = name.strip("()") + " (the runtime reports no device name)"
    return "device: %s, %d CUs, %.0f GB" % (name, cu, mem / 1e9)


def report(lines, what, times, reps, yardstick, rbytes):
    times()  # warm
    t = np.array([times() for _ in range(reps)])
    lines.append(what)
    for k, name in enumerate(STAGES):
        lines.append("  %-30s %s ms; best %.3f ms" % (name + ":", " ".join("%.3f" % v for v in t[:, k]), t[:, k].min()))
    best = t[:, 1].min()
    lines.append("  the sweep: %.2f TB/s read; %.2f x the yardstick" % (rbytes / best / 1e9, best / yardstick))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density_c3.txt"))
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
    lines = ["density of the C3 store: %d chains x %d-D, %d + %d, N = %d values per column, %.2f GB of rows, n = 512"
             % (n, d, nburn, nsamp, N, rbytes / 1e9),
             device_line()]
    eg.covariance_times()  # warm
    mom = [eg.covariance_times()[0] for _ in range(a.reps)]
    lines.append("column-sum sweep (k_sum_moments), the yardstick: %s ms; best %.3f ms = %.2f TB/s read"
                 % (" ".join("%.3f" % v for v in mom), min(mom), rbytes / min(mom) / 1e9))
    plain = report(lines, "Engine.density() of the run's store:", eg.density_times, a.reps, min(mom), rbytes)
    dens = eg.density()
    assert np.all(dens["nbinned"] == N) and np.all(dens["flags"] == 0)
    A = np.eye(d, dtype=np.float32)
    A[0, 0] = 0.0
    b = np.zeros(d, np.float32)
    b[0] = 3.0
    st = eg.derive(M.derive_linear(A, b))
    hot = report(lines, "DerivedStore.density() of the store whose first column is the constant 3 (one slot takes all its values):",
                 st.density_times, a.reps, min(mom), rbytes)
    dh = st.density()
    assert dh["nbinned"][0] == N and dh["sd"][0] == 0.0
    for k in ("x", "y"):  # the other columns are the run's
        assert dh[k][1:].tobytes() == dens[k][1:].tobytes(), k
    lines.append("the constant column costs the sweep %.3f ms (%.2f x)" % (hot - plain, hot / plain))
    st.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
