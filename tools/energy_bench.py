#!/usr/bin/env python3
"""Cost of the joint comparison of two stores on the C3 run (65 536 chains x 16-D, 500 + 1000): the first
against the second 500 kept steps, n_a = n_b = 2048 and 8192 draws with 999 permutations; one warm call, then --reps timed,
every stage from mcx_debug_energy_times.  k_energy_pairs is held against the flop it executes -- N^2 pairs times the label
columns padded to blocks of 16, two flop each; the full matrix, the symmetry is not used -- and that rate against two
yardsticks: section 10's k_cov_tiles in the same process (the same instruction) and the part's nominal fp64 matrix rate.  The
same computation in numpy on the copied rows at n = 2048 is timed beside it.

  python tools/energy_bench.py [--out profiles/energy_c3.txt] [--reps 3] [--np 16] [--nc 65536]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import mcpar_amd as M  # noqa: E402
from mcpar_amd import engine as E  # noqa: E402

STAGES = ("gather of both sides", "scale, flags and z (host)", "label vectors (host)", "uploads", "k_energy_pairs", "k_energy_reduce",
          "whole call (host clock)")
NOMINAL = 78.6e12  # fp64 matrix flop/s of the MI355X as published


def device_line():
    name, cu, mem = M.device_info()
    name = name.strip()
    if name.startswith("("):
        name = name.strip("()") + " (the runtime reports no device name)"
    return "device: %s, %d CUs, %.0f GB" % (name, cu, mem / 1e9)


def numpy_energy(a, b, nperm, seed):
    """energy_rows(n_a = n_b = -1) of rows a, b in numpy: the distances, then one matrix product per sum"""
    na, nb = len(a), len(b)
    x = np.concatenate([a, b])[:, :-1].astype(np.float64)
    z = x / x.std(axis=0, ddof=1)
    L = np.stack([E.debug_energy_labels(seed, na, nb, p) for p in range(nperm + 1)]).astype(np.float64)
    t0 = time.perf_counter()
    d = np.zeros((len(z), len(z)))
    for c in range(z.shape[1]):
        t = z[:, None, c] - z[None, :, c]
        d += t * t
    np.sqrt(d, out=d)
    G = L @ d
    S, SA, SAA = d.sum(), G.sum(axis=1), np.einsum("pi,pi->p", G, L)
    e = 2.0 * (SA - SAA) / (na * nb) - SAA / (na * na) - (S - 2.0 * SA + SAA) / (nb * nb)
    return time.perf_counter() - t0, e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "energy_c3.txt"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--np", type=int, default=16)
    ap.add_argument("--nc", type=int, default=65536)
    ap.add_argument("--sizes", default="2048,8192")
    a = ap.parse_args()
    d, n, nburn, nsamp, nperm = a.np, a.nc, 500, 1000, 999
    half = nsamp // 2
    M.load().mcx_set_device(0)
    vl, keep = M.make_vlfunc(M.VL_ROSENBROCK1, d)
    eg = M.Engine(d, n, pl=1.0)
    g = np.arange(n, dtype=np.float64)[:, None]
    i = np.arange(d, dtype=np.float64)[None, :]
    eg.run(nsamp, nburn, (0.5 * np.sin(0.37 * (g * d + i))).astype(np.float32), vl)
    eg.synchronize()
    lines = ["energy of the C3 store's halves: %d chains x %d-D, %d + %d, steps [0, %d) against [%d, %d), %d permutations, %d columns used"
             % (n, d, nburn, nsamp, half, half, nsamp, nperm, d), device_line()]
    eg.covariance_times()  # warm
    cv = np.array([eg.covariance_times() for _ in range(a.reps)])
    ntile = (d + 15) // 16
    cov_flop = 2.0 * nsamp * n * 256 * (ntile * (ntile + 1) // 2)
    cov_rate = cov_flop / (cv[:, 1].min() * 1e-3)
    lines.append("section 10's k_cov_tiles on the whole store, the first yardstick: %s ms; best %.3f ms = %.1f Tflop/s as executed"
                 % (" ".join("%.3f" % v for v in cv[:, 1]), cv[:, 1].min(), cov_rate / 1e12))
    lines.append("the part's nominal fp64 matrix rate, the second: %.1f Tflop/s" % (NOMINAL / 1e12))
    for side in [int(s) for s in a.sizes.split(",")]:
        kw = dict(n_a=side, n_b=side, nperm=nperm, seed=1)
        geo = E.debug_energy_geometry(side, side, d, nperm)
        N = 2 * side
        flop = 2.0 * (geo["tiles"] * geo["tile_rows"]) * (-(-N // 64) * 64) * (geo["label_blocks"] * 16)
        lines.append("n_a = n_b = %d: N = %d pooled rows, %d tiles x %d slabs x %d chunks = %d workgroups, %d label columns in %d blocks, "
                     "%.1f MB of scratch, %.3g flop as executed (N^2 (1 + P) 2 = %.3g)"
                     % (side, N, geo["tiles"], geo["slabs"], geo["chunks"], geo["workgroups"], geo["label_cols"], geo["label_blocks"],
                        geo["scratch_bytes"] / 1e6, flop, 2.0 * N * N * (1 + nperm)))
        eg.energy_times(0, half, half, half, **kw)  # warm
        t = np.array([eg.energy_times(0, half, half, half, **kw) for _ in range(a.reps)])
        for k, name in enumerate(STAGES):
            lines.append("  %-28s %s ms; best %.3f ms" % (name + ":", " ".join("%.3f" % v for v in t[:, k]), t[:, k].min()))
        rate = flop / (t[:, 4].min() * 1e-3)
        lines.append("  k_energy_pairs: %.1f Tflop/s as executed = %.2f x k_cov_tiles' rate = %.2f of the nominal rate"
                     % (rate / 1e12, rate / cov_rate, rate / NOMINAL))
        r = eg.energy(0, half, half, half, **kw)
        lines.append("  what it says of the run's halves: e %.6g h %.4g p_value %.4g (nge %d of %d), largest perm_e %.6g"
                     % (r["e"], r["h"], r["p_value"], r["nge"], nperm, r["perm_e"].max()))
        if side <= 2048:
            ra = eg.samples_range(0, half)[E.debug_draw_indices(1, half * n, 0, side)]
            rb = eg.samples_range(half, half)[E.debug_draw_indices(1, half * n, side, side)]
            sec, e = numpy_energy(ra, rb, nperm, 1)
            lines.append("  the same in numpy on the copied rows (distances, then L @ d): %.2f s; e %.6g, largest |perm_e - numpy's| %.3g"
                         % (sec, e[0], np.abs(r["perm_e"] - e[1:]).max()))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
