#!/usr/bin/env python3
"""Cost of the mutual information between columns on the C3 run (65 536 chains x 16-D, 500 + 1000): all 136
pairs of the 17 columns (log L included), n = 4096 and 16 384 rows, 0 and 99 permutations; one warm call, then --reps timed, every
stage from mcx_debug_mutinfo_times.  k_mi_pairs is held against its own model -- 2 m^2 pairs (1 + nperm) visits (two sweeps) times
the FP64_PER_VISIT fp64 vector instructions a visit issues in the disassembly, at the fp64 vector rate tools/ubench.hip prices
(its dist_f64 group at 8 wavefronts per SIMD, profiles/modes_c3.txt) --, against k_energy_pairs per visit in the same process, and
against numpy on the same rows.

  python tools/mutinfo_bench.py [--out profiles/mutinfo_c3.txt] [--reps 3] [--np 16] [--nc 65536]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import mcpar_amd as M  # noqa: E402
from mcpar_amd import engine as E  # noqa: E402

STAGES = ("gather", "scale, flags, repeats and z (host)", "permutations and table (host)", "uploads", "k_mi_pairs", "k_mi_reduce and its copy",
          "pearson and the null (host)", "whole call (host clock)")
FP64_PER_VISIT = 4       # sweep 1: two v_add_f64, v_max_f64, v_cmp_lt_f64; sweep 2: two v_add_f64, two v_cmp_lt_f64 (+ two v_addc_co_u32)
FP64_LANE_RATE = 37.17e12  # lane operations/s of the dist_f64 group of tools/ubench.hip at 8 wavefronts per SIMD (section 25)


def device_line():
    name, cu, mem = M.device_info()
    name = name.strip()
    if name.startswith("("):
        name = name.strip("()") + " (the runtime reports no device name)"
    return "device: %s, %d CUs, %.0f GB" % (name, cu, mem / 1e9)


def numpy_pair(u, v, k):
    """one (pair, permutation) in numpy: both distance matrices, the k-th smallest, the counts, the digamma sum"""
    t0 = time.perf_counter()
    m = len(u)
    da, db = np.abs(u[:, None] - u[None, :]), np.abs(v[:, None] - v[None, :])
    ii = np.arange(m)
    da[ii, ii] = db[ii, ii] = np.inf
    eps = np.partition(np.maximum(da, db), k - 1, axis=1)[:, k - 1]
    na, nb = (da < eps[:, None]).sum(axis=1), (db < eps[:, None]).sum(axis=1)
    t = E.debug_mutinfo_psi(m)
    mi = (t[k - 1] + t[m - 1]) - (t[na] + t[nb]).sum() / m
    return time.perf_counter() - t0, mi


def selected_rows(eg, nsamp, nc, n):
    """the n rows floor(i N / n) of the store, copied step range by step range"""
    idx = E.debug_mutinfo_rows(nsamp * nc, n)
    out = np.zeros((n, eg.np + 1), np.float32)
    for s0 in range(0, nsamp, 50):
        sel = np.flatnonzero((idx >= s0 * nc) & (idx < (s0 + 50) * nc))
        if len(sel):
            out[sel] = eg.samples_range(s0, min(50, nsamp - s0))[idx[sel] - s0 * nc]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mutinfo_c3.txt"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--np", type=int, default=16)
    ap.add_argument("--nc", type=int, default=65536)
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--perms", default="0,99")
    a = ap.parse_args()
    d, nc, nburn, nsamp, k = a.np, a.nc, 500, 1000, 3
    M.load().mcx_set_device(0)
    vl, keep = M.make_vlfunc(M.VL_ROSENBROCK1, d)
    eg = M.Engine(d, nc, pl=1.0)
    g = np.arange(nc, dtype=np.float64)[:, None]
    i = np.arange(d, dtype=np.float64)[None, :]
    eg.run(nsamp, nburn, (0.5 * np.sin(0.37 * (g * d + i))).astype(np.float32), vl)
    eg.synchronize()
    npairs = (d + 1) * d // 2
    lines = ["mutual information of the C3 store's columns: %d chains x %d-D, %d + %d, %d columns with log L, %d pairs, k = %d"
             % (nc, d, nburn, nsamp, d + 1, npairs, k), device_line(),
             "the model: 2 m^2 pairs (1 + nperm) visits x %d fp64 vector instructions a visit / %.2f T lane operations/s" % (FP64_PER_VISIT,
                                                                                                                           FP64_LANE_RATE / 1e12)]
    # k_energy_pairs per visit, in the same process: the halves of the store, 2048 draws a side, 999 permutations
    ekw = dict(n_a=2048, n_b=2048, nperm=999, seed=1)
    eg.energy_times(0, nsamp // 2, nsamp // 2, nsamp // 2, **ekw)
    et = min(eg.energy_times(0, nsamp // 2, nsamp // 2, nsamp // 2, **ekw)[4] for _ in range(a.reps))
    evisits = 4096.0 ** 2 * 1001
    lines.append("k_energy_pairs (section 21), N = 4096, 1001 label vectors: %.3f ms = %.4g ns per visit (a distance of %d columns times a label)"
                 % (et, et * 1e6 / evisits, d))
    for n in [int(s) for s in a.sizes.split(",")]:
        for nperm in [int(s) for s in a.perms.split(",")]:
            kw = dict(n=n, k=k, nperm=nperm, seed=1, with_ll=True)
            eg.mutual_info_times(**kw)  # warm
            t = np.array([eg.mutual_info_times(**kw) for _ in range(a.reps)])
            r = eg.mutual_info(**kw)
            m = r["m"]
            geo = E.debug_mutinfo_geometry(m, npairs, nperm, k)
            visits = 2.0 * m * m * npairs * (1 + nperm)
            model = visits * FP64_PER_VISIT / FP64_LANE_RATE * 1e3
            best = t[:, 4].min()
            lines.append("n = %d, nperm = %d: ndup %d, m = %d points, %d tiles x %d pairs x %d = %d workgroups, %d stages of %d, %.1f MB of scratch, "
                         "%.4g visits" % (n, nperm, r["ndup"], m, geo["tiles"], npairs, 1 + nperm, geo["workgroups"], geo["stages"], geo["stage_rows"],
                                          (geo["scratch_bytes"] + 8.0 * m * (d + 1)) / 1e6, visits))
            for s, name in enumerate(STAGES):
                lines.append("  %-38s %s ms; best %.3f ms" % (name + ":", " ".join("%.3f" % v for v in t[:, s]), t[:, s].min()))
            lines.append("  k_mi_pairs: %.4g ns per visit = %.2f x k_energy_pairs'; the model %.3f ms: measured / model = %.2f"
                         % (best * 1e6 / visits, best * 1e6 / visits / (et * 1e6 / evisits), model, best / model))
            mi = r["pairs"]["mi"]
            top = np.argsort(-mi)[:3]
            lines.append("  what it says: largest mi " + ", ".join("%s-%s %.3f (pearson %.3f)" % (
                "p%d" % r["pairs"]["a"][j], "LL" if r["pairs"]["b"][j] == d else "p%d" % r["pairs"]["b"][j], mi[j], r["pairs"]["pearson"][j])
                for j in top) + "; median %.3f" % np.median(mi) + ("; pairs with p_value = 1 / %d: %d" % (
                    1 + nperm, int((r["pairs"]["nge"] == 0).sum())) if nperm else ""))
            if n <= 4096 and nperm == 0:
                rows = selected_rows(eg, nsamp, nc, n)
                pts = E.debug_mutinfo_points(rows, n, 1, n=-1, with_ll=True)
                assert pts["m"] == m
                secs, worst = [], 0.0
                for j in (0, npairs - 1):
                    sec, v = numpy_pair(pts["z"][r["pairs"]["a"][j]], pts["z"][r["pairs"]["b"][j]], k)
                    secs.append(sec)
                    worst = max(worst, abs(v - mi[j]))
                per = float(np.mean(secs))
                lines.append("  the same in numpy on the copied rows: %.2f s a (pair, permutation) = %.0f s for the %d pairs = %.0f x the whole call; "
                             "largest |mi - numpy's| %.3g" % (per, per * npairs, npairs, per * npairs / (t[:, 7].min() * 1e-3), worst))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
