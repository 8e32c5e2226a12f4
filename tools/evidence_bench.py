#!/usr/bin/env python3
"""Cost of the evidence of a store on the C3 run (65 536 chains x 16-D, 500 + 1000): one warm call, then
--reps timed, every stage with HIP events (mcx_debug_evidence_times).  The proposal is fitted on the first half of the steps, so
the sweep k_ev_logg reads the second half: N1 = nsamp / 2 * nc rows.  The yardstick is mcx_samples_covariance's column-sum sweep
k_sum_moments over that same second half in the same process (mcx_debug_covariance_times): one read of the rows.  A second
proposal of K = 8 Gaussians (the modes of the first half, section 25) shows what a component costs.  A comparison: log g in
numpy on the copied rows of a sub-range (scaled, and marked as scaled).

The model, stated before the measurement: the sweep reads the N1 rows once and writes 8 B a row, so at np = 16 it should sit near
the yardstick; a bridge pass reads 8 (N1 + N2) B.  The sweep issues about K np (np + 1) fp64 vector operations a row (a subtraction
and a multiply-add per entry of the triangle), which at np = 16 is below the read.

  python tools/evidence_bench.py [--out profiles/evidence_c3.txt] [--reps 3] [--np 16] [--nc 65536] [--nsamp 1000]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import mcpar_amd as M  # noqa: E402
from mcpar_amd import engine as E  # noqa: E402

STAGES = ("fit (section 10)", "draws (k_ev_draw)", "likelihood of the draws", "sweep of the rows (k_ev_logg)", "sweep of the draws",
          "neff and ess_f2 (summary passes)", "bridge passes and reducers")


def device_line():
    name, cu, mem = M.device_info()
    name = name.strip()
    if name.startswith("("):
        name = name.strip("()") + " (the runtime reports no device name)"
    return "device: %s, %d CUs, %.0f GB" % (name, cu, mem / 1e9)


def numpy_logg(x, c, W, lc):
    t = []
    for k in range(len(lc)):
        z = (x.astype(np.float64) - c[k]) @ W[k].T
        t.append(lc[k] - 0.5 * (z * z).sum(1))
    t = np.stack(t)
    mx = t.max(0)
    return mx + np.log(np.exp(t - mx).sum(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evidence_c3.txt"))
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
    fit = nsamp // 2
    N1 = (nsamp - fit) * n
    row_bytes = 4.0 * N1 * d
    lines = ["evidence of the C3 store: %d chains x %d-D, %d + %d; fitted on the first %d steps, N1 = %d rows (%.2f GB of parameters), "
             "N2 = 2^20 draws" % (n, d, nburn, nsamp, fit, N1, row_bytes / 1e9), device_line()]
    eg.covariance_times(fit, nsamp - fit)  # warm
    ys = np.array([eg.covariance_times(fit, nsamp - fit) for _ in range(a.reps)])
    yard = ys[:, 0].min()
    lines.append("k_sum_moments over the same %d steps, the yardstick: %s ms; best %.3f ms = %.2f TB/s (it reads log L too)"
                 % (nsamp - fit, " ".join("%.3f" % v for v in ys[:, 0]), yard, 4.0 * N1 * (d + 1) / yard / 1e9))
    with eg.modes(8, first_step=0, nsteps=fit, seed=1, max_iter=10) as m:
        mixture = E.proposal_from_modes(m, nc=1024)  # (each mode's covariance from its rows in 1024 pseudo-chains)
    for name, prop in (("K = 1, fitted", None), ("K = 8, the modes of the first half", mixture)):
        K = 1 if prop is None else prop.k
        geo = E.debug_evidence_geometry(d, N1, 1 << 20, K)
        spec = dict(ndraw=1 << 20, seed=1, fit_steps=fit)
        try:
            eg.evidence_times(None, prop, **spec)  # warm
        except M.McxError as err:
            lines.append("Engine.evidence(), %s: refused: %s" % (name, err))
            continue
        runs = [eg.evidence_times(None, prop, **spec) for _ in range(a.reps)]
        t, res = np.array([r[0] for r in runs]), runs[0][1]
        sweep = t[:, 3].min()
        npass = res["iters"] + 4   # the statistics, the loop, two passes of the error, the by-products
        lines.append("Engine.evidence(), %s (%d workgroups of %d-row tiles, %d lanes a row, %.1f KB of LDS, %.1f MB of scratch): log_z %.6g, "
                     "se %.3g, neff %.4g, %d passes, flags %d"
                     % (name, geo["sweep_workgroups"], geo["tile_rows"], geo["slices"], geo["sweep_lds_bytes"] / 1e3, geo["scratch_bytes"] / 1e6,
                        res["log_z"], res["se"], res["neff"], res["iters"], res["flags"]))
        for k, stage in enumerate(STAGES):
            lines.append("  %-34s %s ms; best %.3f ms" % (stage + ":", " ".join("%.3f" % v for v in t[:, k]), t[:, k].min()))
        lines.append("  %-34s %s ms; best %.3f ms" % ("whole call (wall clock):", " ".join("%.3f" % v for v in t[:, 7]), t[:, 7].min()))
        lines.append("  the sweep = %.2f x the yardstick, %.2f TB/s of rows read and l written; one bridge pass with its reducer and copy "
                     "= %.3f ms (%d passes), its model 8 (N1 + N2) B at the yardstick's rate = %.3f ms"
                     % (sweep / yard, (row_bytes + 4.0 * N1 + 8.0 * N1) / sweep / 1e9, t[:, 6].min() / npass, npass,
                        8.0 * (N1 + (1 << 20)) / (4.0 * N1 * (d + 1) / yard)))
    # numpy on copied rows, a 1/125 sub-range of the rows the sweep reads
    sub = max((nsamp - fit) // 125, 1)
    cv = eg.covariance(0, fit)
    p = E.Proposal([1.0], cv["mean"][:d], cv["cov"][:d, :d])
    _, W, lc = E.evidence_proposal(p)
    t0 = time.perf_counter()
    rows = eg.samples_range(fit, sub)
    t1 = time.perf_counter()
    numpy_logg(rows[:, :d], p.centres, W, lc)
    t2 = time.perf_counter()
    k = (nsamp - fit) // sub
    lines.append("numpy, float64, log g at K = 1 on the copied rows of %d steps (1/%d of the rows): copy %.1f ms, log g %.1f ms; SCALED by %d "
                 "to the N1 rows: copy %.0f ms, log g %.0f ms" % (sub, k, 1e3 * (t1 - t0), 1e3 * (t2 - t1), k, 1e3 * (t1 - t0) * k, 1e3 * (t2 - t1) * k))
    eg.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
