#!/usr/bin/env python3
"""Cost of reading sample text back on the GPU, on the text of the first --steps steps of the C3 store
(65 536 chains x 16-D, 500 + 1000; all 1000 steps are 11.5 GB of text, more than this tool holds on the host at once): one
warm call, then --reps timed ones of mcx_debug_text_times -- the upload and the mark, scan, scatter and parse sweeps with
HIP events summed over the pieces, the host's line count and staging and the whole call by the wall clock -- and of
mcx_file_store on the same text in a file; next to them mcx_samples_text for the same rows (the whole call, wall clock), the
column-sum sweep k_sum_moments over the same rows (the unit of the other sections) and numpy.loadtxt on a slice, scaled up.
The model: the text is read twice from HBM and crosses PCIe once, 4 bytes are written per number.

  python tools/parse_bench.py [--out profiles/parse_c3.txt] [--reps 3] [--steps 100] [--piece-bytes 0]"""
import argparse
import io
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import mcpar_amd as M  # noqa: E402
from mcpar_amd import engine as E  # noqa: E402

STAGES = ("upload (HIP events)", "k_mark (HIP events)", "k_text_scan (HIP events)", "k_scatter (HIP events)", "k_parse (HIP events)",
          "host: line count (wall)", "host: staging of the pieces (wall)", "whole call (wall)")
HBM, PCIE = 6.29e12, 63e9  # measured float4 copy; PCIe Gen5 x16 by the data sheet


def device_line():
    name, cu, mem = M.device_info()
    name = name.strip()
    if name.startswith("("):
        name = name.strip("()") + " (the runtime reports no device name)"
    return "device: %s, %d CUs, %.0f GB" % (name, cu, mem / 1e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parse_c3.txt"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--piece-bytes", type=int, default=0)
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
    S = min(a.steps, nsamp)
    eg.samples_text(0, 1)  # warm
    t0 = time.perf_counter()
    text = eg.samples_text(0, S)
    t_text = (time.perf_counter() - t0) * 1e3
    N = S * n
    ntok = N * (d + 1)
    lines = ["text of the first %d steps of the C3 store: %d chains x %d-D, %d rows, %d numbers, %.3f GB of text (%.2f bytes a number)"
             % (S, n, d, N, ntok, len(text) / 1e9, len(text) / ntok), device_line()]
    lines.append("mcx_samples_text of the same rows, whole call (wall): %.1f ms" % t_text)
    eg.covariance_times(0, S)  # warm
    mom = [eg.covariance_times(0, S)[0] for _ in range(a.reps)]
    lines.append("column-sum sweep (k_sum_moments) over the same rows, the yardstick: %s ms; best %.3f ms"
                 % (" ".join("%.3f" % v for v in mom), min(mom)))
    E.debug_text_times(text[:text.index(b"\n", 1 << 20) + 1], 1, d + 1)  # warm
    t = []
    for _ in range(a.reps):
        ms, rep = E.debug_text_times(text, n, d + 1, a.piece_bytes)
        assert rep["nrows"] == N and rep["nfallback"] == 0
        t.append(ms)
    t = np.array(t)
    lines.append("mcx_text_store, %d pieces (piece_bytes %s), %d runs; per stage: the runs, then the best per piece" %
                 (rep["npieces"], a.piece_bytes or "default", a.reps))
    for k, name in enumerate(STAGES):
        lines.append("  %-36s %s ms; best %.3f ms, %.3f ms a piece" % (name, " ".join("%.3f" % v for v in t[:, k]), t[:, k].min(),
                                                                         t[:, k].min() / rep["npieces"]))
    dev = t[:, 1:5].sum(axis=1).min()
    model_dev = (2.0 * len(text) + 4.0 * ntok) / HBM * 1e3
    model_pcie = len(text) / PCIE * 1e3
    lines.append("the four sweeps together: best %.3f ms = %.1f GB/s of text, %.2f x the column-sum sweep; the model (text read twice, "
                 "4 B written a number, at %.2f TB/s): %.3f ms, ratio %.1f" % (dev, len(text) / dev / 1e6, dev / min(mom), HBM / 1e12,
                                                                               model_dev, dev / model_dev))
    lines.append("the upload: best %.3f ms = %.1f GB/s; the model (once over PCIe at %.0f GB/s): %.3f ms, ratio %.2f"
                 % (t[:, 0].min(), len(text) / t[:, 0].min() / 1e6, PCIE / 1e9, model_pcie, t[:, 0].min() / model_pcie))
    lines.append("the whole call: best %.1f ms = %.2f GB/s of text" % (t[:, 7].min(), len(text) / t[:, 7].min() / 1e6))
    with tempfile.NamedTemporaryFile(suffix=".txt") as f:
        f.write(text)
        f.flush()
        tf = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            store, rep = E.store_from_file(f.name, n, d + 1, piece_bytes=a.piece_bytes)
            tf.append((time.perf_counter() - t0) * 1e3)
            store.close()
    lines.append("mcx_file_store of the same text in a file (page cache), whole call (wall): %s ms" % " ".join("%.1f" % v for v in tf))
    k = 2000
    sl = text[:text.index(b"\n", len(text) * k // N) + 1]
    nl = sl.count(b"\n")
    t0 = time.perf_counter()
    ref = np.loadtxt(io.BytesIO(sl), dtype=np.float32)
    t_np = time.perf_counter() - t0
    assert ref.shape == (nl, d + 1)
    lines.append("numpy.loadtxt on the first %d rows: %.1f ms; scaled to %d rows: %.1f s" % (nl, t_np * 1e3, N, t_np * N / nl))
    out = "\n".join(lines) + "\n"
    print(out, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(out)


if __name__ == "__main__":
    main()
