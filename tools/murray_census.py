#!/usr/bin/env python3
"""Census of the Murray step's results, for comparing two builds of libmcx.so (MCX_LIBMCX=<other build> selects one): one
line per record with the SHA-256 of every result array and every counter that is not a time.  Records: standalone
gen_remote over the shapes of tests/test_gpu_murray_cull.py (plus np = 65, the kernels past the register ones, and np =
12, not a power of two) x every MCX_OPT_CULL; whole jobs (16-D Rosenbrock x 8192, 32-D mixture x 4096) x every
MCX_OPT_CULL; the same likelihoods with MCX_OPT_MURRAY_OVERLAP 0 / 4 at sizes whose big passes are chunked; a two-shard
job through the exchange hook; three jobs in a row on one engine in auto mode (the give-up state carries over).
Every field is the same from run to run but one: remote_pairs_evaluated where a screen sorted its chains (boxes and one
direction always, the per-pair bound from 2048 chains) -- k_cull_scatter places the chains of one key bin in the order its
atomics happen to run, the groups of 128 and with them the masks differ, the results do not.  Two runs of ONE build differ there.
usage: murray_census.py > a.txt; MCX_LIBMCX=other/libmcx.so murray_census.py > b.txt; diff a.txt b.txt"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import mcpar_amd as M
from mcpar_amd import engine as E
from test_gpu_configs import mix_params
from test_gpu_multishard import run_sharded_gpu
from test_gpu_murray_cull import realistic_state

TIMES = ("exchange_wait_ns",)
SHAPES = [(16, 1500, 1), (32, 700, 2), (16, 129, 3), (32, 4096, 1), (16, 1501, 1), (16, 999, 3), (16, 65, 5), (32, 333, 4),
          (16, 8200, 2), (65, 130, 1), (12, 130, 2)]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def record(name, arrays, counters):
    print(name, " ".join("%s=%s" % (k, sha(v)) for k, v in arrays), " ".join("%s=%d" % (k, v) for k, v in counters.items() if k not in TIMES))


def job_arrays(e, samples=True):
    names = ("state", "loglike", "mean", "var", "musigall") + (("samples",) if samples else ())
    return [(k, getattr(e, k)) for k in names]


def pinit(d, n, g0=0):
    g = (g0 + np.arange(n, dtype=np.float64))[:, None]
    return (0.5 * np.sin(0.37 * (g * d + np.arange(d, dtype=np.float64)[None, :]))).astype(np.float32)


def vlfunc(cfg, d):
    if cfg == "rosen16":
        return M.make_vlfunc(M.VL_ROSENBROCK1, d)
    return M.make_vlfunc(M.VL_GAUSSMIX, d, mix_params(d, 8), 8)


def main():
    for d, n, nshards in SHAPES:
        rng = np.random.default_rng(d * 1000 + n)
        ms, _ = realistic_state(rng, n * nshards, d, n, stuck_every=7)
        own = slice((nshards - 1) * n, nshards * n)
        pv = (ms[own, :, 0] + np.sqrt(ms[own, :, 1]) * rng.standard_normal((n, d))).astype(np.float32)
        pv[::7] = ms[own][::7, :, 0]
        for mode in (-1, 0, 1, 2, 3):
            e = M.Engine(d, n, nshards=nshards, shard=nshards - 1)
            e.set_option(E.OPT_CULL, mode)
            r = e.gen_remote(41, pv, ms)
            record("gen_remote %dx%dx%d cull=%d npass=%d" % (d, n, nshards, mode, r[4]),
                   list(zip(("ptrial", "cfac", "mutrial", "sigtrial"), r[:4])), e.counters)
            e.close()
    for cfg, d, n in (("rosen16", 16, 8192), ("mix32", 32, 4096)):
        vl, _keep = vlfunc(cfg, d)
        for mode in (-1, 0, 1, 2, 3):
            e = M.Engine(d, n, pl=0.9)
            e.set_option(E.OPT_CULL, mode)
            e.run(60, 500, pinit(d, n), vl)
            record("job %s cull=%d" % (cfg, mode), job_arrays(e), e.counters)
            e.close()
    for cfg, d, n in (("rosen16", 16, 16384), ("mix32", 32, 8192)):
        vl, _keep = vlfunc(cfg, d)
        for chunks in (0, 4):
            e = M.Engine(d, n, pl=0.85)
            e.set_option(E.OPT_SAMPLES, 0)
            e.set_option(E.OPT_MURRAY_OVERLAP, chunks)
            e.run(40, 300, pinit(d, n), vl)
            record("job %s overlap=%d" % (cfg, chunks), job_arrays(e, samples=False), e.counters)
            e.close()
    for s, e in enumerate(run_sharded_gpu(16, 512, 2, 120, 40, 0.8)):
        record("two shards, shard %d" % s, job_arrays(e), e.counters)
        e.close()
    d, n = 32, 4096
    vl, _keep = vlfunc("mix32", d)
    e = M.Engine(d, n, pl=0.9)
    for k in range(3):
        e.run(60, 200, pinit(d, n), vl)
        record("auto mode, job %d in a row" % k, job_arrays(e), e.counters)
    e.close()


if __name__ == "__main__":
    main()
