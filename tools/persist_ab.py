#!/usr/bin/env python3
"""A/B of the one-launch small-n kernel on ONE box: builds of libmcx.so, given as paths, time the same jobs in turn
(A B A B ...), several rounds, each run in a process of its own (MCX_LIBMCX picks the library).  Prints the job time and the
kernel's own time (HIP events, MCX_OPT_PROFILE) per library, and for every library after the first whether its median job
time stays within the first one's median plus the spread (max - min) of the first one's own repeats.
usage: tools/persist_ab.py ROUNDS LIB_A LIB_B [LIB_C ...]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import sys, os, time, json
sys.path.insert(0, %r)
import numpy as np
import mcpar_amd as M
from mcpar_amd import engine as E
def pinit(d, n):
    g = np.arange(n, dtype=np.float64)[:, None]; i = np.arange(d, dtype=np.float64)[None, :]
    return (0.5 * np.sin(0.37 * (g * d + i))).astype(np.float32)
out = {}
for d, n, bpl in ((8, 4096, 0), (16, 8192, 0), (16, 4096, 0), (8, 16384, 0), (16, 16384, 0), (16, 12288, 0)):
    vl, keep = M.make_vlfunc(M.VL_ROSENBROCK1, d)
    e = M.Engine(d, n, pl=1.0)
    e.set_option(E.OPT_PERSIST, 1)
    e.set_option(E.OPT_BLOCKS_PER_LANE, bpl)
    e.stage_pinit(pinit(d, n))
    for _ in range(5):
        e.run(1000, 500, None, vl)
    reps = 60
    t0 = time.perf_counter()
    for _ in range(reps):
        e.run(1000, 500, None, vl)
    job = (time.perf_counter() - t0) / reps * 1e3
    e.set_option(E.OPT_PROFILE, 1)
    for _ in range(10):
        e.run(1000, 500, None, vl)
    pr = e.profile
    ker = pr["run_small"]["ms"] / max(pr["run_small"]["launches"], 1)
    out["%%dx%%d bpl%%d" %% (n, d, bpl)] = (round(job, 4), round(ker, 4), int(e.counters["small_n_blocks_per_lane"]))
    e.close()
print(json.dumps(out))
''' % ROOT


def main():
    if len(sys.argv) < 4:
        print(__doc__)
        return 2
    rounds, variants = int(sys.argv[1]), [os.path.abspath(v) for v in sys.argv[2:]]
    res = {}
    for r in range(rounds):
        for v in variants:
            env = dict(os.environ, MCX_LIBMCX=v)
            o = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=600)
            if o.returncode != 0:
                print("variant %s failed:\n%s" % (v, o.stderr[-2000:]))
                return 1
            got = json.loads(o.stdout.strip().splitlines()[-1])
            for k, val in got.items():
                res.setdefault(k, {}).setdefault(v, []).append(val)
            print("round %d variant %s: %s" % (r, v, got), flush=True)
    print("\nshape: library -> job ms median (min .. max) / kernel ms median over %d rounds" % rounds)
    med = lambda xs: sorted(xs)[len(xs) // 2] if len(xs) % 2 else 0.5 * (sorted(xs)[len(xs) // 2 - 1] + sorted(xs)[len(xs) // 2])
    for k, byv in res.items():
        ref = [x[0] for x in byv[variants[0]]]
        for v, xs in byv.items():
            job = [x[0] for x in xs]
            verdict = "" if v == variants[0] else ("  within" if med(job) <= med(ref) + (max(ref) - min(ref)) else "  SLOWER") + " (first + spread)"
            print("%s %s: job %.4f (%.4f .. %.4f) kernel %.4f%s" % (k, v, med(job), min(job), max(job), med([x[1] for x in xs]), verdict))
    return 0


if __name__ == "__main__":
    sys.exit(main())
