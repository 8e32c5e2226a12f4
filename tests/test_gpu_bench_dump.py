"""`python bench.py --gpus 1 --steps K --warmup W` as it is run for every change: a plain run times exactly K jobs, prints one
line with the headline fields and nothing that only --full measures, and --dump-outputs writes what the last timed job
computed -- bit for bit the oracle's state, log-likelihood, moments and sample rows after W + K runs of the same job (the
generator's counter carries on from run to run, tests/test_gpu_run_parity.py::test_second_run_continues_rng)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from test_bench_dump_cpu import load_bench

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_what_the_last_timed_job_computed(tmp_path):
    d, n, nburn, nsamp, steps, warmup = 16, 2048, 60, 40, 2, 1
    out_dir = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--chains", str(n), "--nburn", str(nburn), "--nsamp", str(nsamp), "--dump-outputs", str(out_dir)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode("utf-8", "replace")[-3000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    o = json.loads(lines[0])
    assert o["steps"] == steps and o["warmup"] == warmup and o["full"] is False
    assert o["unit"] == "chain-steps/s" and o["higher_is_better"] is True and o["dtype"] == "f32" and o["metric"].startswith("chain-steps")
    assert o["value"] == pytest.approx(n * (nburn + nsamp) / (o["ms_per_step"] * 1e-3), rel=1e-9)
    assert all(o[k] is None for k in ("roofline", "murray_roofline", "cpu_baseline", "end_to_end", "host_callback", "device_vlfunc"))
    assert o["config"]["value_with_host_pinit"] is None and o["config"]["other_configs"] is None
    assert list(o)[-1] == "summary"

    got = {f[:-4]: np.load(out_dir / f) for f in os.listdir(out_dir)}
    assert sorted(got) == ["loglike", "mean", "samples", "state", "var"]
    assert o["outputs"]["chains"] == "all"
    eo = O.Engine(d, n, pl=1.0)
    vo, _k = O.make_vlfunc(O.VL_ROSENBROCK1, d)
    p = load_bench().pinit_for(d, n, 0)
    for _ in range(warmup + steps):
        eo.run(nsamp, nburn, p, vo)
    for name in ("state", "loglike", "mean", "var"):
        assert np.array_equal(got[name].view(np.uint32), getattr(eo, name).view(np.uint32)), name
    rows = eo.samples[-nsamp * n:].reshape(nsamp, n, d + 1)  # (the oracle keeps every run's rows)
    assert np.array_equal(got["samples"].view(np.uint32), rows[o["outputs"]["sample_steps"]].view(np.uint32))
    eo.close()
