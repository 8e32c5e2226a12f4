"""mcx_samples_summary / Engine.summary: every field against the float64 numpy restatement of DESIGN.md "Sample-store
summaries" (tests/summary_ref.py), on the rows samples_range returns -- order statistics and min / max bit-exact,
quantiles 1e-12 relative, mean / sd 1e-9 relative, rhat 1e-7 absolute, ess_lag equal, ess / mcse 1e-4 relative."""
import math
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import summary_ref as R

pytestmark = pytest.mark.gpu

PROBS = (0.01, 0.25, 0.5, 0.9, 0.99)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, "mcpar_amd", "drivers")


def mix_params(d, K):
    """K unit-variance Gaussians at 5k/(K-1) * 1, weights (5, 1, ..., 1)"""
    m = np.array([[5.0 * k / (K - 1)] * d for k in range(K)], np.float32).reshape(-1)
    return np.concatenate([m, np.array([5.0] + [1.0] * (K - 1), np.float32)])


def run(d, n, nburn, nsamp, kind=None, pl=1.0, stride=1, params=None, K=0, pinit=None):
    import mcpar_amd as M
    from mcpar_amd import engine as E
    kind = M.VL_ROSENBROCK1 if kind is None else kind
    vg, keep = M.make_vlfunc(kind, d, params, ncomp=K)
    eg = M.Engine(d, n, pl=pl)
    if stride > 1:
        eg.set_option(E.OPT_SAMPLE_STRIDE, stride)
    eg.run(nsamp, nburn, O.default_pinit(d, n) if pinit is None else pinit, vg)
    eg._vl_keep = keep
    return eg


def check_range(eg, first, nsteps, probs=PROBS):
    got = eg.summary(probs, first_step=first, nsteps=nsteps)
    rows = eg.samples_range(first, nsteps)
    R.check(got, R.restate(rows, nsteps, eg.nc, probs))
    return got


CONFIGS = {
    "rosen1-16x4096": dict(d=16, n=4096, nburn=300, nsamp=400),
    "rosen1-8x1000-odd": dict(d=8, n=1000, nburn=200, nsamp=301),
    "one-chain": dict(d=4, n=1, nburn=200, nsamp=1501),
    "small-n-512": dict(d=16, n=512, nburn=300, nsamp=300),
    "stride-3": dict(d=16, n=2048, nburn=200, nsamp=600, stride=3),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_summary_matches_numpy(name):
    eg = run(**CONFIGS[name])
    got = check_range(eg, 0, eg.samples.shape[0] // eg.nc)
    assert got["ess_lag"].max() > 0


def test_sub_range():
    eg = run(**CONFIGS["rosen1-8x1000-odd"])
    check_range(eg, 50, 101)


def test_gaussmix_32d_murray():
    import mcpar_amd as M
    d, K = 32, 8
    eg = run(d, 2048, 150, 200, kind=M.VL_GAUSSMIX, pl=0.85, params=mix_params(d, K), K=K)
    assert eg.counters["remote_steps"] > 0
    check_range(eg, 0, 200)


def test_same_bytes_every_call():
    eg = run(**CONFIGS["rosen1-8x1000-odd"])
    a, b = eg.summary(PROBS), eg.summary(PROBS)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_errors():
    import mcpar_amd as M
    from mcpar_amd import engine as E
    eg = M.Engine(4, 64)
    with pytest.raises(M.McxError):  # no run yet
        eg.summary()
    vg, keep = M.make_vlfunc(M.VL_ROSENBROCK1, 4)
    eg.run(20, 10, O.default_pinit(4, 64), vg)
    for kw in (dict(first_step=0, nsteps=21), dict(first_step=-1, nsteps=8), dict(first_step=17, nsteps=4),
               dict(first_step=0, nsteps=3), dict(probs=(0.5, 1.5)), dict(probs=(-0.1,)), dict(probs=(math.nan,)),
               dict(probs=[0.5] * 33)):
        with pytest.raises(M.McxError):
            eg.summary(**kw)
    eg.summary(probs=[0.5] * 32)  # 32 is allowed
    assert eg.summary(probs=())["quantiles"].shape == (5, 0)
    eg.set_option(E.OPT_SAMPLES, 0)
    eg.run(20, 0, O.default_pinit(4, 64), vg)
    with pytest.raises(M.McxError):
        eg.summary()
    eg.set_option(E.OPT_SAMPLES, 1)
    eg.set_sink(lambda first, nsteps, rows: 0, 5)
    eg.run(20, 0, O.default_pinit(4, 64), vg)
    with pytest.raises(M.McxError):  # a run into a sink leaves no store
        eg.summary()


def test_minus_inf_log_likelihood():
    """a host likelihood that is -inf beyond x0 > 5: chain 0 starts there and never leaves, so its log L stays -inf"""
    import mcpar_amd as M
    d, n = 4, 64

    def lik(x):
        y = -0.5 * (x.astype(np.float64) ** 2).sum(axis=1)
        y[x[:, 0] > 5.0] = -np.inf
        return y.astype(np.float32)
    v, keep = M.make_vlfunc(M.VL_HOST, d, host_fn=lik)
    eg = M.Engine(d, n, pl=1.0)
    p = O.default_pinit(d, n)
    p[0, 0] = 100.0
    eg.run(60, 20, p, v)
    got = check_range(eg, 0, 60)
    assert got["flags"][d] == 1 and math.isnan(got["rhat"][d]) and got["min"][d] == -np.inf
    assert not got["flags"][:d].any() and np.isfinite(got["ess"][:d]).all()


def test_async_run_equals_synchronous():
    import mcpar_amd as M
    from mcpar_amd import engine as E
    d, n = 16, 8192
    vg, keep = M.make_vlfunc(M.VL_ROSENBROCK1, d)
    a = M.Engine(d, n, pl=1.0)
    a.set_option(E.OPT_ASYNC_RUN, 1)
    a.run(200, 300, O.default_pinit(d, n), vg)
    sa = a.summary(PROBS)  # straight after the queued run
    b = M.Engine(d, n, pl=1.0)
    b.run(200, 300, O.default_pinit(d, n), vg)
    sb = b.summary(PROBS)
    for k in sa:
        assert sa[k].tobytes() == sb[k].tobytes(), k


def test_statistics_gaussian_mixes():
    """a Gaussian with known mean: converged chains, the mean within 5 mcse of it"""
    import mcpar_amd as M
    d, n, mu = 4, 256, 1.5
    params = np.array([mu] * d + [1.0] * d, np.float32)
    eg = run(d, n, 1000, 2000, kind=M.VL_GAUSSIAN, params=params)
    s = eg.summary()
    print("gaussian: rhat", s["rhat"][:d], "ess", s["ess"][:d], "mean", s["mean"][:d], "mcse", s["mcse_mean"][:d])
    assert (s["rhat"][:d] < 1.01).all()
    assert (np.abs(s["mean"][:d] - mu) < 5 * s["mcse_mean"][:d]).all()


def test_statistics_separate_modes():
    """two far modes, half the chains started in each, no Murray step: R-hat sees that they never mix"""
    import mcpar_amd as M
    n = 512
    p = np.zeros((n, 2), np.float32)
    p[n // 2:] = 12.0
    params = np.array([0, 0, 12, 12, 5, 1], np.float32)
    eg = run(2, n, 200, 400, kind=M.VL_GAUSSMIX, params=params, K=2, pinit=p)
    s = eg.summary()
    print("two modes: rhat", s["rhat"])
    assert (s["rhat"][:2] > 1.1).all()


def test_c3_full_shape():
    """C3: 65 536 chains x 16-D, 500 + 1000; columns 0, 15 and log L against numpy from chunked copies"""
    d, n, nburn, nsamp = 16, 65536, 500, 1000
    eg = run(d, n, nburn, nsamp)
    got = eg.summary(PROBS)
    want = (0, 15, d)
    cols = {c: np.empty((nsamp, n), np.float32) for c in want}
    for s0 in range(0, nsamp, 50):
        rows = eg.samples_range(s0, 50).reshape(50, n, d + 1)
        for c in want:
            cols[c][s0:s0 + 50] = rows[:, :, c]
    R.check(got, {c: R.restate_column(cols[c], PROBS) for c in want})


def test_driver_summary(tmp_path):
    args = [os.path.join(DRV, "mcpar-run"), "--func", "gauss", "--np", "4", "--nc", "256", "--nsamp", "201", "--nburn",
            "100", "--binary"]
    a = subprocess.run(args + ["--out", "rows.bin", "--summary", "s.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert a.returncode == 0, a.stderr.decode()
    os.rename(tmp_path / "rows.bin", tmp_path / "rows_s.bin")
    b = subprocess.run(args + ["--out", "rows.bin"], cwd=tmp_path, capture_output=True, timeout=300)
    assert b.returncode == 0, b.stderr.decode()
    assert a.stdout == b.stdout
    assert (tmp_path / "rows_s.bin").read_bytes() == (tmp_path / "rows.bin").read_bytes()
    rows = np.fromfile(tmp_path / "rows.bin", np.float32).reshape(-1, 5)
    assert rows.shape[0] == 201 * 256
    ref = R.restate(rows, 201, 256, (0.01, 0.5, 0.99))
    lines = (tmp_path / "s.txt").read_text().splitlines()
    assert lines[0].split() == ["name", "mean", "sd", "q01", "q50", "q99", "rhat", "ess", "mcse"]
    assert [ln.split()[0] for ln in lines[1:]] == ["p0", "p1", "p2", "p3", "LL"]
    for c, ln in enumerate(lines[1:]):
        v = [float(t) for t in ln.split()[1:]]
        r = ref[c]
        np.testing.assert_allclose(v[0:2], [r["mean"], r["sd"]], rtol=1e-9)
        np.testing.assert_allclose(v[2:5], r["quantiles"], rtol=1e-12)
        assert abs(v[5] - r["rhat"]) < 1e-7
        np.testing.assert_allclose(v[6:8], [r["ess"], r["mcse_mean"]], rtol=1e-4)
    # no store on the host to summarise: refused
    c = subprocess.run(args[:-1] + ["--stream-text", "--summary", "s2.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert c.returncode == 2 and b"--summary" in c.stderr
