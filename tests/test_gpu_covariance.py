"""mcx_samples_covariance / Engine.covariance on the rows samples_range returns, against the float64 numpy restatement of
DESIGN.md section 10 (tests/covariance_ref.py).  Every entry within 4 (N + 16) 2^-53 sqrt(ref_ii ref_jj) -- derived in
covariance_ref.bound, not tuned -- exactly 0 for a constant column; the mean the bits of Engine.summary's; sqrt(diag)
its sd to 1e-9; symmetric bit for bit; the same bytes every call.  Each case prints its largest error / bound."""
import os
import subprocess

import numpy as np
import pytest

import covariance_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, "mcpar_amd", "drivers")


def mix_params(d, K):
    """K unit-variance Gaussians at 5k/(K-1) * 1, weights (5, 1, ..., 1)"""
    m = np.array([[5.0 * k / (K - 1)] * d for k in range(K)], np.float32).reshape(-1)
    return np.concatenate([m, np.array([5.0] + [1.0] * (K - 1), np.float32)])


def run(d, n, nburn, nsamp, kind=None, pl=1.0, stride=1, params=None, K=0, pinit=None, incov=None, opts=()):
    import mcpar_amd as M
    from mcpar_amd import engine as E
    kind = M.VL_ROSENBROCK1 if kind is None else kind
    vg, keep = M.make_vlfunc(kind, d, params, ncomp=K)
    eg = M.Engine(d, n, pl=pl)
    if stride > 1:
        eg.set_option(E.OPT_SAMPLE_STRIDE, stride)
    for o, v in opts:
        eg.set_option(o, v)
    eg.run(nsamp, nburn, O.default_pinit(d, n) if pinit is None else pinit, vg, incov)
    eg._vl_keep = keep
    return eg


def same_bytes(a, b):
    for k in ("mean", "cov", "corr", "flags"):
        assert a[k].tobytes() == b[k].tobytes(), k


def check_range(eg, first, nsteps, name, with_summary=True):
    got = eg.covariance(first_step=first, nsteps=nsteps)
    rows = eg.samples_range(first, nsteps)
    N = rows.shape[0]
    ratio = R.check(got, R.restate(rows), N, name)
    print("covariance %s: N = %d, np = %d, largest error / bound = %.3g" % (name, N, eg.np, ratio))
    ok = got["flags"] == 0
    c = got["corr"]
    pos = ok & (np.diag(got["cov"]) > 0)
    assert (np.diag(c)[pos] == 1.0).all() and np.isnan(c[~pos]).all() and np.isnan(c[:, ~pos]).all()
    assert np.array_equal(c[np.ix_(pos, pos)], R.corr_of(got["cov"])[np.ix_(pos, pos)])
    assert np.nanmax(np.abs(c), initial=0.0) <= 1 + 1e-9
    if with_summary and nsteps >= 4:
        s = eg.summary((), first_step=first, nsteps=nsteps)
        assert got["mean"].tobytes() == s["mean"].tobytes(), (name, "mean is not the summary's, bit for bit")
        np.testing.assert_allclose(np.sqrt(np.diag(got["cov"])[ok]), s["sd"][ok], rtol=1e-9, err_msg=name)
    return got


CONFIGS = {
    "rosen1-16x4096": dict(d=16, n=4096, nburn=300, nsamp=400),
    "rosen1-8x1000-odd": dict(d=8, n=1000, nburn=200, nsamp=301),
    "one-chain": dict(d=4, n=1, nburn=200, nsamp=1501),
    "small-n-512": dict(d=16, n=512, nburn=300, nsamp=300),
    "stride-3": dict(d=16, n=2048, nburn=200, nsamp=600, stride=3),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_covariance_matches_numpy(name):
    eg = run(**CONFIGS[name])
    check_range(eg, 0, eg.samples.shape[0] // eg.nc, name)


def test_sub_range():
    eg = run(**CONFIGS["rosen1-8x1000-odd"])
    check_range(eg, 50, 101, "sub-range")


def test_gaussmix_32d_murray():
    import mcpar_amd as M
    d, K = 32, 8
    eg = run(d, 2048, 150, 200, kind=M.VL_GAUSSMIX, pl=0.85, params=mix_params(d, K), K=K)
    assert eg.counters["remote_steps"] > 0
    check_range(eg, 0, 200, "gaussmix-32d-murray")


@pytest.mark.parametrize("d", [1, 2, 5, 17, 40, 256])
def test_tile_padding_and_tile_pairs(d):
    """np on either side of the 16-column tiles: one padded tile, two tiles, every pair of 16 tiles"""
    import mcpar_amd as M
    sig2 = np.linspace(0.5, 2.0, d)
    params = np.concatenate([np.linspace(-1.0, 1.0, d), sig2]).astype(np.float32)
    eg = run(d, 24, 100, 120, kind=M.VL_GAUSSIAN, params=params)
    got = check_range(eg, 0, 120, "gaussian-np-%d" % d)
    assert (np.diag(got["cov"]) > 0).all()


@pytest.mark.parametrize("nc", [1, 2, 3, 5, 7, 33])
def test_row_group_tail(nc):
    """one step of nc chains, nc not a multiple of the four rows of a matrix-core issue (N = 1 is refused)"""
    import mcpar_amd as M
    eg = run(6, nc, 50, 9)
    if nc == 1:
        with pytest.raises(M.McxError):
            eg.covariance(first_step=3, nsteps=1)
        check_range(eg, 3, 2, "tail-nc-1-two-steps")
        return
    check_range(eg, 3, 1, "tail-nc-%d" % nc)


def test_offset_column():
    """mean 1e4, variance 1: the case a one-pass sum xy - N m m formula loses"""
    import mcpar_amd as M
    d, n = 4, 256
    params = np.array([1e4] * d + [1.0] * d, np.float32)
    pinit = (1e4 + O.default_pinit(d, n)).astype(np.float32)
    eg = run(d, n, 500, 500, kind=M.VL_GAUSSIAN, params=params, pinit=pinit)
    got = check_range(eg, 0, 500, "offset-1e4")
    assert (np.abs(got["mean"][:d] - 1e4) < 1.0).all() and (np.diag(got["cov"])[:d] < 10.0).all()


def test_same_bytes_every_call():
    eg = run(**CONFIGS["rosen1-8x1000-odd"])
    same_bytes(eg.covariance(), eg.covariance())
    eg.summary()  # shares the scratch buffer
    same_bytes(eg.covariance(first_step=10, nsteps=77), eg.covariance(first_step=10, nsteps=77))


def test_async_run_equals_synchronous():
    import mcpar_amd as M
    from mcpar_amd import engine as E
    d, n = 16, 8192
    vg, keep = M.make_vlfunc(M.VL_ROSENBROCK1, d)
    a = M.Engine(d, n, pl=1.0)
    a.set_option(E.OPT_ASYNC_RUN, 1)
    a.run(200, 300, O.default_pinit(d, n), vg)
    ca = a.covariance()  # straight after the queued run
    b = M.Engine(d, n, pl=1.0)
    b.run(200, 300, O.default_pinit(d, n), vg)
    same_bytes(ca, b.covariance())


def test_minus_inf_log_likelihood():
    """the host likelihood of test_gpu_summary: chain 0 never leaves x0 > 5, so its log L stays -inf"""
    import mcpar_amd as M
    from mcpar_amd import engine as E
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
    got = check_range(eg, 0, 60, "minus-inf-logL")
    assert got["flags"].tolist() == [0] * d + [E.SUMMARY_NONFINITE]
    assert np.isnan(got["cov"][d]).all() and np.isnan(got["cov"][:, d]).all() and np.isfinite(got["cov"][:d, :d]).all()


def test_nan_planted_in_a_parameter_column():
    from mcpar_amd import engine as E
    eg = run(**CONFIGS["rosen1-8x1000-odd"])
    nsteps, nc = 40, eg.nc
    rows = eg.samples_range(0, nsteps).copy()
    clean = E.rows_covariance(rows, nsteps, nc)
    rows[12345, 3] = np.nan
    got = E.rows_covariance(rows, nsteps, nc)
    ratio = R.check(got, R.restate(rows), rows.shape[0], "nan-planted")
    print("covariance nan-planted: largest error / bound = %.3g" % ratio)
    assert got["flags"].tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 0]
    keep = [0, 1, 2, 4, 5, 6, 7, 8]
    assert got["cov"][np.ix_(keep, keep)].tobytes() == clean["cov"][np.ix_(keep, keep)].tobytes()


def test_rows_covariance_equals_engine_covariance():
    from mcpar_amd import engine as E
    for name, first, nsteps in (("rosen1-8x1000-odd", 0, 301), ("rosen1-8x1000-odd", 7, 50), ("small-n-512", 0, 300)):
        eg = run(**CONFIGS[name])
        same_bytes(E.rows_covariance(eg.samples_range(first, nsteps), nsteps, eg.nc), eg.covariance(first, nsteps))


def test_errors():
    import mcpar_amd as M
    from mcpar_amd import engine as E
    eg = M.Engine(4, 64)
    with pytest.raises(M.McxError):  # no run yet
        eg.covariance()
    vg, keep = M.make_vlfunc(M.VL_ROSENBROCK1, 4)
    eg.run(20, 10, O.default_pinit(4, 64), vg)
    for kw in (dict(first_step=0, nsteps=21), dict(first_step=-1, nsteps=8), dict(first_step=17, nsteps=4),
               dict(first_step=0, nsteps=0), dict(first_step=20, nsteps=1)):
        with pytest.raises(M.McxError) as ei:
            eg.covariance(**kw)
        assert ei.value.code == 1
    eg.covariance(first_step=19, nsteps=1)  # one step of 64 chains is enough
    with pytest.raises(M.McxError):
        eg.proposal_cov(first_step=0, nsteps=21)
    eg.set_option(E.OPT_SAMPLES, 0)
    eg.run(20, 0, O.default_pinit(4, 64), vg)
    with pytest.raises(M.McxError):
        eg.covariance()
    eg.set_option(E.OPT_SAMPLES, 1)
    eg.set_sink(lambda first, nsteps, rows: 0, 5)
    eg.run(20, 0, O.default_pinit(4, 64), vg)
    with pytest.raises(M.McxError):  # a run into a sink leaves no store
        eg.covariance()
    one = M.Engine(4, 1)
    one.run(20, 10, O.default_pinit(4, 1), vg)
    with pytest.raises(M.McxError) as ei:  # nsteps = 1, nc = 1: one row
        one.covariance(first_step=0, nsteps=1)
    assert ei.value.code == 1
    one.covariance(first_step=0, nsteps=2)


def test_c3_full_shape():
    """C3: 65 536 chains x 16-D, 500 + 1000; the matrix against float64 Xc^T Xc accumulated from chunked copies about the
    returned mean"""
    d, n, nburn, nsamp = 16, 65536, 500, 1000
    eg = run(d, n, nburn, nsamp)
    got = eg.covariance()
    N = nsamp * n
    s = eg.summary(())
    assert got["mean"].tobytes() == s["mean"].tobytes()
    acc = np.zeros((d + 1, d + 1))
    tot = np.zeros(d + 1)
    for s0 in range(0, nsamp, 50):
        x = eg.samples_range(s0, 50).astype(np.float64)
        tot += x.sum(axis=0)
        x -= got["mean"]
        acc += x.T @ x
    ref = dict(mean=tot / N, cov=acc / (N - 1), flags=np.zeros(d + 1, np.int32))
    ratio = R.check(got, ref, N, "c3")
    print("covariance c3: N = %d, largest error / bound = %.3g" % (N, ratio))
    np.testing.assert_allclose(np.sqrt(np.diag(got["cov"])), s["sd"], rtol=1e-9)


def test_pilot_covariance_improves_the_second_run():
    """the loop closed: a Gaussian with variances from 1e-2 to 1e2; run A with the identity proposal, run B with
    proposal_cov() of A's store.  B's worst ESS exceeds A's (CPU oracle: 1128 against 5481)."""
    import mcpar_amd as M
    d, n = 8, 1024
    sig2 = np.logspace(-2, 2, d)
    params = np.concatenate([np.zeros(d), sig2]).astype(np.float32)
    a = run(d, n, 500, 1000, kind=M.VL_GAUSSIAN, params=params)
    P = a.proposal_cov()
    assert P.dtype == np.float32 and np.array_equal(P, P.T)
    assert np.array_equal(P, R.proposal(a.covariance()["cov"], d)[0])
    ess_a = a.summary(())["ess"][:d].min()
    b = run(d, n, 500, 1000, kind=M.VL_GAUSSIAN, params=params, incov=P)
    ess_b = b.summary(())["ess"][:d].min()
    print("pilot covariance: min ESS over parameters %.0f (identity proposal) -> %.0f (proposal_cov of the pilot)" % (ess_a, ess_b))
    assert ess_b > ess_a
    dg = np.diag(b.chol)
    assert dg.max() > dg.min() and np.unique(dg).size > 1


def test_driver_covariance_proposal_incov(tmp_path):
    exe = os.path.join(DRV, "mcpar-run")
    args = [exe, "--func", "gauss", "--np", "4", "--nc", "256", "--nsamp", "201", "--nburn", "100", "--binary"]
    a = subprocess.run(args + ["--out", "rows.bin", "--covariance", "c.txt", "--proposal", "p.txt"], cwd=tmp_path,
                       capture_output=True, timeout=300)
    assert a.returncode == 0, a.stderr.decode()
    os.rename(tmp_path / "rows.bin", tmp_path / "rows_c.bin")
    b = subprocess.run(args + ["--out", "rows.bin"], cwd=tmp_path, capture_output=True, timeout=300)
    assert b.returncode == 0, b.stderr.decode()
    assert a.stdout == b.stdout
    assert (tmp_path / "rows_c.bin").read_bytes() == (tmp_path / "rows.bin").read_bytes()
    rows = np.fromfile(tmp_path / "rows.bin", np.float32).reshape(-1, 5)
    assert rows.shape[0] == 201 * 256
    ref = R.restate(rows)
    lines = (tmp_path / "c.txt").read_text().splitlines()
    names = ["p0", "p1", "p2", "p3", "LL"]
    assert lines[0].split() == ["name", "mean"] + names
    assert [ln.split()[0] for ln in lines[1:]] == names
    v = np.array([[float(t) for t in ln.split()[1:]] for ln in lines[1:]])
    got = dict(mean=v[:, 0].copy(), cov=np.ascontiguousarray(v[:, 1:]), flags=np.zeros(5, np.int32))
    R.check(got, ref, rows.shape[0], "driver")  # %.17g gives the doubles back
    P = np.array([[float(t) for t in ln.split()] for ln in (tmp_path / "p.txt").read_text().splitlines()])
    assert P.shape == (4, 4)
    assert np.array_equal(P.astype(np.float32), R.proposal(got["cov"], 4)[0])  # %.9g gives the floats back
    # the second stage: the pilot's proposal as incov
    c = subprocess.run(args + ["--out", "rows2.bin", "--incov", "p.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert c.returncode == 0, c.stderr.decode()
    rows2 = np.fromfile(tmp_path / "rows2.bin", np.float32).reshape(-1, 5)
    assert rows2.shape == rows.shape and not np.array_equal(rows2, rows)
    # np * np - 1 numbers
    (tmp_path / "short.txt").write_text(" ".join(str(t) for t in P.reshape(-1)[:-1]) + "\n")
    e = subprocess.run(args + ["--out", "rows3.bin", "--incov", "short.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert e.returncode == 2 and b"--incov" in e.stderr
    # a matrix covar_setup rejects
    Q = P.copy()
    Q[1, 1] = 0.0
    (tmp_path / "bad.txt").write_text("\n".join(" ".join(repr(float(t)) for t in r) for r in Q) + "\n")
    e = subprocess.run(args + ["--out", "rows3.bin", "--incov", "bad.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert e.returncode == 2 and b"--incov" in e.stderr
    # no rows on the host: refused
    for flag, f in (("--covariance", "c2.txt"), ("--proposal", "p2.txt")):
        e = subprocess.run(args[:-1] + ["--stream-text", flag, f], cwd=tmp_path, capture_output=True, timeout=300)
        assert e.returncode == 2 and b"--covariance" in e.stderr
