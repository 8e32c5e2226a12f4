"""mcx_*_evidence on the GPU against tests/evidence_ref.py.  No assertion carries a statistical tolerance.

What is held:
  log g      (debug_evidence_logg) per row within the forward bound of an fp64 product and a sum of squares in any order plus
             1-ulp exp and log: max_k (4 np + 16) 2^-53 A_k / 2 + 16 2^-53 (1 + |lg|), A_k = sum_i (sum_l |W_il u_l|)^2, against
             the restatement fed the library's own W and lc; at R - 1, R, R + 1 rows for the tile height R of the geometry entry,
             with more tiles than workgroups, a NaN parameter (NaN) and a row at a centre (lc)
  draws      (debug_evidence_draws) the rows and components bit for bit the restatement's; their log g within the bound; their
             log L exactly mcx_vlfunc_eval's
  the call   on the inputs tests/test_evidence_cpu.py shows to be decisive: l1 and l2 within the bound (the float log L is the
             device's), log_z, se, the halves and the by-products within a relative 1e-9 of evidence_ref.bridge on the device's
             own l1 and l2, iters and flags exactly, neff and ess_f2 section 9's numbers
  exact      a proposal equal to the target: log_z within 1e-4 of the closed form, at most 2 passes, se below 1e-4
  bytes      the engine, rows_evidence of its copied rows and a store of all its chains, and two calls in a row
The product runs on the vector unit at every np (use_mfma = 0 in the geometry entry), so there is no switch to cross."""
import os

import numpy as np
import pytest

import evidence_ref as R
import oracle_lib as O
from test_gpu_store_view import assert_same_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-9


def make_proposal(np_, K, seed, spread=2.0):
    """K components with random full covariances and centres that are floats"""
    from mcpar_amd import engine as E
    rng = np.random.default_rng(seed)
    covs = np.empty((K, np_, np_))
    for k in range(K):
        A = rng.normal(size=(np_, np_)) / np.sqrt(np_)
        covs[k] = A @ A.T + np.diag(rng.uniform(0.5, 1.5, np_))
    centres = (rng.normal(size=(K, np_)) * spread).astype(np.float32).astype(np.float64)
    return E.Proposal(rng.uniform(0.5, 2.0, K), centres, covs, scale=rng.uniform(0.8, 1.3))


def rows_near(p, n, seed):
    """n float rows scattered about the proposal's centres"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, p.k, n)
    return (p.centres[k] + rng.normal(size=(n, p.np)) * 1.5).astype(np.float32)


def check_logg(x, p, where):
    from mcpar_amd import engine as E
    _, W, lc = E.evidence_proposal(p)
    lg = E.debug_evidence_logg(x, p)
    ref, bound = R.logg(x, p.centres, W, lc)
    assert np.array_equal(np.isnan(lg), np.isnan(ref)), where
    ok = ~np.isnan(ref)
    err = np.abs(lg - ref)[ok]
    assert (err <= bound[ok]).all(), (where, float((err / bound[ok]).max()))
    return float((err / bound[ok]).max()) if ok.any() else 0.0, lg, lc


@pytest.mark.parametrize("np_", [1, 3, 4, 5, 16, 17, 64, 256])
def test_log_g_is_within_the_forward_bound(np_):
    from mcpar_amd import engine as E
    g = E.debug_evidence_geometry(np_, 1, 1, 1)
    Rt = g["tile_rows"]
    assert Rt == (64 if np_ <= 128 else 32) and g["slices"] * Rt == g["block"] == 256 and g["use_mfma"] == 0
    assert g["sweep_lds_bytes"] <= 64 * 1024
    worst = 0.0
    for K in (1, 2, 8):
        p = make_proposal(np_, K, 10 * np_ + K)
        for N in (Rt - 1, Rt, Rt + 1):
            gg = E.debug_evidence_geometry(np_, N, 1, K)
            assert gg["sweep_tiles"] == gg["sweep_workgroups"] == (2 if N > Rt else 1)
            x = rows_near(p, N, N + K)
            x[0] = p.centres[0]       # a row exactly at a centre
            if N > 2:
                x[N - 2, np_ - 1] = np.nan
                x[1, 0] = np.inf
            ratio, lg, lc = check_logg(x, p, (np_, K, N))
            assert np.isnan(lg[N - 2]) and np.isnan(lg[1])
            if K == 1:
                assert lg[0] == lc[0]
            worst = max(worst, ratio)
    print("np = %d: largest |lg - lg_ref| / bound %.3g" % (np_, worst))


def test_log_g_with_more_tiles_than_workgroups():
    """np = 1 and nc = 257 chains of 1021 steps: 4100 tiles for 4096 workgroups, so four workgroups take a second tile"""
    from mcpar_amd import engine as E
    N = 257 * 1021
    g = E.debug_evidence_geometry(1, N, 1, 2)
    assert g["sweep_tiles"] == 4100 and g["sweep_workgroups"] == g["sweep_max_workgroups"] == 4096
    p = make_proposal(1, 2, 5)
    ratio, _, _ = check_logg(rows_near(p, N, 6), p, "many tiles")
    print("many tiles: largest |lg - lg_ref| / bound %.3g" % ratio)


@pytest.mark.parametrize("np_", [1, 4, 5, 17, 256])
def test_draws_equal_the_restatement_bit_for_bit(np_):
    import mcpar_amd as M
    from mcpar_amd import engine as E
    vl, _keep = M.make_vlfunc(M.VL_GAUSSIAN, np_)
    worst = 0.0
    for K in (1, 8):
        p = make_proposal(np_, K, 77 * np_ + K, spread=0.5)
        Cf, W, lc = E.evidence_proposal(p)
        seed = 1000 + np_ + K
        xr, cr = R.draws(p.weights, p.centres, Cf, seed, 257)
        for n in (255, 256, 257):
            x, comp, lg, ll = E.debug_evidence_draws(p, n, seed, vl)
            assert np.array_equal(comp, cr[:n]), (np_, K, n)
            assert x.tobytes() == xr[:n].tobytes(), (np_, K, n, np.argwhere(x != xr[:n])[:4])
            ref, bound = R.logg(x, p.centres, W, lc)
            err = np.abs(lg - ref)
            assert (err <= bound).all(), (np_, K, n)
            worst = max(worst, float((err / bound).max()))
            assert ll.tobytes() == M.vlfunc_eval(M.VL_GAUSSIAN, np_, x).tobytes(), (np_, K, n)
        if K == 8:
            assert len(set(cr.tolist())) > 1
    print("np = %d: log g of the draws, largest ratio to the bound %.3g" % (np_, worst))


def lower_median(v):
    return float(np.sort(np.asarray(v))[(len(v) - 1) // 2])


@pytest.mark.parametrize("K", [1, 2], ids=["fitted", "two-components"])
@pytest.mark.parametrize("seed", R.DEC_SEEDS)
def test_the_whole_call_on_the_decisive_inputs(seed, K):
    import mcpar_amd as M
    from mcpar_amd import engine as E
    rows, which = R.decisive_rows(seed)
    T, nc, d, fit = R.DEC_T, R.DEC_NC, R.DEC_D, R.DEC_T // 2
    vl, _keep = M.make_vlfunc(M.VL_GAUSSMIX, d, R.DEC_PARAMS, 2)
    if K == 1:   # the library fits: section 10 on the first half
        cv = E.rows_covariance(rows[:fit * nc], fit, nc)
        p, arg = E.Proposal([1.0], cv["mean"][:d], cv["cov"][:d, :d]), None
    else:
        p = arg = E.Proposal(*R.decisive_proposal(rows, which, 2))
    res, l1, l2 = E.debug_evidence_l(rows, T, nc, vl, arg, ndraw=R.DEC_N2, seed=seed, fit_steps=fit)
    again = E.rows_evidence(rows, T, nc, vl, arg, ndraw=R.DEC_N2, seed=seed, fit_steps=fit)
    assert_same_bytes({k: np.asarray(v) for k, v in res.items()}, {k: np.asarray(v) for k, v in again.items()}, "two calls")
    assert (res["n1"], res["n2"], res["k"], res["fit_steps"]) == ((T - fit) * nc, R.DEC_N2, K, fit)
    # l1 and l2: the restatement with the library's factors, the float log L of the draws from the device
    _, W, lc = E.evidence_proposal(p)
    post = rows[fit * nc:]
    lg1, b1 = R.logg(post[:, :d], p.centres, W, lc)
    assert (np.abs(l1 - (post[:, d].astype(np.float64) - lg1)) <= b1).all()
    x, _, _, ll = E.debug_evidence_draws(p, R.DEC_N2, seed, vl)
    lg2, b2 = R.logg(x, p.centres, W, lc)
    assert np.isfinite(ll).all() and (np.abs(l2 - (ll.astype(np.float64) - lg2)) <= b2).all()
    # neff and ess_f2: section 9's numbers
    neff = min(lower_median(E.rows_summary(post, T - fit, nc, ())["ess"][:d]), float(post.shape[0]))
    assert res["neff"] == neff
    ref = R.bridge(l1, l2, neff=neff, ess_f2=res["ess_f2"])
    f2 = ref["f2"].astype(np.float32)
    ess_f2 = E.rows_summary(np.stack([f2, f2], axis=1), T - fit, nc, ())["ess"][0]
    assert abs(res["ess_f2"] - ess_f2) <= 1e-6 * ess_f2   # (the device's f2 floats may round another way in the last place)
    assert (res["iters"], res["flags"], res["ndraw_zero"]) == (ref["iters"], ref["flags"], ref["ndraw_zero"]) and res["iters"] < 50
    for name in ("lstar", "log_z", "se", "re2_draws", "re2_rows", "log_z_is", "log_z_ris"):
        assert abs(res[name] - ref[name]) <= RTOL * abs(ref[name]), (name, res[name], ref[name])
    print("seed %d, K = %d: log_z - truth = %+.4g, se = %.3g, %d passes" % (seed, K, res["log_z"] - R.DEC_TRUTH, res["se"], res["iters"]))


def test_an_exact_proposal_gives_log_z_at_once():
    """MCX_VL_GAUSSIAN with np = 3 and the caller's proposal (mu, diag sigma^2): every l is log Z up to the float log L, whose
    error is below 64 2^-24 8 for |log L| <= 64"""
    import mcpar_amd as M
    from mcpar_amd import engine as E
    d, nc, T = 3, 16, 64
    mu, s2 = np.array([0.5, -1.0, 2.0]), np.array([0.25, 1.0, 4.0])
    params = np.concatenate([mu, s2]).astype(np.float32)
    vl, _keep = M.make_vlfunc(M.VL_GAUSSIAN, d, params)
    rng = np.random.default_rng(3)
    x = (mu + rng.normal(size=(T * nc, d)) * np.sqrt(s2)).astype(np.float32)
    ll = M.vlfunc_eval(M.VL_GAUSSIAN, d, x, params)
    assert np.abs(ll).max() <= 64
    rows = np.concatenate([x, ll[:, None]], axis=1)
    res = E.rows_evidence(rows, T, nc, vl, E.Proposal([1.0], mu, np.diag(s2)), ndraw=1024, seed=9)
    truth = float(0.5 * np.log(2 * np.pi * s2).sum())
    print("exact proposal: log_z - truth = %+.3g, se = %.3g, %d passes" % (res["log_z"] - truth, res["se"], res["iters"]))
    assert abs(res["log_z"] - truth) <= 1e-4 and res["iters"] <= 2 and res["se"] < 1e-4 and res["fit_steps"] == 0


def test_engine_rows_and_store_give_the_same_bytes():
    import mcpar_amd as M
    from mcpar_amd import engine as E
    nc, d, steps = 256, 4, 48
    params = np.concatenate([np.linspace(-1.0, 1.0, d), np.linspace(0.5, 2.0, d)]).astype(np.float32)
    vl, _keep = M.make_vlfunc(M.VL_GAUSSIAN, d, params)
    eg = M.Engine(d, nc, pl=1.0)
    eg.run(steps, 40, O.default_pinit(d, nc), vl)
    spec = dict(ndraw=3000, seed=11)
    a = eg.evidence(**spec)                       # the last run's likelihood
    b = eg.evidence(vl, **spec)
    c = E.rows_evidence(eg.samples, steps, nc, vl, **spec)
    st = eg.select_chains(list(range(nc)))
    e = st.evidence(vl, **spec)
    st.close()
    f = eg.evidence(**spec)
    as_arrays = lambda r: {k: np.asarray(v) for k, v in r.items()}  # noqa: E731
    for other, what in ((b, "given L"), (c, "rows"), (e, "store"), (f, "again")):
        assert_same_bytes(as_arrays(a), as_arrays(other), what)
    assert a["fit_steps"] == steps // 2 and a["n1"] == (steps - steps // 2) * nc and a["k"] == 1 and np.isfinite(a["log_z"])
    ms, g = eg.evidence_times(**spec)
    assert_same_bytes(as_arrays(a), as_arrays(g), "timed")
    assert (ms >= 0).all() and ms[7] > 0
    eg.close()


def test_proposal_from_modes_takes_the_mode_table():
    from mcpar_amd import engine as E
    rows, which = R.decisive_rows(0)
    m = E.rows_modes(rows, R.DEC_T, R.DEC_NC, 2, seed=1)
    p = E.proposal_from_modes(m)
    assert p.k == 2 and np.array_equal(p.weights, np.asarray(m.table["weight"], np.float64))
    assert np.array_equal(p.centres, np.asarray(m.table["mean"], np.float64))
    order = np.argsort(p.centres[:, 0])
    for j, comp in zip(order, (0, 1)):   # the modes are the true components: their covariances are near the identity
        assert abs(p.weights[j] - (which == comp).mean()) < 1e-12
        assert np.abs(p.covs[j] - np.cov(rows[which == comp, :3].astype(np.float64).T)).max() < 1e-9
    m.close()


def test_refusals_that_need_the_device():
    import mcpar_amd as M
    from mcpar_amd import engine as E
    rows, _ = R.decisive_rows(1)
    T, nc, d = R.DEC_T, R.DEC_NC, R.DEC_D
    vl, _keep = M.make_vlfunc(M.VL_GAUSSMIX, d, R.DEC_PARAMS, 2)
    bad = rows.copy()
    fit = T // 2
    bad[fit * nc + 70, d] = np.inf
    bad[fit * nc + 9, 1] = np.nan
    bad[3, d] = np.nan   # (a fitting row's log L is not read)
    with pytest.raises(M.McxError) as ei:
        E.rows_evidence(bad, T, nc, vl, ndraw=256)
    assert ei.value.code == 1 and "row 9 is not finite" in str(ei.value)
    nothing, _k2 = M.make_vlfunc(M.VL_HOST, d, host_fn=lambda x: np.full(len(x), -np.inf, np.float32))
    with pytest.raises(M.McxError) as ei:
        E.rows_evidence(rows, T, nc, nothing, ndraw=256)
    assert ei.value.code == 1 and "every one of the 256 draws has L = 0" in str(ei.value)
    some, _k3 = M.make_vlfunc(M.VL_HOST, d, host_fn=lambda x: np.where(x[:, 0] > 3, -np.inf, -0.5 * (x * x).sum(axis=1)).astype(np.float32))
    res = E.rows_evidence(rows, T, nc, some, ndraw=256)
    assert 0 < res["ndraw_zero"] < 256 and np.isfinite(res["log_z"])
    short = E.rows_evidence(rows[:5 * nc], 5, nc, vl, fit_steps=2, ndraw=256)   # three steps are too few for section 9
    assert short["flags"] & E.EVIDENCE_NO_ESS and short["neff"] == short["ess_f2"] == 3 * nc


def test_a_likelihood_from_source_gives_the_built_ins_bytes():
    """mcpar_amd/examples restates Rosenbrock1 bit for bit (it holds no Gaussian): the same rows, the same result bytes"""
    import mcpar_amd as M
    from mcpar_amd import engine as E
    if not M.user_source_available():
        pytest.skip("no run-time compiler: " + M.load().mcx_last_error().decode())
    d, nc, steps = 2, 64, 64
    built, _k1 = M.make_vlfunc(M.VL_ROSENBROCK1, d)
    text = open(os.path.join(ROOT, "mcpar_amd", "examples", "user_rosenbrock1_whole.hip")).read()
    src, _k2 = M.make_vlfunc(M.VL_SOURCE, d, params=[1.0], source=text)
    eg = M.Engine(d, nc, pl=1.0)
    eg.run(steps, 200, O.default_pinit(d, nc), built)
    rows = eg.samples
    eg.close()
    a = E.rows_evidence(rows, steps, nc, built, ndraw=2048, seed=2)
    b = E.rows_evidence(rows, steps, nc, src, ndraw=2048, seed=2)
    assert_same_bytes({k: np.asarray(v) for k, v in a.items()}, {k: np.asarray(v) for k, v in b.items()}, "source")
