"""The oracle alone on chains that start at log L = -inf or NaN, or with an infinite or NaN coordinate (no GPU): the
semantics of DESIGN.md section 3 "Non-finite values" replayed from the rows, the isolation of a poisoned chain from its
neighbours, and the end of a Murray call that cannot succeed.  tests/test_gpu_nonfinite.py asks the same of the kernels.
Every Murray job runs in a process of its own under a time limit: before the loop was bounded some of them never returned."""
import functools

import numpy as np
import pytest

import nonfinite_cases as N
import oracle_lib as O
import step_ref as R


def oracle_run(c, pinit, nburn, nsamp, seed=N.SEED, incov="case"):
    vo, keep = O.make_vlfunc(c["kind"], c["d"], c["params"], c["ncomp"])
    eo = O.Engine(c["d"], c["n"], pl=1.0, sync=c["sync"], seed=seed, threads=4)
    eo.set_record(samples=True, mask=True)
    eo.run(nsamp, nburn, pinit, vo, c["incov"] if isinstance(incov, str) else incov)
    return eo


_RUNS = {}


def runs_without_burn_in(name):
    """the case at nburn = 0, pl = 1, with and without its poisoned chains: computed once, shared, left unchanged"""
    if name not in _RUNS:
        c = N.poisoned_start(name)
        nsamp = min(c["nsamp"], 40)
        _RUNS[name] = (c, nsamp, oracle_run(c, c["pinit"], 0, nsamp), oracle_run(c, c["clean"], 0, nsamp))
    return _RUNS[name]


@pytest.fixture(scope="module", autouse=True)
def close_the_shared_engines():
    yield
    for c, nsamp, eo, ec in _RUNS.values():
        eo.close(); ec.close()
    _RUNS.clear()


def loglike_of(c):
    return lambda x: O.vl_eval(c["kind"], c["d"], x, c["params"], c["ncomp"])


def test_the_draw_that_is_zero():
    assert N.u0_draw_is_zero()
    assert O.lib().mcxo_accept_lu(0x61) == -np.inf and O.lib().mcxo_accept_lu(0xff) == -np.inf
    assert np.isfinite(O.lib().mcxo_accept_lu(0x100))


@pytest.mark.parametrize("name", N.FAMILIES)
def test_semantics_from_the_rows(name):
    c, nsamp, eo, _clean = runs_without_burn_in(name)
    ll = loglike_of(c)
    start = N.row_of_start(c["pinit"], ll(c["pinit"]))
    rows = eo.samples.reshape(nsamp, c["n"], c["d"] + 1)
    seen = N.check_semantics(start, rows, eo.accept_mask, lambda t, x: eo.gen_local(t, x)[0], ll, name)
    print(name, seen, {j: (w, float(start[j, -1])) for j, w in c["where"].items()})
    # the poisons reach both classes in every family, and healthy chains meet proposals they must refuse
    assert seen["nan_stays"] >= 2 * nsamp and seen["minf_stays"] >= nsamp
    # the classes of the starts: a NaN coordinate gives a NaN log L; nothing poisoned is +inf
    for j, w in c["where"].items():
        assert (w in ("one_nan", "all_nan")) == bool(np.isnan(start[j, -1])), (j, w, start[j, -1])
        assert start[j, -1] != np.inf


@pytest.mark.parametrize("name", N.FAMILIES)
def test_a_poisoned_chain_reaches_no_other(name):
    c, nsamp, eo, ec = runs_without_burn_in(name)
    h, p = c["healthy"], c["poisoned"]
    rows = eo.samples.reshape(nsamp, c["n"], -1)
    clean = ec.samples.reshape(nsamp, c["n"], -1)
    assert np.isfinite(clean).all()
    assert np.array_equal(N.bits(rows[:, h]), N.bits(clean[:, h]))
    for what in ("state", "loglike", "mean", "var"):
        assert np.array_equal(N.bits(getattr(eo, what)[h]), N.bits(getattr(ec, what)[h])), what
    assert np.array_equal(eo.accept_counts[h], ec.accept_counts[h])
    assert np.array_equal(eo.accept_mask[:, h], ec.accept_mask[:, h])
    # a poisoned chain holds its start row at every step (1e12 + z rounds to 1e12: even a chain that may move stays put)
    start = N.row_of_start(c["pinit"], loglike_of(c)(c["pinit"]))
    for t in range(nsamp):
        N.assert_same(rows[t, p], start[p], "%s step %d" % (name, t))
    # and whoever has a non-finite log L was never counted as accepted
    stuck = p[~np.isfinite(start[p, -1])]
    assert not eo.accept_counts[stuck].any() and not eo.accept_mask[:, stuck].any()
    assert eo.naccept_main - int(eo.accept_counts[p].sum()) == ec.naccept_main - int(ec.accept_counts[p].sum())


def test_mixture_classes_against_float64():
    """the mixture's log-sum-exp at the poisoned starts: finite and right wherever sum (x - m)^2 fits fp32, NaN for a NaN
    coordinate, neither finite nor +inf beyond"""
    c = N.poisoned_start("mixture_32d")
    K, d = c["ncomp"], c["d"]
    means, wts = c["params"][:K * d].reshape(K, d).astype(np.float64), c["params"][K * d:].astype(np.float64)
    x = c["pinit"].astype(np.float64)
    y = loglike_of(c)(c["pinit"])
    with np.errstate(invalid="ignore", over="ignore"):
        sq = ((x[:, None, :] - means[None]) ** 2).sum(-1)
        e = -0.5 * sq + np.log(wts)[None]
        ref = np.logaddexp.reduce(e, axis=1)
    fits = np.nan_to_num(sq.max(1), nan=np.inf) < 1e38
    assert fits[c["healthy"]].all() and not fits[c["poisoned"]].all()
    # fp32: d fma per component and an exp / log pair of relative error < 4 ulp each: (d + 8) ulp of the largest exponent
    tol = (d + 8) * 2.0 ** -24 * np.maximum(1.0, np.abs(e).max(1))
    assert np.isfinite(y[fits]).all() and (np.abs(y[fits] - ref[fits]) <= tol[fits]).all()
    hasnan = np.isnan(x).any(1)
    assert np.isnan(y[hasnan]).all()
    rest = ~fits & ~hasnan
    assert rest.any() and not np.isfinite(y[rest]).any() and not (y[rest] == np.inf).any()


def test_a_zero_draw_takes_any_finite_proposal():
    """u24 = 0: log1(u24) = -inf, below every difference but -inf and NaN.  Proposals of scale 10 on Rosenbrock1 drop log L
    by millions: only the chain whose draw is 0 takes one."""
    d, n, j = 16, 128, N.U0_CHAIN
    c = dict(kind=O.VL_ROSENBROCK1, d=d, n=n, params=None, ncomp=0, sync=10, incov=None)
    incov = (100.0 * np.eye(d)).astype(np.float32)
    pinit = N.default_pinit(d, n)
    eo = oracle_run(c, pinit, 0, 1, seed=N.U0_SEED, incov=incov)
    ll = loglike_of(c)
    xp = eo.gen_local(0, pinit)[0]
    drop = ll(xp) - ll(pinit)
    assert np.isfinite(drop).all() and drop[j] < -1000.0
    u = R.accept_u(N.U0_SEED, 0, np.arange(n))
    assert u[j] == 0.0 and (np.log(u[np.arange(n) != j]) > drop[np.arange(n) != j]).all()   # (every other draw refuses, by a wide margin)
    assert eo.accept_mask[0, j] == 1 and eo.accept_mask[0].sum() == 1
    assert np.array_equal(N.bits(eo.state[j]), N.bits(xp[j]))
    N.check_semantics(N.row_of_start(pinit, ll(pinit)), eo.samples.reshape(1, n, d + 1), eo.accept_mask, lambda t, x: xp, ll, "u24 = 0")


def box_run(pl, seed=N.SEED, pinit=None, nburn=N.BOX_NBURN, nsamp=N.BOX_NSAMP, incov=None):
    d, n = N.BOX_D, N.BOX_N
    def tramp(ctx, npset, x, y):
        np.ctypeslib.as_array(y, shape=(npset,))[:] = N.box_numpy(np.ctypeslib.as_array(x, shape=(npset, d)))
        return 0
    cb = O.HOSTFN(tramp)
    vo, keep = O.make_vlfunc(O.VL_HOST, d, fn=cb)
    eo = O.Engine(d, n, pl=pl, seed=seed)
    eo.set_record(samples=True, mask=True)
    eo.run(nsamp, nburn, N.box_pinit() if pinit is None else pinit, vo, incov)
    eo._keep.append((cb, keep))
    return eo


def test_box_prior_at_pl_1():
    """a chain outside the box (-inf) takes the first proposal that lands inside, a chain inside never leaves: nburn = 0,
    proposals of scale 0.1"""
    incov = (0.01 * np.eye(N.BOX_D)).astype(np.float32)
    pinit = N.box_pinit()
    eo = box_run(1.0, nburn=0, nsamp=60, incov=incov)
    start = N.row_of_start(pinit, N.box_numpy(pinit))
    assert list(np.flatnonzero(start[:, -1] == -np.inf)) == list(N.BOX_OUTSIDE)
    seen = N.check_semantics(start, eo.samples.reshape(60, N.BOX_N, -1), eo.accept_mask, lambda t, x: eo.gen_local(t, x)[0], N.box_numpy, "box")
    print(seen)
    assert seen["minf_leaves"] >= 1 and seen["minf_stays"] >= 1 and seen["finite_refuses"] >= 100
    assert np.isfinite(eo.loglike[N.BOX_OUTSIDE[0]])   # the chain just outside has come in


def test_a_zero_draw_lets_a_chain_at_minus_inf_in():
    """the chain whose first draw is u24 = 0 starts outside the box, its first proposal lands inside: taken"""
    d, n, j = N.BOX_D, N.BOX_N, N.U0_CHAIN
    incov = (0.01 * np.eye(d)).astype(np.float32)
    z = R.normals(N.U0_SEED, R.ST_LOCAL, 0, np.array([j]), d)[0]
    pinit = N.default_pinit(d, n)
    pinit[j] = (-0.1 * z).astype(np.float32)                      # the proposal lands near the origin ...
    pinit[j, 0] = np.float32(-np.sign(z[0]) * (0.6 + 0.05 * abs(z[0])))   # ... from outside the box in coordinate 0
    assert abs(z[0]) > 0.01 and np.abs(pinit[j, 1:]).max() < 0.6
    eo = box_run(1.0, seed=N.U0_SEED, pinit=pinit, nburn=0, nsamp=1, incov=incov)
    xp = eo.gen_local(0, pinit)[0]
    assert N.box_numpy(pinit)[j] == -np.inf and np.isfinite(N.box_numpy(xp)[j])
    assert eo.accept_mask[0, j] == 1 and np.array_equal(N.bits(eo.state[j]), N.bits(xp[j]))


def test_the_box_prior_sources_build():
    """both source forms of the box prior compile into the step kernels (hiprtc cross-compiles for gfx950: no GPU needed)"""
    import ctypes as C
    import mcpar_amd as M
    lib = M.load()
    assert lib.mcx_user_source_available() == 1, lib.mcx_last_error()
    n = C.c_size_t(0)
    for text in (N.BOX_BLOCK_FORM, N.BOX_WHOLE_FORM):
        assert lib.mcx_debug_user_source_compile(text.encode(), N.BOX_D, C.byref(n)) == 0 and n.value > 10000, lib.mcx_last_error()
    assert lib.mcx_debug_user_source_compile_small(N.BOX_BLOCK_FORM.encode(), N.BOX_D, 1, 1, C.byref(n)) == 0, lib.mcx_last_error()


# ---- Murray steps --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def job(name, max_passes=0):
    return N.oracle_job_in_child(name, max_passes)


@pytest.mark.parametrize("name", ["minf_16d", "minf_36d"])
def test_murray_rescues_chains_at_minus_inf(name):
    r = job(name)
    d, n, nshards, nburn, nsamp, pl, poison, lik = N.MURRAY_JOBS[name]
    print(name, "Murray steps", r["remote_steps"], "passes", r["remote_passes"])
    assert r["status"] == 0 and r["remote_steps"][0] >= 5
    start_ly = O.vl_eval(O.VL_ROSENBROCK1, d, N.murray_pinit(name))
    assert (start_ly[list(poison)] == -np.inf).all()
    assert np.isfinite(r["loglike"][0][list(poison)]).all(), "a chain was left at -inf"
    for what in ("mean", "var", "musigall", "state"):
        assert not np.isnan(r[what]).any(), what


def test_box_prior_with_murray_steps_ends():
    r = job("box_pl08")
    print("Murray steps", r["remote_steps"], "passes", r["remote_passes"], "rows at -inf", int((r["samples"][0][:, -1] == -np.inf).sum()))
    assert r["status"] == 0 and r["remote_steps"][0] >= 5 and r["remote_passes"][0] >= r["remote_steps"][0]
    assert not np.isnan(r["samples"]).any() and not np.isnan(r["musigall"]).any()


@pytest.mark.parametrize("name", ["nan_16d", "inf_16d", "nan_sharded"])
def test_nan_moments_end_the_first_murray_step(name):
    r = job(name)
    d, n, nshards, nburn, nsamp, pl, poison, lik = N.MURRAY_JOBS[name]
    isamp, t = N.first_murray_step(name)
    (chain,) = poison
    assert r["status"] == O.ERR_NONFINITE
    for msg in r["error"].split("|"):   # every shard: the same step, the same chain
        assert "step %d:" % t in msg and "global chain %d " % chain in msg, r["error"]
    assert list(r["remote_steps"]) == [0] * nshards
    # what the run computed before that step is kept: the rows of isamp steps, the state those rows end in
    for s in range(nshards):
        rows = r["samples"][s].reshape(-1, n, d + 1)
        assert rows.shape[0] == isamp
        N.assert_same(r["state"][s], rows[-1][:, :d], "state")
        N.assert_same(r["loglike"][s], rows[-1][:, d], "loglike")
        assert np.isnan(r["musigall"][s][chain]).any()


def test_the_lowered_cap():
    r = job("healthy_2d")
    most = int(r["remote_passes_max"][0])
    assert r["status"] == 0 and most >= 2
    low = job("healthy_2d", 1)
    assert low["status"] == O.ERR_NONFINITE and "after 1 passes" in low["error"], low["error"]
    # one pass fewer than the longest call needs: the run ends at that call; exactly as many: the bits of today
    short = job("healthy_2d", most - 1)
    assert short["status"] == O.ERR_NONFINITE and "after %d passes" % (most - 1) in short["error"]
    for cap in (most, 1000000):
        same = job("healthy_2d", cap)
        assert same["status"] == 0
        for what in ("state", "loglike", "mean", "var", "musigall", "samples", "accept_mask", "remote_passes", "remote_steps"):
            assert np.array_equal(same[what].view(np.uint8), r[what].view(np.uint8)), (cap, what)
