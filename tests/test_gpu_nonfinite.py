"""Chains that start at log L = -inf or NaN, or with an infinite or NaN coordinate, through every family of step kernels and
through the Murray kernels ("Non-finite values").  The contract: the oracle's bits on everything
finite, its NaN / -inf class elsewhere (x86 and gfx950 produce different default NaNs), and every integer counter.
Cases and the oracle-free replay of the semantics: tests/nonfinite_cases.py; the oracle alone: tests/test_nonfinite_cpu.py.

A Murray case with non-finite values runs here only after the oracle has ended on exactly that case, in a child process
under a time limit: before the loop of a Murray call was bounded a NaN moment kept both from ever returning."""
import functools

import numpy as np
import pytest

import nonfinite_cases as N

pytestmark = pytest.mark.gpu


def gpu_engine(c, pl=1.0, seed=N.SEED, mask=None, profile=None):
    import mcpar_amd as M
    from mcpar_amd import engine as E
    eg = M.Engine(c["d"], c["n"], pl=pl, sync=c["sync"], seed=seed)
    eg.set_option(E.OPT_ACCEPT_MASK, int(c["mask"] if mask is None else mask))
    eg.set_option(E.OPT_PROFILE, int(c["ran"] != "small") if profile is None else profile)   # (the one-launch kernel says so in the counters)
    for k, v in c["opts"].items():
        eg.set_option(getattr(E, k), v)
    return eg


def assert_family(c, eg, nburn):
    """which kernels ran: tests/test_gpu_step_ref.py's assertions (a run without burn-in has no burn-in launch to show)"""
    cnt, prof = eg.counters, eg.profile
    launches = {k: v["launches"] for k, v in prof.items() if v["launches"]}
    print(c["name"], "launches", launches, "small_n_launches", cnt["small_n_launches"])
    if c["ran"] == "small":
        assert cnt["small_n_launches"] >= 1
    elif c["ran"] == "unfused":
        assert cnt["small_n_launches"] == 0 and launches.get("propose", 0) >= 1 and "fused_burn" not in launches and "fused_main" not in launches
    else:
        assert cnt["small_n_launches"] == 0 and launches.get("fused_burn" if nburn else "fused_main", 0) >= 1 and "propose" not in launches
        if "OPT_SPLIT_RNG" in c["opts"]:
            assert (launches.get("gen_normals", 0) >= 1) == bool(c["opts"]["OPT_SPLIT_RNG"])


def gpu_run(c, pinit, nburn, nsamp):
    import mcpar_amd as M
    vg, keep = M.make_vlfunc(c["kind"], c["d"], c["params"], c["ncomp"])
    eg = gpu_engine(c)
    eg.run(nsamp, nburn, pinit, vg, c["incov"])
    assert_family(c, eg, nburn)
    return eg


def assert_equals_oracle(eg, o, what, mask, shard=0):
    """o: a job of nonfinite_cases.run_oracle_job, or an oracle engine"""
    get = (lambda k: o[k][shard]) if isinstance(o, dict) else (lambda k: getattr(o, k))
    c = eg.counters
    assert (c["naccept_burn"], c["naccept_main"]) == (int(get("naccept_burn")), int(get("naccept_main"))), what
    assert (c["remote_steps"], c["remote_passes"]) == (int(get("remote_steps")), int(get("remote_passes"))), what
    assert np.array_equal(eg.accept_counts, get("accept_counts")), what
    if mask:
        bad = np.argwhere(eg.accept_mask != get("accept_mask"))
        assert bad.size == 0, "%s: accept mask differs first at (step, chain) %s" % (what, bad[:3].tolist())
    assert np.array_equal(N.bits(eg.tuner_trace), N.bits(get("tuner_trace"))), what
    for name in ("state", "loglike", "mean", "var", "musigall", "samples"):
        N.assert_same(getattr(eg, name), get(name), "%s %s" % (what, name))


@pytest.mark.parametrize("name", N.FAMILIES)
def test_every_family_equals_the_oracle(name):
    """with the burn-in, so that the tuner counts the poisoned chains' rejections; pl = 1"""
    import oracle_lib as O
    c = N.poisoned_start(name)
    vo, keep = O.make_vlfunc(c["kind"], c["d"], c["params"], c["ncomp"])
    eo = O.Engine(c["d"], c["n"], pl=1.0, sync=c["sync"], threads=8)
    eo.run(c["nsamp"], c["nburn"], c["pinit"], vo, c["incov"])
    eg = gpu_run(c, c["pinit"], c["nburn"], c["nsamp"])
    assert_equals_oracle(eg, eo, name, c["mask"])
    stuck = c["poisoned"][~np.isfinite(eo.loglike[c["poisoned"]])]
    assert stuck.size >= 6 and not eg.accept_counts[stuck].any()
    eg.close(); eo.close()


@pytest.mark.parametrize("name", N.FAMILIES)
def test_semantics_and_isolation_without_the_oracle(name):
    """nburn = 0, pl = 1: the three rules replayed from the rows (the engine's own genLocal and likelihood give the
    proposals), the healthy chains bit for bit what they are in a run without the poisoned ones"""
    import mcpar_amd as M
    c = N.poisoned_start(name)
    nsamp = min(c["nsamp"], 40)
    eg = gpu_run(c, c["pinit"], 0, nsamp)
    ec = gpu_run(c, c["clean"], 0, nsamp)
    ll = lambda x: M.vlfunc_eval(c["kind"], c["d"], x, c["params"], c["ncomp"])   # noqa: E731
    start = N.row_of_start(c["pinit"], ll(c["pinit"]))
    rows = eg.samples.reshape(nsamp, c["n"], -1)
    clean = ec.samples.reshape(nsamp, c["n"], -1)
    seen = N.check_semantics(start, rows, eg.accept_mask if c["mask"] else None, lambda t, x: eg.gen_local(t, x)[0], ll, name)
    print(name, seen)
    assert seen["nan_stays"] >= 2 * nsamp and seen["minf_stays"] >= nsamp
    h, p = c["healthy"], c["poisoned"]
    assert np.isfinite(clean).all()
    assert np.array_equal(N.bits(rows[:, h]), N.bits(clean[:, h]))
    for what in ("state", "loglike", "mean", "var"):
        assert np.array_equal(N.bits(getattr(eg, what)[h]), N.bits(getattr(ec, what)[h])), what
    assert np.array_equal(eg.accept_counts[h], ec.accept_counts[h])
    for t in range(nsamp):
        N.assert_same(rows[t, p], start[p], "%s step %d" % (name, t))
    stuck = p[~np.isfinite(start[p, -1])]
    assert not eg.accept_counts[stuck].any()
    cg, cc = eg.counters, ec.counters
    assert cg["naccept_main"] - int(eg.accept_counts[p].sum()) == cc["naccept_main"] - int(ec.accept_counts[p].sum())
    eg.close(); ec.close()


ZERO_DRAW_OPTS = {"one_launch": ({}, 0), "hot": (N.CASES["hot_16d"][10], 0), "generic": ({}, 1), "unfused": ({"OPT_FUSE": 0}, 1)}


@pytest.mark.parametrize("path", sorted(ZERO_DRAW_OPTS))
def test_a_zero_draw_takes_any_finite_proposal(path):
    """u24 = 0: log1(u24) = -inf (the kernels' integer range reduction has no exponent to reduce there).  Proposals of
    scale 10 on Rosenbrock1 drop log L by millions: the chain whose draw is 0 takes its own, no other chain does."""
    import mcpar_amd as M
    d, n, j = 16, 128, N.U0_CHAIN
    assert N.u0_draw_is_zero()
    opts, mask = ZERO_DRAW_OPTS[path]
    c = dict(name=path, d=d, n=n, sync=10, mask=mask, opts=opts, ran="", kind=M.VL_ROSENBROCK1, params=None, ncomp=0)
    incov = (100.0 * np.eye(d)).astype(np.float32)
    pinit = N.default_pinit(d, n)
    vg, keep = M.make_vlfunc(M.VL_ROSENBROCK1, d)
    eg = gpu_engine(c, seed=N.U0_SEED, profile=0)
    eg.run(1, 0, pinit, vg, incov)
    ll = lambda x: M.vlfunc_eval(M.VL_ROSENBROCK1, d, x)   # noqa: E731
    xp = eg.gen_local(0, pinit)[0]
    drop = ll(xp) - ll(pinit)
    others = np.arange(n) != j
    u = N.R.accept_u(N.U0_SEED, 0, np.arange(n))
    assert np.isfinite(drop).all() and drop[j] < -1000.0 and u[j] == 0.0 and (np.log(u[others]) > drop[others] + 1000.0).all()
    assert eg.accept_counts[j] == 1 and eg.counters["naccept_main"] == 1
    assert np.array_equal(N.bits(eg.state[j]), N.bits(xp[j])) and np.array_equal(N.bits(eg.state[others]), N.bits(pinit[others]))
    if mask:
        assert eg.accept_mask[0, j] == 1 and eg.accept_mask.sum() == 1
    eg.close()


def test_maxlike_through_a_sink_on_a_fused_path():
    """the running maximum a sink run keeps on the device: the first maximum over the rows with ly > -inf (src/mcout.cc:140)"""
    c = N.poisoned_start("hot_32d_257")
    import mcpar_amd as M
    vg, keep = M.make_vlfunc(c["kind"], c["d"], c["params"], c["ncomp"])
    eg = gpu_engine(c)
    got = []
    eg.set_sink(lambda first, nsteps, rows: got.append(rows.copy()) and 0, 7)
    eg.run(c["nsamp"], c["nburn"], c["pinit"], vg)
    assert_family(c, eg, c["nburn"])
    rows = np.concatenate(got)
    assert rows.shape == (c["nsamp"] * c["n"], c["d"] + 1)
    ly = rows[:, -1]
    assert np.isnan(ly).any() and (ly == -np.inf).any()
    ok = ly > -np.inf
    i = int(np.argmax(np.where(ok, ly, -np.inf)))
    gl, gp = eg.maxlike()
    assert np.isfinite(gl) and np.float32(gl) == ly[i] and np.array_equal(N.bits(gp), N.bits(rows[i, :-1]))
    eg.set_sink(None, 0)
    eg.close()


# ---- the box prior: host callback, block form, whole-vector form ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def box_oracle(pl):
    r = N.oracle_job_in_child("box_pl08") if pl < 1.0 else N.run_oracle_job("box_pl1")
    assert r["status"] == 0
    return r


def box_vlfunc(form):
    import mcpar_amd as M
    if form == "host":
        return M.make_vlfunc(M.VL_HOST, N.BOX_D, host_fn=N.box_numpy)
    return M.make_vlfunc(M.VL_SOURCE, N.BOX_D, params=N.BOX_PAR, source=N.BOX_BLOCK_FORM if form == "block" else N.BOX_WHOLE_FORM)


@pytest.mark.parametrize("pl", [1.0, 0.8])
@pytest.mark.parametrize("form", ["host", "block", "whole"])
def test_box_prior_equals_the_oracle_with_the_numpy_functor(form, pl):
    import mcpar_amd as M
    from mcpar_amd import engine as E
    o = box_oracle(pl)
    vg, keep = box_vlfunc(form)
    eg = M.Engine(N.BOX_D, N.BOX_N, pl=pl)
    eg.set_option(E.OPT_ACCEPT_MASK, int(form == "host"))
    eg.run(N.BOX_NSAMP, N.BOX_NBURN, N.box_pinit(), vg)
    assert_equals_oracle(eg, o, "box %s pl=%g" % (form, pl), form == "host")
    c = eg.counters
    print(form, pl, "Murray steps", c["remote_steps"], "passes", c["remote_passes"], "rows at -inf", int((eg.samples[:, -1] == -np.inf).sum()))
    if pl < 1.0:
        assert c["remote_steps"] >= 5
    eg.close()


@pytest.mark.parametrize("form", ["host", "block"])
def test_a_zero_draw_lets_a_chain_at_minus_inf_in(form):
    import mcpar_amd as M
    d, n, j = N.BOX_D, N.BOX_N, N.U0_CHAIN
    incov = (0.01 * np.eye(d)).astype(np.float32)
    z = N.R.normals(N.U0_SEED, N.R.ST_LOCAL, 0, np.array([j]), d)[0]
    pinit = N.default_pinit(d, n)
    pinit[j] = (-0.1 * z).astype(np.float32)
    pinit[j, 0] = np.float32(-np.sign(z[0]) * (0.6 + 0.05 * abs(z[0])))
    vg, keep = box_vlfunc(form)
    eg = M.Engine(d, n, pl=1.0, seed=N.U0_SEED)
    eg.run(1, 0, pinit, vg, incov)
    xp = eg.gen_local(0, pinit)[0]
    assert N.box_numpy(pinit)[j] == -np.inf and np.isfinite(N.box_numpy(xp)[j])
    assert eg.accept_counts[j] == 1 and np.array_equal(N.bits(eg.state[j]), N.bits(xp[j]))
    eg.close()


# ---- Murray steps ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_job(name, max_passes=0):
    return N.oracle_job_in_child(name, max_passes)   # (subprocess.TimeoutExpired: the oracle did not end: nothing runs on the GPU)


def gpu_job(name, max_passes=0):
    import mcpar_amd as M
    from mcpar_amd import engine as E
    d, n, nshards, nburn, nsamp, pl, poison, lik = N.MURRAY_JOBS[name]
    vg, keep = M.make_vlfunc(M.VL_ROSENBROCK1, d)
    eg = M.Engine(d, n, pl=pl)
    eg.set_option(E.OPT_ACCEPT_MASK, 1)
    eg.set_option(E.OPT_MURRAY_MAX_PASSES, max_passes)
    err = None
    try:
        eg.run(nsamp, nburn, N.murray_pinit(name), vg)
    except M.McxError as ex:
        err = ex
    return eg, err


@pytest.mark.parametrize("name", ["minf_16d", "minf_36d"])
def test_murray_rescues_chains_at_minus_inf(name):
    o = oracle_job(name)
    assert o["status"] == 0 and o["remote_steps"][0] >= 5
    eg, err = gpu_job(name)
    assert err is None, err
    assert_equals_oracle(eg, o, name, True)
    assert np.isfinite(eg.loglike).all()
    eg.close()


def test_nan_moments_end_the_first_murray_step():
    from mcpar_amd import engine as E
    name = "nan_16d"
    o = oracle_job(name)
    assert o["status"] == E.ERR_NONFINITE
    d, n, nshards, nburn, nsamp, pl, poison, lik = N.MURRAY_JOBS[name]
    isamp, t = N.first_murray_step(name)
    eg, err = gpu_job(name)
    assert err is not None and err.code == E.ERR_NONFINITE
    print(err, "|", o["error"])
    assert "step %d:" % t in str(err) and "global chain %d " % list(poison)[0] in str(err)
    assert "step %d:" % t in o["error"]
    # the steps before it are kept: the state they ended in
    N.assert_same(eg.state, o["state"][0], "state")
    N.assert_same(eg.loglike, o["loglike"][0], "loglike")
    # and the engine is still usable
    import mcpar_amd as M
    vg, keep = M.make_vlfunc(M.VL_ROSENBROCK1, d)
    eg.run(20, 20, N.default_pinit(d, n), vg)
    assert np.isfinite(eg.samples).all()
    eg.close()


def test_the_lowered_cap():
    from mcpar_amd import engine as E
    name = "healthy_2d"
    o = oracle_job(name)
    most = int(o["remote_passes_max"][0])
    assert o["status"] == 0 and most >= 6   # (more than a turn over four candidates: the cap falls inside one)
    for cap in (1, most - 1):
        assert oracle_job(name, cap)["status"] == E.ERR_NONFINITE
        eg, err = gpu_job(name, cap)
        assert err is not None and err.code == E.ERR_NONFINITE and "after %d passes" % cap in str(err), (cap, err)
        N.assert_same(eg.state, oracle_job(name, cap)["state"][0], "state at the failed step, cap %d" % cap)
        eg.close()
    eg, err = gpu_job(name, most)
    assert err is None, err
    assert_equals_oracle(eg, o, "cap = the longest call", True)
    eg.close()


def test_two_shards_fail_at_the_same_step():
    from mcpar_amd import engine as E
    from test_gpu_multishard import run_sharded_gpu
    name = "nan_sharded"
    o = oracle_job(name)
    assert o["status"] == E.ERR_NONFINITE
    d, n, nshards, nburn, nsamp, pl, poison, lik = N.MURRAY_JOBS[name]
    isamp, t = N.first_murray_step(name)
    p = N.murray_pinit(name)
    errors = []
    engs = run_sharded_gpu(d, n, nshards, nburn, nsamp, pl, pinits=[p[s * n:(s + 1) * n] for s in range(nshards)], errors=errors)
    assert sorted(s for s, ex in errors) == [0, 1], errors
    for s, ex in errors:
        assert getattr(ex, "code", None) == E.ERR_NONFINITE, (s, ex)
        assert "step %d:" % t in str(ex) and "global chain %d " % list(poison)[0] in str(ex), ex
    for s in range(nshards):
        N.assert_same(engs[s].state, o["state"][s], "shard %d state" % s)
        engs[s].close()
