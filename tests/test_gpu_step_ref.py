"""The float64 model of the step loop (tests/step_ref.py) against the GPU engine, through the C ABI.  The oracle is not
loaded: what passes here is pinned to the documented algorithm without it.

The hot-path kernels record no acceptance mask (mcx_run.hip fused_choice: `lanes_ok = lpc <= 8 && a.vec4 && !a.mask`, and
small_n_config's `hot_path ... && !e->opt_mask`): a run with MCX_OPT_ACCEPT_MASK goes to the generic kernels.  So the
cases that are to reach a hot-path kernel run without the mask -- the replay then follows the model's own decisions
through the burn-in and reads the main loop's acceptances off the rows (step_ref.replay_run) -- and the cases with the
mask are the generic kernels' and the unfused path's."""
import numpy as np
import pytest

import step_ref as R

pytestmark = pytest.mark.gpu

SEED = 8675309


def default_pinit(d, n):
    """pinit[g][i] = 0.5 sin(0.37 (g d + i))"""
    g = np.arange(n, dtype=np.float64)[:, None]
    i = np.arange(d, dtype=np.float64)[None, :]
    return (0.5 * np.sin(0.37 * (g * d + i))).astype(np.float32)


def spd(d, seed):
    a = np.random.default_rng(seed).normal(size=(d, d))
    return ((a @ a.T / d + np.eye(d)) * 0.04).astype(np.float32)


def mix_params(d, K):
    means = np.zeros((K, d), np.float32)
    for k in range(K):
        means[k, :] = 5.0 * k / max(K - 1, 1)
    w = np.ones(K, np.float32)
    w[0] = 5.0
    return np.concatenate([means.ravel(), w])


# name: (kind, d, n, nburn, nsamp, pl, SYNCSTEP, ncomp, full covariance, mask, options, what must have run)
# SYNCSTEP 40 where there are Murray steps: see tests/test_step_ref_cpu.py.  Shapes: the smallest the existing tests
# document as reaching each kernel family (test_gpu_run_parity.py, test_gpu_blocks_per_lane.py, test_gpu_configs.py).
PERSIST_OFF = {"OPT_PERSIST": 0, "OPT_SPLIT_RNG": 0}
CASES = {
    # d = 6 is no multiple of 4 (vec4 false) and the mask is on: k_fused_generic
    "generic_6d": (R.VL_ROSENBROCK1, 6, 100, 110, 100, 0.8, 40, 0, False, True, {}, "generic"),
    # the one-launch small-n kernel, Murray steps between its launches
    "small_n_16d": (R.VL_ROSENBROCK1, 16, 512, 110, 100, 0.85, 40, 0, False, False, {"OPT_PERSIST": 1}, "small"),
    # 20 000 x 16-D with the small-n modes off: fused_choice returns FUSED_HOT, one block per lane (k_fused_fast)
    "hot_16d": (R.VL_ROSENBROCK1, 16, 20000, 60, 30, 1.0, 10, 0, False, False, PERSIST_OFF, "segments"),
    # 8 lanes per chain, a chain count that fills no wavefront
    "hot_32d_257": (R.VL_ROSENBROCK1, 32, 257, 110, 40, 1.0, 10, 0, False, False, PERSIST_OFF, "segments"),
    # the random numbers from a generator kernel (FUSED_SPLIT: k_fused_fast_pregen)
    "pregen_16d": (R.VL_ROSENBROCK1, 16, 333, 110, 100, 0.9, 40, 0, False, False, {"OPT_PERSIST": 0, "OPT_SPLIT_RNG": 1}, "segments"),
    # np > 32: 16 lanes per chain, the Murray kernels with the chain vector in memory
    "generic_36d": (R.VL_ROSENBROCK1, 36, 50, 60, 40, 1.0, 10, 0, False, True, {}, "generic"),
    "generic_64d_murray": (R.VL_ROSENBROCK1, 64, 100, 110, 100, 0.8, 40, 0, False, True, {}, "generic"),
    # full covariance: FUSED_HOT_FULLCOV, one block per lane at d = 8, the mirrored kernel at 32-D (lpc == 8)
    "fullcov_8d": (R.VL_ROSENBROCK1, 8, 128, 110, 100, 0.8, 40, 0, True, False, {}, "segments"),
    "fullcov_32d_mirrored": (R.VL_ROSENBROCK1, 32, 128, 110, 100, 0.8, 40, 0, True, False, {}, "segments"),
    # the mixture of C5's shape: FUSED_HOT with two blocks per lane by itself (LIK_MIX && lpc == 8)
    "mixture_32d": (R.VL_GAUSSMIX, 32, 128, 110, 100, 0.8, 40, 8, False, False, PERSIST_OFF, "segments"),
    "gauss_33d": (R.VL_GAUSSIAN, 33, 120, 110, 100, 0.8, 40, 0, False, True, {}, "generic"),
    "rosen2fixed_16d": (R.VL_ROSENBROCK2_FIXED, 16, 100, 110, 100, 0.8, 40, 0, False, False, {}, "segments"),
    # Rosenbrock2 as written reads across the chain boundary: not fusable (mcx_run.hip `r.fused = e->opt_fuse && e->lik.fusable()`)
    "rosen2_6d": (R.VL_ROSENBROCK2, 6, 32, 60, 30, 1.0, 10, 0, False, True, {}, "unfused"),
    "dualgauss": (R.VL_DUALGAUSS, 2, 128, 60, 100, 0.8, 40, 0, False, True, {}, "generic"),
    # propose / eval / accept as kernels of their own
    "unfused_16d": (R.VL_ROSENBROCK1, 16, 300, 110, 60, 0.9, 10, 0, False, True, {"OPT_FUSE": 0}, "unfused"),
    # k_fused_fastb, two blocks per lane by option
    "two_blocks_per_lane_16d": (R.VL_ROSENBROCK1, 16, 3000, 110, 40, 1.0, 10, 0, False, False,
                                dict(PERSIST_OFF, OPT_BLOCKS_PER_LANE=2), "segments"),
}


def params_of(kind, d, ncomp):
    if kind == R.VL_GAUSSIAN:
        return np.concatenate([np.linspace(-2, 2, d), np.linspace(0.25, 4, d)]).astype(np.float32)
    if kind == R.VL_DUALGAUSS:
        return np.array([5.0], np.float32)
    if kind == R.VL_GAUSSMIX:
        return mix_params(d, ncomp)
    return None


@pytest.mark.parametrize("name", sorted(CASES))
def test_replay_of_a_gpu_run(name):
    import mcpar_amd as M
    from mcpar_amd import engine as E
    kind, d, n, nburn, nsamp, pl, sync, ncomp, full, mask, opts, ran = CASES[name]
    params = params_of(kind, d, ncomp)
    incov = spd(d, 5) if full else None
    pinit = default_pinit(d, n)
    vg, keep = M.make_vlfunc(kind, d, params, ncomp)
    eg = M.Engine(d, n, pl=pl, sync=sync, seed=SEED)
    chol0 = np.eye(d, dtype=np.float32)
    if full:
        chol0 = eg.covar_setup(incov)
        back, fwd = R.cholesky_check(incov, chol0)
        print("Cholesky: backward %.3g, forward %.3g of their bounds" % (back, fwd))
        assert back <= 1.0 and fwd <= 1.0
    eg.set_option(E.OPT_ACCEPT_MASK, int(mask))
    eg.set_option(E.OPT_PROFILE, int(ran != "small"))   # (the one-launch kernel says so in the counters)
    for k, v in opts.items():
        eg.set_option(getattr(E, k), v)
    eg.run(nsamp, nburn, pinit, vg, incov)
    c, prof = eg.counters, eg.profile
    launches = {k: v["launches"] for k, v in prof.items() if v["launches"]}
    print(name, "launches", launches, "small_n_launches", c["small_n_launches"])
    if ran == "small":
        assert c["small_n_launches"] >= 1
    elif ran == "unfused":
        assert c["small_n_launches"] == 0 and launches.get("propose", 0) >= 1 and "fused_burn" not in launches and "fused_main" not in launches
    else:   # per-segment fused kernels; which of them: the line of fused_choice cited at the case
        assert c["small_n_launches"] == 0 and launches.get("fused_burn", 0) >= 1 and "propose" not in launches
        if "OPT_SPLIT_RNG" in opts:
            assert (launches.get("gen_normals", 0) >= 1) == bool(opts["OPT_SPLIT_RNG"])
    cfg = R.Config(d, n, nburn, nsamp, R.Likelihood(kind, d, params, ncomp), pinit, chol0, pl=pl, sync=sync, seed=SEED)
    rec = R.record_of(eg, c["remote_steps"], c["remote_passes"], c["naccept_burn"], c["naccept_main"], mask=mask)
    st = R.replay_run(cfg, rec)
    R.check_caps(st, name)
    if pl < 1.0:
        assert st["murray_steps"] > 0 and c["naccept_main"] > 0
    eg.close()


# tests/test_gpu_ops.py's shapes
@pytest.mark.parametrize("d,n", [(2, 5), (8, 1000), (16, 4097), (12, 130), (32, 64), (50, 37), (256, 11)])
def test_gen_local(d, n):
    import mcpar_amd as M
    x = np.random.default_rng(d).normal(size=(n, d)).astype(np.float32)
    eg = M.Engine(d, n, nshards=2, shard=1, seed=SEED)   # global chains n .. 2 n - 1 in the counters
    for incov in (None, spd(d, 3)):
        chol = eg.covar_setup(incov)
        for t in (0, 7, 123456):
            pt, cf = eg.gen_local(t, x)
            exc = R.check_gen_local(SEED, t, n + np.arange(n), x, chol, pt, cf)
    print("largest excess %.3g" % exc)


@pytest.mark.parametrize("d,n,nshards", [(2, 64, 1), (16, 300, 1), (8, 96, 3), (5, 40, 1), (32, 33, 2), (33, 40, 1), (48, 70, 1), (64, 65, 2),
                                         (65, 30, 1), (80, 24, 2), (32, 513, 1), (32, 1030, 2), (16, 700, 1), (4, 520, 1)])
def test_gen_remote(d, n, nshards):
    import mcpar_amd as M
    rng = np.random.default_rng(10 * d + nshards)
    N = n * nshards
    ms = np.empty((N, d, 2), np.float32)
    ms[:, :, 0] = rng.normal(0, 1.0, (N, d))
    ms[:, :, 1] = rng.uniform(0.05, 0.6, (N, d))
    x = rng.normal(0, 1.0, (n, d)).astype(np.float32)
    shard = nshards - 1
    eg = M.Engine(d, n, nshards=nshards, shard=shard, seed=SEED)
    out = eg.gen_remote(42, x, ms)
    R.check_gen_remote(SEED, 42, shard * n + np.arange(n), N, x, ms, out)
