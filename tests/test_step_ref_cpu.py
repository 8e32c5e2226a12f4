"""The float64 model of the step loop (tests/step_ref.py) against the CPU oracle: known answers of the model's own
generator, teacher-forced replays of whole oracle runs, and the two single-step entry points.  The model shares no
code or arithmetic with the oracle, so what they agree on is pinned to the documented algorithm."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import step_ref as R

SEED = 8675309


def test_philox_known_answers_of_the_model():
    # Random123 kat_vectors for philox4x32-10, through the model's vectorised generator
    kat = (([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]))
    for ctr, key, out in kat:
        assert [int(v) for v in R.philox4x32(*ctr, *key)] == out
    # and as arrays: every lane its own counter
    w = R.philox4x32(np.array([0, 0xffffffff, 0x243f6a88]), np.array([0, 0xffffffff, 0x85a308d3]), np.array([0, 0xffffffff, 0x13198a2e]),
                     np.array([0, 0xffffffff, 0x03707344]), 0, 0)
    assert int(w[0][0]) == 0x6627e8d5 and int(w[3][0]) == 0x9b00dbd8


def test_uniforms_and_mulhi():
    w = np.array([0, 1, 255, 256, 0x80000000, 0xffffff7f, 0xffffff80, 0xffffffff], np.uint64)
    L = O.lib()
    assert np.array_equal(R.u24(w), [float(L.mcxo_u24(int(v))) for v in w])
    assert np.array_equal(R.uopen(w), [float(L.mcxo_uopen(int(v))) for v in w])   # an fp32 value by contract
    assert R.uopen(w).min() > 0 and R.uopen(w).max() == 1.0 and R.u24(w).max() < 1.0
    assert list(R.mulhi(np.array([0, 0xffffffff, 0x80000000], np.uint64), 300)) == [0, 299, 150]


def test_normal_distance_constant():
    """the measured constant of step_ref.NORMAL_DIST: 200 000 blocks of the oracle's normals lie within the 4 x bound of the
    model's, and not absurdly far inside it (the measurement is of this quantity)"""
    L = O.lib()
    n = 200000
    z, zo = np.zeros(4, np.float32), np.empty((n, 4), np.float32)
    for i in range(n):
        L.mcxo_normal4(SEED, 4, 99, i, 3, 7, O.fptr(z))
        zo[i] = z
    zm = R.normals_from_words(R.philox4x32(99, np.arange(n), 3, 7, SEED, 4))
    dist = (np.abs(zo - zm) / np.maximum(1.0, np.abs(zm))).max()
    print("largest distance %.3g of %.3g allowed" % (dist, R.NORMAL_DIST))
    assert R.NORMAL_DIST == 4 * R.NORMAL_DIST_MEASURED
    assert R.NORMAL_DIST / 16 < dist <= R.NORMAL_DIST


def oracle_chol(d, incov):
    a = np.eye(d, dtype=np.float32) if incov is None else np.ascontiguousarray(incov, np.float32).copy()
    assert O.lib().mcxo_cholesky(d, O.fptr(a)) == 0
    return a


def spd(d, seed):
    a = np.random.default_rng(seed).normal(size=(d, d))
    return ((a @ a.T / d + np.eye(d)) * 0.04).astype(np.float32)


def gauss_params(d):
    return np.concatenate([np.linspace(-2, 2, d), np.linspace(0.25, 4, d)]).astype(np.float32)


def mix_params(d, K, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.normal(0, 1.5, K * d), rng.uniform(0.5, 3.0, K)]).astype(np.float32)


# name: (kind, d, n, nburn, nsamp, pl, params, ncomp, full covariance, SYNCSTEP)
# SYNCSTEP: a chain that has not moved since the moments started has sigma^2 = 1e-14 / pwgt, and a trial drawn from it is
# mu + 1e-7 z, which fp32 rounds to mu or its neighbour: arg = ulp^2 / sigma^2 is 0 or ~1e2, rounding alone decides, and no
# float64 model can say which.  With the reference's default of 10 the first Murray steps meet such chains wherever the
# acceptance rate is low (2-D Rosenbrock: 42 % of the chains of a step undecided), so most cases start their Murray steps
# at step 40, when every chain has moved; two keep the default.  n >= 100 where there are Murray steps, so that the cap of
# 2 % of a step's chains is not one chain.
RUNS = {
    "rosen1_8d_pl1": (O.VL_ROSENBROCK1, 8, 256, 160, 60, 1.0, None, 0, False, 10),
    "rosen1_16d": (O.VL_ROSENBROCK1, 16, 300, 120, 60, 0.8, None, 0, False, 10),
    "rosen1_30d_pl1": (O.VL_ROSENBROCK1, 30, 19, 120, 40, 1.0, None, 0, False, 10),
    "rosen1_30d": (O.VL_ROSENBROCK1, 30, 100, 110, 100, 0.8, None, 0, False, 40),
    "rosen1_8d_fullcov": (O.VL_ROSENBROCK1, 8, 128, 110, 100, 0.8, None, 0, True, 40),
    "rosen1_2d": (O.VL_ROSENBROCK1, 2, 200, 110, 100, 0.8, None, 0, False, 40),
    "gauss_5d": (O.VL_GAUSSIAN, 5, 100, 110, 100, 0.8, gauss_params(5), 0, False, 40),
    "gauss_33d": (O.VL_GAUSSIAN, 33, 120, 110, 100, 0.8, gauss_params(33), 0, False, 40),
    "gauss_68d": (O.VL_GAUSSIAN, 68, 100, 110, 100, 0.8, gauss_params(68), 0, False, 40),
    "dualgauss": (O.VL_DUALGAUSS, 2, 128, 60, 100, 0.8, np.array([5.0], np.float32), 0, False, 40),
    "mixture_16d": (O.VL_GAUSSMIX, 16, 100, 110, 60, 0.8, mix_params(16, 3, 1), 3, False, 10),
    "rosen2fixed_16d": (O.VL_ROSENBROCK2_FIXED, 16, 100, 110, 100, 0.8, None, 0, False, 40),
    "rosen2_6d_pl1": (O.VL_ROSENBROCK2, 6, 32, 60, 30, 1.0, None, 0, False, 10),
}


def oracle_run(kind, d, n, nburn, nsamp, pl, params, ncomp, full, sync):
    incov = spd(d, 5) if full else None
    vo, keep = O.make_vlfunc(kind, d, params, ncomp)
    eo = O.Engine(d, n, pl=pl, sync=sync, threads=4)
    eo.set_record(samples=True, mask=True, stride=1)
    pinit = O.default_pinit(d, n)
    eo.run(nsamp, nburn, pinit, vo, incov)
    chol0 = oracle_chol(d, incov)
    if full:
        back, fwd = R.cholesky_check(incov, chol0)
        print("Cholesky: backward %.3g, forward %.3g of their bounds" % (back, fwd))
        assert back <= 1.0 and fwd <= 1.0
    cfg = R.Config(d, n, nburn, nsamp, R.Likelihood(kind, d, params, ncomp), pinit, chol0, pl=pl, sync=sync, seed=SEED)
    rec = R.record_of(eo, eo.remote_steps, eo.remote_passes, eo.naccept_burn, eo.naccept_main)
    return cfg, rec


@pytest.mark.parametrize("name", sorted(RUNS))
def test_replay_of_an_oracle_run(name):
    cfg, rec = oracle_run(*RUNS[name])
    st = R.replay_run(cfg, rec)
    R.check_caps(st, name)
    if RUNS[name][5] < 1.0:
        assert st["murray_steps"] > 0 and rec["naccept_main"] > 0


def test_replay_without_the_mask():
    """the replay the GPU's hot-path kernels get (they record no mask): burn-in by the model's own decisions, main-loop
    acceptances read off the rows"""
    cfg, rec = oracle_run(*RUNS["rosen1_16d"])
    rec["mask"] = None
    st = R.replay_run(cfg, rec)
    R.check_caps(st, "no mask")
    assert st["murray_steps"] > 0


@pytest.mark.parametrize("d,n,full", [(2, 5, False), (8, 300, True), (33, 40, False), (68, 11, True)])
def test_gen_local_of_the_oracle(d, n, full):
    x = np.random.default_rng(d).normal(size=(n, d)).astype(np.float32)
    shard = 0 if full else 1   # (shard 1 of 2: global chains n .. 2 n - 1 in the counters)
    eo = O.Engine(d, n, nshards=1 + shard, shard=shard)
    if full:   # the oracle installs a factor only in a run: a run of no steps does it
        vo, keep = O.make_vlfunc(O.VL_GAUSSIAN, d)
        eo.run(0, 0, x, vo, spd(d, 3))
    for t in (0, 7, 123456):
        pt, cf = eo.gen_local(t, x)
        exc = R.check_gen_local(SEED, t, shard * n + np.arange(n), x, eo.chol, pt, cf)
    print("largest excess %.3g" % exc)


# test_gpu_ops.py::test_gen_remote's shapes and inputs: (4, 520, 1) is the many-pass one, (32, 33, 2) and (80, 24, 2) run as
# shard 1 of 2 (the global chain id in the counters), d = 65 and 80 put Q at the FPEPS seeds of qisum / qimax
@pytest.mark.parametrize("d,n,nshards", [(2, 64, 1), (16, 300, 1), (5, 40, 1), (32, 33, 2), (33, 40, 1), (65, 30, 1), (80, 24, 2), (4, 520, 1)])
def test_gen_remote_of_the_oracle(d, n, nshards):
    rng = np.random.default_rng(10 * d + nshards)
    N = n * nshards
    ms = np.empty((N, d, 2), np.float32)
    ms[:, :, 0] = rng.normal(0, 1.0, (N, d))
    ms[:, :, 1] = rng.uniform(0.05, 0.6, (N, d))
    x = rng.normal(0, 1.0, (n, d)).astype(np.float32)
    shard = nshards - 1
    eo = O.Engine(d, n, nshards=nshards, shard=shard, threads=4)
    out = eo.gen_remote(42, x, ms)
    R.check_gen_remote(SEED, 42, shard * n + np.arange(n), N, x, ms, out)
