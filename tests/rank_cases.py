"""Inputs the rank-summary tests share (tests/test_rank_summary_cpu.py, tests/test_gpu_rank_summary.py): the two
demonstration cases that basic R-hat / ESS call converged, and rows built from columns."""
import numpy as np

DEMO_T, DEMO_NC = 1000, 4
SCALE_SEED, CAUCHY_SEED = 12, 14  # chosen on the float64 reference: every threshold below holds with room to spare


def demo_scale(seed=SCALE_SEED):
    """four iid normal chains, one with 3 x the scale: x [T, nc] float32"""
    x = np.random.default_rng(seed).standard_normal((DEMO_T, DEMO_NC))
    x[:, 3] *= 3.0
    return x.astype(np.float32)


def demo_cauchy(seed=CAUCHY_SEED):
    """four Cauchy chains, one shifted by 1: x [T, nc] float32"""
    x = np.random.default_rng(seed).standard_cauchy((DEMO_T, DEMO_NC))
    x[:, 3] += 1.0
    return x.astype(np.float32)


def check_demo_scale(basic_rhat, basic_ess, rhat_folded, ess_tail):
    assert basic_rhat <= 1.01, basic_rhat
    assert rhat_folded >= 1.05, rhat_folded
    assert ess_tail < basic_ess / 20, (ess_tail, basic_ess)


def check_demo_cauchy(basic_rhat, basic_ess, ess_bulk):
    assert basic_rhat <= 1.01, basic_rhat
    assert ess_bulk < basic_ess / 10, (ess_bulk, basic_ess)


KINDS = ["equal", "two", "top-byte", "low-byte", "zeros", "mh", "ascending", "descending", "normal"]


def content(kind, T, nc, rng):
    """one column [T, nc] float32 of the contents where a radix sort and a scatter break"""
    N = T * nc
    if kind == "equal":
        return np.full((T, nc), 1.5, np.float32)
    if kind == "two":
        return rng.choice(np.array([-2.0, 3.0], np.float32), (T, nc))
    if kind == "top-byte":  # +-2^(16 j): the keys differ in their top byte only
        return (rng.choice([-1.0, 1.0], (T, nc)) * 2.0 ** (16 * rng.integers(-3, 4, (T, nc)))).astype(np.float32)
    if kind == "low-byte":  # consecutive floats: the keys differ in their lowest byte only
        return (np.float32(1.0).view(np.uint32) + rng.integers(0, 200, (T, nc)).astype(np.uint32)).view(np.float32)
    if kind == "zeros":
        return rng.choice(np.array([-0.0, 0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, -3e-39], np.float32), (T, nc))
    if kind == "mh":  # every value repeats its predecessor in the chain with probability 0.7
        x = rng.standard_normal((T, nc)).astype(np.float32)
        keep = rng.random((T, nc)) < 0.7
        for s in range(1, T):
            x[s] = np.where(keep[s], x[s - 1], x[s])
        return x
    if kind == "ascending":
        return (np.arange(N, dtype=np.float32) - np.float32(N // 3)).reshape(T, nc)
    if kind == "descending":
        return (np.float32(N // 3) - np.arange(N, dtype=np.float32) * np.float32(0.5)).reshape(T, nc)
    return rng.standard_normal((T, nc)).astype(np.float32)


def repeats(T, nc, rng, p):
    """src [T, nc]: the step whose fresh value step s of a chain holds when every step but the first repeats its
    predecessor with probability p -- the "mh" kind without a loop over the steps, for millions of them"""
    fresh = rng.random((T, nc)) >= p
    fresh[0] = True
    return np.maximum.accumulate(np.where(fresh, np.arange(T)[:, None], 0), axis=0)


BIG_SHAPE = (1, 2, 2101267)  # np, nc, T: 514 sort tiles (three steps of 256 in k_rank_scan), 65 steps per workgroup


def big_columns():
    """the two columns [T, nc] of BIG_SHAPE: normals, and log-L-like negatives, in both of which a step repeats its
    predecessor (the whole row, as a rejected Metropolis step does) with probability 0.3"""
    _, nc, T = BIG_SHAPE
    rng = np.random.default_rng(20211)
    src, chains = repeats(T, nc, rng, 0.3), np.arange(nc)
    x = rng.standard_normal((T, nc), np.float32)[src, chains]
    ll = (np.float32(-2.0) * rng.standard_exponential((T, nc), np.float32) - np.float32(1e-3))[src, chains]
    return [x, ll]


def rows_of(cols):
    """columns [T, nc] -> rows [T * nc, ncol] float32 (MCout layout)"""
    x = np.stack([np.asarray(c, np.float32) for c in cols], axis=2)
    T, nc, ncol = x.shape
    return np.ascontiguousarray(x.reshape(T * nc, ncol))
