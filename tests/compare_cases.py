"""The stores the compare tests share (tests/test_compare_cpu.py, tests/test_gpu_compare*.py): rows in MCout layout [T * nc, np + 1]."""
import numpy as np

NAN, INF = float("nan"), float("inf")
TILE = 8192  # keys per sort and sweep tile (mcx_debug_compare_geometry's tile_keys)


def tie_rows(np_, nc, T, seed, stay=0.35, shift=0.0):
    """tests/test_gpu_scratch_history.py's make_rows with every value rounded to eighths: normal rows, log L below zero, with
    probability `stay` a chain's row repeats the step before.  Many ties inside a store and many values shared by two"""
    rng = np.random.default_rng([seed, np_, nc, T])
    a = rng.normal(shift, 1.0, (T, nc, np_ + 1))
    a[:, :, -1] = -np.abs(a[:, :, -1]) - 0.125
    a = (np.round(a * 8.0) / 8.0).astype(np.float32)
    for t in range(1, T):
        rep = rng.random(nc) < stay
        a[t, rep] = a[t - 1, rep]
    return a.reshape(T * nc, np_ + 1)


def normal_rows(np_, nc, T, seed, scale0=1.0):
    """iid standard normal values in every column (column 0 times scale0)"""
    rng = np.random.default_rng([seed, np_, nc, T])
    a = rng.normal(0.0, 1.0, (T * nc, np_ + 1))
    a[:, 0] *= scale0
    return a.astype(np.float32)


# a statement with content: two stores of 4 iid normal chains x 1000 steps, and B's column 0 scaled by 1.5
CONTENT = dict(np_=3, nc=4, T=1000, seed_a=11, seed_b=12)


def content_rows():
    c = CONTENT
    return (normal_rows(c["np_"], c["nc"], c["T"], c["seed_a"]), normal_rows(c["np_"], c["nc"], c["T"], c["seed_b"]),
            normal_rows(c["np_"], c["nc"], c["T"], c["seed_b"], scale0=1.5))


def check_content(same, scaled):
    """same: the dict of A against B; scaled: of A against B with column 0 times 1.5"""
    assert (same["ks_p"] > 0.01).all(), same["ks_p"]
    assert scaled["ks_p"][0] < 1e-6 and abs(scaled["z_mean"][0]) < 4, (scaled["ks_p"][0], scaled["z_mean"][0])
    assert (scaled["ks_p"][1:] > 0.01).all()


def straddle(N, value, first, count, rng, lo, hi):
    """N float32 values: `count` copies of `value` at sorted positions [first, first + count), distinct values of (lo, value)
    below them and of (value, hi) above, shuffled"""
    below = rng.uniform(lo, value - 1e-3, first)
    above = rng.uniform(value + 1e-3, hi, N - first - count)
    x = np.concatenate([below, np.full(count, value), above]).astype(np.float32)
    srt = np.sort(x)
    assert srt[first] == np.float32(value) == srt[first + count - 1] and (first == 0 or srt[first - 1] < np.float32(value))
    assert first + count == N or srt[first + count] > np.float32(value)
    return rng.permutation(x)


def one_col_rows(x, rng):
    """np = 1: the column x and a log L column of its own values in another order"""
    return np.stack([x, -np.abs(rng.permutation(x)) - 1.0], axis=1).astype(np.float32)
