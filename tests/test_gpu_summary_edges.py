"""mcx_rows_summary and mcx_debug_rows_acov at the edges of mcx_summary.hip, against the float64 restatement of DESIGN.md
"Sample-store summaries" (tests/summary_ref.py): shapes with idle lanes and partial tiles, every lag of the autocovariance
windows, more than 32 target prefixes, several histogram step chunks, and the values where an order or a sum goes wrong
(signed zeros and NaNs, infinities, subnormals, ties, extremes, W = 0).  Every call is made twice and must give the same
bytes."""
import numpy as np
import pytest

import oracle_lib as O
import summary_ref as R

pytestmark = pytest.mark.gpu

PROBS = (0.01, 0.25, 0.5, 0.9, 0.99)
EPS = 2.0 ** -53


def same_bytes(a, b):
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def summarise(rows, T, nc, probs=PROBS):
    from mcpar_amd import engine as E
    a = E.rows_summary(rows, T, nc, probs)
    same_bytes(a, E.rows_summary(rows, T, nc, probs))
    return a


def rows_acov(rows, T, nc, nlags):
    from mcpar_amd import engine as E
    a, s = E.debug_rows_acov(rows, T, nc, nlags)
    b, t = E.debug_rows_acov(rows, T, nc, nlags)
    assert a.tobytes() == b.tobytes() and s.tobytes() == t.tobytes()
    return a, s


def series(T, nc, ncol, kind, seed, phi=0.7, offset=0.0):
    """x [T, nc, ncol] float32: iid normals, AR(1) or random walks per (chain, column), chains offset by N(0, offset)"""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((T, nc, ncol))
    if kind == "ar":
        for i in range(1, T):
            e[i] += phi * e[i - 1]
    elif kind == "rw":
        e = np.cumsum(e, axis=0)
    return (e + rng.normal(0.0, offset, (nc, ncol)) if offset else e).astype(np.float32)


def as_rows(x):
    T, nc, ncol = x.shape
    return np.ascontiguousarray(x.reshape(T * nc, ncol))


def check_rows(x, probs=PROBS):
    T, nc, _ = x.shape
    rows = as_rows(x)
    got = summarise(rows, T, nc, probs)
    ref = R.restate(rows, T, nc, probs)
    R.check(got, ref)
    return got, ref


# ---- shapes: idle lanes (256 % ct != 0), a partial last tile (np % 16 != 0), one or few chains, n in {2, 3, 31, 32, 33}
SHAPES = [  # np, nc, T, kind, seed
    (1, 1, 4, "iid", 1), (3, 2, 5, "ar", 2), (12, 255, 6, "iid", 3), (17, 257, 7, "ar", 4), (33, 1000, 63, "ar", 5),
    (256, 2, 64, "iid", 6), (1, 257, 65, "ar", 7), (3, 1000, 66, "iid", 8), (17, 1, 67, "ar", 9), (256, 255, 65, "ar", 10),
    (12, 1000, 67, "iid", 11), (33, 255, 4, "ar", 12), (1, 2, 63, "iid", 13),
]


@pytest.mark.parametrize("np_,nc,T,kind,seed", SHAPES)
def test_shapes(np_, nc, T, kind, seed):
    check_rows(series(T, nc, np_ + 1, kind, seed, offset=0.3))


# ---- the lag windows, lag by lag: the ring's tail block, the last partial window, and launches of KW windows growing
# 2 -> 4 -> 3 (n = 257), 2 -> 4 -> 4 (300), 2 -> 4 -> 8 -> 8 -> 1 (705)
LAG_N = [2, 3, 31, 32, 33, 63, 64, 65, 96, 97, 257, 300, 705]


def launches(n):
    """the KW of each k_sum_acov launch that takes all ceil(n / 32) windows"""
    nwin, k0, kw, out = -(-n // 32), 0, 2, []
    while k0 < nwin:
        out.append(min(kw, 8, nwin - k0))
        k0, kw = k0 + out[-1], kw * 2
    return out


@pytest.mark.parametrize("np_", [1, 5, 16, 17])
@pytest.mark.parametrize("n", LAG_N)
def test_every_lag(n, np_):
    T, nc = 2 * n + n % 2, 300 if n in (257, 300) else 37  # 300 chains: two workgroups of the log L column
    assert n != 705 or launches(n) == [2, 4, 8, 8, 1]
    x = series(T, nc, np_ + 1, "ar", 100 * n + np_)
    acov, sumsq = rows_acov(as_rows(x), T, nc, n)
    xd = x.astype(np.float64)
    for c in range(np_ + 1):
        sims = np.concatenate([xd[:n, :, c], xd[T - n:, :, c]], axis=1)
        want = R.direct_acov(sims, n)
        tol = (2 * n + 1024) * EPS * want[0]  # the recursive-summation bound of the longest serial sum
        err = np.abs(acov[c] - want)
        assert err.max() <= tol, ("column", c, "lag", int(err.argmax()), err.max(), tol)
        v = xd[:, :, c].reshape(-1)
        ss = ((v - v.mean()) ** 2).sum()
        assert abs(sumsq[c] - ss) <= (2 * n + 1024) * EPS * ss, ("column", c, sumsq[c], ss)


def test_random_walk_uses_every_window():
    """unmixed random walks: the Geyer loop runs to n - 5, so its last pair reads lags in the last, partial window"""
    n, nc, np_ = 116, 64, 5
    T = 2 * n + 1
    x = series(T, nc, np_ + 1, "rw", 21, offset=30.0)
    got, ref = check_rows(x)
    for c, r in enumerate(ref):
        assert r["ess_lag"] >= n - 5 and got["ess_lag"][c] == r["ess_lag"]
        assert r["ess_lag"] + 1 >= 32 * (n // 32) and n % 32  # a lag the ESS used lies in the partial window


# ---- order statistics: 32 probabilities, 66 targets, more than 32 prefixes per column (a second k_sum_hist group)
Q_PROBS = [0.0, 1.0, 0.29, 0.57, 0.58, 0.5, 0.01, 0.02, 0.03, 0.05, 0.07, 0.1, 0.13, 0.17, 0.2, 0.25, 0.31, 0.37, 0.42,
           0.63, 0.66, 0.71, 0.75, 0.8, 0.83, 0.88, 0.9, 0.95, 0.97, 0.99, 0.123, 0.9001]


@pytest.mark.parametrize("np_", [16, 3])
def test_order_statistics_many_prefixes(np_):
    T, nc = 133, 97
    N = T * nc
    assert len(set(Q_PROBS)) == 32
    x = series(T, nc, np_ + 1, "iid", 30 + np_)
    x[:, :, 1] = np.round(x[:, :, 1], 1)  # ties
    got, _ = check_rows(x, Q_PROBS)
    h = [(N - 1) * p for p in Q_PROBS]
    exact = [k for k, v in enumerate(h) if v == int(v)]
    below = [k for k, v in enumerate(h) if 0 < round(v) - v < 1e-9]
    assert len(exact) >= 25 and {Q_PROBS[k] for k in below} == {0.29, 0.57, 0.58}
    ranks = [0, N - 1] + [r for v in h for r in (min(int(v), N - 1), min(int(v) + 1, N - 1))]
    most = 0
    for c in range(np_ + 1):
        keys = np.sort(R.okey(x[:, :, c]).reshape(-1))
        srt = R.key_float(keys)
        for k in exact:  # h integral: the quantile is the order statistic itself, to the bit
            assert got["quantiles"][c][k] == float(srt[int(h[k])]), (c, Q_PROBS[k])
        for d in (1, 2, 3):
            most = max(most, len(set((keys[ranks] >> (32 - 8 * d)).tolist())))
    assert most > 32


# ---- steps in three histogram chunks of 65 536, odd T
def test_histogram_step_chunks():
    T, nc, np_ = 140001, 3, 2
    assert (T + 65535) // 65536 == 3
    check_rows(series(T, nc, np_ + 1, "iid", 40))


# ---- values: each kind in parameter column 1 and in log L, ordinary data around them
def value_column(kind, T, nc, rng, neg=False):
    if kind == "ties":
        v = rng.choice(np.array([0.5, -1.25, 3.0], np.float32), size=(T, nc), p=[0.9, 0.05, 0.05])
    elif kind in ("zeros+-", "zeros-+"):  # -0 and +0 among positives (log L: among negatives), in both orders
        v = np.abs(rng.standard_normal((T, nc))).astype(np.float32)
        z = rng.random((T, nc)) < 0.3
        v[z] = 0.0
        v[z & (rng.random((T, nc)) < 0.5)] = -0.0
        first = np.flatnonzero(z.reshape(-1))[0]
        v.reshape(-1)[first] = -0.0 if kind == "zeros-+" else 0.0
        v = -v if neg else v
    elif kind == "subnormal":
        bits = rng.integers(1, 1 << 23, size=(T, nc), dtype=np.uint32) | (rng.integers(0, 2, (T, nc), np.uint32) << 31)
        v = bits.view(np.float32)
    elif kind == "inf":
        v = rng.standard_normal((T, nc)).astype(np.float32)
        v[rng.random((T, nc)) < 0.1] = -np.inf
        if not neg:
            v[rng.random((T, nc)) < 0.1] = np.inf
    elif kind in ("nan+", "nan-"):
        v = rng.standard_normal((T, nc)).astype(np.float32)
        v.reshape(-1)[rng.choice(T * nc, 3, replace=False)] = np.array(
            [0x7fc00000, 0x7f800001, 0x7fc12345] if kind == "nan+" else [0xffc00000, 0xff800001, 0xffc12345],
            np.uint32).view(np.float32)
    elif kind == "huge":
        v = (np.sign(rng.standard_normal((T, nc))) * (3.0e38 + 4.0e37 * rng.random((T, nc)))).astype(np.float32)
        v.reshape(-1)[:2] = [np.finfo(np.float32).max, -np.finfo(np.float32).max]
    elif kind == "offset":  # 1e6 plus a few ulps (0.0625)
        v = (1e6 + 0.0625 * rng.integers(-3, 4, (T, nc))).astype(np.float32)
    elif kind == "constant":
        v = np.full((T, nc), 0.1, np.float32)
    elif kind == "halves":  # constant within every half-chain, not across: W = 0; the middle step (odd T) differs
        v = np.empty((T, nc), np.float32)
        n = T // 2
        v[:n] = rng.standard_normal(nc)
        v[T - n:] = rng.standard_normal(nc)
        v[n:T - n] = 9.0
    elif kind == "frozen":  # one chain stuck, the others moving
        v = series(T, nc, 1, "ar", int(rng.integers(1 << 30)))[:, :, 0]
        v[:, 1] = v[0, 1]
    return v


VALUE_KINDS = ["ties", "zeros+-", "zeros-+", "subnormal", "inf", "nan+", "nan-", "huge", "offset", "constant", "halves",
               "frozen"]


@pytest.mark.parametrize("kind", VALUE_KINDS)
def test_values(kind):
    T, nc, np_ = 33, 3, 3
    rng = np.random.default_rng(VALUE_KINDS.index(kind) + 50)
    x = series(T, nc, np_ + 1, "ar", VALUE_KINDS.index(kind) + 60)
    x[:, :, 1] = value_column(kind, T, nc, rng)
    x[:, :, np_] = value_column(kind, T, nc, rng, neg=True)
    got, ref = check_rows(x)
    for c in (1, np_):
        if kind.startswith("zeros"):  # -0 orders before +0
            assert R.okey(np.float32(got["min" if c == 1 else "max"][c]))[()] == (0x7fffffff if c == 1 else 0x80000000)
        if kind in ("constant", "halves"):
            assert np.isnan(got["rhat"][c]) and np.isnan(got["ess"][c]) and got["ess_lag"][c] == 0
        if kind == "constant":
            # N = 99: 99 * 0.1f times the double 1/99 is not 0.1f, so a mean formed with 1/N would leave sd != 0
            assert got["sd"][c] == 0.0 and (99 * float(np.float32(0.1))) * (1.0 / 99) != float(np.float32(0.1))
        if kind == "subnormal":
            assert got["sd"][c] > 0 and got["flags"][c] == 0


# ---- Engine.summary and rows_summary of the same store: the same bytes
@pytest.mark.parametrize("d,stride", [(12, 1), (17, 1), (12, 3)])
def test_entry_points_agree(d, stride):
    import mcpar_amd as M
    from mcpar_amd import engine as E
    n, nburn, nsamp = 257, 100, 131
    vg, keep = M.make_vlfunc(M.VL_GAUSSIAN, d, np.array([1.5] * d + [1.0] * d, np.float32))
    eg = M.Engine(d, n, pl=1.0)
    if stride > 1:
        eg.set_option(E.OPT_SAMPLE_STRIDE, stride)
    eg.run(nsamp, nburn, O.default_pinit(d, n), vg)
    T = eg.samples.shape[0] // n
    assert T == -(-nsamp // stride)
    a = eg.summary(PROBS)
    same_bytes(a, eg.summary(PROBS))
    same_bytes(a, summarise(eg.samples_range(0, T), T, n))
