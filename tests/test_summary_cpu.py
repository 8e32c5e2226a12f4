"""mcx_debug_summary_finish -- the host step of mcx_samples_summary (R-hat, Geyer's ESS, quantile interpolation) --
against the float64 restatement of DESIGN.md "Sample-store summaries" (tests/summary_ref.py).  No GPU."""
import math

import numpy as np
import pytest

import summary_ref as R
from mcpar_amd import McxError
from mcpar_amd import engine as E


def finish(n, M, acov, var_means, probs=(), ostat=None, N=None, flags=0, mean=0.25, var_all=1.5):
    N = N if N is not None else 2 * n * M // 2
    ostat = ostat if ostat is not None else np.zeros(2 + 2 * len(probs), np.float32)
    return E.debug_summary_finish(n, M, mean, var_all, var_means, acov, ostat, N, probs, flags)


def expect(n, M, acov, var_means):
    W = acov[0] * n / (n - 1)
    var_plus = acov[0] + var_means
    ess, max_t, pairs = R.geyer(n, M, np.asarray(acov), W, var_plus)
    return math.sqrt(var_plus / W), ess, max_t, pairs


def check_col(col, n, M, acov, var_means, var_all=1.5):
    rhat, ess, max_t, _ = expect(n, M, acov, var_means)
    assert abs(col["rhat"] - rhat) < 1e-14
    assert col["ess_lag"] == max_t
    assert col["ess"] == pytest.approx(ess, rel=1e-13)
    assert col["mcse_mean"] == pytest.approx(math.sqrt(var_all) / math.sqrt(ess), rel=1e-13)
    assert col["sd"] == pytest.approx(math.sqrt(var_all), rel=1e-15)
    assert col["flags"] == 0


def ar_acov(n, M, phi, seed):
    """per-half-chain means / variances and the chain-averaged autocovariance of M synthetic AR(1) half-chains"""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, M))
    x[0] = rng.standard_normal(M)
    for i in range(1, n):
        x[i] = phi * x[i - 1] + rng.standard_normal(M)
    x += rng.normal(0, 0.05, M)  # chain offsets
    m = x.mean(axis=0)
    acov = R.half_chain_acov(x) / (n * M)
    s2 = x.var(axis=0, ddof=1)
    assert acov[0] * n / (n - 1) == pytest.approx(s2.mean(), rel=1e-12)  # W from lag 0
    return acov, m.var(ddof=1)


@pytest.mark.parametrize("n,M,phi,seed", [(100, 8, 0.6, 1), (257, 4, 0.9, 2), (64, 2, 0.3, 3), (500, 16, -0.4, 4)])
def test_synthetic_half_chains(n, M, phi, seed):
    acov, vm = ar_acov(n, M, phi, seed)
    col, _, need = finish(n, M, acov, vm)
    assert need == 0
    check_col(col, n, M, acov, vm)


def test_asks_for_more_lags():
    n, M = 400, 8
    acov, vm = ar_acov(n, M, 0.97, 5)
    _, _, max_t, _ = expect(n, M, acov, vm)
    assert max_t > 40
    col, _, need = finish(n, M, acov[:32], vm)
    assert 32 < need <= max_t + 4
    got = need
    while need:  # the device's windows arrive 32 lags at a time
        got = min(n, got + 32)
        col, _, need = finish(n, M, acov[:got], vm)
    check_col(col, n, M, acov, vm)


def test_monotone_step_fires():
    n, M = 60, 4
    rho = np.zeros(n)
    rho[:10] = [1.0, 0.5, 0.2, 0.1, 0.35, 0.3, 0.05, 0.02, -0.3, -0.2]
    rho[10:] = -0.01
    acov0, vm = 2.0, 0.1
    var_plus = acov0 + vm
    W = acov0 * n / (n - 1)
    acov = W - (1 - rho) * var_plus  # rho(t) = 1 - (W - acov(t)) / var+
    acov[0] = acov0
    rr = 1 - (W - acov) / var_plus
    rr[0] = 1
    assert rr[4] + rr[5] > rr[2] + rr[3]  # the pair the monotone step replaces
    col, _, need = finish(n, M, acov, vm)
    assert need == 0
    check_col(col, n, M, acov, vm)
    rhat, ess, max_t, _ = expect(n, M, acov, vm)
    # without the monotone step tau would hold the larger pair
    tau_raw = -1 + 2 * rr[:max_t].sum() + (rr[max_t] if rr[max_t] > 0 else 0)
    assert col["ess"] > M * n / tau_raw


def test_pair_sums_never_end():
    n, M = 30, 4
    acov, vm = ar_acov(n, M, 0.995, 6)
    col, _, need = finish(n, M, acov, vm)
    assert need == 0
    _, _, max_t, pairs = expect(n, M, acov, vm)
    assert max_t >= n - 5 and pairs[-1] > 0
    check_col(col, n, M, acov, vm)


def test_log10_floor():
    n, M = 50, 4
    acov0, vm = 1.0, 0.0
    var_plus = acov0 + vm
    W = acov0 * n / (n - 1)
    rho = np.full(n, -0.3)
    rho[1] = -0.95  # strongly antithetic: the sum goes below the floor
    acov = W - (1 - rho) * var_plus
    acov[0] = acov0
    col, _, need = finish(n, M, acov, vm)
    assert need == 0
    assert col["ess"] == pytest.approx(M * n * math.log10(M * n), rel=1e-14)
    check_col(col, n, M, acov, vm)


def test_quantile_interpolation():
    N = 101
    rng = np.random.default_rng(7)
    srt = np.sort(rng.standard_normal(N).astype(np.float32))
    probs = (0.0, 1.0, 0.25, 0.013, 0.5, 0.99)
    want, lo_hi = R.quantiles_from_sorted(srt, probs)
    ostat = np.array([srt[0], srt[-1]] + [v for ab in lo_hi for v in ab], np.float32)
    acov, vm = ar_acov(50, 2, 0.5, 8)
    col, q, need = finish(50, 2, acov, vm, probs, ostat, N)
    assert q[0] == srt[0] and q[1] == srt[-1]  # p = 0 and 1: the extremes, exactly
    assert q[2] == srt[25]                     # h = 25 integral: the order statistic itself
    np.testing.assert_allclose(q, want, rtol=1e-15)
    assert col["min"] == srt[0] and col["max"] == srt[-1]
    np.testing.assert_allclose(q, np.quantile(srt.astype(np.float64), probs), rtol=1e-12)


def test_nonfinite_and_nan():
    N = 8
    ostat = np.array([-np.inf, 3.0, -np.inf, 2.0], np.float32)  # min, max, x(lo), x(lo+1) for p = 0.1
    col, q, need = finish(2, 2, [1.0, 0.5], 0.1, (0.1,), ostat, N, flags=E.SUMMARY_NONFINITE)
    assert need == 0 and col["flags"] == E.SUMMARY_NONFINITE
    for f in ("mean", "sd", "rhat", "ess", "mcse_mean"):
        assert math.isnan(col[f])
    assert col["min"] == -np.inf and col["max"] == 3.0
    assert math.isnan(q[0])  # -inf + 0.7 (2 - -inf): the formula's inf - inf
    ostat = np.array([-np.inf, np.inf, np.inf, np.inf], np.float32)
    col, q, _ = finish(2, 2, [1.0, 0.5], 0.1, (0.5,), ostat, N, flags=E.SUMMARY_NONFINITE)
    assert q[0] == np.inf  # inside a run of equal values: that value
    ostat = np.array([-1.0, np.nan, 0.0, 1.0], np.float32)
    col, q, _ = finish(2, 2, [1.0, 0.5], 0.1, (0.5,), ostat, N, flags=E.SUMMARY_NONFINITE)
    assert math.isnan(col["min"]) and math.isnan(col["max"]) and math.isnan(q[0])


def test_constant_column():
    col, _, need = finish(10, 4, np.zeros(10), 0.0, var_all=0.0)
    assert need == 0
    assert math.isnan(col["rhat"]) and math.isnan(col["ess"]) and col["sd"] == 0.0


def test_bad_arguments():
    with pytest.raises(McxError):
        E.debug_summary_finish(1, 2, 0.0, 1.0, 0.0, [1.0], np.zeros(2, np.float32), 4)


# ---- the reference itself on the edges of the contract: key order, quantiles, the lag sums, W = 0

def edge_values(seed):
    """float32 values with every kind of edge: signed zeros and NaNs, infinities, subnormals, ties, extremes"""
    rng = np.random.default_rng(seed)
    bits = [0x00000000, 0x80000000, 0x7fc00000, 0xffc00000, 0x7f800001, 0x7f800000, 0xff800000, 0x00000001, 0x80000001,
            0x007fffff, 0x807fffff, 0x00800000, 0x7f7fffff, 0xff7fffff]
    special = np.array(bits, np.uint32).view(np.float32)
    x = np.concatenate([special, special, rng.standard_normal(200).astype(np.float32), np.full(20, 1.5, np.float32)])
    return x[rng.permutation(x.size)]


def py_key(v):
    """the kernel's key of one float32, bit by bit in plain Python"""
    u = int(np.float32(v).view(np.uint32))
    if math.isnan(v):
        return 0xffffffff
    return (~u & 0xffffffff) if u >> 31 else (u | 0x80000000)


@pytest.mark.parametrize("seed", [1, 2])
def test_reference_order_is_the_key_order(seed):
    x = edge_values(seed)
    want = sorted((py_key(v) for v in x))
    assert R.okey(x).tolist() == [py_key(v) for v in x]
    srt = R.key_sort(x)
    finite = ~np.isnan(srt)
    assert [py_key(v) for v in srt[finite]] == want[:int(finite.sum())]
    assert np.isnan(srt[~finite]).all() and not finite[-int((~finite).sum()):].any()
    # -0 strictly before +0: the first zero is -0 whichever comes first in x
    z = np.flatnonzero(srt == 0)
    assert srt[z[0]].view(np.uint32) == 0x80000000 and srt[z[-1]].view(np.uint32) == 0


@pytest.mark.parametrize("first", [0.0, -0.0])
def test_reference_min_max_signed_zero(first):
    x = np.array([[first, -first], [1.0, 2.0], [-first, first], [3.0, 4.0]], np.float32)
    r = R.restate_column(x, (0.0, 1.0))
    assert np.float32(r["min"]).view(np.uint32) == 0x80000000
    y = -x
    r = R.restate_column(y, (0.0, 1.0))
    assert np.float32(r["max"]).view(np.uint32) == 0x00000000


@pytest.mark.parametrize("nan_bits", [0x7fc00000, 0xffc00000, 0x7f800001])
def test_reference_nan_column(nan_bits):
    x = np.arange(12, dtype=np.float32).reshape(6, 2)
    x[3, 1] = np.array([nan_bits], np.uint32).view(np.float32)[0]
    r = R.restate_column(x, (0.0, 0.5, 1.0))
    assert r["flags"] == 1 and math.isnan(r["min"]) and math.isnan(r["max"]) and np.isnan(r["quantiles"]).all()
    got = dict(flags=[1], min=[np.float32(np.nan)], max=[np.array([0xffffffff], np.uint32).view(np.float32)[0]],
               quantiles=[np.full(3, np.nan)], mean=[np.nan], sd=[np.nan], rhat=[np.nan], ess=[np.nan], mcse_mean=[np.nan])
    R.check(got, {0: r})  # any NaN payload is "a NaN"
    got["max"] = [np.float32(11.0)]
    with pytest.raises(AssertionError):
        R.check(got, {0: r})


@pytest.mark.parametrize("N,seed", [(101, 1), (8385, 2), (1000, 3)])
def test_reference_quantiles_match_numpy(N, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(N).astype(np.float32)
    x[:N // 10] = x[N // 10]  # a run of ties
    probs = np.concatenate([[0.0, 1.0, 0.29, 0.5, 1 / 64, 63 / 64], rng.random(20)])
    q, _ = R.quantiles_from_sorted(R.key_sort(x), probs)
    np.testing.assert_allclose(q, np.quantile(x.astype(np.float64), probs, method="linear"), rtol=1e-12, atol=0)


@pytest.mark.parametrize("n,M,phi,seed", [(2, 2, 0.0, 1), (33, 4, 0.5, 2), (97, 6, 0.9, 3), (300, 2, -0.3, 4)])
def test_direct_acov_equals_fft(n, M, phi, seed):
    rng = np.random.default_rng(seed)
    x = np.zeros((n, M))
    x[0] = rng.standard_normal(M)
    for i in range(1, n):
        x[i] = phi * x[i - 1] + rng.standard_normal(M)
    x += rng.normal(0, 3, M)
    d, f = R.direct_acov(x, n), R.half_chain_acov(x)
    assert abs(d - f).max() <= 1e-12 * d[0]
    c = x - x.mean(axis=0)
    assert d[n - 1] == pytest.approx((c[0] * c[n - 1]).sum(), rel=1e-15)  # the last lag: one product per half-chain


def test_reference_w_zero():
    """W = 0 (constant within every half-chain): NaN rhat, ess, mcse; ess_lag 0; sd the plain value"""
    T, nc = 9, 3
    with np.errstate(all="raise"):  # no division by zero on the way
        r = R.restate_column(np.full((T, nc), 0.1, np.float32), (0.5,))
        assert r["sd"] == 0.0 and r["mean"] == pytest.approx(np.float32(0.1), rel=1e-15) and r["flags"] == 0
        assert math.isnan(r["rhat"]) and math.isnan(r["ess"]) and math.isnan(r["mcse_mean"]) and r["ess_lag"] == 0
        x = np.empty((T, nc), np.float32)
        x[:4], x[4], x[5:] = [1.0, 2.0, 3.0], 7.0, [-1.0, 0.5, 4.0]  # halves differ; the middle step of odd T is in neither
        r = R.restate_column(x, (0.5,))
    assert math.isnan(r["rhat"]) and math.isnan(r["ess"]) and r["ess_lag"] == 0
    assert r["sd"] == pytest.approx(x.astype(np.float64).std(ddof=1), rel=1e-15) and r["sd"] > 0
    nan = float("nan")
    got = {k: [v] for k, v in dict(flags=0, min=r["min"], max=r["max"], quantiles=r["quantiles"], mean=r["mean"],
                                   sd=r["sd"], rhat=nan, ess=nan, mcse_mean=nan, ess_lag=0).items()}
    R.check(got, {0: r})
    got["ess"] = [1.0]
    with pytest.raises(AssertionError):
        R.check(got, {0: r})


def test_debug_rows_acov_bad_arguments():
    rows = np.zeros((8 * 2, 3), np.float32)  # nsteps 8, nc 2, np 2: n = 4
    for nsteps, nlags in ((8, 0), (8, 5), (3, 1)):
        with pytest.raises(McxError):
            E.debug_rows_acov(rows, nsteps, 2, nlags)


# ---- mcx_debug_select_step: the digit walk of the radix select, driven from numpy -----------------------------------------
def radix_select(keys, k):
    """the k-th smallest of uint32 keys: four passes, most significant byte first; numpy histograms the keys that match the
    prefix found so far, the library walks the histogram"""
    keys = np.asarray(keys, np.uint32)
    prefix, rem = 0, k
    for p in range(4):
        shift = 24 - 8 * p
        under = keys[(keys.astype(np.uint64) >> (shift + 8)) == prefix]
        hist = np.bincount((under >> np.uint32(shift)) & np.uint32(255), minlength=256)
        digit, rem = E.debug_select_step(hist, rem)
        assert 0 <= digit <= 255 and 0 <= rem < max(hist[digit], 1), (p, digit, rem)
        prefix = (prefix << 8) | digit
    return prefix


SELECT_CASES = {
    # name: (keys, target ranks)
    "one key": ([0x12345678], [0]),
    "all equal": ([0x80000001] * 7, [0, 3, 6]),
    "first and last": ([5, 0xfffffffe, 0x01020304, 0x01020305, 0], [0, 4]),
    # 0xff in every position: each pass ends at the b < 255 stop, before and behind smaller keys in the same buckets
    "all bytes 0xff": ([0xffffffff, 0xffffff00, 0xff00ffff, 0x00ffffff, 0xffffffff, 0xfffffffe], [0, 3, 4, 5]),
    # a run of duplicates (ranks 2 .. 6): inside it, on both of its ends, and its two neighbours
    "duplicates": ([0x40000000, 0x40000001] + [0x40000100] * 5 + [0x40000101, 0x41000000], [1, 2, 3, 4, 6, 7]),
    # two targets that share three bytes and differ in the last
    "last byte": ([0xabcdef01, 0xabcdef02, 0xabcdee02, 0xabcdef00, 0xabcdf000], [1, 2, 3]),
}


@pytest.mark.parametrize("name", sorted(SELECT_CASES))
def test_select_step_radix_select(name):
    keys, ranks = SELECT_CASES[name]
    keys = np.array(keys, np.uint32)
    want = np.sort(keys)
    rng = np.random.default_rng(len(name))
    for order in (keys, keys[::-1], rng.permutation(keys)):  # the counts, not the order, decide
        for k in ranks:
            assert radix_select(order, k) == int(want[k]), (name, k)


def test_select_step_stops_at_255():
    """a rank past every count lands in bucket 255 (a histogram the device never makes: the walk must still end)"""
    hist = np.zeros(256, np.uint64)
    hist[3] = 2
    assert E.debug_select_step(hist, 1) == (3, 1)
    assert E.debug_select_step(hist, 2) == (255, 0)
    assert E.debug_select_step(hist, 9) == (255, 7)
    hist[255] = 4
    assert E.debug_select_step(hist, 5) == (255, 3)
    with pytest.raises(McxError):
        E.debug_select_step(hist, -1)
