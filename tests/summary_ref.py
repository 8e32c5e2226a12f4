"""float64 numpy restatement of mcx_samples_summary (DESIGN.md "Sample-store summaries"), for the tests.

Every definition here is the one DESIGN.md writes out: split chains, R-hat, Geyer's ESS on the chain-averaged biased
autocovariance (posterior's ess_basic), numpy "linear" / R type 7 quantiles from exact order statistics.  Order
statistics follow the kernel's total key order (okey): -0 before +0, every NaN last."""
import math

import numpy as np


def geyer(n, M, acov, W, var_plus):
    """ESS from acov[t] = mean over the M half-chains of (1/n) sum_{i<n-t} c_i c_{i+t}.
    Returns (ess, max_t, pair sums the loop looked at)."""
    rho = np.zeros(n + 2)
    R = lambda t: 1.0 - (W - acov[t]) / var_plus  # noqa: E731
    t = 0
    even, odd = 1.0, R(1)
    rho[0], rho[1] = even, odd
    pairs = [even + odd]
    while t < n - 5 and not math.isnan(even + odd) and even + odd > 0:
        t += 2
        even, odd = R(t), R(t + 1)
        pairs.append(even + odd)
        if even + odd >= 0:
            rho[t], rho[t + 1] = even, odd
    max_t = t
    if even > 0:
        rho[max_t] = even
    t = 0
    while t <= max_t - 4:  # Geyer's initial monotone sequence
        t += 2
        if rho[t] + rho[t + 1] > rho[t - 2] + rho[t - 1]:
            rho[t] = (rho[t - 2] + rho[t - 1]) / 2
            rho[t + 1] = rho[t]
    tau = -1.0 + 2.0 * rho[:max_t].sum() + rho[max_t]
    tau = max(tau, 1.0 / math.log10(M * n))
    return M * n / tau, max_t, pairs


def okey(x):
    """the kernel's order-preserving u32 key of float32 values: sign-flipped bits, every NaN 0xffffffff"""
    x = np.asarray(x, np.float32)
    u = x.view(np.uint32)
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[np.isnan(x)] = 0xffffffff
    return k


def key_float(k):
    """the float32 of a key (okey's inverse on every key that is not a NaN's)"""
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(np.float32)


def key_sort(x):
    """the values of x in key order"""
    return key_float(np.sort(okey(x.reshape(-1))))


def quantiles_from_sorted(srt, probs):
    """(values, order statistics x(lo), x(lo+1)) from the column sorted in float order"""
    N = srt.size
    out, lo_hi = [], []
    for p in probs:
        h = (N - 1) * float(p)
        lo = math.floor(h)
        g = h - lo
        a, b = float(srt[min(lo, N - 1)]), float(srt[min(lo + 1, N - 1)])
        lo_hi.append((srt[min(lo, N - 1)], srt[min(lo + 1, N - 1)]))
        out.append(a if g == 0 or a == b else a + g * (b - a))
    return np.array(out), lo_hi


def half_chain_acov(sims, chunk=8192):
    """sum over half-chains of sum_{i<n-t} c_i c_{i+t} for t < n (c = the half-chain centred on its mean); sims [n, M]"""
    n, M = sims.shape
    nfft = 1 << (2 * n - 1).bit_length()
    power = np.zeros(nfft // 2 + 1)
    for c0 in range(0, M, chunk):
        c = sims[:, c0:c0 + chunk]
        c = c - c.mean(axis=0)
        f = np.fft.rfft(c, nfft, axis=0)
        power += (f.real ** 2 + f.imag ** 2).sum(axis=1)
    return np.fft.irfft(power, nfft)[:n]


def direct_acov(sims, nlags):
    """half_chain_acov's sums for t < nlags by plain float64 products, no FFT; sims [n, M]"""
    n, M = sims.shape
    c = sims - sims.mean(axis=0)
    return np.array([np.einsum("im,im->", c[:n - t], c[t:]) for t in range(nlags)])


def restate_column(x, probs):
    """x [nsteps, nc] float32: the summary of one column as a dict (plus 'ostat' and 'pairs')"""
    T, nc = x.shape
    N = T * nc
    n, M = T // 2, 2 * nc
    srt = key_sort(x)
    has_nan = bool(np.isnan(srt[-1]))
    q, lo_hi = quantiles_from_sorted(srt, probs)
    r = dict(min=np.float32(np.nan) if has_nan else srt[0], max=srt[-1], quantiles=np.full(len(probs), np.nan) if has_nan else q,
             ostat=lo_hi, flags=0, pairs=[])
    if not np.all(np.isfinite(x)):
        r.update(flags=1, mean=np.nan, sd=np.nan, rhat=np.nan, ess=np.nan, mcse_mean=np.nan, ess_lag=0)
        return r
    xd = x.astype(np.float64)
    r["mean"] = xd.mean()
    r["sd"] = xd.std(ddof=1)
    sims = np.concatenate([xd[:n], xd[T - n:]], axis=1)  # [n, M]
    m = sims.mean(axis=0)
    W = sims.var(axis=0, ddof=1).mean()
    if not W > 0:  # constant within every half-chain
        r.update(rhat=np.nan, ess=np.nan, mcse_mean=np.nan, ess_lag=0, n=n)
        return r
    var_plus = (n - 1) / n * W + m.var(ddof=1)
    r["rhat"] = math.sqrt(var_plus / W)
    acov = half_chain_acov(sims) / (n * M)
    ess, max_t, pairs = geyer(n, M, acov, W, var_plus)
    r.update(ess=ess, ess_lag=max_t, mcse_mean=r["sd"] / math.sqrt(ess), pairs=pairs, n=n)
    return r


def restate(rows, nsteps, nc, probs):
    """rows [nsteps * nc, np + 1] (MCout layout): one dict per column"""
    ncol = rows.shape[1]
    x = rows.reshape(nsteps, nc, ncol)
    return [restate_column(np.ascontiguousarray(x[:, :, c]), probs) for c in range(ncol)]


def same_float(got, want, where):
    """a NaN where the contract says NaN (any payload), else the same float32 bits"""
    got, want = np.float32(got), np.float32(want)
    if np.isnan(want):
        assert np.isnan(got), (where, got)
    else:
        assert got.view(np.uint32) == want.view(np.uint32), (where, got, want)


def check(got, ref, rel_mean=1e-9, abs_rhat=1e-7, rel_ess=1e-4, rel_q=1e-12, margin=1e-5):
    """assert the GPU's dict (Engine.summary) against restate()'s list, or a {column: restate_column()} dict"""
    refs = dict(enumerate(ref)) if isinstance(ref, list) else ref
    for c, r in sorted(refs.items()):
        where = "column %d" % c
        assert got["flags"][c] == r["flags"], where
        same_float(got["min"][c], r["min"], (where, "min"))
        same_float(got["max"][c], r["max"], (where, "max"))
        assert (np.isnan(got["quantiles"][c]) == np.isnan(r["quantiles"])).all(), (where, got["quantiles"][c])
        np.testing.assert_allclose(got["quantiles"][c], r["quantiles"], rtol=rel_q, atol=0, err_msg=where)
        if r["flags"]:
            for f in ("mean", "sd", "rhat", "ess", "mcse_mean"):
                assert math.isnan(got[f][c]), (where, f)
            continue
        np.testing.assert_allclose(got["mean"][c], r["mean"], rtol=rel_mean, atol=1e-300, err_msg=where)
        np.testing.assert_allclose(got["sd"][c], r["sd"], rtol=rel_mean, err_msg=where)
        assert got["ess_lag"][c] == r["ess_lag"], (where, got["ess_lag"][c], r["ess_lag"])
        if math.isnan(r["rhat"]):  # W = 0
            for f in ("rhat", "ess", "mcse_mean"):
                assert math.isnan(got[f][c]), (where, f)
            continue
        assert abs(got["rhat"][c] - r["rhat"]) < abs_rhat, (where, got["rhat"][c], r["rhat"])
        np.testing.assert_allclose(got["ess"][c], r["ess"], rtol=rel_ess, err_msg=where)
        np.testing.assert_allclose(got["mcse_mean"][c], r["mcse_mean"], rtol=rel_ess, err_msg=where)
        # the fixed-seed case does not pass by luck: the pair sums around the stop are clear of 0
        if r["ess_lag"] < r["n"] - 5:
            assert abs(r["pairs"][-1]) > margin and abs(r["pairs"][-2]) > margin, (where, r["pairs"][-2:])
