"""The chain table, the keep rule and the selection of DESIGN.md section 16, restated in float64 numpy from the definitions of
include/mcx.h alone: two-pass mean, sd and rho1 per (chain, column) series, moves and longest_stay on the rows' bits, the
rule with np.median.  rows are MCout rows [T * nc, ncol] float32, step-major then chain."""
import numpy as np

NONFINITE, STUCK, OUTLIER = 1, 2, 4


def order_key(b):
    """u32 keys ascending in float order: -inf < finite < +inf, -0 before +0"""
    b = b.astype(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000))


def table(rows, T, nc):
    rows = np.ascontiguousarray(rows, np.float32)
    ncol = rows.shape[1]
    a = rows.reshape(T, nc, ncol)
    x = a.astype(np.float64)
    fin = np.isfinite(x).all(axis=0)  # [nc, ncol]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mean = x.sum(axis=0) / T
        c = x - mean
        ss = (c * c).sum(axis=0)
        sd = np.sqrt(ss / (T - 1)) if T > 1 else np.full((nc, ncol), np.nan)
        sc = (c[:-1] * c[1:]).sum(axis=0)
        rho1 = np.where(ss > 0, sc / np.where(ss > 0, ss, 1.0), np.nan) if T > 1 else np.full((nc, ncol), np.nan)
    mean, sd, rho1 = (np.where(fin, v, np.nan) for v in (mean, sd, rho1))
    bits = a.view(np.uint32)
    changed = (bits[1:] != bits[:-1]).any(axis=2)  # [T - 1, nc]
    moves = changed.sum(axis=0).astype(np.int64)
    longest = np.ones(nc, np.int64)
    run = np.ones(nc, np.int64)
    for t in range(T - 1):
        run = np.where(changed[t], 1, run + 1)
        longest = np.maximum(longest, run)
    ll = a[:, :, -1]
    key = order_key(bits[:, :, -1])
    step = key.argmax(axis=0).astype(np.int32)  # (the first of equal keys)
    ll_max = ll[step, np.arange(nc)].copy()
    llnan = np.isnan(ll).any(axis=0)
    ll_max[llnan] = np.nan
    step[llnan] = -1
    flags = np.where(fin.all(axis=1), 0, 1).astype(np.int32)
    return dict(mean=mean, sd=sd, rho1=rho1, moves=moves, longest_stay=longest, ll_max=ll_max.astype(np.float32), ll_max_step=step,
                flags=flags)


def table_longdouble(rows, T, nc):
    """mean, sd, rho1 of table() in numpy's longdouble, for the restatement's own error on an offset series"""
    x = np.ascontiguousarray(rows, np.float32).reshape(T, nc, -1).astype(np.longdouble)
    mean = x.sum(axis=0) / T
    c = x - mean
    ss = (c * c).sum(axis=0)
    return mean, np.sqrt(ss / (T - 1)), (c[:-1] * c[1:]).sum(axis=0) / ss


def keep(t, z=5.0, min_moves=1, max_stay=0, use_col=None):
    """(reasons [nc], centre [ncol, 2], kept indices) of the rule of mcx_chains_keep on a table dict"""
    mean = np.asarray(t["mean"], np.float64)
    nc, ncol = mean.shape
    use = np.ones(ncol, bool) if use_col is None else np.asarray(use_col) != 0
    nonfinite = (np.asarray(t["flags"]) & 1).astype(bool) | ~np.isfinite(mean).all(axis=1)
    stuck = (np.asarray(t["moves"]) < min_moves) | ((max_stay > 0) & (np.asarray(t["longest_stay"]) > max_stay))
    reasons = np.where(nonfinite, NONFINITE, np.where(stuck, STUCK, 0)).astype(np.int32)
    centre = np.full((ncol, 2), np.nan)
    for c in np.flatnonzero(use):
        m = mean[:, c]
        f = m[np.isfinite(m)]
        if f.size == 0:
            continue
        med = np.median(f)
        scale = 1.4826 * np.median(np.abs(f - med))
        centre[c] = med, scale
        if np.isfinite(z):
            with np.errstate(invalid="ignore"):
                out = np.abs(m - med) > z * scale
            reasons[out & ~nonfinite] |= OUTLIER
    return reasons, centre, np.flatnonzero(reasons == 0).astype(np.int32)


def select(rows, T, nc, chains):
    """the MCout rows of the store of chosen chains: out[t][k] = in[t][chains[k]]"""
    rows = np.ascontiguousarray(rows, np.float32)
    a = rows.reshape(T, nc, rows.shape[1])
    return np.ascontiguousarray(a[:, np.asarray(chains, np.int64), :]).reshape(-1, rows.shape[1])
