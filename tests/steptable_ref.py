"""The step table and the settle rule of DESIGN.md section 17, restated in float64 numpy from the definitions of include/mcx.h
alone: per (step, column) over the nc chains the two-pass mean and sd, min, max and type-7 quantiles from exact order
statistics in float order; per step the chains whose row's bits changed, the largest log L and the lowest chain that holds it.
rows are MCout rows [T * nc, ncol] float32, step-major then chain."""
import math

import numpy as np

NONFINITE = 1


def order_key(b):
    """u32 keys ascending in float order: -inf < finite < +inf, -0 before +0 (the bits of a NaN are not meant)"""
    b = b.astype(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000))


def table(rows, T, nc, probs=(0.05, 0.5, 0.95)):
    rows = np.ascontiguousarray(rows, np.float32)
    ncol = rows.shape[1]
    a = rows.reshape(T, nc, ncol)
    x = a.astype(np.float64)
    probs = np.asarray(probs, np.float64).reshape(-1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        tot = x.sum(axis=1)                                   # [T, ncol]
        fin = np.isfinite(tot)
        mean = tot / nc
        c = x - mean[:, None, :]
        ss = (c * c).sum(axis=1)
        sd = np.sqrt(ss / (nc - 1)) if nc > 1 else np.full((T, ncol), np.nan)
    mean, sd = np.where(fin, mean, np.nan), np.where(fin, sd, np.nan)
    bits = a.view(np.uint32)
    has_nan = np.isnan(a).any(axis=1)                         # [T, ncol]
    # the values of every (step, column) in float order: sort the keys, take the floats along
    order = np.argsort(order_key(bits), axis=1, kind="stable")
    srt = np.take_along_axis(a, order, axis=1)                # [T, nc, ncol] float32
    vmin, vmax = srt[:, 0, :].copy(), srt[:, -1, :].copy()
    vmin[has_nan] = np.nan
    vmax[has_nan] = np.nan
    q = np.zeros((T, ncol, probs.size))
    for k, p in enumerate(probs):
        h = (nc - 1) * float(p)
        lo = math.floor(h)
        g = h - lo
        x0 = srt[:, min(lo, nc - 1), :].astype(np.float64)
        x1 = srt[:, min(lo + 1, nc - 1), :].astype(np.float64)
        with np.errstate(invalid="ignore"):
            q[:, :, k] = np.where((g == 0.0) | (x0 == x1), x0, x0 + g * (x1 - x0))
    q[has_nan] = np.nan
    moved = np.full(T, -1, np.int32)
    if T > 1:
        moved[1:] = (bits[1:] != bits[:-1]).any(axis=2).sum(axis=1)
    ll = a[:, :, -1]
    chain = order_key(bits[:, :, -1]).argmax(axis=1).astype(np.int32)  # (the first of equal keys)
    ll_max = ll[np.arange(T), chain].copy()
    llnan = np.isnan(ll).any(axis=1)
    ll_max[llnan] = np.nan
    chain[llnan] = -1
    flags = np.where(fin, 0, NONFINITE).astype(np.int32)
    return dict(mean=mean, sd=sd, min=vmin, max=vmax, flags=flags, quantiles=q, moved=moved, ll_max=ll_max.astype(np.float32),
                ll_max_chain=chain, step_flags=flags.max(axis=1).astype(np.int32))


def settle(t, tol_mean=0.1, tol_sd=0.1, ref_frac=0.5, use_col=None):
    """(settled_step, dict of m_ref, s_ref, max_dev_mean, max_dev_sd, last_out [ncol]) of the rule of mcx_steps_settle"""
    mean, sd = np.asarray(t["mean"], np.float64), np.asarray(t["sd"], np.float64)
    T, ncol = mean.shape
    use = np.ones(ncol, bool) if use_col is None else np.asarray(use_col) != 0
    R = min(T, max(1, math.ceil(ref_frac * T)))
    out = dict(m_ref=np.full(ncol, np.nan), s_ref=np.full(ncol, np.nan), max_dev_mean=np.full(ncol, np.nan),
               max_dev_sd=np.full(ncol, np.nan), last_out=np.full(ncol, -1, np.int32))
    usable = True
    for c in np.flatnonzero(use):
        sm = sv = 0.0
        for i in range(T - R, T):  # in step order
            sm += mean[i, c]
            sv += sd[i, c] * sd[i, c]
        m_ref, s_ref = sm / R, math.sqrt(sv / R) if sv >= 0 else float("nan")
        out["m_ref"][c], out["s_ref"][c] = m_ref, s_ref
        scaled = math.isfinite(m_ref) and math.isfinite(s_ref) and s_ref > 0
        usable = usable and scaled
        fin = np.isfinite(mean[:, c]) & np.isfinite(sd[:, c])
        with np.errstate(invalid="ignore"):
            am, asd = np.abs(mean[:, c] - m_ref), np.abs(sd[:, c] - s_ref)
            inb = fin & (am <= tol_mean * s_ref) & (asd <= tol_sd * s_ref)
        if not inb.all():
            out["last_out"][c] = np.flatnonzero(~inb)[-1]
        if scaled:
            out["max_dev_mean"][c] = (am[fin] / s_ref).max() if fin.any() else 0.0
            out["max_dev_sd"][c] = (asd[fin] / s_ref).max() if fin.any() else 0.0
    last = int(out["last_out"][use].max())
    settled = -1 if not usable else 0 if last < 0 else -1 if last + 1 > T - R else last + 1
    return settled, out
