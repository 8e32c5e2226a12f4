"""DESIGN.md section 26 restated in numpy float64: the proposal's factors, log g with its forward error bound, the draws (the
engine's normals come from the CPU oracle's mcxo_normal4, the uniforms from its Philox), and the bridge with its error and
by-products.  Nothing here calls the library under test."""
import ctypes as C

import numpy as np

import oracle_lib as O

MAX_K = 8
STREAM = 8
NOT_CONVERGED, NO_ESS = 1, 2
LOG_2PI = float(np.log(2.0 * np.pi))
EPS = 2.0 ** -53


def proposal(weights, centres, covs, scale=1.0):
    """(C [k, np, np] lower Cholesky factors of scale^2 covs, W = their inverses, lc [k])"""
    w = np.asarray(weights, np.float64)
    covs = np.asarray(covs, np.float64)
    k, np_ = covs.shape[0], covs.shape[1]
    Cf = np.stack([np.linalg.cholesky(scale * scale * covs[j]) for j in range(k)])
    W = np.stack([np.linalg.inv(Cf[j]) for j in range(k)])
    W = np.tril(W)
    lc = np.array([np.log(w[j] / w.sum()) - np.log(np.diag(Cf[j])).sum() - 0.5 * np_ * LOG_2PI for j in range(k)])
    return Cf, W, lc


def logg(x, centres, W, lc):
    """(lg [n], bound [n]): log g of float rows x [n, np] and the forward bound of section 26 on |lg_device - lg|:
    max_k (4 np + 16) 2^-53 A_k / 2 + 16 2^-53 (1 + |lg|), A_k = sum_i (sum_l |W_il u_l|)^2.  A row with a non-finite
    parameter has lg = NaN"""
    x = np.asarray(x, np.float32)
    n, np_ = x.shape
    k = len(lc)
    xd = x.astype(np.float64)
    t = np.empty((k, n))
    A = np.empty((k, n))
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(k):
            u = xd - np.asarray(centres, np.float64)[j][None, :]
            z = u @ W[j].T
            t[j] = lc[j] - 0.5 * (z * z).sum(axis=1)
            az = np.abs(u) @ np.abs(W[j]).T
            A[j] = (az * az).sum(axis=1)
        mx = t.max(axis=0)
        lg = mx + np.log(np.exp(t - mx[None, :]).sum(axis=0))
    lg[~np.isfinite(xd).all(axis=1)] = np.nan
    bound = (4 * np_ + 16) * EPS * A.max(axis=0) / 2 + 16 * EPS * (1 + np.abs(lg))
    return lg, bound


def uniform(seed, j):
    """the uniform that picks the component of draw j: the top 53 bits of words x : y of Philox block (j, 0, 1, 0), key (seed, 8)"""
    w = O.philox((j, 0, 1, 0), (seed, STREAM))
    return float(((w[0] << 32) | w[1]) >> 11) * 2.0 ** -53


def normals(seed, j, np_):
    """z [4 ceil(np / 4)] of draw j: blocks b = 0 .. of counter (t = j, g = b, a = 0, q = 0), stream 8"""
    nb = (np_ + 3) // 4
    out = np.empty(4 * nb, np.float32)
    buf = (C.c_float * 4)()
    f = O.lib().mcxo_normal4
    for b in range(nb):
        f(seed, STREAM, j, b, 0, 0, buf)
        out[4 * b:4 * b + 4] = buf[:]
    return out


def draws(weights, centres, Cf, seed, n):
    """(x [n, np] float32, comp [n]): x_i = (float)(c_i + sum_{l <= i} C_il (double)z_l), the sum from 0.0 with l ascending, every
    product and sum rounded on its own"""
    w = np.asarray(weights, np.float64)
    centres = np.asarray(centres, np.float64)
    k, np_ = centres.shape
    cum = np.cumsum(w)  # (sequential in index order, as the library's)
    comp = np.empty(n, np.int32)
    z = np.empty((n, np_), np.float64)
    for j in range(n):
        target = uniform(seed, j) * cum[-1]
        c = k - 1
        for q in range(k - 1):
            if cum[q] > target:
                c = q
                break
        comp[j] = c
        z[j] = normals(seed, j, np_)[:np_].astype(np.float64)
    s = np.zeros((n, np_))
    for c in range(k):
        m = comp == c
        if not m.any():
            continue
        sc, zc = np.zeros((int(m.sum()), np_)), z[m]
        for col in range(np_):
            sc[:, col:] = sc[:, col:] + Cf[c][col:, col][None, :] * zc[:, col:col + 1]
        s[m] = centres[c][None, :] + sc
    return s.astype(np.float32), comp


def _num(a, r, s1, s2):
    out = np.empty_like(a)
    p = a >= 0
    with np.errstate(over="ignore"):
        out[p] = 1.0 / (s1 + s2 * r * np.exp(-a[p]))
        ea = np.exp(a[~p])
    out[~p] = ea / (s1 * ea + s2 * r)
    return out


def _den(a, r, s1, s2):
    out = np.empty_like(a)
    p = a >= 0
    ema = np.exp(-a[p])
    out[p] = ema / (s1 + s2 * r * ema)
    out[~p] = 1.0 / (s1 * np.exp(a[~p]) + s2 * r)
    return out


def _f1(d, s1, s2):
    out = np.empty_like(d)
    p = d >= 0
    out[p] = 1.0 / (s1 + s2 * np.exp(-d[p]))
    e = np.exp(d[~p])
    out[~p] = e / (s1 * e + s2)
    return out


def _f2(d, s1, s2):
    out = np.empty_like(d)
    p = d >= 0
    q = np.exp(-d[p])
    out[p] = q / (s1 + s2 * q)
    out[~p] = 1.0 / (s1 * np.exp(d[~p]) + s2)
    return out


def bridge(l1, l2, neff=None, ess_f2=None, tol=1e-10, max_iter=1000):
    """the estimator on l1 [n1] (rows) and l2 [n2] (draws; -inf = a draw with L = 0) -> dict.  neff, ess_f2 None: n1"""
    l1, l2 = np.asarray(l1, np.float64), np.asarray(l2, np.float64)
    n1, n2 = l1.size, l2.size
    if not np.isfinite(l1).all():
        raise ValueError("l1 is not finite")
    zero = np.isneginf(l2)
    if not np.isfinite(l2[~zero]).all():
        raise ValueError("l2 holds +inf or NaN")
    if zero.all():
        raise ValueError("every draw has L = 0")
    neff = float(min(n1 if neff is None else neff, n1))
    ess_f2 = float(n1 if ess_f2 is None else ess_f2)
    s1 = neff / (neff + n2)
    s2 = 1.0 - s1   # n2 / (neff + n2), formed as the library forms it: s1 + s2 is 1 in floating point
    lstar = float(l1.sum() / n1)
    r, logr, iters, flags = 1.0, 0.0, 0, 0
    while True:
        rn = (_num(l2 - lstar, r, s1, s2).sum() / n2) / (_den(l1 - lstar, r, s1, s2).sum() / n1)
        ln = float(np.log(rn))
        delta = abs(ln - logr)
        r, logr, iters = float(rn), ln, iters + 1
        if delta <= tol or delta != delta:
            break
        if iters >= max_iter:
            flags |= NOT_CONVERGED
            break
    log_z = logr + lstar
    f1, f2 = _f1(l2 - log_z, s1, s2), _f2(l1 - log_z, s1, s2)

    def half(f, n, ess):
        m = f.sum() / n
        var = ((f - m) ** 2).sum() / (n - 1) if n > 1 else 0.0
        return float(var / (m * m * ess))

    re2_draws, re2_rows = half(f1, n2, float(n2)), half(f2, n1, ess_f2)
    m2, m1 = float(l2[~zero].max()), float((-l1).max())
    return dict(n1=n1, n2=n2, neff=neff, lstar=lstar, log_z=log_z, se=float(np.sqrt(re2_draws + re2_rows)), re2_draws=re2_draws,
                re2_rows=re2_rows, ess_f2=ess_f2, log_z_is=m2 + float(np.log(np.exp(l2 - m2).sum() / n2)),
                log_z_ris=-(m1 + float(np.log(np.exp(-l1 - m1).sum() / n1))), ndraw_zero=int(zero.sum()), iters=iters, flags=flags,
                f2=f2)


# ---- the decisive inputs: MCX_VL_GAUSSMIX with d = 3, centres (0,0,0) and (6,6,6), weights 0.3 and 0.7 -> log Z = 1.5 log 2 pi
DEC_D, DEC_NC, DEC_T, DEC_N2 = 3, 16, 256, 2048
DEC_PARAMS = np.array([0, 0, 0, 6, 6, 6, 0.3, 0.7], np.float32)
DEC_TRUTH = 1.5 * LOG_2PI
DEC_SEEDS = (0, 1, 2, 3, 4)


def decisive_rows(seed):
    """4096 iid float rows of the target in 16 "chains" with the oracle's float log L: (rows [4096, 4], which component)"""
    rng = np.random.default_rng(1000 + seed)
    n = DEC_T * DEC_NC
    which = (rng.random(n) < 0.7).astype(np.int64)
    x = (rng.standard_normal((n, DEC_D)) + 6.0 * which[:, None]).astype(np.float32)
    ll = O.vl_eval(O.VL_GAUSSMIX, DEC_D, x, DEC_PARAMS, 2)
    return np.concatenate([x, ll[:, None]], axis=1).astype(np.float32), which


def decisive_proposal(rows, which, k):
    """(weights, centres, covs) from the first half of the rows: k = 1 the moments of all of them, k = 2 the moments per true
    component"""
    half = rows[:DEC_T // 2 * DEC_NC, :DEC_D].astype(np.float64)
    wh = which[:DEC_T // 2 * DEC_NC]
    if k == 1:
        return np.ones(1), half.mean(axis=0)[None, :], np.cov(half.T)[None, :, :]
    parts = [half[wh == c] for c in (0, 1)]
    return (np.array([len(p) / len(half) for p in parts]), np.stack([p.mean(axis=0) for p in parts]),
            np.stack([np.cov(p.T) for p in parts]))


def decisive_case(seed, k):
    """the reference alone on one case: (bridge's dict, l1, l2)"""
    rows, which = decisive_rows(seed)
    w, c, cov = decisive_proposal(rows, which, k)
    Cf, W, lc = proposal(w, c, cov)
    post = rows[DEC_T // 2 * DEC_NC:]
    l1 = post[:, DEC_D].astype(np.float64) - logg(post[:, :DEC_D], c, W, lc)[0]
    x, _ = draws(w, c, Cf, seed, DEC_N2)
    ll = O.vl_eval(O.VL_GAUSSMIX, DEC_D, x, DEC_PARAMS, 2).astype(np.float64)
    l2 = ll - logg(x, c, W, lc)[0]
    l2[~np.isfinite(ll)] = -np.inf
    return bridge(l1, l2), l1, l2
