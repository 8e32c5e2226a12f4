"""float64 numpy restatement of mcx_samples_covariance and mcx_proposal_from_cov, for the tests.

N rows of np + 1 columns (the parameters, then log L): mean = column sum / N, cov = Xc^T Xc / (N - 1) with Xc the rows
centred on that mean (two passes, float64).  A column holding an inf or NaN is flagged, its mean and its row and column
of cov are NaN, and every other entry is computed as if the column were not there."""
import numpy as np

NONFINITE = 1


def restate(rows):
    """rows [N, ncol] float32 -> dict mean [ncol], cov [ncol, ncol], flags [ncol]"""
    x = np.asarray(rows, np.float32).astype(np.float64)
    N, ncol = x.shape
    fin = np.isfinite(x).all(axis=0)
    mean = np.full(ncol, np.nan)
    cov = np.full((ncol, ncol), np.nan)
    k = np.flatnonzero(fin)
    xf = x[:, k]
    m = xf.sum(axis=0) / N
    c = xf - m
    mean[k] = m
    cov[np.ix_(k, k)] = c.T @ c / (N - 1)
    return dict(mean=mean, cov=cov, flags=np.where(fin, 0, NONFINITE).astype(np.int32))


def bound(ref_cov, N):
    """the largest admissible |got - ref| per entry: 4 (N + 16) 2^-53 sqrt(ref_ii ref_jj).  Each centred factor and product
    is one fp64 rounding, a sum of N terms in any order errs by at most (N - 1) 2^-53 sum |a b|, and sum |a b| <=
    sqrt(sum a^2 sum b^2); the factor 4 covers the reference's own summation, the factors' roundings and the mean's error."""
    d = np.diag(ref_cov)
    return 4.0 * (N + 16) * 2.0 ** -53 * np.sqrt(np.outer(d, d))


def check(got, ref, N, where=""):
    """got: Engine.covariance() / rows_covariance(); ref: restate().  Returns the largest error / bound seen."""
    assert np.array_equal(got["flags"], ref["flags"]), (where, got["flags"], ref["flags"])
    bad = ref["flags"] != 0
    assert np.isnan(got["mean"][bad]).all() and np.isnan(got["cov"][bad, :]).all() and np.isnan(got["cov"][:, bad]).all(), where
    k = np.flatnonzero(~bad)
    g, r = got["cov"][np.ix_(k, k)], ref["cov"][np.ix_(k, k)]
    assert np.isfinite(g).all(), where
    np.testing.assert_allclose(got["mean"][k], ref["mean"][k], rtol=1e-9, atol=1e-300, err_msg=where)
    b = bound(r, N)
    err = np.abs(g - r)
    zero = b == 0  # a pair with a constant column: exactly 0
    assert (g[zero] == 0).all(), (where, "entries of a constant column", g[zero])
    ratio = float((err[~zero] / b[~zero]).max()) if (~zero).any() else 0.0
    assert ratio <= 1.0, (where, "largest error / bound", ratio, np.unravel_index(np.argmax(np.where(zero, 0, err / np.where(zero, 1, b))), b.shape))
    assert got["cov"].tobytes() == np.ascontiguousarray(got["cov"].T).tobytes(), (where, "cov[i][j] and cov[j][i] differ in bits")
    return ratio


def corr_of(cov):
    """cov_ij / sqrt(cov_ii cov_jj): NaN where a variance is 0 or NaN, exactly 1 on the diagonal otherwise"""
    v = np.diag(cov).copy()
    v[~(v > 0)] = np.nan
    s = np.sqrt(v)
    with np.errstate(invalid="ignore"):
        c = cov / np.outer(s, s)
    k = np.flatnonzero(~np.isnan(v))
    c[k, k] = 1.0
    return c


# ---- mcx_proposal_from_cov

def fmaf(a, b, c):
    """float32 fma(a, b, c), correctly rounded: the product of two float32 is exact in float64; the sum is rounded to odd
    in float64 (53 >= 2 * 24 + 2 bits), which makes the final rounding to float32 the rounding of the exact value"""
    p = float(np.float32(a)) * float(np.float32(b))
    c = float(np.float32(c))
    t = p + c
    if not np.isfinite(t):
        return np.float32(t)
    bb = t - p
    e = (p - (t - bb)) + (c - bb)  # TwoSum: p + c = t + e exactly
    if e != 0.0:
        bits = np.array([t], np.float64).view(np.int64)
        if not (int(bits[0]) & 1):
            t = float(np.nextafter(t, np.inf if e > 0 else -np.inf))
    return np.float32(t)


def cholesky_lower_f32(a):
    """the library's float Cholesky (cholesky_lower of mcx_engine.hip), operation by operation: 0 and the factor, or
    1 + the pivot that is not > 0"""
    a = np.array(a, np.float32)
    d = a.shape[0]
    for i in range(d):
        for j in range(i + 1):
            s = a[i, j]
            for k in range(j):
                s = fmaf(-a[i, k], a[j, k], s)
            if i == j:
                if not s > 0:
                    return i + 1, a
                a[i, i] = np.sqrt(np.float32(s))
            else:
                a[i, j] = np.float32(s) / a[j, j]
        a[i, i + 1:] = 0
    return 0, a


def proposal(cov, np_, scale=None):
    """(incov float32 [np_, np_], rc): scale * the parameter block, rounded to float32, the upper triangle mirrored; rc = 0
    when cholesky_lower_f32 accepts it, -1 for an entry that is not finite, else 1 + the failing pivot"""
    s = 2.38 * 2.38 / np_ if scale is None or scale <= 0 else float(scale)
    c = np.asarray(cov, np.float64)[:np_, :np_]
    with np.errstate(over="ignore", invalid="ignore"):
        f = (s * c).astype(np.float32)
    if not (np.isfinite(c).all() and np.isfinite(f).all()):
        return f, -1
    f = np.triu(f) + np.triu(f, 1).T
    return f, cholesky_lower_f32(f)[0]
