"""float64 numpy restatement of mcx_samples_lagcov and mcx_mess_finish, for the tests.

Rows [T * nc, ncol] are step-major: row r is step r // nc of chain r % nc; the columns are the parameters, then log L.
  G(t)[i][j] = (1 / N) sum_c sum_{s < T - t} (x[c, s, i] - m_i) (x[c, s + t, j] - m_j),  m the column mean, N = T nc
  S(t) = (G(t) + G(t)^T) / 2, P(k) = S(2k) + S(2k + 1), Sigma_k = -S(0) + 2 sum_{i <= k} P(i), on the chosen columns
  the walk: s the first k <= K = (L - 1) // 2 (L the last lag) with Sigma_k positive definite; then k goes on while Sigma_k stays
  positive definite and its log-determinant grows; Sigma = Sigma_k_used
  mess = N exp((logdet Lambda - logdet Sigma) / p), Lambda = G(0) N / (N - 1); ess_j = N Lambda_jj / Sigma_jj; mcse_j =
  sqrt(Sigma_jj / N)
A column holding an inf or NaN is flagged NONFINITE: NaN mean, NaN row and column in every G(t), left out of Sigma.  A constant
column (G(0)_jj = 0) is flagged CONSTANT and left out of Sigma too."""
import numpy as np

NONFINITE, CONSTANT = 1, 2
NOT_PD, TRUNCATED, LAMBDA_SINGULAR = 1, 2, 4


def gamma_of(rows, T, nc, nlags):
    """G(0) .. G(nlags - 1) [nlags, ncol, ncol], the means [ncol] and the column flags (NONFINITE only)"""
    x = np.asarray(rows, np.float32).astype(np.float64).reshape(T, nc, -1)
    ncol = x.shape[2]
    N = T * nc
    fin = np.isfinite(x).all(axis=(0, 1))
    k = np.flatnonzero(fin)
    mean = np.full(ncol, np.nan)
    m = x[:, :, k].reshape(N, -1).sum(axis=0) / N
    mean[k] = m
    c = x[:, :, k] - m
    g = np.full((nlags, ncol, ncol), np.nan)
    for t in range(nlags):
        a, b = c[:T - t].reshape(-1, k.size), c[t:].reshape(-1, k.size)
        g[t][np.ix_(k, k)] = a.T @ b / N if t < T else 0.0
    return g, mean, np.where(fin, 0, NONFINITE).astype(np.int32)


def bound(g0, N):
    """the largest admissible |got - ref| per entry of any G(t): 4 (N + 16) 2^-53 sqrt(G(0)_ii G(0)_jj) -- covariance_ref.bound
    divided through by N, the lagged sum bounded by the lag-0 ones (Cauchy-Schwarz)"""
    d = np.diag(g0)
    return 4.0 * (N + 16) * 2.0 ** -53 * np.sqrt(np.outer(d, d))


def cholesky_logdet(m):
    """(True, log det m) when every pivot of the lower Cholesky factor is > 0, else (False, the pivots' index); the smallest and
    largest squared pivots ride along"""
    d = m.shape[0]
    L = np.zeros((d, d))
    piv = []
    for i in range(d):
        for j in range(i + 1):
            s = m[i, j] - float(L[i, :j] @ L[j, :j])
            if i == j:
                if not s > 0.0:
                    return False, i, piv
                piv.append(s)
                L[i, i] = np.sqrt(s)
            else:
                L[i, j] = s / L[j, j]
    return True, float(np.sum(np.log(piv))), piv


def finish(gamma, N, use):
    """the walk on G(0) .. G(nlags - 1).  A dict: p, s, k_used, lags_used, flags, mess, logdet_lambda, logdet_sigma, sigma
    [ncol, ncol], ess, mcse, col_flags [ncol], and what says whether the input is decisive: margins (|logdet Sigma_k - logdet
    Sigma_{k-1}| of every comparison the walk made) and pivot_ratio (the smallest squared pivot of Sigma_s over the largest)"""
    gamma = np.asarray(gamma, np.float64)
    nlags, ncol, _ = gamma.shape
    d0 = np.diag(gamma[0])
    col_flags = np.where(d0 == 0.0, CONSTANT, 0).astype(np.int32)
    idx = np.flatnonzero(np.asarray(use, bool) & (d0 > 0.0))
    p = idx.size
    out = dict(p=p, s=-1, k_used=-1, lags_used=0, flags=0, mess=np.nan, logdet_lambda=np.nan, logdet_sigma=np.nan,
               sigma=np.full((ncol, ncol), np.nan), ess=np.full(ncol, np.nan), mcse=np.full(ncol, np.nan), col_flags=col_flags,
               margins=[], pivot_ratio=np.nan)
    K = (nlags - 2) // 2
    if p == 0 or nlags < 2:
        out["flags"] |= NOT_PD
        return out
    S = [0.5 * (g[np.ix_(idx, idx)] + g[np.ix_(idx, idx)].T) for g in gamma]
    cur = -S[0]
    lam = S[0] * (N / (N - 1))
    best, ld_best, stopped = None, 0.0, False
    for k in range(K + 1):
        cur = cur + 2.0 * (S[2 * k] + S[2 * k + 1])
        pd, ld, piv = cholesky_logdet(cur)
        if out["s"] < 0:
            if not pd:
                continue
            out["s"] = k
            out["pivot_ratio"] = min(piv) / max(piv)
        else:
            if pd:
                out["margins"].append(abs(ld - ld_best))
            if not pd or not ld > ld_best:
                stopped = True
                break
        out["k_used"], ld_best, best = k, ld, cur
    if out["s"] < 0:
        out["flags"] |= NOT_PD
        return out
    if not stopped:
        out["flags"] |= TRUNCATED
    out["lags_used"] = 2 * out["k_used"] + 2
    out["logdet_sigma"] = ld_best
    pd, ldl, _ = cholesky_logdet(lam)
    if pd:
        out["logdet_lambda"] = ldl
        out["mess"] = N * np.exp((ldl - ld_best) / p)
    else:
        out["flags"] |= LAMBDA_SINGULAR
    out["sigma"][np.ix_(idx, idx)] = best
    out["ess"][idx] = N * np.diag(lam) / np.diag(best)
    out["mcse"][idx] = np.sqrt(np.diag(best) / N)
    return out


def use_of(col_flags, with_ll):
    use = np.asarray(col_flags) == 0
    if not with_ll:
        use[-1] = False
    return use


def restate(rows, T, nc, max_lag=None, with_ll=False):
    """the whole call on every lag 0 .. min(T - 1, max_lag): finish()'s dict with gamma, mean and the NONFINITE flags merged"""
    L = T - 1 if max_lag is None else min(T - 1, max_lag)
    g, mean, fl = gamma_of(rows, T, nc, L + 1)
    out = finish(g, T * nc, use_of(fl, with_ll))
    out.update(gamma=g, mean=mean, N=T * nc)
    out["col_flags"] = out["col_flags"] | fl
    return out


def ccf_of(gamma):
    """G(t)_ij / sqrt(G(0)_ii G(0)_jj): NaN where a variance is 0 or NaN, exactly 1 on the diagonal of lag 0 otherwise"""
    v = np.diag(gamma[0]).copy()
    v[~(v > 0)] = np.nan
    s = np.sqrt(v)
    with np.errstate(invalid="ignore"):
        c = gamma / np.outer(s, s)
    k = np.flatnonzero(~np.isnan(v))
    c[0, k, k] = 1.0
    return c


def check_finish(got, ref, rtol=1e-9, where=""):
    """the integers exact, the floats within rtol; got: the library's dict (mess_finish / lagcov), ref: finish()'s"""
    for f in ("p", "s", "k_used", "lags_used"):
        assert got[f] == ref[f], (where, f, got[f], ref[f])
    assert got["flags"] == ref["flags"], (where, "flags", got["flags"], ref["flags"])
    for f in ("mess", "logdet_lambda", "logdet_sigma"):
        np.testing.assert_allclose(got[f], ref[f], rtol=rtol, atol=0, equal_nan=True, err_msg=where + f)
    for f in ("ess", "mcse"):
        np.testing.assert_allclose(got[f], ref[f], rtol=rtol, atol=0, equal_nan=True, err_msg=where + f)
    assert np.array_equal(np.isnan(got["sigma"]), np.isnan(ref["sigma"])), (where, "the NaN pattern of sigma")
    scale = np.sqrt(np.abs(np.outer(np.diag(ref["sigma"]), np.diag(ref["sigma"]))))
    ok = ~np.isnan(ref["sigma"])
    assert (np.abs(got["sigma"] - ref["sigma"])[ok] <= rtol * scale[ok]).all(), (where, "sigma")


def decisive(ref):
    """the condition on an input that makes the walk's integers safe to compare exactly"""
    return all(m > 1e-6 for m in ref["margins"]) and (ref["s"] < 0 or ref["pivot_ratio"] > 1e-6)


# ---- the rows and shapes the tests share
SHAPES = [(1, 2, 8), (3, 5, 16), (16, 37, 48), (17, 37, 64), (40, 8, 96), (3, 7, 5)]  # (np, nc, T); the last: 35 rows, a unit and 3


def dependent_rows(np_, nc, T, seed=11, stay=0.7):
    """tests/test_gpu_intervals.py's Metropolis-like rows with column 1 made to depend on column 0: the matrices are not diagonal"""
    from test_gpu_intervals import make_rows
    rows = make_rows(np_, nc, T, seed=seed, stay=stay)
    if np_ > 1:
        rows[:, 1] = (rows[:, 1] + np.float32(0.5) * rows[:, 0]).astype(np.float32)
    return rows


def antithetic_rows(ncol, nc, T, phi=-0.9, seed=5):
    """ncol independent AR(1) columns with coefficient phi, started in their stationary law"""
    rng = np.random.default_rng([seed, ncol, nc, T])
    x = np.empty((T, nc, ncol))
    x[0] = rng.normal(0.0, 1.0 / np.sqrt(1.0 - phi * phi), (nc, ncol))
    for t in range(1, T):
        x[t] = phi * x[t - 1] + rng.normal(0.0, 1.0, (nc, ncol))
    return x.reshape(T * nc, ncol).astype(np.float32)


def same(a, b):
    """two dicts of the library hold the same bytes (NaN equal to NaN)"""
    def eq(u, v):
        u, v = np.asarray(u), np.asarray(v)
        return u.dtype == v.dtype and u.shape == v.shape and np.array_equal(u, v, equal_nan=u.dtype.kind == "f")
    return sorted(a) == sorted(b) and all(eq(a[k], b[k]) for k in a)
