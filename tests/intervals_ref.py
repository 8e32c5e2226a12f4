"""float64 numpy restatement of mcx_samples_intervals, for the tests, on top of tests/summary_ref.py.

Every definition is the one include/mcx.h writes out.  A column's sorted values s follow the key order of the rank summary (-0 and
+0 one value, reported as +0; every NaN last).  The beta quantiles are scipy's (boost's ibeta_inv), which the library's own
mcx_beta_quantile is held to in tests/test_intervals_cpu.py."""
import math

import numpy as np

import summary_ref as S

P_LO, P_HI = 0.1586553, 0.8413447


def sorted_values(x):
    """the float32 values of x in the key order of section 11"""
    x = np.asarray(x, np.float32).reshape(-1).copy()
    x[x == 0] = np.float32(0.0)  # -0 and +0 are one value
    return S.key_float(np.sort(S.okey(x)))


def hdi_span(p, N):
    return min(int(math.floor(float(p) * float(N))), N - 1)


def hdi(srt, p):
    """arviz's _hdi on sorted values: (lo, hi, width, index, span), the first of the narrowest windows"""
    N = srt.size
    m = hdi_span(p, N)
    with np.errstate(invalid="ignore"):  # (inf - inf in a column that is refused anyway)
        w = srt[m:].astype(np.float64) - srt[:N - m].astype(np.float64)
    i = int(np.argmin(w))  # (the first occurrence of the minimum)
    return srt[i], srt[i + m], float(w[i]), i, m


def hdi_brute(srt, p):
    """the same by a loop over every window, one Python float subtraction each"""
    N = len(srt)
    m = min(int(math.floor(p * N)), N - 1)
    best = None
    for i in range(N - m):
        w = float(srt[i + m]) - float(srt[i])
        if best is None or w < best[0]:
            best = (w, i)
    return srt[best[1]], srt[best[1] + m], best[0], best[1], m


def mcse_sd(N, mean_c2, sd_c2, ess):
    return math.sqrt((N - 1) / N * sd_c2 ** 2 / ess / mean_c2 / 4)


def mcse_sd_posterior(x, ess):
    """posterior::mcse_sd's expression in float64 throughout, the effective size given"""
    c = np.asarray(x, np.float64).reshape(-1)
    c = c - c.mean()
    evar = np.mean(c ** 2)
    return math.sqrt((np.mean(c ** 4) - evar ** 2) / ess / evar / 4)


def quantile_ranks(N, prob, ess):
    """(u_lo, u_hi, k_lo, k_hi) with scipy's beta quantiles; NaN and -1 for an ess that is not a positive finite number"""
    from scipy.stats import beta
    if not (ess > 0 and math.isfinite(ess)):
        return math.nan, math.nan, -1, -1
    a, b = ess * prob + 1, ess * (1 - prob) + 1
    u_lo, u_hi = float(beta.ppf(P_LO, a, b)), float(beta.ppf(P_HI, a, b))
    return u_lo, u_hi, max(math.floor(u_lo * N), 1) - 1, min(math.ceil(u_hi * N), N) - 1


def rank_margin(N, prob, ess):
    """how far u_lo N and u_hi N lie from an integer: a case is decided by scipy's u only when this is clear of the error of u"""
    u_lo, u_hi, _, _ = quantile_ranks(N, prob, ess)
    return min(abs(v * N - round(v * N)) for v in (u_lo, u_hi))


def restate_column(x, masses, probs):
    """x [nsteps, nc] float32: the intervals of one column as a dict"""
    T, nc = x.shape
    N = T * nc
    srt = sorted_values(x)
    base = S.restate_column(x, probs)
    r = dict(flags=base["flags"], mean=base["mean"], sd=base["sd"], sorted=srt, hdi=[], quantiles=[])
    bad = bool(base["flags"])
    for p in masses:
        lo, hi, w, i, m = hdi(srt, p)
        r["hdi"].append(dict(lo=np.float32(np.nan), hi=np.float32(np.nan), width=math.nan, index=-1, span=m) if bad else
                        dict(lo=lo, hi=hi, width=w, index=i, span=m))
    if bad:
        r.update(ess_sd=math.nan, mcse_sd=math.nan, ess_sd_lag=0)
        for p in probs:
            r["quantiles"].append(dict(q=math.nan, ess_q=math.nan, ess_q_lag=0))
        return r
    xd = x.astype(np.float64)
    with np.errstate(over="ignore"):
        c2 = ((xd - base["mean"]) ** 2).astype(np.float32)
    rc = S.restate_column(c2, ())
    r.update(ess_sd=rc["ess"], ess_sd_lag=rc["ess_lag"])
    r["mcse_sd"] = math.nan if math.isnan(rc["ess"]) else mcse_sd(N, rc["mean"], rc["sd"], rc["ess"])
    for k, p in enumerate(probs):
        q = float(base["quantiles"][k])
        ri = S.restate_column((xd <= q).astype(np.float32), ())
        r["quantiles"].append(dict(q=q, ess_q=ri["ess"], ess_q_lag=ri["ess_lag"]))
    return r


def restate(rows, nsteps, nc, masses, probs):
    """rows [nsteps * nc, np + 1] (MCout layout): one dict per column"""
    ncol = rows.shape[1]
    x = rows.reshape(nsteps, nc, ncol)
    return [restate_column(np.ascontiguousarray(x[:, :, c]), masses, probs) for c in range(ncol)]


def same_double(got, want, where):
    if math.isnan(want):
        assert math.isnan(got), (where, got)
    else:
        assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (where, got, want)


def check(got, ref, probs, rel_ess=1e-4, rel_mcse_sd=2e-4):
    """assert the GPU's dict (Engine.intervals) against restate()'s list.  HDI fields bit for bit; ess within rel_ess with exact
    lags; the ranks by the reference rule on the ess returned; s and mcse_q exactly those of the reference's sorted column"""
    N = ref[0]["sorted"].size
    for c, r in enumerate(ref):
        where = "column %d" % c
        assert got["flags"][c] == r["flags"], where
        for j, h in enumerate(r["hdi"]):
            g = {k: got["hdi"][k][c, j] for k in got["hdi"]}
            assert (g["index"], g["span"]) == (h["index"], h["span"]), (where, j, g, h)
            S.same_float(g["lo"], h["lo"], (where, j, "lo"))
            S.same_float(g["hi"], h["hi"], (where, j, "hi"))
            same_double(g["width"], h["width"], (where, j, "width"))
        if r["flags"]:
            for f in ("mean", "sd", "ess_sd", "mcse_sd"):
                assert math.isnan(got[f][c]), (where, f)
            for f in ("q", "ess_q", "u_lo", "u_hi", "mcse_q", "s_lo", "s_hi"):
                assert np.isnan(got["quantiles"][f][c]).all(), (where, f)
            assert (got["quantiles"]["k_lo"][c] == -1).all() and (got["quantiles"]["k_hi"][c] == -1).all(), where
            continue
        np.testing.assert_allclose(got["mean"][c], r["mean"], rtol=1e-9, atol=1e-300, err_msg=where)
        np.testing.assert_allclose(got["sd"][c], r["sd"], rtol=1e-9, err_msg=where)
        if math.isnan(r["ess_sd"]):
            assert math.isnan(got["ess_sd"][c]) and math.isnan(got["mcse_sd"][c]), where
        else:
            assert got["ess_sd_lag"][c] == r["ess_sd_lag"], (where, got["ess_sd_lag"][c], r["ess_sd_lag"])
            np.testing.assert_allclose(got["ess_sd"][c], r["ess_sd"], rtol=rel_ess, err_msg=where)
            np.testing.assert_allclose(got["mcse_sd"][c], r["mcse_sd"], rtol=rel_mcse_sd, err_msg=where)
        for k, (p, rq) in enumerate(zip(probs, r["quantiles"])):
            g = {f: got["quantiles"][f][c, k] for f in got["quantiles"]}
            wk = (where, "prob", p)
            np.testing.assert_allclose(g["q"], rq["q"], rtol=1e-12, atol=0, err_msg=str(wk))
            if math.isnan(rq["ess_q"]):  # the indicator is constant within every half-chain
                assert math.isnan(g["ess_q"]) and math.isnan(g["mcse_q"]) and math.isnan(g["u_lo"]) and math.isnan(g["u_hi"]), wk
                assert np.isnan(g["s_lo"]) and np.isnan(g["s_hi"]) and (g["k_lo"], g["k_hi"]) == (-1, -1), wk
                continue
            assert g["ess_q_lag"] == rq["ess_q_lag"], (wk, g["ess_q_lag"], rq["ess_q_lag"])
            np.testing.assert_allclose(g["ess_q"], rq["ess_q"], rtol=rel_ess, err_msg=str(wk))
            u_lo, u_hi, k_lo, k_hi = quantile_ranks(N, p, float(g["ess_q"]))
            print("%s prob %g: ess_q %.6g, u N = %.6f, %.6f" % (where, p, g["ess_q"], u_lo * N, u_hi * N))
            assert (g["k_lo"], g["k_hi"]) == (k_lo, k_hi), (wk, g, k_lo, k_hi)
            assert abs(g["u_lo"] - u_lo) * N < 1e-3 and abs(g["u_hi"] - u_hi) * N < 1e-3, (wk, g, u_lo, u_hi)
            S.same_float(g["s_lo"], r["sorted"][k_lo], (wk, "s_lo"))
            S.same_float(g["s_hi"], r["sorted"][k_hi], (wk, "s_hi"))
            same_double(g["mcse_q"], (float(r["sorted"][k_hi]) - float(r["sorted"][k_lo])) / 2, (wk, "mcse_q"))
