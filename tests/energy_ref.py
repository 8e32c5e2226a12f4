"""The joint comparison of two stores restated in float64 numpy and Python integers: the rows of each
side, the pooled scale and the dropped columns, every pairwise distance formed directly, the sums S, S_A, S_AA of every label
vector, the energy statistic and its permutation p-value.  Nothing here calls the library except draw_rows' index rule
(debug_draw_indices, section 12's own test subject)."""
import math

import numpy as np

import step_ref

ST_ENERGY = 6
COL_NONFINITE, COL_CONSTANT, COL_UNUSED = 1, 2, 4
EPS = 2.0 ** -53
NAN = float("nan")


def labels(seed, n_a, n_b, p):
    """the label vector of permutation p: a partial Fisher-Yates driven by Philox stream 6, in Python integers"""
    N = n_a + n_b
    out = np.zeros(N, np.uint8)
    if p == 0:
        out[:n_a] = 1
        return out
    w = step_ref.philox4x32(np.arange(n_a), p, 0, 0, seed, ST_ENERGY)
    idx = list(range(N))
    for i in range(n_a):
        r = (int(w[0][i]) << 32) | int(w[1][i])
        j = i + ((r * (N - i)) >> 64)
        idx[i], idx[j] = idx[j], idx[i]
        out[idx[i]] = 1
    return out


def side_rows(rows, n, seed, first):
    """the rows a side gives: n > 0 draws (draws first ... first + n - 1 of (seed, rows)), 0: min(rows, 2048) draws, -1: all"""
    from mcpar_amd import engine as E
    rows = np.asarray(rows, np.float32)
    if n == -1:
        return rows
    k = n if n > 0 else min(len(rows), 2048)
    return rows[E.debug_draw_indices(seed, len(rows), first, k)]


def scale_and_flags(pooled, with_ll=False, raw=False):
    N, ncol = pooled.shape
    x = pooled.astype(np.float64)
    scale, flags = np.full(ncol, NAN), np.zeros(ncol, np.int32)
    for c in range(ncol):
        if c == ncol - 1 and not with_ll:
            flags[c] = COL_UNUSED
            continue
        if not np.isfinite(x[:, c]).all():
            flags[c] = COL_NONFINITE
            continue
        m = math.fsum(x[:, c]) / N
        sd = math.sqrt(math.fsum((x[:, c] - m) ** 2) / (N - 1))
        scale[c] = 1.0 if raw else sd
        if not raw and sd == 0.0:
            flags[c] = COL_CONSTANT
    return scale, flags


def distances(z):
    """d[i, j] = sqrt(sum_c (z_ic - z_jc)^2), every difference formed directly"""
    N = len(z)
    d = np.zeros((N, N))
    for c in range(z.shape[1]):
        t = z[:, None, c] - z[None, :, c]
        d += t * t
    return np.sqrt(d)


def sums_of(d, lab):
    lab = lab.astype(np.float64)
    r = d.sum(axis=1)
    return float(r.sum()), float(lab @ r), float(lab @ d @ lab)


def energy_of(S, SA, SAA, n_a, n_b):
    SAB, SBB = SA - SAA, S - 2.0 * SA + SAA
    return 2.0 * SAB / (n_a * n_b) - SAA / (n_a * n_a) - SBB / (n_b * n_b)


def finish(S, SA, SAA, n_a, n_b):
    """SA, SAA [1 + P] -> the result's derived fields"""
    P = len(SA) - 1
    out = dict(mean_ab=(SA[0] - SAA[0]) / (n_a * n_b), mean_aa=SAA[0] / (n_a * n_a), mean_bb=(S - 2.0 * SA[0] + SAA[0]) / (n_b * n_b))
    out["e"] = 2.0 * out["mean_ab"] - out["mean_aa"] - out["mean_bb"]
    out["h"] = out["e"] / (2.0 * out["mean_ab"]) if out["mean_ab"] != 0.0 else NAN
    out["perm_e"] = np.array([energy_of(S, SA[p], SAA[p], n_a, n_b) for p in range(1, P + 1)], np.float64)
    out["nge"] = int((out["perm_e"] >= out["e"]).sum())
    out["p_value"] = (1 + out["nge"]) / (1 + P) if P > 0 else NAN
    return out


def restate(rows_a, rows_b, n_a=0, n_b=0, nperm=999, seed=0, with_ll=False, raw=False):
    """the whole call on host rows: energy_rows' dict plus S, S_A, S_AA [1 + nperm]"""
    a = side_rows(rows_a, n_a, seed, 0)
    b = side_rows(rows_b, n_b, seed, len(a))
    na, nb = len(a), len(b)
    pooled = np.concatenate([a, b])
    scale, flags = scale_and_flags(pooled, with_ll, raw)
    used = np.flatnonzero(flags == 0)
    out = dict(n_a=na, n_b=nb, nperm=nperm, nused=len(used), na_rows=len(rows_a), nb_rows=len(rows_b), scale=scale, flags=flags)
    if len(used) == 0:
        out.update(e=NAN, h=NAN, mean_ab=NAN, mean_aa=NAN, mean_bb=NAN, p_value=NAN, nge=0, perm_e=np.full(nperm, NAN), S=NAN,
                   SA=np.full(nperm + 1, NAN), SAA=np.full(nperm + 1, NAN))
        return out
    z = pooled[:, used].astype(np.float64) / scale[used]
    d = distances(z)
    r = d.sum(axis=1)
    L = np.stack([labels(seed, na, nb, p) for p in range(nperm + 1)]).astype(np.float64)
    S, SA = float(r.sum()), L @ r
    SAA = np.einsum("pi,pi->p", L @ d, L)
    out.update(S=S, SA=SA, SAA=SAA)
    out.update(finish(S, SA, SAA, na, nb))
    return out


def eps_of(N, ncol):
    """the relative bound of a sum: N^2 terms in any order, each with about ncol + 4 roundings"""
    return (N * N + ncol + 4) * EPS


def e_bound(ref, ncol):
    N = ref["n_a"] + ref["n_b"]
    return 16.0 * eps_of(N, ncol) * ref["S"] / min(ref["n_a"], ref["n_b"]) ** 2


def check(got, ref, ncol, sums=None):
    """got (energy_rows' dict; sums: debug_energy_sums' triple) against the restatement ref, by the rules of section 21.
    Returns the largest error / bound seen"""
    worst = 0.0
    for f in ("n_a", "n_b", "nperm", "nused", "na_rows", "nb_rows"):
        assert got[f] == ref[f], (f, got[f], ref[f])
    assert np.array_equal(got["flags"], ref["flags"]), (got["flags"], ref["flags"])
    N = ref["n_a"] + ref["n_b"]
    ok = ~np.isnan(ref["scale"])
    assert np.array_equal(np.isnan(got["scale"]), ~ok)
    assert (np.abs(got["scale"][ok] - ref["scale"][ok]) <= 4.0 * N * EPS * np.abs(ref["scale"][ok])).all(), (got["scale"], ref["scale"])
    P = ref["nperm"]
    assert got["perm_e"].shape == (P,)
    if ref["nused"] == 0:
        assert all(math.isnan(got[f]) for f in ("e", "h", "mean_ab", "mean_aa", "mean_bb", "p_value")) and got["nge"] == 0
        assert np.isnan(got["perm_e"]).all()
        if sums is not None:
            assert math.isnan(sums[0]) and np.isnan(sums[1]).all() and np.isnan(sums[2]).all()
        return worst
    eps = eps_of(N, ncol)
    if sums is not None:
        for g, r in ((np.array([sums[0]]), np.array([ref["S"]])), (sums[1], ref["SA"]), (sums[2], ref["SAA"])):
            assert g.shape == r.shape
            err = np.abs(g - r)
            assert (err <= 2.0 * eps * r).all(), (err.max(), (2.0 * eps * r).min())
            nz = r > 0
            if nz.any():
                worst = max(worst, float((err[nz] / (2.0 * eps * r[nz])).max()))
    bound = e_bound(ref, ncol)
    for f in ("e", "mean_ab", "mean_aa", "mean_bb"):
        assert abs(got[f] - ref[f]) <= bound, (f, got[f], ref[f], bound)
    if bound > 0:
        worst = max(worst, abs(got["e"] - ref["e"]) / bound)
    if ref["mean_ab"] != 0.0:
        # h = e / (2 mean_ab) <= 1: e moves by at most bound and 2 mean_ab by at most 2 bound
        assert abs(got["h"] - ref["h"]) <= 3.0 * bound / (2.0 * ref["mean_ab"]), (got["h"], ref["h"])
    else:
        assert math.isnan(got["h"])
    if P:
        err = np.abs(got["perm_e"] - ref["perm_e"])
        assert (err <= bound).all(), (err.max(), bound)
        if bound > 0:
            worst = max(worst, float(err.max() / bound))
    # nge and p_value: the definition applied to the returned perm_e; the reference's where none of its perm_e is near e
    nge = int((got["perm_e"] >= got["e"]).sum())
    assert got["nge"] == nge
    if P:
        assert got["p_value"] == (1 + nge) / (1 + P)
        if (np.abs(ref["perm_e"] - ref["e"]) > 2.0 * bound).all():
            assert got["nge"] == ref["nge"] and got["p_value"] == ref["p_value"]
    else:
        assert math.isnan(got["p_value"])
    return worst
