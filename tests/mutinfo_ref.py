"""The mutual information between columns of a store restated in float64 numpy and Python integers: the
rows taken, the scale and flags, the repeated rows dropped, z, the permutations, every pairwise distance formed directly, eps, na,
nb, the digamma table and the estimate with its null.  Nothing here calls the library."""
import math

import numpy as np

import step_ref

ST_MUTINFO = 9
COL_NONFINITE, COL_CONSTANT, COL_UNUSED = 1, 2, 4
PAIR_UNUSED, PAIR_FEW, PAIR_TIES = 1, 2, 4
MAX_ROWS, MAX_PERM, MAX_K, MAX_PAIRS = 16384, 999, 8, 1024
GAMMA = 0.57721566490153286060651209008240243
EPS = 2.0 ** -53
NAN = float("nan")


def row_index(N, n):
    """the n rows taken of N: floor(i N / n), in Python integers"""
    return np.array([(i * N) // n for i in range(n)], np.int64)


def n_of(n, N):
    return n if n > 0 else min(N, 4096) if n == 0 else N


def perm(seed, m, p):
    """pi_p on [0, m): the identity, or a full Fisher-Yates driven by Philox stream 9, in Python integers"""
    idx = list(range(m))
    if p == 0 or m < 2:
        return np.array(idx, np.int64)
    w = step_ref.philox4x32(np.arange(m - 1), p, 0, 0, seed, ST_MUTINFO)
    for i in range(m - 1):
        r = (int(w[0][i]) << 32) | int(w[1][i])
        j = i + ((r * (m - i)) >> 64)
        idx[i], idx[j] = idx[j], idx[i]
    return np.array(idx, np.int64)


def psi_table(q_max):
    """table[q - 1] = psi(q) = H_{q-1} - gamma, H by cumsum in index order"""
    h = np.concatenate([[0.0], np.cumsum(1.0 / np.arange(1, q_max, dtype=np.float64))])[:q_max]
    return h - GAMMA


def scale_and_flags(sel, with_ll=False, raw=False):
    n, ncol = sel.shape
    x = sel.astype(np.float64)
    scale, flags = np.full(ncol, NAN), np.zeros(ncol, np.int32)
    for c in range(ncol):
        if c == ncol - 1 and not with_ll:
            flags[c] = COL_UNUSED
            continue
        if not np.isfinite(x[:, c]).all():
            flags[c] = COL_NONFINITE
            continue
        mean = math.fsum(x[:, c]) / n
        sd = math.sqrt(math.fsum((x[:, c] - mean) ** 2) / (n - 1))
        scale[c] = 1.0 if raw else sd
        if not raw and sd == 0.0:
            flags[c] = COL_CONSTANT
    return scale, flags


def kept_rows(sel, flags):
    """kept[n]: 0 where an earlier selected row equals this one (float ==) in every column without a flag"""
    used = np.flatnonzero(flags == 0)
    kept = np.ones(len(sel), np.uint8)
    if len(used):
        key = sel[:, used] + np.float32(0.0)  # -0 == +0
        _, first = np.unique(key, axis=0, return_index=True)
        kept[:] = 0
        kept[first] = 1
    return kept


def points(rows, n=0, with_ll=False, raw=False, scale=None):
    """the host half: index, kept, scale, flags, z [ncol, m].  scale: the library's, once held to this one's (z is x / scale, and
    the kernel's integers are compared exactly, so both sides divide by the same bits)"""
    rows = np.asarray(rows, np.float32)
    N = len(rows)
    index = row_index(N, n_of(n, N))
    sel = rows[index]
    own, flags = scale_and_flags(sel, with_ll, raw)
    kept = kept_rows(sel, flags)
    use = own if scale is None else np.asarray(scale, np.float64)
    pts = sel[kept == 1].astype(np.float64)
    z = np.zeros((rows.shape[1], len(pts)))
    for c in np.flatnonzero(flags == 0):
        z[c] = pts[:, c] / use[c]
    return dict(n_rows=N, n_sel=len(sel), index=index, kept=kept, ndup=int((kept == 0).sum()), m=len(pts), scale=own, flags=flags, z=z,
                nused=int((flags == 0).sum()))


def counts(u, v, k):
    """eps, na, nb [m] of the points (u_i, v_i): every difference formed directly, j = i left out by index"""
    m = len(u)
    da = np.abs(u[:, None] - u[None, :])
    db = np.abs(v[:, None] - v[None, :])
    ii = np.arange(m)
    da[ii, ii] = np.inf
    db[ii, ii] = np.inf
    d = np.maximum(da, db)
    eps = np.partition(d, k - 1, axis=1)[:, k - 1]
    na = (da < eps[:, None]).sum(axis=1).astype(np.int32)
    nb = (db < eps[:, None]).sum(axis=1).astype(np.int32)
    return eps, na, nb


def finish(eps, na, nb, k):
    """the library's own order (mutinfo_finish is held to this bit for bit): the sum over i in index order, a point's two table
    values added first; then psi(k) + psi(m) - sum / m"""
    m = len(eps)
    t = psi_table(m)
    s = 0.0
    for a, b in zip(t[na], t[nb]):
        s += a + b
    return (t[k - 1] + t[m - 1]) - s / m, int((eps == 0.0).sum())


def mi_exact(na, nb, k):
    """mi with the sum by fsum, and T = sum |psi terms| for the bound"""
    m = len(na)
    t = psi_table(m)
    s = math.fsum(np.concatenate([t[na], t[nb]]))
    T = math.fsum(np.abs(np.concatenate([t[na], t[nb]])))
    return (t[k - 1] + t[m - 1]) - s / m, T


def mi_bound(m, k, T):
    """|mi - mi_exact| for any fixed-order fp64 sum of the 2 m table values: the sum errs by at most (2 m - 1) u T to first order
    (u = 2^-53; + 1 for fsum's own rounding, + 2 for the second-order terms, which are below 2 m u of the first), so its share
    after / m is (2 m + 2) u T / m; the two divisions round once each, u T / m each; psi(k) + psi(m) is the same operation on the
    same bits on both sides; the two final subtractions round once each, by at most u (|psi(k) + psi(m)| + T / m)"""
    t = psi_table(m)
    return (2 * m + 6) * EPS * T / m + 2.0 * EPS * abs(t[k - 1] + t[m - 1])


def r_info(mi):
    return math.sqrt(1.0 - math.exp(-2.0 * max(mi, 0.0)))


def pearson(a, b):
    ma, mb = math.fsum(a) / len(a), math.fsum(b) / len(b)
    ta, tb = a - ma, b - mb
    den = math.sqrt(math.fsum(ta * ta) * math.fsum(tb * tb))
    return math.fsum(ta * tb) / den if den > 0.0 else NAN  # (a column without spread, which raw lets through)


def pair_list(ncol, pairs, with_ll):
    if pairs is not None:
        return [tuple(int(x) for x in p) for p in np.asarray(pairs).reshape(-1, 2)]
    U = ncol - (0 if with_ll else 1)
    return [(a, b) for a in range(U) for b in range(a + 1, U)]


def restate(rows, n=0, k=0, nperm=0, seed=0, pairs=None, with_ll=False, raw=False, scale=None):
    """the whole call on host rows: rows_mutual_info's dict plus, per pair, bound (of mi) and perm_bound [nperm]"""
    k = k or 3
    P = points(rows, n, with_ll, raw, scale)
    m, z = P["m"], P["z"]
    plist = pair_list(np.asarray(rows).shape[1], pairs, with_ll)
    out = dict(n_rows=P["n_rows"], n_sel=P["n_sel"], ndup=P["ndup"], m=m, k=k, npairs=len(plist), nperm=nperm, nused=P["nused"],
               scale=P["scale"], flags=P["flags"], pairs=[], perm_mi=np.full((len(plist), nperm), NAN))
    perms = [perm(seed, m, p) for p in range(nperm + 1)]
    out.update(z=z, perms=perms)
    for i, (a, b) in enumerate(plist):
        o = dict(a=a, b=b, mi=NAN, r_info=NAN, pearson=NAN, perm_mean=NAN, perm_sd=NAN, p_value=NAN, nge=0, nzero=0, flags=0, bound=0.0,
                 perm_bound=np.zeros(nperm))
        if P["flags"][a] or P["flags"][b]:
            o["flags"] |= PAIR_UNUSED
        if m <= k:
            o["flags"] |= PAIR_FEW
        out["pairs"].append(o)
        if o["flags"]:
            continue
        for p in range(nperm + 1):
            eps, na, nb = counts(z[a], z[b][perms[p]], k)
            mi, T = mi_exact(na, nb, k)
            if p == 0:
                o.update(mi=mi, bound=mi_bound(m, k, T), nzero=int((eps == 0.0).sum()), eps=eps, na=na, nb=nb)
            else:
                out["perm_mi"][i, p - 1] = mi
                o["perm_bound"][p - 1] = mi_bound(m, k, T)
        if o["nzero"]:
            o["flags"] |= PAIR_TIES
        o["r_info"] = r_info(o["mi"])
        o["pearson"] = pearson(z[a], z[b])
        if nperm:
            pm = out["perm_mi"][i]
            o["perm_mean"] = math.fsum(pm) / nperm
            o["perm_sd"] = math.sqrt(math.fsum((pm - o["perm_mean"]) ** 2) / (nperm - 1)) if nperm > 1 else NAN
            o["nge"] = int((pm >= o["mi"]).sum())
            o["p_value"] = (1 + o["nge"]) / (1 + nperm)
    return out


def close_or_nan(got, want, tol):
    return (math.isnan(got) and math.isnan(want)) or abs(got - want) <= tol


def counts_of(ref, pair, p):
    """eps, na, nb of pair `pair` of the restatement ref under permutation p"""
    o = ref["pairs"][pair]
    return counts(ref["z"][o["a"]], ref["z"][o["b"]][ref["perms"][p]], ref["k"])


def flat(got):
    """rows_mutual_info's dict with the pair records as one array per field: plain arrays, for the byte comparisons"""
    out = {f: np.array(v) for f, v in got.items() if f != "pairs"}
    for f in got["pairs"].dtype.names:
        out["pair_" + f] = got["pairs"][f].copy()
    return out


def check(got, ref):
    """got (rows_mutual_info's dict) against the restatement ref made with got's scale, by the rules of section 28.  Returns the
    largest error / bound seen among mi and perm_mi"""
    worst = 0.0
    for f in ("n_rows", "n_sel", "ndup", "m", "k", "npairs", "nperm", "nused"):
        assert got[f] == ref[f], (f, got[f], ref[f])
    assert np.array_equal(got["flags"], ref["flags"]), (got["flags"], ref["flags"])
    ok = ~np.isnan(ref["scale"])
    assert np.array_equal(np.isnan(got["scale"]), ~ok)
    n, m, P = ref["n_sel"], ref["m"], ref["nperm"]
    assert (np.abs(got["scale"][ok] - ref["scale"][ok]) <= 4.0 * n * EPS * np.abs(ref["scale"][ok])).all(), (got["scale"], ref["scale"])
    assert len(got["pairs"]) == len(ref["pairs"]) and got["perm_mi"].shape == (len(ref["pairs"]), P)
    for i, r in enumerate(ref["pairs"]):
        g = got["pairs"][i]
        for f in ("a", "b", "flags", "nzero"):
            assert int(g[f]) == r[f], (i, f, g[f], r[f])
        if r["flags"] & (PAIR_UNUSED | PAIR_FEW):
            assert all(math.isnan(g[f]) for f in ("mi", "r_info", "pearson", "perm_mean", "perm_sd", "p_value")) and g["nge"] == 0
            assert np.isnan(got["perm_mi"][i]).all()
            continue
        err = abs(g["mi"] - r["mi"])
        assert err <= r["bound"], (i, g["mi"], r["mi"], r["bound"])
        worst = max(worst, err / r["bound"])
        # r_info: the definition applied to the returned mi; w = 1 - exp(.) errs by at most 2 u (exp's rounding and its own), the
        # root by that over 2 sqrt(w), and rounds once
        rd = r_info(float(g["mi"]))
        assert abs(g["r_info"] - rd) <= 2.0 * EPS / max(rd, math.sqrt(2.0 * EPS)) + 2.0 * EPS * rd, (g["r_info"], rd)
        # pearson: five sequential sums of m terms, two of them the means inside the other three: below (8 m + 32) u of 1
        assert close_or_nan(g["pearson"], r["pearson"], (8 * m + 32) * EPS), (g["pearson"], r["pearson"])
        pm = got["perm_mi"][i]
        if P:
            perr = np.abs(pm - ref["perm_mi"][i])
            assert (perr <= r["perm_bound"]).all(), (i, perr.max(), r["perm_bound"].min())
            worst = max(worst, float((perr / r["perm_bound"]).max()))
            big = float(np.abs(pm).max())
            mean = math.fsum(pm) / P
            assert abs(g["perm_mean"] - mean) <= (P + 4) * EPS * big
            if P > 1:
                sd = math.sqrt(math.fsum((pm - mean) ** 2) / (P - 1))
                assert abs(g["perm_sd"] - sd) <= (4 * P + 16) * EPS * big, (g["perm_sd"], sd)
            else:
                assert math.isnan(g["perm_sd"])
            # nge and p_value: the definition applied to the returned perm_mi; the reference's where none of its values is near mi
            nge = int((pm >= g["mi"]).sum())
            assert g["nge"] == nge and g["p_value"] == (1 + nge) / (1 + P)
            if (np.abs(ref["perm_mi"][i] - r["mi"]) > 2.0 * np.maximum(r["perm_bound"], r["bound"])).all():
                assert g["nge"] == r["nge"] and g["p_value"] == r["p_value"]
        else:
            assert g["nge"] == 0 and all(math.isnan(g[f]) for f in ("perm_mean", "perm_sd", "p_value"))
    return worst
