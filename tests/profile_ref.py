"""DESIGN.md section 27 restated in numpy / Python float64: the order of log L as a key, the grid of a column, the bins with
their maximum keys and counts, the curve, the least concave majorant, the intervals, the cells of a pair.  Nothing here calls
the library under test.  Every fp64 expression has the operands and the order of the definition, so that the library can be
held to it bit for bit where the definition is exact and to 1e-12 where a libm function enters (the levels)."""
import math

import numpy as np

N_MIN, N_MAX, G_MIN, G_MAX, MAX_LEVELS = 2, 512, 8, 64, 8
DEFAULT_LEVELS = (0.6827, 0.9545)
NONFINITE, LL_NONFINITE, OPEN_LO, OPEN_HI, NO_BIN, HULL_OPEN_LO, HULL_OPEN_HI = 1, 2, 4, 8, 16, 32, 64
INTERVAL_DTYPE = np.dtype([("p", np.float64), ("drop", np.float64), ("lo", np.float64), ("hi", np.float64), ("lo_hull", np.float64),
                           ("hi_hull", np.float64), ("nseg", np.int32), ("flags", np.int32)], align=True)


# ---- the order of log L ---------------------------------------------------------------------------------------------------------
def ll_key(l):
    """k(l) = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000) of float32 l, a NaN counted as -inf"""
    l = np.asarray(l, np.float32).copy()
    l[np.isnan(l)] = -np.inf
    b = l.view(np.uint32)
    return b ^ np.where(b >> 31, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def key_ll(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def row_keys(ll):
    """K(r) = k(l_r) << 32 | (0xFFFFFFFF - r) of every row"""
    r = np.arange(ll.size, dtype=np.uint64)
    return (ll_key(ll).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - r)


def key_row(K):
    K = np.asarray(K, np.uint64)
    return np.where(K == 0, -1, (np.uint64(0xFFFFFFFF) - (K & np.uint64(0xFFFFFFFF))).astype(np.int64))


def key_lmax(K):
    K = np.asarray(K, np.uint64)
    return np.where(K == 0, np.float32(-np.inf), key_ll((K >> np.uint64(32)).astype(np.uint32))).astype(np.float32)


# ---- levels -----------------------------------------------------------------------------------------------------------------------
_A = (2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4,
      1.3731693765509461125e+4, 1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e+0)
_B = (5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4,
      5.3941960214247511077e+3, 6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0)
_C = (7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e+0,
      3.64784832476320460504e+0, 5.76949722146069140550e+0, 4.63033784615654529590e+0, 1.42343711074968357734e+0)
_D = (1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
      6.89767334985100004550e-1, 1.67638483018380384940e+0, 2.05319162663775882187e+0, 1.0)
_E = (2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2,
      2.96560571828504891230e-1, 1.78482653991729133580e+0, 5.46378491116411436990e+0, 6.65790464350110377720e+0)
_F = (2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
      1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0)


def _horner(c, r):
    acc = c[0]
    for k in c[1:]:
        acc = acc * r + k
    return acc


def normal_quantile(p):
    """Wichura's AS 241, routine PPND16, as the definition names it (Applied Statistics 37, 1988): Horner with the highest power
    first, numerator and denominator apart, one division.  test_profile_cpu.py holds it to erfc"""
    q = p - 0.5
    if abs(q) <= 0.425:
        r = 0.180625 - q * q
        return _horner(_A, r) * q / _horner(_B, r)
    r = math.sqrt(-math.log(p if q <= 0.0 else 1.0 - p))
    if r <= 5.0:
        r -= 1.6
        x = _horner(_C, r) / _horner(_D, r)
    else:
        r -= 5.0
        x = _horner(_E, r) / _horner(_F, r)
    return -x if q < 0.0 else x


def drop_1d(p):
    z = normal_quantile((1.0 + p) / 2.0)
    return 0.5 * z * z


def drop_2d(p):
    return -math.log(1.0 - p)


# ---- the grid and the bins ----------------------------------------------------------------------------------------------------
def quantile7(sorted_vals, p):
    """section 9's type-7 quantile of a sorted float32 column"""
    N = sorted_vals.size
    h = (N - 1) * p
    lo = math.floor(h)
    g = h - lo
    a, b = float(sorted_vals[min(lo, N - 1)]), float(sorted_vals[min(lo + 1, N - 1)])
    return a if (g == 0.0 or a == b) else a + g * (b - a)


def grid_of(v, bins, clip=(0, 1), from_=None, to=None):
    """(from, to, inv) of a finite float32 column v"""
    f, t = float(v.min()), float(v.max())
    if tuple(clip) != (0, 1):
        s = np.sort(v)
        f, t = quantile7(s, clip[0]), quantile7(s, clip[1])
    if from_ is not None and not math.isnan(from_):
        f = float(from_)
    if to is not None and not math.isnan(to):
        t = float(to)
    assert f <= t
    with np.errstate(divide="ignore"):
        inv = float(np.float64(bins) / np.float64(t - f))
    return f, t, inv


def bins_of(v, bins, f, t, inv):
    """the bin of every value of float32 v, -1 for a dropped one"""
    d = v.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        xp = (d - f) * inv
    ib = np.full(v.size, -1, np.int64)
    ok = (xp >= 0.0) & (xp < float(bins))
    ib[ok] = np.floor(xp[ok]).astype(np.int64)
    ib[d == t] = 0 if f == t else bins - 1
    return ib


def max_keys(ib, K, nslots):
    """(keys [nslots], cnt [nslots]) of the rows with ib >= 0"""
    keys, cnt = np.zeros(nslots, np.uint64), np.zeros(nslots, np.uint64)
    ok = ib >= 0
    np.maximum.at(keys, ib[ok], K[ok])
    np.add.at(cnt, ib[ok], np.uint64(1))
    return keys, cnt


# ---- the curve, the hull, the intervals ---------------------------------------------------------------------------------------
def curve(lmax, row, lhat):
    if not math.isfinite(float(lhat)):
        return np.full(lmax.size, np.nan)
    pl = lmax.astype(np.float64) - float(lhat)
    pl[row < 0] = -np.inf
    return pl


def hull(x, y):
    """the least concave majorant of the points (x, y) with x not NaN and y finite, evaluated at x"""
    n = len(x)
    plh = np.full(n, np.nan)
    h = []
    for j in range(n):
        if math.isnan(x[j]):
            continue
        plh[j] = y[j]
        if not math.isfinite(y[j]):
            continue
        while len(h) >= 2:
            o, a = h[-2], h[-1]
            cr = (x[a] - x[o]) * (y[j] - y[o]) - (y[a] - y[o]) * (x[j] - x[o])
            if cr >= 0.0:
                h.pop()
            else:
                break
        h.append(j)
    for a, b in zip(h[:-1], h[1:]):
        for j in range(a + 1, b):
            if not math.isnan(x[j]) and math.isfinite(y[j]):
                chord = y[a] + (y[b] - y[a]) * ((x[j] - x[a]) / (x[b] - x[a]))
                plh[j] = max(chord, y[j])
    return plh


def interval(x, y, drop):
    """(lo, hi, nseg, open): open bit 0 / 1 the lower / upper end, bit 2 no bin reaches the level"""
    n = len(x)
    live = [j for j in range(n) if not math.isnan(x[j])]
    if any(math.isnan(y[j]) for j in live):
        return math.nan, math.nan, 0, 0
    inside = [j for j in live if y[j] >= -drop]
    if not inside:
        return math.nan, math.nan, 0, 4
    nseg, prev = 0, False
    for j in live:
        cur = y[j] >= -drop
        nseg += int(cur and not prev)
        prev = cur
    jl, jh = inside[0], inside[-1]

    def cross(jin, jout):
        if y[jout] == -math.inf:
            return float(x[jin])
        t = (-drop - y[jout]) / (y[jin] - y[jout])
        return float(x[jout] + (x[jin] - x[jout]) * t)

    below = [j for j in live if j < jl]
    above = [j for j in live if j > jh]
    op = 0
    if below:
        lo = cross(jl, below[-1])
    else:
        lo, op = float(x[jl]), op | 1
    if above:
        hi = cross(jh, above[0])
    else:
        hi, op = float(x[jh]), op | 2
    return lo, hi, nseg, op


def levels_of(levels=None, drops=None, two_d=False):
    """(p [L], drop [L])"""
    if drops is not None:
        return [math.nan] * len(drops), [float(d) for d in drops]
    levels = DEFAULT_LEVELS if levels is None else levels
    return [float(p) for p in levels], [drop_2d(p) if two_d else drop_1d(p) for p in levels]


def intervals_of(x, pl, plh, levels=None, drops=None):
    ps, ds = levels_of(levels, drops)
    out = np.zeros(len(ps), INTERVAL_DTYPE)
    for i, (p, d) in enumerate(zip(ps, ds)):
        lo, hi, nseg, op = interval(x, pl, d)
        lo_h, hi_h, _, op_h = interval(x, plh, d)
        fl = (OPEN_LO if op & 1 else 0) | (OPEN_HI if op & 2 else 0) | (NO_BIN if op & 4 else 0)
        fl |= (HULL_OPEN_LO if op_h & 1 else 0) | (HULL_OPEN_HI if op_h & 2 else 0)
        out[i] = (p, d, lo, hi, lo_h, hi_h, nseg, fl)
    return out


# ---- a whole call -----------------------------------------------------------------------------------------------------------------
def profile(rows, n=64, levels=None, drops=None, clip=(0, 1), from_=None, to=None):
    """the dict of Engine.profile_likelihood / rows_profile for rows [N, np + 1] float32, with path"""
    rows = np.ascontiguousarray(rows, np.float32)
    N, ncol = rows.shape
    np_ = ncol - 1
    ll = rows[:, np_]
    K = row_keys(ll)
    hat = K.max()
    lhat, row_hat = key_lmax(hat)[()], int(key_row(hat))
    L = len(levels_of(levels, drops)[0])
    o = dict(cnt=np.zeros((np_, n), np.uint64), lmax=np.zeros((np_, n), np.float32), row=np.zeros((np_, n), np.int64),
             xat=np.zeros((np_, n), np.float32), pl=np.zeros((np_, n)), plh=np.zeros((np_, n)), intervals=np.zeros((np_, L), INTERVAL_DTYPE),
             path=np.full((np_, n, ncol), np.nan, np.float32))
    for name in ("from", "to", "lhat", "xhat"):
        o[name] = np.full(np_, np.nan)
    o["row_hat"], o["nvalues"] = np.full(np_, row_hat, np.int64), np.full(np_, N, np.int64)
    o["nbinned"], o["ndropped"] = np.zeros(np_, np.int64), np.zeros(np_, np.int64)
    o["nempty"], o["flags"] = np.full(np_, n, np.int32), np.zeros(np_, np.int32)
    ps, ds = levels_of(levels, drops)
    for c in range(np_):
        v = rows[:, c]
        if not np.isfinite(v).all():
            o["flags"][c] = NONFINITE
            o["lmax"][c], o["row"][c], o["xat"][c] = -np.inf, -1, np.nan
            o["pl"][c] = o["plh"][c] = np.nan
            for i in range(L):
                o["intervals"][c, i] = (ps[i], ds[i], np.nan, np.nan, np.nan, np.nan, 0, NONFINITE)
            continue
        f, t, inv = grid_of(v, n, clip, None if from_ is None else from_[c], None if to is None else to[c])
        keys, cnt = max_keys(bins_of(v, n, f, t, inv), K, n)
        row = key_row(keys)
        lmax = key_lmax(keys)
        x = np.where(row >= 0, v[np.maximum(row, 0)].astype(np.float64), np.nan)
        pl = curve(lmax, row, lhat)
        plh = hull(x, pl) if math.isfinite(float(lhat)) else np.full(n, np.nan)
        o["cnt"][c], o["lmax"][c], o["row"][c], o["xat"][c], o["pl"][c], o["plh"][c] = cnt, lmax, row, x.astype(np.float32), pl, plh
        o["intervals"][c] = intervals_of(x, pl, plh, levels, drops)
        o["path"][c][row >= 0] = rows[row[row >= 0]]
        o["from"][c], o["to"][c], o["lhat"][c], o["xhat"][c] = f, t, float(lhat), float(v[row_hat])
        o["nbinned"][c] = int(cnt.sum())
        o["ndropped"][c] = N - int(cnt.sum())
        o["nempty"][c] = int((keys == 0).sum())
        o["flags"][c] = 0 if math.isfinite(float(lhat)) else LL_NONFINITE
    return o


def profile2d(rows, g=32, pairs=None, levels=None, drops=None, clip=(0, 1), from_=None, to=None):
    """the dict of Engine.profile_likelihood2d / rows_profile2d for rows [N, np + 1] float32"""
    rows = np.ascontiguousarray(rows, np.float32)
    N, ncol = rows.shape
    np_ = ncol - 1
    if pairs is None:
        pairs = [(a, b) for a in range(np_) for b in range(a + 1, np_)]
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    K = row_keys(rows[:, np_])
    hat = K.max()
    lhat, row_hat = key_lmax(hat)[()], int(key_row(hat))
    finite = [bool(np.isfinite(rows[:, c]).all()) for c in range(np_)]
    ib, o = {}, {}
    for name in ("from", "to", "lhat", "xhat"):
        o[name] = np.full(np_, np.nan)
    o["row_hat"], o["nvalues"], o["col_flags"] = np.full(np_, row_hat, np.int64), np.full(np_, N, np.int64), np.zeros(np_, np.int32)
    for c in range(np_):
        if not finite[c]:
            o["col_flags"][c] = NONFINITE
            continue
        v = rows[:, c]
        f, t, inv = grid_of(v, g, clip, None if from_ is None else from_[c], None if to is None else to[c])
        ib[c] = bins_of(v, g, f, t, inv)
        o["from"][c], o["to"][c], o["lhat"][c], o["xhat"][c] = f, t, float(lhat), float(v[row_hat])
        o["col_flags"][c] = 0 if math.isfinite(float(lhat)) else LL_NONFINITE
    ps, ds = levels_of(levels, drops, two_d=True)
    P, gg = pairs.shape[0], g * g
    o.update(pairs=pairs, nbinned=np.zeros(P, np.int64), nempty=np.full(P, gg, np.int32), flags=np.zeros(P, np.int32),
             cnt=np.zeros((P, g, g), np.uint64), lmax=np.full((P, g, g), -np.inf, np.float32), row=np.full((P, g, g), -1, np.int64),
             xat_a=np.full((P, g, g), np.nan, np.float32), xat_b=np.full((P, g, g), np.nan, np.float32), z=np.full((P, g, g), np.nan),
             nlevel=np.zeros((P, len(ds)), np.int64))
    for p, (a, b) in enumerate(pairs):
        if not (finite[a] and finite[b]):
            o["flags"][p] = NONFINITE
            continue
        cell = np.where((ib[a] >= 0) & (ib[b] >= 0), ib[a] * g + ib[b], -1)
        keys, cnt = max_keys(cell, K, gg)
        row, lmax = key_row(keys), key_lmax(keys)
        z = curve(lmax, row, lhat)
        o["cnt"][p], o["lmax"][p], o["row"][p], o["z"][p] = cnt.reshape(g, g), lmax.reshape(g, g), row.reshape(g, g), z.reshape(g, g)
        o["xat_a"][p] = np.where(row >= 0, rows[np.maximum(row, 0), a], np.float32(np.nan)).reshape(g, g)
        o["xat_b"][p] = np.where(row >= 0, rows[np.maximum(row, 0), b], np.float32(np.nan)).reshape(g, g)
        o["nbinned"][p], o["nempty"][p] = int(cnt.sum()), int((keys == 0).sum())
        with np.errstate(invalid="ignore"):
            o["nlevel"][p] = [int(((keys != 0) & (z >= -d)).sum()) for d in ds]
        o["flags"][p] = 0 if math.isfinite(float(lhat)) else LL_NONFINITE
    return o


# ---- the brute force the restatement itself is held to (<= 200 rows) ----------------------------------------------------------
def brute_bins(v, ll, bins, f, t):
    """per bin (cnt, the row of the largest log L in key order with the first row on ties, -1 for none) by a loop over the rows,
    with Python floats and struct for the order"""
    import struct

    def order(l):
        if math.isnan(l):
            l = -math.inf
        b = struct.unpack("<I", struct.pack("<f", l))[0]
        return b ^ (0xFFFFFFFF if b >> 31 else 0x80000000)

    cnt, best = [0] * bins, [-1] * bins
    for r in range(len(v)):
        d = float(v[r])
        if d == t:
            j = 0 if f == t else bins - 1
        elif f == t:
            continue
        else:
            xp = (d - f) * (bins / (t - f))
            if not (0.0 <= xp < bins):
                continue
            j = int(math.floor(xp))
        cnt[j] += 1
        if best[j] < 0 or order(float(ll[r])) > order(float(ll[best[j]])):
            best[j] = r
    return cnt, best
