"""The float64 numpy model of the pair densities of the sample store: MASS::kde2d with bandwidth.nrd,
its linear binning made order-free in fixed point.  Every function restates one definition of that section; nothing here
calls the library."""
import numpy as np

import density_ref as D1

F = 4096


def nrd4(N, sd, q25, q75, vmin, adjust=1.0):
    """bandwidth.nrd / 4 with section 13's fallbacks"""
    s = min(sd, (q75 - q25) / 1.34)
    if s == 0.0:
        s = sd
    if s == 0.0:
        s = abs(float(vmin))
    if s == 0.0:
        s = 1.0
    return adjust * 1.06 * s * float(N) ** -0.2


def grid(col_f32, adjust=1.0, clip=(0.0, 1.0), is_last_col=False, bw=None, from_=None, to=None):
    """dict(bw, from, to, lo, up, mean, sd) of one column: from, to, mean and sd are section 13's"""
    g = D1.grid(col_f32, adjust=adjust, clip=clip, is_last_col=is_last_col, bw=bw, from_=from_, to=to)
    if bw is None or np.isnan(bw):
        v = np.sort(np.asarray(col_f32, np.float32))
        g["bw"] = nrd4(v.size, g["sd"], D1.quantile7(v, 0.25), D1.quantile7(v, 0.75), v[0], adjust)
    g["lo"] = g["from"] - 4.0 * g["bw"]
    g["up"] = g["to"] + 4.0 * g["bw"]
    return g


def axis(g, G):
    delta = (g["up"] - g["lo"]) / (G - 1)
    return g["lo"] + np.arange(G, dtype=np.float64) * delta


def codes(col_f32, lo, up, G):
    """(on [N] bool, s [N] int64 in [0, G], w [N] int64 in [0, F]) of one column on the grid [lo, up] of G nodes"""
    inv = (G - 1) / (up - lo)
    with np.errstate(invalid="ignore", over="ignore"):
        xpos = (np.asarray(col_f32, np.float32).astype(np.float64) - lo) * inv
        on = (xpos >= -1.0) & (xpos < float(G))
    xp = np.where(on, xpos, 0.0)
    fl = np.floor(xp)
    return on, fl.astype(np.int64) + 1, np.floor((xp - fl) * F).astype(np.int64)


def slots(col_a, col_b, lo_a, up_a, lo_b, up_b, G):
    """slots [(G + 1)^2, 4] uint64 = (cnt, Sa, Sb, Sab) of one pair"""
    oa, sa, wa = codes(col_a, lo_a, up_a, G)
    ob, sb, wb = codes(col_b, lo_b, up_b, G)
    ok = oa & ob
    idx = sa[ok] * (G + 1) + sb[ok]
    wa, wb = wa[ok], wb[ok]
    out = np.zeros(((G + 1) ** 2, 4), np.uint64)
    n = (G + 1) ** 2
    assert idx.size < 1 << 28  # the float64 sums of bincount are exact integers while they stay below 2^53
    out[:, 0] = np.bincount(idx, minlength=n).astype(np.uint64)
    out[:, 1] = np.bincount(idx, weights=wa, minlength=n).astype(np.uint64)
    out[:, 2] = np.bincount(idx, weights=wb, minlength=n).astype(np.uint64)
    out[:, 3] = np.bincount(idx, weights=(wa * wb).astype(np.float64), minlength=n).astype(np.uint64)
    return out


def masses(sl, N, G):
    """mass [G, G]: the bilinear node masses, exact integers until the one division"""
    s = np.asarray(sl, np.uint64).reshape(G + 1, G + 1, 4).astype(np.int64)
    cnt, Sa, Sb, Sab = s[..., 0], s[..., 1], s[..., 2], s[..., 3]
    num = ((F * F * cnt - F * Sa - F * Sb + Sab)[1:, 1:] + (F * Sa - Sab)[:-1, 1:] + (F * Sb - Sab)[1:, :-1] + Sab[:-1, :-1])
    return num.astype(np.float64) / (float(F * F) * float(N))


def kernel(g, G):
    delta = (g["up"] - g["lo"]) / (G - 1)
    u = (np.arange(G, dtype=np.float64) * delta) / g["bw"]
    return np.exp(-0.5 * (u * u)) / (g["bw"] * np.sqrt(2.0 * np.pi))


def finish(ga, gb, sl, N, G):
    """z [G, G] of one pair from its two grid records, its slots and N"""
    mass = masses(sl, N, G)
    d = np.abs(np.arange(G)[:, None] - np.arange(G)[None, :])
    Ta, Tb = kernel(ga, G)[d], kernel(gb, G)[d]  # Ta[j, m] = K_a[|m - j|]
    return (Ta @ mass) @ Tb


def kde2d_direct(col_a, col_b, ga, gb, G):
    """the estimator itself on the same nodes: z[j, k] = sum over rows of phi((x_j - a_r) / h_a) phi((y_k - b_r) / h_b) /
    (N h_a h_b)"""
    a, b = np.asarray(col_a, np.float64), np.asarray(col_b, np.float64)
    phi = lambda u: np.exp(-0.5 * u * u) / np.sqrt(2.0 * np.pi)  # noqa: E731
    A = phi((axis(ga, G)[:, None] - a[None, :]) / ga["bw"])
    B = phi((axis(gb, G)[:, None] - b[None, :]) / gb["bw"])
    return (A @ B.T) / (a.size * ga["bw"] * gb["bw"])
