"""float64 / Python-integer restatement of mcx_*_compare, for the tests.

Two stores A and B, column by column.  Values are ordered by the rank summary's key: -0 and +0 one point, -inf and +inf ordinary
end points, every NaN one point that sorts last.  cA(x), cB(x) = the number of values <= x in that order.
  ks_plus_num  = max over the distinct x of A of cA(x) NB - cB(x) NA, ks_plus_x the smallest x that attains it
  ks_minus_num = max over the distinct x of B of cB(x) NA - cA(x) NB
  ks           = float(max of the two) / (float(NA) * float(NB))
  w1           = sum over the pooled distinct x_k but the last of float(|cA NB - cB NA|) (x_{k+1} - x_k), / (float(NA) * float(NB))
mean, sd, ess of a side are summary_ref's when the side has T >= 4 and iid is not asked; else ess = N."""
import math

import numpy as np

import summary_ref

NONFINITE_A, NONFINITE_B = 1, 2
FIELDS = ("ks_plus_num", "ks_minus_num", "ks_plus_x", "ks_minus_x", "ks", "w1", "mean_a", "sd_a", "ess_a", "mean_b", "sd_b", "ess_b",
          "z_mean", "ks_neff", "ks_p", "na", "nb", "flags")
NAN_WHEN_FLAGGED = ("w1", "z_mean", "ks_neff", "ks_p")


def ckey(x):
    """the order-preserving u32 key of float32 values: -0 as +0, every NaN 0xffffffff"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    u = x.view(np.uint32).copy()
    u[u == np.uint32(0x80000000)] = 0
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[np.isnan(x)] = 0xffffffff
    return k


def key_value(k):
    """float64 value of keys (NaN for the NaN key)"""
    k = np.asarray(k, np.uint32)
    v = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(np.float32).astype(np.float64)
    v[k == np.uint32(0xffffffff)] = np.nan
    return v


def distances(a, b):
    """the integer KS numerators with their points, ks and w1 of two columns (1-D float32)"""
    ka, kb = np.sort(ckey(a)), np.sort(ckey(b))
    NA, NB = int(ka.size), int(kb.size)
    pooled = np.unique(np.concatenate([ka, kb]))
    cA = np.searchsorted(ka, pooled, "right").astype(object)
    cB = np.searchsorted(kb, pooled, "right").astype(object)
    d = cA * NB - cB * NA  # Python integers
    in_a = np.isin(pooled, ka)
    in_b = np.isin(pooled, kb)
    xs = key_value(pooled)

    def best(vals, mask):
        top, at = None, None
        for i in np.flatnonzero(mask):
            if top is None or vals[i] > top:
                top, at = vals[i], i
        return int(top), float(xs[at])

    plus, plus_x = best(d, in_a)
    minus, minus_x = best(-d, in_b)
    assert plus >= 0 and minus >= 0 and max(plus, minus) < 2 ** 62
    ks = float(max(plus, minus)) / (float(NA) * float(NB))
    terms = [float(abs(int(d[k]))) * (xs[k + 1] - xs[k]) for k in range(len(pooled) - 1)]
    with np.errstate(invalid="ignore"):
        w1 = (math.fsum(terms) if np.all(np.isfinite(terms)) else float(np.sum(terms))) / (float(NA) * float(NB))
    return dict(ks_plus_num=plus, ks_minus_num=minus, ks_plus_x=plus_x, ks_minus_x=minus_x, ks=ks, w1=w1)


def distances_numpy(a, b):
    """distances() without its Python loops, for columns of millions of values: the same definitions on the sorted keys, the
    products in int64 (NA NB < 2^62 is asserted), np.argmax for the lowest position that attains a maximum.
    tests/test_compare_cpu.py pins it to distances()"""
    ka, kb = np.sort(ckey(a)), np.sort(ckey(b))
    NA, NB = int(ka.size), int(kb.size)
    assert NA * NB < 2 ** 62
    pooled = np.unique(np.concatenate([ka, kb]))
    cA = np.searchsorted(ka, pooled, "right").astype(np.int64)
    cB = np.searchsorted(kb, pooled, "right").astype(np.int64)
    d = cA * NB - cB * NA
    in_a, in_b = np.diff(cA, prepend=0) > 0, np.diff(cB, prepend=0) > 0
    xs = key_value(pooled)
    ia, ib = np.flatnonzero(in_a), np.flatnonzero(in_b)
    pa, pb = ia[np.argmax(d[ia])], ib[np.argmax(-d[ib])]
    plus, minus = int(d[pa]), int(-d[pb])
    assert plus >= 0 and minus >= 0
    with np.errstate(invalid="ignore"):
        terms = np.abs(d[:-1]).astype(np.float64) * np.diff(xs)
        w1 = (math.fsum(terms) if np.all(np.isfinite(terms)) else float(np.sum(terms))) / (float(NA) * float(NB))
    return dict(ks_plus_num=plus, ks_minus_num=minus, ks_plus_x=float(xs[pa]), ks_minus_x=float(xs[pb]),
                ks=float(max(plus, minus)) / (float(NA) * float(NB)), w1=w1)


def counting(a, b):
    """distances() by the counting definition alone: every pooled point against every value, no sort"""
    ka, kb = ckey(a), ckey(b)
    NA, NB = len(ka), len(kb)
    pts = sorted(set(ka.tolist()) | set(kb.tolist()))
    sa, sb = set(ka.tolist()), set(kb.tolist())
    rec = []
    for p in pts:
        ca, cb = sum(1 for k in ka.tolist() if k <= p), sum(1 for k in kb.tolist() if k <= p)
        rec.append((p, ca * NB - cb * NA))
    plus = max(d for p, d in rec if p in sa)
    minus = max(-d for p, d in rec if p in sb)
    plus_x = min(p for p, d in rec if p in sa and d == plus)
    minus_x = min(p for p, d in rec if p in sb and -d == minus)
    xs = key_value(np.array([p for p, _ in rec], np.uint32))
    w1 = 0.0
    for k in range(len(rec) - 1):
        w1 += float(abs(rec[k][1])) * (xs[k + 1] - xs[k])
    return dict(ks_plus_num=plus, ks_minus_num=minus, ks_plus_x=float(key_value(np.array([plus_x], np.uint32))[0]),
                ks_minus_x=float(key_value(np.array([minus_x], np.uint32))[0]), ks=float(max(plus, minus)) / (float(NA) * float(NB)),
                w1=w1 / (float(NA) * float(NB)))


def kolmogorov_q(lam):
    """P(K > lam): the alternating series from 1.18 on, the theta-function form below; clamped to [0, 1]"""
    if math.isnan(lam):
        return lam
    if lam <= 0:
        return 1.0
    if lam >= 1.18:
        s, sign = 0.0, 1.0
        for k in range(1, 101):
            s1 = s + sign * math.exp(-2.0 * k * k * lam * lam)
            if s1 == s:
                break
            s, sign = s1, -sign
        q = 2.0 * s
    else:
        a = math.pi ** 2 / (8.0 * lam * lam)
        s = 0.0
        for k in range(1, 101):
            s1 = s + math.exp(-((2 * k - 1) ** 2) * a)
            if s1 == s:
                break
            s = s1
        q = 1.0 - math.sqrt(2.0 * math.pi) / lam * s
    return min(max(q, 0.0), 1.0)


def ks_lambda(ks, ne):
    return (math.sqrt(ne) + 0.12 + 0.11 / math.sqrt(ne)) * ks


def ks_prob(ks, ess_a, ess_b):
    """(ks_neff, ks_p)"""
    if math.isnan(ess_a) or math.isnan(ess_b):
        return math.nan, math.nan
    ne = ess_a * ess_b / (ess_a + ess_b)
    return ne, kolmogorov_q(ks_lambda(ks, ne))


def z_mean(ma, sa, ea, mb, sb, eb):
    with np.errstate(all="ignore"):
        return float(np.float64(ma - mb) / np.sqrt(np.float64(sa) * sa / ea + np.float64(sb) * sb / eb))


def side(x, iid):
    """x [T, nc] float32 -> (mean, sd, ess, nonfinite)"""
    T, nc = x.shape
    N = T * nc
    if not np.all(np.isfinite(x)):
        return math.nan, math.nan, math.nan, True
    if not iid and T >= 4:
        r = summary_ref.restate_column(x, ())
        return r["mean"], r["sd"], r["ess"], False
    xd = x.astype(np.float64)
    return xd.mean(), (xd.std(ddof=1) if N >= 2 else math.nan), float(N), False


def restate(rows_a, Ta, nca, rows_b, Tb, ncb, iid=False):
    """rows [T * nc, ncol] (MCout layout) on both sides -> the dict of arrays of Engine.compare"""
    rows_a, rows_b = np.ascontiguousarray(rows_a, np.float32), np.ascontiguousarray(rows_b, np.float32)
    ncol = rows_a.shape[1]
    assert rows_b.shape[1] == ncol and rows_a.shape[0] == Ta * nca and rows_b.shape[0] == Tb * ncb
    out = {f: [] for f in FIELDS}
    for c in range(ncol):
        a, b = rows_a[:, c], rows_b[:, c]
        r = distances(a, b)
        ma, sa, ea, bad_a = side(a.reshape(Ta, nca), iid)
        mb, sb, eb, bad_b = side(b.reshape(Tb, ncb), iid)
        r.update(mean_a=ma, sd_a=sa, ess_a=ea, mean_b=mb, sd_b=sb, ess_b=eb, na=Ta * nca, nb=Tb * ncb,
                 flags=(NONFINITE_A if bad_a else 0) | (NONFINITE_B if bad_b else 0))
        if r["flags"]:
            r.update(w1=math.nan, z_mean=math.nan, ks_neff=math.nan, ks_p=math.nan)
        else:
            r["z_mean"] = z_mean(ma, sa, ea, mb, sb, eb)
            r["ks_neff"], r["ks_p"] = ks_prob(r["ks"], ea, eb)
        for f in FIELDS:
            out[f].append(r[f])
    ints = ("ks_plus_num", "ks_minus_num", "na", "nb")
    return {f: np.array(v, np.int64 if f in ints else np.int32 if f == "flags" else np.float64) for f, v in out.items()}


def same_double(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))))


def check(got, ref, rel_w1=1e-10, rel_mean=1e-9, rel_ess=1e-4):
    """assert a dict of Engine.compare against restate()'s: the integer fields, ks and the two points bit for bit (a NaN for a
    NaN), w1 at rel_w1, mean and sd at rel_mean, ess at rel_ess (tests/test_gpu_summary.py's), z_mean, ks_neff and ks_p as the
    host formulas give them from the dict's own ks, means, sds and ess.  Returns the largest relative difference of w1"""
    assert sorted(got) == sorted(FIELDS)
    for f in ("ks_plus_num", "ks_minus_num", "na", "nb", "flags"):
        assert np.array_equal(got[f], ref[f]), (f, got[f], ref[f])
    for f in ("ks", "ks_plus_x", "ks_minus_x"):
        assert same_double(got[f], ref[f]), (f, got[f], ref[f])
    worst = 0.0
    for c in range(len(ref["ks"])):
        where = "column %d" % c
        for f in ("mean_a", "sd_a", "ess_a", "mean_b", "sd_b", "ess_b", "w1", "z_mean", "ks_neff", "ks_p"):
            assert math.isnan(got[f][c]) == math.isnan(ref[f][c]), (where, f, got[f][c], ref[f][c])
        if not math.isnan(ref["w1"][c]):
            if ref["w1"][c] == 0.0:
                assert got["w1"][c] == 0.0, (where, got["w1"][c])
            else:
                rel = abs(got["w1"][c] - ref["w1"][c]) / ref["w1"][c]
                worst = max(worst, rel)
                assert rel <= rel_w1, (where, "w1", got["w1"][c], ref["w1"][c], rel)
        for s in "ab":
            if not math.isnan(ref["mean_" + s][c]):
                np.testing.assert_allclose(got["mean_" + s][c], ref["mean_" + s][c], rtol=rel_mean, atol=1e-300, err_msg=where)
            if not math.isnan(ref["sd_" + s][c]):
                np.testing.assert_allclose(got["sd_" + s][c], ref["sd_" + s][c], rtol=rel_mean, err_msg=where)
            if not math.isnan(ref["ess_" + s][c]):
                np.testing.assert_allclose(got["ess_" + s][c], ref["ess_" + s][c], rtol=rel_ess, err_msg=where)
        g = {f: float(got[f][c]) for f in FIELDS}
        if not math.isnan(ref["z_mean"][c]):
            np.testing.assert_allclose(g["z_mean"], z_mean(g["mean_a"], g["sd_a"], g["ess_a"], g["mean_b"], g["sd_b"], g["ess_b"]),
                                       rtol=1e-12, atol=1e-300, err_msg=where)
        if not math.isnan(ref["ks_p"][c]):
            ne, p = ks_prob(g["ks"], g["ess_a"], g["ess_b"])
            np.testing.assert_allclose(g["ks_neff"], ne, rtol=1e-12, err_msg=where)
            np.testing.assert_allclose(g["ks_p"], p, rtol=1e-9, atol=1e-12, err_msg=where)
    return worst
