"""DESIGN.md section 22 restated in numpy float64 and Python integers: the fixed-point weights q, the integer sums, Kish's
effective size, the log of the mean weight, the k-hat fit of the tail, the weighted moments, the weighted inverse ECDF and the
resample rule.  Everything behind q is defined on q: the GPU tests feed restate() the library's own q and hold the integers
exactly and the fp64 sums to their derived bounds; fixed_point() is held to within one unit of the library's q."""
import math

import numpy as np

TWO31 = 2 ** 31
NO_TAIL, KHAT_HIGH = 1, 2
NONFINITE = 1


def okey(col):
    """mcx_samples_summary's key of float32 values as uint32: NaN last, -0 before +0"""
    col = np.ascontiguousarray(col, np.float32)
    u = col.view(np.uint32)
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[np.isnan(col)] = np.uint32(0xffffffff)
    return k


def log_weights(v, scale):
    """lw = scale * (double)v, one product"""
    with np.errstate(invalid="ignore"):
        return np.float64(scale) * np.asarray(v, np.float32).astype(np.float64)


def first_refused(lw):
    """the lowest row whose lw is NaN or +inf, or None"""
    bad = np.flatnonzero(np.isnan(lw) | (lw == np.inf))
    return int(bad[0]) if len(bad) else None


def fixed_point(lw):
    """(q uint32 [N], lwmax): q = rint(2^31 exp(lw - lwmax)), ties to even"""
    lwmax = float(np.max(lw))
    with np.errstate(under="ignore"):
        q = np.rint(float(TWO31) * np.exp(lw - lwmax))
    return q.astype(np.uint32), lwmax


def tail_length(N):
    return min(N // 5, math.ceil(3.0 * math.sqrt(float(N))))


def khat_of_tail(x):
    """(khat, sigma, flags) of rising exceedances x: Zhang and Stephens' estimator with the weak prior of Vehtari et al., every
    sum in index order"""
    x = [float(v) for v in x]
    n = len(x)
    if n < 5:
        return math.nan, math.nan, NO_TAIL
    xn, xstar = x[n - 1], x[int(math.floor(n / 4.0 + 0.5)) - 1]
    if not xstar > 0.0 or not xn > 0.0:
        return math.nan, math.nan, NO_TAIL
    m = 30 + int(math.floor(math.sqrt(float(n))))

    def mean_log1p(theta):
        s = 0.0
        for v in x:
            s += math.log1p(-theta * v)
        return s / float(n)

    th, ell = [], []
    for j in range(1, m + 1):
        t = 1.0 / xn + (1.0 - math.sqrt(float(m) / (float(j) - 0.5))) / (3.0 * xstar)
        k = mean_log1p(t)
        th.append(t)
        ell.append(float(n) * (math.log(-t / k) - k - 1.0))
    theta = 0.0
    for j in range(m):
        s = 0.0
        for i in range(m):
            d = ell[i] - ell[j]
            s += math.exp(d) if d < 709.0 else math.inf
        theta += th[j] * (1.0 / s)
    k = mean_log1p(theta)
    khat = (k * float(n) + 5.0) / (float(n) + 10.0)
    return khat, -k / theta, (KHAT_HIGH if khat > 0.7 else 0)


def threshold(p, Q):
    """min(Q, max(1, ceil(p (double)Q))) in IEEE double"""
    return min(Q, max(1, int(math.ceil(float(p) * float(Q)))))


def weighted_quantile_keys(col, q, ts):
    """per threshold t the float of the column with the smallest key whose cumulative q reaches t (rows with q > 0 only)"""
    col = np.ascontiguousarray(col, np.float32)
    use = q > 0
    k, v, w = okey(col)[use], col[use], q[use].astype(np.int64)
    order = np.argsort(k, kind="stable")
    k, v, w = k[order], v[order], w[order]
    cum = np.cumsum(w)  # below 2^62
    out = []
    for t in ts:
        i = int(np.searchsorted(cum, t, side="left"))
        # the whole tie run of that key lies at or before the crossing: any of its floats has the key; the library reports the key's float
        out.append(v[i])
    return np.array(out, np.float32), k


def key_float(k):
    k = np.asarray(k, np.uint32)
    u = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32)
    return u.view(np.float32)


def integer_sums_slow(q):
    """(sum q, sum q^2, the count of q = 0) in Python integers, one row at a time: the definition"""
    qi = [int(v) for v in q]
    return sum(qi), sum(v * v for v in qi), sum(1 for v in qi if v == 0)


def integer_sums(q):
    """integer_sums_slow without the loop, for N < 2^31 values below 2^32: q = a 2^16 + b, and the three sums of a^2, a b and b^2
    (each below 2^63) are exact in int64; tests/test_reweight_cpu.py pins the two to each other"""
    q = np.asarray(q, np.uint32).astype(np.int64)
    assert q.size < 2 ** 31
    a, b = q >> 16, q & 0xffff
    Q2 = (int(np.sum(a * a)) << 32) + (int(np.sum(a * b)) << 17) + int(np.sum(b * b))
    return int(np.sum(q)), Q2, int(np.count_nonzero(q == 0))


def restate(rows, q, lwmax, probs):
    """the result of mcx_*_reweight for rows [N, ncol] float32 and fixed-point weights q: a dict with Python integers for the
    sums, floats for the rest, and per column arrays"""
    rows = np.ascontiguousarray(rows, np.float32)
    N, ncol = rows.shape
    Q, Q2, nzero = integer_sums(q)
    out = dict(n=N, nzero=nzero, lwmax=lwmax, sumq=Q, sumq2=Q2, sumq2_hi=Q2 >> 64, sumq2_lo=Q2 & (2 ** 64 - 1))
    out["ess_kish"] = float(Q * Q / Q2) if Q2 < 2 ** 1000 else math.nan  # (integer true division: correctly rounded)
    out["log_mean_w"] = lwmax + math.log(float(Q) / (float(TWO31) * float(N)))
    M = tail_length(N)
    out["tail_m"] = M
    if M >= 5:
        srt = np.sort(np.asarray(q, np.uint32))
        cutoff = int(srt[N - M - 1])
        x = [(int(v) - cutoff) / float(TWO31) for v in srt[N - M:]]
        out["khat"], out["tail_sigma"], out["flags"] = khat_of_tail(x)
    else:
        out["khat"], out["tail_sigma"], out["flags"] = math.nan, math.nan, NO_TAIL
    ts = [1, Q] + [threshold(p, Q) for p in probs]
    use = np.asarray(q) > 0
    qd = np.asarray(q, np.uint32).astype(np.float64)[use]
    cols = {k: np.full(ncol, np.nan) for k in ("mean", "sd", "mcse_mean", "scale")}
    cols["min"], cols["max"], cols["flags"] = np.zeros(ncol, np.float32), np.zeros(ncol, np.float32), np.zeros(ncol, np.int32)
    quant = np.zeros((ncol, len(probs)))
    for c in range(ncol):
        col = rows[:, c]
        vals, _ = weighted_quantile_keys(col, np.asarray(q), ts)
        cols["min"][c], cols["max"][c] = vals[0], vals[1]
        quant[c] = vals[2:].astype(np.float64)
        x = col[use].astype(np.float64)
        if not np.all(np.isfinite(x)):
            cols["flags"][c] = NONFINITE
            continue
        mean = math.fsum(qd * x) / float(Q)
        d2 = (x - mean) ** 2
        cols["mean"][c] = mean
        cols["sd"][c] = math.sqrt(math.fsum(qd * d2) / float(Q))
        cols["mcse_mean"][c] = math.sqrt(math.fsum(qd * qd * d2)) / float(Q)
        cols["scale"][c] = math.fsum(qd * np.abs(x)) / float(Q)  # what the mean's bound is relative to
    out["cols"], out["quantiles"] = cols, quant
    return out


def brute_quantile(col, q, p):
    """the definition, slowly: sort (key, q) pairs, Python-integer cumulative sums, the first value whose sum reaches t"""
    pairs = sorted((int(k), float(v), int(w)) for k, v, w in zip(okey(col), np.asarray(col, np.float32), q) if w > 0)
    Q = sum(w for _, _, w in pairs)
    t = threshold(p, Q)
    # C(x) counts every row whose key is at most x's: the whole tie run
    i = 0
    cum = 0
    while i < len(pairs):
        j = i
        while j < len(pairs) and pairs[j][0] == pairs[i][0]:
            cum += pairs[j][2]
            j += 1
        if cum >= t:
            return np.float32(pairs[i][1])
        i = j
    raise AssertionError("the thresholds never exceed Q")


def draw_r(seed, k):
    """r of draw k: Philox4x32-10, counter (k lo, k hi, 0, 0), key (seed, 5), r = w.x : w.y"""
    M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
    c = [k & 0xffffffff, (k >> 32) & 0xffffffff, 0, 0]
    k0, k1 = seed & 0xffffffff, 5
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xffffffff, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xffffffff]
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return (c[0] << 32) | c[1]


def resample_index(q, seed, K):
    """index[k]: the smallest j with q_0 + ... + q_j > u_k, u_k = (r_k Q) >> 64; and u"""
    cum = np.cumsum(np.asarray(q, np.uint32).astype(np.int64))
    Q = int(cum[-1])
    u = np.array([(draw_r(seed, k) * Q) >> 64 for k in range(K)], np.int64)
    return np.searchsorted(cum, u, side="right").astype(np.int64), u
