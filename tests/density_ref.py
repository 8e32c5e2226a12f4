"""The float64 numpy model of the sample-store densities: R's density.default with a Gaussian
kernel and bw.nrd0, its linear binning made order-free in fixed point.  Every function restates one definition of that
section; nothing here calls the library."""
import numpy as np

NG = 512          # grid points
TWO24 = 16777216.0


def quantile7(sorted_f32, p):
    """the type-7 quantile from exact float order statistics, as mcx_samples_summary forms it"""
    N = sorted_f32.size
    h = (N - 1) * p
    lo = int(np.floor(h))
    g = h - lo
    a, b = float(sorted_f32[min(lo, N - 1)]), float(sorted_f32[min(lo + 1, N - 1)])
    return a if (g == 0.0 or a == b) else a + g * (b - a)


def nrd0(N, sd, q25, q75, vmin, adjust=1.0):
    hi = sd
    lo = min(hi, (q75 - q25) / 1.34)
    if lo == 0.0:
        lo = hi
    if lo == 0.0:
        lo = abs(float(vmin))
    if lo == 0.0:
        lo = 1.0
    return adjust * 0.9 * lo * float(N) ** -0.2


def grid(col_f32, adjust=1.0, clip=(0.0, 1.0), is_last_col=False, bw=None, from_=None, to=None):
    """dict(bw, from, to, lo, up, mean, sd) of one column of float32 values"""
    v = np.sort(np.asarray(col_f32, np.float32))
    d = v.astype(np.float64)
    N = d.size
    mean = d.sum() / N
    sd = float(np.sqrt(((d - mean) ** 2).sum() / (N - 1)))
    q25, q75 = quantile7(v, 0.25), quantile7(v, 0.75)
    b = nrd0(N, sd, q25, q75, v[0], adjust) if bw is None or np.isnan(bw) else float(bw)
    f, t = float(v[0]), float(v[-1])
    if tuple(clip) != (0.0, 1.0):
        f = quantile7(v, clip[0])
        if not is_last_col:
            t = quantile7(v, clip[1])
    if from_ is not None and not np.isnan(from_):
        f = float(from_)
    if to is not None and not np.isnan(to):
        t = float(to)
    return {"bw": b, "from": f, "to": t, "lo": f - 4.0 * b, "up": t + 4.0 * b, "mean": mean, "sd": sd}


def bins(col_f32, lo, up):
    """slots [NG + 1, 2] uint64 = (cnt, frac) of one column on the grid [lo, up]"""
    inv = (NG - 1) / (up - lo)
    with np.errstate(invalid="ignore", over="ignore"):
        xpos = (np.asarray(col_f32, np.float32).astype(np.float64) - lo) * inv
        ok = (xpos >= -1.0) & (xpos < float(NG))
        xpos = xpos[ok]
    fl = np.floor(xpos)
    w = np.floor((xpos - fl) * TWO24)
    s = fl.astype(np.int64) + 1
    assert xpos.size < 1 << 28  # the float64 sums of bincount are exact integers while they stay below 2^53
    out = np.zeros((NG + 1, 2), np.uint64)
    out[:, 0] = np.bincount(s, minlength=NG + 1).astype(np.uint64)
    out[:, 1] = np.bincount(s, weights=w, minlength=NG + 1).astype(np.uint64)
    return out


def masses(slots, N):
    cnt, frac = slots[:, 0].astype(np.float64), slots[:, 1].astype(np.float64)
    y = np.zeros(2 * NG)
    y[:NG] = ((cnt[1:] - frac[1:] / TWO24) + frac[:-1] / TWO24) / N
    return y


def kernel(bw, delta):
    m = np.arange(2 * NG, dtype=np.float64)
    k = np.where(m <= NG, m * delta, -(2 * NG - m) * delta)
    return np.exp(-0.5 * (k / bw) ** 2) / (bw * np.sqrt(2.0 * np.pi))


def finish(g, slots, N, n=NG):
    """(x [n], y [n]) from a grid record (bw, from, to, lo, up), a column's slots and N: the convolution in its FFT form"""
    lo, up = g["lo"], g["up"]
    delta = (up - lo) / (NG - 1)
    y = masses(slots, N)
    K = kernel(g["bw"], delta)
    # d[j] = sum_m y[m] K[(m - j) mod 2 NG]: a circular correlation
    d = np.fft.irfft(np.fft.rfft(y) * np.conj(np.fft.rfft(K)), 2 * NG)[:NG]
    d = np.maximum(0.0, d)
    xg = lo + np.arange(NG, dtype=np.float64) * delta
    x = g["from"] + np.arange(n, dtype=np.float64) * ((g["to"] - g["from"]) / (n - 1))
    x[n - 1] = g["to"]
    i = np.clip(np.searchsorted(xg, x, side="right") - 1, 0, NG - 2)
    yo = d[i] + (d[i + 1] - d[i]) * ((x - xg[i]) / (xg[i + 1] - xg[i]))
    return x, yo


def finish_direct(g, slots, N):
    """d [NG] by the plain sum, for the model's own check of its FFT form"""
    delta = (g["up"] - g["lo"]) / (NG - 1)
    y = masses(slots, N)
    K = kernel(g["bw"], delta)
    idx = (np.arange(2 * NG)[None, :] - np.arange(NG)[:, None]) % (2 * NG)
    return np.maximum(0.0, (y[None, :] * K[idx]).sum(axis=1))


def density(col_f32, n=NG, **kw):
    """the whole estimate of one column: (grid record, slots, x, y)"""
    g = grid(col_f32, **kw)
    s = bins(col_f32, g["lo"], g["up"])
    x, y = finish(g, s, np.asarray(col_f32).size, n)
    return g, s, x, y
