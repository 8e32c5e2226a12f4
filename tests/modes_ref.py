"""The modes of a store restated in float64 numpy and Python integers: the scale, the distance in its
stated order, the labels, the k-means++ seeding, Lloyd's loop with its stopping rule, the mode table and the chain and step
tables.  Nothing here calls the library."""
import math

import numpy as np

import step_ref

ST_MODES = 7
MAX_K, NONE = 32, 255
CONVERGED, NOT_CONVERGED, EMPTY = 1, 2, 4
EPS = 2.0 ** -53
NAN = float("nan")

# (np, nc, T, K): the shapes of the loop tests, on which tests/test_modes_cpu.py shows the reference alone to be decisive
SHAPES = [(1, 129, 7, 2), (5, 33, 40, 3), (16, 64, 50, 8), (17, 19, 64, 32), (64, 16, 20, 4), (256, 8, 9, 2)]


def make_rows(np_, nc, T, K, seed, spread=12.0, hop=0.02, stay=0.7):
    """Metropolis-like rows [T * nc, np + 1] float32 of a K-mode target: a chain repeats its row with probability stay, hops to
    another mode with probability hop, else draws a new point of its mode (unit normal around the mode's centre); log L =
    -r^2 / 2 of the point within its mode.  Returns (rows, the mode of every row [T, nc])."""
    rng = np.random.default_rng(seed)
    cen = rng.normal(size=(K, np_)) * spread / math.sqrt(np_)
    for k in range(K):  # the centres apart along the first coordinates too, so that no two modes touch
        cen[k, k % np_] += spread * (1 + k // np_) * (1 if k % 2 else -1)
        cen[k, 0] += 3.0 * spread * k
    mode = rng.integers(0, K, size=nc)
    x = cen[mode] + rng.normal(size=(nc, np_))
    rows = np.zeros((T, nc, np_ + 1), np.float32)
    modes = np.zeros((T, nc), np.int64)
    for t in range(T):
        if t > 0:
            u = rng.random(nc)
            hopm = u < hop
            mode = np.where(hopm, (mode + 1 + rng.integers(0, max(K - 1, 1), size=nc)) % K, mode)
            move = hopm | (u >= stay)
            x =np.where(move[:, None], cen[mode] + rng.normal(size=(nc, np_)), x)
        rows[t, :, :np_] = x
        rows[t, :, np_] = -0.5 * ((x - cen[mode]) ** 2).sum(1)
        modes[t] = mode
    return rows.reshape(T * nc, np_ + 1), modes


def scale_of(rows, scale=True):
    """s [np]: 1 / sd (two passes, divisor N - 1) of every parameter column; 0 where the sd is 0 or not finite; ones without scale"""
    x = np.asarray(rows, np.float32)[:, :-1].astype(np.float64)
    N, p = x.shape
    s = np.ones(p)
    if not scale:
        return s
    for j in range(p):
        if not np.isfinite(x[:, j]).all():
            s[j] = 0.0
            continue
        m = math.fsum(x[:, j]) / N
        sd = math.sqrt(math.fsum((x[:, j] - m) ** 2) / (N - 1))
        s[j] = 1.0 / sd if sd > 0.0 and math.isfinite(1.0 / sd) else 0.0
    return s


def scaled(rows, s):
    """u [N, np] = (double)x s, one rounding each"""
    return np.asarray(rows, np.float32)[:, :-1].astype(np.float64) * np.asarray(s, np.float64)[None, :]


def dist2(u, c, s):
    """d2 [N, K]: over j in order e = u - c, acc = acc + e e, each operation rounded on its own (numpy fuses nothing)"""
    N, p = u.shape
    K = c.shape[0]
    acc = np.zeros((N, K))
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(p):
            if s[j] == 0.0:
                continue
            e = u[:, j][:, None] - c[None, :, j]
            acc = acc + e * e
    return acc


def finite_rows(rows):
    return np.isfinite(np.asarray(rows, np.float32)[:, :-1]).all(1)


def assign(rows, c, s):
    """one pass: (labels [N] uint8, d2 of the winner [N] (NaN for NONE), n [K], S [K, np] by fsum, margin [N])
    margin = (d2_2 - d2_1) / d2_2 of the two nearest centres (1 for K = 1 or d2_2 = 0 ... inf)"""
    rows = np.asarray(rows, np.float32)
    c = np.asarray(c, np.float64)
    K = c.shape[0]
    ok = finite_rows(rows)
    u = scaled(np.where(ok[:, None], rows, 0), s)
    d = dist2(u, c, s)
    lab = np.argmin(d, axis=1).astype(np.uint8)  # (the first of equal minima: the lowest k)
    win = d[np.arange(len(d)), lab]
    margin = np.ones(len(d))
    if K > 1:
        two = np.partition(d, 1, axis=1)[:, :2]
        with np.errstate(invalid="ignore", divide="ignore"):
            margin = np.where(two[:, 1] > 0, (two[:, 1] - two[:, 0]) / two[:, 1], 0.0)
    lab[~ok] = NONE
    win = np.where(ok, win, NAN)
    margin = np.where(ok, margin, 1.0)
    n = np.array([(lab == k).sum() for k in range(K)], np.int64)
    S = np.array([[math.fsum(u[lab == k, j]) for j in range(u.shape[1])] for k in range(K)]).reshape(K, u.shape[1])
    return lab, win, n, S, margin


def sum_abs(rows, lab, s, K):
    """sum |u| per mode and column [K, np]: what the bound on S is made of"""
    ok = finite_rows(rows)
    u = np.abs(scaled(np.where(ok[:, None], np.asarray(rows, np.float32), 0), s))
    return np.array([[math.fsum(u[lab == k, j]) for j in range(u.shape[1])] for k in range(K)]).reshape(K, u.shape[1])


def seed_uniform(seed, k):
    w = step_ref.philox4x32(k, 0, 0, 0, seed, ST_MODES)
    r = (int(w[0]) << 32) | int(w[1])
    return float(r >> 11) * 2.0 ** -53


def seed(rows, K, seed_, s):
    """the k-means++ indices [K] of include/mcx.h's mcx_modes_seed"""
    rows = np.asarray(rows, np.float32)
    s = np.asarray(s, np.float64)
    ok = finite_rows(rows)
    if ok.sum() < K:
        raise ValueError("fewer than k finite rows")
    ll = rows[:, -1].astype(np.float64)
    ll = np.where(np.isnan(ll), -np.inf, ll)
    valid = np.flatnonzero(ok)
    idx = [int(valid[np.argmax(ll[valid])])]  # (argmax: the first of equal maxima)
    u = scaled(np.where(ok[:, None], rows, 0), s)
    D = np.full(len(rows), np.inf)
    taken = np.zeros(len(rows), bool)
    taken[idx[0]] = True
    for k in range(1, K):
        d = dist2(u, u[idx[-1]][None, :], s)[:, 0]
        D = np.where(ok, np.minimum(D, d), 0.0)
        cum = np.cumsum(D)  # (a running sum in index order)
        total = cum[-1]
        pick = -1
        if total > 0.0 and math.isfinite(total):
            hit = np.flatnonzero(cum > seed_uniform(seed_, k) * total)
            pick = int(hit[0]) if len(hit) else int(np.flatnonzero(D > 0)[-1])
        if pick < 0 or taken[pick]:
            pick = int(np.flatnonzero(ok & ~taken)[0])
        idx.append(pick)
        taken[pick] = True
    return np.array(idx, np.int64)


def lloyd(rows, c0, s, max_iter=50):
    """the loop from scaled centres c0 [K, np]: dict of labels, iters, n_changed, flags, centres (scaled, the argmin's), n, S,
    n_nonfinite, margins (the least margin of every pass)"""
    c = np.array(c0, np.float64)
    K = c.shape[0]
    prev = np.full(len(rows), NONE, np.uint8)
    flags, margins = 0, []
    it = 0
    while True:
        it += 1
        lab, _win, n, S, margin = assign(rows, c, s)
        margins.append(float(margin.min()))
        changed = int((lab != prev).sum())
        if (n == 0).any():
            flags |= EMPTY
        if changed == 0:
            flags |= CONVERGED
            break
        if it == max_iter:
            flags |= NOT_CONVERGED
            break
        for k in range(K):
            if n[k] > 0:
                c[k] = S[k] / float(n[k])
        prev = lab
    return dict(labels=lab, iters=it, n_changed=changed, flags=flags, centres=c, n=n, S=S,
                n_nonfinite=int((lab == NONE).sum()), margins=margins)


def table(rows, lab, c, s):
    """the mode table of labels lab and scaled centres c: dict of n, weight, mean, sd (unscaled [K, np]), inertia, ll_mean,
    ll_max (float32), ll_max_row"""
    rows = np.asarray(rows, np.float32)
    K, p = c.shape
    ok = finite_rows(rows)
    u = scaled(np.where(ok[:, None], rows, 0), s)
    nvalid = int(ok.sum())
    out = dict(n=np.zeros(K, np.int64), weight=np.full(K, NAN), mean=np.full((K, p), NAN), sd=np.full((K, p), NAN),
               inertia=np.full(K, NAN), ll_mean=np.full(K, NAN), ll_max=np.full(K, NAN, np.float32), ll_max_row=np.full(K, -1, np.int64))
    d = dist2(u, c, s)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(K):
            mem = np.flatnonzero(lab == k)
            n = len(mem)
            out["n"][k] = n
            out["weight"][k] = n / nvalid if nvalid else NAN
            if n == 0:
                continue
            out["inertia"][k] = math.fsum(d[mem, k])
            ll = rows[mem, -1]
            if np.isfinite(ll).all():
                out["ll_mean"][k] = math.fsum(ll.astype(np.float64)) / n
            if not np.isnan(ll).any():
                out["ll_max"][k] = ll.max()
                out["ll_max_row"][k] = mem[np.argmax(ll)]
            for j in range(p):
                if s[j] == 0.0:
                    continue
                m = math.fsum(u[mem, j]) / n
                out["mean"][k, j] = m / s[j]
                out["sd"][k, j] = math.sqrt(math.fsum((u[mem, j] - m) ** 2) / (n - 1)) / s[j] if n > 1 else NAN
    return out


def chain_table(lab, T, nc, K):
    """integers from labels [T * nc]: dict of visits [nc, K], hops, dominant, dominant_steps, first_label, last_label [nc],
    trans [K, K], occupancy [T, K], in plain loops"""
    L = np.asarray(lab).reshape(T, nc).astype(np.int64)
    visits, trans, occ = np.zeros((nc, K), np.int64), np.zeros((K, K), np.int64), np.zeros((T, K), np.int64)
    hops = np.zeros(nc, np.int64)
    for t in range(T):
        for c in range(nc):
            cur = L[t, c]
            if cur == NONE:
                continue
            visits[c, cur] += 1
            occ[t, cur] += 1
            if t > 0 and L[t - 1, c] != NONE:
                trans[L[t - 1, c], cur] += 1
                hops[c] += cur != L[t - 1, c]
    dom = np.where(visits.max(1) > 0, visits.argmax(1), NONE)
    return dict(visits=visits, hops=hops, dominant=dom, dominant_steps=visits.max(1), first_label=L[0], last_label=L[-1],
                trans=trans, occupancy=occ)
