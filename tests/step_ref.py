"""A float64 model of the step loop, independent of the oracle -- test infrastructure only.

numpy float64 throughout, no ctypes, nothing imported from oracle_lib.  The model states the documented algorithm once
more -- generator, likelihoods, local step, tuner, Welford and adoption, Murray step -- and `replay_run` / `murray_step`
hold an engine (the CPU oracle or the GPU engine: both expose the same getters) against it.

The engines compute in fp32, the model in float64, so they agree only within bands.  Every band below is derived: it
counts the roundings u = 2^-24 of the fp32 path of §3 (per term, per level of a sum, per fma), multiplies by the float64
magnitudes involved, and adds the accuracy the fixed polynomials are held to by tests/test_oracle_numerics.py
(LOG1_ERR, EXP1_REL, SINCOS_ERR).  No band was fitted to make a case pass.  What the contract itself states in fp32 is
taken as stated, not banded: u24 (exact), uopen (an fp32 value: `fma(float(w), 2^-32, 2^-33)`, computed here exactly
and rounded once), the tuner's scale product and arate, the Murray weight w = 1/sigma^2 as the fp32 quotient.

The one constant that is measured, not derived, is NORMAL_DIST (see there).
"""
import math

import numpy as np

U = 2.0 ** -24                 # unit roundoff of fp32, round to nearest even
LOG1_ERR = 2e-7                # |log1(x) - ln x| <= LOG1_ERR max(1, |ln x|)      (tests/test_oracle_numerics.py)
EXP1_REL = 3e-7                # |exp1(x) - e^x| <= EXP1_REL e^x
SINCOS_ERR = 3e-7              # |sincos - sin, cos| <= SINCOS_ERR (inside NORMAL_DIST, which is measured)
FPEPS = float(np.float32(1e-14))   # the seed of psum2, qisum and qimax (src/mcpar.cc:15), an fp32 value
EXP_CUT = -125.5 * math.log(2.0)   # exp1(x) = 0 for floor(x log2 e + 1/2) < -125: everything below 2^-125.5, so no result is denormal
ST_LOCAL, ST_ACCEPT, ST_COIN, ST_RSEL, ST_RNORM = 0, 1, 2, 3, 4

VL_ROSENBROCK1, VL_ROSENBROCK2, VL_GAUSSIAN, VL_DUALGAUSS, VL_GAUSSMIX, VL_ROSENBROCK2_FIXED = 1, 2, 3, 4, 5, 6

# The distance of an fp32 normal of §3 from the float64 one of the same words, max |z32 - z64| / max(1, |z64|).
# It cannot be derived tightly: z = r c with r = sqrt(-2 ln u), and the absolute error LOG1_ERR of log1 becomes an
# unbounded relative error of r as u -> 1 (ln u -> 0).  Measured on the CPU, the oracle's mcxo_normal4 against
# `normals_from_words`: 2 200 000 random Philox blocks (8 800 000 normals, three streams): 2.645e-7; and, composed of the oracle's exported
# uopen / log1 / sincos as §3 composes them, the edge words w.x in {0, 1, 0xffffffff, 0xffffff7f, 0xffffff80, 0xfffffeff,
# 0xffffff00} (around where uopen reaches 1 and r = 0) crossed with every quadrant boundary of tests/test_gpu_numerics.py as
# the angle word: 1.18e-7.  A sample maximum underestimates the supremum, so the bands use 4 x the larger of the two
# (tests/test_step_ref_cpu.py::test_normal_distance_constant repeats a smaller measurement against the 4 x bound).
NORMAL_DIST_MEASURED = 2.65e-7
NORMAL_DIST = 4.0 * NORMAL_DIST_MEASURED

_M32 = np.uint64(0xffffffff)
_S32 = np.uint64(32)


def gamma(k):
    """k roundings of relative size U compound to at most k U / (1 - k U) (Higham, Accuracy and Stability, lemma 3.1)"""
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------------------------------------------
# generator
# ------------------------------------------------------------------------------------------------------------------
def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on uint64 arrays holding 32-bit words; counters broadcast against each other.
    Returns the four output words as uint64 arrays."""
    c0, c1, c2, c3 = [np.asarray(v, np.uint64) & _M32 for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(int(k0) & 0xffffffff), np.uint64(int(k1) & 0xffffffff)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2   # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _M32, (p0 >> _S32) ^ c3 ^ k1, p0 & _M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def u24(w):
    """[0, 1) on a 2^-24 grid: exact in either precision"""
    return (np.asarray(w, np.uint64) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def uopen(w):
    """(0, 1]: fma(float(w), 2^-32, 2^-33) as §3 states it, an fp32 value.  float(w) rounds w to 24 bits; the product and
    the sum are exact in float64 (at most 25 significant bits), so one rounding to fp32 is the fma's."""
    f = np.asarray(w, np.uint64).astype(np.float32).astype(np.float64)
    return (f * 2.0 ** -32 + 2.0 ** -33).astype(np.float32).astype(np.float64)


def mulhi(w, N):
    """the high word of the 32 x 32 bit product: an index in [0, N)"""
    return ((np.asarray(w, np.uint64) * np.uint64(N)) >> _S32).astype(np.int64)


def normals_from_words(w):
    """Box-Muller, both branches: words (0, 1) -> z0, z1; words (2, 3) -> z2, z3.  [..., 4] float64"""
    out = []
    for a, b in ((w[0], w[1]), (w[2], w[3])):
        r = np.sqrt(-2.0 * np.log(uopen(a)))
        ang = 2.0 * np.pi * (np.asarray(b, np.uint64).astype(np.float64) * 2.0 ** -32)
        out += [r * np.cos(ang), r * np.sin(ang)]
    return np.stack(out, -1)


def normals(seed, stream, t, g, d, a=None):
    """the d normals of chains g at step t: LOCAL blocks at counter (t, g, q, 0), RNORM blocks of pass a at (t, g, a, q).
    [len(g), d] float64"""
    nb = (d + 3) // 4
    g = np.asarray(g, np.uint64)
    blocks = []
    for q in range(nb):
        w = philox4x32(t, g, q, 0, seed, stream) if a is None else philox4x32(t, g, a, q, seed, stream)
        blocks.append(normals_from_words(w))
    return np.concatenate(blocks, -1)[:, :d]


def accept_u(seed, t, g):
    """the acceptance draw of step t: word t & 3 of the ACCEPT block (t >> 2, g, 0, 0)"""
    w = philox4x32(t >> 2, np.asarray(g, np.uint64), 0, 0, seed, ST_ACCEPT)
    return u24(w[t & 3])


def coin_u(seed, t):
    """the local/remote coin of step t, one for the whole job: word 0 of the COIN block (t, 0, 0, 0)"""
    return float(u24(philox4x32(t, 0, 0, 0, seed, ST_COIN)[0]))


def is_remote(seed, t, isamp, sync, pl):
    """main-loop step isamp is a Murray step when isamp >= SYNCSTEP and the coin exceeds PLOCAL (an fp32 value)"""
    return isamp >= sync and coin_u(seed, t) > float(np.float32(pl))


# ------------------------------------------------------------------------------------------------------------------
# likelihoods (§3.3).  Each returns (log L, mag, aux): mag is the sum of the magnitudes of the terms log L is a sum of.
# ------------------------------------------------------------------------------------------------------------------
def rosenbrock1(x):
    """-sum over the pairs (x_k, x_{k+1}), k even, of (1 - x_k)^2 + 100 (x_{k+1} - x_k^2)^2"""
    a, b = x[:, 0::2], x[:, 1::2]
    s = ((1.0 - a) ** 2 + 100.0 * (b - a * a) ** 2).sum(-1)
    return -s, s, None


def rosenbrock2_fixed(x):
    """-sum_{k < d-1} (1 - x_k)^2 + 100 (x_{k+1} - x_k^2)^2, the overlapping Rosenbrock function"""
    a, b = x[:, :-1], x[:, 1:]
    s = ((1.0 - a) ** 2 + 100.0 * (b - a * a) ** 2).sum(-1)
    return -s, s, None


def rosenbrock2(x):
    """the reference's Rosenbrock2 as written: one flat loop over all n d values, so chain j's last term reads chain
    j + 1's first parameter (the very last value has no term), and the second term is subtracted"""
    n, d = x.shape
    f = x.reshape(-1)
    nxt = np.concatenate([f[1:], [0.0]])
    t1, t2 = (1.0 - f) ** 2, 100.0 * (nxt - f * f) ** 2
    t1[-1] = t2[-1] = 0.0
    return -(t1 - t2).reshape(n, d).sum(-1), (t1 + t2).reshape(n, d).sum(-1), None


def gaussian(x, mu, s2):
    """-sum_k (x_k - mu_k)^2 / (2 sigma_k^2)"""
    s = (0.5 * (x - mu) ** 2 / s2).sum(-1)
    return -s, s, None


def mixture(x, means, wts):
    """log sum_c w_c exp(-|x - m_c|^2 / 2) as a log-sum-exp.  aux = (e [n, K], p [n, K] the components' shares, S [n, K] the
    squared distances)"""
    S = ((x[:, None, :] - means[None]) ** 2).sum(-1)
    e = -0.5 * S + np.log(wts)[None]
    emax = e.max(-1)
    ex = np.exp(e - emax[:, None])
    s = ex.sum(-1)
    ly = emax + np.log(s)
    p = ex / s[:, None]
    return ly, (p * 0.5 * S).sum(-1), (e, p, S)


class Likelihood:
    """one of the five likelihoods with its fp32 parameters.  value(x) -> (log L, mag, aux); band(...) the distance the
    fp32 evaluation of §3 may lie from it; sens(x, bx) how far log L moves when x moves by at most bx per coordinate."""

    def __init__(self, kind, d, params=None, ncomp=0):
        self.kind, self.d = kind, d
        p = None if params is None else np.asarray(params, np.float32).astype(np.float64)
        if kind == VL_GAUSSIAN:
            self.mu = p[:d] if p is not None else np.zeros(d)
            self.s2 = p[d:2 * d] if p is not None else np.ones(d)
        elif kind == VL_DUALGAUSS:
            self.means = np.array([[0.0, 0.0], [5.0, 5.0]])
            self.wts = np.array([p[0], 1.0])
        elif kind == VL_GAUSSMIX:
            self.means = p[:ncomp * d].reshape(ncomp, d)
            self.wts = p[ncomp * d:ncomp * d + ncomp]

    def value(self, x):
        k = self.kind
        if k == VL_ROSENBROCK1:
            return rosenbrock1(x)
        if k == VL_ROSENBROCK2:
            return rosenbrock2(x)
        if k == VL_ROSENBROCK2_FIXED:
            return rosenbrock2_fixed(x)
        if k == VL_GAUSSIAN:
            return gaussian(x, self.mu, self.s2)
        return mixture(x, self.means, self.wts)

    def levels(self):
        """additions one term passes on its way into the sum: 4 inside its block of 4 parameters (left to right from 0)
        and one per level of the butterfly over the blocks; Rosenbrock2 as written is one left-to-right loop"""
        if self.kind == VL_ROSENBROCK2:
            return self.d
        nb = (self.d + 3) // 4
        return 4 + int(math.ceil(math.log2(nb))) if nb > 1 else 4

    def band(self, ly, mag, aux):
        """|fp32 log L of §3 - ly| for the same fp32 x.

        Rosenbrock term fma(100 t2, t2, t1 t1): t1 = 1 - x and t2 = fma(-x, x, x') are one rounding each, so t1 t1 and
        (100 t2) t2 carry 2 U from their factor and 1 U of their own product (100 t2; t1 t1), and the fma adds 1 U:
        4 roundings on a term's magnitude t1^2 + 100 t2^2.  Gaussian term fma((0.5 a) a, 1 / sigma^2, acc): a = x - mu
        1 U, squared 2 U, the product 1 U, the quotient 1 / sigma^2 1 U: 4, and the fma's rounding is the sum's.  Then
        `levels()` additions, each 1 U of a partial sum that is at most mag: gamma(4 + levels) mag.

        Mixture: e_c = fma(-0.5, S_c, log1 w_c) with S_c a sum of fma(a, a, acc) (a: 2 U, then the levels):
        d_c = gamma(2 + levels) S_c / 2 + LOG1_ERR max(1, |ln w_c|) + U |e_c|.  Then e_c - e_max (U |e_c - e_max|, and both
        d_c and d_max move it), exp1 (EXP1_REL), K additions: the sum s moves by at most the p-weighted mean of
        rho_c = d_c + d_max + U |e_c - e_max| + EXP1_REL + K U relative (p_c = the components' shares); log1 s adds
        LOG1_ERR max(1, |ln s|) and the last addition U |ly|.  e_max itself moves by d_max.  (A component that exp1
        flushes to 0 lies 2^-125 below the largest, which is 1: nothing at this scale.)"""
        if self.kind in (VL_DUALGAUSS, VL_GAUSSMIX):
            e, p, S = aux
            K = e.shape[1]
            emax = e.max(-1)
            dc = gamma(2 + self.levels()) * 0.5 * S + LOG1_ERR * np.maximum(1.0, np.abs(np.log(self.wts)))[None] + U * np.abs(e)
            dmax = np.take_along_axis(dc, e.argmax(-1)[:, None], 1)[:, 0]
            rho = dc + dmax[:, None] + U * np.abs(e - emax[:, None]) + EXP1_REL + K * U
            lns = ly - emax
            return dmax + (p * rho).sum(-1) + LOG1_ERR * np.maximum(1.0, np.abs(lns)) + U * np.abs(ly)
        return gamma(4 + self.levels()) * mag

    def sens(self, x, bx):
        """sum_k |d log L / d x_k| bx_k (first order; bx is of the order 1e-6, the second order 1e-12 of the curvature)"""
        k = self.kind
        if k == VL_ROSENBROCK1:
            a, b = x[:, 0::2], x[:, 1::2]
            t2 = b - a * a
            return (np.abs(2.0 * (1.0 - a) + 400.0 * a * t2) * bx[:, 0::2] + np.abs(200.0 * t2) * bx[:, 1::2]).sum(-1)
        if k == VL_ROSENBROCK2_FIXED:
            a, b = x[:, :-1], x[:, 1:]
            t2 = b - a * a
            return (np.abs(2.0 * (1.0 - a) + 400.0 * a * t2) * bx[:, :-1] + np.abs(200.0 * t2) * bx[:, 1:]).sum(-1)
        if k == VL_ROSENBROCK2:
            n, d = x.shape
            f, bf = x.reshape(-1), bx.reshape(-1)
            nxt, bn = np.concatenate([f[1:], [0.0]]), np.concatenate([bf[1:], [0.0]])
            t2 = nxt - f * f
            s = np.abs(2.0 * (1.0 - f) - 400.0 * f * t2) * bf + np.abs(200.0 * t2) * bn
            s[-1] = 0.0
            return s.reshape(n, d).sum(-1)
        if k == VL_GAUSSIAN:
            return (np.abs(x - self.mu) / self.s2 * bx).sum(-1)
        _, _, (e, p, S) = self.value(x)
        g = (p[:, :, None] * (self.means[None] - x[:, None, :])).sum(1)
        return (np.abs(g) * bx).sum(-1)

    def evaluate(self, x, bx=None):
        """(log L, band): band bounds |engine's fp32 log L at its own x - log L| when the engine's x lies within bx of x"""
        ly, mag, aux = self.value(x)
        b = self.band(ly, mag, aux)
        if bx is not None:
            b = b + self.sens(x, bx)
        return ly, b


# ------------------------------------------------------------------------------------------------------------------
# local step
# ------------------------------------------------------------------------------------------------------------------
def local_trial(x, T, z):
    """x' = x + T z, T lower triangular.  (x', band): row i is a chain of one fma per non-zero T_ij, each 1 U of a partial
    sum that is at most |x_i| + sum_j |T_ij z_j| -- a zero T_ij makes its fma exact, which is why the count is of the
    non-zeros -- and z_j itself lies within NORMAL_DIST max(1, |z_j|) of the fp32 normal."""
    T = np.tril(T)
    xp = x + z @ T.T
    aT = np.abs(T)
    nnz = (T != 0).sum(1).astype(np.float64)
    band = gamma(nnz)[None, :] * (np.abs(x) + np.abs(z) @ aT.T) + (NORMAL_DIST * np.maximum(1.0, np.abs(z))) @ aT.T
    return xp, band


def log_u(u):
    with np.errstate(divide="ignore"):
        return np.log(u)   # -inf at u = 0


def band_log_u(lu):
    """log1 of the acceptance draw: LOG1_ERR max(1, |ln u|); the -inf of u = 0 is exact"""
    return np.where(np.isfinite(lu), LOG1_ERR * np.maximum(1.0, np.abs(np.where(np.isfinite(lu), lu, 0.0))), 0.0)


def cholesky_check(incov, chol):
    """A float64 Cholesky of incov against the engine's fp32 factor.  Backward: the computed factor satisfies
    |L L^T - A| <= gamma(d + 1) |L| |L|^T (Higham, theorem 10.3; the fma form has no more roundings).  Forward, first order
    (Sun 1991): ||L - L64||_F <= kappa_2(A) ||dA||_F ||L||_F / (sqrt(2) ||A||_2) with ||dA||_F <= gamma(d + 1) ||L||_F^2.
    Returns (backward excess, forward excess), both <= 1 when the factor is right."""
    A = np.asarray(incov, np.float32).astype(np.float64)
    L = np.asarray(chol, np.float32).astype(np.float64)
    d = A.shape[0]
    assert np.all(np.triu(L, 1) == 0)
    back = np.abs(L @ L.T - A) / (gamma(d + 1) * (np.abs(L) @ np.abs(L).T))
    L64 = np.linalg.cholesky(A)
    nL = np.linalg.norm(L64)
    fwd = np.linalg.norm(L - L64) / (np.linalg.cond(A) * gamma(d + 1) * nL ** 3 / (math.sqrt(2.0) * np.linalg.norm(A, 2)))
    return float(back.max()), float(fwd)


# ------------------------------------------------------------------------------------------------------------------
# Murray step
# ------------------------------------------------------------------------------------------------------------------
def exp_cut(x):
    """exp with §3's flush: 0 below 2^-125.5"""
    with np.errstate(under="ignore", over="ignore"):
        return np.where(x >= EXP_CUT, np.exp(x), 0.0)


def murray_args(x, bx, mu, w, bmu, relw, own=None, bx_own=None):
    """arg[j, i] = sum_k (mu_ik - x_jk)^2 w_ik and its band.

    fp32 path: xm = mu - x (1 U), xm xm (2 U + 1 U), then fma(xm xm, w, arg) ascending k: d levels on sums of positive
    terms -> gamma(d + 3) arg.  The engine's mu, x and w lie within bmu, bx and relw (relative) of the model's: with
    e = bmu + bx, (xm + e)^2 - xm^2 = 2 xm e + e^2 exactly (the square term matters: w reaches 1e14 for a chain that has
    not moved), and the weight's share is xm^2 w relw.  own / bx_own: chain j's x was drawn from Gaussian own[j] as
    mu + sigma z, so against that Gaussian the engine forms fl(mu~ - fl(mu~ + sigma~ z~)) with one and the same mu~: the
    distance of its mean from the model's cancels, and e is bx_own, the band of x without the mean's share."""
    n, d = x.shape
    N = mu.shape[0]
    a, da = np.empty((n, N)), np.empty((n, N))
    step = max(1, int(2.0e6 // max(1, N * d)))
    for i0 in range(0, n, step):
        i1 = min(n, i0 + step)
        xm = mu[None] - x[i0:i1, None, :]
        e = bmu[None] + bx[i0:i1, None, :]
        t = xm * xm * w[None]
        a[i0:i1] = t.sum(-1)
        da[i0:i1] = ((2.0 * np.abs(xm) * e + e * e) * w[None] + t * relw[None]).sum(-1)
    if own is not None:
        j = np.arange(n)
        xm, e = mu[own] - x, bx_own
        da[j, own] = ((2.0 * np.abs(xm) * e + e * e) * w[own] + xm * xm * w[own] * relw[own]).sum(-1)
    return a, da + gamma(d + 3) * a


def _grow(rho):
    """a relative shift rho of an exponent moves the exponential by at most e^rho - 1"""
    return np.expm1(np.minimum(rho, 60.0))


class MurrayResult:
    pass


def murray_step(seed, t, g, N, x, bx, mu, s2, bmu, bs2, known=None, known_x=None, maxpass=20000):
    """One Murray step (genRemote) of the chains with global ids g at state x against the N Gaussians (mu, s2).

    bx, bmu, bs2: how far the engine's fp32 state and moments may lie from the model's (zeros when they are given
    exactly).  known (bool [n]) / known_x: chains whose accepted trial the engine recorded -- their pass is the one whose
    trial matches known_x, every earlier pass must be a rejection and that one an acceptance; all other chains follow the
    model's own decisions.  A pass decision inside its band makes the chain `undecided`.

    Per pass (counter (t, g, pass, .)): sel = mulhi(w0, N); x' = mu_sel + sqrt(s2_sel) z (RNORM normals);
    Q_i = exp(-arg_i(x') / 2) flushed; qisum = FPEPS + sum Q_i; qimax = max(FPEPS, Q_i); accept when u24(w1) < qimax / qisum.
    cfac = max_i Q_i(x) / qimax, the numerator flushed too, = exp(-min_i arg_i(x) / 2).

    Bands.  Q_i moves by e^rho_i - 1 relative, rho_i = darg_i / 2 + EXP1_REL + U (the halving is exact, the product
    rounding is not counted twice).  qisum: sum_i Q_i (e^rho_i - 1), plus the summation order -- blocks of 256 left to
    right, block sums left to right: at most min(N, 256) + ceil(N / 256) additions over a term, gamma of that times
    qisum -- plus N 2^-125 for terms on either side of the flush.  qimax: a maximum moves by at most the largest move of
    its candidates.  pacpt = qimax / qisum adds 1 U.  x': sqrt (1 U), fma (1 U of |x'|), z within NORMAL_DIST, and the
    donor's moments within (bmu, bs2): d sigma = bs2 / (2 sigma)."""
    g = np.asarray(g, np.int64)
    n, d = x.shape
    w = (np.float32(1.0) / s2.astype(np.float32)).astype(np.float64)   # the fp32 quotient: part of the contract
    relw = np.where(bs2 > 0, bs2 / s2 + 2.0 * U, 0.0)
    lsum = min(N, 256) + (N + 255) // 256
    res = MurrayResult()
    # the numerator of cfac: independent of the pass
    a0, da0 = murray_args(x, bx, mu, w, bmu, relw)
    amin = a0.min(1)
    cand = (a0 - da0) <= (a0 + da0).min(1)[:, None]   # who could be the minimum in the engine
    damin = np.where(cand, da0, 0.0).max(1)
    cmax = exp_cut(-0.5 * amin)
    res.cmax_amb = np.abs(-0.5 * amin - EXP_CUT) <= 0.5 * damin + 2.0 * U * abs(EXP_CUT)   # either side of the flush
    relcmax = _grow(0.5 * damin + EXP1_REL + U)
    res.passes = np.full(n, -1, np.int64)
    res.sel = np.zeros(n, np.int64)
    res.xt, res.bxt = np.zeros((n, d)), np.zeros((n, d))
    res.cfac, res.relcfac = np.zeros(n), np.zeros(n)
    res.undecided = np.zeros(n, bool)
    res.pairs = 0
    known = np.zeros(n, bool) if known is None else np.asarray(known, bool)
    live = np.arange(n)
    p = 0
    while live.size:
        assert p < maxpass, "Murray step does not end: %d chains left after %d passes" % (live.size, p)
        wd = philox4x32(t, g[live].astype(np.uint64), p, 0, seed, ST_RSEL)
        sel = mulhi(wd[0], N)
        u = u24(wd[1])
        z = normals(seed, ST_RNORM, t, g[live], d, a=p)
        sig = np.sqrt(s2[sel])
        xt = mu[sel] + sig * z
        bxt = (bmu[sel] + np.abs(z) * bs2[sel] / (2.0 * sig) + U * np.abs(sig * z) + sig * NORMAL_DIST * np.maximum(1.0, np.abs(z))
               + U * np.abs(xt))
        a, da = murray_args(xt, bxt, mu, w, bmu, relw, own=sel, bx_own=bxt - bmu[sel])
        res.pairs += a.size
        Q = exp_cut(-0.5 * a)
        dQ = Q * _grow(0.5 * da + EXP1_REL + U)
        qs = FPEPS + Q.sum(1)
        qm = np.maximum(FPEPS, Q.max(1))
        dqs = dQ.sum(1) + gamma(lsum) * qs + N * 2.0 ** -125
        dqm = dQ.max(1)
        pac = qm / qs
        dpac = pac * (dqm / qm + dqs / qs + U)
        dec = u < pac
        inband = np.abs(u - pac) <= dpac
        kn = known[live]
        match = np.zeros(live.size, bool)
        if kn.any():
            match[kn] = np.all(np.abs(known_x[live[kn]] - xt[kn]) <= bxt[kn], axis=1)
        # a recorded chain: decided by the record; any other: by the model
        bad = kn & ~inband & (match != dec)
        assert not bad.any(), ("Murray pass %d at t = %d: chains %s: the recorded trial %s this pass's, the model's pass decision is "
                               "the opposite, outside the band" % (p, t, g[live[bad]][:5], "is" if match[bad][0] else "is not"))
        res.undecided[live[inband]] = True
        taken = np.where(kn, match, dec | inband)   # an unrecorded chain inside the band stops here, undecided
        idx = live[taken]
        res.passes[idx] = p
        res.sel[idx] = sel[taken]
        res.xt[idx], res.bxt[idx] = xt[taken], bxt[taken]
        res.cfac[idx] = cmax[idx] / qm[taken]
        res.relcfac[idx] = relcmax[idx] + dqm[taken] / qm[taken] + 2.0 * U
        live = live[~taken]
        p += 1
    res.npass = p
    return res


def cfac_band(res):
    """|engine's cfac - model's|: relative, and the whole value where the numerator lies at the flush"""
    return res.cfac * res.relcfac + np.where(res.cmax_amb, np.maximum(res.cfac, 2.0 ** -125 / FPEPS), 0.0)


# ------------------------------------------------------------------------------------------------------------------
# whole runs
# ------------------------------------------------------------------------------------------------------------------
class Config:
    def __init__(self, d, n, nburn, nsamp, lik, pinit, chol0, pl=0.9, armin=0.2, armax=0.5, dfac=0.2, ifac=1.5, sync=10,
                 seed=8675309, tbase=0):
        self.d, self.n, self.nburn, self.nsamp, self.lik = d, n, nburn, nsamp, lik
        self.pinit = np.asarray(pinit, np.float32).reshape(n, d)
        self.chol0 = np.asarray(chol0, np.float32).reshape(d, d)
        self.pl, self.armin, self.armax, self.dfac, self.ifac = pl, armin, armax, dfac, ifac
        self.sync, self.seed, self.tbase = sync, seed, tbase


def record_of(eng, remote_steps, remote_passes, naccept_burn, naccept_main, mask=True):
    """what replay_run reads of a finished engine (the oracle's and the GPU engine's getters have the same names)"""
    nsamp, n, d = eng.nsamp, eng.nc, eng.np
    return dict(rows=eng.samples.reshape(nsamp, n, d + 1), mask=eng.accept_mask.astype(bool) if mask else None,
                state=eng.state, loglike=eng.loglike, mean=eng.mean, var=eng.var, musigall=eng.musigall,
                accept_counts=eng.accept_counts, tuner_trace=eng.tuner_trace, chol=eng.chol,
                remote_steps=remote_steps, remote_passes=remote_passes, naccept_burn=naccept_burn, naccept_main=naccept_main)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def replay_run(cfg, rec):
    """Teacher-forced replay of one single-shard run against the model.  rec: record_of(engine).

    Burn-in has no rows: the state follows the model's own arithmetic, steered by the recorded mask, and the bands of x
    and log L grow with every accepted step.  From the first main step on the state is re-seated on the recorded row
    after every step (its band is then 0).  Without a mask (the GPU's hot-path kernels record none) the burn-in follows
    the model's own decisions -- a chain with a decision inside the band is `lost` until the first row re-seats it, and
    everything that depends on it is not checked -- and a main-loop step counts as accepted when its row changed.

    Checked at every step: (1) the decision equals the mask unless |delta - ln u| is inside the band; (2) an accepted
    row equals x' within the state band; (3) a rejected row equals the previous row bit for bit; (4) the row's log L
    equals the model's likelihood of the row; (5) local or Murray step as the coin and SYNCSTEP say (a wrong kind fails
    (2), and the count of Murray steps is compared).  At the end: state, loglike, accept counts, the tuner trace and
    the factor exactly; mean, var, musigall within the Welford bands.

    Welford bands (running, per element; at most linear in the number of steps: every step adds terms of the order U
    times the current magnitudes, and what was there is carried over with a factor <= 1).  With e the engine's mu minus the
    model's, mu' = fl(mu + w~ fl(x - mu)) gives e' = (1 - w) e + w r1 + delta (w~ - w) + r2 with |r1| <= U (|delta| + |e|) the
    subtraction's rounding, |w~ - w| <= U w the host-rounded 1 / pwgt and |r2| <= U |mu'| the fma's:
    bmu' = (1 - w) bmu + w U (2 |delta| + bmu) + U |mu'|.  delta itself lies within bdelta = U |delta| + bmu.
    S' = fma(delta, x - mu', S): bS' = bS + |x - mu'| bdelta + |delta| (U |x - mu'| + bmu') + U |S'|.  sigma^2 = S' w:
    bS' w + 2 U sigma^2.  Where delta = 0 with nothing uncertain (a chain that has not moved since the moments started)
    every operation is exact and the bands stay 0.  Adoption: mu, sigma^2 <- the donor's published pair with its bands,
    sigma^2 through sqrt and square (3 U); S = sigma^2 (pwgt - 1): 1 U.

    Returns the counts of the run."""
    d, n, nburn, nsamp, lik, seed = cfg.d, cfg.n, cfg.nburn, cfg.nsamp, cfg.lik, cfg.seed
    rows, mask = rec["rows"], rec["mask"]
    rx = rows[:, :, :d].astype(np.float64)
    rly = rows[:, :, d].astype(np.float32)
    g = np.arange(n)
    x, bx = cfg.pinit.astype(np.float64), np.zeros((n, d))
    ly, bly = lik.evaluate(x)
    T32 = cfg.chol0.copy()
    nt = na = 0
    na_unsure = 0
    irate = 50
    trace = []
    lost = np.zeros(n, bool)
    ever_lost = np.zeros(n, bool)
    nacc_slack = main_slack = 0
    counts = np.zeros(n, np.int64)
    st = dict(local_decisions=0, local_inband=0, murray_steps=0, murray_decisions=0, murray_inband=0, murray_chain_steps=0,
              murray_undecided=0, murray_undecided_max_share=0.0, murray_pairs=0, lost=0, remote_passes=0, max_state_excess=0.0,
              max_ly_excess=0.0)
    any_undecided = False
    nacc_burn = nacc_main = 0
    # moments
    mu = np.zeros((n, d)); S = np.full((n, d), FPEPS); s2 = np.zeros((n, d))
    bmu = np.zeros((n, d)); bS = np.zeros((n, d)); bs2 = np.zeros((n, d))
    pmu, ps2, pbmu, pbs2 = mu.copy(), s2.copy(), bmu.copy(), bs2.copy()   # as published into musigall
    pw = 0
    prev_bits = None
    for s in range(nburn + nsamp):
        t = cfg.tbase + s
        main = s >= nburn
        isamp = s - nburn
        remote = main and is_remote(seed, t, isamp, cfg.sync, cfg.pl)
        u = accept_u(seed, t, g)
        if main:
            row_x, row_ly = rx[isamp], rly[isamp]
            bits = rows[isamp].view(np.uint32)
            if mask is not None:
                m = mask[s].copy()
            elif prev_bits is not None:
                m = np.any(bits != prev_bits, axis=1)
            else:
                m = None   # decided below: the first row against x and x'
        else:
            m = mask[s].copy() if mask is not None else None
        mres = None
        if not remote:
            z = normals(seed, ST_LOCAL, t, g, d)
            xp, bstep = local_trial(x, T32.astype(np.float64), z)
            bxp = bx + bstep
        else:
            mres = murray_step(seed, t, g, n, x, bx, pmu, ps2, pbmu, pbs2, known=m, known_x=row_x)
            xp, bxp = mres.xt, mres.bxt
            st["murray_steps"] += 1
            st["murray_pairs"] += mres.pairs
        if main and m is None:   # no mask, first row: accepted where the row is x' (lost chains: wherever it is not x)
            isxp = np.all(np.abs(row_x - xp) <= bxp, axis=1)
            isx = np.all(np.abs(row_x - x) <= bx, axis=1)
            assert np.all(isxp | isx | lost), "first row is neither x nor x' for chains %s" % np.flatnonzero(~(isxp | isx | lost))[:5]
            m = isxp & ~(isx & ~isxp)
            main_slack = int((lost & ~isxp & ~isx).sum())   # a lost chain off both: its first decision is not known
        # the hybrid trial: the recorded row where the step was accepted (exact), the model's x' elsewhere
        if main:
            xh = np.where(m[:, None], row_x, xp)
            bxh = np.where(m[:, None], 0.0, bxp)
            exc = np.abs(row_x - xp) / np.maximum(bxp, 1e-300)
            exc = np.where((m & ~lost)[:, None], exc, 0.0)
            if mres is not None:
                exc = np.where(mres.undecided[:, None], 0.0, exc)   # (a recorded chain matched its pass already)
            st["max_state_excess"] = max(st["max_state_excess"], float(exc.max()))
            assert exc.max() <= 1.0, "step %d: accepted rows off x' by %.3g bands (chain %d)" % (s, exc.max(), int(exc.max(1).argmax()))
        else:
            xh, bxh = xp, bxp
        lyp, blyp = lik.evaluate(xh, bxh)
        if main:   # (4) the row's log L is the likelihood of the row
            chk = m & ~lost
            e4 = np.where(chk, np.abs(row_ly.astype(np.float64) - lyp) / np.maximum(blyp, 1e-300), 0.0)
            st["max_ly_excess"] = max(st["max_ly_excess"], float(e4.max()))
            assert e4.max() <= 1.0, "step %d: log L of an accepted row off by %.3g bands (chain %d)" % (s, e4.max(), int(e4.argmax()))
            keep = ~m & ~lost
            if prev_bits is not None:   # (3) a rejected row is the previous row
                assert np.array_equal(bits[~m], prev_bits[~m]), "step %d: a rejected chain's row changed" % s
            else:   # the first row of a rejected chain is where the burn-in left it
                assert np.all(np.abs(row_x - x)[keep] <= bx[keep]) and np.all(np.abs(row_ly.astype(np.float64) - ly)[keep] <= bly[keep]), \
                    "first row of a rejected chain is not the state after the burn-in"
        # (1) the decision
        if main:
            # accepted after a re-seated step: both log L are recorded fp32 values, so the engine's own difference is known exactly
            prev_exact = bly == 0
            d32 = (row_ly - ly.astype(np.float32)).astype(np.float64)
            delta = np.where(m, np.where(prev_exact, d32, row_ly.astype(np.float64) - ly), lyp - ly)
            bdelta = np.where(m, np.where(prev_exact, 0.0, bly + U * np.abs(delta)), blyp + bly + U * np.abs(delta))
        else:
            delta = lyp - ly
            bdelta = blyp + bly + U * np.abs(delta)
        if not remote:
            lu = log_u(u)
            with np.errstate(invalid="ignore"):
                gap = np.abs(delta - lu)
            band = bdelta + band_log_u(lu)
            dec = lu < delta
            inband = gap <= band
            inband = np.where(np.isnan(gap), False, inband)
            st["local_decisions"] += n
            st["local_inband"] += int(inband.sum())
            und = np.zeros(n, bool)
        else:
            # u24 < exp1(ly' - ly) cfac: the exponent within bdelta, exp1 EXP1_REL, cfac within its band, the product 1 U
            cf, bcf = mres.cfac, cfac_band(mres)
            ex = exp_cut(delta)
            with np.errstate(over="ignore", invalid="ignore"):
                P = ex * cf
                bP = P * (_grow(bdelta) + EXP1_REL + U) + ex * bcf * (1.0 + _grow(bdelta))
            near_cut = np.abs(delta - EXP_CUT) <= bdelta + 2.0 * U * abs(EXP_CUT)
            bP = np.where(near_cut, np.maximum(bP, np.exp(np.minimum(delta, 0.0)) * (cf + bcf) * 2.0), bP)
            dec = u < P
            inband = np.abs(u - P) <= bP
            inband = np.where(np.isfinite(P), inband, False)
            und = mres.undecided.copy()
            st["murray_decisions"] += n
            st["murray_inband"] += int((inband & ~und).sum())
            und |= inband
            st["murray_chain_steps"] += n
            st["murray_undecided"] += int(und.sum())
            st["murray_undecided_max_share"] = max(st["murray_undecided_max_share"], float(und.mean()))
            any_undecided |= bool((mres.undecided & ~m).any())   # (a recorded chain's pass is known from its row)
            st["remote_passes"] += mres.npass
        if m is None:   # burn-in without a mask: the model decides
            newly = inband & ~lost
            lost |= newly
            ever_lost |= newly
            na_unsure += int(newly.sum())
            nacc_slack += int(newly.sum()) * (nburn - s)   # a lost chain's later burn-in decisions are its own
            m = dec
        else:
            skip = lost | und if remote else lost
            bad = (dec != m) & ~inband & ~skip
            assert not bad.any(), ("step %d (%s): %d decisions differ outside the band, e.g. chain %d: delta %.9g, u %.9g, band %.3g"
                                   % (s, "Murray" if remote else "local", bad.sum(), np.flatnonzero(bad)[0], delta[np.flatnonzero(bad)[0]],
                                      u[np.flatnonzero(bad)[0]], (bP if remote else band)[np.flatnonzero(bad)[0]]))
        counts += m
        # the state after the step
        if main:
            if lost.any():
                st["lost"] += int(lost.sum())
                lost[:] = False
            x, bx = row_x.copy(), np.zeros((n, d))
            ly, bly = row_ly.astype(np.float64), np.zeros(n)
            prev_bits = bits
            nacc_main += int(m.sum())
        else:
            x = np.where(m[:, None], xp, x)
            bx = np.where(m[:, None], bxp, bx)
            ly = np.where(m, lyp, ly)
            bly = np.where(m, blyp, bly)
            nacc_burn += int(m.sum())
            # the tuner: integer counters, arate and the scale product in fp32
            nt += n
            na += int(m.sum())
            if s > irate:
                arate = np.float32(na) / np.float32(nt)
                slack = int(ever_lost.sum()) * 50 + na_unsure   # (a lost chain may differ at every step since the last event)
                lo, hi = np.float32(max(na - slack, 0)) / np.float32(nt), np.float32(min(na + slack, nt)) / np.float32(nt)
                branch = lambda r: -1 if r < np.float32(cfg.armin) else (1 if r > np.float32(cfg.armax) else 0)
                assert branch(lo) == branch(hi) == branch(arate), "the tuner's branch hangs on decisions inside the band: choose another case"
                if branch(arate):
                    nt = na = na_unsure = 0
                    T32 = (T32 * np.float32(cfg.dfac if branch(arate) < 0 else cfg.ifac)).astype(np.float32)
                irate += 50
                trace.append(T32[0, 0])
        if not main:
            continue
        # Welford, adoption, publication
        pw += 1
        w = 1.0 / pw
        if remote:
            ad = m
            sel = mres.sel
            dmu, ds2 = pmu[sel], ps2[sel]
            mu = np.where(ad[:, None], dmu, mu)
            bmu = np.where(ad[:, None], pbmu[sel], bmu)
            s2a_b = pbs2[sel] + 3.0 * U * ds2
            S = np.where(ad[:, None], ds2 * (pw - 1.0), S)
            bS = np.where(ad[:, None], s2a_b * (pw - 1.0) + U * np.abs(ds2 * (pw - 1.0)), bS)
        delta_ = x - mu
        exact = (delta_ == 0) & (bmu == 0)
        bd = np.where(exact, 0.0, U * np.abs(delta_) + bmu)
        mu_n = mu + delta_ * w
        bmu_n = np.where(exact, bmu, (1.0 - w) * bmu + w * U * (2.0 * np.abs(delta_) + bmu) + U * np.abs(mu_n))
        r_ = x - mu_n
        S_n = S + delta_ * r_
        bS_n = np.where(exact, bS, bS + np.abs(r_) * bd + np.abs(delta_) * (U * np.abs(r_) + bmu_n) + U * np.abs(S_n))
        if pw == 1:   # mu = 0, S = FPEPS, w = 1: delta = x, mu' = x, S' = FPEPS, all exact
            bmu_n, bS_n = np.zeros((n, d)), np.zeros((n, d))
        mu, S, bmu, bS = mu_n, S_n, bmu_n, bS_n
        s2 = S * w
        bs2 = bS * w + 2.0 * U * np.abs(s2)
        pmu, ps2, pbmu, pbs2 = mu.copy(), s2.copy(), bmu.copy(), bs2.copy()
    # the end of the run
    if nsamp > 0:
        assert _same_bits(rec["state"], rows[-1][:, :d]) and _same_bits(rec["loglike"], rows[-1][:, d]), "state / loglike are not the last row"
        ok = np.isfinite(bmu)
        for name, got, ref, b in (("mean", rec["mean"], mu, bmu), ("var", rec["var"], s2, bs2),
                                  ("musigall mu", rec["musigall"][:, :, 0], mu, bmu), ("musigall var", rec["musigall"][:, :, 1], s2, bs2)):
            exc = np.where(ok, np.abs(got.astype(np.float64) - ref) / np.maximum(b, 1e-300), 0.0)
            exc = np.where(ok & (b == 0), np.where(got.astype(np.float64) == ref, 0.0, np.inf), exc)
            st["max_%s_excess" % name.replace(" ", "_")] = float(exc.max())
            assert exc.max() <= 1.0, "%s off by %.3g Welford bands at %s" % (name, exc.max(), np.unravel_index(exc.argmax(), exc.shape))
        st["moments_unchecked"] = int((~ok).any(1).sum())
    else:
        keep = ~lost
        assert np.all(np.abs(rec["state"].astype(np.float64) - x)[keep] <= bx[keep]), "state after the burn-in off the model's"
        assert np.all(np.abs(rec["loglike"].astype(np.float64) - ly)[keep] <= (bly + lik.sens(x, bx))[keep])
    if mask is not None:
        assert np.array_equal(rec["accept_counts"].astype(np.int64), counts), "accept_counts are not the mask's column sums"
        assert rec["naccept_burn"] == nacc_burn and rec["naccept_main"] == nacc_main
    else:
        assert abs(rec["naccept_burn"] - nacc_burn) <= nacc_slack and abs(rec["naccept_main"] - nacc_main) <= main_slack, \
            (rec["naccept_burn"], nacc_burn, nacc_slack, rec["naccept_main"], nacc_main, main_slack)
        assert np.array_equal(rec["accept_counts"].astype(np.int64)[~ever_lost], counts[~ever_lost]), "accept_counts are not the decisions' sums"
    assert rec["remote_steps"] == st["murray_steps"], "Murray steps: engine %d, coin and SYNCSTEP %d" % (rec["remote_steps"], st["murray_steps"])
    if not any_undecided:
        assert rec["remote_passes"] == st["remote_passes"], "Murray passes: engine %d, model %d" % (rec["remote_passes"], st["remote_passes"])
    assert _same_bits(rec["tuner_trace"], np.array(trace, np.float32)), "tuner trace: engine %s, model %s" % (rec["tuner_trace"], trace)
    assert _same_bits(rec["chol"], T32), "the factor after the run is not the installed one times the tuner's scales"
    st["passes_compared"] = not any_undecided
    return st


def check_caps(st, label=""):
    """the caps of a case: at most 0.2 % of the local decisions inside the band, at most 2 % of the chains of any Murray
    step undecided.  Prints the counts."""
    share = st["local_inband"] / max(1, st["local_decisions"])
    print("%s local decisions %d, inside the band %d (%.4f %%), lost %d | Murray steps %d, chain-steps %d, undecided %d (largest share "
          "of one step %.3f %%), passes %d%s, pairs %.3g | largest excess: state %.3g, log L %.3g, moments %s"
          % (label, st["local_decisions"], st["local_inband"], 100 * share, st["lost"], st["murray_steps"], st["murray_chain_steps"],
             st["murray_undecided"], 100 * st["murray_undecided_max_share"], st["remote_passes"], "" if st["passes_compared"] else " (not compared)",
             st["murray_pairs"], st["max_state_excess"], st["max_ly_excess"],
             ", ".join("%.3g" % st[k] for k in ("max_mean_excess", "max_var_excess") if k in st)))
    assert share <= 0.002, "%.4f %% of the local decisions inside the band" % (100 * share)
    assert st["murray_undecided_max_share"] <= 0.02, "%.3f %% of the chains of one Murray step undecided" % (100 * st["murray_undecided_max_share"])


# ------------------------------------------------------------------------------------------------------------------
# the single-step entry points
# ------------------------------------------------------------------------------------------------------------------
def check_gen_local(seed, t, g, x, chol, ptrial, cfac):
    """genLocal's output against x + T z; returns the largest excess over the band"""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    z = normals(seed, ST_LOCAL, t, g, x64.shape[1])
    xp, b = local_trial(x64, np.asarray(chol, np.float32).astype(np.float64), z)
    exc = np.abs(ptrial.astype(np.float64) - xp) / b
    assert exc.max() <= 1.0, "genLocal off by %.3g bands at %s" % (exc.max(), np.unravel_index(exc.argmax(), exc.shape))
    assert np.all(cfac == 1.0)
    return float(exc.max())


def check_gen_remote(seed, t, g, N, x, musigall, out, label=""):
    """genRemote's output (ptrial, cfac, mutrial, sigtrial, npass) against murray_step, per chain with no undecided pass:
    ptrial within its band (which also fixes the pass taken: every pass draws its own trial), mutrial exactly the donor's
    mean, sigtrial the donor's variance through sqrt and square (3 U), cfac within its band; npass when no chain is
    undecided.  At most 2 % of the chains may be undecided.  Prints and returns the counts."""
    pt, cf, mt, sg, npass = out
    ms = np.asarray(musigall, np.float32).astype(np.float64)
    mu, s2 = ms[:, :, 0], ms[:, :, 1]
    x64 = np.asarray(x, np.float32).astype(np.float64)
    zero, zeroN = np.zeros_like(x64), np.zeros_like(mu)
    res = murray_step(seed, t, g, N, x64, zero, mu, s2, zeroN, zeroN)
    ok = ~res.undecided
    nund = int(res.undecided.sum())
    print("%s genRemote %d-D x %d over %d: passes model %d engine %d, undecided chains %d, pairs %d, cfac in [%.3g, %.3g], flushed %d"
          % (label, x64.shape[1], x64.shape[0], N, res.npass, npass, nund, res.pairs, cf.min(), cf.max(), int((res.cfac == 0).sum())))
    exc = np.abs(pt.astype(np.float64) - res.xt)[ok] / res.bxt[ok]
    assert exc.max() <= 1.0, "ptrial off by %.3g bands" % exc.max()
    assert _same_bits(mt[ok], mu[res.sel][ok]), "mutrial is not the selected chain's mean"
    assert np.all(np.abs(sg.astype(np.float64) - s2[res.sel])[ok] <= gamma(3) * s2[res.sel][ok]), "sigtrial is not the selected chain's variance"
    excf = (np.abs(cf.astype(np.float64) - res.cfac) - cfac_band(res))[ok]
    assert excf.max() <= 0.0, "cfac: engine %.9g, model %.9g, band %.3g (chain %d)" % (
        cf[ok][excf.argmax()], res.cfac[ok][excf.argmax()], cfac_band(res)[ok][excf.argmax()], np.flatnonzero(ok)[excf.argmax()])
    if nund == 0:
        assert npass == res.npass, "passes: engine %d, model %d" % (npass, res.npass)
    assert nund <= 0.02 * x64.shape[0], "%d of %d chains undecided" % (nund, x64.shape[0])
    return dict(npass=res.npass, undecided=nund, flushed=int((res.cfac == 0).sum()), ambiguous=int(res.cmax_amb.sum()))
