// mcx_evidence_host.hpp -- the host half of the evidence of a store: what a call refuses, the proposal's
// factors (Cholesky factor C of scale^2 Sigma, W = C^-1 and the constant lc per component), the uniform that picks a draw's
// component, the terms of a bridge pass, of the error and of the two by-products, and the update and finish of the iterative
// estimator of Meng & Wong.  Plain C++ in fp64, no HIP and no library state: mcx_evidence.hip calls these very functions (the
// term functions inside its kernels too: MCX_EV_HD), and a host-only program can include this header alone.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#if defined(__HIPCC__)
#define MCX_EV_HD __host__ __device__ inline
#else
#define MCX_EV_HD inline
#endif

namespace mcx_evidence_host {

// Philox stream of the proposal's draws.  The step kernels use streams 0-4, section 12's draws 5, section 21's permutations 6
// and section 25's seeding 7; the constant lives here because no other unit has any business with it
constexpr uint32_t ST_EVIDENCE = 8;
constexpr int MAX_K = 8;                                // MCX_EVIDENCE_MAX_K
constexpr int F_NOT_CONVERGED = 1, F_NO_ESS = 2;        // MCX_EVIDENCE_*
constexpr int OK = 0, ERR_INVALID = 1, ERR_UNSUPPORTED = 4;  // MCX_OK, MCX_ERR_INVALID, MCX_ERR_UNSUPPORTED
constexpr long long NMAX = 1ll << 31;
constexpr long long NDRAW_DEFAULT_MAX = 1ll << 20;
constexpr int MAX_ITER_DEFAULT = 1000;
constexpr double LOG_2PI = 1.8378770664093454835606594728112;

// Philox4x32-10 as mcx_numerics.hpp has it, restated without HIP: words x and y of the block
inline void philox_xy(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t *x, uint32_t *y)
{
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * (uint64_t)c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * (uint64_t)c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  *x = c0;
  *y = c1;
}

// the uniform of words x : y of a block: their top 53 bits, in [0, 1)
MCX_EV_HD double uniform53(uint32_t x, uint32_t y)
{
  const uint64_t r = ((uint64_t)x << 32) | (uint64_t)y;
  return (double)(r >> 11) * 0x1p-53;
}
// the uniform that picks the component of draw j: block (j, 0, 1, 0) under key (seed, ST_EVIDENCE)
inline double draw_uniform(uint32_t seed, uint32_t j)
{
  uint32_t x, y;
  philox_xy(j, 0u, 1u, 0u, seed, ST_EVIDENCE, &x, &y);
  return uniform53(x, y);
}
// the smallest k whose cumulative weight cum[k] exceeds u * cum[K - 1] (the last component if none does)
MCX_EV_HD int pick_component(double u, const double *cum, int K)
{
  const double target = u * cum[K - 1];
  for (int k = 0; k < K - 1; ++k)
    if (cum[k] > target) return k;
  return K - 1;
}

// what mcx_evidence_proposal refuses
inline int mixture_check(int np, int k, const double *weights, const double *centres, const double *covs, double scale, char *msg, size_t len)
{
  if (np < 1 || np > 256) {
    snprintf(msg, len, "np = %d: 1 to 256 parameters", np);
    return ERR_INVALID;
  }
  if (k < 1 || k > MAX_K) {
    snprintf(msg, len, "k = %d: 1 to %d components", k, MAX_K);
    return ERR_INVALID;
  }
  if (!weights || !centres || !covs) {
    snprintf(msg, len, "the proposal's weights, centres or covs is NULL");
    return ERR_INVALID;
  }
  if (!(scale > 0.0) || !std::isfinite(scale)) {
    snprintf(msg, len, "scale = %g: finite and positive", scale);
    return ERR_INVALID;
  }
  for (int c = 0; c < k; ++c) {
    if (!(weights[c] > 0.0) || !std::isfinite(weights[c])) {
      snprintf(msg, len, "weights[%d] = %g: finite and positive", c, weights[c]);
      return ERR_INVALID;
    }
    for (int i = 0; i < np; ++i)
      if (!std::isfinite(centres[(size_t)c * np + i])) {
        snprintf(msg, len, "centres[%d][%d] is not finite", c, i);
        return ERR_INVALID;
      }
  }
  return OK;
}

// One component: C = the lower Cholesky factor of scale^2 cov (row-major [np][np], the strict upper triangle zero), W = C^-1
// (lower, likewise), *sumlog = sum log diag C.  Returns 0, or 1 + the index of the pivot that is not positive and finite
// (*pivot = its value)
inline int factor_component(int np, const double *cov, double scale, double *Cf, double *W, double *sumlog, double *pivot)
{
  const double s2 = scale * scale;
  double sl = 0.0;
  for (int i = 0; i < np; ++i) {
    for (int j = 0; j <= i; ++j) {
      double s = s2 * cov[(size_t)i * np + j];
      for (int l = 0; l < j; ++l) s -= Cf[(size_t)i * np + l] * Cf[(size_t)j * np + l];
      if (i == j) {
        if (!(s > 0.0) || !std::isfinite(s)) {
          *pivot = s;
          return i + 1;
        }
        Cf[(size_t)i * np + i] = std::sqrt(s);
        sl += std::log(Cf[(size_t)i * np + i]);
      } else {
        Cf[(size_t)i * np + j] = s / Cf[(size_t)j * np + j];
      }
    }
    for (int j = i + 1; j < np; ++j) Cf[(size_t)i * np + j] = 0.0;
  }
  // W = C^-1 by forward substitution, column by column
  for (int j = 0; j < np; ++j) {
    for (int i = 0; i < j; ++i) W[(size_t)i * np + j] = 0.0;
    W[(size_t)j * np + j] = 1.0 / Cf[(size_t)j * np + j];
    for (int i = j + 1; i < np; ++i) {
      double s = 0.0;
      for (int l = j; l < i; ++l) s -= Cf[(size_t)i * np + l] * W[(size_t)l * np + j];
      W[(size_t)i * np + j] = s / Cf[(size_t)i * np + i];
    }
  }
  *sumlog = sl;
  return 0;
}

// the whole proposal: Cf[k][np][np], W[k][np][np], lc[k] = log(w_k / sum w) - sum log diag C_k - (np / 2) log 2 pi
inline int proposal(int np, int k, const double *weights, const double *centres, const double *covs, double scale, double *Cf, double *W,
                    double *lc, char *msg, size_t len)
{
  const int rc = mixture_check(np, k, weights, centres, covs, scale, msg, len);
  if (rc != OK) return rc;
  double sw = 0.0;
  for (int c = 0; c < k; ++c) sw += weights[c];
  for (int c = 0; c < k; ++c) {
    double sl = 0.0, piv = 0.0;
    const size_t o = (size_t)c * np * np;
    const int bad = factor_component(np, covs + o, scale, Cf + o, W + o, &sl, &piv);
    if (bad) {
      snprintf(msg, len, "the covariance of component %d is not positive definite: pivot %d = %g is not positive and finite", c, bad - 1,
               piv);
      return ERR_INVALID;
    }
    lc[c] = std::log(weights[c] / sw) - sl - 0.5 * (double)np * LOG_2PI;
  }
  return OK;
}

// log g of one float row by the definition: u = (double)x - c_k, z = W_k u, Q_k = sum z_i^2, t_k = lc_k - Q_k / 2, the
// log-sum-exp over the components.  (The device sums in another order; tests hold it to the forward bound.)
inline double logg_row(int np, int k, const double *centres, const double *W, const double *lc, const float *x)
{
  for (int i = 0; i < np; ++i)
    if (!std::isfinite(x[i])) return std::numeric_limits<double>::quiet_NaN();
  double t[MAX_K], mx = -std::numeric_limits<double>::infinity();
  for (int c = 0; c < k; ++c) {
    const double *Wc = W + (size_t)c * np * np, *cc = centres + (size_t)c * np;
    double Q = 0.0;
    for (int i = 0; i < np; ++i) {
      double z = 0.0;
      for (int l = 0; l <= i; ++l) z += Wc[(size_t)i * np + l] * ((double)x[l] - cc[l]);
      Q += z * z;
    }
    t[c] = lc[c] - 0.5 * Q;
    if (t[c] > mx) mx = t[c];
  }
  double s = 0.0;
  for (int c = 0; c < k; ++c) s += std::exp(t[c] - mx);
  return mx + std::log(s);
}

// ---- the terms.  a = l - l*, r the current estimate; each in the branch that cannot overflow.  l = -inf (a draw with L = 0)
// gives a numerator term of 0
MCX_EV_HD double term_num(double a, double r, double s1, double s2)
{
  if (a >= 0.0) return 1.0 / (s1 + s2 * r * exp(-a));
  const double ea = exp(a);
  return ea / (s1 * ea + s2 * r);
}
MCX_EV_HD double term_den(double a, double r, double s1, double s2)
{
  if (a >= 0.0) {
    const double ema = exp(-a);
    return ema / (s1 + s2 * r * ema);
  }
  return 1.0 / (s1 * exp(a) + s2 * r);
}
// the error's f1 (draws) and f2 (rows) with d = l - log Z: p = e^d, f1 = p / (s1 p + s2), f2 = 1 / (s1 p + s2), each in the
// branch that cannot overflow
MCX_EV_HD double term_f1(double d, double s1, double s2)
{
  if (d >= 0.0) return 1.0 / (s1 + s2 * exp(-d));
  const double p = exp(d);
  return p / (s1 * p + s2);
}
MCX_EV_HD double term_f2(double d, double s1, double s2)
{
  if (d >= 0.0) {
    const double q = exp(-d);
    return q / (s1 + s2 * q);
  }
  return 1.0 / (s1 * exp(d) + s2);
}

// ---- the loop's host side
struct Bridge {
  long long n1 = 0, n2 = 0;
  double neff = 0.0, s1 = 0.0, s2 = 0.0, lstar = 0.0;
  double tol = 1e-10;
  int max_iter = MAX_ITER_DEFAULT;
  double r = 1.0, logr = 0.0;
  int iters = 0, flags = 0;
  void begin(long long n1_, long long n2_, double neff_, double lstar_, double tol_, int max_iter_)
  {
    n1 = n1_; n2 = n2_; neff = neff_; lstar = lstar_; tol = tol_;
    max_iter = max_iter_ > 0 ? max_iter_ : MAX_ITER_DEFAULT;
    s1 = neff / (neff + (double)n2);
    s2 = 1.0 - s1;  // N2 / (neff + N2), formed so that s1 + s2 is 1 in floating point: equal l give terms of exactly 1
    r = 1.0; logr = 0.0; iters = 0; flags = 0;
  }
  // one pass's sums in: true when the loop is over
  bool update(double sum_num, double sum_den)
  {
    const double rn = (sum_num / (double)n2) / (sum_den / (double)n1), ln = std::log(rn);
    const double delta = std::fabs(ln - logr);
    r = rn;
    logr = ln;
    ++iters;
    if (delta <= tol) return true;
    if (!(delta == delta)) return true;  // (a NaN cannot improve)
    if (iters >= max_iter) {
      flags |= F_NOT_CONVERGED;
      return true;
    }
    return false;
  }
  double log_z() const { return logr + lstar; }
};

// the error from the sums of f1 over the draws and f2 over the rows and, in a second pass about their means m = sum / n, the sums
// of (f - m)^2 (variances with divisor n - 1; 0 for n = 1)
inline void finish_error(double sf1, double cf1, long long n2, double sf2, double cf2, long long n1, double ess_f2, double *re2_draws,
                         double *re2_rows, double *se)
{
  auto half = [](double s, double c, long long n, double ess) {
    const double m = s / (double)n, var = n > 1 ? c / (double)(n - 1) : 0.0;
    return var / (m * m * ess);
  };
  *re2_draws = half(sf1, cf1, n2, (double)n2);
  *re2_rows = half(sf2, cf2, n1, ess_f2);
  *se = std::sqrt(*re2_draws + *re2_rows);
}
// the by-products from their max-shifted sums: sis = sum e^(l2 - m2) over the draws, sris = sum e^(-(l1) - m1) over the rows
inline double finish_is(double m2, double sis, long long n2) { return m2 + std::log(sis / (double)n2); }
inline double finish_ris(double m1, double sris, long long n1) { return -(m1 + std::log(sris / (double)n1)); }

// the lower median of v[n] (sorted in place); NaN when any value is
inline double lower_median(std::vector<double> &v)
{
  for (double x : v)
    if (!(x == x)) return std::numeric_limits<double>::quiet_NaN();
  for (size_t i = 1; i < v.size(); ++i)  // (insertion sort: at most 256 values)
    for (size_t j = i; j > 0 && v[j] < v[j - 1]; --j) {
      const double t = v[j];
      v[j] = v[j - 1];
      v[j - 1] = t;
    }
  return v[(v.size() - 1) / 2];
}

struct IterateResult {
  double lstar, log_z, se, re2_draws, re2_rows, log_z_is, log_z_ris;
  long long ndraw_zero;
  int iters, flags;
};

// mcx_evidence_iterate: the whole estimator on host arrays.  ess_f2 is the caller's (the host has no spectral estimate).
// Returns ERR_INVALID with a message for a non-finite l1, an l2 of +inf or NaN, or draws that all have L = 0
inline int iterate(const double *l1, long long n1, const double *l2, long long n2, double neff, double ess_f2, double tol, int max_iter,
                   IterateResult *o, char *msg, size_t len)
{
  const double ninf = -std::numeric_limits<double>::infinity();
  double sl = 0.0, m1 = ninf, m2 = ninf;
  for (long long i = 0; i < n1; ++i) {
    if (!std::isfinite(l1[i])) {
      snprintf(msg, len, "l1 of row %lld is not finite (the lowest such row)", i);
      return ERR_INVALID;
    }
    sl += l1[i];
    if (-l1[i] > m1) m1 = -l1[i];
  }
  long long nz = 0;
  for (long long j = 0; j < n2; ++j) {
    if (l2[j] == ninf) {
      ++nz;
      continue;
    }
    if (!std::isfinite(l2[j])) {
      snprintf(msg, len, "l2 of draw %lld is +inf or NaN (the lowest such draw)", j);
      return ERR_INVALID;
    }
    if (l2[j] > m2) m2 = l2[j];
  }
  if (nz == n2) {
    snprintf(msg, len, "every one of the %lld draws has L = 0: the proposal misses the sampled function", n2);
    return ERR_INVALID;
  }
  Bridge b;
  b.begin(n1, n2, neff, sl / (double)n1, tol, max_iter);
  for (;;) {
    double sn = 0.0, sd = 0.0;
    for (long long j = 0; j < n2; ++j) sn += term_num(l2[j] - b.lstar, b.r, b.s1, b.s2);
    for (long long i = 0; i < n1; ++i) sd += term_den(l1[i] - b.lstar, b.r, b.s1, b.s2);
    if (b.update(sn, sd)) break;
  }
  const double lz = b.log_z();
  double f1 = 0.0, f2 = 0.0, c1 = 0.0, c2 = 0.0, sis = 0.0, sris = 0.0;
  for (long long j = 0; j < n2; ++j) {
    f1 += term_f1(l2[j] - lz, b.s1, b.s2);
    sis += std::exp(l2[j] - m2);
  }
  for (long long i = 0; i < n1; ++i) {
    f2 += term_f2(l1[i] - lz, b.s1, b.s2);
    sris += std::exp(-l1[i] - m1);
  }
  const double mf1 = f1 / (double)n2, mf2 = f2 / (double)n1;
  for (long long j = 0; j < n2; ++j) {
    const double d = term_f1(l2[j] - lz, b.s1, b.s2) - mf1;
    c1 += d * d;
  }
  for (long long i = 0; i < n1; ++i) {
    const double d = term_f2(l1[i] - lz, b.s1, b.s2) - mf2;
    c2 += d * d;
  }
  o->lstar = b.lstar;
  o->log_z = lz;
  finish_error(f1, c1, n2, f2, c2, n1, ess_f2, &o->re2_draws, &o->re2_rows, &o->se);
  o->log_z_is = finish_is(m2, sis, n2);
  o->log_z_ris = finish_ris(m1, sris, n1);
  o->ndraw_zero = nz;
  o->iters = b.iters;
  o->flags = b.flags;
  return OK;
}

}  // namespace mcx_evidence_host
