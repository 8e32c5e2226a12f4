// mcx_intervals_host.hpp -- the host half of mcx_*_intervals: the quantile of a beta law (the inverse of
// the regularised incomplete beta function, fp64), the two ranks around a quantile that its Monte-Carlo error is read from, and
// the error of a standard deviation.  No HIP and no library state: tests/cpp/intervals_host_check.cc compiles it alone.
//
// I_x(a, b) is Lentz's evaluation of the continued fraction (Numerical Recipes' betacf) times x^a (1 - x)^b / (a B(a, b)).  That
// factor is where a plain lgamma loses everything for large a and b (lgamma(2^31) is 4.6e10: its last bit is 8e-6), so it is
// formed as Loader's saddle-point expansion of a binomial density ("Fast and accurate computation of binomial probabilities",
// 2000; R's dbinom_raw): the Stirling errors and the deviances bd0 are each O(1) near the quantile.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>

namespace mcx_intervals_host {

constexpr double P_LO = 0.1586553, P_HI = 0.8413447;  // the normal law's mass below -1 and below +1, as posterior writes them
constexpr double LN_SQRT_2PI = 0.918938533204672741780329736406;
constexpr double TWO_PI = 6.283185307179586476925286766559;

// lgamma(n + 1) - ((n + 1/2) log n - n + log sqrt(2 pi)), n > 0
inline double stirlerr(double n)
{
  constexpr double S0 = 1.0 / 12.0, S1 = 1.0 / 360.0, S2 = 1.0 / 1260.0, S3 = 1.0 / 1680.0, S4 = 1.0 / 1188.0;
  if (n <= 15.0) return std::lgamma(n + 1.0) - (n + 0.5) * std::log(n) + n - LN_SQRT_2PI;
  const double nn = n * n;
  if (n > 500.0) return (S0 - S1 / nn) / n;
  if (n > 80.0) return (S0 - (S1 - S2 / nn) / nn) / n;
  if (n > 35.0) return (S0 - (S1 - (S2 - S3 / nn) / nn) / nn) / n;
  return (S0 - (S1 - (S2 - (S3 - S4 / nn) / nn) / nn) / nn) / n;
}

// x log(x / m) + m - x, x > 0, m > 0, without the cancellation where x is close to m
inline double bd0(double x, double m)
{
  if (std::fabs(x - m) < 0.1 * (x + m)) {
    double v = (x - m) / (x + m), s = (x - m) * v;
    if (std::fabs(s) < std::numeric_limits<double>::min()) return s;
    double ej = 2.0 * x * v;
    v *= v;
    for (int j = 1; j < 1000; ++j) {
      ej *= v;
      const double s1 = s + ej / (double)(2 * j + 1);
      if (s1 == s) return s1;
      s = s1;
    }
  }
  return x * std::log(x / m) + m - x;
}

// log of C(n, x) p^x (1 - p)^(n - x) for real 0 <= x <= n, 0 < p < 1
inline double log_binomial(double x, double n, double p)
{
  if (x <= 0.0) return n * std::log1p(-p);
  if (x >= n) return n * std::log(p);
  const double q = 1.0 - p;
  return stirlerr(n) - stirlerr(x) - stirlerr(n - x) - bd0(x, n * p) - bd0(n - x, n * q) + 0.5 * std::log(n / (TWO_PI * x * (n - x)));
}

// log of x^a (1 - x)^b / B(a, b), a >= 1, b >= 1, 0 < x < 1: x (1 - x) (a + b - 1) times the binomial density above
inline double log_beta_front(double x, double a, double b)
{
  return std::log(x) + std::log1p(-x) + std::log(a + b - 1.0) + log_binomial(a - 1.0, a + b - 2.0, x);
}

// the continued fraction of I_x(a, b), for x < (a + 1) / (a + b + 2): it needs some sqrt(max(a, b)) terms
inline double beta_cf(double x, double a, double b)
{
  constexpr double TINY = 1e-300, EPS = 1e-16;
  const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
  double c = 1.0, d = 1.0 - qab * x / qap;
  if (std::fabs(d) < TINY) d = TINY;
  d = 1.0 / d;
  double h = d;
  for (int m = 1; m <= 4000000; ++m) {
    const double dm = (double)m, m2 = 2.0 * dm;
    double aa = dm * (b - dm) * x / ((qam + m2) * (a + m2));
    d = 1.0 + aa * d;
    if (std::fabs(d) < TINY) d = TINY;
    c = 1.0 + aa / c;
    if (std::fabs(c) < TINY) c = TINY;
    d = 1.0 / d;
    h *= d * c;
    aa = -(a + dm) * (qab + dm) * x / ((a + m2) * (qap + m2));
    d = 1.0 + aa * d;
    if (std::fabs(d) < TINY) d = TINY;
    c = 1.0 + aa / c;
    if (std::fabs(c) < TINY) c = TINY;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (std::fabs(del - 1.0) <= EPS) break;
  }
  return h;
}

// I_x(a, b), a >= 1, b >= 1
inline double beta_cdf(double x, double a, double b)
{
  if (!(x > 0.0)) return 0.0;
  if (!(x < 1.0)) return 1.0;
  if (x < (a + 1.0) / (a + b + 2.0)) return std::exp(log_beta_front(x, a, b)) * beta_cf(x, a, b) / a;
  return 1.0 - std::exp(log_beta_front(x, a, b)) * beta_cf(1.0 - x, b, a) / b;
}

// the x with I_x(a, b) = p: Newton's steps from the mean, kept inside a bracket that every evaluation narrows (a step that leaves
// it is replaced by the bracket's middle).  NaN unless 0 <= p <= 1, a >= 1, b >= 1 and both finite
inline double beta_quantile(double p, double a, double b)
{
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  if (!(p >= 0.0 && p <= 1.0) || !(a >= 1.0) || !(b >= 1.0) || !std::isfinite(a) || !std::isfinite(b)) return qnan;
  if (p == 0.0) return 0.0;
  if (p == 1.0) return 1.0;
  double lo = 0.0, hi = 1.0, x = a / (a + b);
  for (int it = 0; it < 200; ++it) {
    const double f = beta_cdf(x, a, b) - p;
    if (f == 0.0) return x;
    if (f < 0.0) lo = x; else hi = x;
    const double dens = std::exp(log_beta_front(x, a, b)) / (x * (1.0 - x));
    double nx = x - f / dens;
    if (!(nx > lo && nx < hi)) nx = 0.5 * (lo + hi);
    const double step = std::fabs(nx - x);
    x = nx;
    if (step <= 2.0 * std::numeric_limits<double>::epsilon() * x || !(hi > lo)) break;
  }
  return x;
}

// The ranks around the quantile of probability prob of N sorted values whose indicator has the effective size ess (posterior's
// mcse_quantile): u_lo, u_hi are the beta(ess prob + 1, ess (1 - prob) + 1) quantiles of P_LO and P_HI, k_lo = max(floor(u_lo N),
// 1) - 1, k_hi = min(ceil(u_hi N), N) - 1, both in [0, N - 1].  An ess that is not a positive finite number gives NaN and -1
inline void quantile_ranks(int64_t N, double prob, double ess, double *u_lo, double *u_hi, int64_t *k_lo, int64_t *k_hi)
{
  *u_lo = *u_hi = std::numeric_limits<double>::quiet_NaN();
  *k_lo = *k_hi = -1;
  if (!(ess > 0.0) || !std::isfinite(ess) || N < 1) return;
  const double a = ess * prob + 1.0, b = ess * (1.0 - prob) + 1.0;
  *u_lo = beta_quantile(P_LO, a, b);
  *u_hi = beta_quantile(P_HI, a, b);
  if (*u_lo != *u_lo || *u_hi != *u_hi) return;
  const double nd = (double)N;
  *k_lo = std::min<int64_t>(std::max<int64_t>((int64_t)std::floor(*u_lo * nd), 1), N) - 1;
  *k_hi = std::max<int64_t>(std::min<int64_t>((int64_t)std::ceil(*u_hi * nd), N), 1) - 1;
}

// the span of a highest-density interval of mass p over N sorted values: floor(p N), and N - 1 at most (one window at least)
inline int64_t hdi_span(double p, int64_t N) { return std::min<int64_t>((int64_t)std::floor(p * (double)N), N - 1); }

// the Monte-Carlo error of a standard deviation from the mean, sd and effective size of the squared deviations c2 (posterior's
// mcse_sd: Kenney and Keeping's variance of a variance with the effective size in place of N)
inline double mcse_sd(int64_t N, double mean_c2, double sd_c2, double ess_c2)
{
  const double nd = (double)N;
  return std::sqrt((nd - 1.0) / nd * (sd_c2 * sd_c2) / ess_c2 / mean_c2 / 4.0);
}

}  // namespace mcx_intervals_host
