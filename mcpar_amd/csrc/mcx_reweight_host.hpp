// mcx_reweight_host.hpp -- the host half of mcx_*_reweight: the Pareto tail index k-hat of the largest
// weights (Zhang and Stephens' estimator with the weak prior of Vehtari et al.), the threshold of a weighted quantile and the
// finish that turns the integer sums of the fixed-point weights into the reported numbers.  No HIP and no library state:
// tests/cpp/reweight_host_check.cc compiles it alone.  Every sum runs in index order.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

namespace mcx_reweight_host {

constexpr int NO_TAIL = 1, KHAT_HIGH = 2;  // include/mcx.h MCX_REWEIGHT_NO_TAIL, MCX_REWEIGHT_KHAT_HIGH
constexpr double TWO31 = 2147483648.0;

// the tail length of N weights: min(floor(N / 5), ceil(3 sqrt(N)))
inline int64_t tail_length(int64_t N) { return std::min<int64_t>(N / 5, (int64_t)std::ceil(3.0 * std::sqrt((double)N))); }

// x[0] <= ... <= x[n - 1], the exceedances of the tail over its cutoff -> khat, sigma and the flags
inline void khat_of_tail(const double *x, int64_t n, double *khat, double *sigma, int *flags)
{
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  *khat = *sigma = qnan;
  *flags = NO_TAIL;
  if (n < 5) return;
  const double xn = x[n - 1], xstar = x[(int64_t)std::floor((double)n / 4.0 + 0.5) - 1];
  if (!(xstar > 0.0) || !(xn > 0.0)) return;  // heavy ties at the cutoff, or constant weights
  const int m = 30 + (int)std::floor(std::sqrt((double)n));
  const double nd = (double)n;
  auto mean_log1p = [&](double theta) {
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) s += std::log1p(-theta * x[i]);
    return s / nd;
  };
  std::vector<double> th((size_t)m), l((size_t)m);
  for (int j = 1; j <= m; ++j) {
    const double t = 1.0 / xn + (1.0 - std::sqrt((double)m / ((double)j - 0.5))) / (3.0 * xstar);
    const double k = mean_log1p(t);
    th[j - 1] = t;
    l[j - 1] = nd * (std::log(-t / k) - k - 1.0);
  }
  double theta = 0.0;
  for (int j = 0; j < m; ++j) {
    double s = 0.0;
    for (int i = 0; i < m; ++i) s += std::exp(l[i] - l[j]);
    theta += th[j] * (1.0 / s);  // (a sum that overflowed to +inf: weight 0)
  }
  const double k = mean_log1p(theta);
  *sigma = -k / theta;
  *khat = (k * nd + 5.0) / (nd + 10.0);
  *flags = *khat > 0.7 ? KHAT_HIGH : 0;
}

// the cumulative weight a quantile of probability p must reach: min(Q, max(1, ceil(p Q))) in IEEE double
inline int64_t quantile_threshold(double p, int64_t Q)
{
  const double c = std::ceil(p * (double)Q);
  const int64_t t = c >= 9223372036854775807.0 ? Q : (int64_t)c;
  return std::min(Q, std::max<int64_t>(1, t));
}

// Kish's effective size Q^2 / Q2 from the integers, Q2 = hi 2^64 + lo
inline double ess_kish(int64_t Q, uint64_t q2_hi, uint64_t q2_lo)
{
  const long double q = (long double)Q, q2 = (long double)q2_hi * 18446744073709551616.0L + (long double)q2_lo;
  return (double)(q * q / q2);
}

// the log of the average weight: lwmax + log(Q / (2^31 N))
inline double log_mean_w(double lwmax, int64_t Q, int64_t N) { return lwmax + std::log((double)Q / (TWO31 * (double)N)); }

}  // namespace mcx_reweight_host
