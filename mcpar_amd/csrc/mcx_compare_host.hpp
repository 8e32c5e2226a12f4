// mcx_compare_host.hpp -- the host half of the two-store comparison: what turns the exact distances of
// the device into a statement about autocorrelated samples.  Plain C++ in fp64, no HIP and no library state: mcx_compare.hip
// calls these very functions (mcx_ks_prob is ks_prob()), and a host-only program can include this header alone.
#pragma once
#include <cmath>
#include <limits>

namespace mcx_compare_host {

// Q(lambda) = P(K > lambda), the survival function of Kolmogorov's distribution, clamped to [0, 1].  The alternating series
// 2 sum_{k >= 1} (-1)^(k-1) exp(-2 k^2 lambda^2) from lambda = 1.18 on; below it the theta-function form
// 1 - sqrt(2 pi) / lambda sum_{k >= 1} exp(-(2k - 1)^2 pi^2 / (8 lambda^2)), which converges fast where the other does not.
// Terms are added until one no longer changes the sum (at most 100 of them); NaN in, NaN out
inline double kolmogorov_q(double lam)
{
  if (lam != lam) return lam;
  if (lam <= 0.0) return 1.0;
  double q;
  if (lam >= 1.18) {
    double s = 0.0, sign = 1.0;
    for (int k = 1; k <= 100; ++k) {
      const double t = std::exp(-2.0 * (double)k * (double)k * lam * lam);
      const double s1 = s + sign * t;
      if (s1 == s) break;
      s = s1;
      sign = -sign;
    }
    q = 2.0 * s;
  } else {
    const double pi = 3.14159265358979323846;
    const double a = pi * pi / (8.0 * lam * lam);
    double s = 0.0;
    for (int k = 1; k <= 100; ++k) {
      const double m = (double)(2 * k - 1);
      const double s1 = s + std::exp(-m * m * a);
      if (s1 == s) break;
      s = s1;
    }
    q = 1.0 - std::sqrt(2.0 * pi) / lam * s;
  }
  return q < 0.0 ? 0.0 : q > 1.0 ? 1.0 : q;
}

// ks_neff = ess_a ess_b / (ess_a + ess_b); lambda = (sqrt(ne) + 0.12 + 0.11 / sqrt(ne)) ks (Stephens' correction);
// ks_p = Q(lambda).  A NaN among the arguments gives NaN in both
inline void ks_prob(double ks, double ess_a, double ess_b, double *neff, double *p)
{
  const double ne = ess_a * ess_b / (ess_a + ess_b);
  const double r = std::sqrt(ne);
  *neff = ne;
  *p = kolmogorov_q((r + 0.12 + 0.11 / r) * ks);
}

// z_mean = (mean_a - mean_b) / sqrt(sd_a^2 / ess_a + sd_b^2 / ess_b)
inline double z_mean(double mean_a, double sd_a, double ess_a, double mean_b, double sd_b, double ess_b)
{
  return (mean_a - mean_b) / std::sqrt(sd_a * sd_a / ess_a + sd_b * sd_b / ess_b);
}

}  // namespace mcx_compare_host
