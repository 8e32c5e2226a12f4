// The host half of the interval estimates (mcpar_amd/csrc/mcx_intervals_host.hpp: the beta quantile, the ranks around a quantile,
// the span of an HDI and the error of a standard deviation) as a stand-alone program: built with -fsanitize=address,undefined by
// tests/test_intervals_cpu.py.  It needs no HIP and no library.
#include "mcpar_amd/csrc/mcx_intervals_host.hpp"

#include <cstdio>

namespace H = mcx_intervals_host;

static int fails = 0;
#define EXPECT(c)                                                \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("line %d: %s\n", __LINE__, #c);                \
      ++fails;                                                   \
    }                                                            \
  } while (0)

int main()
{
  // closed forms: the uniform law, beta(1, b) and beta(a, 1), the symmetric median
  EXPECT(std::fabs(H::beta_quantile(0.3, 1.0, 1.0) - 0.3) < 1e-15);
  for (double b : {1.0, 2.5, 100.0, 65536.0, 2147483649.0}) {
    for (double p : {H::P_LO, 0.5, H::P_HI}) {
      const double x = -std::expm1(std::log1p(-p) / b);  // 1 - (1 - p)^(1 / b)
      EXPECT(std::fabs(H::beta_quantile(p, 1.0, b) - x) <= 1e-12 * x);
      EXPECT(std::fabs(H::beta_quantile(p, b, 1.0) - std::pow(p, 1.0 / b)) <= 1e-12);
    }
    EXPECT(std::fabs(H::beta_quantile(0.5, b, b) - 0.5) * 2.0 * b <= 1e-6);
  }
  // the round trip through the distribution function, and its monotony in p
  for (double a : {1.0, 3.7, 412.5, 1048576.5})
    for (double b : {1.5, 57.0, 30000.25}) {
      const double lo = H::beta_quantile(H::P_LO, a, b), hi = H::beta_quantile(H::P_HI, a, b);
      EXPECT(0.0 < lo && lo < hi && hi < 1.0);
      EXPECT(std::fabs(H::beta_cdf(lo, a, b) - H::P_LO) < 1e-9 && std::fabs(H::beta_cdf(hi, a, b) - H::P_HI) < 1e-9);
    }
  EXPECT(H::beta_quantile(0.0, 2.0, 3.0) == 0.0 && H::beta_quantile(1.0, 2.0, 3.0) == 1.0);
  EXPECT(std::isnan(H::beta_quantile(0.5, 0.5, 2.0)) && std::isnan(H::beta_quantile(1.5, 2.0, 2.0)) &&
         std::isnan(H::beta_quantile(0.5, INFINITY, 2.0)) && std::isnan(H::beta_quantile(NAN, 2.0, 2.0)));
  // the ranks stay inside [0, N - 1] at every edge
  double ul = 0.0, uh = 0.0;
  int64_t kl = 0, kh = 0;
  for (int64_t N : {1, 2, 8, 888, 2147483647})
    for (double prob : {0.0, 0.05, 0.5, 1.0})
      for (double ess : {1e-3, 1.0, 31.0, 3793.0, 4e9}) {
        H::quantile_ranks(N, prob, ess, &ul, &uh, &kl, &kh);
        EXPECT(0 <= kl && kl <= kh && kh <= N - 1 && 0.0 <= ul && ul <= uh && uh <= 1.0);
      }
  H::quantile_ranks(888, 0.5, 100.0, &ul, &uh, &kl, &kh);
  EXPECT(kl == 399 && kh == 487);
  for (double ess : {0.0, -1.0, (double)NAN, (double)INFINITY}) {
    H::quantile_ranks(888, 0.5, ess, &ul, &uh, &kl, &kh);
    EXPECT(std::isnan(ul) && std::isnan(uh) && kl == -1 && kh == -1);
  }
  // spans: floor(p N), one window at least
  EXPECT(H::hdi_span(0.9, 10) == 9 && H::hdi_span(0.94, 888) == 834 && H::hdi_span(1e-12, 888) == 0 && H::hdi_span(0.5, 1) == 0 &&
         H::hdi_span(1.0 - 1e-16, 2147483647) == 2147483646);
  // the error of a sd: for iid normal draws sd / sqrt(2 N); c2 of a unit normal has mean 1 and sd sqrt(2)
  EXPECT(std::fabs(H::mcse_sd(1000000, 1.0, std::sqrt(2.0), 1e6) - 1.0 / std::sqrt(2e6)) < 1e-9);
  std::printf(fails ? "%d checks failed\n" : "intervals host checks ok\n", fails);
  return fails ? 1 : 0;
}
