// The host half of the importance weights (mcpar_amd/csrc/mcx_reweight_host.hpp: k-hat, the quantile threshold and the finish) as
// a stand-alone program: built with -fsanitize=address,undefined by tests/test_reweight_cpu.py.  It needs no HIP and no library.
#include "mcpar_amd/csrc/mcx_reweight_host.hpp"

#include <cstdio>

namespace H = mcx_reweight_host;

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
  double k = 0.0, s = 0.0;
  int f = 0;
  // every tail length from none to a few hundred, exactly n doubles each (a read past them is the sanitizer's to find): the
  // exceedances of a Pareto law with shape 1/2 at the plotting positions
  for (int n = 0; n <= 400; n += (n < 12 ? 1 : 97)) {
    std::vector<double> x((size_t)n);
    for (int i = 0; i < n; ++i) x[(size_t)i] = 2.0 * (std::pow(1.0 - (i + 0.5) / n, -0.5) - 1.0);
    H::khat_of_tail(x.data(), n, &k, &s, &f);
    if (n < 5) EXPECT(f == H::NO_TAIL && std::isnan(k) && std::isnan(s));
    else EXPECT(!(f & H::NO_TAIL) && std::isfinite(k) && s > 0.0);
    if (n >= 100) EXPECT(std::fabs(k - 0.5) < 0.15);
  }
  const double zeros[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ties[8] = {0, 0, 0, 0.5, 0.6, 0.7, 0.8, 0.9};
  H::khat_of_tail(zeros, 8, &k, &s, &f);
  EXPECT(f == H::NO_TAIL && std::isnan(k));
  H::khat_of_tail(ties, 8, &k, &s, &f);  // xstar = x[floor(2.5) - 1] = x[1] = 0
  EXPECT(f == H::NO_TAIL && std::isnan(s));
  // the tail length and the thresholds at their edges
  EXPECT(H::tail_length(1) == 0 && H::tail_length(24) == 4 && H::tail_length(25) == 5 && H::tail_length(225) == 45 &&
         H::tail_length(226) == 45 && H::tail_length(40000) == 600 && H::tail_length(2147483647) == 139023);
  const int64_t Q = (int64_t)1 << 61;
  EXPECT(H::quantile_threshold(0.0, 10) == 1 && H::quantile_threshold(1.0, 10) == 10 && H::quantile_threshold(0.25, 10) == 3 &&
         H::quantile_threshold(1e-30, 10) == 1 && H::quantile_threshold(1.0, Q) == Q && H::quantile_threshold(0.5, Q) == Q / 2 &&
         H::quantile_threshold(1.0, INT64_MAX) == INT64_MAX);
  // 444 rows of full weight: Q = 444 2^31, Q2 = 444 2^62 carries into the high word
  const uint64_t hi = 444 >> 2, lo = (uint64_t)(444 & 3) << 62;
  EXPECT(H::ess_kish((int64_t)444 << 31, hi, lo) == 444.0);
  EXPECT(H::log_mean_w(1.5, (int64_t)444 << 31, 444) == 1.5);
  EXPECT(H::ess_kish((int64_t)1 << 31, 0, (uint64_t)1 << 62) == 1.0);
  std::printf(fails ? "%d checks failed\n" : "reweight host checks ok\n", fails);
  return fails ? 1 : 0;
}
