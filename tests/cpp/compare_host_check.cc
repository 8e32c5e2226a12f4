// The host half of the two-store comparison (mcpar_amd/csrc/mcx_compare_host.hpp) as a stand-alone program: built with
// -fsanitize=address,undefined by tests/test_compare_cpu.py.  It needs no HIP and no library.
#include "mcpar_amd/csrc/mcx_compare_host.hpp"

#include <cstdio>

namespace H = mcx_compare_host;

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
  const double nan = std::numeric_limits<double>::quiet_NaN();
  EXPECT(H::kolmogorov_q(0.0) == 1.0 && H::kolmogorov_q(-1.0) == 1.0 && H::kolmogorov_q(0.05) == 1.0);
  EXPECT(H::kolmogorov_q(50.0) == 0.0 && H::kolmogorov_q(1e300) == 0.0);
  EXPECT(H::kolmogorov_q(nan) != H::kolmogorov_q(nan));
  // Q(1.36) = 0.0495 (the 5 % point of the two-sample test), and the two forms meet at the switch
  EXPECT(std::fabs(H::kolmogorov_q(1.36) - 0.04948) < 1e-4);
  EXPECT(std::fabs(H::kolmogorov_q(1.18) - H::kolmogorov_q(std::nextafter(1.18, 0.0))) < 1e-14);
  double last = 1.0;
  for (int i = 0; i <= 4000; ++i) {
    const double q = H::kolmogorov_q(i * 0.002);
    EXPECT(q >= 0.0 && q <= 1.0 && q <= last + 1e-15);
    last = q;
  }
  double ne = 0.0, p = 0.0;
  H::ks_prob(0.0, 8.0, 8.0, &ne, &p);
  EXPECT(ne == 4.0 && p == 1.0);
  H::ks_prob(1.0, 1e4, 1e4, &ne, &p);
  EXPECT(ne == 5e3 && p == 0.0);
  H::ks_prob(0.3, nan, 10.0, &ne, &p);
  EXPECT(ne != ne && p != p);
  EXPECT(H::z_mean(1.0, 2.0, 4.0, 0.0, 2.0, 4.0) == 1.0 / std::sqrt(2.0));
  EXPECT(H::z_mean(1.0, 0.0, 4.0, 1.0, 0.0, 4.0) != H::z_mean(1.0, 0.0, 4.0, 1.0, 0.0, 4.0));  // 0 / 0
  if (fails == 0) std::printf("compare_host_check ok\n");
  return fails ? 1 : 0;
}
