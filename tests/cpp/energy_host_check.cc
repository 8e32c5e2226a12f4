// The host half of the joint two-store comparison (mcpar_amd/csrc/mcx_energy_host.hpp: the label rule and the finish) as a
// stand-alone program: built with -fsanitize=address,undefined by tests/test_energy_cpu.py.  It needs no HIP and no library.
#include "mcpar_amd/csrc/mcx_energy_host.hpp"

#include <cstdio>

namespace H = mcx_energy_host;

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
  // Philox4x32-10, the known answer for counter and key of zeros (Random123 kat_vectors)
  uint32_t x = 0, y = 0;
  H::philox_xy(0u, 0u, 0u, 0u, 0u, 0u, &x, &y);
  EXPECT(x == 0x6627e8d5u && y == 0xe169c58du);
  EXPECT(H::mulhi_64x32(~0ull, 7) == 6 && H::mulhi_64x32(0, 7) == 0 && H::mulhi_64x32(1ull << 63, 0xffffffffull) == 0x7fffffffull);
  // the label rule: n_a ones, p = 0 the identity, every size at its edges
  std::vector<uint32_t> idx;
  const int sizes[][2] = {{1, 1}, {2, 2}, {15, 2}, {2, 15}, {63, 66}, {1, 300}, {300, 1}};
  for (const auto &s : sizes) {
    std::vector<uint8_t> l((size_t)(s[0] + s[1]));  // (exactly N bytes: a write past them is the sanitizer's to find)
    for (int p = 0; p < 40; ++p) {
      H::labels(12345u + (uint32_t)p, s[0], s[1], p, l.data(), idx);
      int ones = 0;
      for (uint8_t b : l) {
        EXPECT(b <= 1);
        ones += b;
      }
      EXPECT(ones == s[0]);
      if (p == 0)
        for (size_t i = 0; i < l.size(); ++i) EXPECT(l[i] == (i < (size_t)s[0] ? 1 : 0));
    }
  }
  // N = 4, n_a = 2: all six labelings turn up
  bool seen[16] = {};
  std::vector<uint8_t> l4(4);
  for (int p = 1; p <= 200; ++p) {
    H::labels(0u, 2, 2, p, l4.data(), idx);
    seen[l4[0] | l4[1] << 1 | l4[2] << 2 | l4[3] << 3] = true;
  }
  int nseen = 0;
  for (bool b : seen) nseen += b;
  EXPECT(nseen == 6);
  // the finish on made-up sums: A = {0, 1}, B = {3} on a line: S = 2 (1 + 3 + 2) = 12, S_A = 4 + 3 = 7, S_AA = 2
  const double sums[] = {12.0, 7.0, 2.0, /* l_1 = (1, 0, 1) */ 4.0 + 5.0, 6.0, /* l_2 = l_0 */ 7.0, 2.0};
  double pe[2] = {0.0, 0.0};
  const H::Finish f = H::finish(sums, 2, 1, 2, pe);
  EXPECT(f.mean_ab == 2.5 && f.mean_aa == 0.5 && f.mean_bb == 0.0 && f.e == 4.5 && f.h == 0.9);
  EXPECT(pe[0] == 2.0 * 3.0 / 2.0 - 6.0 / 4.0 - 0.0 && pe[1] == f.e && f.nge == 1 && f.p_value == 2.0 / 3.0);
  const H::Finish f0 = H::finish(sums, 2, 1, 0, nullptr);
  EXPECT(f0.e == 4.5 && f0.nge == 0 && f0.p_value != f0.p_value);
  const H::Finish fn = H::finish(nullptr, 2, 1, 2, pe);
  EXPECT(fn.e != fn.e && fn.h != fn.h && fn.p_value != fn.p_value && fn.nge == 0 && pe[0] != pe[0] && pe[1] != pe[1]);
  const double zero[] = {0.0, 0.0, 0.0};
  const H::Finish fz = H::finish(zero, 2, 2, 0, nullptr);
  EXPECT(fz.e == 0.0 && fz.h != fz.h);
  // the scale: two-pass, divisor N - 1; a value that is not finite is reported
  const float col[] = {1.0f, 9.0f, 2.0f, 9.0f, 3.0f, 9.0f, 6.0f, 9.0f};
  bool finite = false;
  EXPECT(H::column_scale(col, 4, 2, &finite) == std::sqrt(14.0 / 3.0) && finite);
  EXPECT(H::column_scale(col + 1, 4, 2, &finite) == 0.0 && finite);
  const float bad[] = {1.0f, std::numeric_limits<float>::infinity(), 2.0f};
  const double sb = H::column_scale(bad, 3, 1, &finite);
  EXPECT(sb != sb && !finite);
  if (fails == 0) std::printf("energy_host_check ok\n");
  return fails ? 1 : 0;
}
