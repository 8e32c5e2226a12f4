// The host half of the mutual information between columns (mcpar_amd/csrc/mcx_mutinfo_host.hpp: the row rule, the permutations,
// the table, the points and the finish) as a stand-alone program: built with -fsanitize=address,undefined by
// tests/test_mutinfo_cpu.py.  It needs no HIP and no library.
#include "mcpar_amd/csrc/mcx_mutinfo_host.hpp"

#include <cstdio>

namespace H = mcx_mutinfo_host;

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
  // the row rule at its ends
  EXPECT(H::row_index(10, 10, 9) == 9 && H::row_index(10, 3, 2) == 6 && H::row_index((1ll << 40) + 3, 16384, 16383) < (1ll << 40) + 3);
  // every pi_p is a permutation of exactly m entries (a write past them is the sanitizer's to find), p = 0 the identity
  for (int m : {1, 2, 3, 64, 1000}) {
    std::vector<uint16_t> pi((size_t)m);
    for (int p = 0; p < 20; ++p) {
      H::permutation(777u, m, p, pi.data());
      std::vector<int> seen((size_t)m, 0);
      for (uint16_t v : pi) {
        EXPECT((int)v < m);
        if ((int)v < m) ++seen[v];
      }
      for (int i = 0; i < m; ++i) EXPECT(seen[(size_t)i] == 1 && (p != 0 || pi[(size_t)i] == i));
    }
  }
  // m = 3: all six orders turn up
  bool orders[27] = {};
  int three[3];
  for (int p = 1; p <= 200; ++p) {
    H::permutation(0u, 3, p, three);
    orders[three[0] * 9 + three[1] * 3 + three[2]] = true;
  }
  int norders = 0;
  for (bool b : orders) norders += b;
  EXPECT(norders == 6);
  // the table: psi(1) = -gamma, psi(3) = 3/2 - gamma
  double t[5];
  H::psi_table(5, t);
  EXPECT(t[0] == -H::EULER_GAMMA && t[2] == 1.5 - H::EULER_GAMMA && t[4] == ((1.0 + 0.5) + 1.0 / 3.0 + 0.25) - H::EULER_GAMMA);
  // the points: 6 rows of 2 parameters and log L; row 3 repeats row 1 (-0 against +0), row 5 repeats row 0 but for log L
  const float rows[] = {1.0f, 2.0f, -1.0f, 0.0f, 4.0f, -2.0f, 3.0f, 6.0f, -3.0f, -0.0f, 4.0f, -2.0f, 5.0f, 8.0f, -5.0f, 1.0f, 2.0f, -9.0f};
  H::Points P;
  H::points(rows, 6, 3, false, false, P);
  EXPECT(P.ndup == 2 && P.m == 4 && P.nused == 2 && P.kept[3] == 0 && P.kept[5] == 0 && P.kept[4] == 1);
  EXPECT(P.flags[0] == 0 && P.flags[1] == 0 && P.flags[2] == H::COL_UNUSED && P.scale[2] != P.scale[2]);
  EXPECT(P.z.size() == 12 && P.z[0] == 1.0 / P.scale[0] && P.z[3] == 5.0 / P.scale[0] && P.z[4 + 2] == 6.0 / P.scale[1] && P.z[8] == 0.0);
  H::points(rows, 6, 3, true, true, P);
  EXPECT(P.ndup == 1 && P.m == 5 && P.nused == 3 && P.scale[2] == 1.0 && P.kept[5] == 1);
  const float flat[] = {1.0f, 7.0f, 0.0f, 2.0f, 7.0f, 0.0f, 3.0f, std::numeric_limits<float>::infinity(), 0.0f};
  H::points(flat, 3, 3, true, false, P);
  EXPECT(P.flags[0] == 0 && P.flags[1] == H::COL_NONFINITE && P.flags[2] == H::COL_CONSTANT && P.nused == 1 && P.m == 3);
  // the finish: four points on a line in both columns, k = 1: eps = 1, na = nb = 0 -> psi(1) + psi(4) - 2 psi(1)
  const double eps[] = {1.0, 1.0, 1.0, 0.0};
  const int na[] = {0, 0, 0, 0}, nb[] = {0, 0, 0, 0};
  double t4[4];
  H::psi_table(4, t4);
  long long nz = -1;
  const double mi = H::finish_pair(eps, na, nb, 4, 1, t4, &nz);
  EXPECT(nz == 1 && mi == (t4[0] + t4[3]) - (4.0 * (t4[0] + t4[0])) / 4.0);
  EXPECT(H::r_info(-0.3) == 0.0 && H::r_info(0.0) == 0.0 && H::r_info(50.0) == 1.0);
  const double a[] = {1.0, 2.0, 3.0, 4.0}, b[] = {2.0, 4.0, 6.0, 8.0}, c[] = {5.0, 5.0, 5.0, 5.0};
  EXPECT(H::pearson(a, b, 4) == 1.0 && H::pearson(a, c, 4) != H::pearson(a, c, 4));
  // the null: NaN without permutations, sd NaN with one
  const double pm[] = {0.1, 0.5, 0.3};
  H::Null n0 = H::null_of(0.3, pm, 0), n1 = H::null_of(0.3, pm, 1), n3 = H::null_of(0.3, pm, 3);
  EXPECT(n0.p_value != n0.p_value && n0.nge == 0 && n1.mean == 0.1 && n1.sd != n1.sd && n1.p_value == 0.5);
  EXPECT(n3.nge == 2 && n3.p_value == 0.75 && n3.sd == std::sqrt(((0.1 - n3.mean) * (0.1 - n3.mean) + (0.5 - n3.mean) * (0.5 - n3.mean) +
                                                                  (0.3 - n3.mean) * (0.3 - n3.mean)) / 2.0));
  if (fails == 0) std::printf("mutinfo_host_check ok\n");
  return fails ? 1 : 0;
}
