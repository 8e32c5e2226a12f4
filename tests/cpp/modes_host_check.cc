// The host half of the modes of a store (mcpar_amd/csrc/mcx_modes_host.hpp) as a stand-alone program: the seeding, the
// centre update, the refusals and the best-log-L merge on small cases whose answers are worked out by hand.  Built plain
// and with -fsanitize=address,undefined by tests/test_modes_cpu.py.
#include "mcpar_amd/csrc/mcx_modes_host.hpp"

#include <cstdio>
#include <cstring>

namespace mh = mcx_modes_host;

static int fails = 0;
#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                  \
    }                                                           \
  } while (0)

int main()
{
  char msg[160];
  // ---- refusals
  CHECK(mh::spec_check(0, 50, 16, nullptr, 2, 10, msg, sizeof msg) == mh::ERR_INVALID);
  CHECK(mh::spec_check(33, 50, 16, nullptr, 2, 100, msg, sizeof msg) == mh::ERR_INVALID && std::strstr(msg, "k = 33"));
  CHECK(mh::spec_check(2, 0, 16, nullptr, 2, 10, msg, sizeof msg) == mh::ERR_INVALID && std::strstr(msg, "max_iter"));
  CHECK(mh::spec_check(2, 1, 0, nullptr, 2, 10, msg, sizeof msg) == mh::ERR_INVALID && std::strstr(msg, "seed_rows"));
  CHECK(mh::spec_check(11, 1, 16, nullptr, 2, 10, msg, sizeof msg) == mh::ERR_INVALID && std::strstr(msg, "10 rows"));
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double cbad[4] = {0.0, 1.0, 2.0, nan}, cinf[4] = {0.0, inf, 2.0, 3.0}, cok[4] = {0.0, 1.0, 2.0, 3.0};
  CHECK(mh::spec_check(2, 1, 16, cbad, 2, 10, msg, sizeof msg) == mh::ERR_INVALID && std::strstr(msg, "centres[1][1]"));
  CHECK(mh::spec_check(2, 1, 16, cinf, 2, 10, msg, sizeof msg) == mh::ERR_INVALID && std::strstr(msg, "centres[0][1]"));
  CHECK(mh::spec_check(2, 1, 16, cok, 2, 10, msg, sizeof msg) == mh::OK);
  CHECK(mh::spec_check(32, 1, 1, nullptr, 256, 32, msg, sizeof msg) == mh::OK);

  // ---- the scale
  CHECK(mh::scale_of_sd(2.0) == 0.5 && mh::scale_of_sd(0.0) == 0.0 && mh::scale_of_sd(nan) == 0.0 && mh::scale_of_sd(inf) == 0.0);
  CHECK(mh::scale_of_sd(-1.0) == 0.0 && mh::scale_of_sd(4.9e-324) == 0.0);

  // ---- the distance: the stated order, skipped columns
  {
    const float x[3] = {1.0f, 2.0f, 3.0f};
    const double s[3] = {1.0, 0.0, 2.0}, c[3] = {0.0, 100.0, 4.0};
    CHECK(mh::dist2(x, s, c, 3) == 1.0 + 4.0);
    CHECK(!mh::row_finite(x, 0) == false);
    const float y[2] = {1.0f, std::numeric_limits<float>::infinity()};
    CHECK(!mh::row_finite(y, 2) && mh::row_finite(y, 1));
  }

  // ---- the seeding: rows (x, ll); two clumps at 0 and 10 and a NaN row
  {
    const float fn = std::numeric_limits<float>::quiet_NaN();
    const float rows[] = {0.0f, -1.0f, 0.5f, -0.5f, fn, 9.0f, 10.0f, -0.25f, 10.5f, -3.0f, 0.5f, -0.5f};
    const double s[1] = {1.0};
    long long idx[3];
    // the largest log L among the finite rows is -0.25 at row 3 (row 2, log L 9, has a NaN parameter)
    CHECK(mh::seed(rows, 6, 1, 1, 0u, s, idx, msg, sizeof msg) == mh::OK && idx[0] == 3);
    for (uint32_t sd = 0; sd < 64; ++sd) {
      CHECK(mh::seed(rows, 6, 1, 3, sd, s, idx, msg, sizeof msg) == mh::OK);
      CHECK(idx[0] == 3 && idx[1] != 2 && idx[2] != 2 && idx[1] != 3 && idx[2] != 3 && idx[1] != idx[2]);
      // D of rows 0, 1, 5 from centre 10 is 100, 90.25, 90.25, of row 4 0.25: the second centre is almost surely in the far clump
      const double u = mh::seed_uniform(sd, 1), t = u * (100.0 + 90.25 + 0.25 + 90.25);
      const long long want = t < 100.0 ? 0 : t < 190.25 ? 1 : t < 190.5 ? 4 : 5;
      CHECK(idx[1] == want);
      CHECK(u >= 0.0 && u < 1.0);
    }
    // five finite rows: six centres are refused, five are five distinct rows
    long long idx6[6];
    CHECK(mh::seed(rows, 6, 1, 6, 1u, s, idx6, msg, sizeof msg) == mh::ERR_INVALID && std::strstr(msg, "5 rows with finite"));
    CHECK(mh::seed(rows, 6, 1, 5, 1u, s, idx6, msg, sizeof msg) == mh::OK);
    int seen = 0;
    for (int k = 0; k < 5; ++k) seen |= 1 << idx6[k];
    CHECK(seen == (1 | 2 | 8 | 16 | 32));
    // every row on one point: total = 0, the first finite rows not yet taken
    const float same[] = {1.0f, 0.0f, 1.0f, 0.0f, 1.0f, 0.0f};
    CHECK(mh::seed(same, 3, 1, 3, 9u, s, idx, msg, sizeof msg) == mh::OK && idx[0] == 0 && idx[1] == 1 && idx[2] == 2);
    // a NaN log L counts as -inf
    const float nll[] = {0.0f, fn, 1.0f, -5.0f};
    CHECK(mh::seed(nll, 2, 1, 1, 0u, s, idx, msg, sizeof msg) == mh::OK && idx[0] == 1);
    // a column that takes no part
    const double s0[1] = {0.0};
    CHECK(mh::seed(rows, 6, 1, 2, 3u, s0, idx, msg, sizeof msg) == mh::OK && idx[0] == 3 && idx[1] == 0);
  }

  // ---- the centre update and the unscaling
  {
    const long long n[3] = {2, 0, 4};
    const double S[6] = {3.0, 5.0, 99.0, 99.0, -8.0, 2.0};
    double c[6] = {0.0, 0.0, 7.0, 8.0, 0.0, 0.0}, out[6];
    CHECK(mh::update_centres(3, 2, n, S, c) == mh::F_EMPTY);
    CHECK(c[0] == 1.5 && c[1] == 2.5 && c[2] == 7.0 && c[3] == 8.0 && c[4] == -2.0 && c[5] == 0.5);
    const long long n2[1] = {1};
    CHECK(mh::update_centres(1, 2, n2, S, c) == 0 && c[0] == 3.0 && c[1] == 5.0);
    const double s[2] = {2.0, 0.0};
    mh::unscale(3, 2, s, c, out);
    CHECK(out[0] == 1.5 && std::isnan(out[1]) && out[2] == 3.5 && std::isnan(out[5]));
  }

  // ---- the best log L of a mode over the workgroups
  {
    auto key = [](float f) {
      uint32_t b;
      std::memcpy(&b, &f, sizeof b);
      return (1ull << 32) | (unsigned long long)mh::order_key(b);
    };
    const unsigned long long w[] = {key(-2.0f), 7, 0, 0, key(1.5f), 40, key(1.5f), 12, key(-0.0f), 3};
    uint32_t bits = 0;
    long long row = -1;
    float f;
    CHECK(mh::best_ll(w, 5, 2, &bits, &row) && row == 12);
    std::memcpy(&f, &bits, sizeof f);
    CHECK(f == 1.5f);
    CHECK(mh::best_ll(w, 2, 2, &bits, &row) && row == 7);
    std::memcpy(&f, &bits, sizeof f);
    CHECK(f == -2.0f);
    CHECK(!mh::best_ll(w + 2, 1, 2, &bits, &row));
    CHECK(key(-0.0f) < key(0.0f) && key(-std::numeric_limits<float>::infinity()) < key(-3.0e38f));
  }
  if (fails) return 1;
  std::printf("modes host ok\n");
  return 0;
}
