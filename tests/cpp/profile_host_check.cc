// profile_host_check.cc -- mcpar_amd/csrc/mcx_profile_host.hpp compiled alone (no HIP, no library): the order of log L, the
// bins, the refusals, the hull, the intervals and the levels on hand-made cases.  tests/test_profile_cpu.py builds it plain and
// with -fsanitize=address,undefined and runs it; it prints what fails and returns the number of failures.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "mcpar_amd/csrc/mcx_profile_host.hpp"

namespace ph = mcx_profile_host;

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);          \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static const double INF = std::numeric_limits<double>::infinity();
static const double QNAN = std::numeric_limits<double>::quiet_NaN();
static const float FINF = std::numeric_limits<float>::infinity();

static void check_keys()
{
  const float ls[] = {-FINF, -3.0e38f, -1.0f, -1.0e-45f, -0.0f, 0.0f, 1.0e-45f, 2.5f, 3.0e38f, FINF};
  for (size_t i = 0; i + 1 < sizeof ls / sizeof *ls; ++i) {
    CHECK(ph::ll_key(ls[i]) < ph::ll_key(ls[i + 1]));
    CHECK(ph::float_bits(ph::key_ll(ph::ll_key(ls[i]))) == ph::float_bits(ls[i]));
  }
  CHECK(ph::ll_key(std::numeric_limits<float>::quiet_NaN()) == ph::ll_key(-FINF));
  CHECK(ph::ll_key(-std::numeric_limits<float>::quiet_NaN()) == ph::ll_key(-FINF));
  // the first row wins a tie, a larger log L wins whatever its row; no key is 0
  CHECK(ph::row_key(1.0f, 3) > ph::row_key(1.0f, 4));
  CHECK(ph::row_key(1.5f, 4000000000ull) > ph::row_key(1.0f, 0));
  CHECK(ph::row_key(-FINF, 0xFFFFFFFEull) != 0);
  CHECK(ph::key_row(ph::row_key(2.0f, 4000000000ull)) == 4000000000ll && ph::key_row(0) == -1);
  CHECK(ph::key_lmax(ph::row_key(-0.0f, 7)) == 0.0f && std::signbit(ph::key_lmax(ph::row_key(-0.0f, 7))));
  CHECK(ph::key_lmax(0) == -FINF);
}

static void check_bins()
{
  ph::Grid g;
  std::string why;
  CHECK(ph::grid_of(0, 4, 0.0f, 8.0f, false, QNAN, QNAN, nullptr, nullptr, g, why) == ph::OK && g.inv == 0.5);
  CHECK(ph::bin_of(0.0f, g, 4) == 0 && ph::bin_of(1.99f, g, 4) == 0 && ph::bin_of(2.0f, g, 4) == 1 && ph::bin_of(7.99f, g, 4) == 3);
  CHECK(ph::bin_of(8.0f, g, 4) == 3);  // v == to
  CHECK(ph::bin_of(-0.01f, g, 4) == -1 && ph::bin_of(8.01f, g, 4) == -1 && ph::bin_of(std::numeric_limits<float>::quiet_NaN(), g, 4) == -1);
  // to == from: the values equal to it go to bin 0, everything else is dropped
  CHECK(ph::grid_of(0, 4, 3.0f, 3.0f, false, QNAN, QNAN, nullptr, nullptr, g, why) == ph::OK && std::isinf(g.inv));
  CHECK(ph::bin_of(3.0f, g, 4) == 0 && ph::bin_of(2.9f, g, 4) == -1 && ph::bin_of(3.1f, g, 4) == -1);
  // the clip pair, the spec over both
  const double from[2] = {QNAN, 1.0}, to[2] = {QNAN, 5.0};
  CHECK(ph::grid_of(0, 2, 0.0f, 8.0f, true, 2.0, 6.0, from, to, g, why) == ph::OK && g.from == 2.0 && g.to == 6.0);
  CHECK(ph::grid_of(1, 2, 0.0f, 8.0f, true, 2.0, 6.0, from, to, g, why) == ph::OK && g.from == 1.0 && g.to == 5.0);
  const double far[1] = {9.0};
  CHECK(ph::grid_of(0, 2, 0.0f, 8.0f, false, QNAN, QNAN, far, nullptr, g, why) == ph::INVALID && !why.empty());
}

static void check_refusals()
{
  std::string why;
  CHECK(ph::spec_check(64, 2, 512, 0.0, 1.0, nullptr, nullptr, 3, 100, why) == ph::OK);
  CHECK(ph::spec_check(1, 2, 512, 0.0, 1.0, nullptr, nullptr, 3, 100, why) == ph::INVALID);
  CHECK(ph::spec_check(513, 2, 512, 0.0, 1.0, nullptr, nullptr, 3, 100, why) == ph::INVALID);
  CHECK(ph::spec_check(64, 2, 512, 0.5, 0.5, nullptr, nullptr, 3, 100, why) == ph::INVALID);
  CHECK(ph::spec_check(64, 2, 512, -0.1, 0.9, nullptr, nullptr, 3, 100, why) == ph::INVALID);
  CHECK(ph::spec_check(64, 2, 512, QNAN, 0.9, nullptr, nullptr, 3, 100, why) == ph::INVALID);
  const double inf3[3] = {QNAN, INF, QNAN}, lo3[3] = {QNAN, 2.0, QNAN}, hi3[3] = {QNAN, 1.0, QNAN};
  CHECK(ph::spec_check(64, 2, 512, 0.0, 1.0, inf3, nullptr, 3, 100, why) == ph::INVALID);
  CHECK(ph::spec_check(64, 2, 512, 0.0, 1.0, lo3, hi3, 3, 100, why) == ph::INVALID);
  CHECK(ph::spec_check(64, 2, 512, 0.0, 1.0, hi3, lo3, 3, 100, why) == ph::OK);
  CHECK(ph::spec_check(64, 2, 512, 0.0, 1.0, nullptr, nullptr, 3, 1, why) == ph::INVALID);
  CHECK(ph::spec_check(64, 2, 512, 0.0, 1.0, nullptr, nullptr, 3, (1ll << 32) - 1, why) == ph::OK);
  CHECK(ph::spec_check(64, 2, 512, 0.0, 1.0, nullptr, nullptr, 3, 1ll << 32, why) == ph::UNSUPPORTED);
  ph::Levels lv;
  CHECK(ph::levels_of(0, nullptr, 0, false, lv, why) == ph::OK && lv.n == 2 && lv.p[0] == 0.6827 && lv.p[1] == 0.9545);
  CHECK(std::fabs(lv.drop[0] - 0.5) < 1e-4 && std::fabs(lv.drop[1] - 2.0) < 1e-4);
  const double ps[2] = {0.5, 0.9};
  CHECK(ph::levels_of(2, ps, 0, true, lv, why) == ph::OK && lv.drop[0] == -std::log(1.0 - 0.5) && lv.drop[1] == -std::log(1.0 - 0.9));
  CHECK(ph::levels_of(2, ps, 1, false, lv, why) == ph::OK && lv.drop[0] == 0.5 && std::isnan(lv.p[0]));
  CHECK(ph::levels_of(9, ps, 0, false, lv, why) == ph::INVALID && ph::levels_of(-1, ps, 0, false, lv, why) == ph::INVALID);
  CHECK(ph::levels_of(2, nullptr, 0, false, lv, why) == ph::INVALID);
  for (double bad : {0.0, 1.0, -0.5, 1.5, QNAN}) CHECK(ph::levels_of(1, &bad, 0, false, lv, why) == ph::INVALID);
  for (double bad : {0.0, -1.0, INF, QNAN}) CHECK(ph::levels_of(1, &bad, 1, false, lv, why) == ph::INVALID);
  std::vector<int> pl;
  CHECK(ph::pair_list(0, nullptr, 3, pl, why) == ph::OK && pl.size() == 6 && pl[0] == 0 && pl[1] == 1 && pl[4] == 1 && pl[5] == 2);
  CHECK(ph::pair_list(0, nullptr, 1, pl, why) == ph::INVALID && ph::pair_list(0, nullptr, 47, pl, why) == ph::INVALID);
  const int same[2] = {1, 1}, out[2] = {0, 3}, ok[4] = {2, 0, 0, 2};
  CHECK(ph::pair_list(1, same, 3, pl, why) == ph::INVALID && ph::pair_list(1, out, 3, pl, why) == ph::INVALID);
  CHECK(ph::pair_list(2, ok, 3, pl, why) == ph::OK && pl.size() == 4 && ph::pair_list(1025, ok, 3, pl, why) == ph::INVALID);
}

static void check_hull()
{
  // a two-humped curve with an empty bin and a bin at -inf
  const int n = 9;
  const double x[n] = {0.0, 1.0, 2.0, QNAN, 4.0, 5.0, 6.0, 7.0, 8.0};
  const double y[n] = {-4.0, -1.0, -3.0, -INF, -2.5, 0.0, -INF, -1.5, -6.0};
  double h[n];
  ph::hull(n, x, y, h);
  CHECK(std::isnan(h[3]) && h[6] == -INF);
  for (int j = 0; j < n; ++j)
    if (!std::isnan(x[j]) && std::isfinite(y[j])) CHECK(h[j] >= y[j]);
  CHECK(h[0] == y[0] && h[1] == y[1] && h[5] == y[5] && h[8] == y[8]);
  CHECK(h[2] == -1.0 + 1.0 * ((2.0 - 1.0) / (5.0 - 1.0)) && h[4] == -1.0 + 1.0 * ((4.0 - 1.0) / (5.0 - 1.0)));
  // concave: the slopes between consecutive finite points do not increase
  double prev = INF;
  int last = -1;
  for (int j = 0; j < n; ++j) {
    if (std::isnan(x[j]) || !std::isfinite(h[j])) continue;
    if (last >= 0) {
      const double s = (h[j] - h[last]) / (x[j] - x[last]);
      CHECK(s <= prev + 1e-15);
      prev = s;
    }
    last = j;
  }
  // a concave curve is its own hull
  const double xc[5] = {0.0, 1.0, 2.5, 3.0, 7.0}, yc[5] = {-9.0, -4.0, 0.0, -0.5, -30.0};
  double hc[5];
  ph::hull(5, xc, yc, hc);
  CHECK(std::memcmp(hc, yc, sizeof yc) == 0);
}

static void check_intervals()
{
  const int n = 9;
  const double x[n] = {0.0, 1.0, 2.0, QNAN, 4.0, 5.0, 6.0, 7.0, 8.0};
  const double y[n] = {-4.0, -1.0, -3.0, -INF, -2.5, 0.0, -INF, -1.5, -6.0};
  ph::Ends e = ph::interval(n, x, y, 2.0);  // inside: bins 1, 5, 7: three runs (2 and 4 and 6 are below)
  CHECK(e.nseg == 3 && e.open == 0);
  CHECK(e.lo == 0.0 + (1.0 - 0.0) * ((-2.0 + 4.0) / (-1.0 + 4.0)) && e.hi == 8.0 + (7.0 - 8.0) * ((-2.0 + 6.0) / (-1.5 + 6.0)));
  e = ph::interval(n, x, y, 0.5);           // bin 5 alone: bin 4 below it (the empty bin 3 is skipped), bin 6 is at -inf
  CHECK(e.nseg == 1 && e.open == 0 && e.lo == 4.0 + (5.0 - 4.0) * ((-0.5 + 2.5) / (0.0 + 2.5)) && e.hi == 5.0);
  e = ph::interval(n, x, y, 100.0);         // every finite bin: both ends open, the bin at -inf splits the run
  CHECK(e.nseg == 2 && e.open == 3 && e.lo == 0.0 && e.hi == 8.0);
  const double xe[4] = {QNAN, 1.0, QNAN, 3.0}, ye[4] = {-INF, -5.0, -INF, -4.0};
  e = ph::interval(4, xe, ye, 1.0);
  CHECK(e.open == 4 && e.nseg == 0 && std::isnan(e.lo) && std::isnan(e.hi));
  e = ph::interval(4, xe, ye, 4.5);         // the last bin alone: the empty bin between is skipped, the upper end is open
  CHECK(e.open == 2 && e.nseg == 1 && e.lo == 1.0 + (3.0 - 1.0) * ((-4.5 + 5.0) / (-4.0 + 5.0)) && e.hi == 3.0);
  const double yn[4] = {QNAN, QNAN, QNAN, QNAN};
  e = ph::interval(4, xe, yn, 1.0);
  CHECK(e.open == 0 && e.nseg == 0 && std::isnan(e.lo));
  double h[n];
  ph::hull(n, x, y, h);
  const ph::Interval iv = ph::interval_of(n, x, y, h, 0.9, 2.0);
  CHECK(iv.nseg == 3 && iv.lo_hull <= iv.lo && iv.hi_hull >= iv.hi && iv.flags == 0 && iv.p == 0.9 && iv.drop == 2.0);
}

static void check_finish()
{
  // four bins: rows 5 (log L 1), none, 2 (log L 3, the maximum of all rows), 9 (log L -inf)
  const uint64_t keys[4] = {ph::row_key(1.0f, 5), 0, ph::row_key(3.0f, 2), ph::row_key(-FINF, 9)};
  const uint64_t cnt[4] = {3, 0, 1, 2};
  const float xat[4] = {0.5f, 123.0f, 2.5f, 3.5f};
  ph::Levels lv;
  std::string why;
  CHECK(ph::levels_of(0, nullptr, 0, false, lv, why) == ph::OK);
  float lmax[4];
  long long row[4], nb;
  int ne;
  double x[4], pl[4], plh[4];
  ph::Interval iv[2];
  int fl = ph::finish_column(4, keys, cnt, xat, keys[2], lv, lmax, row, x, pl, plh, iv, &nb, &ne);
  CHECK(fl == 0 && nb == 6 && ne == 1 && row[0] == 5 && row[1] == -1 && row[2] == 2 && row[3] == 9);
  CHECK(pl[0] == -2.0 && pl[1] == -INF && pl[2] == 0.0 && pl[3] == -INF && std::isnan(x[1]) && std::isnan(plh[1]) && plh[3] == -INF);
  CHECK(iv[0].nseg == 1 && iv[0].flags == 0 && iv[0].hi == 2.5 && iv[0].lo > 0.5 && iv[0].lo < 2.5);
  // a maximum that is not finite
  fl = ph::finish_column(4, keys, cnt, xat, ph::row_key(FINF, 0), lv, lmax, row, x, pl, plh, iv, &nb, &ne);
  CHECK(fl == ph::F_LL_NONFINITE && std::isnan(pl[0]) && std::isnan(plh[2]) && std::isnan(iv[1].lo) && iv[1].nseg == 0);
  // a pair
  const uint64_t pk[64] = {ph::row_key(3.0f, 2), 0, ph::row_key(2.5f, 1)};
  const uint64_t pc[64] = {1, 0, 4};
  float plm[64];
  long long prow[64], nlev[2];
  double z[64];
  ph::Levels l2;
  CHECK(ph::levels_of(0, nullptr, 0, true, l2, why) == ph::OK);
  ph::finish_pair(8, pk, pc, pk[0], l2, plm, prow, z, nlev, &nb, &ne);
  CHECK(nb == 5 && ne == 62 && z[0] == 0.0 && z[2] == -0.5 && z[1] == -INF && nlev[0] == 2 && nlev[1] == 2);
}

int main()
{
  check_keys();
  check_bins();
  check_refusals();
  check_hull();
  check_intervals();
  check_finish();
  if (failures) std::printf("%d checks failed\n", failures);
  return failures;
}
