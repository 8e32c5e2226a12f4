// clip_thresholds_check -- the host half of the tail clip (mcpar_amd/csrc/mcx_clip_host.hpp: what mcx_debug_clip_thresholds and
// the spec check of every clip call are made of) as a stand-alone program, to be built with -fsanitize=address,undefined on
// the host and run without a device (tests/test_clip_cpu.py does).  The arrays are heap blocks of exactly ncol entries, so a
// read or write past a column is the sanitizer's to report.
#include "mcpar_amd/csrc/mcx_clip_host.hpp"

#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static int failures = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("%s:%d: %s is false\n", __FILE__, __LINE__, #cond);  \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

int main()
{
  using namespace mcx_clip_host;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  char msg[160];
  int cols_dummy = 0;
  long long nkept = 0;

  // the spec check
  mcx_clip_spec s = {0.01, 0.99, 0.0, nullptr, nullptr};
  CHECK(spec_check(&s, &cols_dummy, &nkept, msg, sizeof msg) == MCX_OK);
  CHECK(spec_check(nullptr, &cols_dummy, &nkept, msg, sizeof msg) == MCX_ERR_INVALID);
  CHECK(spec_check(&s, nullptr, &nkept, msg, sizeof msg) == MCX_ERR_INVALID);
  CHECK(spec_check(&s, &cols_dummy, nullptr, msg, sizeof msg) == MCX_ERR_INVALID);
  const double bad[][2] = {{0.5, 0.5}, {0.9, 0.1}, {-0.1, 0.9}, {0.1, 1.5}, {nan, 0.9}, {0.1, nan}};
  for (const auto &b : bad) {
    mcx_clip_spec t = {b[0], b[1], 0.0, nullptr, nullptr};
    char tiny[8];  // (a message longer than its buffer is cut, not written past it)
    CHECK(spec_check(&t, &cols_dummy, &nkept, tiny, sizeof tiny) == MCX_ERR_INVALID);
    CHECK(std::strlen(tiny) < sizeof tiny);
  }
  mcx_clip_spec edge = {0.0, 1.0, nan, nullptr, nullptr};
  CHECK(spec_check(&edge, &cols_dummy, &nkept, msg, sizeof msg) == MCX_OK);

  // the thresholds, for 1, 2 and 17 columns
  for (int ncol : {1, 2, 17}) {
    std::vector<double> q((size_t)ncol * 2), lo(ncol), hi(ncol), glo(ncol, nan), ghi(ncol, nan);
    for (int c = 0; c < ncol; ++c) {
      q[2 * c] = -1.0 - c;
      q[2 * c + 1] = 1.0 + c;
    }
    // ll_hi = 0, +inf, NaN
    for (double ll : {0.0, inf, nan}) {
      mcx_clip_spec t = {0.01, 0.99, ll, nullptr, nullptr};
      CHECK(thresholds(ncol, q.data(), &t, lo.data(), hi.data(), msg, sizeof msg) == MCX_OK);
      for (int c = 0; c < ncol; ++c) {
        CHECK(lo[c] == q[2 * c]);
        CHECK(hi[c] == (c == ncol - 1 && !std::isnan(ll) ? ll : q[2 * c + 1]));
      }
      CHECK(needs_quantiles(&t, ncol));
    }
    // overrides: NaN entries are defaults, the last column's hi replaces ll_hi, +-inf are bounds like any other
    glo[0] = -inf;
    ghi[ncol - 1] = -0.25;
    mcx_clip_spec t = {0.01, 0.99, 0.0, glo.data(), ghi.data()};
    CHECK(thresholds(ncol, q.data(), &t, lo.data(), hi.data(), msg, sizeof msg) == MCX_OK);
    CHECK(lo[0] == -inf && hi[ncol - 1] == -0.25);
    for (int c = 1; c < ncol; ++c) CHECK(lo[c] == q[2 * c]);
    for (int c = 0; c < ncol - 1; ++c) CHECK(hi[c] == q[2 * c + 1]);
    // every bound given: no quantile is read (q = NULL) or needed
    for (int c = 0; c < ncol; ++c) {
      glo[c] = -2.0;
      ghi[c] = 2.0;
    }
    CHECK(!needs_quantiles(&t, ncol));
    CHECK(thresholds(ncol, nullptr, &t, lo.data(), hi.data(), msg, sizeof msg) == MCX_OK);
    for (int c = 0; c < ncol; ++c) CHECK(lo[c] == -2.0 && hi[c] == 2.0);
    // all but the last column's hi given: ll_hi stands in for it, still no quantile pass
    ghi[ncol - 1] = nan;
    CHECK(!needs_quantiles(&t, ncol));
    t.ll_hi = nan;
    CHECK(needs_quantiles(&t, ncol));
    // q = NULL without overrides: NaN thresholds
    mcx_clip_spec plain = {0.01, 0.99, nan, nullptr, nullptr};
    CHECK(thresholds(ncol, nullptr, &plain, lo.data(), hi.data(), msg, sizeof msg) == MCX_OK);
    for (int c = 0; c < ncol; ++c) CHECK(std::isnan(lo[c]) && std::isnan(hi[c]));
  }
  mcx_clip_spec t = {0.01, 0.99, 0.0, nullptr, nullptr};
  double one = 0.0;
  CHECK(thresholds(0, nullptr, &t, &one, &one, msg, sizeof msg) == MCX_ERR_INVALID);
  CHECK(thresholds(1, nullptr, nullptr, &one, &one, msg, sizeof msg) == MCX_ERR_INVALID);
  CHECK(thresholds(1, nullptr, &t, nullptr, &one, msg, sizeof msg) == MCX_ERR_INVALID);

  if (failures) return 1;
  std::printf("clip_thresholds_check ok\n");
  return 0;
}
