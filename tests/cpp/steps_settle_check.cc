// steps_settle_check -- the host half of the step table (mcpar_amd/csrc/mcx_steptable_host.hpp: what mcx_steps_settle and the
// table's check of its probabilities are made of) as a stand-alone program, for a build under AddressSanitizer and UBSan
// (tests/test_steptable_cpu.py).  Heap-allocated arrays of exactly the documented sizes, so that a read or write past one of
// them is seen.
#include "mcpar_amd/csrc/mcx_steptable_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <memory>

#define CHECK(cond)                                            \
  do {                                                         \
    if (!(cond)) {                                             \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                \
    }                                                          \
  } while (0)

int main()
{
  using namespace mcx_steptable_host;
  char msg[160];
  const double inf = std::numeric_limits<double>::infinity(), qnan = std::numeric_limits<double>::quiet_NaN();
  CHECK(window_steps(1, 0.5) == 1 && window_steps(7, 0.5) == 4 && window_steps(8, 0.5) == 4 && window_steps(9, 1.0) == 9);
  CHECK(window_steps(1000, 1e-9) == 1);
  for (int T : {1, 2, 7, 8, 40}) {
    const int ncol = 3;
    std::unique_ptr<mcx_step_col[]> cols(new mcx_step_col[(size_t)T * ncol]);
    std::unique_ptr<mcx_step_settle_col[]> out(new mcx_step_settle_col[ncol]);
    std::unique_ptr<unsigned char[]> use(new unsigned char[ncol]);
    auto flat = [&] {
      for (int t = 0; t < T; ++t)
        for (int c = 0; c < ncol; ++c) cols[(size_t)t * ncol + c] = {1.0 + c, 2.0, -1.0f, 1.0f, 0, 0};
    };
    flat();
    mcx_step_rule rule = {0.1, 0.1, 0.5, nullptr};
    int settled = -7;
    CHECK(settle(T, ncol, cols.get(), &rule, out.get(), &settled, msg, sizeof msg) == MCX_OK);
    CHECK(settled == 0);
    for (int c = 0; c < ncol; ++c)
      CHECK(out[c].m_ref == 1.0 + c && out[c].s_ref == 2.0 && out[c].last_out == -1 && out[c].max_dev_mean == 0.0 && out[c].max_dev_sd == 0.0);
    const int R = window_steps(T, 0.5);
    if (T - R >= 1) {  // a drift in column 1 that ends with step T - R - 1: settled at the window's first step
      for (int t = 0; t < T - R; ++t) cols[(size_t)t * ncol + 1].mean = 9.0;
      CHECK(settle(T, ncol, cols.get(), &rule, out.get(), &settled, msg, sizeof msg) == MCX_OK);
      CHECK(settled == T - R && out[1].last_out == T - R - 1 && out[0].last_out == -1 && out[1].max_dev_mean == 3.5);
      use[0] = 1; use[1] = 0; use[2] = 1;
      rule.use_col = use.get();
      CHECK(settle(T, ncol, cols.get(), &rule, out.get(), &settled, msg, sizeof msg) == MCX_OK);
      CHECK(settled == 0 && std::isnan(out[1].m_ref) && out[1].last_out == -1);
      rule.use_col = nullptr;
    }
    flat();
    cols[(size_t)(T - 1) * ncol + 2].sd = 3.0;  // the last step out of band (a window of 4 or more steps): inside the window
    CHECK(settle(T, ncol, cols.get(), &rule, out.get(), &settled, msg, sizeof msg) == MCX_OK);
    if (T >= 7) CHECK(settled == -1 && out[2].last_out == T - 1);
    flat();
    cols[0].mean = qnan;  // a non-finite step is out of band; in the window (T <= 2) it makes m_ref NaN
    cols[0].sd = qnan;
    CHECK(settle(T, ncol, cols.get(), &rule, out.get(), &settled, msg, sizeof msg) == MCX_OK);
    CHECK(out[0].last_out == 0 && settled == (T - R >= 1 ? 1 : -1));
    flat();
    for (int t = 0; t < T; ++t) cols[(size_t)t * ncol].sd = 0.0;  // s_ref = 0: not settled
    CHECK(settle(T, ncol, cols.get(), &rule, out.get(), &settled, msg, sizeof msg) == MCX_OK);
    CHECK(settled == -1 && out[0].s_ref == 0.0 && std::isnan(out[0].max_dev_mean));
    use[0] = use[1] = use[2] = 0;
    rule.use_col = use.get();
    CHECK(settle(T, ncol, cols.get(), &rule, out.get(), &settled, msg, sizeof msg) == MCX_ERR_INVALID);
    rule.use_col = nullptr;
    for (double bad : {-0.1, qnan}) {
      mcx_step_rule r2 = {bad, 0.1, 0.5, nullptr};
      CHECK(settle(T, ncol, cols.get(), &r2, out.get(), &settled, msg, sizeof msg) == MCX_ERR_INVALID);
      r2 = {0.1, bad, 0.5, nullptr};
      CHECK(settle(T, ncol, cols.get(), &r2, out.get(), &settled, msg, sizeof msg) == MCX_ERR_INVALID);
    }
    for (double bad : {0.0, -1.0, 1.5, qnan, inf}) {
      mcx_step_rule r2 = {0.1, 0.1, bad, nullptr};
      CHECK(settle(T, ncol, cols.get(), &r2, out.get(), &settled, msg, sizeof msg) == MCX_ERR_INVALID);
    }
    CHECK(settle(0, ncol, cols.get(), &rule, out.get(), &settled, msg, sizeof msg) == MCX_ERR_INVALID);
    CHECK(settle(T, ncol, nullptr, &rule, out.get(), &settled, msg, sizeof msg) == MCX_ERR_INVALID);
    CHECK(settle(T, ncol, cols.get(), &rule, out.get(), nullptr, msg, sizeof msg) == MCX_ERR_INVALID);
  }
  for (int n : {0, 1, 8}) {
    std::unique_ptr<double[]> p(new double[n ? n : 1]);
    for (int k = 0; k < n; ++k) p[k] = (double)k / (n > 1 ? n - 1 : 1);
    CHECK(probs_args(p.get(), n, msg, sizeof msg) == MCX_OK);
    if (n) {
      p[n - 1] = qnan;
      CHECK(probs_args(p.get(), n, msg, sizeof msg) == MCX_ERR_INVALID);
      p[n - 1] = 1.0000001;
      CHECK(probs_args(p.get(), n, msg, sizeof msg) == MCX_ERR_INVALID);
      CHECK(probs_args(nullptr, n, msg, sizeof msg) == MCX_ERR_INVALID);
    }
  }
  CHECK(probs_args(nullptr, 0, msg, sizeof msg) == MCX_OK);
  CHECK(probs_args(nullptr, 9, msg, sizeof msg) == MCX_ERR_INVALID && probs_args(nullptr, -1, msg, sizeof msg) == MCX_ERR_INVALID);
  printf("steps_settle_check ok\n");
  return 0;
}
