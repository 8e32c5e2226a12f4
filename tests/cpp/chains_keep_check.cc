// chains_keep_check -- the host half of the chain table (mcpar_amd/csrc/mcx_chains_host.hpp: what mcx_chains_keep is made of)
// as a stand-alone program, for a build under AddressSanitizer and UBSan (tests/test_chains_cpu.py).  Heap-allocated
// arrays of exactly the documented sizes, so that a read or write past one of them is seen.
#include "mcpar_amd/csrc/mcx_chains_host.hpp"

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
  using namespace mcx_chains_host;
  char msg[160];
  const double inf = std::numeric_limits<double>::infinity(), qnan = std::numeric_limits<double>::quiet_NaN();
  for (int nc : {1, 2, 5, 6}) {
    const int ncol = 3;
    std::unique_ptr<mcx_chain_col[]> cols(new mcx_chain_col[(size_t)nc * ncol]);
    std::unique_ptr<mcx_chain_row[]> rows(new mcx_chain_row[nc]);
    std::unique_ptr<int[]> reasons(new int[nc]);
    std::unique_ptr<double[]> centre(new double[ncol * 2]);
    std::unique_ptr<unsigned char[]> use(new unsigned char[ncol]);
    for (int k = 0; k < nc; ++k) {
      for (int c = 0; c < ncol; ++c) cols[(size_t)k * ncol + c] = {k == nc - 1 && c == 1 ? 100.0 : 0.25 * k + c, 1.0, 0.5};
      rows[k] = {k == 0 ? 0 : 7, k == 0 ? 8 : 2, -1.0f, 3, 0};
    }
    use[0] = 1; use[1] = 0; use[2] = 1;
    int nkept = -1;
    mcx_chain_rule rule = {3.0, 1, 0, nullptr};
    CHECK(keep(nc, ncol, cols.get(), rows.get(), &rule, reasons.get(), centre.get(), &nkept, msg, sizeof msg) == MCX_OK);
    CHECK(reasons[0] & MCX_CHAIN_STUCK);
    if (nc >= 5) CHECK(reasons[nc - 1] == MCX_CHAIN_OUTLIER);
    rule.use_col = use.get();
    CHECK(keep(nc, ncol, cols.get(), rows.get(), &rule, reasons.get(), centre.get(), &nkept, msg, sizeof msg) == MCX_OK);
    CHECK(std::isnan(centre[2]) && std::isnan(centre[3]));
    if (nc >= 2) CHECK(reasons[nc - 1] == 0);  // (the column of its outlying mean takes no part)
    rule.z = inf;
    rule.max_stay = 1;
    cols[0].mean = qnan;
    CHECK(keep(nc, ncol, cols.get(), rows.get(), &rule, reasons.get(), nullptr, &nkept, msg, sizeof msg) == MCX_OK);
    CHECK(reasons[0] == MCX_CHAIN_NONFINITE && nkept == 0);
    rule.z = 0.0;
    CHECK(keep(nc, ncol, cols.get(), rows.get(), &rule, reasons.get(), nullptr, &nkept, msg, sizeof msg) == MCX_ERR_INVALID);
    rule.z = qnan;
    CHECK(keep(nc, ncol, cols.get(), rows.get(), &rule, reasons.get(), nullptr, &nkept, msg, sizeof msg) == MCX_ERR_INVALID);
    CHECK(keep(0, ncol, cols.get(), rows.get(), &rule, reasons.get(), nullptr, &nkept, msg, sizeof msg) == MCX_ERR_INVALID);
    CHECK(keep(nc, ncol, nullptr, rows.get(), &rule, reasons.get(), nullptr, &nkept, msg, sizeof msg) == MCX_ERR_INVALID);
  }
  printf("chains_keep_check ok\n");
  return 0;
}
