// mcx_chains_host.hpp -- the host half of the chain table: the rule that turns a table into the list of
// chains to keep.  Plain C++ over include/mcx.h, no HIP and no library state: mcx_chains.hip calls this very function
// (mcx_chains_keep is keep() behind the library's error text), and tests/cpp/chains_keep_check.cc compiles it on its own
// under a sanitizer.
#pragma once
#include "../../include/mcx.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <limits>
#include <vector>

namespace mcx_chains_host {

// numpy's median of v (which it may reorder): the mean of the two middle values when the count is even; NaN of none
inline double median(std::vector<double> &v)
{
  const size_t n = v.size();
  if (n == 0) return std::numeric_limits<double>::quiet_NaN();
  std::sort(v.begin(), v.end());
  return n % 2 ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) / 2.0;
}

inline bool chain_nonfinite(int ncol, const mcx_chain_col *cols, const mcx_chain_row &row)
{
  if (row.flags & MCX_SUMMARY_NONFINITE) return true;
  for (int c = 0; c < ncol; ++c)
    if (!std::isfinite(cols[c].mean)) return true;
  return false;
}

// MCX_OK, or MCX_ERR_INVALID with the reason in msg[len].  reasons[nc]; centre[ncol][2] = (med, scale) of the columns that
// take part, NaN of the others (may be NULL); *nkept = the chains with reasons 0
inline int keep(int nc, int ncol, const mcx_chain_col *cols, const mcx_chain_row *chains, const mcx_chain_rule *rule, int *reasons,
                double *centre, int *nkept, char *msg, size_t len)
{
  if (nc < 1 || ncol < 1) {
    snprintf(msg, len, "nc = %d, ncol = %d: a table of at least one chain and one column", nc, ncol);
    return MCX_ERR_INVALID;
  }
  if (!cols || !chains || !rule || !reasons || !nkept) {
    snprintf(msg, len, "cols, chains, rule, reasons or nkept is NULL");
    return MCX_ERR_INVALID;
  }
  if (!(rule->z > 0.0)) {  // (a NaN fails the comparison too)
    snprintf(msg, len, "z = %g: a positive number of scales, or +inf for no outlier test", rule->z);
    return MCX_ERR_INVALID;
  }
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  for (int k = 0; k < nc; ++k) {
    const mcx_chain_row &r = chains[k];
    if (chain_nonfinite(ncol, cols + (size_t)k * ncol, r)) {
      reasons[k] = MCX_CHAIN_NONFINITE;
      continue;
    }
    const bool stuck = r.moves < rule->min_moves || (rule->max_stay > 0 && r.longest_stay > rule->max_stay);
    reasons[k] = stuck ? MCX_CHAIN_STUCK : 0;
  }
  std::vector<double> v;
  for (int c = 0; c < ncol; ++c) {
    double med = qnan, scale = qnan;
    if (!rule->use_col || rule->use_col[c]) {
      auto mean = [&](int k) { return cols[(size_t)k * ncol + c].mean; };
      v.clear();
      for (int k = 0; k < nc; ++k)
        if (std::isfinite(mean(k))) v.push_back(mean(k));
      med = median(v);
      for (double &d : v) d = std::fabs(d - med);
      scale = 1.4826 * median(v);
      if (!std::isinf(rule->z)) {
        const double bound = rule->z * scale;
        for (int k = 0; k < nc; ++k)
          if (reasons[k] != MCX_CHAIN_NONFINITE && std::fabs(mean(k) - med) > bound) reasons[k] |= MCX_CHAIN_OUTLIER;
      }
    }
    if (centre) {
      centre[2 * c] = med;
      centre[2 * c + 1] = scale;
    }
  }
  int kept = 0;
  for (int k = 0; k < nc; ++k) kept += reasons[k] == 0;
  *nkept = kept;
  return MCX_OK;
}

}  // namespace mcx_chains_host
