// mcx_steptable_host.hpp -- the host half of the step table: the rule that turns a table into the step
// from which the ensemble no longer drifts, and what the table's entry points refuse of a list of probabilities.  Plain C++
// over include/mcx.h, no HIP and no library state: mcx_steptable.hip calls these very functions (mcx_steps_settle is settle()
// behind the library's error text), and tests/cpp/steps_settle_check.cc compiles them on their own under a sanitizer.
#pragma once
#include "../../include/mcx.h"

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <limits>

namespace mcx_steptable_host {

// MCX_OK, or MCX_ERR_INVALID with the reason in msg[len]: nprobs in [0, MCX_STEP_MAX_PROBS], every p in [0, 1]
inline int probs_args(const double *probs, int nprobs, char *msg, size_t len)
{
  if (nprobs < 0 || nprobs > MCX_STEP_MAX_PROBS) {
    snprintf(msg, len, "nprobs = %d: 0 to %d probabilities", nprobs, (int)MCX_STEP_MAX_PROBS);
    return MCX_ERR_INVALID;
  }
  if (nprobs > 0 && !probs) {
    snprintf(msg, len, "probs is NULL with nprobs = %d", nprobs);
    return MCX_ERR_INVALID;
  }
  for (int k = 0; k < nprobs; ++k)
    if (!(probs[k] >= 0.0 && probs[k] <= 1.0)) {  // (a NaN fails the comparison too)
      snprintf(msg, len, "probs[%d] = %g is not a probability in [0, 1]", k, probs[k]);
      return MCX_ERR_INVALID;
    }
  return MCX_OK;
}

// the steps of the reference window: max(1, ceil(ref_frac T)), T at most
inline int window_steps(int T, double ref_frac)
{
  const double r = std::ceil(ref_frac * (double)T);
  return r < 1.0 ? 1 : r > (double)T ? T : (int)r;
}

// MCX_OK, or MCX_ERR_INVALID with the reason in msg[len].  cols[T][ncol]; out_cols[ncol]; *settled_step as include/mcx.h
// states it
inline int settle(int T, int ncol, const mcx_step_col *cols, const mcx_step_rule *rule, mcx_step_settle_col *out_cols,
                  int *settled_step, char *msg, size_t len)
{
  if (T < 1 || ncol < 1) {
    snprintf(msg, len, "nsteps = %d, ncol = %d: a table of at least one step and one column", T, ncol);
    return MCX_ERR_INVALID;
  }
  if (!cols || !rule || !out_cols || !settled_step) {
    snprintf(msg, len, "cols, rule, out_cols or settled_step is NULL");
    return MCX_ERR_INVALID;
  }
  if (!(rule->tol_mean >= 0.0) || !(rule->tol_sd >= 0.0)) {  // (a NaN fails the comparison too)
    snprintf(msg, len, "tol_mean = %g, tol_sd = %g: tolerances of at least 0", rule->tol_mean, rule->tol_sd);
    return MCX_ERR_INVALID;
  }
  if (!(rule->ref_frac > 0.0 && rule->ref_frac <= 1.0)) {
    snprintf(msg, len, "ref_frac = %g: a share of the steps in (0, 1]", rule->ref_frac);
    return MCX_ERR_INVALID;
  }
  int nuse = 0;
  for (int c = 0; c < ncol; ++c) nuse += !rule->use_col || rule->use_col[c];
  if (nuse == 0) {
    snprintf(msg, len, "use_col names none of the %d columns", ncol);
    return MCX_ERR_INVALID;
  }
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  const int R = window_steps(T, rule->ref_frac);
  int last = -1;
  bool usable = true;
  for (int c = 0; c < ncol; ++c) {
    mcx_step_settle_col &o = out_cols[c];
    o.m_ref = o.s_ref = o.max_dev_mean = o.max_dev_sd = qnan;
    o.last_out = -1;
    o.reserved = 0;
    if (rule->use_col && !rule->use_col[c]) continue;
    auto at = [&](int t) -> const mcx_step_col & { return cols[(size_t)t * ncol + c]; };
    double sm = 0.0, sv = 0.0;
    for (int t = T - R; t < T; ++t) {
      sm += at(t).mean;
      sv += at(t).sd * at(t).sd;
    }
    const double m_ref = sm / (double)R, s_ref = std::sqrt(sv / (double)R);
    o.m_ref = m_ref;
    o.s_ref = s_ref;
    const bool scaled = std::isfinite(m_ref) && std::isfinite(s_ref) && s_ref > 0.0;
    if (!scaled) usable = false;
    double dm = 0.0, ds = 0.0;
    for (int t = 0; t < T; ++t) {
      const double mean = at(t).mean, sd = at(t).sd;
      const bool fin = std::isfinite(mean) && std::isfinite(sd);
      const double am = std::fabs(mean - m_ref), as = std::fabs(sd - s_ref);
      // (written so that a NaN on either side is out of band)
      const bool in = fin && am <= rule->tol_mean * s_ref && as <= rule->tol_sd * s_ref;
      if (!in) o.last_out = t;
      if (fin && scaled) {
        if (am / s_ref > dm) dm = am / s_ref;
        if (as / s_ref > ds) ds = as / s_ref;
      }
    }
    if (scaled) {
      o.max_dev_mean = dm;
      o.max_dev_sd = ds;
    }
    if (o.last_out > last) last = o.last_out;
  }
  *settled_step = !usable ? -1 : last < 0 ? 0 : last + 1 > T - R ? -1 : last + 1;
  return MCX_OK;
}

}  // namespace mcx_steptable_host
