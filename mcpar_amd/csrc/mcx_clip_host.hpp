// mcx_clip_host.hpp -- the host half of the tail clip: the checks of an mcx_clip_spec and the rule that
// turns a column's (qlo, qhi) quantiles and the spec into its thresholds.  Plain C++ over include/mcx.h, no HIP and no
// library state: mcx_clip.hip calls these very functions (mcx_debug_clip_thresholds is thresholds() behind the library's
// error text), and tests/cpp/clip_thresholds_check.cc compiles them on their own under a sanitizer.
#pragma once
#include "../../include/mcx.h"

#include <cmath>
#include <cstddef>
#include <cstdio>

namespace mcx_clip_host {

inline bool given(const double *a, int c) { return a && !std::isnan(a[c]); }

// MCX_OK, or MCX_ERR_INVALID with the reason in msg[len]: what a clip call refuses before a device is touched
inline int spec_check(const mcx_clip_spec *s, const void *cols, const void *nkept, char *msg, size_t len)
{
  if (!s) {
    snprintf(msg, len, "the clip spec is NULL");
    return MCX_ERR_INVALID;
  }
  if (!cols || !nkept) {
    snprintf(msg, len, "cols or nkept is NULL");
    return MCX_ERR_INVALID;
  }
  if (!(s->qlo >= 0.0 && s->qlo < s->qhi && s->qhi <= 1.0)) {
    snprintf(msg, len, "clip = (%g, %g): 0 <= qlo < qhi <= 1", s->qlo, s->qhi);
    return MCX_ERR_INVALID;
  }
  return MCX_OK;
}

// does some column take a bound from its quantiles?  (No: the quantile pass does not run.)
inline bool needs_quantiles(const mcx_clip_spec *s, int ncol)
{
  for (int c = 0; c < ncol; ++c) {
    if (!given(s->lo, c)) return true;
    if (!given(s->hi, c) && !(c == ncol - 1 && !std::isnan(s->ll_hi))) return true;
  }
  return false;
}

// lo[ncol], hi[ncol] from q[ncol][2] = the (qlo, qhi) quantiles (NULL: every one NaN).  Column c: (q[c][0], q[c][1]); the
// last column's upper threshold is ll_hi unless that is NaN; a non-NaN spec->lo[c] / spec->hi[c] replaces either
inline int thresholds(int ncol, const double *q, const mcx_clip_spec *s, double *lo, double *hi, char *msg, size_t len)
{
  if (ncol < 1 || !s || !lo || !hi) {
    snprintf(msg, len, "ncol = %d, or the clip spec, lo or hi is NULL", ncol);
    return MCX_ERR_INVALID;
  }
  for (int c = 0; c < ncol; ++c) {
    double l = q ? q[2 * c] : std::nan(""), h = q ? q[2 * c + 1] : std::nan("");
    if (c == ncol - 1 && !std::isnan(s->ll_hi)) h = s->ll_hi;
    if (given(s->lo, c)) l = s->lo[c];
    if (given(s->hi, c)) h = s->hi[c];
    lo[c] = l;
    hi[c] = h;
  }
  return MCX_OK;
}

}  // namespace mcx_clip_host
