// mcx_profile_host.hpp -- the host half of mcx_*_profile and mcx_*_profile2d: the order of log L as an
// integer key, the checks of a spec, the grid of a column, and what is made of the swept keys and counts: the curve, its
// least concave majorant, the intervals at a drop of log L, the cells of a pair above a level.  No HIP and no library state:
// tests/cpp/profile_host_check.cc compiles it alone.  The product path (mcx_profile.hip) calls exactly these functions, and
// mcx_debug_profile_finish / mcx_profile_interval expose them.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "mcx_ppnd16.hpp"

namespace mcx_profile_host {

constexpr int N_MIN = 2, N_MAX = 512;      // bins of a column
constexpr int G_MIN = 8, G_MAX = 64;       // nodes per axis of a pair
constexpr int MAX_LEVELS = 8, MAX_PAIRS = 1024;
constexpr double DEFAULT_LEVELS[2] = {0.6827, 0.9545};
// flags (include/mcx.h: MCX_SUMMARY_NONFINITE = 1 and MCX_PROFILE_*)
constexpr int F_NONFINITE = 1, F_LL_NONFINITE = 2, F_OPEN_LO = 4, F_OPEN_HI = 8, F_NO_BIN = 16, F_HULL_OPEN_LO = 32, F_HULL_OPEN_HI = 64;
// codes (include/mcx.h: MCX_OK, MCX_ERR_INVALID, MCX_ERR_UNSUPPORTED)
constexpr int OK = 0, INVALID = 1, UNSUPPORTED = 4;

// ---- the order of log L: section 9's float order as a u32, a NaN counted as -inf ------------------------------------------
inline uint32_t float_bits(float f)
{
  uint32_t b;
  static_assert(sizeof b == sizeof f, "a float is 32 bits");
  __builtin_memcpy(&b, &f, sizeof b);
  return b;
}
inline float bits_float(uint32_t b)
{
  float f;
  __builtin_memcpy(&f, &b, sizeof f);
  return f;
}
inline uint32_t ll_key(float l)
{
  uint32_t b = l != l ? 0xFF800000u : float_bits(l);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
inline float key_ll(uint32_t k) { return bits_float((k & 0x80000000u) ? k ^ 0x80000000u : ~k); }
// K(r) = k(l_r) << 32 | (0xFFFFFFFF - r): the maximum is the largest log L, the first row on ties; 0 is "empty"
inline uint64_t row_key(float l, uint64_t r) { return ((uint64_t)ll_key(l) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)r); }
inline long long key_row(uint64_t K) { return K ? (long long)(0xFFFFFFFFu - (uint32_t)(K & 0xFFFFFFFFu)) : -1; }
inline float key_lmax(uint64_t K) { return K ? key_ll((uint32_t)(K >> 32)) : -std::numeric_limits<float>::infinity(); }

// ---- levels ---------------------------------------------------------------------------------------------------------------
// one parameter: half the chi-square quantile of one degree of freedom; two: half that of two, which is exact
inline double drop_of_level_1d(double p)
{
  const double z = mcx_ppnd16((1.0 + p) / 2.0);
  return 0.5 * (z * z);
}
inline double drop_of_level_2d(double p) { return -std::log(1.0 - p); }

struct Levels {
  int n = 0;
  double p[MAX_LEVELS], drop[MAX_LEVELS];  // p is NaN where the spec gave drops
};

// nlevels = 0 or levels = NULL: the two defaults.  INVALID with a message otherwise for a bad count or entry
inline int levels_of(int nlevels, const double *levels, int are_drops, bool two_d, Levels &out, std::string &why)
{
  char buf[160];
  if (nlevels < 0 || nlevels > MAX_LEVELS) {
    std::snprintf(buf, sizeof buf, "nlevels = %d: 0 (the defaults) to %d levels", nlevels, MAX_LEVELS);
    why = buf;
    return INVALID;
  }
  if (nlevels > 0 && !levels) {
    why = "levels is NULL with nlevels > 0";
    return INVALID;
  }
  if (nlevels == 0) {
    nlevels = 2;
    levels = DEFAULT_LEVELS;
    are_drops = 0;
  }
  out.n = nlevels;
  for (int i = 0; i < nlevels; ++i) {
    const double v = levels[i];
    if (are_drops) {
      if (!(v > 0.0) || !std::isfinite(v)) {
        std::snprintf(buf, sizeof buf, "levels[%d] = %g is not a positive finite drop of log L", i, v);
        why = buf;
        return INVALID;
      }
      out.p[i] = std::numeric_limits<double>::quiet_NaN();
      out.drop[i] = v;
    } else {
      if (!(v > 0.0 && v < 1.0)) {
        std::snprintf(buf, sizeof buf, "levels[%d] = %g is not a confidence level in (0, 1)", i, v);
        why = buf;
        return INVALID;
      }
      out.p[i] = v;
      out.drop[i] = two_d ? drop_of_level_2d(v) : drop_of_level_1d(v);
    }
  }
  return OK;
}

// ---- what a spec is refused for before a device is touched ----------------------------------------------------------------
inline bool given(const double *a, int c) { return a && !std::isnan(a[c]); }
inline bool clipped(double clip_lo, double clip_hi) { return !(clip_lo == 0.0 && clip_hi == 1.0); }

// bins: n of a profile, g of a pair profile; ncol: the profiled columns; N: rows
inline int spec_check(int bins, int bins_min, int bins_max, double clip_lo, double clip_hi, const double *from, const double *to, int ncol,
                      long long N, std::string &why)
{
  char buf[200];
  if (bins < bins_min || bins > bins_max) {
    std::snprintf(buf, sizeof buf, "%d bins per column: %d to %d", bins, bins_min, bins_max);
    why = buf;
    return INVALID;
  }
  if (clipped(clip_lo, clip_hi) && !(clip_lo >= 0.0 && clip_lo < clip_hi && clip_hi <= 1.0)) {
    std::snprintf(buf, sizeof buf, "clip = (%g, %g): 0 <= clip_lo < clip_hi <= 1", clip_lo, clip_hi);
    why = buf;
    return INVALID;
  }
  for (int c = 0; c < ncol; ++c) {
    if ((given(from, c) && !std::isfinite(from[c])) || (given(to, c) && !std::isfinite(to[c]))) {
      std::snprintf(buf, sizeof buf, "from[%d] or to[%d] is infinite", c, c);
      why = buf;
      return INVALID;
    }
    if (given(from, c) && given(to, c) && from[c] > to[c]) {
      std::snprintf(buf, sizeof buf, "from[%d] = %g is above to[%d] = %g", c, from[c], c, to[c]);
      why = buf;
      return INVALID;
    }
  }
  if (N < 2) {
    std::snprintf(buf, sizeof buf, "a profile needs nsteps * nc >= 2 rows, got %lld", N);
    why = buf;
    return INVALID;
  }
  if (N >= (1ll << 32)) {
    std::snprintf(buf, sizeof buf, "a profile of %lld rows: fewer than 2^32 (the row index is half of a key)", N);
    why = buf;
    return UNSUPPORTED;
  }
  return OK;
}

// the pairs of a call: the spec's, or every a < b in ascending order (section 15's rules over the profiled columns)
inline int pair_list(int npairs, const int *pairs, int ncol, std::vector<int> &out, std::string &why)
{
  char buf[200];
  out.clear();
  if (!pairs) {
    const long long all = (long long)ncol * (ncol - 1) / 2;
    if (all > MAX_PAIRS) {
      std::snprintf(buf, sizeof buf, "%d columns have %lld pairs, more than %d: name the pairs", ncol, all, MAX_PAIRS);
      why = buf;
      return INVALID;
    }
    for (int a = 0; a < ncol; ++a)
      for (int b = a + 1; b < ncol; ++b) {
        out.push_back(a);
        out.push_back(b);
      }
    if (out.empty()) {
      why = "one column has no pair";
      return INVALID;
    }
    return OK;
  }
  if (npairs < 1 || npairs > MAX_PAIRS) {
    std::snprintf(buf, sizeof buf, "npairs = %d: 1 to %d pairs", npairs, MAX_PAIRS);
    why = buf;
    return INVALID;
  }
  for (int p = 0; p < npairs; ++p) {
    const int a = pairs[2 * p], b = pairs[2 * p + 1];
    if (a < 0 || a >= ncol || b < 0 || b >= ncol || a == b) {
      std::snprintf(buf, sizeof buf, "pair %d = (%d, %d): two different columns of 0 to %d", p, a, b, ncol - 1);
      why = buf;
      return INVALID;
    }
    out.push_back(a);
    out.push_back(b);
  }
  return OK;
}

// ---- the grid of a column -------------------------------------------------------------------------------------------------
struct Grid {
  double from, to, inv;
};
// from / to: min / max, the clip pair's quantiles when clipped, the spec's finite entries over both; inv = bins / (to - from)
// (+inf when to == from: the sweep puts the values equal to it into bin 0).  INVALID when that is no finite range
inline int grid_of(int col, int bins, float mn, float mx, bool clip, double qlo, double qhi, const double *sfrom, const double *sto, Grid &g,
                   std::string &why)
{
  double from = (double)mn, to = (double)mx;
  if (clip) {
    from = qlo;
    to = qhi;
  }
  if (given(sfrom, col)) from = sfrom[col];
  if (given(sto, col)) to = sto[col];
  if (!std::isfinite(from) || !std::isfinite(to) || !(from <= to) || !std::isfinite(to - from)) {
    char buf[200];
    std::snprintf(buf, sizeof buf, "column %d: from = %g and to = %g are not a finite range", col, from, to);
    why = buf;
    return INVALID;
  }
  g.from = from;
  g.to = to;
  g.inv = (double)bins / (to - from);
  return OK;
}
// the bin of a value, -1 for a dropped one: what the sweep computes, for the restatements of the tests
inline int bin_of(float v, const Grid &g, int bins)
{
  const double d = (double)v, xp = (d - g.from) * g.inv;
  if (d == g.to) return g.from == g.to ? 0 : bins - 1;
  if (xp >= 0.0 && xp < (double)bins) return (int)xp;
  return -1;
}

// ---- the curve, the hull, the intervals -----------------------------------------------------------------------------------
// pl[j] = lmax[j] - lhat in fp64: -inf for an empty bin (row < 0), NaN everywhere when lhat is not finite
inline void curve(int n, const float *lmax, const long long *row, float lhat, double *pl)
{
  const double qnan = std::numeric_limits<double>::quiet_NaN(), ninf = -std::numeric_limits<double>::infinity();
  const bool bad = !std::isfinite(lhat);
  for (int j = 0; j < n; ++j) pl[j] = bad ? qnan : row[j] < 0 ? ninf : (double)lmax[j] - (double)lhat;
}

// plh: the least concave majorant of the points (x[j], y[j]) of the non-empty bins (x[j] not NaN) with y[j] > -inf, evaluated
// at x[j]: Andrew's monotone chain from left to right, a point popped on a cross product >= 0.  NaN for an empty bin; a
// non-empty bin at -inf takes no part and keeps -inf.  x ascends over the non-empty bins
inline void hull(int n, const double *x, const double *y, double *plh)
{
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  std::vector<int> h;
  for (int j = 0; j < n; ++j) {
    plh[j] = qnan;
    if (std::isnan(x[j])) continue;
    plh[j] = y[j];
    if (!std::isfinite(y[j])) continue;
    while (h.size() >= 2) {
      const int o = h[h.size() - 2], a = h[h.size() - 1];
      const double cr = (x[a] - x[o]) * (y[j] - y[o]) - (y[a] - y[o]) * (x[j] - x[o]);
      if (cr >= 0.0) h.pop_back();
      else break;
    }
    h.push_back(j);
  }
  for (size_t i = 0; i + 1 < h.size(); ++i) {
    const int a = h[i], b = h[i + 1];
    for (int j = a + 1; j < b; ++j)
      if (!std::isnan(x[j]) && std::isfinite(y[j])) {
        const double chord = y[a] + (y[b] - y[a]) * ((x[j] - x[a]) / (x[b] - x[a]));
        plh[j] = chord > y[j] ? chord : y[j];  // (a popped collinear point: the chord may round below it)
      }
  }
}

struct Ends {
  double lo, hi;
  int nseg, open;  // open: bit 0 the lower end, bit 1 the upper end, bit 2 no bin reaches the level
};
// The outermost interval of the curve y over the non-empty bins (x[j] not NaN) at y >= -drop: jl / jh the first / last such
// bin; an end is the linear interpolation at -drop towards the nearest non-empty bin outside (that bin at -inf: the end is
// x[jl] / x[jh] itself), and x[jl] / x[jh] with `open` set when there is none.  nseg: the maximal runs of non-empty bins with
// y >= -drop.  A NaN in y (lhat not finite) gives NaN ends, nseg = 0 and open = 0
inline Ends interval(int n, const double *x, const double *y, double drop)
{
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  Ends e{qnan, qnan, 0, 0};
  int jl = -1, jh = -1;
  bool in = false;
  for (int j = 0; j < n; ++j) {
    if (std::isnan(x[j])) continue;
    if (std::isnan(y[j])) return Ends{qnan, qnan, 0, 0};
    if (y[j] >= -drop) {
      if (jl < 0) jl = j;
      jh = j;
      if (!in) ++e.nseg;
      in = true;
    } else {
      in = false;
    }
  }
  if (jl < 0) {
    e.open = 4;
    return e;
  }
  auto cross = [&](int jin, int jout) {
    if (y[jout] == -std::numeric_limits<double>::infinity()) return x[jin];
    const double t = (-drop - y[jout]) / (y[jin] - y[jout]);
    return x[jout] + (x[jin] - x[jout]) * t;
  };
  int b = jl - 1;
  while (b >= 0 && std::isnan(x[b])) --b;
  if (b < 0) {
    e.lo = x[jl];
    e.open |= 1;
  } else {
    e.lo = cross(jl, b);
  }
  int a = jh + 1;
  while (a < n && std::isnan(x[a])) ++a;
  if (a >= n) {
    e.hi = x[jh];
    e.open |= 2;
  } else {
    e.hi = cross(jh, a);
  }
  return e;
}

// one level of one column: the raw curve and the hull
struct Interval {
  double p, drop, lo, hi, lo_hull, hi_hull;
  int nseg, flags;
};
inline Interval interval_of(int n, const double *x, const double *pl, const double *plh, double p, double drop)
{
  const Ends r = interval(n, x, pl, drop), h = interval(n, x, plh, drop);
  Interval o{p, drop, r.lo, r.hi, h.lo, h.hi, r.nseg, 0};
  if (r.open & 1) o.flags |= F_OPEN_LO;
  if (r.open & 2) o.flags |= F_OPEN_HI;
  if (r.open & 4) o.flags |= F_NO_BIN;
  if (h.open & 1) o.flags |= F_HULL_OPEN_LO;
  if (h.open & 2) o.flags |= F_HULL_OPEN_HI;
  return o;
}

// ---- one column from its swept keys and counts ----------------------------------------------------------------------------
// keys[n], cnt[n], xat[n] (the column's value in the row of each key; not read for an empty bin), hat = the maximum key of all
// rows -> lmax, row, x (xat as fp64, NaN for an empty bin), pl, plh [n], iv[lv.n]; nbinned, nempty.  Returns the column's
// flags: 0 or F_LL_NONFINITE
inline int finish_column(int n, const uint64_t *keys, const uint64_t *cnt, const float *xat, uint64_t hat, const Levels &lv, float *lmax,
                         long long *row, double *x, double *pl, double *plh, Interval *iv, long long *nbinned, int *nempty)
{
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  long long nb = 0;
  int ne = 0;
  for (int j = 0; j < n; ++j) {
    lmax[j] = key_lmax(keys[j]);
    row[j] = key_row(keys[j]);
    x[j] = keys[j] ? (double)xat[j] : qnan;
    nb += (long long)cnt[j];
    ne += keys[j] ? 0 : 1;
  }
  const float lhat = key_lmax(hat);
  curve(n, lmax, row, lhat, pl);
  const bool bad = !std::isfinite(lhat);
  if (bad)
    for (int j = 0; j < n; ++j) plh[j] = qnan;
  else
    hull(n, x, pl, plh);
  for (int i = 0; i < lv.n; ++i) iv[i] = interval_of(n, x, pl, plh, lv.p[i], lv.drop[i]);
  *nbinned = nb;
  *nempty = ne;
  return bad ? F_LL_NONFINITE : 0;
}

// ---- one pair from its swept keys -----------------------------------------------------------------------------------------
// keys[g * g] -> lmax, row, z = lmax - lhat (-inf for an empty cell, NaN when lhat is not finite); nlevel[lv.n]: the non-empty
// cells with z >= -drop
inline void finish_pair(int g, const uint64_t *keys, const uint64_t *cnt, uint64_t hat, const Levels &lv, float *lmax, long long *row,
                        double *z, long long *nlevel, long long *nbinned, int *nempty)
{
  const int gg = g * g;
  long long nb = 0;
  int ne = 0;
  for (int i = 0; i < gg; ++i) {
    lmax[i] = key_lmax(keys[i]);
    row[i] = key_row(keys[i]);
    nb += (long long)cnt[i];
    ne += keys[i] ? 0 : 1;
  }
  curve(gg, lmax, row, key_lmax(hat), z);
  for (int l = 0; l < lv.n; ++l) {
    long long c = 0;
    for (int i = 0; i < gg; ++i) c += (keys[i] && z[i] >= -lv.drop[l]) ? 1 : 0;
    nlevel[l] = c;
  }
  *nbinned = nb;
  *nempty = ne;
}

}  // namespace mcx_profile_host
