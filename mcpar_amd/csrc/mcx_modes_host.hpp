// mcx_modes_host.hpp -- the host half of the modes of a store: what a call refuses, the scale, the
// k-means++ seeding on a sample of rows, the centre update of a Lloyd pass and the finish of the mode table.  Plain C++ in fp64
// and integers, no HIP and no library state: mcx_modes.hip calls these very functions, and a host-only program can include
// this header alone.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

namespace mcx_modes_host {

// Philox stream of the seeding.  The step kernels use streams 0-4, the draws of section 12 stream 5 and the permutations of
// section 21 stream 6; the constant lives here because no other unit has any business with it
constexpr uint32_t ST_MODES = 7;
constexpr int MAX_K = 32;          // MCX_MODES_MAX_K
constexpr int NONE = 255;          // MCX_MODE_NONE
constexpr int F_CONVERGED = 1, F_NOT_CONVERGED = 2, F_EMPTY = 4;  // MCX_MODES_*
constexpr int OK = 0, ERR_INVALID = 1;  // MCX_OK, MCX_ERR_INVALID

// Philox4x32-10 as mcx_numerics.hpp has it, restated without HIP: words x and y of the block
inline void philox_xy(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t *x, uint32_t *y)
{
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * (uint64_t)c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * (uint64_t)c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  *x = c0;
  *y = c1;
}

// the uniform of centre k: the top 53 bits of words x : y of block (k, 0, 0, 0), in [0, 1)
inline double seed_uniform(uint32_t seed, int k)
{
  uint32_t x, y;
  philox_xy((uint32_t)k, 0u, 0u, 0u, seed, ST_MODES, &x, &y);
  const uint64_t r = ((uint64_t)x << 32) | (uint64_t)y;
  return (double)(r >> 11) * 0x1p-53;
}

// what every call refuses before a device is touched; centres: NULL or [k][np], unscaled
inline int spec_check(int k, int max_iter, int seed_rows, const double *centres, int np, long long N, char *msg, size_t len)
{
  if (k < 1 || k > MAX_K) {
    snprintf(msg, len, "k = %d: 1 to %d modes", k, MAX_K);
    return ERR_INVALID;
  }
  if (max_iter < 1) {
    snprintf(msg, len, "max_iter = %d: at least one pass", max_iter);
    return ERR_INVALID;
  }
  if (seed_rows < 1) {
    snprintf(msg, len, "seed_rows = %d: a seed sample of at least one row", seed_rows);
    return ERR_INVALID;
  }
  if ((long long)k > N) {
    snprintf(msg, len, "k = %d modes of %lld rows", k, N);
    return ERR_INVALID;
  }
  if (centres)
    for (int i = 0; i < k; ++i)
      for (int j = 0; j < np; ++j)
        if (!std::isfinite(centres[(size_t)i * np + j])) {
          snprintf(msg, len, "centres[%d][%d] is not finite", i, j);
          return ERR_INVALID;
        }
  return OK;
}

// s_j of a column of standard deviation sd: 1 / sd, 0 where sd is 0 or not finite (or too small for 1 / sd to be finite)
inline double scale_of_sd(double sd)
{
  if (!(sd > 0.0) || !std::isfinite(sd)) return 0.0;
  const double s = 1.0 / sd;
  return std::isfinite(s) ? s : 0.0;
}

inline bool row_finite(const float *x, int np)
{
  for (int j = 0; j < np; ++j)
    if (!std::isfinite(x[j])) return false;
  return true;
}

// d^2 of row x from centre c (scaled): over j in order e = u - c, acc = acc + e e, every operation rounded on its own (this
// header is built without contraction; the volatile keeps a compiler that contracts anyway from fusing them)
inline double dist2(const float *x, const double *s, const double *c, int np)
{
  double acc = 0.0;
  for (int j = 0; j < np; ++j) {
    if (s[j] == 0.0) continue;
    const double u = (double)x[j] * s[j];
    const double e = u - c[j];
    volatile double ee = e * e;
    acc = acc + ee;
  }
  return acc;
}

// k-means++ on rows[M][np + 1] (MCout layout: the parameters, then log L) with the scale s[np]: index[k] of the K seed rows.
//   centre 0: the row of the largest log L (first on ties; a NaN log L counts as -inf) among the rows whose parameters are
//             all finite
//   centre k: D_i = the least d^2 of row i from centres 0 .. k - 1 (0 for a row that is not finite), cum_i their running
//             sum in index order in fp64, total = cum_{M-1}; the first i with cum_i > u total, u = seed_uniform(seed, k).
//             total = 0 (every row sits on a centre): the first finite row not yet taken.
// MCX_ERR_INVALID when fewer than K rows are finite
inline int seed(const float *rows, long long M, int np, int K, uint32_t seed_, const double *s, long long *index, char *msg,
                size_t len)
{
  const size_t ncol = (size_t)np + 1;
  std::vector<uint8_t> ok((size_t)M);
  long long nvalid = 0, best = -1;
  const double ninf = -std::numeric_limits<double>::infinity();
  double bestll = 0.0;
  for (long long i = 0; i < M; ++i) {
    const float *x = rows + (size_t)i * ncol;
    ok[(size_t)i] = row_finite(x, np) ? 1 : 0;
    if (!ok[(size_t)i]) continue;
    ++nvalid;
    const double ll = std::isnan(x[np]) ? ninf : (double)x[np];
    if (best < 0 || ll > bestll) {
      best = i;
      bestll = ll;
    }
  }
  if (nvalid < (long long)K) {
    snprintf(msg, len, "k = %d modes, but the seed sample of %lld rows has %lld rows with finite parameters", K, M, nvalid);
    return ERR_INVALID;
  }
  index[0] = best;
  std::vector<double> D((size_t)M, std::numeric_limits<double>::infinity()), c((size_t)np);
  std::vector<uint8_t> taken((size_t)M, 0);
  taken[(size_t)best] = 1;
  for (int k = 1; k < K; ++k) {
    const float *xc = rows + (size_t)index[k - 1] * ncol;
    for (int j = 0; j < np; ++j) c[(size_t)j] = (double)xc[j] * s[j];
    double total = 0.0;
    for (long long i = 0; i < M; ++i) {
      if (!ok[(size_t)i]) {
        D[(size_t)i] = 0.0;
        continue;
      }
      const double d = dist2(rows + (size_t)i * ncol, s, c.data(), np);
      if (d < D[(size_t)i]) D[(size_t)i] = d;
      total = total + D[(size_t)i];
    }
    long long pick = -1;
    if (total > 0.0 && std::isfinite(total)) {
      const double target = seed_uniform(seed_, k) * total;
      double cum = 0.0;
      long long last = -1;
      for (long long i = 0; i < M && pick < 0; ++i) {
        cum = cum + D[(size_t)i];
        if (D[(size_t)i] > 0.0) last = i;
        if (cum > target) pick = i;
      }
      if (pick < 0) pick = last;  // (u total rounded up to total)
    }
    if (pick < 0 || taken[(size_t)pick])
      for (long long i = 0; i < M; ++i)
        if (ok[(size_t)i] && !taken[(size_t)i]) {
          pick = i;
          break;
        }
    index[k] = pick;
    taken[(size_t)pick] = 1;
  }
  return OK;
}

// the centre update of a Lloyd pass: c_k <- S_k / n_k; a cluster without rows keeps its centre.  Returns F_EMPTY or 0
inline int update_centres(int K, int np, const long long *n, const double *S, double *c)
{
  int flags = 0;
  for (int k = 0; k < K; ++k) {
    if (n[k] == 0) {
      flags |= F_EMPTY;
      continue;
    }
    for (int j = 0; j < np; ++j) c[(size_t)k * np + j] = S[(size_t)k * np + j] / (double)n[k];
  }
  return flags;
}

// scaled [K][np] -> unscaled: v / s_j, NaN in a column that takes no part (s_j = 0)
inline void unscale(int K, int np, const double *s, const double *v, double *out)
{
  for (int k = 0; k < K; ++k)
    for (int j = 0; j < np; ++j)
      out[(size_t)k * np + j] = s[j] == 0.0 ? std::numeric_limits<double>::quiet_NaN() : v[(size_t)k * np + j] / s[j];
}

// ascending in float order: -inf < finite < +inf, -0 before +0 (section 9's key)
inline uint32_t order_key(uint32_t b) { return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u); }
inline uint32_t order_key_inverse(uint32_t k) { return k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu); }

// The best log L of a mode from what every workgroup found: words[2 w] = 1 << 32 | the order key of its best (0: it saw no
// member), words[2 w + 1] = the first source row that holds it.  The largest key, then the smallest row.  false: no member
inline bool best_ll(const unsigned long long *words, size_t nwg, size_t stride, uint32_t *bits, long long *row)
{
  unsigned long long bk = 0, br = 0;
  for (size_t w = 0; w < nwg; ++w) {
    const unsigned long long k = words[w * stride], r = words[w * stride + 1];
    if (k == 0) continue;
    if (bk == 0 || k > bk || (k == bk && r < br)) {
      bk = k;
      br = r;
    }
  }
  if (bk == 0) return false;
  *bits = order_key_inverse((uint32_t)bk);
  *row = (long long)br;
  return true;
}

}  // namespace mcx_modes_host
