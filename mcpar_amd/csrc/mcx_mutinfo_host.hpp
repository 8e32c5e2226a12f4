// mcx_mutinfo_host.hpp -- the host half of the mutual information between columns of a store: which
// rows are taken, the scale and flags of the columns, the repeated rows dropped, z, the permutations of the null, the digamma
// table and what turns the device's sums into the estimate.  Plain C++ in fp64 and integers, no HIP and no library state:
// mcx_mutinfo.hip calls these very functions, and a host-only program can include this header alone.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <unordered_map>
#include <vector>

namespace mcx_mutinfo_host {

// Philox stream of the permutations.  Streams 0-8 are taken (the step kernels, section 12's draws, ST_ENERGY, ST_MODES,
// ST_EVIDENCE); the constant lives here because no step kernel has any business with it
constexpr uint32_t ST_MUTINFO = 9;

// include/mcx.h's flags, restated so that the header stands alone (mcx_mutinfo.hip asserts that they agree)
enum { COL_NONFINITE = 1, COL_CONSTANT = 2, COL_UNUSED = 4 };
enum { PAIR_UNUSED = 1, PAIR_FEW = 2, PAIR_TIES = 4 };

// Euler's constant, one literal
constexpr double EULER_GAMMA = 0.57721566490153286060651209008240243;

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

// (r m) >> 64 for m < 2^32: the high word of a 64 x 32 bit product, in 64-bit pieces
inline uint64_t mulhi_64x32(uint64_t r, uint64_t m)
{
  const uint64_t lo = (r & 0xffffffffull) * m, hi = (r >> 32) * m;
  return (hi + (lo >> 32)) >> 32;
}

// selected row i of n among N: floor(i N / n), evenly spaced in store order.  i < n <= 2^14 and N < 2^49: the product fits
inline int64_t row_index(int64_t N, int64_t n, int64_t i) { return (int64_t)(((uint64_t)i * (uint64_t)N) / (uint64_t)n); }

// pi_p on [0, m): p = 0 the identity; p >= 1 a full Fisher-Yates -- for i = 0 ... m - 2, w = philox(counter (i, p, 0, 0),
// key (seed, ST_MUTINFO)), r = w.x : w.y, j = i + ((r (m - i)) >> 64), swap
template <class T> inline void permutation(uint32_t seed, int m, int p, T *out)
{
  for (int i = 0; i < m; ++i) out[i] = (T)i;
  if (p == 0) return;
  for (int i = 0; i + 1 < m; ++i) {
    uint32_t x, y;
    philox_xy((uint32_t)i, (uint32_t)p, 0u, 0u, seed, ST_MUTINFO, &x, &y);
    const uint64_t r = ((uint64_t)x << 32) | (uint64_t)y;
    const int j = i + (int)mulhi_64x32(r, (uint64_t)(m - i));
    const T t = out[i];
    out[i] = out[j];
    out[j] = t;
  }
}

// table[q] = psi(q + 1) = H_q - gamma, q = 0 ... n - 1: H_0 = 0, H_q = H_{q - 1} + 1 / q in index order
inline void psi_table(int n, double *table)
{
  double h = 0.0;
  for (int q = 0; q < n; ++q) {
    if (q > 0) h += 1.0 / (double)q;
    table[q] = h - EULER_GAMMA;
  }
}

// the scale of one column over n rows of stride ncol: fp64, centred two-pass, divisor n - 1.  *finite = every value is
inline double column_scale(const float *col, size_t n, size_t stride, bool *finite)
{
  double s = 0.0;
  *finite = true;
  for (size_t i = 0; i < n; ++i) {
    const double v = (double)col[i * stride];
    if (!std::isfinite(v)) *finite = false;
    s += v;
  }
  if (!*finite) return std::numeric_limits<double>::quiet_NaN();
  const double mean = s / (double)n;
  double q = 0.0;
  for (size_t i = 0; i < n; ++i) {
    const double t = (double)col[i * stride] - mean;
    q += t * t;
  }
  return std::sqrt(q / (double)(n - 1));
}

// What the host makes of the n selected rows sel[n][ncol] (MCout layout, selection order): scale and flags of every column,
// kept[n] (0: an earlier selected row equals this one, float ==, in every column without a flag), the m kept rows' z,
// column-major z[c][m] for every column (a flagged column's stretch is left 0)
struct Points {
  std::vector<double> scale;
  std::vector<int> flags;
  std::vector<uint8_t> kept;
  std::vector<double> z;
  int m = 0, ndup = 0, nused = 0;
};
inline void points(const float *sel, int n, int ncol, bool with_ll, bool raw, Points &P)
{
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  P.scale.assign((size_t)ncol, qnan);
  P.flags.assign((size_t)ncol, 0);
  std::vector<int> used;
  for (int c = 0; c < ncol; ++c) {
    if (c == ncol - 1 && !with_ll) {
      P.flags[(size_t)c] = COL_UNUSED;
      continue;
    }
    bool finite = true;
    const double sd = column_scale(sel + c, (size_t)n, (size_t)ncol, &finite);
    P.scale[(size_t)c] = !finite ? qnan : raw ? 1.0 : sd;
    if (!finite) P.flags[(size_t)c] = COL_NONFINITE;
    else if (!raw && !(sd > 0.0)) P.flags[(size_t)c] = COL_CONSTANT;
    if (!P.flags[(size_t)c]) used.push_back(c);
  }
  P.nused = (int)used.size();
  // repeated rows: a hash of the used values (-0 as +0, so that == rows meet in one bucket), then == on the bucket's rows
  P.kept.assign((size_t)n, (uint8_t)1);
  P.ndup = 0;
  if (!used.empty()) {
    std::unordered_map<uint64_t, std::vector<int>> seen;
    seen.reserve((size_t)n * 2);
    for (int i = 0; i < n; ++i) {
      const float *r = sel + (size_t)i * ncol;
      uint64_t h = 1469598103934665603ull;
      for (int c : used) {
        const float v = r[c] == 0.0f ? 0.0f : r[c];
        uint32_t b;
        std::memcpy(&b, &v, sizeof b);
        h = (h ^ b) * 1099511628211ull;
      }
      std::vector<int> &bucket = seen[h];
      bool dup = false;
      for (int j : bucket) {
        const float *q = sel + (size_t)j * ncol;
        bool same = true;
        for (int c : used)
          if (!(r[c] == q[c])) {
            same = false;
            break;
          }
        if (same) {
          dup = true;
          break;
        }
      }
      if (dup) {
        P.kept[(size_t)i] = 0;
        ++P.ndup;
      } else
        bucket.push_back(i);
    }
  }
  P.m = n - P.ndup;
  P.z.assign((size_t)ncol * (size_t)P.m, 0.0);
  for (int c : used) {
    double *zc = P.z.data() + (size_t)c * (size_t)P.m;
    const double s = P.scale[(size_t)c];
    int k = 0;
    for (int i = 0; i < n; ++i)
      if (P.kept[(size_t)i]) zc[k++] = (double)sel[(size_t)i * ncol + c] / s;
  }
}

// mi of one (pair, permutation) from the sum over the m points of psi(na + 1) + psi(nb + 1): three operations
inline double mi_of_sum(double sum, int m, int k, const double *table) { return (table[k - 1] + table[m - 1]) - sum / (double)m; }

// eps, na, nb [m] of one pair -> mi and nzero = #{eps == 0}: the sum in index order, each point's two table values added first.
// table: psi_table(m)
inline double finish_pair(const double *eps, const int *na, const int *nb, int m, int k, const double *table, long long *nzero)
{
  double s = 0.0;
  long long nz = 0;
  for (int i = 0; i < m; ++i) {
    s += table[na[i]] + table[nb[i]];
    if (eps[i] == 0.0) ++nz;
  }
  if (nzero) *nzero = nz;
  return mi_of_sum(s, m, k, table);
}

// Linfoot's coefficient: sqrt(1 - exp(-2 max(mi, 0)))
inline double r_info(double mi) { return std::sqrt(1.0 - std::exp(-2.0 * std::max(mi, 0.0))); }

// Pearson's r of two columns of z over the m points: fp64, centred two-pass (NaN when a column has no spread)
inline double pearson(const double *a, const double *b, int m)
{
  double sa = 0.0, sb = 0.0;
  for (int i = 0; i < m; ++i) {
    sa += a[i];
    sb += b[i];
  }
  const double ma = sa / (double)m, mb = sb / (double)m;
  double qaa = 0.0, qbb = 0.0, qab = 0.0;
  for (int i = 0; i < m; ++i) {
    const double ta = a[i] - ma, tb = b[i] - mb;
    qaa += ta * ta;
    qbb += tb * tb;
    qab += ta * tb;
  }
  const double den = std::sqrt(qaa * qbb);
  return den > 0.0 ? qab / den : std::numeric_limits<double>::quiet_NaN();
}

// the null of one pair from perm[nperm] = mi_1 ... mi_nperm: mean, sd (two-pass, divisor nperm - 1: NaN below 2), nge and
// p_value = (1 + nge) / (1 + nperm); all NaN (nge 0) at nperm = 0 or a NaN mi
struct Null {
  double mean, sd, p_value;
  long long nge;
};
inline Null null_of(double mi, const double *perm, int nperm)
{
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  Null o{qnan, qnan, qnan, 0};
  if (nperm < 1 || std::isnan(mi)) return o;
  double s = 0.0;
  for (int p = 0; p < nperm; ++p) {
    s += perm[p];
    if (perm[p] >= mi) ++o.nge;
  }
  o.mean = s / (double)nperm;
  if (nperm > 1) {
    double q = 0.0;
    for (int p = 0; p < nperm; ++p) {
      const double t = perm[p] - o.mean;
      q += t * t;
    }
    o.sd = std::sqrt(q / (double)(nperm - 1));
  }
  o.p_value = (double)(1 + o.nge) / (double)(1 + nperm);
  return o;
}

}  // namespace mcx_mutinfo_host
