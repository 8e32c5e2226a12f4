// mcx_energy_host.hpp -- the host half of the joint two-store comparison: the label vectors of the
// permutation test and what turns the device's sums into the energy statistic.  Plain C++ in fp64 and integers, no HIP and
// no library state: mcx_energy.hip calls these very functions, and a host-only program can include this header alone.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

namespace mcx_energy_host {

// Philox stream of the permutations.  The step kernels use streams 0-4 and the draws of section 12 stream 5; the constant
// lives here because no step kernel has any business with it
constexpr uint32_t ST_ENERGY = 6;

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

// labels[N] of permutation p among N = n_a + n_b pooled rows, exactly n_a ones.  p = 0: the first n_a rows.  p >= 1: a
// partial Fisher-Yates on idx = [0, N): for i < n_a, w = philox(counter (i, p, 0, 0), key (seed, ST_ENERGY)), r = w.x : w.y,
// j = i + ((r (N - i)) >> 64), swap idx[i] and idx[j], labels[idx[i]] = 1.  idx is the caller's scratch of N words
inline void labels(uint32_t seed, int n_a, int n_b, int p, uint8_t *out, std::vector<uint32_t> &idx)
{
  const int N = n_a + n_b;
  for (int i = 0; i < N; ++i) out[i] = (p == 0 && i < n_a) ? 1 : 0;
  if (p == 0) return;
  idx.resize((size_t)N);
  for (int i = 0; i < N; ++i) idx[(size_t)i] = (uint32_t)i;
  for (int i = 0; i < n_a; ++i) {
    uint32_t x, y;
    philox_xy((uint32_t)i, (uint32_t)p, 0u, 0u, seed, ST_ENERGY, &x, &y);
    const uint64_t r = ((uint64_t)x << 32) | (uint64_t)y;
    const int j = i + (int)mulhi_64x32(r, (uint64_t)(N - i));
    const uint32_t t = idx[(size_t)i];
    idx[(size_t)i] = idx[(size_t)j];
    idx[(size_t)j] = t;
    out[idx[(size_t)i]] = 1;
  }
}

// the three normalised sums of a label vector from S = sum_ij d_ij, S_A = sum_i l_i r_i and S_AA = sum_ij l_i l_j d_ij
struct Means {
  double ab, aa, bb;
};
inline Means means(double S, double SA, double SAA, int n_a, int n_b)
{
  const double na = (double)n_a, nb = (double)n_b;
  const double SAB = SA - SAA, SBB = S - 2.0 * SA + SAA;
  return Means{SAB / (na * nb), SAA / (na * na), SBB / (nb * nb)};
}
// E = 2 S_AB / (n_a n_b) - S_AA / n_a^2 - S_BB / n_b^2
inline double energy(double S, double SA, double SAA, int n_a, int n_b)
{
  const Means m = means(S, SA, SAA, n_a, n_b);
  return 2.0 * m.ab - m.aa - m.bb;
}

struct Finish {
  double e, h, mean_ab, mean_aa, mean_bb, p_value;
  long long nge;
};
// sums[0] = S, then (S_A, S_AA) of l_0 ... l_P; perm_e (may be NULL): E(l_p), p = 1 ... P.  sums == NULL: no column was left,
// every statistic is NaN and nge = 0
inline Finish finish(const double *sums, int n_a, int n_b, int nperm, double *perm_e)
{
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  Finish f{qnan, qnan, qnan, qnan, qnan, qnan, 0};
  if (!sums) {
    if (perm_e)
      for (int p = 0; p < nperm; ++p) perm_e[p] = qnan;
    return f;
  }
  const Means m = means(sums[0], sums[1], sums[2], n_a, n_b);
  f.mean_ab = m.ab;
  f.mean_aa = m.aa;
  f.mean_bb = m.bb;
  f.e = 2.0 * m.ab - m.aa - m.bb;
  f.h = m.ab == 0.0 ? qnan : f.e / (2.0 * m.ab);
  for (int p = 1; p <= nperm; ++p) {
    const double ep = energy(sums[0], sums[1 + 2 * (size_t)p], sums[2 + 2 * (size_t)p], n_a, n_b);
    if (perm_e) perm_e[p - 1] = ep;
    if (ep >= f.e) ++f.nge;
  }
  if (nperm > 0) f.p_value = (double)(1 + f.nge) / (double)(1 + nperm);
  return f;
}

// the pooled scale of one column over N rows of stride ncol: fp64, centred two-pass, divisor N - 1.  *finite = every value is
inline double column_scale(const float *col, size_t N, size_t stride, bool *finite)
{
  double s = 0.0;
  *finite = true;
  for (size_t i = 0; i < N; ++i) {
    const double v = (double)col[i * stride];
    if (!std::isfinite(v)) *finite = false;
    s += v;
  }
  if (!*finite) return std::numeric_limits<double>::quiet_NaN();
  const double mean = s / (double)N;
  double q = 0.0;
  for (size_t i = 0; i < N; ++i) {
    const double t = (double)col[i * stride] - mean;
    q += t * t;
  }
  return std::sqrt(q / (double)(N - 1));
}

}  // namespace mcx_energy_host
