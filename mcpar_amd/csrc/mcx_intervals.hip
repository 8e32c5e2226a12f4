// mcx_intervals.hip -- mcx_samples_intervals / mcx_rows_intervals / mcx_store_intervals: the interval estimates of a step range
// of the sample store on the device: per column the highest-density intervals of given masses (arviz's
// hdi) and the Monte-Carlo standard errors of the standard deviation and of quantiles, with the effective sizes behind them
// (posterior's mcse_sd, ess_sd, mcse_quantile, ess_quantile).
//
// The store is x[step][chain][np] plus ly[step][chain]; N = T * nc values per column.  Both estimates read a column in sorted
// order, s(0) <= ... <= s(N - 1) in the key order of section 11 (mcx_sort_kernels.hpp).  The passes, in order:
//   1. summary_spread     mcx_summary.hip: mean, sd, flags and the type-7 quantiles of the probabilities
//   2. k_iv_transform     one sweep in the summary's tiles per transform: c2 = float((x - mean)^2), or the indicator x <= q of one
//                         probability, of every column -> a store-shaped scratch; summary_mixing gives its mean, sd and ESS
//   3. the host           mcx_intervals_host.hpp: the beta quantiles u and the ranks k around every quantile
//   4. k_iv_keys, sort_columns   the sorted keys of G columns at a time
//   5. k_hdi_windows      grid (window tiles, columns): w(i) = s(i + m) - s(i) in fp64 for every mass, the minimum of (bits of w,
//                         i) in integer order per workgroup -> slab[column][mass][tile]
//   6. k_hdi_reduce       one workgroup per (column, mass): the minimum over the tiles, and the two keys at its ends
//   7. k_iv_pick          the keys at the host's ranks
// The minimum of a total order does not depend on the order it is taken in; no atomics, no float sums across threads: the same
// store and arguments give the same bytes.
#include "mcx_sort_kernels.hpp"
#include "mcx_store.hpp"
#include "mcx_intervals_host.hpp"

#include <limits>

namespace {

namespace H = mcx_intervals_host;

constexpr int HKPT = 16;            // windows per thread of a window tile
constexpr int HTILE = SB * HKPT;    // window starts per workgroup of k_hdi_windows
constexpr int HWAVES = SB / 64;
constexpr long long NO_INDEX = 0x7fffffffffffffffLL;

// mcx_debug_intervals_times
enum { IT_SPREAD = 0, IT_TRANSFORM, IT_MIXING, IT_KEYS, IT_PASS0, IT_WINDOWS = IT_PASS0 + 4, IT_REDUCE, IT_PICK, IT_TOTAL, IT_N };
static_assert(IT_N == MCX_INTERVAL_TIMES, "include/mcx.h lists the stages");

struct HdiSpans {
  int64_t m[MCX_INTERVAL_MAX_MASSES];
};
struct HdiBest {  // the least (w, i) of a set of windows; w as the bits of a double that is not negative
  unsigned long long w;
  long long i;
};
struct HdiOut {
  unsigned long long w;
  long long i;
  uint32_t klo, khi;  // the keys s(i), s(i + m)
};

__device__ __forceinline__ float key_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ bool hdi_less(unsigned long long w, long long i, unsigned long long bw, long long bi)
{
  return w < bw || (w == bw && i < bi);
}

// 2. one transform of every column of a tile set.  thr[1 + nprobs][ncol]: the means, then the quantile of each probability;
// what = 0: c2, what = 1 + k: the indicator of probability k.  dst has the layout of t.src.  grid = (nbc * ntiles, step chunks)
__global__ void __launch_bounds__(SB) k_iv_transform(TileSet t, int nc, int64_t T, int what, const double *thr, int ncol, float *dst,
                                                     int64_t rchunk)
{
  const int tile = blockIdx.x % t.ntiles, bc = blockIdx.x / t.ntiles;
  const Lane l = lane_of(t, tile, bc, nc);
  if (!l.ok) return;
  const size_t off = (size_t)l.chain * t.cs + l.lcol;
  const float *p = t.src + off;
  float *q = dst + off;
  const double a = thr[(size_t)what * ncol + t.col0 + l.lcol];
  const int64_t s0 = (int64_t)blockIdx.y * rchunk, s1 = min(T, s0 + rchunk);
  if (what == 0) {
    for (int64_t s = s0; s < s1; ++s) {
      const double d = (double)p[s * t.rs] - a;
      q[s * t.rs] = (float)(d * d);
    }
    return;
  }
  for (int64_t s = s0; s < s1; ++s) q[s * t.rs] = (double)p[s * t.rs] <= a ? 1.0f : 0.0f;
}

// 4. keys of columns [c0, c1) of a tile set -> keys[column - c0][N], index = step * nc + chain.  The grid of k_iv_transform
__global__ void __launch_bounds__(SB) k_iv_keys(TileSet t, int nc, int64_t T, int c0, int c1, uint32_t *keys, int64_t N, int64_t rchunk)
{
  const int tile = blockIdx.x % t.ntiles, bc = blockIdx.x / t.ntiles;
  const Lane l = lane_of(t, tile, bc, nc);
  const int col = t.col0 + l.lcol;
  if (!l.ok || col < c0 || col >= c1) return;
  const float *p = t.src + (size_t)l.chain * t.cs + l.lcol;
  uint32_t *k = keys + (size_t)(col - c0) * (size_t)N + l.chain;
  const int64_t s0 = (int64_t)blockIdx.y * rchunk, s1 = min(T, s0 + rchunk);
  for (int64_t s = s0; s < s1; ++s) k[s * nc] = rkey(p[s * t.rs]);
}

// 5. the windows that start in one tile.  grid = (window tiles, columns); keys[column][N] sorted; mass j has the windows
// i < N - m[j].  A thread's starts ascend, so its first least w is the one of the lowest index.  slab[(column * nmass + j) *
// ntiles + tile]; a tile without a window of a mass writes (all ones, NO_INDEX), which loses against every window
__global__ void __launch_bounds__(SB) k_hdi_windows(const uint32_t *keys, int64_t N, int nmass, HdiSpans spans, uint32_t ntiles,
                                                    HdiBest *slab)
{
  __shared__ unsigned long long sw[HWAVES];
  __shared__ long long si[HWAVES];
  const uint32_t *k = keys + (size_t)blockIdx.y * (size_t)N;
  const int64_t base = (int64_t)blockIdx.x * HTILE + threadIdx.x;
  float a[HKPT];
#pragma unroll
  for (int e = 0; e < HKPT; ++e) {
    const int64_t i = base + (int64_t)e * SB;
    a[e] = i < N ? key_value(k[i]) : 0.0f;
  }
  for (int j = 0; j < nmass; ++j) {
    const int64_t m = spans.m[j], nwin = N - m;
    unsigned long long bw = ~0ull;
    long long bi = NO_INDEX;
#pragma unroll
    for (int e = 0; e < HKPT; ++e) {
      const int64_t i = base + (int64_t)e * SB;
      if (i < nwin) {
        const double w = (double)key_value(k[i + m]) - (double)a[e];
        const unsigned long long wb = (unsigned long long)__double_as_longlong(w);
        if (wb < bw) {
          bw = wb;
          bi = i;
        }
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long ow = __shfl_xor(bw, off);
      const long long oi = __shfl_xor(bi, off);
      if (hdi_less(ow, oi, bw, bi)) {
        bw = ow;
        bi = oi;
      }
    }
    if ((threadIdx.x & 63) == 0) {
      sw[threadIdx.x >> 6] = bw;
      si[threadIdx.x >> 6] = bi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int v = 1; v < HWAVES; ++v)
        if (hdi_less(sw[v], si[v], bw, bi)) {
          bw = sw[v];
          bi = si[v];
        }
      slab[((size_t)blockIdx.y * nmass + j) * ntiles + blockIdx.x] = HdiBest{bw, bi};
    }
    __syncthreads();
  }
}

// 6. the least (w, i) over the tiles of one (column, mass) and the keys at the window's ends.  grid = (nmass, columns)
__global__ void __launch_bounds__(SB) k_hdi_reduce(const HdiBest *slab, uint32_t ntiles, int nmass, HdiSpans spans, const uint32_t *keys,
                                                   int64_t N, HdiOut *out)
{
  __shared__ unsigned long long sw[SB];
  __shared__ long long si[SB];
  const size_t r = (size_t)blockIdx.y * nmass + blockIdx.x;
  const HdiBest *row = slab + r * ntiles;
  unsigned long long bw = ~0ull;
  long long bi = NO_INDEX;
  for (uint32_t t = threadIdx.x; t < ntiles; t += SB) {
    const HdiBest b = row[t];
    if (hdi_less(b.w, b.i, bw, bi)) {
      bw = b.w;
      bi = b.i;
    }
  }
  sw[threadIdx.x] = bw;
  si[threadIdx.x] = bi;
  __syncthreads();
  for (int w = SB / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w && hdi_less(sw[threadIdx.x + w], si[threadIdx.x + w], sw[threadIdx.x], si[threadIdx.x])) {
      sw[threadIdx.x] = sw[threadIdx.x + w];
      si[threadIdx.x] = si[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int64_t m = spans.m[blockIdx.x], i = si[0];
    const uint32_t *k = keys + (size_t)blockIdx.y * (size_t)N;
    const bool ok = i >= 0 && i < N - m;
    out[r] = HdiOut{sw[0], ok ? (long long)i : -1LL, ok ? k[i] : 0xffffffffu, ok ? k[i + m] : 0xffffffffu};
  }
}

// 7. the keys at ranks[column][npick] of the sorted keys[column][N] (a rank outside [0, N): a NaN's key).  One thread per rank
__global__ void __launch_bounds__(SB) k_iv_pick(const uint32_t *keys, int64_t N, const int64_t *ranks, int npick, int ncols, uint32_t *out)
{
  const int i = blockIdx.x * SB + threadIdx.x;
  if (i >= ncols * npick) return;
  const int64_t r = ranks[i];
  out[i] = r >= 0 && r < N ? keys[(size_t)(i / npick) * (size_t)N + r] : 0xffffffffu;
}

inline float host_key_value(uint32_t k)
{
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

// ---- launch geometry: what the launches below use and mcx_debug_intervals_geometry reports
struct IntervalsGeometry {
  RankGeometry r;        // the transform and key sweeps, and the sort tiles
  uint32_t wtiles;       // window tiles per column
  int group_cap;         // columns sorted at a time at most
  size_t bytes_per_col;  // keys (two arrays), the sort's counts, the slab and the outputs of one column of a group
};
IntervalsGeometry intervals_geometry(int64_t T, int64_t N, int ncol, int nmass, int nprobs)
{
  IntervalsGeometry g;
  g.r = rank_geometry(T, N);
  g.wtiles = (uint32_t)((N + HTILE - 1) / HTILE);
  g.group_cap = ncol;
  if (const char *cap = std::getenv("MCX_RANK_GROUP_COLS")) g.group_cap = std::max(1, std::min(ncol, std::atoi(cap)));
  g.bytes_per_col = (size_t)N * 8 + ((size_t)g.r.nblk + 1) * 1024 + (size_t)nmass * g.wtiles * sizeof(HdiBest) +
                    (size_t)nmass * sizeof(HdiOut) + (size_t)nprobs * 2 * 4;
  return g;
}

// the scratch of one call, released when it is over
struct IvScratch {
  DevBuf<float> xs, lys;               // the transformed store
  DevBuf<double> thr;                  // [1 + nprobs][ncol]
  DevBuf<uint32_t> ka, kb, hist, rowsum, picked;
  DevBuf<HdiBest> slab;
  DevBuf<HdiOut> best;
  DevBuf<int64_t> ranks;               // [ncol][2 nprobs]
};

struct IvPass {
  hipStream_t st;
  Bufs B;
  const StoreView &v;
  const mcx_interval_spec &spec;
  StageTimer tm;
  IvScratch S;
  IntervalsGeometry g;
  HdiSpans spans;
  int G = 0;
  IvPass(hipStream_t st_, Bufs B_, const StoreView &v_, const mcx_interval_spec &spec_, double *ms)
      : st(st_), B(B_), v(v_), spec(spec_), tm{st_, ms, IT_N, {}}, g(intervals_geometry(v_.T, v_.N, v_.ncol, spec_.nmass, spec_.nprobs))
  {
    for (int j = 0; j < MCX_INTERVAL_MAX_MASSES; ++j) spans.m[j] = j < spec.nmass ? H::hdi_span(spec.mass[j], v.N) : 0;
  }
};

// 2. transform `what` of every column -> S.xs, S.lys, then the mean, sd and ESS of that store -> cs
int transformed_mixing(IvPass &p, int what, std::vector<mcx_col_summary> &cs)
{
  const StoreView &v = p.v;
  MCXCHK(p.tm.run(IT_TRANSFORM, [&]() -> int {
    for (const TileSet *t : {&v.tx, &v.tl}) {
      hipLaunchKernelGGL(k_iv_transform, dim3((unsigned)(t->nbc * t->ntiles), p.g.r.chunks), dim3(SB), 0, p.st, *t, v.nc, v.T, what,
                         (const double *)p.S.thr.p, v.ncol, t == &v.tx ? p.S.xs.p : p.S.lys.p, p.g.r.rchunk);
      HIPCHK(hipGetLastError());
    }
    return MCX_OK;
  }));
  return p.tm.run(IT_MIXING, [&]() -> int {
    return summary_mixing(p.st, p.B, StoreSpan{p.S.xs.p, p.S.lys.p, v.nc, v.np, v.T}, cs.data());
  });
}

// the keys of as many columns at a time as fit -> p.G
int sort_scratch(IvPass &p)
{
  IvScratch &S = p.S;
  const size_t N = (size_t)p.v.N;
  const int nmass = p.spec.nmass, npick = 2 * p.spec.nprobs;
  for (int G = p.g.group_cap;; G = (G + 1) / 2) {
    const bool ok = S.ka.alloc((size_t)G * N) == MCX_OK && S.kb.alloc((size_t)G * N) == MCX_OK &&
                    S.hist.alloc((size_t)G * 256 * p.g.r.nblk) == MCX_OK && S.rowsum.alloc((size_t)G * 256) == MCX_OK &&
                    S.slab.alloc((size_t)G * nmass * p.g.wtiles) == MCX_OK && S.best.alloc((size_t)G * nmass) == MCX_OK &&
                    S.picked.alloc((size_t)G * npick) == MCX_OK;
    if (ok) {
      p.G = G;
      return MCX_OK;
    }
    if (G == 1)
      return fail(MCX_ERR_ALLOC, "intervals: %zu bytes of scratch are needed for one column at a time (DESIGN.md section 23)", p.g.bytes_per_col);
    S.ka.release(); S.kb.release(); S.hist.release(); S.rowsum.release(); S.slab.release(); S.best.release(); S.picked.release();
  }
}

// 4 to 7 for columns [c0, c1): their sorted keys, the least window of every mass and the keys at the ranks -> best, picked (host)
int sorted_group(IvPass &p, int c0, int c1, HdiOut *best, uint32_t *picked)
{
  const StoreView &v = p.v;
  IvScratch &S = p.S;
  const unsigned g = (unsigned)(c1 - c0);
  const int nmass = p.spec.nmass, npick = 2 * p.spec.nprobs;
  MCXCHK(p.tm.run(IT_KEYS, [&]() -> int {
    for (const TileSet *t : {&v.tx, &v.tl}) {
      if (t->col0 + t->ncs <= c0 || t->col0 >= c1) continue;
      hipLaunchKernelGGL(k_iv_keys, dim3((unsigned)(t->nbc * t->ntiles), p.g.r.chunks), dim3(SB), 0, p.st, *t, v.nc, v.T, c0, c1, S.ka.p,
                         v.N, p.g.r.rchunk);
      HIPCHK(hipGetLastError());
    }
    return MCX_OK;
  }));
  MCXCHK(sort_columns(p.st, S.ka.p, S.kb.p, S.hist.p, S.rowsum.p, v.N, g, p.g.r.nblk,
                      [&](int pass, auto f) -> int { return p.tm.run(IT_PASS0 + pass, f); }));
  if (nmass > 0) {
    MCXCHK(p.tm.run(IT_WINDOWS, [&]() -> int {
      hipLaunchKernelGGL(k_hdi_windows, dim3(p.g.wtiles, g), dim3(SB), 0, p.st, (const uint32_t *)S.ka.p, v.N, nmass, p.spans, p.g.wtiles,
                         S.slab.p);
      HIPCHK(hipGetLastError());
      return MCX_OK;
    }));
    MCXCHK(p.tm.run(IT_REDUCE, [&]() -> int {
      hipLaunchKernelGGL(k_hdi_reduce, dim3((unsigned)nmass, g), dim3(SB), 0, p.st, (const HdiBest *)S.slab.p, p.g.wtiles, nmass, p.spans,
                         (const uint32_t *)S.ka.p, v.N, S.best.p);
      HIPCHK(hipGetLastError());
      return MCX_OK;
    }));
    HIPCHK(hipMemcpyAsync(best, S.best.p, (size_t)g * nmass * sizeof(HdiOut), hipMemcpyDeviceToHost, p.st));
  }
  if (npick > 0) {
    MCXCHK(p.tm.run(IT_PICK, [&]() -> int {
      hipLaunchKernelGGL(k_iv_pick, dim3((g * (unsigned)npick + SB - 1) / SB), dim3(SB), 0, p.st, (const uint32_t *)S.ka.p, v.N,
                         (const int64_t *)(S.ranks.p + (size_t)c0 * npick), npick, (int)g, S.picked.p);
      HIPCHK(hipGetLastError());
      return MCX_OK;
    }));
    HIPCHK(hipMemcpyAsync(picked, S.picked.p, (size_t)g * npick * sizeof(uint32_t), hipMemcpyDeviceToHost, p.st));
  }
  HIPCHK(hipStreamSynchronize(p.st));  // (the next group sorts into the same arrays)
  return MCX_OK;
}

// the intervals of a view on stream st, the stages of DESIGN.md section 23 in their order.  ms (IT_N doubles, or NULL): their times
int intervals_device(hipStream_t st, Bufs B, const StoreView &v, const mcx_interval_spec &spec, mcx_col_intervals *cols, mcx_col_hdi *hdi,
                     mcx_col_quantile_se *qse, double *ms)
{
  const int ncol = v.ncol, nmass = spec.nmass, nprobs = spec.nprobs, npick = 2 * nprobs;
  const size_t N = (size_t)v.N;
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  const float fnan = std::numeric_limits<float>::quiet_NaN();
  IvPass p(st, B, v, spec, ms);
  MCXCHK(p.tm.run(IT_TOTAL, [&]() -> int {
    // 1. mean, sd, flags and the quantiles
    std::vector<mcx_col_summary> c0s(ncol), cs(ncol);
    std::vector<double> q((size_t)ncol * std::max(nprobs, 1));
    MCXCHK(p.tm.run(IT_SPREAD, [&]() -> int { return summary_spread(st, B, v, spec.probs, nprobs, c0s.data(), q.data()); }));
    std::vector<double> thr((size_t)(1 + nprobs) * ncol);
    for (int c = 0; c < ncol; ++c) {
      thr[c] = c0s[c].mean;
      for (int k = 0; k < nprobs; ++k) thr[(size_t)(1 + k) * ncol + c] = q[(size_t)c * nprobs + k];
      cols[c].mean = c0s[c].mean;
      cols[c].sd = c0s[c].sd;
      cols[c].flags = c0s[c].flags;
    }
    // 2. the transformed stores and their effective sizes
    MCXCHK(p.S.thr.alloc(thr.size()));
    HIPCHK(hipMemcpyAsync(p.S.thr.p, thr.data(), thr.size() * sizeof(double), hipMemcpyHostToDevice, st));
    if (p.S.xs.alloc(N * v.np) != MCX_OK || p.S.lys.alloc(N) != MCX_OK)
      return fail(MCX_ERR_ALLOC, "intervals: %zu bytes of scratch are needed for the transformed store (DESIGN.md section 23)", N * ncol * 4);
    MCXCHK(transformed_mixing(p, 0, cs));
    for (int c = 0; c < ncol; ++c) {
      const bool bad = (cols[c].flags & MCX_SUMMARY_NONFINITE) || (cs[c].flags & MCX_SUMMARY_NONFINITE);  // (a c2 beyond the floats)
      cols[c].ess_sd = bad ? qnan : cs[c].ess;
      cols[c].ess_sd_lag = bad ? 0 : cs[c].ess_lag;
      cols[c].mcse_sd = bad ? qnan : H::mcse_sd(v.N, cs[c].mean, cs[c].sd, cs[c].ess);
    }
    // 3. the ranks around every quantile
    std::vector<int64_t> ranks((size_t)ncol * std::max(npick, 1), -1);
    for (int k = 0; k < nprobs; ++k) {
      MCXCHK(transformed_mixing(p, 1 + k, cs));
      for (int c = 0; c < ncol; ++c) {
        mcx_col_quantile_se &o = qse[(size_t)c * nprobs + k];
        const bool bad = cols[c].flags & MCX_SUMMARY_NONFINITE;
        o.q = bad ? qnan : q[(size_t)c * nprobs + k];
        o.ess_q = bad ? qnan : cs[c].ess;
        o.ess_q_lag = bad ? 0 : cs[c].ess_lag;
        o.reserved = 0;
        int64_t *r = ranks.data() + (size_t)c * npick + 2 * k;
        H::quantile_ranks(v.N, spec.probs[k], o.ess_q, &o.u_lo, &o.u_hi, &r[0], &r[1]);
        o.k_lo = r[0];
        o.k_hi = r[1];
      }
    }
    HIPCHK(hipStreamSynchronize(st));
    p.S.xs.release(); p.S.lys.release();  // mid-life: room for the keys
    // 4 to 7. the sorted columns, a group at a time
    MCXCHK(p.S.ranks.alloc(ranks.size()));
    HIPCHK(hipMemcpyAsync(p.S.ranks.p, ranks.data(), ranks.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    MCXCHK(sort_scratch(p));
    std::vector<HdiOut> best((size_t)p.G * std::max(nmass, 1));
    std::vector<uint32_t> picked((size_t)p.G * std::max(npick, 1));
    for (int c0 = 0; c0 < ncol; c0 += p.G) {
      const int c1 = std::min(ncol, c0 + p.G);
      MCXCHK(sorted_group(p, c0, c1, best.data(), picked.data()));
      for (int c = c0; c < c1; ++c) {
        const bool bad = cols[c].flags & MCX_SUMMARY_NONFINITE;
        for (int j = 0; j < nmass; ++j) {
          const HdiOut &b = best[(size_t)(c - c0) * nmass + j];
          mcx_col_hdi &o = hdi[(size_t)c * nmass + j];
          o.span = p.spans.m[j];
          if (bad || b.i < 0) {
            o.width = qnan;
            o.lo = o.hi = fnan;
            o.index = -1;
            continue;
          }
          std::memcpy(&o.width, &b.w, 8);
          o.index = b.i;
          o.lo = host_key_value(b.klo);
          o.hi = host_key_value(b.khi);
        }
        for (int k = 0; k < nprobs; ++k) {
          mcx_col_quantile_se &o = qse[(size_t)c * nprobs + k];
          const uint32_t *pk = picked.data() + (size_t)(c - c0) * npick + 2 * k;
          o.s_lo = o.k_lo < 0 ? fnan : host_key_value(pk[0]);
          o.s_hi = o.k_hi < 0 ? fnan : host_key_value(pk[1]);
          o.mcse_q = o.k_lo < 0 || o.k_hi < 0 ? qnan : ((double)o.s_hi - (double)o.s_lo) / 2.0;
        }
      }
    }
    return MCX_OK;
  }));
  return p.tm.collect();
}

// what every entry point refuses before a device is touched
int intervals_args(int nsteps, int nc, const mcx_interval_spec *spec, const mcx_col_intervals *cols, const mcx_col_hdi *hdi,
                   const mcx_col_quantile_se *qse)
{
  if (!spec) return fail(MCX_ERR_INVALID, "spec is NULL");
  if (!cols) return fail(MCX_ERR_INVALID, "cols is NULL");
  if (spec->nmass < 0 || spec->nmass > MCX_INTERVAL_MAX_MASSES)
    return fail(MCX_ERR_INVALID, "nmass = %d: 0 to %d masses", spec->nmass, MCX_INTERVAL_MAX_MASSES);
  if (spec->nprobs < 0 || spec->nprobs > MCX_INTERVAL_MAX_PROBS)
    return fail(MCX_ERR_INVALID, "nprobs = %d: 0 to %d probabilities", spec->nprobs, MCX_INTERVAL_MAX_PROBS);
  if (spec->nmass > 0 && (!spec->mass || !hdi)) return fail(MCX_ERR_INVALID, "mass and hdi are needed when nmass > 0");
  if (spec->nprobs > 0 && (!spec->probs || !qse)) return fail(MCX_ERR_INVALID, "probs and qse are needed when nprobs > 0");
  for (int j = 0; j < spec->nmass; ++j)
    if (!(spec->mass[j] > 0.0 && spec->mass[j] < 1.0)) return fail(MCX_ERR_INVALID, "mass[%d] = %g is not in (0, 1)", j, spec->mass[j]);
  for (int k = 0; k < spec->nprobs; ++k)
    if (!(spec->probs[k] >= 0.0 && spec->probs[k] <= 1.0)) return fail(MCX_ERR_INVALID, "probs[%d] = %g is not in [0, 1]", k, spec->probs[k]);
  MCXCHK(half_chain_args(nsteps));
  if (nc >= 1 && (int64_t)nsteps * nc >= ((int64_t)1 << 31))
    return fail(MCX_ERR_UNSUPPORTED, "intervals: %lld values per column, fewer than 2^31 are supported", (long long)nsteps * nc);
  return MCX_OK;
}

}  // namespace

extern "C" int mcx_samples_intervals(mcx_engine *e, int first_step, int nsteps, const mcx_interval_spec *spec, mcx_col_intervals *cols,
                                     mcx_col_hdi *hdi, mcx_col_quantile_se *qse)
{
  return on_store(
      e, first_step, nsteps, [&] { return intervals_args(nsteps, e->nchain, spec, cols, hdi, qse); },
      [&](hipStream_t st, Bufs B, const StoreView &v) { return intervals_device(st, B, v, *spec, cols, hdi, qse, nullptr); });
}

extern "C" int mcx_rows_intervals(const float *rows, int nsteps, int nc, int np, const mcx_interval_spec *spec, mcx_col_intervals *cols,
                                  mcx_col_hdi *hdi, mcx_col_quantile_se *qse)
{
  if (!rows) return fail(MCX_ERR_INVALID, "rows is NULL");
  if (nc < 1) return fail(MCX_ERR_INVALID, "nc = %d: at least one chain", nc);
  if (np < 1 || np > 256) return fail(MCX_ERR_INVALID, "np = %d: 1 to 256 parameters", np);
  MCXCHK(intervals_args(nsteps, nc, spec, cols, hdi, qse));
  return on_rows(rows, nsteps, nc, np,
                 [&](hipStream_t st, Bufs B, const StoreView &v) { return intervals_device(st, B, v, *spec, cols, hdi, qse, nullptr); });
}

extern "C" int mcx_store_intervals(mcx_store *s, const mcx_interval_spec *spec, mcx_col_intervals *cols, mcx_col_hdi *hdi,
                                   mcx_col_quantile_se *qse)
{
  if (!s) return fail(MCX_ERR_INVALID, "the store s is NULL");
  MCXCHK(intervals_args(s->T, s->nc, spec, cols, hdi, qse));
  HIPCHK(hipSetDevice(s->device));
  return intervals_device(s->st, s->bufs(), StoreView(s->span()), *spec, cols, hdi, qse, nullptr);
}

extern "C" int mcx_debug_intervals_times(mcx_engine *e, int first_step, int nsteps, const mcx_interval_spec *spec, double *ms)
{
  std::vector<mcx_col_intervals> cols;
  std::vector<mcx_col_hdi> hdi;
  std::vector<mcx_col_quantile_se> qse;
  return on_store(
      e, first_step, nsteps,
      [&] {
        if (!ms) return fail(MCX_ERR_INVALID, "ms is NULL");
        if (!spec) return fail(MCX_ERR_INVALID, "spec is NULL");
        const size_t ncol = (size_t)e->nparam + 1;
        cols.resize(ncol);
        hdi.resize(ncol * MCX_INTERVAL_MAX_MASSES);
        qse.resize(ncol * MCX_INTERVAL_MAX_PROBS);
        return intervals_args(nsteps, e->nchain, spec, cols.data(), hdi.data(), qse.data());
      },
      [&](hipStream_t st, Bufs B, const StoreView &v) { return intervals_device(st, B, v, *spec, cols.data(), hdi.data(), qse.data(), ms); });
}

// host only
extern "C" int mcx_debug_intervals_geometry(int nsteps, int nc, int np, int nmass, int nprobs, mcx_intervals_geometry *g)
{
  if (!g) return fail(MCX_ERR_INVALID, "g is NULL");
  if (nc < 1 || np < 1 || np > 256) return fail(MCX_ERR_INVALID, "nc = %d, np = %d: at least one chain, 1 to 256 parameters", nc, np);
  if (nmass < 0 || nmass > MCX_INTERVAL_MAX_MASSES || nprobs < 0 || nprobs > MCX_INTERVAL_MAX_PROBS)
    return fail(MCX_ERR_INVALID, "nmass = %d, nprobs = %d: 0 to %d masses, 0 to %d probabilities", nmass, nprobs, MCX_INTERVAL_MAX_MASSES,
                MCX_INTERVAL_MAX_PROBS);
  MCXCHK(half_chain_args(nsteps));
  const int64_t N = (int64_t)nsteps * nc;
  if (N >= ((int64_t)1 << 31)) return fail(MCX_ERR_UNSUPPORTED, "intervals: %lld values per column, fewer than 2^31 are supported", (long long)N);
  const IntervalsGeometry ig = intervals_geometry(nsteps, N, np + 1, nmass, nprobs);
  g->block = SB;
  g->window_tile = HTILE;
  g->window_tiles = ig.wtiles;
  g->slab_entries = (long long)nmass * ig.wtiles;
  g->slab_bytes = (long long)nmass * ig.wtiles * (long long)sizeof(HdiBest);
  g->reduce_workgroups = nmass;
  g->pick_ranks = 2 * nprobs;
  g->transforms = 1 + nprobs;
  g->sort_tiles = ig.r.nblk;
  g->step_chunk = ig.r.rchunk;
  g->grid_y = ig.r.chunks;
  g->group_cols = ig.group_cap;
  g->groups = (np + 1 + ig.group_cap - 1) / ig.group_cap;
  g->store_scratch_bytes = N * (long long)(np + 1) * 4;
  g->scratch_bytes_per_col = (long long)ig.bytes_per_col;
  return MCX_OK;
}

// host only
extern "C" int mcx_beta_quantile(double p, double a, double b, double *x)
{
  if (!x) return fail(MCX_ERR_INVALID, "x is NULL");
  *x = H::beta_quantile(p, a, b);
  if (*x != *x) return fail(MCX_ERR_INVALID, "beta quantile: p = %g in [0, 1], a = %g and b = %g finite and at least 1 are needed", p, a, b);
  return MCX_OK;
}

// host only
extern "C" int mcx_intervals_quantile_ranks(long long N, double prob, double ess, double *u_lo, double *u_hi, long long *k_lo,
                                            long long *k_hi)
{
  if (!u_lo || !u_hi || !k_lo || !k_hi) return fail(MCX_ERR_INVALID, "an output is NULL");
  if (N < 1 || !(prob >= 0.0 && prob <= 1.0)) return fail(MCX_ERR_INVALID, "N = %lld, prob = %g: at least one value, a probability in [0, 1]", N, prob);
  int64_t lo = -1, hi = -1;
  H::quantile_ranks(N, prob, ess, u_lo, u_hi, &lo, &hi);
  *k_lo = lo;
  *k_hi = hi;
  return MCX_OK;
}
