// mcx_reweight.hip -- mcx_*_reweight and mcx_*_resample: importance weights on the rows of a store.
// A per-row log-weight (a host array, a column of another store, or the view's own log L, times a scale) becomes a fixed-point
// weight q in [0, 2^31] once; after that everything is integer adds of q or fp64 sums in a fixed order.
//   1. k_rw_max, k_rw_maxred   lw = scale * v per row: the maximum, and the lowest row with a NaN or +inf (integer atomicMin)
//   2. k_rw_q, k_rw_scan       q[N]; per scan tile of RS rows (one workgroup) the sum of q, the 128-bit sum of q^2 and the count of
//                              zeros -> slabs; one workgroup turns the tile sums into their exclusive scan toff[tiles + 1] and
//                              adds the other slabs up
//   3. k_rw_moments x 2        section 9's tiles, one lane per (chain, column) series: sum q x; then about the mean sum q (x - m)^2
//                              and sum q^2 (x - m)^2 -> per-chain sums, k_sum_rows over the chains
//   4. k_rw_hist x 4           section 9's radix select with weights: LDS bins of 64 bits take q of the rows whose key matches a
//                              target prefix, integer-added to global; the host walk is mcx_debug_select_step's, rem = t - 1
//   5. sort_columns            q itself, one column of sortable keys, sorted in place (the last pass of a reweight): the top
//                              M + 1 go to the host for mcx_khat_of_tail
//   6. k_rw_draw               one lane per draw: r as mcx_samples_draw has it, u = (r Q) >> 64, a binary search of toff, a walk
//                              of the tile's q to the row; the workgroup then copies its rows into the new store
// No float atomics; integer atomics only where the sum does not depend on the order.  Every region of scratch is written,
// zeroed or uploaded by the call before it is read.
#include "mcx_sort_kernels.hpp"
#include "mcx_store.hpp"

#include "mcx_reweight_host.hpp"

#include <limits>

namespace {

constexpr int RS = 1024;                    // rows per scan tile, a power of two: one workgroup of k_rw_max and k_rw_q
constexpr int RPT = RS / SB;                // rows per thread of a scan tile
constexpr int RW_GMAX = 16;                 // target prefixes per column and histogram launch
constexpr size_t RW_HIST_LDS = 32768;       // bytes of 64-bit bins per workgroup: four workgroups fit a compute unit's 160 KiB
constexpr int64_t RW_HIST_CHUNK = 1 << 16;  // steps per workgroup of a histogram pass
constexpr int64_t NMAX = (int64_t)1 << 31;
constexpr uint32_t ST_DRAW = 5;             // mcx_derive.hip's Philox stream of the draws: the same rule, the same stream
constexpr uint32_t NO_ROW = 0xffffffffu;
enum { RT_MAX = 0, RT_Q, RT_MOMENTS, RT_HIST, RT_SORT, RT_DRAW, RT_REWEIGHT, RT_RESAMPLE, RT_N };  // mcx_debug_reweight_times

// the value of row i is p[i * stride]; lw = scale * (double)value
struct WSrc {
  const float *p;
  size_t stride;
  double scale;
};
__device__ __forceinline__ double lw_of(const WSrc &w, int64_t i) { return w.scale * (double)w.p[(size_t)i * w.stride]; }

// mcx_summary.hip's key: NaN last, -0 before +0
__device__ __forceinline__ uint32_t rw_okey(float v)
{
  const uint32_t u = __float_as_uint(v);
  if (v != v) return 0xffffffffu;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
inline float rw_key_float(uint32_t k)
{
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

// 1. grid = scan tiles.  slab[tile] = the largest lw of the tile that is neither NaN nor +inf (-inf if none); *bad = the lowest
// row whose lw is one of the two
__global__ void __launch_bounds__(SB) k_rw_max(WSrc w, int64_t N, double *slab, uint32_t *bad)
{
  __shared__ double red[SB];
  const int tid = (int)threadIdx.x;
  const double pinf = __longlong_as_double(0x7ff0000000000000ll);
  double m = -pinf;
  uint32_t b = NO_ROW;
  for (int j = 0; j < RPT; ++j) {
    const int64_t i = (int64_t)blockIdx.x * RS + (int64_t)j * SB + tid;
    if (i >= N) break;
    const double lw = lw_of(w, i);
    if (lw != lw || lw == pinf) b = min(b, (uint32_t)i);
    else m = fmax(m, lw);
  }
  if (b != NO_ROW) atomicMin(bad, b);
  red[tid] = m;
  __syncthreads();
  for (int s = SB / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
    __syncthreads();
  }
  if (tid == 0) slab[blockIdx.x] = red[0];
}

// one workgroup: out[0] = the maximum of slab[ntile]
__global__ void __launch_bounds__(SB) k_rw_maxred(const double *slab, uint32_t ntile, double *out)
{
  __shared__ double red[SB];
  const int tid = (int)threadIdx.x;
  double m = -__longlong_as_double(0x7ff0000000000000ll);
  for (uint32_t i = tid; i < ntile; i += SB) m = fmax(m, slab[i]);
  red[tid] = m;
  __syncthreads();
  for (int s = SB / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
    __syncthreads();
  }
  if (tid == 0) out[0] = red[0];
}

// (lo, hi) += (blo, bhi) in 128 bits
__device__ __forceinline__ void add128(unsigned long long &lo, unsigned long long &hi, unsigned long long blo, unsigned long long bhi)
{
  const unsigned long long s = lo + blo;
  hi += bhi + (s < lo ? 1ull : 0ull);
  lo = s;
}

// the workgroup's sums of four integers a lane each: behind it r0[0], (r1[0], r2[0]) as 128 bits, r3[0] hold them
__device__ __forceinline__ void rw_tree(unsigned long long *r0, unsigned long long *r1, unsigned long long *r2, unsigned long long *r3, int tid)
{
  __syncthreads();
  for (int s = SB / 2; s > 0; s >>= 1) {
    if (tid < s) {
      r0[tid] += r0[tid + s];
      add128(r1[tid], r2[tid], r1[tid + s], r2[tid + s]);
      r3[tid] += r3[tid + s];
    }
    __syncthreads();
  }
}

// 2. grid = scan tiles.  q[i] = (uint32)rint(2^31 exp(lw_i - lwmax)); tsum[tile] = the tile's sum of q, (sqlo, sqhi)[tile] its sum
// of q^2, nz[tile] its rows with q = 0
__global__ void __launch_bounds__(SB) k_rw_q(WSrc w, int64_t N, const double *lwmax, uint32_t *q, unsigned long long *tsum,
                                             unsigned long long *sqlo, unsigned long long *sqhi, unsigned long long *nz)
{
  __shared__ unsigned long long r0[SB], r1[SB], r2[SB], r3[SB];
  const int tid = (int)threadIdx.x;
  const double mx = lwmax[0];
  unsigned long long s = 0, lo = 0, hi = 0, z = 0;
  for (int j = 0; j < RPT; ++j) {
    const int64_t i = (int64_t)blockIdx.x * RS + (int64_t)j * SB + tid;
    if (i >= N) break;
    const double d = lw_of(w, i) - mx;
    const uint32_t qq = (uint32_t)rint(2147483648.0 * exp(d));
    q[i] = qq;
    s += qq;
    add128(lo, hi, (unsigned long long)qq * qq, 0ull);
    z += qq == 0u ? 1ull : 0ull;
  }
  r0[tid] = s; r1[tid] = lo; r2[tid] = hi; r3[tid] = z;
  rw_tree(r0, r1, r2, r3, tid);
  if (tid == 0) {
    tsum[blockIdx.x] = r0[0];
    sqlo[blockIdx.x] = r1[0];
    sqhi[blockIdx.x] = r2[0];
    nz[blockIdx.x] = r3[0];
  }
}

// the consecutive scan tiles a lane of k_rw_scan owns (the last lanes own fewer, or none)
__host__ __device__ inline uint32_t scan_tiles_per_lane(uint32_t ntile) { return (ntile + SB - 1) / SB; }

// one workgroup: toff[0 .. ntile) the tile sums -> their exclusive scan in place, toff[ntile] = Q; out[4] = Q, the sum of q^2
// (lo, hi), the rows with q = 0.  A lane owns ceil(ntile / SB) consecutive tiles
__global__ void __launch_bounds__(SB) k_rw_scan(unsigned long long *toff, uint32_t ntile, const unsigned long long *sqlo,
                                                const unsigned long long *sqhi, const unsigned long long *nz, unsigned long long *out)
{
  __shared__ unsigned long long r0[SB], r1[SB], r2[SB], r3[SB];
  const int tid = (int)threadIdx.x;
  const uint32_t per = scan_tiles_per_lane(ntile);
  const uint32_t t0 = min(ntile, (uint32_t)tid * per), t1 = min(ntile, t0 + per);
  unsigned long long s = 0, lo = 0, hi = 0, z = 0;
  for (uint32_t t = t0; t < t1; ++t) {
    s += toff[t];
    add128(lo, hi, sqlo[t], sqhi[t]);
    z += nz[t];
  }
  r0[tid] = s; r1[tid] = lo; r2[tid] = hi; r3[tid] = z;
  __syncthreads();
  // the exclusive scan of the lanes' sums
  for (int off = 1; off < SB; off <<= 1) {
    const unsigned long long a = tid >= off ? r0[tid - off] : 0ull;
    __syncthreads();
    r0[tid] += a;
    __syncthreads();
  }
  unsigned long long run = r0[tid] - s;
  const unsigned long long total = r0[SB - 1];
  for (uint32_t t = t0; t < t1; ++t) {
    const unsigned long long v = toff[t];
    toff[t] = run;
    run += v;
  }
  __syncthreads();
  r0[tid] = 0;
  rw_tree(r0, r1, r2, r3, tid);
  if (tid == 0) {
    toff[ntile] = total;
    out[0] = total;
    out[1] = r1[0];
    out[2] = r2[0];
    out[3] = r3[0];
  }
}

// 3. grid = nbc * ntiles.  mean == NULL: o0[col][nc] = the series' sum of q x.  Else, m = mean[col]: o0 = its sum of q (x - m)^2,
// o1 = its sum of q^2 (x - m)^2.  Rows with q = 0 are not read into the sums
__global__ void __launch_bounds__(SB) k_rw_moments(TileSet t, int nc, int64_t T, const uint32_t *q, const double *mean, double *o0,
                                                   double *o1)
{
  const int tile = blockIdx.x % t.ntiles, bc = blockIdx.x / t.ntiles;
  const Lane l = lane_of(t, tile, bc, nc);
  if (!l.ok) return;
  const float *p = t.src + (size_t)l.chain * t.cs + l.lcol;
  const uint32_t *qp = q + l.chain;
  const int col = t.col0 + l.lcol;
  // A row with q = 0 is loaded but a zero is multiplied in its place, so that the loads of a stretch of steps go out together;
  // the sums start at +0 and never become -0, so adding its +0 changes no bit
  double a = 0.0, b = 0.0;
  if (!mean) {
#pragma unroll 8
    for (int64_t s = 0; s < T; ++s) {
      const uint32_t qq = qp[s * nc];
      const double v = (double)p[s * t.rs];
      a += (double)qq * (qq ? v : 0.0);
    }
    o0[(size_t)col * nc + l.chain] = a;
  } else {
    const double m = mean[col];
#pragma unroll 8
    for (int64_t s = 0; s < T; ++s) {
      const uint32_t qq = qp[s * nc];
      const double v = (double)p[s * t.rs];
      const double d = qq ? v - m : 0.0, d2 = d * d, qd = (double)qq;
      a += qd * d2;
      b += (qd * qd) * d2;
    }
    o0[(size_t)col * nc + l.chain] = a;
    o1[(size_t)col * nc + l.chain] = b;
  }
}

// 4. one radix digit, k_sum_hist with weights.  grid = (nbc * ntiles, step chunks); LDS: bins[ct][gn][256] of 64 bits,
// prefixes[ct][gn], the columns' prefix counts [ct]
__global__ void __launch_bounds__(SB) k_rw_hist(TileSet t, int nc, int64_t T, const uint32_t *q, int shift, const uint32_t *gpfx,
                                                const int *gcnt, int G, int g0, int gn, unsigned long long *hist)
{
  extern __shared__ unsigned long long lds64[];
  unsigned long long *cnt = lds64;
  uint32_t *pfx = (uint32_t *)(lds64 + (size_t)t.ct * gn * 256);
  int *ng = (int *)(pfx + (size_t)t.ct * gn);
  const int tile = blockIdx.x % t.ntiles, bc = blockIdx.x / t.ntiles;
  for (int i = threadIdx.x; i < t.ct * gn * 256; i += SB) cnt[i] = 0ull;
  for (int i = threadIdx.x; i < t.ct * gn; i += SB) {
    const int j = i / gn, g = i - j * gn, lc = tile * t.ct + j;
    pfx[i] = lc < t.ncs && g0 + g < G ? gpfx[(size_t)(t.col0 + lc) * G + g0 + g] : 0u;
  }
  for (int j = threadIdx.x; j < t.ct; j += SB) {
    const int lc = tile * t.ct + j;
    ng[j] = lc < t.ncs ? min(gn, max(0, gcnt[t.col0 + lc] - g0)) : 0;
  }
  __syncthreads();
  const Lane l = lane_of(t, tile, bc, nc);
  const int m = l.ok ? ng[l.j] : 0;
  if (m > 0) {
    const uint32_t *mp = pfx + (size_t)l.j * gn;
    unsigned long long *mc = cnt + (size_t)l.j * gn * 256;
    const float *p = t.src + (size_t)l.chain * t.cs + l.lcol;
    const uint32_t *qp = q + l.chain;
    const int64_t s0 = (int64_t)blockIdx.y * RW_HIST_CHUNK, s1 = min(T, s0 + RW_HIST_CHUNK);
    const int dsh = shift - 8;
    auto add = [&](uint32_t qq, float v) {
      if (!qq) return;
      const uint32_t key = rw_okey(v);
      const uint32_t kp = (uint32_t)((uint64_t)key >> shift);
      int lo = 0, hi = m;  // the column's prefixes are sorted and distinct: binary search
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (mp[mid] <= kp) lo = mid; else hi = mid;
      }
      if (mp[lo] == kp) atomicAdd(&mc[lo * 256 + ((key >> dsh) & 255u)], (unsigned long long)qq);
    };
    // the loads of HU steps go out before the first of their adds
    constexpr int HU = 8;
    int64_t s = s0;
    for (; s + HU <= s1; s += HU) {
      uint32_t qq[HU];
      float v[HU];
#pragma unroll
      for (int u = 0; u < HU; ++u) {
        qq[u] = qp[(s + u) * nc];
        v[u] = p[(s + u) * t.rs];
      }
#pragma unroll
      for (int u = 0; u < HU; ++u) add(qq[u], v[u]);
    }
    for (; s < s1; ++s) add(qp[s * nc], p[s * t.rs]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < t.ct * gn * 256; i += SB) {
    const unsigned long long c = cnt[i];
    if (!c) continue;
    const int j = i / (gn * 256), r = i - j * gn * 256, g = r >> 8, lc = tile * t.ct + j;
    if (lc < t.ncs && g0 + g < G) atomicAdd(&hist[((size_t)(t.col0 + lc) * G + g0 + g) * 256 + (r & 255)], c);
  }
}

struct DrawArgs {
  const uint32_t *q;               // [N]
  const unsigned long long *toff;  // [ntile + 1]
  uint32_t ntile, seed;
  int64_t N, K;
  unsigned long long Q;
  const float *x, *ly;  // the source rows
  int np;
  float *xo, *lyo;   // the new store
  long long *index;  // [K]
};

// 6. grid = ceil(K / SB).  Lane k: the smallest row j with q_0 + ... + q_j > u_k; then the workgroup copies its rows
__global__ void __launch_bounds__(SB) k_rw_draw(const DrawArgs a)
{
  __shared__ long long src[SB];
  const int tid = (int)threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * SB, k = base + tid;
  const int cnt = (int)min((int64_t)SB, a.K - base);
  if (tid < cnt) {
    const u32x4 w = philox4x32_10((uint32_t)k, (uint32_t)((uint64_t)k >> 32), 0u, 0u, a.seed, ST_DRAW);
    const unsigned long long r = ((unsigned long long)w.x << 32) | (unsigned long long)w.y;
    const unsigned long long u = __umul64hi(r, a.Q);  // < Q = toff[ntile]
    uint32_t lo = 0, hi = a.ntile;                    // the last tile whose offset is at most u: toff[lo + 1] > u
    while (hi - lo > 1) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (a.toff[mid] <= u) lo = mid; else hi = mid;
    }
    unsigned long long acc = a.toff[lo];
    int64_t i = (int64_t)lo * RS;
    const int64_t end = min(a.N, i + RS), last = end - 1;  // the walk ends at last at the latest: the tile's sum lies above u
    for (; i + 4 <= end; i += 4) {  // four rows a load (a tile starts 4 KiB into q's allocation or at a multiple of it)
      const uint4 v = *reinterpret_cast<const uint4 *>(a.q + i);
      const unsigned long long s4 = (unsigned long long)v.x + v.y + v.z + v.w;
      if (acc + s4 > u) break;
      acc += s4;
    }
    for (; i < last; ++i) {
      acc += a.q[i];
      if (acc > u) break;
    }
    src[tid] = i;
    a.index[k] = i;
    a.lyo[k] = a.ly[i];
  }
  __syncthreads();
  const int total = cnt * a.np;
  float *out = a.xo + (size_t)base * a.np;
  for (int e = tid; e < total; e += SB) {
    const int r = e / a.np, c = e - r * a.np;
    out[e] = a.x[(size_t)src[r] * a.np + c];
  }
}

// ---- launch geometry: what the launches below use and mcx_debug_reweight_geometry reports
inline uint32_t scan_tiles(int64_t N) { return (uint32_t)((N + RS - 1) / RS); }
inline uint32_t sort_tiles(int64_t N) { return (uint32_t)((N + RTILE - 1) / RTILE); }
inline unsigned draw_workgroups(int64_t K) { return (unsigned)((K + SB - 1) / SB); }
inline unsigned hist_step_chunks(int64_t T) { return (unsigned)((T + RW_HIST_CHUNK - 1) / RW_HIST_CHUNK); }  // k_rw_hist's grid.y
// a tile set for a histogram launch of gn prefixes per column: narrower parameter tiles keep the 64-bit bins within the budget
TileSet rw_hist_tiles(TileSet t, int gn, int nc)
{
  while (t.ct > 1 && (size_t)t.ct * gn * 256 * 8 > RW_HIST_LDS) t.ct /= 2;
  t.cg = SB / t.ct; t.ntiles = (t.ncs + t.ct - 1) / t.ct; t.nbc = (nc + t.cg - 1) / t.cg;
  return t;
}
inline size_t rw_hist_lds(const TileSet &t, int gn) { return (size_t)t.ct * gn * 256 * 8 + (size_t)t.ct * gn * 4 + (size_t)t.ct * 4; }
// words of the u64 scratch of passes 1 and 2: toff[ntile + 1] | sqlo[ntile] | sqhi[ntile] | nz[ntile] | out[4]
inline size_t scan_words(uint32_t ntile) { return 4 * (size_t)ntile + 1 + 4; }

// ---- the weight source
int weights_args(const mcx_weights *w, int nsteps, int nc, int device, bool have_device)
{
  if (!w) return fail(MCX_ERR_INVALID, "the weight source w is NULL");
  if (w->kind != MCX_WEIGHT_HOST && w->kind != MCX_WEIGHT_STORE && w->kind != MCX_WEIGHT_LL)
    return fail(MCX_ERR_INVALID, "w.kind = %d: MCX_WEIGHT_HOST (1), MCX_WEIGHT_STORE (2) or MCX_WEIGHT_LL (3)", w->kind);
  if (!std::isfinite(w->scale)) return fail(MCX_ERR_INVALID, "w.scale = %g is not finite", w->scale);
  if (w->kind == MCX_WEIGHT_HOST && !w->logw) return fail(MCX_ERR_INVALID, "w.logw is NULL (MCX_WEIGHT_HOST)");
  if (w->kind == MCX_WEIGHT_STORE) {
    const mcx_store *ws = w->store;
    if (!ws) return fail(MCX_ERR_INVALID, "w.store is NULL (MCX_WEIGHT_STORE)");
    if (ws->T != nsteps || ws->nc != nc)
      return fail(MCX_ERR_INVALID, "reweight: the weight store is %d steps of %d chains, the rows are %d of %d", ws->T, ws->nc, nsteps, nc);
    if (w->col < 0 || w->col > ws->nout) return fail(MCX_ERR_INVALID, "w.col = %d: the weight store has columns 0 to %d", w->col, ws->nout);
    if (have_device && ws->device != device)
      return fail(MCX_ERR_INVALID, "reweight: the rows are on device %d and the weight store on device %d", device, ws->device);
  }
  return MCX_OK;
}

int shape_args(int nsteps, int nc)
{
  if (nsteps < 1 || nc < 1) return fail(MCX_ERR_INVALID, "nsteps = %d, nc = %d: at least one step of one chain", nsteps, nc);
  if ((int64_t)nsteps * nc >= NMAX)
    return fail(MCX_ERR_UNSUPPORTED, "reweight: %lld rows, fewer than 2^31 are supported", (long long)nsteps * nc);
  return MCX_OK;
}

int reweight_args(const double *probs, int nprobs, const mcx_reweight_result *res, const mcx_col_reweight *cols, const double *quantiles)
{
  if (!res) return fail(MCX_ERR_INVALID, "res is NULL");
  if (!cols) return fail(MCX_ERR_INVALID, "cols is NULL");
  if (nprobs < 0 || nprobs > MCX_REWEIGHT_MAX_PROBS) return fail(MCX_ERR_INVALID, "nprobs = %d: 0 to %d probabilities", nprobs, MCX_REWEIGHT_MAX_PROBS);
  if (nprobs > 0 && (!probs || !quantiles)) return fail(MCX_ERR_INVALID, "probs and quantiles are needed when nprobs > 0");
  for (int k = 0; k < nprobs; ++k)
    if (!(probs[k] >= 0.0 && probs[k] <= 1.0)) return fail(MCX_ERR_INVALID, "probs[%d] = %g is not in [0, 1]", k, probs[k]);
  return MCX_OK;
}

int resample_args(int nsteps_out, int nc_out, mcx_store *const *out)
{
  if (!out) return fail(MCX_ERR_INVALID, "out is NULL");
  if (nsteps_out < 1 || nc_out < 1)
    return fail(MCX_ERR_INVALID, "nsteps_out = %d, nc_out = %d: a store of at least one step of one chain", nsteps_out, nc_out);
  if ((int64_t)nsteps_out * nc_out >= NMAX)
    return fail(MCX_ERR_UNSUPPORTED, "resample: %lld draws, fewer than 2^31 are supported", (long long)nsteps_out * nc_out);
  return MCX_OK;
}

// the per-call scratch of the fixed-point weights, released when the call is over
struct RwScratch {
  DevBuf<float> wup;               // MCX_WEIGHT_HOST: the uploaded log-weights
  DevBuf<uint32_t> q, bad;         // q[N]; the lowest refused row
  DevBuf<double> mx;               // slab[ntile] | lwmax
  DevBuf<unsigned long long> t64;  // scan_words(ntile)
  DevBuf<uint32_t> alt, shist, srow;  // the sort of q
  DevBuf<long long> index;         // the draws
  uint32_t ntile = 0;
  double lwmax = 0.0;
  unsigned long long sums[4] = {0, 0, 0, 0};  // Q, sum q^2 lo, hi, zeros
  const unsigned long long *toff() const { return t64.p; }
};

// passes 1 and 2 on stream st: S.q, S.t64 (toff), S.lwmax, S.sums.  The weight store's stream is idle (the caller saw to it)
int weights_device(hipStream_t st, const StoreView &v, const mcx_weights *w, RwScratch &S, StageTimer &tm)
{
  const int64_t N = v.N;
  const uint32_t ntile = S.ntile = scan_tiles(N);
  WSrc src{v.ly, 1, w->scale};
  if (w->kind == MCX_WEIGHT_HOST) {
    MCXCHK(S.wup.alloc((size_t)N));
    HIPCHK(hipMemcpyAsync(S.wup.p, w->logw, (size_t)N * sizeof(float), hipMemcpyHostToDevice, st));
    src.p = S.wup.p;
  } else if (w->kind == MCX_WEIGHT_STORE) {
    const mcx_store *ws = w->store;
    if (w->col == ws->nout) src.p = ws->ly.p;
    else {
      src.p = ws->x.p + w->col;
      src.stride = (size_t)ws->nout;
    }
  }
  MCXCHK(S.q.alloc((size_t)N));
  MCXCHK(S.bad.alloc(1));
  MCXCHK(S.mx.alloc((size_t)ntile + 1));
  MCXCHK(S.t64.alloc(scan_words(ntile)));
  double *lwmax_d = S.mx.p + ntile;
  uint32_t bad = NO_ROW;
  MCXCHK(tm.run(RT_MAX, [&]() -> int {
    HIPCHK(hipMemsetAsync(S.bad.p, 0xff, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_rw_max, dim3(ntile), dim3(SB), 0, st, src, N, S.mx.p, S.bad.p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_rw_maxred, dim3(1), dim3(SB), 0, st, (const double *)S.mx.p, ntile, lwmax_d);
    HIPCHK(hipGetLastError());
    return MCX_OK;
  }));
  HIPCHK(hipMemcpyAsync(&S.lwmax, lwmax_d, sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&bad, S.bad.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (bad != NO_ROW) return fail(MCX_ERR_INVALID, "reweight: the log-weight of row %u is NaN or +inf (the lowest such row)", bad);
  if (!(S.lwmax > -std::numeric_limits<double>::infinity())) return fail(MCX_ERR_INVALID, "reweight: the log-weight of every row is -inf");
  unsigned long long *T64 = S.t64.p, *sqlo = T64 + ntile + 1, *sqhi = sqlo + ntile, *nz = sqhi + ntile, *out = nz + ntile;
  MCXCHK(tm.run(RT_Q, [&]() -> int {
    hipLaunchKernelGGL(k_rw_q, dim3(ntile), dim3(SB), 0, st, src, N, (const double *)lwmax_d, S.q.p, T64, sqlo, sqhi, nz);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_rw_scan, dim3(1), dim3(SB), 0, st, T64, ntile, (const unsigned long long *)sqlo, (const unsigned long long *)sqhi,
                       (const unsigned long long *)nz, out);
    HIPCHK(hipGetLastError());
    return MCX_OK;
  }));
  HIPCHK(hipMemcpyAsync(S.sums, out, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return MCX_OK;
}

// ---- 3. the two moment passes -> per column S1 = sum q x, S2 = sum q (x - mean)^2, S3 = sum q^2 (x - mean)^2 (mean = S1 / Q)
// device doubles: tot[3][ncol][nc] | cs[3][ncol] | mean[ncol]
int moments_passes(hipStream_t st, Bufs B, const StoreView &v, const RwScratch &S, std::vector<double> &cs, std::vector<double> &mean)
{
  const size_t ncol = (size_t)v.ncol, nc = (size_t)v.nc;
  const double Qd = (double)(int64_t)S.sums[0];
  MCXCHK(B.d->alloc(3 * ncol * nc + 4 * ncol));
  double *tot = B.d->p, *csd = tot + 3 * ncol * nc, *md = csd + 3 * ncol;
  cs.assign(3 * ncol, 0.0);
  mean.assign(ncol, 0.0);
  auto rows = [&](const double *in, size_t nrows, double *out) -> int {
    hipLaunchKernelGGL(k_sum_rows, dim3((unsigned)nrows), dim3(SB), 0, st, in, nc, 1, v.ncol, v.np, nc, nc, (const double *)nullptr, 0.0, out);
    HIPCHK(hipGetLastError());
    return MCX_OK;
  };
  for (const TileSet *t : {&v.tx, &v.tl}) {
    hipLaunchKernelGGL(k_rw_moments, dim3((unsigned)(t->nbc * t->ntiles)), dim3(SB), 0, st, *t, v.nc, v.T, (const uint32_t *)S.q.p,
                       (const double *)nullptr, tot, (double *)nullptr);
    HIPCHK(hipGetLastError());
  }
  MCXCHK(rows(tot, ncol, csd));
  HIPCHK(hipMemcpyAsync(cs.data(), csd, ncol * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (size_t c = 0; c < ncol; ++c) mean[c] = cs[c] / Qd;
  HIPCHK(hipMemcpyAsync(md, mean.data(), ncol * sizeof(double), hipMemcpyHostToDevice, st));
  for (const TileSet *t : {&v.tx, &v.tl}) {
    hipLaunchKernelGGL(k_rw_moments, dim3((unsigned)(t->nbc * t->ntiles)), dim3(SB), 0, st, *t, v.nc, v.T, (const uint32_t *)S.q.p,
                       (const double *)md, tot + ncol * nc, tot + 2 * ncol * nc);
    HIPCHK(hipGetLastError());
  }
  MCXCHK(rows(tot + ncol * nc, 2 * ncol, csd + ncol));
  HIPCHK(hipMemcpyAsync(cs.data() + ncol, csd + ncol, 2 * ncol * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return MCX_OK;
}

// ---- 4. the weighted radix select -> pre[ncol][nt], the keys of min, max and every quantile.  mcx_summary.hip's
// order_stats_pass with the thresholds in place of the ranks
int select_passes(hipStream_t st, Bufs B, const StoreView &v, const RwScratch &S, const double *probs, int nprobs, std::vector<uint32_t> &pre)
{
  const int ncol = v.ncol, nt = 2 + nprobs;
  const int64_t Q = (int64_t)S.sums[0];
  std::vector<long long> rem0((size_t)nt);
  rem0[0] = 0;
  rem0[1] = Q - 1;
  for (int k = 0; k < nprobs; ++k) rem0[2 + k] = mcx_reweight_host::quantile_threshold(probs[k], Q) - 1;
  std::vector<long long> rem((size_t)ncol * nt);
  for (int c = 0; c < ncol; ++c) std::copy(rem0.begin(), rem0.end(), rem.begin() + (size_t)c * nt);
  pre.assign((size_t)ncol * nt, 0u);
  std::vector<std::vector<uint32_t>> lists((size_t)ncol);
  std::vector<uint32_t> gp;
  std::vector<int> gc((size_t)ncol);
  std::vector<unsigned long long> hh;
  const unsigned chunks = hist_step_chunks(v.T);
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 32 - 8 * pass;
    int G = 1;  // the longest list of distinct prefixes
    for (int c = 0; c < ncol; ++c) {
      auto &L = lists[c];
      L.assign(pre.begin() + (size_t)c * nt, pre.begin() + (size_t)(c + 1) * nt);
      std::sort(L.begin(), L.end());
      L.erase(std::unique(L.begin(), L.end()), L.end());
      G = std::max(G, (int)L.size());
    }
    gp.assign((size_t)ncol * G, 0u);
    for (int c = 0; c < ncol; ++c) {
      std::copy(lists[c].begin(), lists[c].end(), gp.begin() + (size_t)c * G);
      gc[c] = (int)lists[c].size();
    }
    const size_t nh = (size_t)ncol * G * 256;
    MCXCHK(B.u->alloc(gp.size() + ncol));
    MCXCHK(B.h->alloc(nh));
    HIPCHK(hipMemcpyAsync(B.u->p, gp.data(), gp.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(B.u->p + gp.size(), gc.data(), (size_t)ncol * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(B.h->p, 0, nh * sizeof(unsigned long long), st));
    for (int g0 = 0; g0 < G; g0 += RW_GMAX) {
      const int gn = std::min(RW_GMAX, G - g0);
      for (const TileSet *t0 : {&v.tx, &v.tl}) {
        const TileSet t = rw_hist_tiles(*t0, gn, v.nc);
        hipLaunchKernelGGL(k_rw_hist, dim3((unsigned)(t.nbc * t.ntiles), chunks), dim3(SB), rw_hist_lds(t, gn), st, t, v.nc, v.T,
                           (const uint32_t *)S.q.p, shift, (const uint32_t *)B.u->p, (const int *)(B.u->p + gp.size()), G, g0, gn, B.h->p);
        HIPCHK(hipGetLastError());
      }
    }
    hh.resize(nh);
    HIPCHK(hipMemcpyAsync(hh.data(), B.h->p, nh * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int c = 0; c < ncol; ++c)
      for (int k = 0; k < nt; ++k) {
        const size_t i = (size_t)c * nt + k;
        const int g = (int)(std::lower_bound(lists[c].begin(), lists[c].end(), pre[i]) - lists[c].begin());
        int b = 0;
        MCXCHK(mcx_debug_select_step(hh.data() + ((size_t)c * G + g) * 256, rem[i], &b, &rem[i]));
        pre[i] = (pre[i] << 8) | (uint32_t)b;
      }
  }
  return MCX_OK;
}

// ---- 5. the tail of q for k-hat: q is sorted in place (nothing reads it in row order after this)
int tail_pass(hipStream_t st, RwScratch &S, int64_t N, int64_t M, std::vector<uint32_t> &top, StageTimer &tm)
{
  const uint32_t nblk = sort_tiles(N);
  MCXCHK(S.alt.alloc((size_t)N));
  MCXCHK(S.shist.alloc((size_t)256 * nblk));
  MCXCHK(S.srow.alloc(256));
  MCXCHK(sort_columns(st, S.q.p, S.alt.p, S.shist.p, S.srow.p, N, 1u, nblk, [&](int, auto f) -> int { return tm.run(RT_SORT, f); }));
  top.resize((size_t)M + 1);
  HIPCHK(hipMemcpyAsync(top.data(), S.q.p + (N - M - 1), ((size_t)M + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return MCX_OK;
}

// the reweight of a view on stream st.  ms (RT_N doubles, or NULL): the stages' times
int reweight_device(hipStream_t st, Bufs B, const StoreView &v, const mcx_weights *w, const double *probs, int nprobs,
                    mcx_reweight_result *res, mcx_col_reweight *cols, double *quantiles, double *ms)
{
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  const int ncol = v.ncol, nt = 2 + nprobs;
  const int64_t N = v.N, M = mcx_reweight_host::tail_length(N);
  StageTimer tm{st, ms, RT_N, {}};
  RwScratch S;
  std::vector<double> cs, mean;
  std::vector<uint32_t> pre, top;
  auto run = [&]() -> int {
    MCXCHK(weights_device(st, v, w, S, tm));
    MCXCHK(tm.run(RT_MOMENTS, [&]() -> int { return moments_passes(st, B, v, S, cs, mean); }));
    MCXCHK(tm.run(RT_HIST, [&]() -> int { return select_passes(st, B, v, S, probs, nprobs, pre); }));
    if (M >= 5) MCXCHK(tail_pass(st, S, N, M, top, tm));
    return MCX_OK;
  };
  const int rc = tm.run(RT_REWEIGHT, run);
  if (rc != MCX_OK) (void)hipStreamSynchronize(st);  // (the scratch is the stream's until here)
  MCXCHK(rc);
  const int64_t Q = (int64_t)S.sums[0];
  *res = mcx_reweight_result{};
  res->n = N;
  res->nzero = (long long)S.sums[3];
  res->lwmax = S.lwmax;
  res->sumq = Q;
  res->sumq2_lo = S.sums[1];
  res->sumq2_hi = S.sums[2];
  res->ess_kish = mcx_reweight_host::ess_kish(Q, S.sums[2], S.sums[1]);
  res->log_mean_w = mcx_reweight_host::log_mean_w(S.lwmax, Q, N);
  res->tail_m = M;
  res->khat = res->tail_sigma = qnan;
  res->flags = MCX_REWEIGHT_NO_TAIL;
  if (M >= 5) {
    std::vector<double> x((size_t)M);
    for (int64_t i = 0; i < M; ++i) x[(size_t)i] = (double)(top[(size_t)i + 1] - top[0]) / mcx_reweight_host::TWO31;
    mcx_reweight_host::khat_of_tail(x.data(), M, &res->khat, &res->tail_sigma, &res->flags);
  }
  const double Qd = (double)Q;
  for (int c = 0; c < ncol; ++c) {
    mcx_col_reweight &o = cols[c];
    o = mcx_col_reweight{};
    o.min = rw_key_float(pre[(size_t)c * nt]);
    o.max = rw_key_float(pre[(size_t)c * nt + 1]);
    for (int k = 0; k < nprobs; ++k) quantiles[(size_t)c * nprobs + k] = (double)rw_key_float(pre[(size_t)c * nt + 2 + k]);
    // (finite terms cannot overflow the sum: it is not finite exactly when a row with q > 0 holds an inf or NaN)
    if (!std::isfinite(cs[c])) {
      o.flags = MCX_REWEIGHT_NONFINITE;
      o.mean = o.sd = o.mcse_mean = qnan;
      continue;
    }
    o.mean = mean[c];
    o.sd = std::sqrt(cs[(size_t)ncol + c] / Qd);
    o.mcse_mean = std::sqrt(cs[2 * (size_t)ncol + c]) / Qd;
  }
  return tm.collect();
}

// the resample of a view on stream st -> a new store on the current device
int resample_device(hipStream_t st, const StoreView &v, const mcx_weights *w, uint32_t seed, int nsteps_out, int nc_out, mcx_store **out,
                    int64_t *index, double *ms)
{
  const int64_t K = (int64_t)nsteps_out * nc_out;
  StageTimer tm{st, ms, RT_N, {}};
  RwScratch S;
  std::unique_ptr<mcx_store> o(new mcx_store);
  auto run = [&]() -> int {
    HIPCHK(hipGetDevice(&o->device));
    o->nc = nc_out; o->nout = v.np; o->T = nsteps_out;
    MCXCHK(o->st.ensure(hipStreamNonBlocking));
    MCXCHK(o->x.alloc((size_t)K * v.np));
    MCXCHK(o->ly.alloc((size_t)K));
    MCXCHK(S.index.alloc((size_t)K));
    MCXCHK(weights_device(st, v, w, S, tm));
    const DrawArgs a{S.q.p, S.toff(), S.ntile, seed, v.N, K, S.sums[0], v.x, v.ly, v.np, o->x.p, o->ly.p, S.index.p};
    MCXCHK(tm.run(RT_DRAW, [&]() -> int {
      hipLaunchKernelGGL(k_rw_draw, dim3(draw_workgroups(K)), dim3(SB), 0, st, a);
      HIPCHK(hipGetLastError());
      return MCX_OK;
    }));
    if (index) HIPCHK(hipMemcpyAsync(index, S.index.p, (size_t)K * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MCX_OK;
  };
  const int rc = tm.run(RT_RESAMPLE, run);
  if (rc != MCX_OK) (void)hipStreamSynchronize(st);  // (before the scratch and the new store go)
  MCXCHK(rc);
  MCXCHK(tm.collect());
  *out = o.release();
  return MCX_OK;
}

// the weight store's work is over before the owner's stream reads it
int weight_store_ready(const mcx_weights *w, hipStream_t st)
{
  if (w->kind == MCX_WEIGHT_STORE && w->store->st && (hipStream_t)w->store->st != st) HIPCHK(hipStreamSynchronize(w->store->st));
  return MCX_OK;
}

// host rows have no device until on_rows has made one current: a weight store lies on that one, and its work is over
int weight_store_here(const mcx_weights *w, int nsteps, int nc, hipStream_t st)
{
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  MCXCHK(weights_args(w, nsteps, nc, dev, true));
  return weight_store_ready(w, st);
}

int store_args(const mcx_store *s)
{
  if (!s) return fail(MCX_ERR_INVALID, "the store s is NULL");
  return MCX_OK;
}

int rows_args(const float *rows, int np)
{
  if (!rows) return fail(MCX_ERR_INVALID, "rows is NULL");
  if (np < 1 || np > 256) return fail(MCX_ERR_INVALID, "np = %d: 1 to 256 parameters", np);
  return MCX_OK;
}

}  // namespace

extern "C" int mcx_store_reweight(mcx_store *s, const mcx_weights *w, const double *probs, int nprobs, mcx_reweight_result *res,
                                  mcx_col_reweight *cols, double *quantiles)
{
  MCXCHK(store_args(s));
  MCXCHK(reweight_args(probs, nprobs, res, cols, quantiles));
  MCXCHK(shape_args(s->T, s->nc));
  MCXCHK(weights_args(w, s->T, s->nc, s->device, true));
  HIPCHK(hipSetDevice(s->device));
  MCXCHK(weight_store_ready(w, s->st));
  return reweight_device(s->st, s->bufs(), StoreView(s->span()), w, probs, nprobs, res, cols, quantiles, nullptr);
}

extern "C" int mcx_samples_reweight(mcx_engine *e, int first_step, int nsteps, const mcx_weights *w, const double *probs, int nprobs,
                                    mcx_reweight_result *res, mcx_col_reweight *cols, double *quantiles)
{
  return on_store(
      e, first_step, nsteps,
      [&]() -> int {
        MCXCHK(reweight_args(probs, nprobs, res, cols, quantiles));
        MCXCHK(shape_args(nsteps, e->nchain));
        return weights_args(w, nsteps, e->nchain, e->device, true);
      },
      [&](hipStream_t st, Bufs B, const StoreView &v) {
        MCXCHK(weight_store_ready(w, st));
        return reweight_device(st, B, v, w, probs, nprobs, res, cols, quantiles, nullptr);
      });
}

extern "C" int mcx_rows_reweight(const float *rows, int nsteps, int nc, int np, const mcx_weights *w, const double *probs, int nprobs,
                                 mcx_reweight_result *res, mcx_col_reweight *cols, double *quantiles)
{
  MCXCHK(rows_args(rows, np));
  MCXCHK(reweight_args(probs, nprobs, res, cols, quantiles));
  MCXCHK(shape_args(nsteps, nc));
  MCXCHK(weights_args(w, nsteps, nc, 0, false));
  return on_rows(rows, nsteps, nc, np, [&](hipStream_t st, Bufs B, const StoreView &v) -> int {
    MCXCHK(weight_store_here(w, nsteps, nc, st));
    return reweight_device(st, B, v, w, probs, nprobs, res, cols, quantiles, nullptr);
  });
}

extern "C" int mcx_store_resample(mcx_store *s, const mcx_weights *w, uint32_t seed, int nsteps_out, int nc_out, mcx_store **out,
                                  int64_t *index)
{
  MCXCHK(store_args(s));
  MCXCHK(resample_args(nsteps_out, nc_out, out));
  MCXCHK(shape_args(s->T, s->nc));
  MCXCHK(weights_args(w, s->T, s->nc, s->device, true));
  HIPCHK(hipSetDevice(s->device));
  MCXCHK(weight_store_ready(w, s->st));
  return resample_device(s->st, StoreView(s->span()), w, seed, nsteps_out, nc_out, out, index, nullptr);
}

extern "C" int mcx_samples_resample(mcx_engine *e, int first_step, int nsteps, const mcx_weights *w, uint32_t seed, int nsteps_out,
                                    int nc_out, mcx_store **out, int64_t *index)
{
  return on_store(
      e, first_step, nsteps,
      [&]() -> int {
        MCXCHK(resample_args(nsteps_out, nc_out, out));
        MCXCHK(shape_args(nsteps, e->nchain));
        return weights_args(w, nsteps, e->nchain, e->device, true);
      },
      [&](hipStream_t st, Bufs, const StoreView &v) {
        MCXCHK(weight_store_ready(w, st));
        return resample_device(st, v, w, seed, nsteps_out, nc_out, out, index, nullptr);
      });
}

extern "C" int mcx_rows_resample(const float *rows, int nsteps, int nc, int np, const mcx_weights *w, uint32_t seed, int nsteps_out,
                                 int nc_out, mcx_store **out, int64_t *index)
{
  MCXCHK(rows_args(rows, np));
  MCXCHK(resample_args(nsteps_out, nc_out, out));
  MCXCHK(shape_args(nsteps, nc));
  MCXCHK(weights_args(w, nsteps, nc, 0, false));
  return on_rows(rows, nsteps, nc, np, [&](hipStream_t st, Bufs, const StoreView &v) -> int {
    MCXCHK(weight_store_here(w, nsteps, nc, st));
    return resample_device(st, v, w, seed, nsteps_out, nc_out, out, index, nullptr);
  });
}

// host only
extern "C" int mcx_khat_of_tail(const double *x, long long n, double *khat, double *sigma, int *flags)
{
  if (!khat || !sigma || !flags) return fail(MCX_ERR_INVALID, "khat, sigma or flags is NULL");
  if (n < 0 || (n > 0 && !x)) return fail(MCX_ERR_INVALID, "n = %lld: not negative, and x not NULL", n);
  for (long long i = 0; i < n; ++i)
    if (!(x[i] >= 0.0) || !std::isfinite(x[i]) || (i > 0 && x[i] < x[i - 1]))
      return fail(MCX_ERR_INVALID, "x[%lld] = %g: finite, not negative and in rising order", i, x[i]);
  mcx_reweight_host::khat_of_tail(x, n, khat, sigma, flags);
  return MCX_OK;
}

extern "C" int mcx_debug_reweight_q(mcx_store *s, const float *rows, int nsteps, int nc, int np, const mcx_weights *w, uint32_t *q,
                                    double *lwmax)
{
  if (!s == !rows) return fail(MCX_ERR_INVALID, "exactly one of the store s and rows is given, not %s", s ? "both" : "neither");
  if (!q || !lwmax) return fail(MCX_ERR_INVALID, "q or lwmax is NULL");
  auto body = [&](hipStream_t st, const StoreView &v) -> int {
    MCXCHK(weight_store_ready(w, st));
    StageTimer tm{st, nullptr, RT_N, {}};
    RwScratch S;
    int rc = weights_device(st, v, w, S, tm);
    if (rc == MCX_OK) {
      hipError_t e1 = hipMemcpyAsync(q, S.q.p, (size_t)v.N * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
      if (e1 != hipSuccess) rc = fail(MCX_ERR_HIP, "%s", hipGetErrorString(e1));
      *lwmax = S.lwmax;
    }
    (void)hipStreamSynchronize(st);  // (before the scratch goes)
    return rc;
  };
  if (s) {
    MCXCHK(shape_args(s->T, s->nc));
    MCXCHK(weights_args(w, s->T, s->nc, s->device, true));
    HIPCHK(hipSetDevice(s->device));
    return body(s->st, StoreView(s->span()));
  }
  MCXCHK(rows_args(rows, np));
  MCXCHK(shape_args(nsteps, nc));
  MCXCHK(weights_args(w, nsteps, nc, 0, false));
  return on_rows(rows, nsteps, nc, np, [&](hipStream_t st, Bufs, const StoreView &v) -> int {
    MCXCHK(weight_store_here(w, nsteps, nc, st));
    return body(st, v);
  });
}

// host only
extern "C" int mcx_debug_reweight_geometry(long long N, int ncol, int nprobs, long long K, mcx_reweight_geometry *g)
{
  if (!g) return fail(MCX_ERR_INVALID, "g is NULL");
  if (ncol < 2 || ncol > 257) return fail(MCX_ERR_INVALID, "ncol = %d: 2 to 257 columns", ncol);
  if (nprobs < 0 || nprobs > MCX_REWEIGHT_MAX_PROBS) return fail(MCX_ERR_INVALID, "nprobs = %d: 0 to %d probabilities", nprobs, MCX_REWEIGHT_MAX_PROBS);
  if (N < 1 || K < 0) return fail(MCX_ERR_INVALID, "N = %lld, K = %lld: at least one row, and no negative number of draws", N, K);
  if (N >= NMAX || K >= NMAX) return fail(MCX_ERR_UNSUPPORTED, "N = %lld, K = %lld: fewer than 2^31 are supported", N, K);
  const int np = ncol - 1, nt = 2 + nprobs, gn = std::min(RW_GMAX, nt);
  const TileSet t = rw_hist_tiles(tiles_x(nullptr, 1, np), gn, 1);
  const uint32_t ntile = scan_tiles(N);
  const int64_t M = mcx_reweight_host::tail_length(N);
  g->block = SB;
  g->scan_tile_rows = RS;
  g->scan_tiles = ntile;
  g->hist_targets = nt;
  g->hist_prefixes = gn;
  g->hist_launches = (nt + RW_GMAX - 1) / RW_GMAX;
  g->hist_tile_cols = t.ct;
  g->hist_lds_bytes = (long long)rw_hist_lds(t, gn);
  g->hist_lds_budget = (long long)RW_HIST_LDS;
  g->tail_m = M;
  g->sort_tiles = M >= 5 ? sort_tiles(N) : 0;
  g->draw_workgroups = draw_workgroups(K);
  // q, the refused row, the maxima, the scan words; then the sort of q (a reweight) or the indices (a resample)
  size_t b = 4 * (size_t)N + 4 + 8 * ((size_t)ntile + 1) + 8 * scan_words(ntile);
  if (K > 0) b += 8 * (size_t)K;
  else if (M >= 5) b += 4 * (size_t)N + 4 * 256 * ((size_t)sort_tiles(N) + 1);
  g->scratch_bytes = (long long)b;
  g->scan_tiles_per_lane = scan_tiles_per_lane(ntile);
  g->hist_step_chunks = 0;
  return MCX_OK;
}

extern "C" int mcx_debug_reweight_store_geometry(int nsteps, int nc, int ncol, int nprobs, long long K, mcx_reweight_geometry *g)
{
  MCXCHK(shape_args(nsteps, nc));
  MCXCHK(mcx_debug_reweight_geometry((long long)nsteps * nc, ncol, nprobs, K, g));
  g->hist_step_chunks = hist_step_chunks(nsteps);
  return MCX_OK;
}

extern "C" int mcx_debug_reweight_times(mcx_engine *e, int first_step, int nsteps, const mcx_weights *w, const double *probs, int nprobs,
                                        uint32_t seed, int nsteps_out, int nc_out, double *ms)
{
  const bool draw = (int64_t)nsteps_out * nc_out != 0;
  mcx_store *o = nullptr;
  mcx_reweight_result res;
  std::vector<mcx_col_reweight> cols(e ? (size_t)e->nparam + 1 : 1);
  std::vector<double> qu(cols.size() * (size_t)std::max(0, std::min(nprobs, (int)MCX_REWEIGHT_MAX_PROBS)) + 1);
  const int rc = on_store(
      e, first_step, nsteps,
      [&]() -> int {
        if (!ms) return fail(MCX_ERR_INVALID, "ms is NULL");
        MCXCHK(reweight_args(probs, nprobs, &res, cols.data(), qu.data()));
        if (draw) MCXCHK(resample_args(nsteps_out, nc_out, &o));
        MCXCHK(shape_args(nsteps, e->nchain));
        return weights_args(w, nsteps, e->nchain, e->device, true);
      },
      [&](hipStream_t st, Bufs B, const StoreView &v) -> int {
        MCXCHK(weight_store_ready(w, st));
        double a[RT_N], b[RT_N] = {0.0};
        MCXCHK(reweight_device(st, B, v, w, probs, nprobs, &res, cols.data(), qu.data(), a));
        if (draw) MCXCHK(resample_device(st, v, w, seed, nsteps_out, nc_out, &o, nullptr, b));
        for (int i = 0; i < RT_N; ++i) ms[i] = a[i];
        ms[RT_DRAW] = b[RT_DRAW];
        ms[RT_RESAMPLE] = b[RT_RESAMPLE];
        return MCX_OK;
      });
  delete o;
  return rc;
}
