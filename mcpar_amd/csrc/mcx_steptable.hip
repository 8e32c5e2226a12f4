// mcx_steptable.hip -- the per-step table of a sample store and the rule that names the step from which the ensemble no longer
// drifts: mcx_*_step_table, mcx_steps_settle.  The one analysis whose unit is the step.
//
// The store is step-major, so the nc values of a (step, column) lie in one segment of the step.  A workgroup of 256 lanes owns
// one step's values of a tile of adjacent columns, all nc chains; its lanes stride over the chains, lane (k, j) taking column j
// of chains k, k + cg, ... (cg = 256 / tile width), so a wavefront's load is one contiguous piece per chain.  The parameter
// columns and log L are separate tiles, as the store keeps them in two arrays.  Three sweeps:
//   k_step_moments   grid = T * (column tiles + 1).  Pass 1: per-lane fp64 sums, a fixed tree in LDS -> mean.  Pass 2 reads the
//                    segment again: sum (x - mean)^2 the same way, min and max by the order-preserving u32 key (integer LDS
//                    atomics) -> cols[t][c]
//   k_step_select    grid = T * (narrower column tiles + 1), only when nprobs > 0.  Exact order statistics by radix select, 8
//                    bits per pass, the four passes in one launch: per (column, distinct prefix of the column's target ranks) a
//                    histogram of 256 u32 bins in LDS (integer LDS atomics), walked by one lane per target rank; then the
//                    type-7 interpolation in fp64 -> quantiles[t][c][k]
//   k_step_rows<V>   grid = (T, chunks).  Section 16's row sweep turned round: G lanes per chain compare step t with step t - 1
//                    as u32, one ballot per row; the workgroup counts the chains that moved and keeps the maximum of
//                    (key << 32) | ~chain of log L, and writes both to its fixed slot; k_step_rows_reduce adds and maximises
//                    the chunks' slots (integers: any order gives the same bytes) -> two words per step
// No float atomics and no global atomics: the bytes do not depend on scheduling.
#include "mcx_store.hpp"

#include "mcx_steptable_host.hpp"

#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>

namespace {

constexpr int MAXP = MCX_STEP_MAX_PROBS;
constexpr int SEL_BIN_KIB = 63;       // a select workgroup's histograms: at most 63 KiB, 1 KiB per (column, slot) ...
constexpr int SEL_STATE_BYTES = 1024;  // ... and 1 KiB of select state behind them: 64 KiB, two workgroups to a CU's 160 KiB
constexpr int SEL_BATCH = 8;          // values a lane of the select sweep loads before it bins them
constexpr int ROW_CHUNKS = 32;        // workgroups per step of the row sweep, at most
constexpr int ROW_WORDS = 2;          // u64 words of a step from the row sweep: moved, (key << 32) | ~chain

// ascending in float order: -inf < finite < +inf, -0 before +0; every NaN sorts last (section 9's key)
__device__ __forceinline__ uint32_t step_key_bits(uint32_t u)
{
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline uint32_t step_key_inverse(uint32_t k) { return (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; }

// ---- launch geometry: what the launches below use and mcx_debug_steptable_geometry reports
struct StepGeometry {
  int mct, mcg, mtiles;  // moments sweep: columns per parameter tile, chains per stride, parameter tiles
  long long mwg;
  size_t mlds;
  int P, sct, scg, stiles;  // select sweep: slots per column, columns per parameter tile, chains per stride, parameter tiles
  long long swg;
  size_t slds;
  RowsGeometry rows;
  int chunks;
  long long rwg;
  size_t nd, nh;  // scratch: doubles (cols as 4 each, then the quantiles), u64 words (the chunks' slots, then the steps')
};
StepGeometry step_geometry(int np, int64_t T, int nc, int nprobs)
{
  StepGeometry g;
  g.mct = std::min(np, CTX);
  g.mcg = SB / g.mct;
  g.mtiles = (np + g.mct - 1) / g.mct;
  g.mwg = (long long)T * (g.mtiles + 1);
  g.mlds = SB * sizeof(double) + 2 * CTX * sizeof(uint32_t);
  g.P = 2 * nprobs;
  g.sct = g.scg = g.stiles = 0;
  g.swg = 0;
  g.slds = 0;
  if (nprobs > 0) {
    g.sct = std::min(std::min(np, CTX), SEL_BIN_KIB / g.P);
    g.scg = SB / g.sct;
    g.stiles = (np + g.sct - 1) / g.sct;
    g.swg = (long long)T * (g.stiles + 1);
    g.slds = (size_t)g.sct * g.P * 256 * sizeof(uint32_t) + SEL_STATE_BYTES;
  }
  g.rows = rows_geometry(np, nc);
  g.chunks = (int)std::min<unsigned>(g.rows.nwg, ROW_CHUNKS);
  g.rwg = (long long)T * g.chunks;
  g.nd = (size_t)T * (np + 1) * (4 + (size_t)nprobs);
  g.nh = (size_t)T * ROW_WORDS * ((size_t)g.chunks + 1);
  return g;
}

// what a workgroup of the moments and select sweeps is given: block b of a grid of T * (ntx + 1) is step b / (ntx + 1), tile b
// % (ntx + 1), tile ntx being log L; ct columns per parameter tile
struct StepTile {
  int64_t t;
  int w, cg, k, j, col;  // the tile's width and chains per stride; the lane's chain offset, column of the tile, global column
  int col0;              // the tile's first global column
  bool isl, ok;          // the tile is log L; the lane has a column and a place in the stride
  const float *p;        // the lane's column at chain 0 of step t
  size_t cs;             // floats per chain
};
__device__ __forceinline__ StepTile step_tile(const float *x, const float *ly, int nc, int np, int ct, int ntx)
{
  StepTile s;
  const int ntile = ntx + 1, tile = (int)(blockIdx.x % (unsigned)ntile), tid = (int)threadIdx.x;
  s.t = (int64_t)(blockIdx.x / (unsigned)ntile);
  const bool isl = tile == ntx;
  s.isl = isl;
  s.col0 = isl ? np : tile * ct;
  s.w = isl ? 1 : ct;
  s.cg = SB / s.w;
  s.k = tid / s.w;
  s.j = tid - s.k * s.w;
  const int lcol = isl ? 0 : tile * ct + s.j;
  s.col = isl ? np : lcol;
  s.ok = s.k < s.cg && (isl || lcol < np);
  s.cs = isl ? 1 : (size_t)np;
  s.p = isl ? ly + (size_t)s.t * nc : x + (size_t)s.t * nc * np + (s.ok ? lcol : 0);
  return s;
}

// red[k * w + j] of k < cg -> red[j] = the sum over k, in a fixed tree; every lane of the workgroup calls it
__device__ __forceinline__ void step_tree(double *red, int tid, int k, int w, int cg)
{
  int top = 1;
  while (top < cg) top <<= 1;
  int lim = cg;
  for (int h = top >> 1; h > 0; h >>= 1) {
    if (k < h && k + h < lim) red[tid] += red[tid + h * w];
    __syncthreads();
    lim = h;
  }
}

// ---- the moments sweep.  grid = T * (ntx + 1); no lane returns before the last barrier
__global__ void __launch_bounds__(SB) k_step_moments(const float *x, const float *ly, int nc, int np, int ct, int ntx, mcx_step_col *cols)
{
  __shared__ double red[SB];
  __shared__ uint32_t kmin[CTX], kmax[CTX];
  const StepTile s = step_tile(x, ly, nc, np, ct, ntx);
  const int tid = (int)threadIdx.x;
  double sum = 0.0;
  if (s.ok) {
#pragma unroll 8
    for (int64_t c = s.k; c < nc; c += s.cg) sum += (double)s.p[(size_t)c * s.cs];
  }
  red[tid] = sum;
  if (tid < CTX) {
    kmin[tid] = 0xffffffffu;
    kmax[tid] = 0u;
  }
  __syncthreads();
  step_tree(red, tid, s.k, s.w, s.cg);
  const double tot = red[s.j];
  __syncthreads();  // (before red is written again)
  const bool fin = isfinite(tot);  // (finite floats cannot overflow an fp64 sum: an inf or NaN among the values, and only that)
  const double mean = tot / (double)nc;
  double ss = 0.0;
  uint32_t lo = 0xffffffffu, hi = 0u;
  if (s.ok) {
#pragma unroll 8
    for (int64_t c = s.k; c < nc; c += s.cg) {  // the same segment again
      const float v = s.p[(size_t)c * s.cs];
      const double d = (double)v - mean;
      ss += d * d;
      const uint32_t key = step_key_bits(__float_as_uint(v));
      lo = min(lo, key);
      hi = max(hi, key);
    }
  }
  red[tid] = ss;
  if (s.ok) {
    atomicMin(&kmin[s.j], lo);
    atomicMax(&kmax[s.j], hi);
  }
  __syncthreads();
  step_tree(red, tid, s.k, s.w, s.cg);
  if (s.ok && s.k == 0) {
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const bool has_nan = kmax[s.j] == 0xffffffffu;
    mcx_step_col o;
    o.mean = fin ? mean : qnan;
    o.sd = fin ? sqrt(red[s.j] / (double)(nc - 1)) : qnan;  // (nc = 1: 0 / 0)
    o.min = __uint_as_float(has_nan ? 0x7fc00000u : step_key_inverse(kmin[s.j]));
    o.max = __uint_as_float(has_nan ? 0x7fc00000u : step_key_inverse(kmax[s.j]));
    o.flags = fin ? 0 : MCX_SUMMARY_NONFINITE;
    o.reserved = 0;
    cols[(size_t)s.t * (np + 1) + s.col] = o;
  }
}

// ---- the select sweep.  grid = T * (ntx + 1); dynamic LDS: bins[ct * P][256] u32, then SEL_STATE_BYTES of state
struct StepSelArgs {
  const float *x, *ly;
  const mcx_step_col *cols;  // of the moments sweep: a NaN max says the column holds a NaN
  double *q;                 // [T][ncol][nprobs]
  int nc, np, ct, ntx, nprobs;
  int rank[2 * MAXP];  // the target ranks: lo and min(lo + 1, nc - 1) of every probability
  double g[MAXP];      // h - lo of every probability
};

__global__ void __launch_bounds__(SB) k_step_select(const StepSelArgs a)
{
  extern __shared__ uint32_t lds[];
  const int P = 2 * a.nprobs, nslot = a.ct * P;
  uint32_t *bins = lds;                       // [w * P][256]
  uint32_t *pfx = lds + (size_t)nslot * 256;  // [w][P] the key bits of target q found so far
  uint32_t *rem = pfx + nslot;                // [w][P] its rank among the values that share them
  unsigned char *slot = reinterpret_cast<unsigned char *>(rem + nslot);  // [w][P] the first target with the same prefix
  unsigned char *lead = slot + nslot;         // [w][P] per column, the targets that are their own slot, packed
  unsigned char *nlead = lead + nslot;        // [w]
  static_assert(SEL_BIN_KIB * (4 + 4 + 1 + 1) + CTX <= SEL_STATE_BYTES, "ct * P <= 63 targets: the select state fits its KiB");
  const StepTile s = step_tile(a.x, a.ly, a.nc, a.np, a.ct, a.ntx);
  const int tid = (int)threadIdx.x, nt = s.w * P;  // targets of this tile
  for (int i = tid; i < nt; i += SB) {
    pfx[i] = 0u;
    rem[i] = (uint32_t)a.rank[i % P];
  }
  __syncthreads();
  for (int d = 0; d < 4; ++d) {
    const int shift = 24 - 8 * d;
    if (tid < s.w) {  // the column's distinct prefixes
      int n = 0;
      for (int q = 0; q < P; ++q) {
        int f = q;
        for (int r = 0; r < q; ++r)
          if (pfx[tid * P + r] == pfx[tid * P + q]) {
            f = r;
            break;
          }
        slot[tid * P + q] = (unsigned char)f;
        if (f == q) lead[tid * P + n++] = (unsigned char)q;
      }
      nlead[tid] = (unsigned char)n;
    }
    for (int i = tid; i < nt * 256; i += SB) bins[i] = 0u;
    __syncthreads();
    if (s.ok) {
      const int n = nlead[s.j];
      const uint32_t *mp = pfx + s.j * P;
      const unsigned char *ml = lead + s.j * P;
      // the column's distinct prefixes and their slots in registers (0xffffffff: none, no prefix has more than 24 bits), so that
      // a value costs compares and one LDS atomic, not a walk through LDS; SEL_BATCH loads in flight per lane, then their
      // bins: at 61 KiB of LDS a SIMD holds two wavefronts, and one load at a time each leaves the memory idle
      uint32_t lp[2 * MAXP], lq[2 * MAXP];
#pragma unroll
      for (int i = 0; i < 2 * MAXP; ++i) {
        const int q = i < n ? (int)ml[i] : 0;
        lq[i] = (uint32_t)(s.j * P + q);
        lp[i] = i < n ? mp[q] : 0xffffffffu;
      }
      for (int64_t c0 = s.k; c0 < a.nc; c0 += (int64_t)SEL_BATCH * s.cg) {
        uint32_t bits[SEL_BATCH];
#pragma unroll
        for (int u = 0; u < SEL_BATCH; ++u) {
          const int64_t c = c0 + (int64_t)u * s.cg;
          bits[u] = c < a.nc ? __float_as_uint(s.p[(size_t)c * s.cs]) : 0u;
        }
#pragma unroll
        for (int u = 0; u < SEL_BATCH; ++u) {
          if (c0 + (int64_t)u * s.cg >= a.nc) break;
          const uint32_t key = step_key_bits(bits[u]);
          const uint32_t hp = d == 0 ? 0u : key >> (shift + 8);
          uint32_t sl = 0xffffffffu;
#pragma unroll
          for (int i = 0; i < 2 * MAXP; ++i) sl = lp[i] == hp ? lq[i] : sl;  // (distinct: one at most)
          if (sl != 0xffffffffu) atomicAdd(&bins[sl * 256u + ((key >> shift) & 255u)], 1u);
        }
      }
    }
    __syncthreads();
    if (tid < nt) {  // one lane per target walks its slot's bins
      const uint32_t *h = bins + (size_t)((tid / P) * P + slot[tid]) * 256;
      const uint32_t r = rem[tid];
      uint32_t cum = 0u;
      int b = 0;
      for (; b < 255; ++b) {
        const uint32_t cnt = h[b];
        if (cum + cnt > r) break;
        cum += cnt;
      }
      rem[tid] = r - cum;
      pfx[tid] = d == 0 ? (uint32_t)b : (pfx[tid] << 8) | (uint32_t)b;
    }
    __syncthreads();
  }
  // x(lo) when g = 0 or x(lo) = x(lo + 1), else x(lo) + g (x(lo + 1) - x(lo)), fp64
  if (tid < s.w * a.nprobs) {
    const int jj = tid / a.nprobs, kq = tid - jj * a.nprobs;
    const int col = s.col0 + jj;
    if (s.isl || col < a.np) {
      const size_t rc = (size_t)s.t * (a.np + 1) + col;
      const double x0 = (double)__uint_as_float(step_key_inverse(pfx[jj * P + 2 * kq]));
      const double x1 = (double)__uint_as_float(step_key_inverse(pfx[jj * P + 2 * kq + 1]));
      const double g = a.g[kq];
      const float mx = a.cols[rc].max;
      const double qnan = __longlong_as_double(0x7ff8000000000000ll);
      a.q[rc * a.nprobs + kq] = mx != mx ? qnan : (g == 0.0 || x0 == x1) ? x0 : x0 + g * (x1 - x0);
    }
  }
}

// ---- the row sweep.  grid = (T, chunks); workgroup (t, y) takes chains [y cpw, (y + 1) cpw), then chunks * cpw further on, ...
struct StepRowArgs {
  const float *x, *ly;       // x[T][nc][np], ly[T][nc]
  unsigned long long *part;  // [T][chunks][ROW_WORDS]
  int nc, np, lg, chunks;    // G = 1 << lg lanes per chain
};

// Every lane of a wavefront goes round the chain loop the same number of times (the ballots are the wavefront's); a lane
// without a chain or without a column contributes "unchanged".
template <int V> __global__ void __launch_bounds__(SB) k_step_rows(const StepRowArgs a)
{
  __shared__ unsigned int s_cnt;
  __shared__ unsigned long long s_best;
  const int G = 1 << a.lg, tid = (int)threadIdx.x, j = tid & (G - 1), np = a.np, nc = a.nc, cpw = SB >> a.lg;
  const int64_t t = blockIdx.x;
  const int first = (tid & 63) & ~(G - 1);  // the group's first lane in its wavefront
  const unsigned long long gmask = (G == 64 ? ~0ull : (1ull << G) - 1ull) << first;
  if (tid == 0) {
    s_cnt = 0u;
    s_best = 0ull;
  }
  __syncthreads();
  const float *x1 = a.x + (size_t)t * nc * np, *l1 = a.ly + (size_t)t * nc;
  const bool cmp = t > 0;  // (the first step of the range has no step before it)
  const float *x0 = cmp ? x1 - (size_t)nc * np : x1, *l0 = cmp ? l1 - nc : l1;
  unsigned int cnt = 0u;
  unsigned long long best = 0ull;  // (below every real entry: a key is never 0 with ~chain = 0)
  for (int64_t base = (int64_t)blockIdx.y * cpw; base < nc; base += (int64_t)a.chunks * cpw) {
    const int64_t chain = base + (tid >> a.lg);
    const bool ok = chain < nc;
    bool ch = false;
#pragma unroll
    for (int r = 0; r < V; ++r) {
      const int c = j + r * G;
      if (ok && c <= np) {
        const bool par = c < np;
        const size_t at = par ? (size_t)chain * np + c : (size_t)chain;
        const uint32_t cur = __float_as_uint(par ? x1[at] : l1[at]);
        const uint32_t prev = __float_as_uint(par ? x0[at] : l0[at]);
        ch = ch || cur != prev;
        if (!par) {
          const unsigned long long e = ((unsigned long long)step_key_bits(cur) << 32) | (unsigned long long)(~(uint32_t)chain);
          best = e > best ? e : best;
        }
      }
    }
    const bool moved = (__ballot(ch) & gmask) != 0ull;
    if (ok && j == 0 && moved) ++cnt;
  }
  if (cnt) atomicAdd(&s_cnt, cnt);
  if (best) atomicMax(&s_best, best);
  __syncthreads();
  if (tid == 0) {
    unsigned long long *o = a.part + ((size_t)t * a.chunks + blockIdx.y) * ROW_WORDS;
    o[0] = (unsigned long long)s_cnt;
    o[1] = s_best;
  }
}

// out[t] = (the sum of the chunks' counts, the maximum of their entries).  grid = ceil(T / SB)
__global__ void __launch_bounds__(SB) k_step_rows_reduce(const unsigned long long *part, int64_t T, int chunks, unsigned long long *out)
{
  const int64_t t = (int64_t)blockIdx.x * SB + threadIdx.x;
  if (t >= T) return;
  const unsigned long long *p = part + (size_t)t * chunks * ROW_WORDS;
  unsigned long long cnt = 0ull, best = 0ull;
  for (int y = 0; y < chunks; ++y) {
    cnt += p[y * ROW_WORDS];
    best = p[y * ROW_WORDS + 1] > best ? p[y * ROW_WORDS + 1] : best;
  }
  out[t * ROW_WORDS] = cnt;
  out[t * ROW_WORDS + 1] = best;
}

int launch_rows(hipStream_t st, const StepGeometry &g, int64_t T, const StepRowArgs &a)
{
  const dim3 grid((unsigned)T, (unsigned)g.chunks);
  switch (g.rows.V) {
  case 1: hipLaunchKernelGGL(k_step_rows<1>, grid, dim3(SB), 0, st, a); break;
  case 2: hipLaunchKernelGGL(k_step_rows<2>, grid, dim3(SB), 0, st, a); break;
  case 3: hipLaunchKernelGGL(k_step_rows<3>, grid, dim3(SB), 0, st, a); break;
  case 4: hipLaunchKernelGGL(k_step_rows<4>, grid, dim3(SB), 0, st, a); break;
  case 5: hipLaunchKernelGGL(k_step_rows<5>, grid, dim3(SB), 0, st, a); break;
  default: return fail(MCX_ERR_INVALID, "np = %d: a step table takes rows of 1 to 256 parameters", a.np);
  }
  HIPCHK(hipGetLastError());
  return MCX_OK;
}

// what a table call refuses before a device is touched
int table_args(int nsteps, const double *probs, int nprobs, const mcx_step_col *cols, const mcx_step_row *steps, const double *quantiles)
{
  if (!cols || !steps) return fail(MCX_ERR_INVALID, "cols or steps is NULL");
  if (nsteps < 1) return fail(MCX_ERR_INVALID, "nsteps = %d: a range of at least one step", nsteps);
  char msg[160];
  if (mcx_steptable_host::probs_args(probs, nprobs, msg, sizeof msg) != MCX_OK) return fail(MCX_ERR_INVALID, "%s", msg);
  if (nprobs > 0 && !quantiles) return fail(MCX_ERR_INVALID, "quantiles is NULL with nprobs = %d", nprobs);
  return MCX_OK;
}

// ms (mcx_debug_step_table_times, else NULL): ms[0] the moments sweep, ms[1] the select sweep, ms[2] the row sweep and its
// reducer (HIP events), ms[3] the whole call (wall clock)
int steps_span(hipStream_t st, Bufs B, const StoreView &v, const double *probs, int nprobs, mcx_step_col *cols, mcx_step_row *steps,
               double *quantiles, double *ms = nullptr)
{
  using clk = std::chrono::steady_clock;
  const clk::time_point t_call = clk::now();
  StageTimer tm{st, ms, 4, {}};
  const int nc = v.nc, np = v.np, ncol = v.ncol;
  const int64_t T = v.T;
  if (np < 1 || np > 256) return fail(MCX_ERR_INVALID, "np = %d: a step table takes rows of 1 to 256 parameters", np);
  const StepGeometry g = step_geometry(np, T, nc, nprobs);
  if (g.mwg > 0x7fffffffll || g.swg > 0x7fffffffll)
    return fail(MCX_ERR_UNSUPPORTED, "step table: %lld steps of %d columns are more (step, column tile) pairs than a grid holds",
                (long long)T, ncol);
  static_assert(sizeof(mcx_step_col) == 4 * sizeof(double), "cols[T][ncol] is four doubles' worth each in the scratch");
  const size_t ncols = (size_t)T * ncol, nq = ncols * (size_t)nprobs, nw = (size_t)T * ROW_WORDS;
  MCXCHK(B.d->alloc(g.nd));
  MCXCHK(B.h->alloc(g.nh));
  mcx_step_col *dcols = reinterpret_cast<mcx_step_col *>(B.d->p);
  double *dq = B.d->p + ncols * 4;
  unsigned long long *part = B.h->p, *dwords = B.h->p + (size_t)T * g.chunks * ROW_WORDS;
  StepSelArgs sa{v.x, v.ly, dcols, dq, nc, np, g.sct, g.stiles, nprobs, {}, {}};
  for (int k = 0; k < nprobs; ++k) {  // section 9's rule with N = nc
    const double h = (double)(nc - 1) * probs[k], lo = std::floor(h);
    sa.rank[2 * k] = (int)std::min<int64_t>((int64_t)lo, nc - 1);
    sa.rank[2 * k + 1] = (int)std::min<int64_t>((int64_t)lo + 1, nc - 1);
    sa.g[k] = h - lo;
  }
  const StepRowArgs ra{v.x, v.ly, part, nc, np, g.rows.lg, g.chunks};
  std::vector<unsigned long long> words(nw);
  auto run = [&]() -> int {
    MCXCHK(tm.run(0, [&]() -> int {
      hipLaunchKernelGGL(k_step_moments, dim3((unsigned)g.mwg), dim3(SB), 0, st, v.x, v.ly, nc, np, g.mct, g.mtiles, dcols);
      HIPCHK(hipGetLastError());
      return MCX_OK;
    }));
    if (nprobs > 0)
      MCXCHK(tm.run(1, [&]() -> int {
        hipLaunchKernelGGL(k_step_select, dim3((unsigned)g.swg), dim3(SB), g.slds, st, sa);
        HIPCHK(hipGetLastError());
        return MCX_OK;
      }));
    MCXCHK(tm.run(2, [&]() -> int {
      MCXCHK(launch_rows(st, g, T, ra));
      hipLaunchKernelGGL(k_step_rows_reduce, dim3((unsigned)((T + SB - 1) / SB)), dim3(SB), 0, st, (const unsigned long long *)part, T,
                         g.chunks, dwords);
      HIPCHK(hipGetLastError());
      return MCX_OK;
    }));
    HIPCHK(hipMemcpyAsync(cols, dcols, ncols * sizeof(mcx_step_col), hipMemcpyDeviceToHost, st));
    if (nq) HIPCHK(hipMemcpyAsync(quantiles, dq, nq * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(words.data(), dwords, nw * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MCX_OK;
  };
  const int rc = run();
  if (rc != MCX_OK) (void)hipStreamSynchronize(st);  // (cols, quantiles and words are the copies' until here)
  MCXCHK(rc);
  for (int64_t t = 0; t < T; ++t) {
    const unsigned long long *w = words.data() + (size_t)t * ROW_WORDS;
    const uint32_t key = (uint32_t)(w[1] >> 32);
    const bool llnan = key == 0xffffffffu;
    const uint32_t bits = llnan ? 0x7fc00000u : step_key_inverse(key);
    mcx_step_row &r = steps[t];
    r.moved = t == 0 ? -1 : (int)w[0];
    memcpy(&r.ll_max, &bits, sizeof bits);
    r.ll_max_chain = llnan ? -1 : (int)~(uint32_t)w[1];
    r.flags = 0;
    for (int c = 0; c < ncol; ++c) r.flags |= cols[(size_t)t * ncol + c].flags;
  }
  MCXCHK(tm.collect());
  if (ms) ms[3] = std::chrono::duration<double, std::milli>(clk::now() - t_call).count();
  return MCX_OK;
}

}  // namespace

extern "C" int mcx_samples_step_table(mcx_engine *e, int first_step, int nsteps, const double *probs, int nprobs, mcx_step_col *cols,
                                      mcx_step_row *steps, double *quantiles)
{
  return on_store(
      e, first_step, nsteps, [&] { return table_args(nsteps, probs, nprobs, cols, steps, quantiles); },
      [&](hipStream_t st, Bufs B, const StoreView &v) { return steps_span(st, B, v, probs, nprobs, cols, steps, quantiles); });
}

// mcx_samples_step_table with its sweeps timed, for tools/steptable_bench.py; the table is let go
extern "C" int mcx_debug_step_table_times(mcx_engine *e, int first_step, int nsteps, const double *probs, int nprobs, double *ms)
{
  std::vector<mcx_step_col> cols;
  std::vector<mcx_step_row> steps;
  std::vector<double> q;
  return on_store(
      e, first_step, nsteps,
      [&] {
        if (!ms) return fail(MCX_ERR_INVALID, "ms is NULL");
        if (nsteps < 1) return fail(MCX_ERR_INVALID, "nsteps = %d: a range of at least one step", nsteps);
        steps.resize((size_t)nsteps);
        cols.resize(steps.size() * ((size_t)e->nparam + 1));
        q.resize(cols.size() * (size_t)std::min(std::max(nprobs, 0), MAXP) + 1);
        return table_args(nsteps, probs, nprobs, cols.data(), steps.data(), q.data());
      },
      [&](hipStream_t st, Bufs B, const StoreView &v) {
        return steps_span(st, B, v, probs, nprobs, cols.data(), steps.data(), q.data(), ms);
      });
}

extern "C" int mcx_rows_step_table(const float *rows, int nsteps, int nc, int np, const double *probs, int nprobs, mcx_step_col *cols,
                                   mcx_step_row *steps, double *quantiles)
{
  MCXCHK(table_args(nsteps, probs, nprobs, cols, steps, quantiles));
  return on_rows(rows, nsteps, nc, np, [&](hipStream_t st, Bufs B, const StoreView &v) {
    return steps_span(st, B, v, probs, nprobs, cols, steps, quantiles);
  });
}

extern "C" int mcx_store_step_table(mcx_store *s, const double *probs, int nprobs, mcx_step_col *cols, mcx_step_row *steps,
                                    double *quantiles)
{
  if (!s) return fail(MCX_ERR_INVALID, "the store s is NULL");
  MCXCHK(table_args(s->T, probs, nprobs, cols, steps, quantiles));
  HIPCHK(hipSetDevice(s->device));
  return steps_span(s->st, s->bufs(), StoreView(s->span()), probs, nprobs, cols, steps, quantiles);
}

// host only
extern "C" int mcx_steps_settle(int nsteps, int ncol, const mcx_step_col *cols, const mcx_step_rule *rule, mcx_step_settle_col *out_cols,
                                int *settled_step)
{
  char msg[160];
  const int rc = mcx_steptable_host::settle(nsteps, ncol, cols, rule, out_cols, settled_step, msg, sizeof msg);
  return rc == MCX_OK ? MCX_OK : fail(rc, "%s", msg);
}

// host only
extern "C" int mcx_debug_steptable_geometry(int np, int nsteps, int nc, int nprobs, mcx_steptable_geometry *g)
{
  if (!g) return fail(MCX_ERR_INVALID, "g is NULL");
  if (np < 1 || np > 256) return fail(MCX_ERR_INVALID, "np = %d: 1 to 256 parameters", np);
  if (nsteps < 1 || nc < 1) return fail(MCX_ERR_INVALID, "nsteps = %d, nc = %d: at least one step of one chain", nsteps, nc);
  if (nprobs < 0 || nprobs > MAXP) return fail(MCX_ERR_INVALID, "nprobs = %d: 0 to %d probabilities", nprobs, MAXP);
  const StepGeometry s = step_geometry(np, nsteps, nc, nprobs);
  g->block = SB;
  g->moments_tile_cols = s.mct;
  g->moments_stride_chains = s.mcg;
  g->moments_col_tiles = s.mtiles;
  g->moments_workgroups = s.mwg;
  g->moments_lds_bytes = (long long)s.mlds;
  g->select_slots = s.P;
  g->select_tile_cols = s.sct;
  g->select_stride_chains = s.scg;
  g->select_col_tiles = s.stiles;
  g->select_workgroups = s.swg;
  g->select_lds_bytes = (long long)s.slds;
  g->rows_lanes_per_chain = s.rows.G;
  g->rows_values_per_lane = s.rows.V;
  g->rows_chains_per_pass = s.rows.cpw;
  g->rows_chunks = s.chunks;
  g->rows_workgroups = s.rwg;
  g->scratch_doubles = (long long)s.nd;
  g->scratch_words = (long long)s.nh;
  return MCX_OK;
}
