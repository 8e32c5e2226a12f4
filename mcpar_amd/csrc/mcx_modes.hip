// mcx_modes.hip -- mcx_samples_modes / mcx_rows_modes / mcx_store_modes and the label handle they make:
// the rows of a step range partitioned into K clusters by Lloyd's k-means, the table of the modes, and what the chains did
// among them.
//
// One call:
//   1. summary_spread (mcx_summary.hip)   the sd of every column -> the scale s (spec->scale), section 9's bits
//   2. the seed: spec->centres, or mcx_modes_host::seed on a sample fetched by section 12's gather
//   3. k_modes_assign, once per Lloyd pass: a workgroup stages R consecutive rows in LDS (section 12's tile copy), a lane
//      keeps eight running distances of its row at a time, the labels go to the handle's byte per row, and the lanes, remapped
//      to (row subgroup, column), add u to LDS accumulators that have one writer each; k_sum_rows adds the workgroups' slabs.
//      The host divides: c_k <- S_k / n_k
//   4. k_modes_table: the same structure with the final labels: centred squares, d2, log L
// and from the labels alone k_modes_chains, k_modes_steps (integers), k_modes_mark (section 14's keep mask of one mode, which
// rowset_from_mask turns into a row set) and k_modes_indicator.
// Float sums have one writer and a fixed order, counts are integers: the bytes do not depend on scheduling.
#include "mcx_derive.hpp"
#include "mcx_store.hpp"

#include "mcx_modes_host.hpp"

#include <chrono>
#include <limits>

struct mcx_modes {
  int device = 0, nc = 0, np = 0, K = 0;
  long long T = 0;
  DevBuf<uint8_t> lab;  // [T * nc]
  DevStream st;
  uint64_t rows() const { return (uint64_t)T * (uint64_t)nc; }
  ~mcx_modes()
  {
    if (st) (void)hipStreamSynchronize(st);  // (before the members go)
  }
};

namespace {

namespace mh = mcx_modes_host;

constexpr int MB = DERIVE_BLOCK;  // threads per workgroup of the two sweeps
constexpr int MODES_KB = 8;       // running distances of a lane
constexpr int MODES_WG = 1024;    // workgroups of a sweep at most: as many slabs
constexpr int MODES_NONE = mh::NONE;
constexpr int MODES_ACC = 2048;   // doubles of the assign pass' LDS accumulators at most (beyond one subgroup's K np): 16 KiB, so
                                  // that four workgroups share a CU at K = 32 as they do at K = 8
constexpr int MODES_SB = 8;       // rows of a subgroup whose labels and values are read before its accumulators are touched
constexpr int MODES_SPW = 4;      // steps per workgroup of k_modes_steps: one per wavefront

// the geometry of the sweeps over N rows of np parameters and K modes: what is launched and what mcx_debug_modes_geometry reports
struct ModesGeometry {
  int R, lgR, Q, nkb, uni;  // rows per tile (the clip's), 256 / R lane groups, centre blocks, wave-uniform centre loads
  int gA;                   // row subgroups of the assign pass' sums: 256 / np, fewer where K np of them pass MODES_ACC doubles
  int ncsT, cwT, gT;        // the table pass: np + 2 values per row, min(ncsT, 256) columns at a time, 256 / cwT subgroups (MODES_ACC too)
  size_t ldsA, ldsT;
  uint64_t ntiles;
  unsigned nwg;
};
ModesGeometry modes_geometry(int np, uint64_t N, int K)
{
  ModesGeometry g;
  g.R = derive_rows(np, 0);
  g.lgR = 0;
  while ((1 << g.lgR) < g.R) ++g.lgR;
  g.Q = MB >> g.lgR;
  g.nkb = (K + MODES_KB - 1) / MODES_KB;
  g.uni = g.R >= 64 ? 1 : 0;
  g.gA = std::max(1, std::min(MB / np, MODES_ACC / (K * np)));
  g.ncsT = np + 2;
  g.cwT = std::min(g.ncsT, MB);
  g.gT = std::max(1, std::min(MB / g.cwT, MODES_ACC / (K * g.ncsT)));
  const size_t sx = (size_t)(np | 1);
  g.ldsA = ((size_t)g.gA * K * np + np) * sizeof(double) + (size_t)g.R * sx * sizeof(float);
  g.ldsT = ((size_t)g.gT * K * g.ncsT + np) * sizeof(double) + (size_t)g.R * (sx + 1) * sizeof(float);
  g.ntiles = sweep_tiles(N, g.R);
  g.nwg = (unsigned)std::min<uint64_t>(g.ntiles, MODES_WG);
  return g;
}

__device__ __forceinline__ bool modes_nonfinite_bits(uint32_t b) { return (b & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ bool modes_nan_bits(uint32_t b) { return (b & 0x7fffffffu) > 0x7f800000u; }
__device__ __forceinline__ uint32_t modes_order_key(uint32_t b) { return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u); }

struct AssignArgs {
  const float *x;           // x[N][np]
  uint8_t *lab;             // [N]: read (the pass before), then written
  double *d2;               // [N] or NULL: d2 of the winner
  double *slab;             // [K * np][nslab]
  unsigned long long *cnt;  // n[K], then n_changed, then n_nonfinite
  uint64_t N, ntiles;
  int np, K, R, lgR, G;
  unsigned nslab;
};

// grid = nslab workgroups; workgroup w takes tiles w, w + nslab, ...  ct[nkb][np][8]: the scaled centres in blocks of eight,
// a block's eight values of one column side by side (a block's tail repeats the last centre and is not looked at); s[np].
// Both are read only and passed apart from the struct as __restrict__, so that no store of the kernel stands between a load
// and its use: with UNI (R >= 64, so tid >> lgR is one value per wavefront) a column's eight centres are one scalar load
template <bool UNI>
__global__ void __launch_bounds__(MB) k_modes_assign(const AssignArgs a, const double *__restrict__ ct, const double *__restrict__ s)
{
  extern __shared__ double modes_lds[];
  __shared__ double bd[MB];
  __shared__ int bk[MB], labs[MB], nfs[MB];
  __shared__ unsigned cnt[mh::MAX_K + 2];
  const int np = a.np, K = a.K, R = a.R, G = a.G, sx = np | 1, tid = (int)threadIdx.x;
  double *acc = modes_lds, *sl = acc + (size_t)G * K * np;
  float *xs = reinterpret_cast<float *>(sl + np);
  for (int i = tid; i < G * K * np; i += MB) acc[i] = 0.0;
  for (int i = tid; i < np; i += MB) sl[i] = s[i];
  if (tid < K + 2) cnt[tid] = 0u;
  const int r = tid & (R - 1), Q = MB >> a.lgR, nkb = (K + MODES_KB - 1) / MODES_KB;
  int q = tid >> a.lgR;
  if (UNI) q = __builtin_amdgcn_readfirstlane(q);
  const int g = tid / np, col = tid - g * np;  // the lane's part in the sums
  const double inf = __longlong_as_double(0x7ff0000000000000ll), qnan = __longlong_as_double(0x7ff8000000000000ll);
  for (uint64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const uint64_t row0 = t * (uint64_t)R, left = a.N - row0;
    const int rows = left < (uint64_t)R ? (int)left : R;
    const float *gx = a.x + row0 * (uint64_t)np;
    __syncthreads();  // (the tile before is read no more; the first time: acc, sl and cnt are set)
    derive_tile_copy<true>(xs, sx, const_cast<float *>(gx), np, rows * np, ((unsigned long)gx & 15ul) == 0);
    if (tid < R) nfs[tid] = 0;
    __syncthreads();
    const bool mine = r < rows;
    const float *xr = xs + (mine ? r : 0) * sx;
    bool bad = false;
    for (int j = q; j < np; j += Q) bad = bad || modes_nonfinite_bits(__float_as_uint(xr[j]));
    if (mine && bad) nfs[r] = 1;  // (every writer stores the same)
    const int prev = mine && tid < R ? (int)a.lab[row0 + r] : MODES_NONE;  // (asked for here, needed behind the distances)
    double best = inf;
    int bestk = MODES_NONE;
    for (int kb = q; kb < nkb; kb += Q) {
      const int k0 = kb * MODES_KB;
      double d[MODES_KB];
#pragma unroll
      for (int i = 0; i < MODES_KB; ++i) d[i] = 0.0;
      const double *cb = ct + (size_t)kb * np * MODES_KB;
      // A column with s_j = 0 is not skipped by a branch: its u is +-0 for a finite row and its centres are 0 (block_centres),
      // so e e = +0 and d + 0 = d in every bit.  A row that is not finite is MODE_NONE whatever d says
#pragma unroll 2
      for (int j = 0; j < np; ++j) {
        double cj[MODES_KB];
#pragma unroll
        for (int i = 0; i < MODES_KB; ++i) cj[i] = cb[j * MODES_KB + i];
        const double u = __dmul_rn((double)xr[j], sl[j]);
#pragma unroll
        for (int i = 0; i < MODES_KB; ++i) {
          const double e = __dsub_rn(u, cj[i]);
          d[i] = __dadd_rn(d[i], __dmul_rn(e, e));
        }
      }
#pragma unroll
      for (int i = 0; i < MODES_KB; ++i) {
        const int k = k0 + i;
        if (k < K && (d[i] < best || (d[i] == best && k < bestk))) {
          best = d[i];
          bestk = k;
        }
      }
    }
    bd[tid] = best;
    bk[tid] = bestk;
    __syncthreads();
    if (tid < R) {  // the lanes of group 0: r = tid
      int l = MODES_NONE;
      if (mine) {
        for (int qq = 1; qq < Q; ++qq) {
          const double dq = bd[qq * R + r];
          const int kq = bk[qq * R + r];
          if (dq < best || (dq == best && kq < bestk)) {
            best = dq;
            bestk = kq;
          }
        }
        l = nfs[r] ? MODES_NONE : bestk;
        a.lab[row0 + r] = (uint8_t)l;
        if (a.d2) a.d2[row0 + r] = l == MODES_NONE ? qnan : best;
        atomicAdd(&cnt[l == MODES_NONE ? K + 1 : l], 1u);
        if (l != prev) atomicAdd(&cnt[K], 1u);
      }
      labs[r] = l;
    }
    __syncthreads();
    // the subgroup's rows in row order, MODES_SB at a time: their labels and values are read first, so that what waits on LDS is
    // the chain of an accumulator alone
    if (g < G) {
      const double sc = sl[col];
      double *pa = acc + (size_t)g * K * np + col;
      for (int r0 = g; r0 < rows; r0 += MODES_SB * G) {
        int l[MODES_SB];
        float xv[MODES_SB];
#pragma unroll
        for (int i = 0; i < MODES_SB; ++i) {
          const int rr = r0 + i * G;
          l[i] = rr < rows ? labs[rr] : MODES_NONE;
          xv[i] = xs[(rr < rows ? rr : 0) * sx + col];
        }
#pragma unroll
        for (int i = 0; i < MODES_SB; ++i)
          if (l[i] != MODES_NONE) {
            double *p = pa + l[i] * np;
            *p = __dadd_rn(*p, __dmul_rn((double)xv[i], sc));
          }
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < K * np; i += MB) {
    double sum = 0.0;
    for (int gg = 0; gg < G; ++gg) sum += acc[(size_t)gg * K * np + i];
    a.slab[(size_t)i * a.nslab + blockIdx.x] = sum;
  }
  if (tid < K + 2 && cnt[tid]) atomicAdd(&a.cnt[tid], (unsigned long long)cnt[tid]);
}

struct TableArgs {
  const float *x, *ly;
  const uint8_t *lab;
  double *slab;                // [K * ncs][nslab]
  unsigned long long *cnt;     // members whose log L is not finite [K], then is NaN [K]
  unsigned long long *best;    // [nslab][K][2]: 1 << 32 | the order key of the best log L (0: no member), its first row
  uint64_t N, ntiles;
  int np, K, R, G, CW, ncs;
  unsigned nslab;
};

// the table pass: per mode and column the sum of (u - mean)^2, then the sum of d2, then the sum of log L.  c, mean: the centres
// and the member means [K][np], scaled; s[np]: read only, __restrict__ as in k_modes_assign
__global__ void __launch_bounds__(MB) k_modes_table(const TableArgs a, const double *__restrict__ c, const double *__restrict__ s,
                                                    const double *__restrict__ mean)
{
  extern __shared__ double modes_lds[];
  __shared__ double d2s[MB];
  __shared__ int labs[MB];
  __shared__ unsigned llc[2 * mh::MAX_K];
  __shared__ unsigned long long tkey[mh::MAX_K];
  const int np = a.np, K = a.K, R = a.R, G = a.G, CW = a.CW, ncs = a.ncs, sx = np | 1, tid = (int)threadIdx.x;
  double *acc = modes_lds, *sl = acc + (size_t)G * K * ncs;
  float *xs = reinterpret_cast<float *>(sl + np), *lys = xs + (size_t)R * sx;
  for (int i = tid; i < G * K * ncs; i += MB) acc[i] = 0.0;
  for (int i = tid; i < np; i += MB) sl[i] = s[i];
  if (tid < 2 * K) llc[tid] = 0u;
  const int g = tid / CW, cl = tid - g * CW;
  unsigned long long bestkey = 0ull, bestrow = 0ull;  // of mode tid, in its thread
  for (uint64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const uint64_t row0 = t * (uint64_t)R, left = a.N - row0;
    const int rows = left < (uint64_t)R ? (int)left : R;
    const float *gx = a.x + row0 * (uint64_t)np;
    __syncthreads();
    if (tid < rows) lys[tid] = a.ly[row0 + tid];
    derive_tile_copy<true>(xs, sx, const_cast<float *>(gx), np, rows * np, ((unsigned long)gx & 15ul) == 0);
    if (tid < K) tkey[tid] = 0ull;
    __syncthreads();
    if (tid < R) {
      int l = MODES_NONE;
      double d = 0.0;
      if (tid < rows) l = (int)a.lab[row0 + tid];
      if (l != MODES_NONE) {
        const float *xr = xs + tid * sx;
        const double *ck = c + (size_t)l * np;
        for (int j = 0; j < np; ++j) {
          const double sj = sl[j];
          if (sj == 0.0) continue;
          const double e = __dsub_rn(__dmul_rn((double)xr[j], sj), ck[j]);
          d = __dadd_rn(d, __dmul_rn(e, e));
        }
        const uint32_t b = __float_as_uint(lys[tid]);
        if (modes_nonfinite_bits(b)) atomicAdd(&llc[l], 1u);
        if (modes_nan_bits(b)) atomicAdd(&llc[K + l], 1u);
        atomicMax(&tkey[l], ((unsigned long long)modes_order_key(b) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)tid));
      }
      labs[tid] = l;
      d2s[tid] = d;
    }
    __syncthreads();
    if (tid < K) {
      const unsigned long long tk = tkey[tid];
      if (tk) {
        const unsigned long long key = (1ull << 32) | (tk >> 32);
        if (key > bestkey) {  // (tiles come in ascending order: the first row stays)
          bestkey = key;
          bestrow = row0 + (unsigned long long)(0xffffffffu - (uint32_t)tk);
        }
      }
    }
    if (g < G)
      for (int rr = g; rr < rows; rr += G) {
        const int l = labs[rr];
        if (l == MODES_NONE) continue;
        for (int cc = cl; cc < ncs; cc += CW) {
          double v;
          if (cc < np) {
            const double e = __dsub_rn(__dmul_rn((double)xs[rr * sx + cc], sl[cc]), mean[(size_t)l * np + cc]);
            v = __dmul_rn(e, e);
          } else v = cc == np ? d2s[rr] : (double)lys[rr];
          double *p = acc + ((size_t)g * K + l) * ncs + cc;
          *p = __dadd_rn(*p, v);
        }
      }
  }
  __syncthreads();
  for (int i = tid; i < K * ncs; i += MB) {
    double sum = 0.0;
    for (int gg = 0; gg < G; ++gg) sum += acc[(size_t)gg * K * ncs + i];
    a.slab[(size_t)i * a.nslab + blockIdx.x] = sum;
  }
  if (tid < 2 * K && llc[tid]) atomicAdd(&a.cnt[tid], (unsigned long long)llc[tid]);
  if (tid < K) {
    unsigned long long *o = a.best + ((size_t)blockIdx.x * K + tid) * 2;
    o[0] = bestkey;
    o[1] = bestrow;
  }
}

// ---- from the labels alone
constexpr int CHAIN_MODE_WORDS = 3;  // u64 words of a chain: hops, dominant_steps, dominant | first << 8 | last << 16

// grid = ceil(nc / MB): one lane per chain walks its T labels.  vis[K][MB] in LDS, a column per lane; tr[K][K] LDS counters
__global__ void __launch_bounds__(MB) k_modes_chains(const uint8_t *lab, int nc, int K, int64_t T, unsigned long long *chains,
                                                     unsigned long long *visits, unsigned long long *trans)
{
  extern __shared__ unsigned modes_vis[];
  __shared__ unsigned long long tr[mh::MAX_K * mh::MAX_K];
  const int tid = (int)threadIdx.x, chain = (int)blockIdx.x * MB + tid;
  for (int k = 0; k < K; ++k) modes_vis[k * MB + tid] = 0u;
  for (int i = tid; i < K * K; i += MB) tr[i] = 0ull;
  __syncthreads();
  if (chain < nc) {
    int prev = (int)lab[chain];
    const int first = prev;
    unsigned long long hops = 0ull;
    if (prev != MODES_NONE) modes_vis[prev * MB + tid] += 1u;
    for (int64_t t = 1; t < T; ++t) {
      const int cur = (int)lab[(size_t)t * nc + chain];
      if (cur != MODES_NONE) {
        modes_vis[cur * MB + tid] += 1u;
        if (prev != MODES_NONE) {
          atomicAdd(&tr[prev * K + cur], 1ull);
          if (cur != prev) ++hops;
        }
      }
      prev = cur;
    }
    unsigned bestv = 0u;
    int dom = MODES_NONE;
    for (int k = 0; k < K; ++k) {
      const unsigned v = modes_vis[k * MB + tid];
      visits[(size_t)chain * K + k] = (unsigned long long)v;
      if (v > bestv) {
        bestv = v;
        dom = k;
      }
    }
    unsigned long long *o = chains + (size_t)chain * CHAIN_MODE_WORDS;
    o[0] = hops;
    o[1] = (unsigned long long)bestv;
    o[2] = (unsigned long long)dom | ((unsigned long long)first << 8) | ((unsigned long long)prev << 16);
  }
  __syncthreads();
  for (int i = tid; i < K * K; i += MB)
    if (tr[i]) atomicAdd(&trans[i], tr[i]);
}

// grid = ceil(T / MODES_SPW): a wavefront counts the chains of one step
__global__ void __launch_bounds__(MB) k_modes_steps(const uint8_t *lab, int nc, int K, int64_t T, unsigned long long *occ)
{
  __shared__ unsigned oc[MODES_SPW][mh::MAX_K];
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (tid < MODES_SPW * mh::MAX_K) oc[tid / mh::MAX_K][tid % mh::MAX_K] = 0u;
  __syncthreads();
  const int64_t t0 = (int64_t)blockIdx.x * MODES_SPW, t = t0 + wave;
  if (t < T)
    for (int c = lane; c < nc; c += 64) {
      const int l = (int)lab[(size_t)t * nc + c];
      if (l != MODES_NONE) atomicAdd(&oc[wave][l], 1u);
    }
  __syncthreads();
  if (tid < MODES_SPW * K) {
    const int w = tid / K, k = tid - w * K;
    if (t0 + w < T) occ[(size_t)(t0 + w) * K + k] = (unsigned long long)oc[w][k];
  }
}

// section 14's keep mask of mode k in the clip's geometry: grid = ceil(N / R), mask[wg][wpw], cnt[wg]
__global__ void __launch_bounds__(MB) k_modes_mark(const uint8_t *lab, uint64_t N, int R, int wpw, int k, unsigned long long *mask,
                                                   uint32_t *cnt)
{
  __shared__ unsigned wkept[MB / 64];
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint64_t row0 = (uint64_t)blockIdx.x * (uint64_t)R, left = N - row0;
  const int rows = left < (uint64_t)R ? (int)left : R;
  if (wave < wpw) {
    const bool keep = tid < rows && (int)lab[row0 + (tid < rows ? tid : 0)] == k;
    const unsigned long long kb = __ballot(keep);
    if (lane == 0) {
      mask[(uint64_t)blockIdx.x * wpw + wave] = kb;
      wkept[wave] = (unsigned)__popcll(kb);
    }
  } else if (lane == 0) wkept[wave] = 0u;
  __syncthreads();
  if (tid == 0) {
    unsigned n = 0;
    for (int w = 0; w < MB / 64; ++w) n += wkept[w];
    cnt[blockIdx.x] = n;
  }
}

// x'[N][K]: 1 in the column of the row's label; ly' = 0
__global__ void __launch_bounds__(MB) k_modes_indicator(const uint8_t *lab, uint64_t N, int K, float *x, float *ly)
{
  const uint64_t i = (uint64_t)blockIdx.x * MB + threadIdx.x;
  if (i >= N * (uint64_t)K) return;
  const uint64_t row = i / (uint64_t)K;
  const int k = (int)(i - row * (uint64_t)K);
  x[i] = (int)lab[row] == k ? 1.0f : 0.0f;
  if (k == 0) ly[row] = 0.0f;
}

int modes_fail(int rc, const char *msg) { return rc == mh::OK ? MCX_OK : fail(MCX_ERR_INVALID, "%s", msg); }

// where a call's results go
struct ModesOut {
  mcx_modes_result *res;
  mcx_mode_row *table;
  double *cs, *c, *means, *sds, *scale;
  mcx_modes **out;
};

// what can be refused before a device is touched
int modes_args(const mcx_modes_spec *spec, const ModesOut &o, int nsteps, int nc, int np)
{
  if (!spec || !o.res || !o.table || !o.cs || !o.c || !o.means || !o.sds || !o.scale)
    return fail(MCX_ERR_INVALID, "spec, res, table, centres_scaled, centres, means, sds or scale is NULL");
  if (nsteps < 1) return fail(MCX_ERR_INVALID, "nsteps = %d: a range of at least one step", nsteps);
  if (np < 1 || np > DERIVE_MAXW) return fail(MCX_ERR_INVALID, "np = %d: modes take rows of 1 to %d parameters", np, DERIVE_MAXW);
  char msg[160];
  MCXCHK(modes_fail(mh::spec_check(spec->k, spec->max_iter, spec->seed_rows, spec->centres, np, (long long)nsteps * nc, msg, sizeof msg), msg));
  if (spec->scale && (long long)nsteps * nc < 2)
    return fail(MCX_ERR_INVALID, "a scale needs nsteps * nc >= 2 rows, got %lld", (long long)nsteps * nc);
  return MCX_OK;
}

int launch_assign(hipStream_t st, const ModesGeometry &g, const AssignArgs &a, const double *ct, const double *s)
{
  // (above the 64 KiB a kernel gets unasked)
  if (g.uni) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_modes_assign<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.ldsA));
    hipLaunchKernelGGL(k_modes_assign<true>, dim3(g.nwg), dim3(MB), g.ldsA, st, a, ct, s);
  } else {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_modes_assign<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.ldsA));
    hipLaunchKernelGGL(k_modes_assign<false>, dim3(g.nwg), dim3(MB), g.ldsA, st, a, ct, s);
  }
  HIPCHK(hipGetLastError());
  return MCX_OK;
}

// out[r] = the sum of slab[r][0 .. nslab), r < nrows, by the fixed-order reducer
int reduce_slabs(hipStream_t st, const double *slab, unsigned nslab, int nrows, double *out)
{
  hipLaunchKernelGGL(k_sum_rows, dim3((unsigned)nrows), dim3(SB), 0, st, slab, (size_t)nslab, 1, 1, 1, (size_t)nslab, (size_t)nslab,
                     (const double *)nullptr, 0.0, out);
  HIPCHK(hipGetLastError());
  return MCX_OK;
}

// the scratch of a call.  doubles: c[K np] | s[np] | mean[K np] | ct[nkb np 8] | slab[K ncsT nslab] | red[K ncsT]; u64 words:
// cnt[2 K + 2] | best[nslab K 2]
struct ModesScratch {
  size_t o_s, o_mean, o_ct, o_slab, o_red, nd, o_best, nh;
};
// c[K][np] -> ct[nkb][np][8], a block's tail filled with the last centre; 0 in a column that takes no part (s_j = 0), which is
// what makes the kernel's unconditional sum the definition's skip
void block_centres(int K, int np, const double *c, const double *s, std::vector<double> &ct)
{
  const int nkb = (K + MODES_KB - 1) / MODES_KB;
  ct.resize((size_t)nkb * np * MODES_KB);
  for (int kb = 0; kb < nkb; ++kb)
    for (int j = 0; j < np; ++j)
      for (int i = 0; i < MODES_KB; ++i)
        ct[((size_t)kb * np + j) * MODES_KB + i] = s[j] == 0.0 ? 0.0 : c[(size_t)std::min(kb * MODES_KB + i, K - 1) * np + j];
}
ModesScratch modes_scratch(const ModesGeometry &g, int np, int K)
{
  ModesScratch s;
  s.o_s = (size_t)K * np;
  s.o_mean = s.o_s + np;
  s.o_ct = s.o_mean + (size_t)K * np;
  s.o_slab = s.o_ct + (size_t)g.nkb * np * MODES_KB;
  s.o_red = s.o_slab + (size_t)K * g.ncsT * g.nwg;
  s.nd = s.o_red + (size_t)K * g.ncsT;
  s.o_best = (size_t)2 * K + 2;
  s.nh = s.o_best + (size_t)g.nwg * K * 2;
  return s;
}

// ms (mcx_debug_modes_times, else NULL): ms[0] the scale, ms[1] the seed (wall clock), ms[2] the assign passes, ms[3] their
// reducers, ms[4] the table pass and its reducer (HIP events), ms[7] the whole call (wall clock)
int modes_span(hipStream_t st, Bufs B, const StoreSpan &v, const mcx_modes_spec *spec, const ModesOut &o, double *ms = nullptr)
{
  using clk = std::chrono::steady_clock;
  auto since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
  const clk::time_point t_call = clk::now();
  StageTimer tm{st, ms, MCX_MODES_TIMES, {}};
  const int np = v.np, nc = v.nc, K = spec->k;
  const uint64_t N = (uint64_t)v.T * (uint64_t)nc;
  const double qnan = std::numeric_limits<double>::quiet_NaN();

  // ---- 1. the scale
  std::vector<double> s((size_t)np, 1.0);
  if (spec->scale) {
    std::vector<mcx_col_summary> sc((size_t)np + 1);
    MCXCHK(summary_spread(st, B, v, nullptr, 0, sc.data(), nullptr));
    for (int j = 0; j < np; ++j) s[(size_t)j] = mh::scale_of_sd(sc[(size_t)j].sd);
  }
  const double ms_scale = since(t_call);

  // ---- 2. the seed
  const clk::time_point t_seed = clk::now();
  std::vector<double> c((size_t)K * np);
  if (spec->centres) {
    for (int k = 0; k < K; ++k)
      for (int j = 0; j < np; ++j) c[(size_t)k * np + j] = spec->centres[(size_t)k * np + j] * s[(size_t)j];
  } else {
    const uint64_t M = std::min<uint64_t>(N, (uint64_t)spec->seed_rows);
    std::vector<float> rows((size_t)M * ((size_t)np + 1));
    MCXCHK(gather_span(st, v, N > M, spec->seed, 0, M, rows.data(), nullptr));
    std::vector<long long> idx((size_t)K);
    char msg[160];
    MCXCHK(modes_fail(mh::seed(rows.data(), (long long)M, np, K, spec->seed, s.data(), idx.data(), msg, sizeof msg), msg));
    for (int k = 0; k < K; ++k)
      for (int j = 0; j < np; ++j) c[(size_t)k * np + j] = (double)rows[(size_t)idx[(size_t)k] * ((size_t)np + 1) + j] * s[(size_t)j];
  }
  const double ms_seed = since(t_seed);

  // ---- 3. the Lloyd passes
  const ModesGeometry g = modes_geometry(np, N, K);
  const ModesScratch L = modes_scratch(g, np, K);
  std::unique_ptr<mcx_modes> m(new mcx_modes);
  HIPCHK(hipGetDevice(&m->device));
  m->nc = nc; m->np = np; m->K = K; m->T = (long long)v.T;
  MCXCHK(m->st.ensure(hipStreamNonBlocking));
  MCXCHK(m->lab.alloc((size_t)N));
  MCXCHK(B.d->alloc(L.nd));
  MCXCHK(B.h->alloc(L.nh));
  double *D = B.d->p;
  unsigned long long *H = B.h->p;
  AssignArgs a{v.x, m->lab.p, nullptr, D + L.o_slab, H, N, g.ntiles, np, K, g.R, g.lgR, g.gA, g.nwg};
  std::vector<double> S((size_t)K * np), red((size_t)K * g.ncsT), ct;
  std::vector<unsigned long long> cnt((size_t)2 * K + 2);
  std::vector<long long> n((size_t)K);
  mcx_modes_result &res = *o.res;
  res = mcx_modes_result{};
  res.k = K;
  res.n = (long long)N;
  auto pass = [&]() -> int {
    block_centres(K, np, c.data(), s.data(), ct);
    HIPCHK(hipMemcpyAsync(D, c.data(), c.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(D + L.o_ct, ct.data(), ct.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(H, 0, ((size_t)K + 2) * sizeof(unsigned long long), st));
    MCXCHK(tm.run(2, [&]() -> int { return launch_assign(st, g, a, D + L.o_ct, D + L.o_s); }));
    MCXCHK(tm.run(3, [&]() -> int { return reduce_slabs(st, D + L.o_slab, g.nwg, K * np, D + L.o_red); }));
    HIPCHK(hipMemcpyAsync(S.data(), D + L.o_red, S.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(cnt.data(), H, ((size_t)K + 2) * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MCX_OK;
  };
  auto loop = [&]() -> int {
    HIPCHK(hipMemcpyAsync(D + L.o_s, s.data(), s.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(m->lab.p, 0xff, (size_t)N, st));  // (before the first pass every label is MCX_MODE_NONE)
    for (int it = 1;; ++it) {
      MCXCHK(pass());
      for (int k = 0; k < K; ++k) {
        n[(size_t)k] = (long long)cnt[(size_t)k];
        if (n[(size_t)k] == 0) res.flags |= MCX_MODES_EMPTY;
      }
      res.iters = it;
      res.n_changed = (long long)cnt[(size_t)K];
      res.n_nonfinite = (long long)cnt[(size_t)K + 1];
      if (res.n_changed == 0) {
        res.flags |= MCX_MODES_CONVERGED;
        break;
      }
      if (it == spec->max_iter) {
        res.flags |= MCX_MODES_NOT_CONVERGED;
        break;
      }
      mh::update_centres(K, np, n.data(), S.data(), c.data());
    }
    return MCX_OK;
  };

  // ---- 4. the table pass
  std::vector<double> mean((size_t)K * np, 0.0);
  std::vector<unsigned long long> best((size_t)g.nwg * K * 2);
  auto table = [&]() -> int {
    for (int k = 0; k < K; ++k)
      if (n[(size_t)k] > 0)
        for (int j = 0; j < np; ++j) mean[(size_t)k * np + j] = S[(size_t)k * np + j] / (double)n[(size_t)k];
    TableArgs t{v.x, v.ly, m->lab.p, D + L.o_slab, H, H + L.o_best, N, g.ntiles,
                np, K, g.R, g.gT, g.cwT, g.ncsT, g.nwg};
    HIPCHK(hipMemcpyAsync(D + L.o_mean, mean.data(), mean.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(H, 0, (size_t)2 * K * sizeof(unsigned long long), st));
    MCXCHK(tm.run(4, [&]() -> int {
      HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_modes_table), hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.ldsT));
      hipLaunchKernelGGL(k_modes_table, dim3(g.nwg), dim3(MB), g.ldsT, st, t, (const double *)D, (const double *)(D + L.o_s),
                         (const double *)(D + L.o_mean));
      HIPCHK(hipGetLastError());
      return reduce_slabs(st, D + L.o_slab, g.nwg, K * g.ncsT, D + L.o_red);
    }));
    HIPCHK(hipMemcpyAsync(red.data(), D + L.o_red, red.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(cnt.data(), H, (size_t)2 * K * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(best.data(), H + L.o_best, best.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MCX_OK;
  };
  int rc = loop();
  if (rc == MCX_OK) rc = table();
  if (rc != MCX_OK) (void)hipStreamSynchronize(st);  // (the host vectors are the copies' until here)
  MCXCHK(rc);

  // ---- the finish
  const long long nvalid = (long long)N - res.n_nonfinite;
  res.inertia = 0.0;
  for (int k = 0; k < K; ++k) {
    mcx_mode_row &r = o.table[k];
    const long long nk = n[(size_t)k];
    const double *rk = red.data() + (size_t)k * g.ncsT;
    r = mcx_mode_row{};
    r.n = nk;
    r.weight = nvalid > 0 ? (double)nk / (double)nvalid : qnan;
    r.flags = nk == 0 ? MCX_MODES_EMPTY : 0;
    r.ll_max_row = -1;
    r.ll_max = std::numeric_limits<float>::quiet_NaN();
    r.inertia = nk > 0 ? rk[np] : qnan;
    r.ll_mean = nk > 0 && cnt[(size_t)k] == 0 ? rk[np + 1] / (double)nk : qnan;
    if (nk > 0) res.inertia += rk[np];
    uint32_t bits = 0;
    long long row = -1;
    if (nk > 0 && cnt[(size_t)K + k] == 0 && mh::best_ll(best.data() + (size_t)k * 2, g.nwg, (size_t)K * 2, &bits, &row)) {
      memcpy(&r.ll_max, &bits, sizeof bits);
      r.ll_max_row = row;
    }
    for (int j = 0; j < np; ++j) {
      const size_t i = (size_t)k * np + j;
      const double sj = s[(size_t)j];
      const bool part = sj != 0.0;
      o.cs[i] = c[i];
      o.c[i] = part ? c[i] / sj : qnan;
      o.means[i] = part && nk > 0 ? mean[i] / sj : qnan;
      o.sds[i] = part && nk > 0 ? std::sqrt(rk[j] / (double)(nk - 1)) / sj : qnan;
    }
  }
  for (int j = 0; j < np; ++j) o.scale[j] = s[(size_t)j];
  MCXCHK(tm.collect());
  if (ms) {
    ms[0] = ms_scale;
    ms[1] = ms_seed;
    ms[7] = since(t_call);
  }
  if (o.out) *o.out = m.release();  // (the unique_ptr's: the handle is the caller's now)
  return MCX_OK;
}

int modes_enter(const mcx_modes *m)
{
  if (!m) return fail(MCX_ERR_INVALID, "the modes handle m is NULL");
  HIPCHK(hipSetDevice(m->device));
  return MCX_OK;
}

// what mode_rows refuses before a device is touched
int mode_rows_args(const mcx_modes *m, int k, mcx_rowset **out, long long nsteps, int nc, int np)
{
  if (!m || !out) return fail(MCX_ERR_INVALID, "the modes handle m or out is NULL");
  if (k < 0 || k >= m->K) return fail(MCX_ERR_INVALID, "k = %d is not a mode of the handle (0 to %d)", k, m->K - 1);
  if (nsteps != m->T || nc != m->nc || np != m->np)
    return fail(MCX_ERR_INVALID, "a source of %lld steps of %d chains of %d columns, but the labels are of %lld x %d x %d", nsteps, nc,
                np + 1, m->T, m->nc, m->np + 1);
  return MCX_OK;
}

// the rows of mode k of span s: the mask label == k in section 14's geometry, then its scan and scatter.  u64 scratch:
// mask[nwg][wpw] | rowset_scan's words; u32: cnt[nwg]
int mode_rows_span(hipStream_t st, Bufs B, const StoreSpan &s, const mcx_modes *m, int k, mcx_rowset **out)
{
  const uint64_t N = m->rows();
  const ClipGeometry g = clip_geometry(s.np, N);
  if (g.nwg > 0x7fffffffull)
    return fail(MCX_ERR_UNSUPPORTED, "mode rows: %llu rows in tiles of %d are more workgroups than a grid holds", (unsigned long long)N, g.R);
  const size_t nmask = (size_t)g.nwg * g.wpw;
  MCXCHK(B.h->alloc(nmask + rowset_scan_words(g)));
  MCXCHK(B.u->alloc((size_t)g.nwg));
  hipLaunchKernelGGL(k_modes_mark, dim3((unsigned)g.nwg), dim3(MB), 0, st, (const uint8_t *)m->lab.p, N, g.R, g.wpw, k, B.h->p, B.u->p);
  HIPCHK(hipGetLastError());
  return rowset_from_mask(st, s, RowMask{B.h->p, B.u->p, B.h->p + nmask}, g, out);
}

}  // namespace

extern "C" int mcx_samples_modes(mcx_engine *e, int first_step, int nsteps, const mcx_modes_spec *spec, mcx_modes_result *res,
                                 mcx_mode_row *table, double *centres_scaled, double *centres, double *means, double *sds,
                                 double *scale, mcx_modes **out)
{
  const ModesOut o{res, table, centres_scaled, centres, means, sds, scale, out};
  return on_store(
      e, first_step, nsteps, [&] { return modes_args(spec, o, nsteps, e->nchain, e->nparam); },
      [&](hipStream_t st, Bufs B, const StoreView &v) { return modes_span(st, B, v, spec, o); });
}

extern "C" int mcx_debug_modes_times(mcx_engine *e, int first_step, int nsteps, const mcx_modes_spec *spec, mcx_modes_result *res,
                                     double *ms)
{
  std::vector<mcx_mode_row> table;
  std::vector<double> w;
  ModesOut o{};
  return on_store(
      e, first_step, nsteps,
      [&] {
        if (!ms || !spec || !res) return fail(MCX_ERR_INVALID, "ms, spec or res is NULL");
        // (sized before modes_args has seen k: within what it can accept, so that a wild k is refused, not allocated for)
        const size_t K = (size_t)std::min(std::max(spec->k, 1), (int)MCX_MODES_MAX_K), np = (size_t)e->nparam;
        table.resize(K);
        w.resize(4 * K * np + np);
        o = ModesOut{res, table.data(), w.data(), w.data() + K * np, w.data() + 2 * K * np, w.data() + 3 * K * np, w.data() + 4 * K * np, nullptr};
        return modes_args(spec, o, nsteps, e->nchain, e->nparam);
      },
      [&](hipStream_t st, Bufs B, const StoreView &v) { return modes_span(st, B, v, spec, o, ms); });
}

extern "C" int mcx_rows_modes(const float *rows, int nsteps, int nc, int np, const mcx_modes_spec *spec, mcx_modes_result *res,
                              mcx_mode_row *table, double *centres_scaled, double *centres, double *means, double *sds, double *scale,
                              mcx_modes **out)
{
  const ModesOut o{res, table, centres_scaled, centres, means, sds, scale, out};
  MCXCHK(modes_args(spec, o, nsteps, nc, np));
  return on_rows(rows, nsteps, nc, np, [&](hipStream_t st, Bufs B, const StoreView &v) { return modes_span(st, B, v, spec, o); });
}

extern "C" int mcx_store_modes(mcx_store *s, const mcx_modes_spec *spec, mcx_modes_result *res, mcx_mode_row *table,
                               double *centres_scaled, double *centres, double *means, double *sds, double *scale, mcx_modes **out)
{
  if (!s) return fail(MCX_ERR_INVALID, "the store s is NULL");
  const ModesOut o{res, table, centres_scaled, centres, means, sds, scale, out};
  MCXCHK(modes_args(spec, o, s->T, s->nc, s->nout));
  HIPCHK(hipSetDevice(s->device));
  return modes_span(s->st, s->bufs(), s->span(), spec, o);
}

extern "C" int mcx_modes_destroy(mcx_modes *m)
{
  if (!m) return MCX_OK;
  (void)hipSetDevice(m->device);
  delete m;
  return MCX_OK;
}

extern "C" int mcx_modes_shape(const mcx_modes *m, int *nsteps, int *nc, int *ncol, int *k)
{
  if (!m) return fail(MCX_ERR_INVALID, "the modes handle m is NULL");
  if (nsteps) *nsteps = (int)m->T;
  if (nc) *nc = m->nc;
  if (ncol) *ncol = m->np + 1;
  if (k) *k = m->K;
  return MCX_OK;
}

extern "C" int mcx_modes_labels(mcx_modes *m, long long first_row, long long nrows, unsigned char *labels)
{
  if (!m) return fail(MCX_ERR_INVALID, "the modes handle m is NULL");
  const long long N = (long long)m->rows();
  if (first_row < 0 || nrows < 0 || first_row > N || nrows > N - first_row)
    return fail(MCX_ERR_INVALID, "rows [%lld,%lld) not among the labels (%lld rows)", first_row, first_row + nrows, N);
  if (nrows == 0) return MCX_OK;
  if (!labels) return fail(MCX_ERR_INVALID, "labels is NULL with nrows = %lld", nrows);
  MCXCHK(modes_enter(m));
  HIPCHK(hipMemcpyAsync(labels, m->lab.p + first_row, (size_t)nrows, hipMemcpyDeviceToHost, m->st));
  HIPCHK(hipStreamSynchronize(m->st));
  return MCX_OK;
}

extern "C" int mcx_modes_chain_table(mcx_modes *m, mcx_mode_chain *chains, long long *visits, long long *trans, long long *occupancy)
{
  MCXCHK(modes_enter(m));
  const int nc = m->nc, K = m->K;
  const int64_t T = m->T;
  const size_t o_vis = (size_t)nc * CHAIN_MODE_WORDS, o_tr = o_vis + (size_t)nc * K, o_occ = o_tr + (size_t)K * K,
               nh = o_occ + (size_t)T * K;
  DevBuf<unsigned long long> h;
  MCXCHK(h.alloc(nh));
  std::vector<unsigned long long> w(nh);
  hipStream_t st = m->st;
  auto run = [&]() -> int {
    HIPCHK(hipMemsetAsync(h.p + o_tr, 0, (size_t)K * K * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_modes_chains, dim3((unsigned)((nc + MB - 1) / MB)), dim3(MB), (size_t)K * MB * sizeof(unsigned), st,
                       (const uint8_t *)m->lab.p, nc, K, T, h.p, h.p + o_vis, h.p + o_tr);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_modes_steps, dim3((unsigned)((T + MODES_SPW - 1) / MODES_SPW)), dim3(MB), 0, st, (const uint8_t *)m->lab.p, nc, K,
                       T, h.p + o_occ);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(w.data(), h.p, nh * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    return MCX_OK;
  };
  const int rc = run();
  const hipError_t es = hipStreamSynchronize(st);  // (before w and h may go)
  MCXCHK(rc);
  HIPCHK(es);
  if (chains)
    for (int c = 0; c < nc; ++c) {
      const unsigned long long *p = w.data() + (size_t)c * CHAIN_MODE_WORDS;
      mcx_mode_chain &r = chains[c];
      r = mcx_mode_chain{};
      r.hops = (long long)p[0];
      r.dominant_steps = (long long)p[1];
      r.dominant = (int)(p[2] & 0xffull);
      r.first_label = (int)((p[2] >> 8) & 0xffull);
      r.last_label = (int)((p[2] >> 16) & 0xffull);
    }
  if (visits)
    for (size_t i = 0; i < (size_t)nc * K; ++i) visits[i] = (long long)w[o_vis + i];
  if (trans)
    for (size_t i = 0; i < (size_t)K * K; ++i) trans[i] = (long long)w[o_tr + i];
  if (occupancy)
    for (size_t i = 0; i < (size_t)T * K; ++i) occupancy[i] = (long long)w[o_occ + i];
  return MCX_OK;
}

extern "C" int mcx_modes_indicator_store(mcx_modes *m, mcx_store **out)
{
  if (!m || !out) return fail(MCX_ERR_INVALID, "the modes handle m or out is NULL");
  MCXCHK(modes_enter(m));
  const uint64_t N = m->rows(), n = N * (uint64_t)m->K;
  if ((n + MB - 1) / MB > 0x7fffffffull)
    return fail(MCX_ERR_UNSUPPORTED, "indicators: %llu values are more workgroups than a grid holds", (unsigned long long)n);
  std::unique_ptr<mcx_store> o(new mcx_store);
  o->device = m->device; o->nc = m->nc; o->nout = m->K; o->T = (int)m->T;
  MCXCHK(o->st.ensure(hipStreamNonBlocking));
  MCXCHK(o->x.alloc((size_t)n));
  MCXCHK(o->ly.alloc((size_t)N));
  hipLaunchKernelGGL(k_modes_indicator, dim3((unsigned)((n + MB - 1) / MB)), dim3(MB), 0, m->st, (const uint8_t *)m->lab.p, N, m->K,
                     o->x.p, o->ly.p);
  const hipError_t el = hipGetLastError(), es = hipStreamSynchronize(m->st);  // (before the new store may go)
  HIPCHK(el);
  HIPCHK(es);
  *out = o.release();
  return MCX_OK;
}

extern "C" int mcx_samples_mode_rows(mcx_engine *e, int first_step, int nsteps, mcx_modes *m, int k, mcx_rowset **out)
{
  return on_store(
      e, first_step, nsteps, [&] { return mode_rows_args(m, k, out, nsteps, e->nchain, e->nparam); },
      [&](hipStream_t st, Bufs B, const StoreView &v) { return mode_rows_span(st, B, v, m, k, out); });
}

extern "C" int mcx_rows_mode_rows(const float *rows, int nsteps, int nc, int np, mcx_modes *m, int k, mcx_rowset **out)
{
  MCXCHK(mode_rows_args(m, k, out, nsteps, nc, np));
  return on_rows(rows, nsteps, nc, np, [&](hipStream_t st, Bufs B, const StoreView &v) { return mode_rows_span(st, B, v, m, k, out); });
}

extern "C" int mcx_store_mode_rows(mcx_store *s, mcx_modes *m, int k, mcx_rowset **out)
{
  if (!s) return fail(MCX_ERR_INVALID, "the store s is NULL");
  MCXCHK(mode_rows_args(m, k, out, s->T, s->nc, s->nout));
  HIPCHK(hipSetDevice(s->device));
  return mode_rows_span(s->st, s->bufs(), s->span(), m, k, out);
}

// host only
extern "C" int mcx_modes_seed(const float *rows, long long nrows, int np, int k, uint32_t seed, const double *s, long long *index)
{
  if (!rows || !s || !index) return fail(MCX_ERR_INVALID, "rows, s or index is NULL");
  if (np < 1 || np > DERIVE_MAXW) return fail(MCX_ERR_INVALID, "np = %d: 1 to %d parameters", np, DERIVE_MAXW);
  if (k < 1 || k > MCX_MODES_MAX_K) return fail(MCX_ERR_INVALID, "k = %d: 1 to %d modes", k, MCX_MODES_MAX_K);
  if (nrows < 1) return fail(MCX_ERR_INVALID, "nrows = %lld: at least one row", nrows);
  char msg[160];
  return modes_fail(mh::seed(rows, nrows, np, k, seed, s, index, msg, sizeof msg), msg);
}

extern "C" int mcx_debug_modes_assign(const float *rows, int nsteps, int nc, int np, int k, const double *centres_scaled, const double *s,
                                      unsigned char *labels, double *d2, long long *n, double *S)
{
  if (!centres_scaled || !s) return fail(MCX_ERR_INVALID, "centres_scaled or s is NULL");
  if (k < 1 || k > MCX_MODES_MAX_K) return fail(MCX_ERR_INVALID, "k = %d: 1 to %d modes", k, MCX_MODES_MAX_K);
  if (nsteps < 1) return fail(MCX_ERR_INVALID, "nsteps = %d: a range of at least one step", nsteps);
  return on_rows(rows, nsteps, nc, np, [&](hipStream_t st, Bufs B, const StoreView &v) -> int {
    const uint64_t N = (uint64_t)v.N;
    const ModesGeometry g = modes_geometry(np, N, k);
    const ModesScratch L = modes_scratch(g, np, k);
    DevBuf<uint8_t> lab;
    DevBuf<double> dd;
    MCXCHK(lab.alloc((size_t)N));
    MCXCHK(dd.alloc((size_t)N));
    MCXCHK(B.d->alloc(L.nd));
    MCXCHK(B.h->alloc(L.nh));
    double *D = B.d->p;
    unsigned long long *H = B.h->p;
    const AssignArgs a{v.x, lab.p, dd.p, D + L.o_slab, H, N, g.ntiles, np, k, g.R, g.lgR, g.gA, g.nwg};
    std::vector<unsigned long long> cnt((size_t)k + 2);
    std::vector<double> ct;
    block_centres(k, np, centres_scaled, s, ct);
    auto run = [&]() -> int {
      HIPCHK(hipMemcpyAsync(D + L.o_ct, ct.data(), ct.size() * sizeof(double), hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(D + L.o_s, s, (size_t)np * sizeof(double), hipMemcpyHostToDevice, st));
      HIPCHK(hipMemsetAsync(lab.p, 0xff, (size_t)N, st));
      HIPCHK(hipMemsetAsync(H, 0, cnt.size() * sizeof(unsigned long long), st));
      MCXCHK(launch_assign(st, g, a, D + L.o_ct, D + L.o_s));
      MCXCHK(reduce_slabs(st, D + L.o_slab, g.nwg, k * np, D + L.o_red));
      if (labels) HIPCHK(hipMemcpyAsync(labels, lab.p, (size_t)N, hipMemcpyDeviceToHost, st));
      if (d2) HIPCHK(hipMemcpyAsync(d2, dd.p, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
      if (S) HIPCHK(hipMemcpyAsync(S, D + L.o_red, (size_t)k * np * sizeof(double), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(cnt.data(), H, cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
      return MCX_OK;
    };
    const int rc = run();
    const hipError_t es = hipStreamSynchronize(st);  // (before lab, dd and cnt may go)
    MCXCHK(rc);
    HIPCHK(es);
    if (n)
      for (int i = 0; i < k; ++i) n[i] = (long long)cnt[(size_t)i];
    return MCX_OK;
  });
}

// host only
extern "C" int mcx_debug_modes_geometry(int np, int nsteps, int nc, int k, mcx_modes_geometry *out)
{
  if (!out) return fail(MCX_ERR_INVALID, "g is NULL");
  if (np < 1 || np > DERIVE_MAXW) return fail(MCX_ERR_INVALID, "np = %d: 1 to %d parameters", np, DERIVE_MAXW);
  if (nsteps < 1 || nc < 1) return fail(MCX_ERR_INVALID, "nsteps = %d, nc = %d: at least one step of one chain", nsteps, nc);
  if (k < 1 || k > MCX_MODES_MAX_K) return fail(MCX_ERR_INVALID, "k = %d: 1 to %d modes", k, MCX_MODES_MAX_K);
  const uint64_t N = (uint64_t)nsteps * (uint64_t)nc;
  const ModesGeometry g = modes_geometry(np, N, k);
  const ModesScratch L = modes_scratch(g, np, k);
  const ClipGeometry c = clip_geometry(np, N);
  out->block = MB;
  out->rows_per_tile = g.R;
  out->tiles = (long long)g.ntiles;
  out->workgroups = g.nwg;
  out->lane_groups = g.Q;
  out->centre_blocks = g.nkb;
  out->uniform_centres = g.uni;
  out->sum_subgroups = g.gA;
  out->table_columns = g.ncsT;
  out->table_subgroups = g.gT;
  out->assign_lds_bytes = (long long)g.ldsA;
  out->table_lds_bytes = (long long)g.ldsT;
  out->mark_workgroups = (long long)c.nwg;
  out->mark_mask_words = c.wpw;
  out->chains_workgroups = (nc + MB - 1) / MB;
  out->steps_workgroups = (nsteps + MODES_SPW - 1) / MODES_SPW;
  out->scratch_bytes = (long long)(L.nd * sizeof(double) + L.nh * sizeof(unsigned long long));
  return MCX_OK;
}
