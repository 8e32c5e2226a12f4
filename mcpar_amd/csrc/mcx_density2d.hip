// mcx_density2d.hip -- mcx_samples_density2d / mcx_rows_density2d / density2d_span: per pair of columns of a step range of the
// sample store, the binned product-Gaussian kernel density estimate of MASS::kde2d with bandwidth.nrd (what geom_density_2d
// evaluates), on the g x g nodes of the two columns' grids.  DESIGN.md section 15 restates every definition.
//
// One call:
//   1. summary_spread (mcx_summary.hip)  the statistics of section 13: moments, min, max, the quartiles, the clip pair
//   2. mcx_debug_density2d_grid          host, per column: bandwidth.nrd / 4, from / to, the grid [lo, up] of g nodes
//   3. k_density2d_codes                 one read of the store: every value of every column that occurs in a pair becomes one
//                                        u32 (its slot and its fixed-point fraction on its column's grid), column-major
//   4. k_density2d_pairs                 a workgroup owns one pair and walks row chunks: the pair's (g + 1)^2 slots in LDS,
//                                        two 64-bit LDS adds per row, drained into a slab of the workgroup's own per chunk
//   5. k_density2d_reduce                the slabs of a pair added in a fixed order
//   6. mcx_debug_density2d_finish        host, per pair: the node masses in integers, the separable fp64 convolution
// Integer adds only on the device, so the same store and arguments give the same bytes.
#include "mcx_summary_kernels.hpp"

#include <chrono>
#include <limits>

namespace {

constexpr int GMIN = 8, GMAX = 64;   // grid nodes per axis
constexpr int MAXPAIRS = 1024;
constexpr int FBITS = 12;            // F = 4096: a value's fraction between two nodes in fixed point
constexpr double FD = (double)(1 << FBITS);
// a code: slot s = floor(xpos) + 1 in [0, g] above WBITS, w = floor(frac * F) in [0, F] below (w = F where xpos - floor(xpos)
// rounds to 1.0); all ones for a value that is not on its column's grid
constexpr int WBITS = FBITS + 1;
constexpr uint32_t CODE_OFF = 0xffffffffu;
static_assert((1 << FBITS) < (1 << WBITS), "w <= F fits its field");
static_assert(((uint32_t)GMAX << WBITS | (1u << FBITS)) < 0x80000000u, "bit 31 is set in CODE_OFF alone");

// Rows of one pair that a workgroup bins between zeroing and draining its LDS.  A slot is two u64 words:
//   word 0 = cnt << CNT_SHIFT | Sab,  word 1 = Sa << SA_SHIFT | Sb
// A row adds w_a * w_b <= F^2 = 2^24 to Sab and w_a, w_b <= F = 2^12 to Sa, Sb.
constexpr int64_t PCHUNK = 1 << 16;
constexpr int CNT_SHIFT = 41, SA_SHIFT = 32;
static_assert(PCHUNK * (1ll << (2 * FBITS)) < (1ll << CNT_SHIFT), "Sab of a chunk stays below the count");
static_assert(PCHUNK < (1ll << (64 - CNT_SHIFT)), "the count of a chunk stays inside the word");
static_assert(PCHUNK * (1ll << FBITS) < (1ll << SA_SHIFT), "Sb of a chunk stays below Sa");
static_assert(PCHUNK * (1ll << FBITS) < (1ll << (64 - SA_SHIFT)), "Sa of a chunk stays inside the word");
static_assert(PCHUNK % 4 == 0, "a chunk starts on a 16-byte boundary of a code column");

constexpr int PB = 1024;             // threads of a pair workgroup: two of them fill a CU's LDS at g = 64
constexpr int TARGET_WGS = 1024;     // pair workgroups of a launch, about
constexpr size_t pair_lds_bytes(int g) { return (size_t)(g + 1) * (g + 1) * 2 * sizeof(unsigned long long); }
static_assert(pair_lds_bytes(GMAX) == 67600 && 2 * pair_lds_bytes(GMAX) <= 160 * 1024, "two workgroups per CU at g = 64");

// ---- 3. the code sweep ----------------------------------------------------------------------------------------------------
// The store is x[N][np] and ly[N], N = T * nc rows: a tile of TR rows by tc <= TCMAX columns is read along the rows, turned in
// LDS and written along the columns.  grid = (ceil(N / TR), ceil(ncol / tc)).  grid2[col] = (lo, inv); cmap[col] = the
// column's index among the code columns, -1 for a column in no pair
constexpr int TR = 128, TCMAX = 32;

__device__ __forceinline__ uint32_t code_of(float v, double lo, double inv, int g)
{
  const double xpos = ((double)v - lo) * inv;      // (-ffp-contract=off: a subtraction and a multiplication)
  if (!(xpos >= -1.0 && xpos < (double)g)) return CODE_OFF;  // a NaN fails both
  const double fl = floor(xpos);
  const uint32_t w = (uint32_t)((xpos - fl) * FD);
  return ((uint32_t)((int)fl + 1) << WBITS) | w;
}

__global__ void __launch_bounds__(SB) k_density2d_codes(const float *x, const float *ly, int np, int64_t N, int64_t npad, int g,
                                                        int tc, const double *grid2, const int *cmap, uint32_t *code)
{
  __shared__ uint32_t tile[TCMAX * (TR + 1)];
  __shared__ double glo[TCMAX], ginv[TCMAX];
  __shared__ int gmap[TCMAX];
  const int64_t row0 = (int64_t)blockIdx.x * TR;
  const int col0 = (int)blockIdx.y * tc;
  const int ncs = min(tc, np + 1 - col0);
  const int nr = (int)min((int64_t)TR, N - row0);
  if ((int)threadIdx.x < ncs) {
    glo[threadIdx.x] = grid2[2 * (col0 + threadIdx.x)];
    ginv[threadIdx.x] = grid2[2 * (col0 + threadIdx.x) + 1];
    gmap[threadIdx.x] = cmap[col0 + threadIdx.x];
  }
  __syncthreads();
  // element e = lr * ncs + lc of the tile, e = thread, thread + SB, ...: the two indices are stepped, not divided out
  const int dq = SB / ncs, dr = SB - dq * ncs;
  int lr = (int)threadIdx.x / ncs, lc = (int)threadIdx.x - lr * ncs;
  while (lr < nr) {
    uint32_t cd = CODE_OFF;
    if (gmap[lc] >= 0) {
      const int64_t row = row0 + lr;
      const int col = col0 + lc;
      const float v = col < np ? x[(size_t)row * np + col] : ly[row];
      cd = code_of(v, glo[lc], ginv[lc], g);
    }
    tile[lc * (TR + 1) + lr] = cd;
    lr += dq;
    lc += dr;
    if (lc >= ncs) {
      lc -= ncs;
      ++lr;
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < ncs * TR; e += SB) {
    const int c = e / TR, r = e - c * TR;
    const int ci = gmap[c];
    if (r < nr && ci >= 0) code[(size_t)ci * npad + row0 + r] = tile[c * (TR + 1) + r];
  }
}

// ---- 4. the pair sweep ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ void add_row(unsigned long long *acc, uint32_t a, uint32_t b, int g1)
{
  if ((int32_t)(a | b) < 0) return;  // one of the two values is not on its grid
  const uint32_t wa = a & ((1u << WBITS) - 1), wb = b & ((1u << WBITS) - 1);
  unsigned long long *s = acc + 2 * ((a >> WBITS) * g1 + (b >> WBITS));
  atomicAdd(s, (1ull << CNT_SHIFT) + (unsigned long long)(wa * wb));
  atomicAdd(s + 1, ((unsigned long long)wa << SA_SHIFT) + wb);
}

// grid = npairs * W, workgroup = w * npairs + pair: the pairs of one row chunk are neighbours in the launch order and read
// the chunk's codes from L2.  Workgroup (pair, w) walks the chunks w, w + W, ... and owns slab[workgroup][(g + 1)^2][4] =
// (cnt, Sa, Sb, Sab); pc[pair] = the pair's two code columns
__global__ void __launch_bounds__(PB) k_density2d_pairs(const uint32_t *code, int64_t N, int64_t npad, int g, int npairs,
                                                        const int *pc, int W, int64_t nchunks, unsigned long long *slab)
{
  extern __shared__ unsigned long long acc[];  // [(g + 1)^2][2]
  const int pair = (int)(blockIdx.x % (unsigned)npairs), w = (int)(blockIdx.x / (unsigned)npairs);
  const int g1 = g + 1, nslot = g1 * g1;
  const uint32_t *ca = code + (size_t)pc[2 * pair] * npad, *cb = code + (size_t)pc[2 * pair + 1] * npad;
  unsigned long long *out = slab + (size_t)blockIdx.x * nslot * 4;
  for (int i = threadIdx.x; i < 2 * nslot; i += PB) acc[i] = 0ull;
  __syncthreads();
  bool first = true;
  for (int64_t ch = w; ch < nchunks; ch += W) {
    const int64_t r0 = ch * PCHUNK, r1 = min(N, r0 + PCHUNK);
    for (int64_t r = r0 + 4 * (int64_t)threadIdx.x; r < r1; r += 4 * PB) {
      if (r + 4 <= r1) {
        const uint4 a = *reinterpret_cast<const uint4 *>(ca + r), b = *reinterpret_cast<const uint4 *>(cb + r);
        add_row(acc, a.x, b.x, g1);
        add_row(acc, a.y, b.y, g1);
        add_row(acc, a.z, b.z, g1);
        add_row(acc, a.w, b.w, g1);
      } else {
        for (int64_t q = r; q < r1; ++q) add_row(acc, ca[q], cb[q], g1);
      }
    }
    __syncthreads();
    // the drain: plain stores and adds, this workgroup alone touches its slab
    for (int i = threadIdx.x; i < nslot; i += PB) {
      const unsigned long long a0 = acc[2 * i], a1 = acc[2 * i + 1];
      const unsigned long long cnt = a0 >> CNT_SHIFT, sab = a0 & ((1ull << CNT_SHIFT) - 1);
      const unsigned long long sa = a1 >> SA_SHIFT, sb = a1 & ((1ull << SA_SHIFT) - 1);
      unsigned long long *o = out + 4 * (size_t)i;
      if (first) {  // (every slot, so that the slab needs no zeroing)
        o[0] = cnt; o[1] = sa; o[2] = sb; o[3] = sab;
      } else if (a0) {
        o[0] += cnt; o[1] += sa; o[2] += sb; o[3] += sab;
      }
      if (a0) {  // (a slot without a row has both words 0)
        acc[2 * i] = 0ull; acc[2 * i + 1] = 0ull;
      }
    }
    first = false;
    __syncthreads();
  }
}

// ---- 5. out[pair][slot][4] = the sum over w of slab[w * npairs + pair][slot][4], w ascending; n = npairs * per ------------
__global__ void __launch_bounds__(SB) k_density2d_reduce(const unsigned long long *slab, size_t n, int W, unsigned long long *out)
{
  const size_t i = (size_t)blockIdx.x * SB + threadIdx.x;
  if (i >= n) return;
  unsigned long long s = 0ull;
  for (int w = 0; w < W; ++w) s += slab[(size_t)w * n + i];
  out[i] = s;
}

// the launch geometry of the pair sweep over N rows and npairs pairs.  A workgroup walks at least two chunks wherever there
// are two, so that the drain into a slab that already holds sums runs for every store of more than 2^16 rows
struct PairGeometry {
  int64_t nchunks;
  int W;
};
PairGeometry pair_geometry(int64_t N, int npairs)
{
  PairGeometry p;
  p.nchunks = (N + PCHUNK - 1) / PCHUNK;
  const int64_t by_chunks = (p.nchunks + 1) / 2, by_target = (TARGET_WGS + npairs - 1) / npairs;
  p.W = (int)std::max<int64_t>(1, std::min(by_chunks, by_target));
  return p;
}

inline size_t nslot_of(int g) { return (size_t)(g + 1) * (g + 1); }

// The device part: grid2 [ncol][2] (a column that is in no pair of `pairs` is not read), pairs [npairs][2] columns ->
// slots [npairs][(g + 1)^2][4].  tm: stages 1, 2, 3 are the three kernels
int bins2d_device(hipStream_t st, Bufs B, const StoreView &v, int g, const std::vector<double> &grid2, const std::vector<int> &pairs,
                  std::vector<unsigned long long> &slots, StageTimer &tm)
{
  const int npairs = (int)(pairs.size() / 2), ncol = v.ncol;
  const size_t per = nslot_of(g) * 4;
  slots.assign((size_t)npairs * per, 0ull);
  if (npairs == 0) return MCX_OK;
  // the code columns
  std::vector<int> meta(ncol, -1);
  int ncode = 0;
  for (int c = 0; c < ncol; ++c) {
    bool used = false;
    for (int p = 0; p < 2 * npairs && !used; ++p) used = pairs[p] == c;
    if (used) meta[c] = ncode++;
  }
  for (int p = 0; p < 2 * npairs; ++p) meta.push_back(meta[pairs[p]]);
  const PairGeometry pg = pair_geometry(v.N, npairs);
  const int64_t npad = (v.N + 3) / 4 * 4;
  const size_t nwg = (size_t)npairs * pg.W, ncodes = (size_t)ncode * npad, nh = (nwg + npairs) * per;
  DevBuf<int> dmeta;
  if (B.u->alloc(ncodes) != MCX_OK || B.h->alloc(nh) != MCX_OK || B.d->alloc(grid2.size()) != MCX_OK || dmeta.alloc(meta.size()) != MCX_OK)
    return fail(MCX_ERR_ALLOC, "pair densities: %zu bytes of scratch are needed (%d code columns of %lld rows, %zu slabs; DESIGN.md section 15)",
                ncodes * 4 + nh * 8 + grid2.size() * 8 + meta.size() * 4, ncode, (long long)v.N, nwg);
  HIPCHK(hipMemcpyAsync(B.d->p, grid2.data(), grid2.size() * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dmeta.p, meta.data(), meta.size() * sizeof(int), hipMemcpyHostToDevice, st));
  const int *cmap = dmeta.p, *pc = dmeta.p + ncol;
  unsigned long long *slab = B.h->p, *out = B.h->p + nwg * per;
  MCXCHK(tm.run(1, [&]() -> int {
    const int tc = std::min(ncol, TCMAX);
    hipLaunchKernelGGL(k_density2d_codes, dim3((unsigned)((v.N + TR - 1) / TR), (unsigned)((ncol + tc - 1) / tc)), dim3(SB), 0, st, v.x,
                       v.ly, v.np, v.N, npad, g, tc, (const double *)B.d->p, cmap, B.u->p);
    HIPCHK(hipGetLastError());
    return MCX_OK;
  }));
  MCXCHK(tm.run(2, [&]() -> int {
    // (above the 64 KiB a kernel gets unasked; the value is the largest the kernel can be launched with)
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_density2d_pairs), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)pair_lds_bytes(GMAX)));
    hipLaunchKernelGGL(k_density2d_pairs, dim3((unsigned)nwg), dim3(PB), pair_lds_bytes(g), st, (const uint32_t *)B.u->p, v.N, npad, g,
                       npairs, pc, pg.W, pg.nchunks, slab);
    HIPCHK(hipGetLastError());
    return MCX_OK;
  }));
  MCXCHK(tm.run(3, [&]() -> int {
    const size_t n = (size_t)npairs * per;
    hipLaunchKernelGGL(k_density2d_reduce, dim3((unsigned)((n + SB - 1) / SB)), dim3(SB), 0, st, (const unsigned long long *)slab, n, pg.W,
                       out);
    HIPCHK(hipGetLastError());
    return MCX_OK;
  }));
  HIPCHK(hipMemcpyAsync(slots.data(), out, slots.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));  // (grid2, meta and dmeta are in use until here)
  return MCX_OK;
}

// the pairs a call works on: the spec's, or every a < b in ascending order
int pair_list(int npairs, const int *pairs, int ncol, std::vector<int> &out)
{
  out.clear();
  if (!pairs) {
    if ((int64_t)ncol * (ncol - 1) / 2 > MAXPAIRS)
      return fail(MCX_ERR_INVALID, "%d columns have %lld pairs, more than %d: name the pairs (mcx_density2d_spec.pairs)", ncol,
                  (long long)ncol * (ncol - 1) / 2, MAXPAIRS);
    for (int a = 0; a < ncol; ++a)
      for (int b = a + 1; b < ncol; ++b) { out.push_back(a); out.push_back(b); }
    if (out.empty()) return fail(MCX_ERR_INVALID, "%d column has no pair", ncol);
    return MCX_OK;
  }
  if (npairs < 1 || npairs > MAXPAIRS) return fail(MCX_ERR_INVALID, "npairs = %d: 1 to %d pairs", npairs, MAXPAIRS);
  for (int p = 0; p < npairs; ++p) {
    const int a = pairs[2 * p], b = pairs[2 * p + 1];
    if (a < 0 || a >= ncol || b < 0 || b >= ncol) return fail(MCX_ERR_INVALID, "pair %d = (%d, %d): columns are 0 to %d", p, a, b, ncol - 1);
    if (a == b) return fail(MCX_ERR_INVALID, "pair %d = (%d, %d) is one column twice", p, a, b);
    out.push_back(a); out.push_back(b);
  }
  return MCX_OK;
}

inline int grid_size_args(int g)
{
  if (g < GMIN || g > GMAX) return fail(MCX_ERR_INVALID, "g = %d: %d to %d grid nodes per axis", g, GMIN, GMAX);
  return MCX_OK;
}

// the fields a pair density shares with section 13's spec, as that spec (n is not used by any of it)
inline mcx_density_spec spec1d(const mcx_density2d_spec *s) { return mcx_density_spec{2, s->adjust, s->clip_lo, s->clip_hi, s->bw, s->from, s->to}; }

// what can be refused before a device is touched; pl: the pairs of the call
int density2d_args(const mcx_density2d_spec *s, int ncol, int64_t N, const mcx_col_density *cols, const double *axes,
                   const mcx_pair_density *pairs_out, const double *z, std::vector<int> &pl)
{
  if (!s) return fail(MCX_ERR_INVALID, "the density spec is NULL");
  if (!cols || !axes || !pairs_out || !z) return fail(MCX_ERR_INVALID, "cols, axes, pairs_out or z is NULL");
  MCXCHK(grid_size_args(s->g));
  const mcx_density_spec s1 = spec1d(s);
  MCXCHK(density_spec_args(&s1, ncol, N, cols, axes, z));
  MCXCHK(pair_list(s->npairs, s->pairs, ncol, pl));
  if (N >= (1ll << 31)) return fail(MCX_ERR_UNSUPPORTED, "pair densities of %lld rows: fewer than 2^31", (long long)N);
  return MCX_OK;
}

void nan_column(mcx_col_density *col, long long N)
{
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  col->bw = col->from = col->to = col->lo = col->up = col->mean = col->sd = qnan;
  col->nvalues = N;
  col->nbinned = 0;
  col->flags = MCX_SUMMARY_NONFINITE;
}

// ms (mcx_debug_density2d_times, else NULL): ms[0] the statistics passes (wall clock), ms[1] k_density2d_codes, ms[2]
// k_density2d_pairs, ms[3] k_density2d_reduce (HIP events), ms[4] the host grids and finish (wall clock), ms[5] the whole call
int density2d_device(hipStream_t st, Bufs B, const StoreView &v, const mcx_density2d_spec *spec, const std::vector<int> &pl,
                     mcx_col_density *cols, double *axes, mcx_pair_density *pairs_out, double *z, double *ms)
{
  using clk = std::chrono::steady_clock;
  auto since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
  const clk::time_point t_call = clk::now();
  StageTimer tm{st, ms, 6, {}};
  const int ncol = v.ncol, g = spec->g, npairs = (int)(pl.size() / 2);
  const bool clip = !(spec->clip_lo == 0.0 && spec->clip_hi == 1.0);
  const double probs[4] = {0.25, 0.75, spec->clip_lo, spec->clip_hi};
  const int nprobs = clip ? 4 : 2;
  const double qnan = std::numeric_limits<double>::quiet_NaN();

  // ---- 1. moments and order statistics
  std::vector<mcx_col_summary> sc(ncol);
  std::vector<double> q((size_t)ncol * nprobs);
  MCXCHK(summary_spread(st, B, v, probs, nprobs, sc.data(), q.data()));
  const double ms_stats = since(t_call);

  // ---- 2. the grids and the axes
  clk::time_point t_host = clk::now();
  std::vector<double> grid2((size_t)ncol * 2, qnan);
  for (int c = 0; c < ncol; ++c) {
    double *ax = axes + (size_t)c * g;
    if (sc[c].flags & MCX_SUMMARY_NONFINITE) {
      nan_column(&cols[c], v.N);
      std::fill(ax, ax + g, qnan);
      continue;
    }
    const double *qc = q.data() + (size_t)c * nprobs;
    MCXCHK(mcx_debug_density2d_grid(v.N, sc[c].mean, sc[c].sd, sc[c].min, sc[c].max, qc[0], qc[1], clip ? qc[2] : qnan, clip ? qc[3] : qnan,
                                    c == ncol - 1, c, spec, &cols[c]));
    grid2[2 * c] = cols[c].lo;
    grid2[2 * c + 1] = (double)(g - 1) / (cols[c].up - cols[c].lo);
    const double delta = (cols[c].up - cols[c].lo) / (double)(g - 1);
    for (int j = 0; j < g; ++j) ax[j] = cols[c].lo + (double)j * delta;
  }
  // the pairs of two finite columns go to the device
  std::vector<int> live, where(npairs, -1);
  for (int p = 0; p < npairs; ++p) {
    if ((cols[pl[2 * p]].flags | cols[pl[2 * p + 1]].flags) & MCX_SUMMARY_NONFINITE) continue;
    where[p] = (int)(live.size() / 2);
    live.push_back(pl[2 * p]); live.push_back(pl[2 * p + 1]);
  }
  double ms_host = since(t_host);

  // ---- 3. to 5. the sweeps
  std::vector<unsigned long long> slots;
  MCXCHK(bins2d_device(st, B, v, g, grid2, live, slots, tm));

  // ---- 6. the finish
  t_host = clk::now();
  const size_t per = nslot_of(g) * 4, gg = (size_t)g * g;
  for (int p = 0; p < npairs; ++p) {
    const int a = pl[2 * p], b = pl[2 * p + 1];
    mcx_pair_density *po = &pairs_out[p];
    double *zp = z + (size_t)p * gg;
    po->a = a; po->b = b; po->nbinned = 0; po->flags = 0;
    if (where[p] < 0) {
      po->flags = MCX_SUMMARY_NONFINITE;
      std::fill(zp, zp + gg, qnan);
      continue;
    }
    const unsigned long long *sl = slots.data() + (size_t)where[p] * per;
    long long nb = 0;
    for (size_t s = 0; s < nslot_of(g); ++s) nb += (long long)sl[4 * s];
    po->nbinned = nb;
    MCXCHK(mcx_debug_density2d_finish(&cols[a], &cols[b], g, sl, a > b, zp));
  }
  ms_host += since(t_host);
  MCXCHK(tm.collect());
  if (ms) {
    ms[0] = ms_stats;
    ms[4] = ms_host;
    ms[5] = since(t_call);
  }
  return MCX_OK;
}

}  // namespace

int density2d_span(hipStream_t st, Bufs B, const StoreSpan &s, const mcx_density2d_spec *spec, mcx_col_density *cols, double *axes,
                   mcx_pair_density *pairs_out, double *z)
{
  std::vector<int> pl;
  MCXCHK(density2d_args(spec, s.np + 1, s.T * (int64_t)s.nc, cols, axes, pairs_out, z, pl));
  return density2d_device(st, B, StoreView(s), spec, pl, cols, axes, pairs_out, z, nullptr);
}

extern "C" int mcx_samples_density2d(mcx_engine *e, int first_step, int nsteps, const mcx_density2d_spec *spec, mcx_col_density *cols,
                                     double *axes, mcx_pair_density *pairs_out, double *z)
{
  std::vector<int> pl;
  return on_store(
      e, first_step, nsteps, [&] { return density2d_args(spec, e->nparam + 1, (int64_t)nsteps * e->nchain, cols, axes, pairs_out, z, pl); },
      [&](hipStream_t st, Bufs B, const StoreView &v) { return density2d_device(st, B, v, spec, pl, cols, axes, pairs_out, z, nullptr); });
}

// mcx_samples_density2d with its stages timed, for tools/density2d_bench.py; the results are let go
extern "C" int mcx_debug_density2d_times(mcx_engine *e, int first_step, int nsteps, const mcx_density2d_spec *spec, double *ms)
{
  std::vector<int> pl;
  std::vector<mcx_col_density> cols;
  std::vector<mcx_pair_density> po;
  std::vector<double> axes, z;
  return on_store(
      e, first_step, nsteps,
      [&] {
        if (!ms) return fail(MCX_ERR_INVALID, "ms is NULL");
        if (!spec) return fail(MCX_ERR_INVALID, "the density spec is NULL");
        MCXCHK(grid_size_args(spec->g));
        const int ncol = e->nparam + 1;
        MCXCHK(pair_list(spec->npairs, spec->pairs, ncol, pl));
        const size_t g = (size_t)spec->g, np = pl.size() / 2;
        cols.resize(ncol);
        axes.resize(ncol * g);
        po.resize(np);
        z.resize(np * g * g);
        return density2d_args(spec, ncol, (int64_t)nsteps * e->nchain, cols.data(), axes.data(), po.data(), z.data(), pl);
      },
      [&](hipStream_t st, Bufs B, const StoreView &v) {
        return density2d_device(st, B, v, spec, pl, cols.data(), axes.data(), po.data(), z.data(), ms);
      });
}

extern "C" int mcx_rows_density2d(const float *rows, int nsteps, int nc, int np, const mcx_density2d_spec *spec, mcx_col_density *cols,
                                  double *axes, mcx_pair_density *pairs_out, double *z)
{
  if (!rows || nc < 1 || np < 1 || np > 256) return fail(MCX_ERR_INVALID, "bad arguments");
  std::vector<int> pl;
  MCXCHK(density2d_args(spec, np + 1, (int64_t)nsteps * nc, cols, axes, pairs_out, z, pl));
  return on_rows(rows, nsteps, nc, np, [&](hipStream_t st, Bufs B, const StoreView &v) {
    return density2d_device(st, B, v, spec, pl, cols, axes, pairs_out, z, nullptr);
  });
}

// the device sweeps alone on given grids
extern "C" int mcx_debug_rows_density2d_bins(const float *rows, int nsteps, int nc, int np, const double *lo, const double *up, int g,
                                             int npairs, const int *pairs, unsigned long long *slots)
{
  if (!rows || nc < 1 || np < 1 || np > 256 || nsteps < 1 || !lo || !up || !slots) return fail(MCX_ERR_INVALID, "bad arguments");
  MCXCHK(grid_size_args(g));
  std::vector<int> pl;
  MCXCHK(pair_list(npairs, pairs, np + 1, pl));
  if ((int64_t)nsteps * nc >= (1ll << 31)) return fail(MCX_ERR_UNSUPPORTED, "pair densities of %lld rows: fewer than 2^31", (long long)nsteps * nc);
  std::vector<double> grid2(((size_t)np + 1) * 2);
  for (int c = 0; c <= np; ++c) {
    if (!(lo[c] < up[c])) return fail(MCX_ERR_INVALID, "lo[%d] = %g is not below up[%d] = %g", c, lo[c], c, up[c]);
    grid2[2 * c] = lo[c];
    grid2[2 * c + 1] = (double)(g - 1) / (up[c] - lo[c]);
  }
  return on_rows(rows, nsteps, nc, np, [&](hipStream_t st, Bufs B, const StoreView &v) -> int {
    StageTimer tm{st, nullptr, 0, {}};
    std::vector<unsigned long long> out;
    MCXCHK(bins2d_device(st, B, v, g, grid2, pl, out, tm));
    std::copy(out.begin(), out.end(), slots);
    return MCX_OK;
  });
}

// ---------------------------------------------------------------------------------------------------------------------
// the host steps (no device calls): DESIGN.md section 15 restates every line
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int mcx_debug_density2d_grid(long long N, double mean, double sd, float min, float max, double q25, double q75,
                                        double qclip_lo, double qclip_hi, int is_last_col, int col, const mcx_density2d_spec *spec,
                                        mcx_col_density *out)
{
  if (!spec || !out) return fail(MCX_ERR_INVALID, "bad arguments");
  // from, to, the refusals and the non-finite record are section 13's; the bandwidth and the grid are this section's
  const mcx_density_spec s1 = spec1d(spec);
  MCXCHK(mcx_debug_density_grid(N, mean, sd, min, max, q25, q75, qclip_lo, qclip_hi, is_last_col, col, &s1, out));
  if (out->flags & MCX_SUMMARY_NONFINITE) return MCX_OK;
  if (!(spec->bw && !std::isnan(spec->bw[col]))) {
    double s = std::min(sd, (q75 - q25) / 1.34);
    if (s == 0.0) s = sd;
    if (s == 0.0) s = std::fabs((double)min);
    if (s == 0.0) s = 1.0;
    out->bw = spec->adjust * 1.06 * s * std::pow((double)N, -0.2);  // bandwidth.nrd / 4
  }
  out->lo = out->from - 4.0 * out->bw;
  out->up = out->to + 4.0 * out->bw;
  if (!(out->lo < out->up) || !std::isfinite(out->up - out->lo))
    return fail(MCX_ERR_INVALID, "column %d: the grid [%g, %g] is not a finite interval", col, out->lo, out->up);
  return MCX_OK;
}

// b_first = 0: t[j][l] = sum over m of mass[m][l] Ka[|m - j|], z[j][k] = sum over l of t[j][l] Kb[|l - k|].
// b_first = 1 (the product path for a > b): the b axis first, u[m][k] = sum over l of mass[m][l] Kb[|l - k|], z[j][k] = sum over
// m of u[m][k] Ka[|m - j|] -- the sums of the pair (b, a) with b_first = 0, so that z is that pair's transpose bit for bit
extern "C" int mcx_debug_density2d_finish(const mcx_col_density *ca, const mcx_col_density *cb, int g, const unsigned long long *slots,
                                          int b_first, double *z)
{
  if (!ca || !cb || !slots || !z || g < GMIN || g > GMAX || ca->nvalues < 2 || ca->nvalues != cb->nvalues || !(ca->bw > 0.0) ||
      !(cb->bw > 0.0) || !(ca->lo < ca->up) || !(cb->lo < cb->up))
    return fail(MCX_ERR_INVALID, "bad arguments");
  const int g1 = g + 1;
  const long long F = 1ll << FBITS;
  const double den = (double)(F * F) * (double)ca->nvalues;
  auto S = [&](int j, int k, int f) { return (long long)slots[((size_t)j * g1 + k) * 4 + f]; };  // f: 0 cnt, 1 Sa, 2 Sb, 3 Sab
  std::vector<double> mass((size_t)g * g), t((size_t)g * g), Ka(g), Kb(g);
  for (int j = 0; j < g; ++j)
    for (int k = 0; k < g; ++k) {
      const long long num = (F * F * S(j + 1, k + 1, 0) - F * S(j + 1, k + 1, 1) - F * S(j + 1, k + 1, 2) + S(j + 1, k + 1, 3)) +
                            (F * S(j, k + 1, 1) - S(j, k + 1, 3)) + (F * S(j + 1, k, 2) - S(j + 1, k, 3)) + S(j, k, 3);
      mass[(size_t)j * g + k] = (double)num / den;
    }
  auto ordinates = [&](const mcx_col_density *c, std::vector<double> &K) {
    const double delta = (c->up - c->lo) / (double)(g - 1), norm = c->bw * std::sqrt(2.0 * M_PI);
    for (int i = 0; i < g; ++i) {
      const double u = ((double)i * delta) / c->bw;
      K[i] = std::exp(-0.5 * (u * u)) / norm;
    }
  };
  ordinates(ca, Ka);
  ordinates(cb, Kb);
  // Every z[j][k] and t[..] below is one accumulator that takes its terms in ascending m, or l, as the definition says; the
  // loops are nested so that the innermost runs along a row of contiguous, independent accumulators (0.0 + x = x exactly).
  std::vector<double> Ta((size_t)g * g), Tb((size_t)g * g);  // Ta[j][m] = Ka[|m - j|], Tb[l][k] = Kb[|l - k|]
  for (int i = 0; i < g; ++i)
    for (int k = 0; k < g; ++k) {
      Ta[(size_t)i * g + k] = Ka[std::abs(k - i)];
      Tb[(size_t)i * g + k] = Kb[std::abs(k - i)];
    }
  std::fill(z, z + (size_t)g * g, 0.0);
  if (!b_first) {
    for (int j = 0; j < g; ++j) {  // t[j][l] = sum over m of mass[m][l] Ka[|m - j|]
      double *tj = &t[(size_t)j * g];
      for (int m = 0; m < g; ++m) {
        const double ka = Ta[(size_t)j * g + m], *mm = &mass[(size_t)m * g];
        for (int l = 0; l < g; ++l) tj[l] += mm[l] * ka;
      }
    }
    for (int j = 0; j < g; ++j) {  // z[j][k] = sum over l of t[j][l] Kb[|l - k|]
      double *zj = z + (size_t)j * g;
      for (int l = 0; l < g; ++l) {
        const double tl = t[(size_t)j * g + l], *kb = &Tb[(size_t)l * g];
        for (int k = 0; k < g; ++k) zj[k] += tl * kb[k];
      }
    }
  } else {
    for (int m = 0; m < g; ++m) {  // u[m][k] = sum over l of mass[m][l] Kb[|l - k|]
      double *um = &t[(size_t)m * g];
      for (int l = 0; l < g; ++l) {
        const double ml = mass[(size_t)m * g + l], *kb = &Tb[(size_t)l * g];
        for (int k = 0; k < g; ++k) um[k] += ml * kb[k];
      }
    }
    for (int j = 0; j < g; ++j) {  // z[j][k] = sum over m of u[m][k] Ka[|m - j|]
      double *zj = z + (size_t)j * g;
      for (int m = 0; m < g; ++m) {
        const double ka = Ta[(size_t)j * g + m], *um = &t[(size_t)m * g];
        for (int k = 0; k < g; ++k) zj[k] += um[k] * ka;
      }
    }
  }
  return MCX_OK;
}
