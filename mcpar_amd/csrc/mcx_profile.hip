// mcx_profile.hip -- mcx_samples_profile / mcx_rows_profile / mcx_store_profile and their *_profile2d: the profile likelihood
// of every parameter of a step range of the sample store, pl_c(x) = max { log L(row) : the row's column c in the bin of x } -
// max log L, and the same over the cells of a pair of parameters.  DESIGN.md section 27 restates every definition.
//
// One profile call:
//   1. summary_spread (mcx_summary.hip)  min, max and the clip pair's quantiles of every column (section 13's statistics)
//   2. grid_of                           host, per column: from, to, inv = n / (to - from)
//   3. k_profile_bins                    the one new sweep: per (column, bin) the maximum of the rows' 64-bit keys (log L in
//                                        float order above, the row index below) and their count; the maximum key of all rows
//   4. k_profile_at, k_profile_path      the column's value in the row of every key; that whole row when asked
//   5. finish_column                     host: the curve, its least concave majorant, the intervals
// One pair call: 1 and 2 with n = g; k_profile_codes (one byte per value: its bin), k_profile_keys (one key per row);
// k_profile_pairs per (pair, row chunks) with the pair's g x g keys and counts in LDS; k_profile_at twice; finish_pair.
// The device does integer max and integer add only, so the same store and arguments give the same bytes.
#include "mcx_profile_host.hpp"
#include "mcx_store.hpp"

#include <chrono>
#include <limits>

namespace {

namespace ph = mcx_profile_host;

constexpr int PCT = 8;             // columns per tile: PCT * N_MAX * (8 + 4) B = 48 KiB of LDS at n = 512
constexpr int PUNROLL = 8;         // steps whose loads are issued before the first of them is binned
// Values of one column that a workgroup bins between zeroing and draining its LDS: a slot's count is a u32
constexpr int64_t PVALS = 1 << 16;
static_assert(PVALS < (1ll << 32), "the counts of a chunk stay inside a u32");
static_assert((size_t)PCT * ph::N_MAX * (sizeof(unsigned long long) + sizeof(uint32_t)) == 48 * 1024, "48 KiB at the largest n");

constexpr size_t bins_lds_bytes(int ct, int n) { return (size_t)ct * n * (sizeof(unsigned long long) + sizeof(uint32_t)); }

// section 9's float order as a u32, a NaN counted as -inf (mcx_profile_host.hpp ll_key)
__device__ __forceinline__ uint32_t dev_ll_key(float l)
{
  uint32_t b = l != l ? 0xFF800000u : __float_as_uint(l);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ unsigned long long dev_row_key(float l, uint32_t r)
{
  return ((unsigned long long)dev_ll_key(l) << 32) | (unsigned long long)(0xFFFFFFFFu - r);
}

// The slot is read first and the atomic skipped when the key cannot win.  A slot only grows, so a stale read is at most the
// slot's value: key > slot implies key > stale, the atomic is then issued and a maximum is never lost; a stale read costs a
// superfluous atomic at the worst.
__device__ __forceinline__ void put_key(unsigned long long *keys, uint32_t *cnts, int slot, unsigned long long key)
{
  if (key > keys[slot]) atomicMax(&keys[slot], key);
  atomicAdd(&cnts[slot], 1u);
}

// the bin of v on (from, inv, to), mcx_profile_host.hpp bin_of: -1 for a dropped value
__device__ __forceinline__ int dev_bin_of(float v, double from, double inv, double to, int n)
{
  const double d = (double)v, xp = (d - from) * inv;  // (-ffp-contract=off: a subtraction and a multiplication)
  if (d == to) return from == to ? 0 : n - 1;
  if (xp >= 0.0 && xp < (double)n) return (int)xp;    // a NaN fails both
  return -1;
}

// ---- 3. the sweep ---------------------------------------------------------------------------------------------------------
// grid = (nbc * ntiles, step chunks) over the parameter tile set.  grid3[col] = (from, inv, to); gkeys, gcnt [np][n], ghat[1]
__global__ void __launch_bounds__(SB) k_profile_bins(TileSet t, const float *ly, int nc, int64_t T, int64_t chunk, int n, const double *grid3,
                                                     unsigned long long *gkeys, unsigned long long *gcnt, unsigned long long *ghat)
{
  extern __shared__ unsigned long long lds[];  // keys [ct][n] | counts [ct][n]
  __shared__ unsigned long long hat;
  unsigned long long *keys = lds;
  uint32_t *cnts = reinterpret_cast<uint32_t *>(lds + t.ct * n);
  const int tile = blockIdx.x % t.ntiles, bc = blockIdx.x / t.ntiles;
  for (int i = threadIdx.x; i < t.ct * n; i += SB) {
    keys[i] = 0ull;
    cnts[i] = 0u;
  }
  if (threadIdx.x == 0) hat = 0ull;
  __syncthreads();
  const Lane l = lane_of(t, tile, bc, nc);
  if (l.ok) {
    const double from = grid3[3 * l.lcol], inv = grid3[3 * l.lcol + 1], to = grid3[3 * l.lcol + 2];
    unsigned long long *mk = keys + l.j * n;
    uint32_t *mc = cnts + l.j * n;
    const float *p = t.src + (size_t)l.chain * t.cs + l.lcol;
    const float *q = ly + l.chain;
    const bool hatlane = l.lcol == 0;  // the lanes of column 0 see every row once: they keep the maximum of all rows
    unsigned long long best = 0ull;
    const int64_t s0 = (int64_t)blockIdx.y * chunk, s1 = min(T, s0 + chunk);
    int64_t s = s0;
    for (; s + PUNROLL <= s1; s += PUNROLL) {
      float v[PUNROLL], w[PUNROLL];
#pragma unroll
      for (int u = 0; u < PUNROLL; ++u) {
        v[u] = p[(s + u) * t.rs];
        w[u] = q[(s + u) * nc];
      }
#pragma unroll
      for (int u = 0; u < PUNROLL; ++u) {
        const unsigned long long key = dev_row_key(w[u], (uint32_t)((s + u) * nc + l.chain));
        const int ib = dev_bin_of(v[u], from, inv, to, n);
        if (ib >= 0) put_key(mk, mc, ib, key);
        if (hatlane) best = max(best, key);
      }
    }
    for (; s < s1; ++s) {
      const unsigned long long key = dev_row_key(q[s * nc], (uint32_t)(s * nc + l.chain));
      const int ib = dev_bin_of(p[s * t.rs], from, inv, to, n);
      if (ib >= 0) put_key(mk, mc, ib, key);
      if (hatlane) best = max(best, key);
    }
    if (hatlane && best > hat) atomicMax(&hat, best);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < t.ct * n; i += SB) {
    const unsigned long long k = keys[i];
    if (!k) continue;  // (a slot with a row has a key: no key is 0)
    const int j = i / n, b = i - j * n, lc = tile * t.ct + j;
    if (lc >= t.ncs) continue;
    const size_t o = (size_t)lc * n + b;
    if (k > gkeys[o]) atomicMax(&gkeys[o], k);
    atomicAdd(&gcnt[o], (unsigned long long)cnts[i]);
  }
  if (threadIdx.x == 0 && hat) atomicMax(ghat, hat);
}

// ---- 4. the values at the keys --------------------------------------------------------------------------------------------
// One lane per slot i < nslots: out[i] = x[row of keys[i]][col], col = colmap ? colmap[i / per] : i / per; NaN for an empty
// slot, whose row is not read.  Lanes nslots .. nslots + nhat - 1: out[i] = x[row of *hat][i - nslots]
__global__ void __launch_bounds__(SB) k_profile_at(const unsigned long long *keys, size_t nslots, int per, const int *colmap,
                                                   const unsigned long long *hat, int nhat, const float *x, int np, float *out)
{
  const size_t i = (size_t)blockIdx.x * SB + threadIdx.x;
  if (i >= nslots + (size_t)nhat) return;
  unsigned long long k;
  int col;
  if (i < nslots) {
    k = keys[i];
    col = colmap ? colmap[i / per] : (int)(i / per);
  } else {
    k = *hat;
    col = (int)(i - nslots);
  }
  float v = __uint_as_float(0x7FC00000u);
  if (k) v = x[(size_t)(0xFFFFFFFFu - (uint32_t)k) * np + col];
  out[i] = v;
}

// One wavefront per slot: path[slot][0 .. np] = the whole row of its key, log L last; NaN for an empty slot
__global__ void __launch_bounds__(SB) k_profile_path(const unsigned long long *keys, size_t nslots, const float *x, const float *ly, int np,
                                                     float *path)
{
  const size_t slot = (size_t)blockIdx.x * (SB / 64) + threadIdx.x / 64;
  if (slot >= nslots) return;
  const unsigned long long k = keys[slot];
  const size_t row = (size_t)(0xFFFFFFFFu - (uint32_t)k);
  float *o = path + slot * ((size_t)np + 1);
  for (int c = threadIdx.x % 64; c <= np; c += 64) o[c] = !k ? __uint_as_float(0x7FC00000u) : c < np ? x[row * np + c] : ly[row];
}

// ---- the pair sweeps ------------------------------------------------------------------------------------------------------
// k_profile_codes: the store is x[N][np]: a tile of TR rows by tc <= TCMAX columns is read along the rows, turned in LDS and
// written along the columns, one byte per value: its bin at g nodes, 0xFF for a dropped value.  grid = (ceil(N / TR),
// ceil(np / tc)); cmap[col] = the column's index among the code columns, -1 for a column in no pair
constexpr int TR = 128, TCMAX = 32;
constexpr uint8_t CODE_OFF = 0xFF;
static_assert(ph::G_MAX - 1 < CODE_OFF, "a bin is a byte below 0xFF");

__global__ void __launch_bounds__(SB) k_profile_codes(const float *x, int np, int64_t N, int64_t npad, int g, int tc, const double *grid3,
                                                      const int *cmap, uint8_t *code)
{
  __shared__ uint8_t tile[TCMAX * (TR + 4)];
  __shared__ double gfrom[TCMAX], ginv[TCMAX], gto[TCMAX];
  __shared__ int gmap[TCMAX];
  const int64_t row0 = (int64_t)blockIdx.x * TR;
  const int col0 = (int)blockIdx.y * tc;
  const int ncs = min(tc, np - col0);
  const int nr = (int)min((int64_t)TR, N - row0);
  if ((int)threadIdx.x < ncs) {
    gfrom[threadIdx.x] = grid3[3 * (col0 + threadIdx.x)];
    ginv[threadIdx.x] = grid3[3 * (col0 + threadIdx.x) + 1];
    gto[threadIdx.x] = grid3[3 * (col0 + threadIdx.x) + 2];
    gmap[threadIdx.x] = cmap[col0 + threadIdx.x];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < nr * ncs; e += SB) {
    const int lr = e / ncs, lc = e - lr * ncs;
    uint8_t cd = CODE_OFF;
    if (gmap[lc] >= 0) {
      const int ib = dev_bin_of(x[(size_t)(row0 + lr) * np + col0 + lc], gfrom[lc], ginv[lc], gto[lc], g);
      if (ib >= 0) cd = (uint8_t)ib;
    }
    tile[lc * (TR + 4) + lr] = cd;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < ncs * TR; e += SB) {
    const int c = e / TR, r = e - c * TR;
    const int ci = gmap[c];
    if (r < nr && ci >= 0) code[(size_t)ci * npad + row0 + r] = tile[c * (TR + 4) + r];
  }
}

// k_profile_keys: rowkey[r] = K(r) of every row, and the maximum of all of them
__global__ void __launch_bounds__(SB) k_profile_keys(const float *ly, int64_t N, unsigned long long *rowkey, unsigned long long *ghat)
{
  __shared__ unsigned long long hat;
  if (threadIdx.x == 0) hat = 0ull;
  __syncthreads();
  unsigned long long best = 0ull;
  for (int64_t r = (int64_t)blockIdx.x * SB + threadIdx.x; r < N; r += (int64_t)gridDim.x * SB) {
    const unsigned long long key = dev_row_key(ly[r], (uint32_t)r);
    rowkey[r] = key;
    best = max(best, key);
  }
  if (best > hat) atomicMax(&hat, best);
  __syncthreads();
  if (threadIdx.x == 0 && hat) atomicMax(ghat, hat);
}

// k_profile_pairs: grid = npairs * W, workgroup = w * npairs + pair: the pairs of one row chunk are neighbours in the launch
// order and read the chunk's codes and keys from L2.  Workgroup (pair, w) walks the chunks w, w + W, ... with the pair's g x g
// keys and counts in LDS and drains them once.  A workgroup's count of a cell is below N < 2^32.  pc[pair] = its two code columns
constexpr int PB2 = 512;
constexpr int64_t P2CHUNK = 1 << 16;
constexpr int TARGET_WGS = 1024;
static_assert(P2CHUNK % 4 == 0, "a chunk starts on a 4-byte boundary of a code column");
constexpr size_t pair_lds_bytes(int g) { return (size_t)g * g * (sizeof(unsigned long long) + sizeof(uint32_t)); }
static_assert(pair_lds_bytes(ph::G_MAX) == 48 * 1024, "48 KiB at g = 64");

__device__ __forceinline__ void put_cell(unsigned long long *keys, uint32_t *cnts, int g, uint32_t a, uint32_t b, unsigned long long key)
{
  if (a == CODE_OFF || b == CODE_OFF) return;  // a row counts only if both values are binned
  put_key(keys, cnts, (int)(a * g + b), key);
}

__global__ void __launch_bounds__(PB2) k_profile_pairs(const uint8_t *code, const unsigned long long *rowkey, int64_t N, int64_t npad, int g,
                                                       int npairs, const int *pc, int W, int64_t nchunks, unsigned long long *gkeys,
                                                       unsigned long long *gcnt)
{
  extern __shared__ unsigned long long lds[];  // keys [g][g] | counts [g][g]
  const int gg = g * g;
  unsigned long long *keys = lds;
  uint32_t *cnts = reinterpret_cast<uint32_t *>(lds + gg);
  const int pair = (int)(blockIdx.x % (unsigned)npairs), w = (int)(blockIdx.x / (unsigned)npairs);
  const uint8_t *ca = code + (size_t)pc[2 * pair] * npad, *cb = code + (size_t)pc[2 * pair + 1] * npad;
  for (int i = threadIdx.x; i < gg; i += PB2) {
    keys[i] = 0ull;
    cnts[i] = 0u;
  }
  __syncthreads();
  for (int64_t ch = w; ch < nchunks; ch += W) {
    const int64_t r0 = ch * P2CHUNK, r1 = min(N, r0 + P2CHUNK);
    for (int64_t r = r0 + 4 * (int64_t)threadIdx.x; r < r1; r += 4 * PB2) {
      if (r + 4 <= r1) {
        const uchar4 a = *reinterpret_cast<const uchar4 *>(ca + r), b = *reinterpret_cast<const uchar4 *>(cb + r);
        const unsigned long long k0 = rowkey[r], k1 = rowkey[r + 1], k2 = rowkey[r + 2], k3 = rowkey[r + 3];
        put_cell(keys, cnts, g, a.x, b.x, k0);
        put_cell(keys, cnts, g, a.y, b.y, k1);
        put_cell(keys, cnts, g, a.z, b.z, k2);
        put_cell(keys, cnts, g, a.w, b.w, k3);
      } else {
        for (int64_t q = r; q < r1; ++q) put_cell(keys, cnts, g, ca[q], cb[q], rowkey[q]);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < gg; i += PB2) {
    const unsigned long long k = keys[i];
    if (!k) continue;
    const size_t o = (size_t)pair * gg + i;
    if (k > gkeys[o]) atomicMax(&gkeys[o], k);
    atomicAdd(&gcnt[o], (unsigned long long)cnts[i]);
  }
}

// ---- launch geometry: one function per sweep, so that mcx_debug_profile_geometry reports what is launched ------------------
TileSet profile_tiles(TileSet t, int nc)
{
  t.ct = std::min(t.ct, PCT);
  t.cg = SB / t.ct;
  t.ntiles = (t.ncs + t.ct - 1) / t.ct;
  t.nbc = (nc + t.cg - 1) / t.cg;
  return t;
}
struct BinsGeometry {
  TileSet t;
  int64_t chunk;
  unsigned chunks;
};
BinsGeometry bins_geometry(const TileSet &tx, int nc, int64_t T)
{
  BinsGeometry b;
  b.t = profile_tiles(tx, nc);
  b.chunk = PVALS / b.t.cg;
  b.chunks = (unsigned)((T + b.chunk - 1) / b.chunk);
  return b;
}
// k_profile_keys: a lane per row up to KEYS_MAX_WGS workgroups, a grid stride beyond
constexpr int64_t KEYS_MAX_WGS = 4096;
inline unsigned keys_workgroups(int64_t N) { return (unsigned)std::min<int64_t>((N + SB - 1) / SB, KEYS_MAX_WGS); }
struct PairGeometry {
  int64_t nchunks;
  int W;
};
PairGeometry pair_geometry(int64_t N, int npairs)
{
  PairGeometry p;
  p.nchunks = (N + P2CHUNK - 1) / P2CHUNK;
  p.W = (int)std::max<int64_t>(1, std::min<int64_t>(p.nchunks, (TARGET_WGS + npairs - 1) / npairs));
  return p;
}

int ph_fail(int code, const std::string &why) { return fail(code, "%s", why.c_str()); }

inline float *as_floats(uint32_t *p) { return reinterpret_cast<float *>(p); }

// The 1-D device part: grid3 [np][3] -> keys [np][n], hat, cnt [np][n], xat [np][n], xhat [np], path [np][n][np + 1] (when
// asked) on the host.  tm: stage 1 is k_profile_bins alone
struct BinsOut {
  std::vector<unsigned long long> words;  // keys [np * n] | hat | cnt [np * n]
  std::vector<float> xat;                 // [np * n] | xhat [np]
};
int bins_device(hipStream_t st, Bufs B, const StoreView &v, int n, const std::vector<double> &grid3, BinsOut &o, float *path, StageTimer &tm)
{
  const int np = v.np;
  const size_t ns = (size_t)np * n, nw = 2 * ns + 1, npath = path ? ns * ((size_t)np + 1) : 0;
  if (B.d->alloc(grid3.size()) != MCX_OK || B.h->alloc(nw) != MCX_OK || B.u->alloc(ns + np + npath) != MCX_OK)
    return fail(MCX_ERR_ALLOC, "profile: %zu bytes of scratch are needed (DESIGN.md section 27)", grid3.size() * 8 + nw * 8 + (ns + np + npath) * 4);
  unsigned long long *dkeys = B.h->p, *dhat = B.h->p + ns, *dcnt = B.h->p + ns + 1;
  float *dxat = as_floats(B.u->p), *dpath = dxat + ns + np;
  HIPCHK(hipMemcpyAsync(B.d->p, grid3.data(), grid3.size() * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(B.h->p, 0, nw * sizeof(unsigned long long), st));
  MCXCHK(tm.run(1, [&]() -> int {
    const BinsGeometry b = bins_geometry(v.tx, v.nc, v.T);
    hipLaunchKernelGGL(k_profile_bins, dim3((unsigned)(b.t.nbc * b.t.ntiles), b.chunks), dim3(SB), bins_lds_bytes(b.t.ct, n), st, b.t, v.ly,
                       v.nc, v.T, b.chunk, n, (const double *)B.d->p, dkeys, dcnt, dhat);
    HIPCHK(hipGetLastError());
    return MCX_OK;
  }));
  hipLaunchKernelGGL(k_profile_at, dim3((unsigned)((ns + np + SB - 1) / SB)), dim3(SB), 0, st, (const unsigned long long *)dkeys, ns, n,
                     (const int *)nullptr, (const unsigned long long *)dhat, np, v.x, np, dxat);
  HIPCHK(hipGetLastError());
  if (path) {
    hipLaunchKernelGGL(k_profile_path, dim3((unsigned)((ns + SB / 64 - 1) / (SB / 64))), dim3(SB), 0, st, (const unsigned long long *)dkeys, ns,
                       v.x, v.ly, np, dpath);
    HIPCHK(hipGetLastError());
  }
  o.words.resize(nw);
  o.xat.resize(ns + np);
  HIPCHK(hipMemcpyAsync(o.words.data(), B.h->p, nw * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(o.xat.data(), dxat, (ns + np) * sizeof(float), hipMemcpyDeviceToHost, st));
  if (path) HIPCHK(hipMemcpyAsync(path, dpath, npath * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));  // (grid3 is read by the upload until here)
  return MCX_OK;
}

// the statistics and the grids of the np profiled columns: cols[c].from / to / nvalues / flags, grid3 (NaN for a column that is
// not finite: it bins nothing)
int grids_device(hipStream_t st, Bufs B, const StoreView &v, int bins, double clip_lo, double clip_hi, const double *from, const double *to,
                 mcx_col_profile *cols, std::vector<double> &grid3)
{
  const bool clip = ph::clipped(clip_lo, clip_hi);
  const double probs[2] = {clip_lo, clip_hi}, qnan = std::numeric_limits<double>::quiet_NaN();
  const int nprobs = clip ? 2 : 0;
  std::vector<mcx_col_summary> sc(v.ncol);
  std::vector<double> q((size_t)v.ncol * 2);
  MCXCHK(summary_spread(st, B, v, probs, nprobs, sc.data(), q.data()));
  grid3.assign((size_t)v.np * 3, qnan);
  for (int c = 0; c < v.np; ++c) {
    mcx_col_profile *o = &cols[c];
    o->from = o->to = o->lhat = o->xhat = qnan;
    o->row_hat = -1;
    o->nvalues = v.N;
    o->nbinned = o->ndropped = 0;
    o->nempty = bins;
    o->flags = 0;
    if (sc[c].flags & MCX_SUMMARY_NONFINITE) {
      o->flags = MCX_SUMMARY_NONFINITE;
      continue;
    }
    ph::Grid g;
    std::string why;
    if (ph::grid_of(c, bins, sc[c].min, sc[c].max, clip, clip ? q[(size_t)c * 2] : qnan, clip ? q[(size_t)c * 2 + 1] : qnan, from, to, g, why))
      return ph_fail(MCX_ERR_INVALID, why);
    o->from = g.from;
    o->to = g.to;
    grid3[3 * c] = g.from;
    grid3[3 * c + 1] = g.inv;
    grid3[3 * c + 2] = g.to;
  }
  return MCX_OK;
}

struct ProfileOut {
  mcx_col_profile *cols;
  unsigned long long *cnt;
  float *lmax;
  long long *row;
  float *xat;
  double *pl, *plh;
  mcx_profile_interval_t *intervals;
  float *path;  // may be NULL
};
static_assert(sizeof(mcx_profile_interval_t) == sizeof(ph::Interval), "the host record is the interface's");

// what can be refused before a device is touched
int profile_args(const mcx_profile_spec *s, int np, int64_t N, const ProfileOut &o, ph::Levels &lv)
{
  if (!s) return fail(MCX_ERR_INVALID, "the profile spec is NULL");
  if (!o.cols || !o.cnt || !o.lmax || !o.row || !o.xat || !o.pl || !o.plh || !o.intervals)
    return fail(MCX_ERR_INVALID, "cols, cnt, lmax, row, xat, pl, plh or intervals is NULL");
  std::string why;
  int rc = ph::spec_check(s->n, ph::N_MIN, ph::N_MAX, s->clip_lo, s->clip_hi, s->from, s->to, np, N, why);
  if (rc) return ph_fail(rc, why);
  rc = ph::levels_of(s->nlevels, s->levels, s->levels_are_drops, false, lv, why);
  if (rc) return ph_fail(rc, why);
  return MCX_OK;
}

// ms (mcx_debug_profile_times, else NULL): ms[0] the statistics passes (wall clock), ms[1] k_profile_bins (HIP events), ms[2]
// the host grids and finish (wall clock), ms[3] the whole call (wall clock)
int profile_device(hipStream_t st, Bufs B, const StoreView &v, const mcx_profile_spec *spec, const ph::Levels &lv, const ProfileOut &o,
                   double *ms)
{
  using clk = std::chrono::steady_clock;
  auto since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
  const clk::time_point t_call = clk::now();
  StageTimer tm{st, ms, 4, {}};
  const int np = v.np, n = spec->n;
  const double qnan = std::numeric_limits<double>::quiet_NaN();

  std::vector<double> grid3;
  MCXCHK(grids_device(st, B, v, n, spec->clip_lo, spec->clip_hi, spec->from, spec->to, o.cols, grid3));
  const double ms_stats = since(t_call);

  BinsOut bo;
  MCXCHK(bins_device(st, B, v, n, grid3, bo, o.path, tm));

  const clk::time_point t_host = clk::now();
  const size_t ns = (size_t)np * n;
  const unsigned long long hat = bo.words[ns], *keys = bo.words.data(), *cnt = bo.words.data() + ns + 1;
  std::vector<double> x(n);
  for (int c = 0; c < np; ++c) {
    mcx_col_profile *col = &o.cols[c];
    const size_t at = (size_t)c * n;
    mcx_profile_interval_t *iv = o.intervals + (size_t)c * lv.n;
    int flags = ph::finish_column(n, reinterpret_cast<const uint64_t *>(keys + at), reinterpret_cast<const uint64_t *>(cnt + at),
                                  bo.xat.data() + at, hat, lv, o.lmax + at, o.row + at, x.data(), o.pl + at, o.plh + at,
                                  reinterpret_cast<ph::Interval *>(iv), &col->nbinned, &col->nempty);
    for (int j = 0; j < n; ++j) {
      o.cnt[at + j] = cnt[at + j];
      o.xat[at + j] = keys[at + j] ? bo.xat[at + j] : std::numeric_limits<float>::quiet_NaN();
    }
    col->row_hat = ph::key_row(hat);
    if (col->flags & MCX_SUMMARY_NONFINITE) {  // nothing was binned: NaN in every double of the record and the curves
      for (int j = 0; j < n; ++j) o.pl[at + j] = o.plh[at + j] = qnan;
      for (int i = 0; i < lv.n; ++i) {
        iv[i].lo = iv[i].hi = iv[i].lo_hull = iv[i].hi_hull = qnan;
        iv[i].nseg = 0;
        iv[i].flags = MCX_SUMMARY_NONFINITE;
      }
      continue;
    }
    col->flags |= flags;
    col->lhat = (double)ph::key_lmax(hat);
    col->xhat = (double)bo.xat[ns + c];
    col->ndropped = col->nvalues - col->nbinned;
  }
  const double ms_host = since(t_host);
  MCXCHK(tm.collect());
  if (ms) {
    ms[0] = ms_stats;
    ms[2] = ms_host;
    ms[3] = since(t_call);
  }
  return MCX_OK;
}

// ---- pairs ----------------------------------------------------------------------------------------------------------------
struct Profile2dOut {
  mcx_col_profile *cols;
  mcx_pair_profile *pairs;
  unsigned long long *cnt;
  float *lmax;
  long long *row;
  float *xat_a, *xat_b;
  double *z;
  long long *nlevel;
};

int profile2d_args(const mcx_profile2d_spec *s, int np, int64_t N, const Profile2dOut &o, ph::Levels &lv, std::vector<int> &pl)
{
  if (!s) return fail(MCX_ERR_INVALID, "the profile spec is NULL");
  if (!o.cols || !o.pairs || !o.cnt || !o.lmax || !o.row || !o.xat_a || !o.xat_b || !o.z || !o.nlevel)
    return fail(MCX_ERR_INVALID, "cols, pairs_out, cnt, lmax, row, xat_a, xat_b, z or nlevel is NULL");
  std::string why;
  int rc = ph::spec_check(s->g, ph::G_MIN, ph::G_MAX, s->clip_lo, s->clip_hi, s->from, s->to, np, N, why);
  if (rc) return ph_fail(rc, why);
  rc = ph::levels_of(s->nlevels, s->levels, s->levels_are_drops, true, lv, why);
  if (rc) return ph_fail(rc, why);
  rc = ph::pair_list(s->npairs, s->pairs, np, pl, why);
  if (rc) return ph_fail(rc, why);
  return MCX_OK;
}

// The 2-D device part: live [nl][2] pairs of finite columns -> words = keys [nl][g][g] | hat | cnt [nl][g][g]; xa = the a
// column's value at every key | xhat [np]; xb = the b column's.  tm: stage 1 the code and key sweeps, 2 the pair sweep, 3 the
// values at the keys
int pairs_device(hipStream_t st, Bufs B, const StoreView &v, int g, const std::vector<double> &grid3, const std::vector<int> &live,
                 std::vector<unsigned long long> &words, std::vector<float> &xa, std::vector<float> &xb, StageTimer &tm)
{
  const int np = v.np, nl = (int)(live.size() / 2);
  const size_t gg = (size_t)g * g, ns = (size_t)nl * gg, nw = 2 * ns + 1;
  // the code columns
  std::vector<int> meta(np, -1);
  int ncode = 0;
  for (int c = 0; c < np; ++c) {
    bool used = false;
    for (int p = 0; p < 2 * nl && !used; ++p) used = live[p] == c;
    if (used) meta[c] = ncode++;
  }
  for (int p = 0; p < 2 * nl; ++p) meta.push_back(meta[live[p]]);  // pc [nl][2]
  for (int p = 0; p < nl; ++p) meta.push_back(live[2 * p]);        // the a columns
  for (int p = 0; p < nl; ++p) meta.push_back(live[2 * p + 1]);    // the b columns
  const PairGeometry pg = pair_geometry(v.N, std::max(nl, 1));
  const int64_t npad = (v.N + 3) / 4 * 4;
  const size_t code_words = (size_t)ncode * npad / 4, nh = (size_t)v.N + nw, nu = code_words + 2 * ns + np;
  DevBuf<int> dmeta;
  if (B.u->alloc(nu) != MCX_OK || B.h->alloc(nh) != MCX_OK || B.d->alloc(grid3.size()) != MCX_OK || dmeta.alloc(meta.size()) != MCX_OK)
    return fail(MCX_ERR_ALLOC, "pair profiles: %zu bytes of scratch are needed (%d code columns of %lld rows, one key per row; DESIGN.md section 27)",
                nu * 4 + nh * 8 + grid3.size() * 8 + meta.size() * 4, ncode, (long long)v.N);
  unsigned long long *rowkey = B.h->p, *dkeys = rowkey + v.N, *dhat = dkeys + ns, *dcnt = dhat + 1;
  uint8_t *code = reinterpret_cast<uint8_t *>(B.u->p);
  float *dxa = as_floats(B.u->p + code_words), *dxb = dxa + ns + np;
  const int *cmap = dmeta.p, *pc = dmeta.p + np, *cola = pc + 2 * nl, *colb = cola + nl;
  HIPCHK(hipMemcpyAsync(B.d->p, grid3.data(), grid3.size() * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dmeta.p, meta.data(), meta.size() * sizeof(int), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(dkeys, 0, nw * sizeof(unsigned long long), st));
  MCXCHK(tm.run(1, [&]() -> int {
    if (ncode > 0) {
      const int tc = std::min(np, TCMAX);
      hipLaunchKernelGGL(k_profile_codes, dim3((unsigned)((v.N + TR - 1) / TR), (unsigned)((np + tc - 1) / tc)), dim3(SB), 0, st, v.x, np, v.N,
                         npad, g, tc, (const double *)B.d->p, cmap, code);
      HIPCHK(hipGetLastError());
    }
    const unsigned nb = keys_workgroups(v.N);
    hipLaunchKernelGGL(k_profile_keys, dim3(nb), dim3(SB), 0, st, v.ly, v.N, rowkey, dhat);
    HIPCHK(hipGetLastError());
    return MCX_OK;
  }));
  if (nl > 0)
    MCXCHK(tm.run(2, [&]() -> int {
      hipLaunchKernelGGL(k_profile_pairs, dim3((unsigned)((size_t)nl * pg.W)), dim3(PB2), pair_lds_bytes(g), st, (const uint8_t *)code,
                         (const unsigned long long *)rowkey, v.N, npad, g, nl, pc, pg.W, pg.nchunks, dkeys, dcnt);
      HIPCHK(hipGetLastError());
      return MCX_OK;
    }));
  MCXCHK(tm.run(3, [&]() -> int {
    hipLaunchKernelGGL(k_profile_at, dim3((unsigned)((ns + np + SB - 1) / SB)), dim3(SB), 0, st, (const unsigned long long *)dkeys, ns, (int)gg,
                       cola, (const unsigned long long *)dhat, np, v.x, np, dxa);
    HIPCHK(hipGetLastError());
    if (nl > 0) {
      hipLaunchKernelGGL(k_profile_at, dim3((unsigned)((ns + SB - 1) / SB)), dim3(SB), 0, st, (const unsigned long long *)dkeys, ns, (int)gg, colb,
                         (const unsigned long long *)dhat, 0, v.x, np, dxb);
      HIPCHK(hipGetLastError());
    }
    return MCX_OK;
  }));
  words.resize(nw);
  xa.resize(ns + np);
  xb.resize(ns);
  HIPCHK(hipMemcpyAsync(words.data(), dkeys, nw * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(xa.data(), dxa, (ns + np) * sizeof(float), hipMemcpyDeviceToHost, st));
  if (ns) HIPCHK(hipMemcpyAsync(xb.data(), dxb, ns * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));  // (grid3, meta and dmeta are in use until here)
  return MCX_OK;
}

// ms (mcx_debug_profile2d_times, else NULL): ms[0] the statistics passes (wall clock), ms[1] k_profile_codes and k_profile_keys,
// ms[2] k_profile_pairs, ms[3] k_profile_at (HIP events), ms[4] the host grids and finish (wall clock), ms[5] the whole call
int profile2d_device(hipStream_t st, Bufs B, const StoreView &v, const mcx_profile2d_spec *spec, const ph::Levels &lv, const std::vector<int> &pl,
                     const Profile2dOut &o, double *ms)
{
  using clk = std::chrono::steady_clock;
  auto since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
  const clk::time_point t_call = clk::now();
  StageTimer tm{st, ms, 6, {}};
  const int np = v.np, g = spec->g, npairs = (int)(pl.size() / 2);
  const size_t gg = (size_t)g * g;
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  const float fnan = std::numeric_limits<float>::quiet_NaN();

  std::vector<double> grid3;
  MCXCHK(grids_device(st, B, v, g, spec->clip_lo, spec->clip_hi, spec->from, spec->to, o.cols, grid3));
  const double ms_stats = since(t_call);

  // the pairs of two finite columns go to the device
  std::vector<int> live, where(npairs, -1);
  for (int p = 0; p < npairs; ++p) {
    if ((o.cols[pl[2 * p]].flags | o.cols[pl[2 * p + 1]].flags) & MCX_SUMMARY_NONFINITE) continue;
    where[p] = (int)(live.size() / 2);
    live.push_back(pl[2 * p]);
    live.push_back(pl[2 * p + 1]);
  }
  std::vector<unsigned long long> words;
  std::vector<float> xa, xb;
  MCXCHK(pairs_device(st, B, v, g, grid3, live, words, xa, xb, tm));

  const clk::time_point t_host = clk::now();
  const size_t ns = live.size() / 2 * gg;
  const unsigned long long hat = words[ns], *keys = words.data(), *cnt = words.data() + ns + 1;
  for (int c = 0; c < np; ++c) {
    mcx_col_profile *col = &o.cols[c];
    col->row_hat = ph::key_row(hat);
    col->nempty = 0;
    if (col->flags & MCX_SUMMARY_NONFINITE) continue;
    col->lhat = (double)ph::key_lmax(hat);
    col->xhat = (double)xa[ns + c];
    if (!std::isfinite(col->lhat)) col->flags |= MCX_PROFILE_LL_NONFINITE;
  }
  for (int p = 0; p < npairs; ++p) {
    mcx_pair_profile *po = &o.pairs[p];
    const size_t at = (size_t)p * gg;
    po->a = pl[2 * p];
    po->b = pl[2 * p + 1];
    po->nbinned = 0;
    po->nempty = (int)gg;
    po->flags = 0;
    long long *nlev = o.nlevel + (size_t)p * lv.n;
    if (where[p] < 0) {
      po->flags = MCX_SUMMARY_NONFINITE;
      for (size_t i = 0; i < gg; ++i) {
        o.cnt[at + i] = 0;
        o.lmax[at + i] = -std::numeric_limits<float>::infinity();
        o.row[at + i] = -1;
        o.xat_a[at + i] = o.xat_b[at + i] = fnan;
        o.z[at + i] = qnan;
      }
      for (int l = 0; l < lv.n; ++l) nlev[l] = 0;
      continue;
    }
    const size_t src = (size_t)where[p] * gg;
    ph::finish_pair(g, reinterpret_cast<const uint64_t *>(keys + src), reinterpret_cast<const uint64_t *>(cnt + src), hat, lv, o.lmax + at,
                    o.row + at, o.z + at, nlev, &po->nbinned, &po->nempty);
    for (size_t i = 0; i < gg; ++i) {
      o.cnt[at + i] = cnt[src + i];
      o.xat_a[at + i] = keys[src + i] ? xa[src + i] : fnan;
      o.xat_b[at + i] = keys[src + i] ? xb[src + i] : fnan;
    }
    if (!std::isfinite(ph::key_lmax(hat))) po->flags |= MCX_PROFILE_LL_NONFINITE;
  }
  const double ms_host = since(t_host);
  MCXCHK(tm.collect());
  if (ms) {
    ms[0] = ms_stats;
    ms[4] = ms_host;
    ms[5] = since(t_call);
  }
  return MCX_OK;
}

int rows_args(const float *rows, int nc, int np)
{
  if (!rows) return fail(MCX_ERR_INVALID, "rows is NULL");
  if (nc < 1) return fail(MCX_ERR_INVALID, "nc = %d: at least one chain", nc);
  if (np < 1 || np > 256) return fail(MCX_ERR_INVALID, "np = %d: 1 to 256 parameters", np);
  return MCX_OK;
}

// buffers of a timed call whose results are let go
struct LetGo {
  std::vector<mcx_col_profile> cols;
  std::vector<unsigned long long> cnt;
  std::vector<float> lmax, xat, xat_b;
  std::vector<long long> row, nlevel;
  std::vector<double> pl, plh;
  std::vector<mcx_profile_interval_t> iv;
  std::vector<mcx_pair_profile> pairs;
  ProfileOut out1(int np, int n)
  {
    const size_t ns = (size_t)np * std::max(n, 1);
    cols.resize(np); cnt.resize(ns); lmax.resize(ns); row.resize(ns); xat.resize(ns); pl.resize(ns); plh.resize(ns);
    iv.resize((size_t)np * ph::MAX_LEVELS);
    return ProfileOut{cols.data(), cnt.data(), lmax.data(), row.data(), xat.data(), pl.data(), plh.data(), iv.data(), nullptr};
  }
  Profile2dOut out2(int np, int g, int npairs)
  {
    const size_t ns = (size_t)std::max(npairs, 1) * std::max(g, 1) * std::max(g, 1);
    cols.resize(np); pairs.resize(std::max(npairs, 1)); cnt.resize(ns); lmax.resize(ns); row.resize(ns); xat.resize(ns); xat_b.resize(ns);
    pl.resize(ns); nlevel.resize((size_t)std::max(npairs, 1) * ph::MAX_LEVELS);
    return Profile2dOut{cols.data(), pairs.data(), cnt.data(), lmax.data(), row.data(), xat.data(), xat_b.data(), pl.data(), nlevel.data()};
  }
};

}  // namespace

// ---- profiles: the three forms --------------------------------------------------------------------------------------------
extern "C" int mcx_samples_profile(mcx_engine *e, int first_step, int nsteps, const mcx_profile_spec *spec, mcx_col_profile *cols,
                                   unsigned long long *cnt, float *lmax, long long *row, float *xat, double *pl, double *plh,
                                   mcx_profile_interval_t *intervals, float *path)
{
  const ProfileOut o{cols, cnt, lmax, row, xat, pl, plh, intervals, path};
  ph::Levels lv;
  return on_store(
      e, first_step, nsteps, [&] { return profile_args(spec, e->nparam, (int64_t)nsteps * e->nchain, o, lv); },
      [&](hipStream_t st, Bufs B, const StoreView &v) { return profile_device(st, B, v, spec, lv, o, nullptr); });
}

extern "C" int mcx_rows_profile(const float *rows, int nsteps, int nc, int np, const mcx_profile_spec *spec, mcx_col_profile *cols,
                                unsigned long long *cnt, float *lmax, long long *row, float *xat, double *pl, double *plh,
                                mcx_profile_interval_t *intervals, float *path)
{
  MCXCHK(rows_args(rows, nc, np));
  const ProfileOut o{cols, cnt, lmax, row, xat, pl, plh, intervals, path};
  ph::Levels lv;
  MCXCHK(profile_args(spec, np, (int64_t)nsteps * nc, o, lv));
  return on_rows(rows, nsteps, nc, np, [&](hipStream_t st, Bufs B, const StoreView &v) { return profile_device(st, B, v, spec, lv, o, nullptr); });
}

extern "C" int mcx_store_profile(mcx_store *s, const mcx_profile_spec *spec, mcx_col_profile *cols, unsigned long long *cnt, float *lmax,
                                 long long *row, float *xat, double *pl, double *plh, mcx_profile_interval_t *intervals, float *path)
{
  if (!s) return fail(MCX_ERR_INVALID, "the store s is NULL");
  const ProfileOut o{cols, cnt, lmax, row, xat, pl, plh, intervals, path};
  ph::Levels lv;
  MCXCHK(profile_args(spec, s->nout, (int64_t)s->T * s->nc, o, lv));
  HIPCHK(hipSetDevice(s->device));
  return profile_device(s->st, s->bufs(), StoreView(s->span()), spec, lv, o, nullptr);
}

// mcx_samples_profile / mcx_store_profile with their stages timed, for tools/profile_bench.py; the results are let go
extern "C" int mcx_debug_profile_times(mcx_engine *e, int first_step, int nsteps, const mcx_profile_spec *spec, double *ms)
{
  LetGo lg;
  ProfileOut o{};
  ph::Levels lv;
  return on_store(
      e, first_step, nsteps,
      [&] {
        if (!ms) return fail(MCX_ERR_INVALID, "ms is NULL");
        if (!spec) return fail(MCX_ERR_INVALID, "the profile spec is NULL");
        o = lg.out1(e->nparam, std::min(std::max(spec->n, 1), ph::N_MAX));
        return profile_args(spec, e->nparam, (int64_t)nsteps * e->nchain, o, lv);
      },
      [&](hipStream_t st, Bufs B, const StoreView &v) { return profile_device(st, B, v, spec, lv, o, ms); });
}

extern "C" int mcx_debug_store_profile_times(mcx_store *s, const mcx_profile_spec *spec, double *ms)
{
  if (!s) return fail(MCX_ERR_INVALID, "the store s is NULL");
  if (!ms || !spec) return fail(MCX_ERR_INVALID, "ms or the profile spec is NULL");
  LetGo lg;
  const ProfileOut o = lg.out1(s->nout, std::min(std::max(spec->n, 1), ph::N_MAX));
  ph::Levels lv;
  MCXCHK(profile_args(spec, s->nout, (int64_t)s->T * s->nc, o, lv));
  HIPCHK(hipSetDevice(s->device));
  return profile_device(s->st, s->bufs(), StoreView(s->span()), spec, lv, o, ms);
}

// the sweep alone on given grids -> keys, cnt [np][n], hat[1]
extern "C" int mcx_debug_rows_profile_bins(const float *rows, int nsteps, int nc, int np, int n, const double *from, const double *to,
                                           unsigned long long *keys, unsigned long long *cnt, unsigned long long *hat)
{
  MCXCHK(rows_args(rows, nc, np));
  if (nsteps < 1 || !from || !to || !keys || !cnt || !hat) return fail(MCX_ERR_INVALID, "bad arguments");
  if (n < ph::N_MIN || n > ph::N_MAX) return fail(MCX_ERR_INVALID, "n = %d: %d to %d bins", n, ph::N_MIN, ph::N_MAX);
  if ((int64_t)nsteps * nc >= (1ll << 32)) return fail(MCX_ERR_UNSUPPORTED, "a profile of %lld rows: fewer than 2^32", (long long)nsteps * nc);
  std::vector<double> grid3((size_t)np * 3);
  for (int c = 0; c < np; ++c) {
    if (!(from[c] <= to[c]) || !std::isfinite(to[c] - from[c]))
      return fail(MCX_ERR_INVALID, "from[%d] = %g and to[%d] = %g are not a finite range", c, from[c], c, to[c]);
    grid3[3 * c] = from[c];
    grid3[3 * c + 1] = (double)n / (to[c] - from[c]);
    grid3[3 * c + 2] = to[c];
  }
  return on_rows(rows, nsteps, nc, np, [&](hipStream_t st, Bufs B, const StoreView &v) -> int {
    StageTimer tm{st, nullptr, 0, {}};
    BinsOut bo;
    MCXCHK(bins_device(st, B, v, n, grid3, bo, nullptr, tm));
    const size_t ns = (size_t)np * n;
    std::copy(bo.words.begin(), bo.words.begin() + ns, keys);
    *hat = bo.words[ns];
    std::copy(bo.words.begin() + ns + 1, bo.words.end(), cnt);
    return MCX_OK;
  });
}

// ---- pair profiles: the three forms ---------------------------------------------------------------------------------------
extern "C" int mcx_samples_profile2d(mcx_engine *e, int first_step, int nsteps, const mcx_profile2d_spec *spec, mcx_col_profile *cols,
                                     mcx_pair_profile *pairs_out, unsigned long long *cnt, float *lmax, long long *row, float *xat_a,
                                     float *xat_b, double *z, long long *nlevel)
{
  const Profile2dOut o{cols, pairs_out, cnt, lmax, row, xat_a, xat_b, z, nlevel};
  ph::Levels lv;
  std::vector<int> pl;
  return on_store(
      e, first_step, nsteps, [&] { return profile2d_args(spec, e->nparam, (int64_t)nsteps * e->nchain, o, lv, pl); },
      [&](hipStream_t st, Bufs B, const StoreView &v) { return profile2d_device(st, B, v, spec, lv, pl, o, nullptr); });
}

extern "C" int mcx_rows_profile2d(const float *rows, int nsteps, int nc, int np, const mcx_profile2d_spec *spec, mcx_col_profile *cols,
                                  mcx_pair_profile *pairs_out, unsigned long long *cnt, float *lmax, long long *row, float *xat_a, float *xat_b,
                                  double *z, long long *nlevel)
{
  MCXCHK(rows_args(rows, nc, np));
  const Profile2dOut o{cols, pairs_out, cnt, lmax, row, xat_a, xat_b, z, nlevel};
  ph::Levels lv;
  std::vector<int> pl;
  MCXCHK(profile2d_args(spec, np, (int64_t)nsteps * nc, o, lv, pl));
  return on_rows(rows, nsteps, nc, np,
                 [&](hipStream_t st, Bufs B, const StoreView &v) { return profile2d_device(st, B, v, spec, lv, pl, o, nullptr); });
}

extern "C" int mcx_store_profile2d(mcx_store *s, const mcx_profile2d_spec *spec, mcx_col_profile *cols, mcx_pair_profile *pairs_out,
                                   unsigned long long *cnt, float *lmax, long long *row, float *xat_a, float *xat_b, double *z, long long *nlevel)
{
  if (!s) return fail(MCX_ERR_INVALID, "the store s is NULL");
  const Profile2dOut o{cols, pairs_out, cnt, lmax, row, xat_a, xat_b, z, nlevel};
  ph::Levels lv;
  std::vector<int> pl;
  MCXCHK(profile2d_args(spec, s->nout, (int64_t)s->T * s->nc, o, lv, pl));
  HIPCHK(hipSetDevice(s->device));
  return profile2d_device(s->st, s->bufs(), StoreView(s->span()), spec, lv, pl, o, nullptr);
}

extern "C" int mcx_debug_profile2d_times(mcx_engine *e, int first_step, int nsteps, const mcx_profile2d_spec *spec, double *ms)
{
  LetGo lg;
  Profile2dOut o{};
  ph::Levels lv;
  std::vector<int> pl;
  return on_store(
      e, first_step, nsteps,
      [&] {
        if (!ms) return fail(MCX_ERR_INVALID, "ms is NULL");
        if (!spec) return fail(MCX_ERR_INVALID, "the profile spec is NULL");
        std::string why;
        if (spec->g < ph::G_MIN || spec->g > ph::G_MAX) return fail(MCX_ERR_INVALID, "g = %d: %d to %d nodes per axis", spec->g, ph::G_MIN, ph::G_MAX);
        const int rc = ph::pair_list(spec->npairs, spec->pairs, e->nparam, pl, why);
        if (rc) return ph_fail(rc, why);
        o = lg.out2(e->nparam, spec->g, (int)(pl.size() / 2));
        return profile2d_args(spec, e->nparam, (int64_t)nsteps * e->nchain, o, lv, pl);
      },
      [&](hipStream_t st, Bufs B, const StoreView &v) { return profile2d_device(st, B, v, spec, lv, pl, o, ms); });
}

// ---- host only ------------------------------------------------------------------------------------------------------------
extern "C" int mcx_profile_drop(double p, int nparams, double *drop)
{
  if (!drop || (nparams != 1 && nparams != 2)) return fail(MCX_ERR_INVALID, "drop is NULL or nparams = %d is not 1 or 2", nparams);
  if (!(p > 0.0 && p < 1.0)) return fail(MCX_ERR_INVALID, "p = %g is not a confidence level in (0, 1)", p);
  *drop = nparams == 1 ? ph::drop_of_level_1d(p) : ph::drop_of_level_2d(p);
  return MCX_OK;
}

extern "C" int mcx_profile_interval(int n, const double *x, const double *y, double drop, double *lo, double *hi, int *nseg, int *flags)
{
  if (n < 1 || !x || !y || !lo || !hi || !nseg || !flags) return fail(MCX_ERR_INVALID, "bad arguments");
  if (!(drop > 0.0) || !std::isfinite(drop)) return fail(MCX_ERR_INVALID, "drop = %g is not a positive finite drop of log L", drop);
  const ph::Ends e = ph::interval(n, x, y, drop);
  *lo = e.lo;
  *hi = e.hi;
  *nseg = e.nseg;
  *flags = (e.open & 1 ? MCX_PROFILE_OPEN_LO : 0) | (e.open & 2 ? MCX_PROFILE_OPEN_HI : 0) | (e.open & 4 ? MCX_PROFILE_NO_BIN : 0);
  return MCX_OK;
}

extern "C" int mcx_debug_profile_finish(int n, const unsigned long long *keys, const unsigned long long *cnt, const float *xat,
                                        unsigned long long hat, int nlevels, const double *levels, int levels_are_drops, float *lmax,
                                        long long *row, double *pl, double *plh, mcx_profile_interval_t *intervals, long long *nbinned,
                                        int *nempty, int *flags)
{
  if (n < 1 || n > ph::N_MAX || !keys || !cnt || !xat || !lmax || !row || !pl || !plh || !intervals || !nbinned || !nempty || !flags)
    return fail(MCX_ERR_INVALID, "bad arguments");
  ph::Levels lv;
  std::string why;
  const int rc = ph::levels_of(nlevels, levels, levels_are_drops, false, lv, why);
  if (rc) return ph_fail(rc, why);
  std::vector<double> x(n);
  *flags = ph::finish_column(n, reinterpret_cast<const uint64_t *>(keys), reinterpret_cast<const uint64_t *>(cnt), xat, hat, lv, lmax, row,
                             x.data(), pl, plh, reinterpret_cast<ph::Interval *>(intervals), nbinned, nempty);
  return MCX_OK;
}

extern "C" int mcx_debug_profile_geometry(int np, int nsteps, int nc, int n, int g, int npairs, mcx_profile_geometry *o)
{
  if (!o || np < 1 || np > 256 || nsteps < 1 || nc < 1 || n < ph::N_MIN || n > ph::N_MAX || g < ph::G_MIN || g > ph::G_MAX || npairs < 1 ||
      npairs > ph::MAX_PAIRS)
    return fail(MCX_ERR_INVALID, "bad arguments");
  const int64_t N = (int64_t)nsteps * nc;
  const BinsGeometry b = bins_geometry(tiles_x(nullptr, nc, np), nc, nsteps);
  const PairGeometry p = pair_geometry(N, npairs);
  o->block = SB;
  o->tile_columns = b.t.ct;
  o->chains_per_workgroup = b.t.cg;
  o->column_tiles = b.t.ntiles;
  o->chain_blocks = b.t.nbc;
  o->chunk_steps = b.chunk;
  o->chunks = b.chunks;
  o->workgroups = (long long)b.t.nbc * b.t.ntiles * b.chunks;
  o->lds_bytes = (long long)bins_lds_bytes(b.t.ct, n);
  o->unroll = PUNROLL;
  o->pair_block = PB2;
  o->pair_chunk_rows = P2CHUNK;
  o->pair_chunks = p.nchunks;
  o->pair_workgroups = (long long)npairs * p.W;
  o->pair_lds_bytes = (long long)pair_lds_bytes(g);
  o->scratch_bytes = (long long)((size_t)np * 3 * 8 + (2 * (size_t)np * n + 1) * 8 + ((size_t)np * n + np) * 4);
  o->keys_workgroups = keys_workgroups(N);
  o->keys_max_workgroups = KEYS_MAX_WGS;
  return MCX_OK;
}
