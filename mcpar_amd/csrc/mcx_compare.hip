// mcx_compare.hip -- mcx_*_compare: two sample stores compared column by column on the device: the exact
// two-sample Kolmogorov-Smirnov distance in integers, the Wasserstein-1 distance in fp64, each side's mean, sd and ESS
// (mcx_summary.hip's passes, unchanged), and on the host what turns them into a statement (mcx_compare_host.hpp).
//
// Stores A and B have the same columns and any nc and T each; NA = TA * ncA and NB = TB * ncB values per column.  G columns at a time:
//   1. k_cmp_keys        section 11's key sweep without a threshold, over each side's own tiles -> keys[column][N]
//   2. sort_columns      mcx_sort_kernels.hpp: A's columns, then B's, sharing the alternate array and the counts
//   3. k_cmp_bounds      one thread per tile of RTILE sorted keys of self: the upper bound in other of the tile's last key ->
//                        ob[tile + 1], ob[0] = 0.  The bounds of a tile's keys lie in [ob[tile], ob[tile + 1]]: its window
//   4. k_cmp_sweep       once with self = A, once with self = B; grid = (tiles, columns), one key per lane and round.  The lane
//                        whose key ends its tie run finds co = the keys of other that are <= its key inside the window (staged
//                        in LDS when it has at most WIN_LDS keys, else searched in global memory; a round's keys are
//                        consecutive, so 31 searches a tile narrow every lane's search to its round's stretch), forms d = (i + 1) No - co Ns in
//                        int64 and the W1 term |d| (next - x) of the pooled point it owns; the workgroup keeps the maximum of d
//                        with the lowest position and adds the terms in a fixed tree -> a slab per (column, tile)
//   5. k_cmp_reduce      one workgroup per column walks both slabs in tile order -> the two maxima with their values, the W1 sum
// No float atomics and no global atomics: the same stores and arguments give the same bytes.  Every region of the per-call
// scratch is written in full by the launch before the one that reads it.
#include "mcx_sort_kernels.hpp"
#include "mcx_store.hpp"

#include "mcx_compare_host.hpp"

#include <climits>
#include <limits>

namespace {

constexpr int WIN_LDS = RTILE;  // a window of at most this many keys of the other side is searched in LDS
constexpr int WIN_PAD = 8;      // behind them: the key before and the key after the window, and up to three keys of alignment
constexpr int64_t NMAX = (int64_t)1 << 31;
// mcx_debug_compare_times
enum { CT_SUMMARY = 0, CT_KEYS_A, CT_SORT_A, CT_KEYS_B, CT_SORT_B, CT_BOUNDS, CT_SWEEP_A, CT_SWEEP_B, CT_REDUCE, CT_TOTAL, CT_N };

// the value of a key: rkey's inverse (a NaN for the one key of every NaN)
__device__ __forceinline__ double key_value(uint32_t k)
{
  if (k == 0xffffffffu) return __longlong_as_double(0x7ff8000000000000ll);
  return (double)__uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// 1. keys of columns [c0, c1) of a tile set: mcx_ranks.hip's k_rank_keys for the values themselves, which needs no threshold.
// grid = (nbc * ntiles, step chunks)
__global__ void __launch_bounds__(SB) k_cmp_keys(TileSet t, int nc, int64_t T, int c0, int c1, uint32_t *keys, int64_t N, int64_t rchunk)
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

// 3. grid = (ceil(tiles / SB), columns); ob[column][tiles + 1]
__global__ void __launch_bounds__(SB) k_cmp_bounds(const uint32_t *self, int64_t Ns, uint32_t tiles, const uint32_t *other, int64_t No,
                                                   uint32_t *ob)
{
  const uint32_t t = blockIdx.x * SB + threadIdx.x;
  if (t >= tiles) return;
  const uint32_t *s = self + (size_t)blockIdx.y * (size_t)Ns, *o = other + (size_t)blockIdx.y * (size_t)No;
  uint32_t *b = ob + (size_t)blockIdx.y * ((size_t)tiles + 1);
  const int64_t last = min(((int64_t)t + 1) * RTILE, Ns) - 1;
  const uint32_t key = s[last];
  int64_t lo = 0, hi = No;  // lo: the first index of other whose key is above
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (o[mid] <= key) lo = mid + 1; else hi = mid;
  }
  b[t + 1] = (uint32_t)lo;
  if (t == 0) b[0] = 0u;
}

struct CmpSweepArgs {
  const uint32_t *self, *other;  // sorted keys [column][Ns], [column][No]
  int64_t Ns, No;
  const uint32_t *ob;  // [column][tiles + 1]
  uint32_t tiles;
  int self_is_a;
  long long *slab_d;  // [column][tiles] the tile's maximum of d (LLONG_MIN: no tie run ends in it)
  uint32_t *slab_k;   //                 the key at the lowest position that attains it
  double *slab_w;     //                 the tile's W1 terms
};

// (d, position): the larger d, and of equal ones the lower position
__device__ __forceinline__ bool cmp_better(long long d, long long p, long long bd, long long bp) { return d > bd || (d == bd && p < bp); }

// the workgroup's (d, position) and sum, every lane calls it: rd[0], rp[0], rw[0] hold them behind it
__device__ __forceinline__ void cmp_tree(long long *rd, long long *rp, double *rw, int tid)
{
  __syncthreads();
  for (int w = SB / 2; w > 0; w >>= 1) {
    if (tid < w) {
      rw[tid] += rw[tid + w];
      if (cmp_better(rd[tid + w], rp[tid + w], rd[tid], rp[tid])) {
        rd[tid] = rd[tid + w];
        rp[tid] = rp[tid + w];
      }
    }
    __syncthreads();
  }
}

// 4. grid = (tiles of self, columns)
__global__ void __launch_bounds__(SB) k_cmp_sweep(const CmpSweepArgs a)
{
  __shared__ __attribute__((aligned(16))) uint32_t win[WIN_LDS + WIN_PAD];
  __shared__ long long rd[SB], rp[SB];
  __shared__ double rw[SB];
  __shared__ uint32_t split[RKPT + 1];
  const int tid = (int)threadIdx.x;
  const uint32_t tile = blockIdx.x;
  const int64_t Ns = a.Ns, No = a.No;
  const uint32_t *s = a.self + (size_t)blockIdx.y * (size_t)Ns, *o = a.other + (size_t)blockIdx.y * (size_t)No;
  const uint32_t *ob = a.ob + (size_t)blockIdx.y * ((size_t)a.tiles + 1);
  const int64_t lo = ob[tile], hi = ob[tile + 1];                             // lo <= hi <= No
  const int64_t w0 = lo > 0 ? lo - 1 : 0, w1 = hi < No ? hi + 1 : No;  // [w0, w1): what a lane of this tile reads of other
  const bool staged = hi - lo <= WIN_LDS;
  int64_t wa = w0;  // the index of other that win[0] holds
  if (staged) {
    // 16-byte loads from the aligned address at or below o + w0.  The keys of a group's first column start an allocation, so
    // this never reaches below it; a later column's aligned start lies in the column before
    wa = w0 - (int64_t)((reinterpret_cast<uintptr_t>(o + w0) >> 2) & 3u);
    const int64_t nvec = (w1 - wa) >> 2;  // w1 - wa <= WIN_LDS + 2 + 3
    const uint4 *src = reinterpret_cast<const uint4 *>(o + wa);
    for (int64_t v = tid; v < nvec; v += SB) reinterpret_cast<uint4 *>(win)[v] = src[v];
    for (int64_t i = wa + nvec * 4 + tid; i < w1; i += SB) win[i - wa] = o[i];
    __syncthreads();
  }
  // the first index of other in [l, h] whose key is above
  auto upper = [&](int64_t l, int64_t h, uint32_t key) -> int64_t {
    if (staged) {
      while (l < h) {
        const int64_t mid = (l + h) >> 1;
        if (win[mid - wa] <= key) l = mid + 1; else h = mid;
      }
    } else {
      while (l < h) {
        const int64_t mid = (l + h) >> 1;
        if (o[mid] <= key) l = mid + 1; else h = mid;
      }
    }
    return l;
  };
  long long bd = LLONG_MIN, bp = LLONG_MAX;
  double sw = 0.0;
  const int64_t base = (int64_t)tile * RTILE;
  // The keys of round j are consecutive: their bounds lie in [split[j], split[j + 1]], split[j] the bound of the key before the
  // round's first (lo for round 0), and hi from the tile's or the column's last key on.  RKPT - 1 searches of the window a tile
  // then leave every lane a search of its round's stretch
  if (tid <= RKPT) {
    const int64_t at = base + (int64_t)tid * SB - 1;
    split[tid] = (uint32_t)(tid == 0 ? lo : (tid == RKPT || at >= Ns - 1) ? hi : upper(lo, hi, s[at]));
  }
  __syncthreads();
  for (int j = 0; j < RKPT; ++j) {
    const int64_t i = base + (int64_t)j * SB + tid;
    if (i >= Ns) break;
    const uint32_t key = s[i];
    const bool has_next = i + 1 < Ns;
    const uint32_t nk = has_next ? s[i + 1] : 0u;
    if (has_next && nk == key) continue;  // not the end of its tie run
    const int64_t co = upper(split[j], split[j + 1], key);
    const long long d = (long long)(i + 1) * (long long)No - (long long)co * (long long)Ns;
    if (d > bd) {  // (positions rise with j: of equal ones the first stays)
      bd = d;
      bp = i;
    }
    // the pooled point belongs to this sweep when self is A, or when A does not hold the key
    const bool mine = a.self_is_a || co == 0 || (staged ? win[co - 1 - wa] : o[co - 1]) != key;
    const bool has_other = co < No;
    if (mine && (has_next || has_other)) {
      const uint32_t ok = has_other ? (staged ? win[co - wa] : o[co]) : 0u;
      const uint32_t nx = !has_other ? nk : !has_next ? ok : min(nk, ok);
      sw += (double)(d < 0 ? -d : d) * (key_value(nx) - key_value(key));
    }
  }
  rd[tid] = bd;
  rp[tid] = bp;
  rw[tid] = sw;
  cmp_tree(rd, rp, rw, tid);
  if (tid == 0) {
    const size_t at = (size_t)blockIdx.y * a.tiles + tile;
    a.slab_d[at] = rd[0];
    a.slab_k[at] = rd[0] == LLONG_MIN ? 0u : s[rp[0]];
    a.slab_w[at] = rw[0];
  }
}

struct CmpReduceArgs {
  const long long *slab_d[2];  // side 0: self = A, side 1: self = B
  const uint32_t *slab_k[2];
  const double *slab_w[2];
  uint32_t tiles[2];
  long long *out_d;  // [column][2] ks_plus_num, ks_minus_num
  double *out_x;     // [column][2] ks_plus_x, ks_minus_x
  double *out_w;     // [column] the sum of the W1 terms
};

// 5. grid = columns.  A lane takes tiles tid, tid + SB, ... in rising order, then the fixed tree
__global__ void __launch_bounds__(SB) k_cmp_reduce(const CmpReduceArgs a)
{
  __shared__ long long rd[SB], rp[SB];
  __shared__ double rw[SB];
  const int tid = (int)threadIdx.x;
  const size_t col = blockIdx.x;
  double wsum = 0.0;
  for (int side = 0; side < 2; ++side) {
    const uint32_t tiles = a.tiles[side];
    const long long *sd = a.slab_d[side] + col * tiles;
    const double *swp = a.slab_w[side] + col * tiles;
    long long bd = LLONG_MIN, bp = LLONG_MAX;
    double sw = 0.0;
    for (uint32_t t = tid; t < tiles; t += SB) {
      const long long d = sd[t];
      if (d > bd) {
        bd = d;
        bp = t;
      }
      sw += swp[t];
    }
    rd[tid] = bd;
    rp[tid] = bp;
    rw[tid] = sw;
    cmp_tree(rd, rp, rw, tid);
    if (tid == 0) {
      a.out_d[col * 2 + side] = rd[0];
      // (the column's last key ends a run, so some tile holds a maximum and rp[0] is that tile)
      a.out_x[col * 2 + side] = key_value(rp[0] < (long long)tiles ? a.slab_k[side][col * tiles + (size_t)rp[0]] : 0xffffffffu);
      wsum += rw[0];
    }
    __syncthreads();  // (before rd, rp, rw are written again)
  }
  if (tid == 0) a.out_w[col] = wsum;
}

// ---- launch geometry: what the launches below use and mcx_debug_compare_geometry reports
struct CompareGeometry {
  uint32_t tiles_a, tiles_b;    // sort and sweep tiles per column of each side
  uint32_t bounds_a, bounds_b;  // k_cmp_bounds' grid.x: a lane per tile
  int G;  // columns at a time, before any halving for memory
  size_t col_bytes;
};
CompareGeometry compare_geometry(int64_t na, int64_t nb, int ncol)
{
  CompareGeometry g;
  g.tiles_a = (uint32_t)((na + RTILE - 1) / RTILE);
  g.tiles_b = (uint32_t)((nb + RTILE - 1) / RTILE);
  g.G = ncol;
  if (const char *cap = std::getenv("MCX_COMPARE_GROUP_COLS")) g.G = std::max(1, std::min(ncol, std::atoi(cap)));
  const size_t nmax = (size_t)std::max(na, nb), tmax = std::max(g.tiles_a, g.tiles_b), ts = (size_t)g.tiles_a + g.tiles_b;
  g.bounds_a = (g.tiles_a + SB - 1) / SB;
  g.bounds_b = (g.tiles_b + SB - 1) / SB;
  g.col_bytes = 4 * ((size_t)na + (size_t)nb + nmax) + 4 * 256 * (tmax + 1) + 4 * (ts + 2) + (8 + 4 + 8) * ts + (16 + 16 + 8);
  return g;
}

// the scratch of one call, released when it is over
struct CompareScratch {
  DevBuf<uint32_t> ka, kb, alt, hist, rowsum, oba, obb, slab_k;
  DevBuf<long long> slab_d, out_d;
  DevBuf<double> slab_w, out_x, out_w;
  void release()
  {
    ka.release(); kb.release(); alt.release(); hist.release(); rowsum.release(); oba.release(); obb.release(); slab_k.release();
    slab_d.release(); out_d.release(); slab_w.release(); out_x.release(); out_w.release();
  }
};

int compare_scratch(CompareScratch &S, const CompareGeometry &g, int64_t na, int64_t nb, int *Gout)
{
  const size_t nmax = (size_t)std::max(na, nb), tmax = std::max(g.tiles_a, g.tiles_b), ts = (size_t)g.tiles_a + g.tiles_b;
  for (int G = g.G;; G = (G + 1) / 2) {
    const size_t k = (size_t)G;
    const bool ok = S.ka.alloc(k * (size_t)na) == MCX_OK && S.kb.alloc(k * (size_t)nb) == MCX_OK && S.alt.alloc(k * nmax) == MCX_OK &&
                    S.hist.alloc(k * 256 * tmax) == MCX_OK && S.rowsum.alloc(k * 256) == MCX_OK &&
                    S.oba.alloc(k * ((size_t)g.tiles_a + 1)) == MCX_OK && S.obb.alloc(k * ((size_t)g.tiles_b + 1)) == MCX_OK &&
                    S.slab_d.alloc(k * ts) == MCX_OK && S.slab_k.alloc(k * ts) == MCX_OK && S.slab_w.alloc(k * ts) == MCX_OK &&
                    S.out_d.alloc(k * 2) == MCX_OK && S.out_x.alloc(k * 2) == MCX_OK && S.out_w.alloc(k) == MCX_OK;
    if (ok) {
      *Gout = G;
      return MCX_OK;
    }
    if (G == 1)
      return fail(MCX_ERR_ALLOC, "compare: %zu bytes of scratch are needed for one column at a time (DESIGN.md section 20)", g.col_bytes);
    S.release();  // mid-life: room for the next, smaller try
  }
}

// mean, sd, ess and the flag of every column of one side -> cs (mean, sd, ess, flags are read)
int side_summary(hipStream_t st, Bufs B, const StoreView &v, bool iid, std::vector<mcx_col_summary> &cs)
{
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  cs.assign((size_t)v.ncol, mcx_col_summary{});
  if (!iid && v.T >= 4) return summary_mixing(st, B, v, cs.data());
  double none = 0.0;  // (no probabilities: nothing is written through it)
  if (v.N >= 2) MCXCHK(summary_spread(st, B, v, nullptr, 0, cs.data(), &none));
  else MCXCHK(summary_thresholds(st, B, v, nullptr, 0, cs.data(), nullptr));
  for (mcx_col_summary &c : cs) {
    const bool bad = c.flags & MCX_SUMMARY_NONFINITE;
    c.ess = bad ? qnan : (double)v.N;
    if (v.N < 2) c.sd = qnan;
  }
  return MCX_OK;
}

// keys of columns [c0, c1) of a view -> keys[column - c0][N]
int launch_keys(hipStream_t st, const StoreView &v, int c0, int c1, uint32_t *keys)
{
  const RankGeometry rg = rank_geometry(v.T, v.N);
  for (const TileSet *t : {&v.tx, &v.tl}) {
    if (t->col0 + t->ncs <= c0 || t->col0 >= c1) continue;
    hipLaunchKernelGGL(k_cmp_keys, dim3((unsigned)(t->nbc * t->ntiles), rg.chunks), dim3(SB), 0, st, *t, v.nc, v.T, c0, c1, keys, v.N,
                       rg.rchunk);
    HIPCHK(hipGetLastError());
  }
  return MCX_OK;
}

int compare_flags(const mcx_compare_spec *spec, int *flags)
{
  *flags = spec ? spec->flags : 0;
  if (*flags & ~MCX_COMPARE_IID) return fail(MCX_ERR_INVALID, "spec.flags = %d: MCX_COMPARE_IID or 0", *flags);
  return MCX_OK;
}

// what every comparison refuses of its two sides before anything is allocated
int compare_sides(int ncol_a, int64_t na, int ncol_b, int64_t nb)
{
  if (ncol_a != ncol_b) return fail(MCX_ERR_INVALID, "compare: A has %d columns and B %d", ncol_a, ncol_b);
  if (na < 1 || nb < 1) return fail(MCX_ERR_INVALID, "compare: %lld and %lld values per column, at least one each", (long long)na, (long long)nb);
  if (na >= NMAX || nb >= NMAX)
    return fail(MCX_ERR_UNSUPPORTED, "compare: %lld and %lld values per column, fewer than 2^31 are supported", (long long)na,
                (long long)nb);
  return MCX_OK;
}

// the comparison of two views on stream st (B's memory is ready: its stream is idle, or it is st).  ms (CT_N doubles): the
// stages' times
int compare_device(hipStream_t st, Bufs B, const StoreView &va, const StoreView &vb, int flags, mcx_col_compare *cols, double *ms)
{
  MCXCHK(compare_sides(va.ncol, va.N, vb.ncol, vb.N));
  const int ncol = va.ncol;
  const int64_t na = va.N, nb = vb.N;
  const bool iid = flags & MCX_COMPARE_IID;
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  StageTimer tm{st, ms, CT_N, {}};
  const CompareGeometry g = compare_geometry(na, nb, ncol);
  CompareScratch S;
  std::vector<mcx_col_summary> sa, sb;
  std::vector<long long> hd(2 * (size_t)ncol);
  std::vector<double> hx(2 * (size_t)ncol), hw((size_t)ncol);
  auto run = [&]() -> int {
    MCXCHK(tm.run(CT_SUMMARY, [&]() -> int {
      MCXCHK(side_summary(st, B, va, iid, sa));
      return side_summary(st, B, vb, iid, sb);
    }));
    int G = 0;
    MCXCHK(compare_scratch(S, g, na, nb, &G));
    for (int c0 = 0; c0 < ncol; c0 += G) {
      const int c1 = std::min(ncol, c0 + G);
      const unsigned k = (unsigned)(c1 - c0);
      MCXCHK(tm.run(CT_KEYS_A, [&]() -> int { return launch_keys(st, va, c0, c1, S.ka.p); }));
      MCXCHK(sort_columns(st, S.ka.p, S.alt.p, S.hist.p, S.rowsum.p, na, k, g.tiles_a,
                          [&](int, auto f) -> int { return tm.run(CT_SORT_A, f); }));
      MCXCHK(tm.run(CT_KEYS_B, [&]() -> int { return launch_keys(st, vb, c0, c1, S.kb.p); }));
      MCXCHK(sort_columns(st, S.kb.p, S.alt.p, S.hist.p, S.rowsum.p, nb, k, g.tiles_b,
                          [&](int, auto f) -> int { return tm.run(CT_SORT_B, f); }));
      MCXCHK(tm.run(CT_BOUNDS, [&]() -> int {
        hipLaunchKernelGGL(k_cmp_bounds, dim3(g.bounds_a, k), dim3(SB), 0, st, (const uint32_t *)S.ka.p, na, g.tiles_a,
                           (const uint32_t *)S.kb.p, nb, S.oba.p);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_cmp_bounds, dim3(g.bounds_b, k), dim3(SB), 0, st, (const uint32_t *)S.kb.p, nb, g.tiles_b,
                           (const uint32_t *)S.ka.p, na, S.obb.p);
        HIPCHK(hipGetLastError());
        return MCX_OK;
      }));
      const size_t offb = (size_t)k * g.tiles_a;  // B's slabs lie behind A's
      const CmpSweepArgs wa{S.ka.p, S.kb.p, na, nb, S.oba.p, g.tiles_a, 1, S.slab_d.p, S.slab_k.p, S.slab_w.p};
      const CmpSweepArgs wb{S.kb.p, S.ka.p, nb, na, S.obb.p, g.tiles_b, 0, S.slab_d.p + offb, S.slab_k.p + offb, S.slab_w.p + offb};
      MCXCHK(tm.run(CT_SWEEP_A, [&]() -> int {
        hipLaunchKernelGGL(k_cmp_sweep, dim3(g.tiles_a, k), dim3(SB), 0, st, wa);
        HIPCHK(hipGetLastError());
        return MCX_OK;
      }));
      MCXCHK(tm.run(CT_SWEEP_B, [&]() -> int {
        hipLaunchKernelGGL(k_cmp_sweep, dim3(g.tiles_b, k), dim3(SB), 0, st, wb);
        HIPCHK(hipGetLastError());
        return MCX_OK;
      }));
      const CmpReduceArgs ra{{wa.slab_d, wb.slab_d}, {wa.slab_k, wb.slab_k}, {wa.slab_w, wb.slab_w}, {g.tiles_a, g.tiles_b},
                             S.out_d.p, S.out_x.p, S.out_w.p};
      MCXCHK(tm.run(CT_REDUCE, [&]() -> int {
        hipLaunchKernelGGL(k_cmp_reduce, dim3(k), dim3(SB), 0, st, ra);
        HIPCHK(hipGetLastError());
        return MCX_OK;
      }));
      HIPCHK(hipMemcpyAsync(hd.data() + 2 * (size_t)c0, S.out_d.p, 2 * (size_t)k * sizeof(long long), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(hx.data() + 2 * (size_t)c0, S.out_x.p, 2 * (size_t)k * sizeof(double), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(hw.data() + (size_t)c0, S.out_w.p, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));  // (the next group writes the same scratch)
    }
    return MCX_OK;
  };
  const int rc = tm.run(CT_TOTAL, run);
  if (rc != MCX_OK) (void)hipStreamSynchronize(st);  // (hd, hx, hw and the scratch are the stream's until here)
  MCXCHK(rc);
  for (int c = 0; c < ncol; ++c) {
    mcx_col_compare &o = cols[c];
    o = mcx_col_compare{};
    o.na = na;
    o.nb = nb;
    o.ks_plus_num = hd[2 * (size_t)c];
    o.ks_minus_num = hd[2 * (size_t)c + 1];
    o.ks_plus_x = hx[2 * (size_t)c];
    o.ks_minus_x = hx[2 * (size_t)c + 1];
    o.ks = (double)std::max(o.ks_plus_num, o.ks_minus_num) / ((double)na * (double)nb);
    o.flags = ((sa[c].flags & MCX_SUMMARY_NONFINITE) ? MCX_COMPARE_NONFINITE_A : 0) |
              ((sb[c].flags & MCX_SUMMARY_NONFINITE) ? MCX_COMPARE_NONFINITE_B : 0);
    o.mean_a = sa[c].mean; o.sd_a = sa[c].sd; o.ess_a = sa[c].ess;
    o.mean_b = sb[c].mean; o.sd_b = sb[c].sd; o.ess_b = sb[c].ess;
    if (o.flags & MCX_COMPARE_NONFINITE_A) o.mean_a = o.sd_a = o.ess_a = qnan;
    if (o.flags & MCX_COMPARE_NONFINITE_B) o.mean_b = o.sd_b = o.ess_b = qnan;
    if (o.flags) {
      o.w1 = o.z_mean = o.ks_neff = o.ks_p = qnan;
      continue;
    }
    o.w1 = hw[c] / ((double)na * (double)nb);
    o.z_mean = mcx_compare_host::z_mean(o.mean_a, o.sd_a, o.ess_a, o.mean_b, o.sd_b, o.ess_b);
    mcx_compare_host::ks_prob(o.ks, o.ess_a, o.ess_b, &o.ks_neff, &o.ks_p);
  }
  return tm.collect();
}

int engine_range(const mcx_engine *e, int first, int nsteps, const char *side)
{
  if (first < 0 || (int64_t)first + nsteps > e->samp_steps)
    return fail(MCX_ERR_INVALID, "%s: steps [%d,%lld) not in the sample store (%d steps)", side, first, (long long)first + nsteps,
                e->samp_steps);
  return MCX_OK;
}

int samples_compare(mcx_engine *e, int first_a, int nsteps_a, int first_b, int nsteps_b, const mcx_compare_spec *spec,
                    mcx_col_compare *cols, double *ms)
{
  int flags = 0;
  return on_store(
      e, first_a, nsteps_a,
      [&]() -> int {
        if (!cols) return fail(MCX_ERR_INVALID, "cols is NULL");
        MCXCHK(compare_flags(spec, &flags));
        if (nsteps_a < 1 || nsteps_b < 1)
          return fail(MCX_ERR_INVALID, "nsteps_a = %d, nsteps_b = %d: ranges of at least one step", nsteps_a, nsteps_b);
        return compare_sides(e->nparam + 1, (int64_t)nsteps_a * e->nchain, e->nparam + 1, (int64_t)nsteps_b * e->nchain);
      },
      [&](hipStream_t st, Bufs B, const StoreView &va) {
        MCXCHK(engine_range(e, first_b, nsteps_b, "B"));
        const size_t nc = (size_t)e->nchain, np = (size_t)e->nparam;
        const StoreView vb(StoreSpan{e->samp_x.p + (size_t)first_b * nc * np, e->samp_ly.p + (size_t)first_b * nc, (int)nc, (int)np, nsteps_b});
        return compare_device(st, B, va, vb, flags, cols, ms);
      });
}

}  // namespace

extern "C" int mcx_store_compare(mcx_store *a, mcx_store *b, const mcx_compare_spec *spec, mcx_col_compare *cols)
{
  if (!a || !b) return fail(MCX_ERR_INVALID, "the store %s is NULL", a ? "b" : "a");
  if (!cols) return fail(MCX_ERR_INVALID, "cols is NULL");
  int flags = 0;
  MCXCHK(compare_flags(spec, &flags));
  MCXCHK(compare_sides(a->nout + 1, (int64_t)a->T * a->nc, b->nout + 1, (int64_t)b->T * b->nc));
  if (a->device != b->device) return fail(MCX_ERR_INVALID, "compare: A is on device %d and B on device %d", a->device, b->device);
  HIPCHK(hipSetDevice(a->device));
  if (b != a && b->st) HIPCHK(hipStreamSynchronize(b->st));
  return compare_device(a->st, a->bufs(), StoreView(a->span()), StoreView(b->span()), flags, cols, nullptr);
}

extern "C" int mcx_rows_compare(const float *rows_a, int nsteps_a, int nc_a, const float *rows_b, int nsteps_b, int nc_b, int np,
                                const mcx_compare_spec *spec, mcx_col_compare *cols)
{
  if (!rows_a || !rows_b) return fail(MCX_ERR_INVALID, "rows_%s is NULL", rows_a ? "b" : "a");
  if (!cols) return fail(MCX_ERR_INVALID, "cols is NULL");
  int flags = 0;
  MCXCHK(compare_flags(spec, &flags));
  if (np < 1 || np > 256) return fail(MCX_ERR_INVALID, "np = %d: 1 to 256 parameters", np);
  if (nsteps_a < 1 || nc_a < 1 || nsteps_b < 1 || nc_b < 1)
    return fail(MCX_ERR_INVALID, "A is %d steps of %d chains, B %d of %d: at least one step of one chain each", nsteps_a, nc_a, nsteps_b, nc_b);
  MCXCHK(compare_sides(np + 1, (int64_t)nsteps_a * nc_a, np + 1, (int64_t)nsteps_b * nc_b));
  return on_rows(rows_a, nsteps_a, nc_a, np, [&](hipStream_t st, Bufs B, const StoreView &va) {
    return on_rows(rows_b, nsteps_b, nc_b, np, [&](hipStream_t stb, Bufs, const StoreView &vb) {
      HIPCHK(hipStreamSynchronize(stb));  // B's upload
      return compare_device(st, B, va, vb, flags, cols, nullptr);
    });
  });
}

extern "C" int mcx_samples_compare(mcx_engine *e, int first_a, int nsteps_a, int first_b, int nsteps_b, const mcx_compare_spec *spec,
                                   mcx_col_compare *cols)
{
  return samples_compare(e, first_a, nsteps_a, first_b, nsteps_b, spec, cols, nullptr);
}

extern "C" int mcx_debug_compare_times(mcx_engine *e, int first_a, int nsteps_a, int first_b, int nsteps_b, const mcx_compare_spec *spec,
                                       double *ms)
{
  if (!ms) return fail(MCX_ERR_INVALID, "ms is NULL");
  std::vector<mcx_col_compare> cols(e ? (size_t)e->nparam + 1 : 1);
  return samples_compare(e, first_a, nsteps_a, first_b, nsteps_b, spec, cols.data(), ms);
}

extern "C" int mcx_samples_compare_store(mcx_engine *e, int first_step, int nsteps, mcx_store *b, const mcx_compare_spec *spec,
                                         mcx_col_compare *cols)
{
  int flags = 0;
  return on_store(
      e, first_step, nsteps,
      [&]() -> int {
        if (!b) return fail(MCX_ERR_INVALID, "the store b is NULL");
        if (!cols) return fail(MCX_ERR_INVALID, "cols is NULL");
        MCXCHK(compare_flags(spec, &flags));
        if (nsteps < 1) return fail(MCX_ERR_INVALID, "nsteps = %d: a range of at least one step", nsteps);
        MCXCHK(compare_sides(e->nparam + 1, (int64_t)nsteps * e->nchain, b->nout + 1, (int64_t)b->T * b->nc));
        if (e->device != b->device) return fail(MCX_ERR_INVALID, "compare: the engine is on device %d and B on device %d", e->device, b->device);
        return MCX_OK;
      },
      [&](hipStream_t st, Bufs B, const StoreView &va) {
        if (b->st) HIPCHK(hipStreamSynchronize(b->st));
        return compare_device(st, B, va, StoreView(b->span()), flags, cols, nullptr);
      });
}

// host only
extern "C" int mcx_ks_prob(double ks, double ess_a, double ess_b, double *neff, double *p)
{
  if (!neff || !p) return fail(MCX_ERR_INVALID, "neff or p is NULL");
  if (ks < 0.0 || ks > 1.0) return fail(MCX_ERR_INVALID, "ks = %g is not in [0, 1]", ks);
  if (ess_a <= 0.0 || ess_b <= 0.0) return fail(MCX_ERR_INVALID, "ess_a = %g, ess_b = %g: effective sizes are positive", ess_a, ess_b);
  mcx_compare_host::ks_prob(ks, ess_a, ess_b, neff, p);
  return MCX_OK;
}

// host only
extern "C" int mcx_debug_compare_geometry(long long na, long long nb, int ncol, mcx_compare_geometry *g)
{
  if (!g) return fail(MCX_ERR_INVALID, "g is NULL");
  if (ncol < 2 || ncol > 257) return fail(MCX_ERR_INVALID, "ncol = %d: 2 to 257 columns", ncol);
  MCXCHK(compare_sides(ncol, na, ncol, nb));
  const CompareGeometry c = compare_geometry(na, nb, ncol);
  g->block = SB;
  g->tile_keys = RTILE;
  g->tiles_a = c.tiles_a;
  g->tiles_b = c.tiles_b;
  g->window_lds_keys = WIN_LDS;
  g->lds_bytes = (long long)((WIN_LDS + WIN_PAD + RKPT + 1) * sizeof(uint32_t) + SB * (2 * sizeof(long long) + sizeof(double)));
  g->group_cols = c.G;
  g->scratch_bytes_per_col = (long long)c.col_bytes;
  g->sort_tiles_a = c.tiles_a;
  g->sort_tiles_b = c.tiles_b;
  g->bounds_workgroups_a = c.bounds_a;
  g->bounds_workgroups_b = c.bounds_b;
  g->step_chunk_a = g->step_chunk_b = g->grid_y_a = g->grid_y_b = 0;
  return MCX_OK;
}

extern "C" int mcx_debug_compare_store_geometry(int nsteps_a, int nc_a, int nsteps_b, int nc_b, int ncol, mcx_compare_geometry *g)
{
  if (nsteps_a < 1 || nc_a < 1 || nsteps_b < 1 || nc_b < 1)
    return fail(MCX_ERR_INVALID, "compare: %d steps of %d chains and %d of %d, at least one each", nsteps_a, nc_a, nsteps_b, nc_b);
  MCXCHK(mcx_debug_compare_geometry((long long)nsteps_a * nc_a, (long long)nsteps_b * nc_b, ncol, g));
  const RankGeometry ra = rank_geometry(nsteps_a, (int64_t)nsteps_a * nc_a), rb = rank_geometry(nsteps_b, (int64_t)nsteps_b * nc_b);
  g->step_chunk_a = ra.rchunk;
  g->step_chunk_b = rb.rchunk;
  g->grid_y_a = ra.chunks;
  g->grid_y_b = rb.chunks;
  return MCX_OK;
}
