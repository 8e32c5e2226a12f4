// mcx_ranks.hip -- mcx_samples_rank_summary / mcx_rows_rank_summary: rank-normalised split R-hat, bulk-ESS and tail-ESS of a
// step range of the sample store on the device (Vehtari, Gelman, Simpson, Carpenter & Buerkner 2021).
//
// The store is x[step][chain][np] plus ly[step][chain]; N = T * nc values per column.  What is new here is the exact pooled
// rank of every value (ties averaged) and the stores made of it; R-hat and ESS of those stores are mcx_summary.hip's passes,
// unchanged (summary_thresholds, summary_mixing).  Per transform that needs ranks (the values, and their distance from the median):
//   1. k_rank_keys       one sweep of the store in mcx_summary.hip's tiles: an order-preserving 32-bit key per value
//                        (-0 and +0 the same key) into keys[column][N], index = step * nc + chain
//   2. sort_columns      mcx_sort_kernels.hpp (shared with mcx_compare.hip): the LSD radix sort of every column's keys, four
//                        passes of { k_rank_hist, k_rank_rowsum, k_rank_scan, k_rank_scatter }
//   3. k_rank_transform  the same sweep as 1: a value's key finds its lower and upper bound lo, hi in its column's sorted
//                        keys, r = (lo + hi + 1) / 2, z = float(PPND16((r - 3/8) / (N + 1/4))) -> a store-shaped scratch
// The tail indicators need no ranks (k_rank_transform, what = 2, 3).  No float atomics anywhere; the same store and arguments
// give the same bytes.
#include "mcx_sort_kernels.hpp"
#include "mcx_ppnd16.hpp"

#include <limits>

namespace {

constexpr int64_t RCHUNK = 64;       // steps per workgroup of the key and transform sweeps (more when T > 2^21: grid.y stays below 2^15)

enum { RANK_BULK = 0, RANK_FOLD = 1, RANK_I05 = 2, RANK_I95 = 3 };
// mcx_debug_rank_summary_times: ms[s * RT_PER + ...] for s = bulk, fold; then the indicators, the thresholds, the whole call
enum { RT_KEYS = 0, RT_PASS0 = 1, RT_TRANSFORM = 5, RT_SUMMARY = 6, RT_PER = 7, RT_I05 = 14, RT_I05_SUMMARY = 15, RT_I95 = 16,
       RT_I95_SUMMARY = 17, RT_THRESHOLDS = 18, RT_TOTAL = 19, RT_N = 20 };

// what is ranked: the value, or (RANK_FOLD) its distance from the column's median, rounded to float
__device__ __forceinline__ float ranked_value(float v, int what, double med)
{
  return what == RANK_FOLD ? (float)fabs((double)v - med) : v;
}

// 1. keys of columns [c0, c1) of a tile set.  grid = (nbc * ntiles, step chunks); thr[3][ncol] = q05, median, q95
__global__ void __launch_bounds__(SB) k_rank_keys(TileSet t, int nc, int64_t T, int what, const double *thr, int ncol, int c0,
                                                  int c1, uint32_t *keys, int64_t N, int64_t rchunk)
{
  const int tile = blockIdx.x % t.ntiles, bc = blockIdx.x / t.ntiles;
  const Lane l = lane_of(t, tile, bc, nc);
  const int col = t.col0 + l.lcol;
  if (!l.ok || col < c0 || col >= c1) return;
  const double med = thr[ncol + col];
  const float *p = t.src + (size_t)l.chain * t.cs + l.lcol;
  uint32_t *k = keys + (size_t)(col - c0) * (size_t)N + l.chain;
  const int64_t s0 = (int64_t)blockIdx.y * rchunk, s1 = min(T, s0 + rchunk);
  for (int64_t s = s0; s < s1; ++s) k[s * nc] = rkey(ranked_value(p[s * t.rs], what, med));
}

// 3. the transformed store.  what = RANK_BULK / RANK_FOLD: normal scores of the ranks, columns [c0, c1), sorted[column - c0][N];
// RANK_I05 / RANK_I95: the tail indicators, every column.  dst has the layout of t.src; ranks (may be NULL): [N][ncol]
__global__ void __launch_bounds__(SB) k_rank_transform(TileSet t, int nc, int64_t T, int what, const double *thr, int ncol,
                                                       int c0, int c1, const uint32_t *sorted, int64_t N, float *dst,
                                                       double *ranks, int64_t rchunk)
{
  const int tile = blockIdx.x % t.ntiles, bc = blockIdx.x / t.ntiles;
  const Lane l = lane_of(t, tile, bc, nc);
  const int col = t.col0 + l.lcol;
  if (!l.ok || col < c0 || col >= c1) return;
  const size_t off = (size_t)l.chain * t.cs + l.lcol;
  const float *p = t.src + off;
  float *q = dst + off;
  const int64_t s0 = (int64_t)blockIdx.y * rchunk, s1 = min(T, s0 + rchunk);
  if (what >= RANK_I05) {
    const double lim = thr[(what == RANK_I05 ? 0 : 2) * ncol + col];
    for (int64_t s = s0; s < s1; ++s) q[s * t.rs] = (double)p[s * t.rs] <= lim ? 1.0f : 0.0f;
    return;
  }
  const double med = thr[ncol + col];
  const uint32_t *sk = sorted + (size_t)(col - c0) * (size_t)N;
  const double denom = (double)N + 0.25;
  for (int64_t s = s0; s < s1; ++s) {
    const uint32_t key = rkey(ranked_value(p[s * t.rs], what, med));
    int64_t lo = 0, hi = N;  // lo: the first index whose key is not below
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (sk[mid] < key) lo = mid + 1; else hi = mid;
    }
    // the end of the tie run, galloping: a run is a chain's rejections, short against N
    int64_t a = lo, step = 1;
    while (a + step < N && sk[a + step] == key) {
      a += step;
      step <<= 1;
    }
    int64_t b = min(a + step, N);  // sk[a] == key; sk[b] > key or b == N
    while (b - a > 1) {
      const int64_t mid = (a + b) >> 1;
      if (sk[mid] == key) a = mid; else b = mid;
    }
    hi = a + 1;
    const double r = (double)(lo + hi + 1) * 0.5;
    q[s * t.rs] = (float)mcx_ppnd16((r - 0.375) / denom);
    if (ranks) ranks[((size_t)s * nc + l.chain) * ncol + col] = r;
  }
}

struct RankDebug {
  int what;
  double *ranks;    // host [N][ncol], or NULL
  float *out_rows;  // host [N][ncol]
};

// the scratch of one call, released when it is over: the transformed store, the keys (two arrays the sort passes alternate
// between), the sort's counts, the thresholds
struct RankScratch {
  DevBuf<float> xs, lys;
  DevBuf<uint32_t> ka, kb, hist, rowsum;
  DevBuf<double> thr, ranks;
};

// one rank-normalised summary of a view: what its stages share
struct RankPass {
  hipStream_t st;
  Bufs B;
  const StoreView &v;
  StageTimer tm;
  RankScratch S;
  bool want_ranks;  // mcx_debug_rows_rank_transform: k_rank_transform also writes the average ranks
  int G = 0;        // columns sorted at a time (rank_scratch)
  int64_t rchunk;   // steps per workgroup of the key and transform sweeps
  unsigned chunks;  // their grid.y
  uint32_t nblk;    // sort tiles per column
  std::vector<mcx_col_summary> c0s;  // thresholds: the flags
  std::vector<double> thr;           // thresholds: [3][ncol] q05, median, q95 (S.thr on the device)

  RankPass(hipStream_t st_, Bufs B_, const StoreView &v_, double *ms, bool want_ranks_)
      : st(st_), B(B_), v(v_), tm{st_, ms, RT_N, {}}, want_ranks(want_ranks_), c0s(v_.ncol), thr(3 * (size_t)v_.ncol)
  {
    const RankGeometry g = rank_geometry(v_.T, v_.N);
    rchunk = g.rchunk; chunks = g.chunks; nblk = g.nblk;
  }
};

// the thresholds: the order-statistics pass of the summary, once -> c0s, thr, S.thr
int thresholds(RankPass &p)
{
  const int ncol = p.v.ncol;
  const double probs[3] = {0.05, 0.5, 0.95};
  std::vector<double> q(3 * (size_t)ncol);
  MCXCHK(p.tm.run(RT_THRESHOLDS, [&]() -> int { return summary_thresholds(p.st, p.B, p.v, probs, 3, p.c0s.data(), q.data()); }));
  for (int c = 0; c < ncol; ++c)
    for (int k = 0; k < 3; ++k) p.thr[(size_t)k * ncol + c] = q[(size_t)c * 3 + k];
  MCXCHK(p.S.thr.alloc(p.thr.size()));
  HIPCHK(hipMemcpyAsync(p.S.thr.p, p.thr.data(), p.thr.size() * sizeof(double), hipMemcpyHostToDevice, p.st));
  return MCX_OK;
}

// the scratch: the transformed store, and keys for as many columns at a time as fit -> G
int rank_scratch(RankPass &p)
{
  const int ncol = p.v.ncol;
  const size_t N = (size_t)p.v.N;
  RankScratch &S = p.S;
  MCXCHK(S.xs.alloc(N * p.v.np));
  MCXCHK(S.lys.alloc(N));
  if (p.want_ranks) MCXCHK(S.ranks.alloc(N * ncol));
  int G = ncol;
  if (const char *cap = std::getenv("MCX_RANK_GROUP_COLS")) G = std::max(1, std::min(ncol, std::atoi(cap)));
  for (;; G = (G + 1) / 2) {
    const bool ok = S.ka.alloc((size_t)G * N) == MCX_OK && S.kb.alloc((size_t)G * N) == MCX_OK &&
                    S.hist.alloc((size_t)G * 256 * p.nblk) == MCX_OK && S.rowsum.alloc((size_t)G * 256) == MCX_OK;
    if (ok) break;
    if (G == 1)
      return fail(MCX_ERR_ALLOC, "rank summary: %zu bytes of scratch are needed for one column at a time (DESIGN.md section 11)",
                  N * ncol * 4 + N * 8 + ((size_t)p.nblk + 1) * 1024 + (size_t)ncol * 24);
    S.ka.release(); S.kb.release(); S.hist.release(); S.rowsum.release();  // mid-life: room for the next, smaller try
  }
  p.G = G;
  return MCX_OK;
}

// the keys of columns [c0, c1) -> S.ka, then their LSD radix sort: four passes, after which the sorted keys are back in S.ka
int sort_group(RankPass &p, int what, int c0, int c1)
{
  const StoreView &v = p.v;
  RankScratch &S = p.S;
  const int t0 = what * RT_PER;
  const unsigned g = (unsigned)(c1 - c0);
  const uint32_t nblk = p.nblk;
  MCXCHK(p.tm.run(t0 + RT_KEYS, [&]() -> int {
    for (const TileSet *t : {&v.tx, &v.tl}) {
      if (t->col0 + t->ncs <= c0 || t->col0 >= c1) continue;
      hipLaunchKernelGGL(k_rank_keys, dim3((unsigned)(t->nbc * t->ntiles), p.chunks), dim3(SB), 0, p.st, *t, v.nc, v.T, what,
                         (const double *)S.thr.p, v.ncol, c0, c1, S.ka.p, v.N, p.rchunk);
      HIPCHK(hipGetLastError());
    }
    return MCX_OK;
  }));
  return sort_columns(p.st, S.ka.p, S.kb.p, S.hist.p, S.rowsum.p, v.N, g, nblk,
                      [&](int pass, auto f) -> int { return p.tm.run(t0 + RT_PASS0 + pass, f); });
}

// k_rank_transform of columns [c0, c1) -> S.xs, S.lys, timed in slot
int transform(RankPass &p, int what, int c0, int c1, int slot)
{
  const StoreView &v = p.v;
  RankScratch &S = p.S;
  return p.tm.run(slot, [&]() -> int {
    for (const TileSet *t : {&v.tx, &v.tl}) {
      if (t->col0 + t->ncs <= c0 || t->col0 >= c1) continue;
      hipLaunchKernelGGL(k_rank_transform, dim3((unsigned)(t->nbc * t->ntiles), p.chunks), dim3(SB), 0, p.st, *t, v.nc, v.T, what,
                         (const double *)S.thr.p, v.ncol, c0, c1, (const uint32_t *)S.ka.p, v.N, t == &v.tx ? S.xs.p : S.lys.p,
                         p.want_ranks ? S.ranks.p : (double *)nullptr, p.rchunk);
      HIPCHK(hipGetLastError());
    }
    return MCX_OK;
  });
}

// z of the ranks of the values (RANK_BULK) or of their distances from the median (RANK_FOLD) -> S.xs, S.lys, G columns at a time
int normal_scores(RankPass &p, int what)
{
  for (int c0 = 0; c0 < p.v.ncol; c0 += p.G) {
    const int c1 = std::min(p.v.ncol, c0 + p.G);
    MCXCHK(sort_group(p, what, c0, c1));
    MCXCHK(transform(p, what, c0, c1, what * RT_PER + RT_TRANSFORM));
  }
  return MCX_OK;
}

// mcx_debug_rows_rank_transform: stop behind transform dbg.what and copy it out as rows
int rank_debug_copy_out(RankPass &p, const RankDebug &dbg)
{
  const int ncol = p.v.ncol, np = p.v.np;
  const size_t N = (size_t)p.v.N;
  if (dbg.what <= RANK_FOLD) MCXCHK(normal_scores(p, dbg.what));
  else MCXCHK(transform(p, dbg.what, 0, ncol, RT_I05));
  std::vector<float> hx(N * np), hl(N);
  HIPCHK(hipMemcpyAsync(hx.data(), p.S.xs.p, hx.size() * sizeof(float), hipMemcpyDeviceToHost, p.st));
  HIPCHK(hipMemcpyAsync(hl.data(), p.S.lys.p, hl.size() * sizeof(float), hipMemcpyDeviceToHost, p.st));
  if (dbg.ranks) HIPCHK(hipMemcpyAsync(dbg.ranks, p.S.ranks.p, N * ncol * sizeof(double), hipMemcpyDeviceToHost, p.st));
  HIPCHK(hipStreamSynchronize(p.st));
  for (size_t r = 0; r < N; ++r) {
    std::memcpy(dbg.out_rows + r * ncol, hx.data() + r * np, (size_t)np * sizeof(float));
    dbg.out_rows[r * ncol + np] = hl[r];
  }
  return MCX_OK;
}

// R-hat and ESS of the transformed store S.xs, S.lys -> cs (rhat, ess, ess_lag), timed in slot
int mixing(RankPass &p, int slot, std::vector<mcx_col_summary> &cs)
{
  return p.tm.run(slot, [&]() -> int {
    return summary_mixing(p.st, p.B, StoreSpan{p.S.xs.p, p.S.lys.p, p.v.nc, p.v.np, p.v.T}, cs.data());
  });
}

inline double nan_max(double a, double b) { return a != a || b != b ? std::numeric_limits<double>::quiet_NaN() : std::max(a, b); }
inline double nan_min(double a, double b) { return a != a || b != b ? std::numeric_limits<double>::quiet_NaN() : std::min(a, b); }

// rhat and ess_tail of every column from its parts; a column that is not finite is NaN throughout
void assemble(mcx_col_rank_summary *out, int ncol)
{
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  for (int c = 0; c < ncol; ++c) {
    mcx_col_rank_summary &o = out[c];
    if (o.flags & MCX_SUMMARY_NONFINITE) {
      o.rhat = o.rhat_bulk = o.rhat_folded = o.ess_bulk = o.ess_tail = o.ess_q05 = o.ess_q95 = o.q05 = o.median = o.q95 = qnan;
      o.ess_bulk_lag = 0;
      continue;
    }
    o.rhat = nan_max(o.rhat_bulk, o.rhat_folded);
    o.ess_tail = nan_min(o.ess_q05, o.ess_q95);
  }
}

// the rank-normalised summary of a view on stream st, the stages of DESIGN.md section 11 in their order.  dbg: stop behind
// that transform and copy it out; ms (RT_N doubles): the stages' times
int rank_device(hipStream_t st, Bufs B, const StoreView &v, mcx_col_rank_summary *out, const RankDebug *dbg, double *ms)
{
  if (v.N >= ((int64_t)1 << 31))
    return fail(MCX_ERR_UNSUPPORTED, "rank summary: %lld values per column, fewer than 2^31 are supported", (long long)v.N);
  const int ncol = v.ncol;
  RankPass p(st, B, v, ms, dbg && dbg->ranks);
  std::vector<mcx_col_summary> cs(ncol);
  MCXCHK(p.tm.run(RT_TOTAL, [&]() -> int {
    MCXCHK(thresholds(p));
    MCXCHK(rank_scratch(p));
    if (dbg) return rank_debug_copy_out(p, *dbg);
    for (int c = 0; c < ncol; ++c) {
      out[c].flags = p.c0s[c].flags;
      out[c].q05 = p.thr[c];
      out[c].median = p.thr[(size_t)ncol + c];
      out[c].q95 = p.thr[2 * (size_t)ncol + c];
    }
    MCXCHK(normal_scores(p, RANK_BULK));
    MCXCHK(mixing(p, RANK_BULK * RT_PER + RT_SUMMARY, cs));
    for (int c = 0; c < ncol; ++c) {
      out[c].rhat_bulk = cs[c].rhat;
      out[c].ess_bulk = cs[c].ess;
      out[c].ess_bulk_lag = cs[c].ess_lag;
    }
    MCXCHK(normal_scores(p, RANK_FOLD));
    MCXCHK(mixing(p, RANK_FOLD * RT_PER + RT_SUMMARY, cs));
    for (int c = 0; c < ncol; ++c) out[c].rhat_folded = cs[c].rhat;
    MCXCHK(transform(p, RANK_I05, 0, ncol, RT_I05));
    MCXCHK(mixing(p, RT_I05_SUMMARY, cs));
    for (int c = 0; c < ncol; ++c) out[c].ess_q05 = cs[c].ess;
    MCXCHK(transform(p, RANK_I95, 0, ncol, RT_I95));
    MCXCHK(mixing(p, RT_I95_SUMMARY, cs));
    for (int c = 0; c < ncol; ++c) out[c].ess_q95 = cs[c].ess;
    assemble(out, ncol);
    return MCX_OK;
  }));
  return p.tm.collect();
}

int rank_args(int nsteps, const void *cols)
{
  if (!cols) return fail(MCX_ERR_INVALID, "cols is NULL");
  return half_chain_args(nsteps);
}

}  // namespace

RankGeometry rank_geometry(int64_t T, int64_t N)
{
  RankGeometry g;
  g.rchunk = std::max(RCHUNK, (T + 32767) / 32768);
  g.chunks = (unsigned)((T + g.rchunk - 1) / g.rchunk);
  g.nblk = (uint32_t)((N + RTILE - 1) / RTILE);
  return g;
}

int rank_span(hipStream_t st, Bufs B, const StoreSpan &s, mcx_col_rank_summary *cols)
{
  MCXCHK(rank_args((int)s.T, cols));
  return rank_device(st, B, StoreView(s), cols, nullptr, nullptr);
}

extern "C" int mcx_samples_rank_summary(mcx_engine *e, int first_step, int nsteps, mcx_col_rank_summary *cols)
{
  return on_store(
      e, first_step, nsteps, [&] { return rank_args(nsteps, cols); },
      [&](hipStream_t st, Bufs B, const StoreView &v) { return rank_device(st, B, v, cols, nullptr, nullptr); });
}

extern "C" int mcx_rows_rank_summary(const float *rows, int nsteps, int nc, int np, mcx_col_rank_summary *cols)
{
  MCXCHK(rank_args(nsteps, cols));
  return on_rows(rows, nsteps, nc, np,
                 [&](hipStream_t st, Bufs B, const StoreView &v) { return rank_device(st, B, v, cols, nullptr, nullptr); });
}

extern "C" int mcx_debug_rows_rank_transform(const float *rows, int nsteps, int nc, int np, int what, double *ranks,
                                             float *out_rows)
{
  MCXCHK(rank_args(nsteps, out_rows));
  if (what < RANK_BULK || what > RANK_I95) return fail(MCX_ERR_INVALID, "what = %d: 0 z(x), 1 z(f), 2 I05, 3 I95", what);
  if (ranks && what > RANK_FOLD) return fail(MCX_ERR_INVALID, "ranks only exist for what = 0 and 1");
  const RankDebug dbg{what, ranks, out_rows};
  return on_rows(rows, nsteps, nc, np,
                 [&](hipStream_t st, Bufs B, const StoreView &v) { return rank_device(st, B, v, nullptr, &dbg, nullptr); });
}

extern "C" int mcx_debug_rank_summary_times(mcx_engine *e, int first_step, int nsteps, double *ms)
{
  return on_store(
      e, first_step, nsteps,
      [&] {
        if (!ms) return fail(MCX_ERR_INVALID, "ms is NULL");
        return half_chain_args(nsteps);
      },
      [&](hipStream_t st, Bufs B, const StoreView &v) {
        std::vector<mcx_col_rank_summary> cols(v.ncol);
        return rank_device(st, B, v, cols.data(), nullptr, ms);
      });
}

extern "C" int mcx_debug_normal_quantile(const double *p, int n, double *z)
{
  if (n < 0 || (n > 0 && (!p || !z))) return fail(MCX_ERR_INVALID, "bad arguments");
  for (int i = 0; i < n; ++i) z[i] = mcx_ppnd16(p[i]);
  return MCX_OK;
}
