// mcx_summary_kernels.hpp -- what mcx_summary.hip, mcx_covariance.hip and mcx_ranks.hip share: the column tiles of the sample
// store and the one view of a store made of them (StoreView), the two ways to a view (on_store: a step range of an engine's
// store; on_rows: host rows uploaded to a scratch store; mcx_derive.hip comes through both to read a span, and its derived
// store is a third way: a span handed to summary_span / rank_span / covariance_span below), pass 1 of every analysis (k_sum_moments: per-series fp64 sums), the
// fixed-order reducer k_sum_rows that every cross-chain or cross-workgroup sum goes through, and the stage timer of the
// mcx_debug_*_times entry points.  Internal to the three analysis units (each gets its own copy of the kernels).
// mcx_derive.hip, mcx_density.hip (section 13, which has its own sweep and gets its statistics from summary_spread below) and
// mcx_clip.hip (section 14: its thresholds are summary_thresholds')
// include it for the view plumbing alone (on_store, on_rows with its k_sum_deinterleave, StageTimer); the
// other kernels' copies in those units are never launched;
// nothing here is part of the library's interface.
#pragma once
#include "mcx_engine_internal.hpp"

// What crosses between the three units is plain: the scratch buffers of a call and a step range of a store on the device.
// (TileSet is a type of each unit's own -- its kernels take it by value -- and so is the StoreView that holds two of them.)
struct Bufs {
  DevBuf<double> *d;
  DevBuf<unsigned long long> *h;
  DevBuf<uint32_t> *u;
};
struct StoreSpan {
  const float *x, *ly;  // x[T][nc][np], ly[T][nc]
  int nc, np;
  int64_t T;
};

// mcx_summary.hip's passes for mcx_ranks.hip, each a subset of mcx_samples_summary's:
// summary_thresholds: moments, order statistics, finish -- rhat, ess, ess_lag and mcse_mean of cols are not valid (any range
// of N >= 1 values: mcx_clip.hip, section 14, asks for fewer than four steps);
// summary_mixing: moments, autocovariance windows, finish -- min and max of cols are not valid
MCXI int summary_thresholds(hipStream_t st, Bufs B, const StoreSpan &s, const double *probs, int nprobs, mcx_col_summary *cols,
                            double *quantiles);
MCXI int summary_mixing(hipStream_t st, Bufs B, const StoreSpan &s, mcx_col_summary *cols);
// and for mcx_density.hip (section 13): moments, order statistics, window 0 of the autocovariance for the centred sum of
// squares, the finish without lags -- mean, sd, min, max, flags and the quantiles are mcx_samples_summary's bits; rhat, ess,
// ess_lag and mcse_mean of cols are not valid.  Any range of N >= 2 values (the summary's nsteps >= 4 is not asked)
MCXI int summary_spread(hipStream_t st, Bufs B, const StoreSpan &s, const double *probs, int nprobs, mcx_col_summary *cols,
                        double *quantiles);

// The three analyses on any span, for the third way to a view (mcx_derive.hip: a derived store): each checks its own
// arguments as its mcx_samples_* entry point does, then runs the passes of that entry point on a StoreView of the span
MCXI int summary_span(hipStream_t st, Bufs B, const StoreSpan &s, const double *probs, int nprobs, mcx_col_summary *cols,
                      double *quantiles);                                                          // mcx_summary.hip
MCXI int rank_span(hipStream_t st, Bufs B, const StoreSpan &s, mcx_col_rank_summary *cols);        // mcx_ranks.hip
MCXI int covariance_span(hipStream_t st, Bufs B, const StoreSpan &s, double *mean, double *cov, int *flags);  // mcx_covariance.hip
MCXI int density_span(hipStream_t st, Bufs B, const StoreSpan &s, const mcx_density_spec *spec, mcx_col_density *cols, double *x,
                      double *y, double *ms = nullptr);  // mcx_density.hip; ms: mcx_debug_density_times' four stages
MCXI int density2d_span(hipStream_t st, Bufs B, const StoreSpan &s, const mcx_density2d_spec *spec, mcx_col_density *cols,
                        double *axes, mcx_pair_density *pairs_out, double *z);  // mcx_density2d.hip (section 15)
// what mcx_density.hip refuses before a device is touched, for mcx_density2d.hip, whose spec shares those fields
MCXI int density_spec_args(const mcx_density_spec *spec, int ncol, int64_t N, const mcx_col_density *cols, const double *x,
                           const double *y);

// The launch geometry of a rank pass over T steps and N = T * nc values per column (mcx_ranks.hip): what RankPass launches
// with and what mcx_debug_store_geometry reports
struct RankGeometry {
  int64_t rchunk;   // steps per workgroup of the key and transform sweeps
  unsigned chunks;  // their grid.y
  uint32_t nblk;    // sort tiles per column
};
MCXI RankGeometry rank_geometry(int64_t T, int64_t N);

namespace {

constexpr int SB = 256;     // threads per workgroup of every summary kernel
constexpr int CTX = 16;     // columns per parameter tile

// where a tile set lives: x (ncs = np columns, chain stride np) or ly (ncs = 1, chain stride 1)
struct TileSet {
  const float *src;  // step 0 of the range
  size_t rs;         // floats per step
  int cs;            // floats per chain
  int ncs;           // columns in this array
  int col0;          // global column of its first column
  int ct, cg, ntiles, nbc;
};

struct Lane {
  int chain, lcol, j;
  bool ok;
};
__device__ __forceinline__ Lane lane_of(const TileSet &t, int tile, int bc, int nc)
{
  Lane l;
  const int k = threadIdx.x / t.ct;
  l.j = threadIdx.x - k * t.ct;
  l.chain = bc * t.cg + k;
  l.lcol = tile * t.ct + l.j;
  l.ok = k < t.cg && l.chain < nc && l.lcol < t.ncs;
  return l;
}

// pass 1: half-chain means and series sums.  grid = nbc * ntiles
__global__ void __launch_bounds__(SB) k_sum_moments(TileSet t, int nc, int64_t T, int64_t n, double *hm, double *tot)
{
  const int tile = blockIdx.x % t.ntiles, bc = blockIdx.x / t.ntiles;
  const Lane l = lane_of(t, tile, bc, nc);
  if (!l.ok) return;
  const float *p = t.src + (size_t)l.chain * t.cs + l.lcol;
  double s0 = 0.0, s1 = 0.0, sm = 0.0;
#pragma unroll 8
  for (int64_t s = 0; s < n; ++s) s0 += (double)p[s * t.rs];
#pragma unroll 8
  for (int64_t s = T - n; s < T; ++s) s1 += (double)p[s * t.rs];
  if (T - 2 * n == 1) sm = (double)p[n * t.rs];
  const int col = t.col0 + l.lcol;
  hm[((size_t)col * 2 + 0) * nc + l.chain] = s0 / (double)n;
  hm[((size_t)col * 2 + 1) * nc + l.chain] = s1 / (double)n;
  tot[(size_t)col * nc + l.chain] = (s0 + sm) + s1;
}

// out[r] = sum over l < len of in[r * stride + l], or of (in - center[col] * cscale)^2; len = lenx for a parameter column,
// lenl for log L (col = (r / qper) % ncol).  One workgroup per row, fixed order: per-thread strided sums, then a tree.
__global__ void __launch_bounds__(SB) k_sum_rows(const double *in, size_t stride, int qper, int ncol, int np, size_t lenx,
                                                 size_t lenl, const double *center, double cscale, double *out)
{
  __shared__ double red[SB];
  const size_t r = blockIdx.x;
  const int col = (int)((r / qper) % ncol);
  const size_t len = col < np ? lenx : lenl;
  const double c = center ? center[col] * cscale : 0.0;
  const double *p = in + r * stride;
  double s = 0.0;
  for (size_t i = threadIdx.x; i < len; i += SB) {
    const double v = p[i];
    s += center ? (v - c) * (v - c) : v;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = SB / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[r] = red[0];
}

__global__ void k_sum_deinterleave(const float *rows, size_t nrows, int np, float *x, float *ly)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t ncol = (size_t)np + 1;
  if (i >= nrows * ncol) return;
  const size_t r = i / ncol;
  const int c = (int)(i - r * ncol);
  if (c < np) x[r * np + c] = rows[i];
  else ly[r] = rows[i];
}

inline TileSet tiles_x(const float *x, int nc, int np)
{
  TileSet t;
  t.src = x; t.rs = (size_t)nc * np; t.cs = np; t.ncs = np; t.col0 = 0;
  t.ct = std::min(np, CTX); t.cg = SB / t.ct; t.ntiles = (np + t.ct - 1) / t.ct; t.nbc = (nc + t.cg - 1) / t.cg;
  return t;
}
inline TileSet tiles_l(const float *ly, int nc, int np)
{
  TileSet t;
  t.src = ly; t.rs = (size_t)nc; t.cs = 1; t.ncs = 1; t.col0 = np;
  t.ct = 1; t.cg = SB; t.ntiles = 1; t.nbc = (nc + SB - 1) / SB;
  return t;
}

// The grouping of a row sweep (mcx_chains.hip's k_chain_rows, mcx_steptable.hip's k_step_rows): G = 1 << lg lanes per chain,
// G = min(64, the power of two >= np + 1), lane j holding columns j, j + G, ... in V = ceil((np + 1) / G) <= 5 values; cpw chains
// per workgroup and nwg = ceil(nc / cpw) workgroups when each takes its chains once
struct RowsGeometry {
  int lg, G, V, cpw;
  unsigned nwg;
};
inline RowsGeometry rows_geometry(int np, int nc)
{
  RowsGeometry g;
  g.lg = 0;
  while (g.lg < 6 && (1 << g.lg) < np + 1) ++g.lg;
  g.G = 1 << g.lg;
  g.V = (np + g.G) / g.G;  // ceil((np + 1) / G)
  g.cpw = SB >> g.lg;
  g.nwg = (unsigned)(((int64_t)nc + g.cpw - 1) / g.cpw);
  return g;
}

// a step range of a store with everything the passes derive from it, formed once
struct StoreView : StoreSpan {
  int ncol;         // np + 1 columns: the parameters, then log L
  int64_t N, n, M;  // values per column T * nc; steps per half-chain T / 2; half-chains 2 * nc
  TileSet tx, tl;
  explicit StoreView(const StoreSpan &s)
      : StoreSpan(s), ncol(s.np + 1), N(s.T * (int64_t)s.nc), n(s.T / 2), M(2 * (int64_t)s.nc), tx(tiles_x(s.x, s.nc, s.np)),
        tl(tiles_l(s.ly, s.nc, s.np))
  {
  }
};

// the text every analysis of half-chains refuses a short range with
inline int half_chain_args(int nsteps)
{
  if (nsteps < 4) return fail(MCX_ERR_INVALID, "a summary needs nsteps >= 4 (two half-chains of >= 2 steps), got %d", nsteps);
  return MCX_OK;
}

// Steps [first_step, first_step + nsteps) of an engine's store on the engine's stream, with its summ_* buffers:
// f(st, bufs, view) runs the device passes there.  Every engine entry point of the three units comes through here, so
// their checks have one order: 1. engine NULL, 2. the call's own arguments (args(), which may read *e), 3. enter,
// 4. store empty, 5. range
template <class A, class F> int on_store(mcx_engine *e, int first_step, int nsteps, A args, F f)
{
  if (!e) return fail(MCX_ERR_INVALID, "engine is NULL");
  MCXCHK(args());
  MCXCHK(enter(e));
  if (e->samp_steps == 0)
    return fail(MCX_ERR_INVALID, "the sample store is empty (no run yet, MCX_OPT_SAMPLES = 0, or a run into a sink)");
  if (first_step < 0 || (int64_t)first_step + nsteps > e->samp_steps)
    return fail(MCX_ERR_INVALID, "steps [%d,%lld) not in the sample store (%d steps)", first_step,
                (long long)first_step + nsteps, e->samp_steps);
  const size_t nc = (size_t)e->nchain, np = (size_t)e->nparam;
  return f(e->stream, Bufs{&e->summ_d, &e->summ_h, &e->summ_u},
           StoreView(StoreSpan{e->samp_x.p + (size_t)first_step * nc * np, e->samp_ly.p + (size_t)first_step * nc, (int)nc, (int)np,
                               nsteps}));
}

// rows [nsteps * nc][np + 1] on the host (MCout layout) uploaded to a scratch store x, ly on a stream of its own:
// f(st, bufs, view) runs the device passes there
template <class F> int on_rows(const float *rows, int nsteps, int nc, int np, F f)
{
  if (!rows || nc < 1 || np < 1 || np > 256) return fail(MCX_ERR_INVALID, "bad arguments");
  MCXCHK(need_device());
  const size_t nr = (size_t)nsteps * nc;
  DevBuf<float> rd, x, ly;
  DevBuf<double> d;
  DevBuf<unsigned long long> h;
  DevBuf<uint32_t> u;
  DevStream st;
  auto run = [&]() -> int {
    MCXCHK(st.ensure(hipStreamNonBlocking));
    MCXCHK(rd.alloc(nr * (np + 1)));
    MCXCHK(x.alloc(nr * np));
    MCXCHK(ly.alloc(nr));
    HIPCHK(hipMemcpyAsync(rd.p, rows, nr * (np + 1) * sizeof(float), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_sum_deinterleave, dim3(nblocks(nr * (np + 1))), dim3(BLOCK), 0, st, rd.p, nr, np, x.p, ly.p);
    HIPCHK(hipGetLastError());
    return f(st, Bufs{&d, &h, &u}, StoreView(StoreSpan{x.p, ly.p, nc, np, nsteps}));
  };
  const int rc = run();
  if (st) (void)hipStreamSynchronize(st);  // (before the buffers go)
  return rc;
}

// pass 1 of every analysis, in two launches' worth: sweep_moments is k_sum_moments over both tile sets -> hm[ncol][2][nc],
// tot[ncol][nc]; column_sums adds tot over the chains -> colsum[ncol].  (Two names because mcx_debug_covariance_times
// times the first alone.)
inline int sweep_moments(hipStream_t st, const StoreView &v, double *hm, double *tot)
{
  for (const TileSet *t : {&v.tx, &v.tl}) {
    hipLaunchKernelGGL(k_sum_moments, dim3((unsigned)(t->nbc * t->ntiles)), dim3(SB), 0, st, *t, v.nc, v.T, v.n, hm, tot);
    HIPCHK(hipGetLastError());
  }
  return MCX_OK;
}
inline int column_sums(hipStream_t st, const StoreView &v, const double *tot, double *colsum)
{
  hipLaunchKernelGGL(k_sum_rows, dim3((unsigned)v.ncol), dim3(SB), 0, st, tot, (size_t)v.nc, 1, v.ncol, v.np, (size_t)v.nc,
                     (size_t)v.nc, (const double *)nullptr, 0.0, colsum);
  HIPCHK(hipGetLastError());
  return MCX_OK;
}
inline int launch_moments(hipStream_t st, const StoreView &v, double *hm, double *tot, double *colsum)
{
  MCXCHK(sweep_moments(st, v, hm, tot));
  return column_sums(st, v, tot, colsum);
}

// HIP events around the stages of a call: ms[slot] += the time of every run(slot, f).  With ms == NULL no event is
// created or recorded and run() is f()
struct StageTimer {
  hipStream_t st;
  double *ms;
  int nslots;
  struct Ev { int idx; DevEvent a, b; };
  std::vector<Ev> evs;
  template <class F> int run(int idx, F f)
  {
    if (!ms) return f();
    Ev e{idx, {}, {}};
    MCXCHK(e.a.ensure(hipEventDefault));
    MCXCHK(e.b.ensure(hipEventDefault));
    const size_t k = evs.size();  // (f may run stages of its own: evs grows and moves under it)
    evs.push_back(std::move(e));
    HIPCHK(hipEventRecord(evs[k].a, st));
    MCXCHK(f());
    HIPCHK(hipEventRecord(evs[k].b, st));
    return MCX_OK;
  }
  int collect()
  {
    if (!ms) return MCX_OK;
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < nslots; ++i) ms[i] = 0.0;
    for (const Ev &e : evs) {
      float t = 0.0f;
      HIPCHK(hipEventElapsedTime(&t, e.a, e.b));
      ms[e.idx] += (double)t;
    }
    return MCX_OK;
  }
};

}  // namespace
