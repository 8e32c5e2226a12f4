// mcx_density.hip -- mcx_samples_density / mcx_rows_density / density_span: per column of a step range of the sample store,
// the binned Gaussian kernel density estimate of R's density.default (what geom_density draws in the reference's
// mcparam.density, src/anly/mcpar-analysis.R:22-28).  DESIGN.md section 13 restates every definition.
//
// One call:
//   1. summary_spread (mcx_summary.hip)  the passes of the summary that a density needs: column sums, exact order statistics
//                                        (min, max, the quartiles, the clip pair), the centred sum of squares
//   2. mcx_debug_density_grid            host, per column: bw.nrd0, from / to, the grid [lo, up] of 512 points
//   3. k_density_bins                    the one new sweep: every value of every column into the fixed-point linear binning
//                                        of its column's grid; integer adds only, so the bytes do not depend on scheduling
//   4. mcx_debug_density_finish          host, per column: the grid masses, the 1024-point convolution with the Gaussian
//                                        ordinates in fp64, the interpolation to the n output points
#include "mcx_summary_kernels.hpp"

#include <chrono>
#include <limits>

namespace {

constexpr int NG = 512;          // grid points per column
constexpr int NSLOT = NG + 1;    // slot s = ix + 1 for ix = -1 .. NG - 1
constexpr int DCT = 8;           // columns per tile: DCT * NSLOT * 8 B = 32.8 KB of LDS
// Values of one column that a workgroup bins between its zeroing and its flush.  An LDS slot is one u64 that holds both
// accumulators: a value adds (1 << 41) + w, w = floor(fx * 2^24) <= 2^24 (fx = xpos - floor(xpos) is below 1 except where
// that subtraction rounds to 1.0, for xpos = -tiny).  With at most 2^16 values the sum of the w is at most 2^40 < 2^41, so
// it never reaches the count, and the count is at most 2^16 < 2^23, so it never leaves the word.
constexpr int64_t DVALS = 1 << 16;
constexpr int CNT_SHIFT = 41;
constexpr int DUNROLL = 8;       // steps whose loads are issued before the first of them is binned
static_assert(DVALS * ((1ll << 24) + 0) < (1ll << CNT_SHIFT), "the fraction sums of a chunk stay below the count");
static_assert(DVALS < (1ll << (64 - CNT_SHIFT)), "the counts of a chunk stay inside the word");

__device__ __forceinline__ void bin_value(unsigned long long *slots, float v, double lo, double inv)
{
  const double xpos = ((double)v - lo) * inv;  // (-ffp-contract=off: a subtraction and a multiplication)
  if (xpos >= -1.0 && xpos < (double)NG) {     // ix in [-1, NG - 1]; a NaN fails both
    const double fl = floor(xpos);
    const unsigned long long w = (unsigned long long)((xpos - fl) * 16777216.0);
    atomicAdd(&slots[(int)fl + 1], (1ull << CNT_SHIFT) + w);
  }
}

// grid = (nbc * ntiles, step chunks).  grid2[col] = (lo, inv); slots[col][NSLOT][2] = (cnt, frac)
__global__ void __launch_bounds__(SB) k_density_bins(TileSet t, int nc, int64_t T, int64_t chunk, const double *grid2,
                                                     unsigned long long *slots)
{
  __shared__ unsigned long long acc[DCT * NSLOT];
  const int tile = blockIdx.x % t.ntiles, bc = blockIdx.x / t.ntiles;
  for (int i = threadIdx.x; i < t.ct * NSLOT; i += SB) acc[i] = 0ull;
  __syncthreads();
  const Lane l = lane_of(t, tile, bc, nc);
  if (l.ok) {
    const int col = t.col0 + l.lcol;
    const double lo = grid2[2 * col], inv = grid2[2 * col + 1];
    unsigned long long *mc = acc + l.j * NSLOT;
    const float *p = t.src + (size_t)l.chain * t.cs + l.lcol;
    const int64_t s0 = (int64_t)blockIdx.y * chunk, s1 = min(T, s0 + chunk);
    int64_t s = s0;
    for (; s + DUNROLL <= s1; s += DUNROLL) {
      float v[DUNROLL];
#pragma unroll
      for (int u = 0; u < DUNROLL; ++u) v[u] = p[(s + u) * t.rs];
#pragma unroll
      for (int u = 0; u < DUNROLL; ++u) bin_value(mc, v[u], lo, inv);
    }
    for (; s < s1; ++s) bin_value(mc, p[s * t.rs], lo, inv);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < t.ct * NSLOT; i += SB) {
    const unsigned long long a = acc[i];
    if (!a) continue;
    const int j = i / NSLOT, sl = i - j * NSLOT, lc = tile * t.ct + j;
    if (lc >= t.ncs) continue;
    unsigned long long *g = slots + ((size_t)(t.col0 + lc) * NSLOT + sl) * 2;
    atomicAdd(g, a >> CNT_SHIFT);
    const unsigned long long fr = a & ((1ull << CNT_SHIFT) - 1);
    if (fr) atomicAdd(g + 1, fr);
  }
}

// a tile set of at most DCT columns per tile (the LDS accumulators), and the steps per workgroup that keep a column's
// values per workgroup within DVALS
TileSet density_tiles(TileSet t, int nc)
{
  t.ct = std::min(t.ct, DCT);
  t.cg = SB / t.ct; t.ntiles = (t.ncs + t.ct - 1) / t.ct; t.nbc = (nc + t.cg - 1) / t.cg;
  return t;
}

// the sweep over both tile sets: grid2 [ncol][2] and slots [ncol][NSLOT][2] on the device, slots zeroed by the caller
int launch_bins(hipStream_t st, const StoreView &v, const double *grid2, unsigned long long *slots)
{
  for (const TileSet *t0 : {&v.tx, &v.tl}) {
    const TileSet t = density_tiles(*t0, v.nc);
    const int64_t chunk = DVALS / t.cg;
    const unsigned chunks = (unsigned)((v.T + chunk - 1) / chunk);
    hipLaunchKernelGGL(k_density_bins, dim3((unsigned)(t.nbc * t.ntiles), chunks), dim3(SB), 0, st, t, v.nc, v.T, chunk, grid2, slots);
    HIPCHK(hipGetLastError());
  }
  return MCX_OK;
}

// upload the columns' (lo, inv), zero the slots, sweep, bring the slots home.  tm: the sweep alone is stage 1
int bins_device(hipStream_t st, Bufs B, const StoreView &v, const std::vector<double> &grid2, std::vector<unsigned long long> &slots,
                StageTimer &tm)
{
  const size_t ns = (size_t)v.ncol * NSLOT * 2;
  MCXCHK(B.d->alloc(grid2.size()));
  MCXCHK(B.h->alloc(ns));
  HIPCHK(hipMemcpyAsync(B.d->p, grid2.data(), grid2.size() * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(B.h->p, 0, ns * sizeof(unsigned long long), st));
  MCXCHK(tm.run(1, [&]() -> int { return launch_bins(st, v, B.d->p, B.h->p); }));
  slots.resize(ns);
  HIPCHK(hipMemcpyAsync(slots.data(), B.h->p, ns * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));  // (grid2 is read by the upload until here)
  return MCX_OK;
}

inline bool given(const double *a, int c) { return a && !std::isnan(a[c]); }
inline bool clipped(const mcx_density_spec *s) { return !(s->clip_lo == 0.0 && s->clip_hi == 1.0); }

// what can be refused before a device is touched
int density_args(const mcx_density_spec *s, int ncol, int64_t N, const mcx_col_density *cols, const double *x, const double *y)
{
  if (!s) return fail(MCX_ERR_INVALID, "the density spec is NULL");
  if (!cols || !x || !y) return fail(MCX_ERR_INVALID, "cols, x or y is NULL");
  if (s->n < 2 || s->n > NG) return fail(MCX_ERR_INVALID, "n = %d: 2 to %d output points", s->n, NG);
  if (!(s->adjust > 0.0) || !std::isfinite(s->adjust)) return fail(MCX_ERR_INVALID, "adjust = %g is not a positive finite number", s->adjust);
  if (clipped(s) && !(s->clip_lo >= 0.0 && s->clip_lo < s->clip_hi && s->clip_hi <= 1.0))
    return fail(MCX_ERR_INVALID, "clip = (%g, %g): 0 <= clip_lo < clip_hi <= 1", s->clip_lo, s->clip_hi);
  for (int c = 0; c < ncol; ++c) {
    if (given(s->bw, c) && !(s->bw[c] > 0.0 && std::isfinite(s->bw[c])))
      return fail(MCX_ERR_INVALID, "bw[%d] = %g is not a positive finite number", c, s->bw[c]);
    if ((given(s->from, c) && !std::isfinite(s->from[c])) || (given(s->to, c) && !std::isfinite(s->to[c])))
      return fail(MCX_ERR_INVALID, "from[%d] or to[%d] is infinite", c, c);
    if (given(s->from, c) && given(s->to, c) && s->from[c] > s->to[c])
      return fail(MCX_ERR_INVALID, "from[%d] = %g is above to[%d] = %g", c, s->from[c], c, s->to[c]);
  }
  if (N < 2) return fail(MCX_ERR_INVALID, "a density needs nsteps * nc >= 2 values per column, got %lld", (long long)N);
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

// ms (mcx_debug_density_times, else NULL): ms[0] the statistics passes (wall clock), ms[1] k_density_bins (HIP events),
// ms[2] the host grid and finish (wall clock), ms[3] the whole call (wall clock)
int density_device(hipStream_t st, Bufs B, const StoreView &v, const mcx_density_spec *spec, mcx_col_density *cols, double *x,
                   double *y, double *ms)
{
  using clk = std::chrono::steady_clock;
  auto since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
  const clk::time_point t_call = clk::now();
  StageTimer tm{st, ms, 4, {}};
  const int ncol = v.ncol, n = spec->n;
  const bool clip = clipped(spec);
  const double probs[4] = {0.25, 0.75, spec->clip_lo, spec->clip_hi};
  const int nprobs = clip ? 4 : 2;
  const double qnan = std::numeric_limits<double>::quiet_NaN();

  // ---- 1. moments and order statistics
  std::vector<mcx_col_summary> sc(ncol);
  std::vector<double> q((size_t)ncol * nprobs);
  MCXCHK(summary_spread(st, B, v, probs, nprobs, sc.data(), q.data()));
  const double ms_stats = since(t_call);

  // ---- 2. the grids
  clk::time_point t_host = clk::now();
  std::vector<double> grid2((size_t)ncol * 2, qnan);  // a column that is not finite is swept with NaN: it bins nothing
  for (int c = 0; c < ncol; ++c) {
    if (sc[c].flags & MCX_SUMMARY_NONFINITE) {
      nan_column(&cols[c], v.N);
      continue;
    }
    const double *qc = q.data() + (size_t)c * nprobs;
    MCXCHK(mcx_debug_density_grid(v.N, sc[c].mean, sc[c].sd, sc[c].min, sc[c].max, qc[0], qc[1], clip ? qc[2] : qnan, clip ? qc[3] : qnan,
                                  c == ncol - 1, c, spec, &cols[c]));
    grid2[2 * c] = cols[c].lo;
    grid2[2 * c + 1] = (double)(NG - 1) / (cols[c].up - cols[c].lo);
  }
  double ms_host = since(t_host);

  // ---- 3. the sweep
  std::vector<unsigned long long> slots;
  MCXCHK(bins_device(st, B, v, grid2, slots, tm));

  // ---- 4. the finish
  t_host = clk::now();
  for (int c = 0; c < ncol; ++c) {
    double *xc = x + (size_t)c * n, *yc = y + (size_t)c * n;
    if (cols[c].flags & MCX_SUMMARY_NONFINITE) {
      std::fill(xc, xc + n, qnan);
      std::fill(yc, yc + n, qnan);
      continue;
    }
    const unsigned long long *sl = slots.data() + (size_t)c * NSLOT * 2;
    long long nb = 0;
    for (int s = 1; s < NSLOT; ++s) nb += (long long)sl[2 * s];
    cols[c].nbinned = nb;
    MCXCHK(mcx_debug_density_finish(&cols[c], sl, n, xc, yc));
  }
  ms_host += since(t_host);
  MCXCHK(tm.collect());
  if (ms) {
    ms[0] = ms_stats;
    ms[2] = ms_host;
    ms[3] = since(t_call);
  }
  return MCX_OK;
}

}  // namespace

int density_spec_args(const mcx_density_spec *spec, int ncol, int64_t N, const mcx_col_density *cols, const double *x, const double *y)
{
  return density_args(spec, ncol, N, cols, x, y);
}

int density_span(hipStream_t st, Bufs B, const StoreSpan &s, const mcx_density_spec *spec, mcx_col_density *cols, double *x, double *y,
                 double *ms)
{
  MCXCHK(density_args(spec, s.np + 1, s.T * (int64_t)s.nc, cols, x, y));
  return density_device(st, B, StoreView(s), spec, cols, x, y, ms);
}

extern "C" int mcx_samples_density(mcx_engine *e, int first_step, int nsteps, const mcx_density_spec *spec, mcx_col_density *cols,
                                   double *x, double *y)
{
  return on_store(
      e, first_step, nsteps, [&] { return density_args(spec, e->nparam + 1, (int64_t)nsteps * e->nchain, cols, x, y); },
      [&](hipStream_t st, Bufs B, const StoreView &v) { return density_device(st, B, v, spec, cols, x, y, nullptr); });
}

// mcx_samples_density with its stages timed, for tools/density_bench.py; the results are let go
extern "C" int mcx_debug_density_times(mcx_engine *e, int first_step, int nsteps, const mcx_density_spec *spec, double *ms)
{
  std::vector<mcx_col_density> cols;
  std::vector<double> x, y;
  return on_store(
      e, first_step, nsteps,
      [&] {
        if (!ms) return fail(MCX_ERR_INVALID, "ms is NULL");
        if (!spec) return fail(MCX_ERR_INVALID, "the density spec is NULL");
        const size_t ncol = (size_t)e->nparam + 1, n = (size_t)std::max(spec->n, 1);
        cols.resize(ncol);
        x.resize(ncol * n);
        y.resize(ncol * n);
        return density_args(spec, (int)ncol, (int64_t)nsteps * e->nchain, cols.data(), x.data(), y.data());
      },
      [&](hipStream_t st, Bufs B, const StoreView &v) { return density_device(st, B, v, spec, cols.data(), x.data(), y.data(), ms); });
}

extern "C" int mcx_rows_density(const float *rows, int nsteps, int nc, int np, const mcx_density_spec *spec, mcx_col_density *cols,
                                double *x, double *y)
{
  if (!rows || nc < 1 || np < 1 || np > 256) return fail(MCX_ERR_INVALID, "bad arguments");
  MCXCHK(density_args(spec, np + 1, (int64_t)nsteps * nc, cols, x, y));
  return on_rows(rows, nsteps, nc, np, [&](hipStream_t st, Bufs B, const StoreView &v) {
    return density_device(st, B, v, spec, cols, x, y, nullptr);
  });
}

// the sweep alone on given grids
extern "C" int mcx_debug_rows_density_bins(const float *rows, int nsteps, int nc, int np, const double *lo, const double *up,
                                           unsigned long long *slots)
{
  if (!rows || nc < 1 || np < 1 || np > 256 || nsteps < 1 || !lo || !up || !slots) return fail(MCX_ERR_INVALID, "bad arguments");
  std::vector<double> grid2(((size_t)np + 1) * 2);
  for (int c = 0; c <= np; ++c) {
    if (!(lo[c] < up[c])) return fail(MCX_ERR_INVALID, "lo[%d] = %g is not below up[%d] = %g", c, lo[c], c, up[c]);
    grid2[2 * c] = lo[c];
    grid2[2 * c + 1] = (double)(NG - 1) / (up[c] - lo[c]);
  }
  return on_rows(rows, nsteps, nc, np, [&](hipStream_t st, Bufs B, const StoreView &v) -> int {
    StageTimer tm{st, nullptr, 0, {}};
    std::vector<unsigned long long> out;
    MCXCHK(bins_device(st, B, v, grid2, out, tm));
    std::copy(out.begin(), out.end(), slots);
    return MCX_OK;
  });
}

// ---------------------------------------------------------------------------------------------------------------------
// the host steps (no device calls): DESIGN.md section 13 restates every line
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int mcx_debug_density_grid(long long N, double mean, double sd, float min, float max, double q25, double q75,
                                      double qclip_lo, double qclip_hi, int is_last_col, int col, const mcx_density_spec *spec,
                                      mcx_col_density *out)
{
  if (!spec || !out || N < 2 || col < 0) return fail(MCX_ERR_INVALID, "bad arguments");
  if (!(spec->adjust > 0.0) || !std::isfinite(spec->adjust)) return fail(MCX_ERR_INVALID, "adjust = %g is not a positive finite number", spec->adjust);
  const bool clip = clipped(spec);
  if (clip && !(spec->clip_lo >= 0.0 && spec->clip_lo < spec->clip_hi && spec->clip_hi <= 1.0))
    return fail(MCX_ERR_INVALID, "clip = (%g, %g): 0 <= clip_lo < clip_hi <= 1", spec->clip_lo, spec->clip_hi);
  if (!std::isfinite(mean) || !std::isfinite(sd) || !std::isfinite(min) || !std::isfinite(max) || !std::isfinite(q25) || !std::isfinite(q75) ||
      (clip && (!std::isfinite(qclip_lo) || !std::isfinite(qclip_hi)))) {
    nan_column(out, N);
    return MCX_OK;
  }
  // bw.nrd0
  double bw;
  if (given(spec->bw, col)) {
    bw = spec->bw[col];
    if (!(bw > 0.0 && std::isfinite(bw))) return fail(MCX_ERR_INVALID, "bw[%d] = %g is not a positive finite number", col, bw);
  } else {
    const double hi = sd;
    double lo_ = std::min(hi, (q75 - q25) / 1.34);
    if (lo_ == 0.0) lo_ = hi;
    if (lo_ == 0.0) lo_ = std::fabs((double)min);
    if (lo_ == 0.0) lo_ = 1.0;
    bw = spec->adjust * 0.9 * lo_ * std::pow((double)N, -0.2);
  }
  double from = min, to = max;
  if (clip) {
    from = qclip_lo;
    if (!is_last_col) to = qclip_hi;  // log L keeps its upper end (mcparam.clip.tails)
  }
  if (given(spec->from, col)) from = spec->from[col];
  if (given(spec->to, col)) to = spec->to[col];
  if (!std::isfinite(from) || !std::isfinite(to) || !(from <= to))
    return fail(MCX_ERR_INVALID, "column %d: from = %g and to = %g are not a finite range", col, from, to);
  out->bw = bw; out->from = from; out->to = to;
  out->lo = from - 4.0 * bw;
  out->up = to + 4.0 * bw;
  out->mean = mean; out->sd = sd;
  out->nvalues = N; out->nbinned = 0; out->flags = 0;
  if (!(out->lo < out->up) || !std::isfinite(out->up - out->lo))
    return fail(MCX_ERR_INVALID, "column %d: the grid [%g, %g] is not a finite interval", col, out->lo, out->up);
  return MCX_OK;
}

extern "C" int mcx_debug_density_finish(const mcx_col_density *col, const unsigned long long *slots, int n, double *x, double *y)
{
  if (!col || !slots || !x || !y || n < 2 || n > NG || col->nvalues < 2 || !(col->bw > 0.0) || !(col->lo < col->up) || !(col->from <= col->to))
    return fail(MCX_ERR_INVALID, "bad arguments");
  const double N = (double)col->nvalues, bw = col->bw, lo = col->lo, up = col->up;
  const double delta = (up - lo) / (double)(NG - 1), two24 = 16777216.0;
  // grid masses
  std::vector<double> mass(NG), K(2 * NG), d(NG), xg(NG);
  for (int k = 0; k < NG; ++k)
    mass[k] = (((double)slots[2 * (k + 1)] - (double)slots[2 * (k + 1) + 1] / two24) + (double)slots[2 * k + 1] / two24) / N;
  // kernel ordinates on the grid's own spacing, wrapped
  const double norm = bw * std::sqrt(2.0 * M_PI);
  for (int m = 0; m < 2 * NG; ++m) {
    const double km = m <= NG ? (double)m * delta : -(double)(2 * NG - m) * delta;
    const double z = km / bw;
    K[m] = std::exp(-0.5 * (z * z)) / norm;
  }
  // the circular convolution; the masses of m >= NG are zero
  for (int j = 0; j < NG; ++j) {
    double s = 0.0;
    for (int m = 0; m < NG; ++m) s += mass[m] * K[(m - j) & (2 * NG - 1)];
    d[j] = std::max(0.0, s);
    xg[j] = lo + (double)j * delta;
  }
  // R's approx at the output points
  const double step = (col->to - col->from) / (double)(n - 1);
  for (int j = 0; j < n; ++j) {
    const double xv = j == n - 1 ? col->to : col->from + (double)j * step;
    int i = (int)(std::upper_bound(xg.begin(), xg.end(), xv) - xg.begin()) - 1;
    i = std::min(std::max(i, 0), NG - 2);
    x[j] = xv;
    y[j] = d[i] + (d[i + 1] - d[i]) * ((xv - xg[i]) / (xg[i + 1] - xg[i]));
  }
  return MCX_OK;
}
