// mcx_lagcov.hip -- mcx_samples_lagcov / mcx_rows_lagcov / mcx_store_lagcov: the lagged covariance matrices G(t) of a step range
// of the sample store on the device, and from them (mcx_lagcov_host.hpp) the multivariate initial sequence estimator and the
// multivariate effective sample size.
//
// The store is step-major: row r is step r / nc of chain r % nc, so the lag-t partner of row r is row r + t nc, and it exists
// exactly when r + t nc < N.  G(t) = (1 / N) A^T B with A the centred rows and B the centred rows t nc further on.  Passes:
//   1. k_sum_moments + k_sum_rows   the column sums (mcx_summary_kernels.hpp: the bytes mcx_samples_summary's mean is made of)
//   2. k_lagcov<.., 1>              lag 0: the upper triangle of tile pairs, as mcx_covariance.hip's k_cov_tiles
//   3. k_lagcov<.., LW>             a window of LW consecutive lags per sweep: a workgroup takes every nwg-th unit of LROWS rows,
//                                   loads A once per row group and B once per lag, and keeps one accumulator (4 doubles a
//                                   lane) per lag.  All workgroups move through the store as one front, so the B rows of a
//                                   lag are the A rows of a unit that is read soon after: cache hits, not HBM reads.  grid =
//                                   (workgroups over rows, tile pairs): one launch for the nt pairs (t, t), which also carry the
//                                   log L products as side FMAs, one for the nt (nt - 1) ordered pairs ti != tj
//   4. k_sum_rows                   the workgroups' partials, [lag][row][workgroup] slabs, summed in a fixed order
// Windows are swept on demand: the host walk runs on the lags there are and asks for twice as many while it has not stopped.
// v_mfma_f64_16x16x4_f64 as in mcx_covariance.hip: a lane holds the centred x[row r0 + (lane >> 4)][column ci + (lane & 15)] as A
// and x[that row + t nc][column cj + (lane & 15)] as B; D[i][j] += sum over four rows of A[i] B[j] is G(t)[ci + i][cj + j].
// No float atomics; a workgroup's four wavefronts are added in wavefront order.
#include "mcx_store.hpp"

#include "mcx_lagcov_host.hpp"

#include <limits>

namespace {

namespace H = mcx_lagcov_host;

typedef double lag_f64x4 __attribute__((ext_vector_type(4)));

constexpr int LTILE = 16;                 // columns per tile: the matrix-core shape
constexpr int LGRP = 2;                   // row groups (of 4 rows) a wavefront loads before it multiplies them
constexpr int LWAVES = SB / 64;           // wavefronts per workgroup
constexpr int LROWS = LWAVES * LGRP * 4;  // rows of a unit: what a workgroup takes per iteration
constexpr size_t LWG_MAX = 512;           // workgroups of a launch at the most: two on each of 256 compute units are resident
constexpr size_t LWG_MIN = 32;            // and over the rows at the least, however many tile pairs share the launch
constexpr int LENT = LTILE * LTILE;       // entries of a tile pair
constexpr int LW = 8;                     // lags per window (the register budget)
// lag 0 on its own has registers to spare: k_cov_tiles' eight row groups and two accumulators
constexpr int lag_groups(int W) { return W == 1 ? 8 : LGRP; }
constexpr int lag_rows(int W) { return LWAVES * lag_groups(W) * 4; }

// a lag's slab: part[row][workgroup], rows: [tile][LTILE] parameter x log L | [tile][LTILE] log L x parameter | log L x log L |
// [pair][LENT]; pair = t for (t, t), nt + k for the k-th pair ti < tj in k_cov_tiles' order, nt + nu + k for its transpose
// (tj, ti), nu = nt (nt - 1) / 2.  Lag 0 has the first nt + nu pairs only.
struct LagGeometry {
  int nt, nu;
  size_t S, R, R0;   // side rows; rows of a slab; rows of lag 0's
  size_t units, cap, nwg;  // units of LROWS rows; workgroups over the rows at the most, LWG_MAX shared among the nt^2 pairs of a
                           // launch (so the slabs, nt^2 LENT rows each, stay bounded); workgroups, each taking units g, g + nwg,
                           // ...: a function of N and np alone
};
inline LagGeometry lag_geometry(size_t N, int np)
{
  LagGeometry g;
  g.nt = (np + LTILE - 1) / LTILE;
  g.nu = g.nt * (g.nt - 1) / 2;
  g.S = 2 * (size_t)g.nt * LTILE + 1;
  g.R = g.S + (size_t)g.nt * g.nt * LENT;
  g.R0 = g.S + (size_t)(g.nt + g.nu) * LENT;
  g.units = (N + LROWS - 1) / LROWS;
  g.cap = std::max(LWG_MIN, LWG_MAX / ((size_t)g.nt * g.nt));
  g.nwg = std::min(g.units, g.cap);
  return g;
}

// a sweep's units of lag_rows(W) rows and its workgroups over them: lg's when W = LW; fewer, larger units for lag 0 alone, a light
// kernel with eight workgroups a compute unit resident and no partners to keep in the caches.  Its slab fits the window's
// (units <= lg.units, 4 lg.cap <= LW lg.cap)
inline size_t lag_sweep_units(size_t N, int W) { return (N + lag_rows(W) - 1) / lag_rows(W); }
inline size_t lag_sweep_workgroups(const LagGeometry &lg, size_t N, int W)
{
  return W == 1 ? std::min(lag_sweep_units(N, 1), 4 * lg.cap) : lg.nwg;
}

// lags t0 .. min(t0 + W - 1, tmax) of the units (of lag_rows(W) rows) blockIdx.x, blockIdx.x + nwg, ...: slab w of part is lag
// t0 + w
template <bool DIAG, int W>
__global__ void __launch_bounds__(SB) k_lagcov(const float *x, const float *ly, int np, int nt, int nc, size_t N, size_t units, int t0,
                                               int tmax, const double *centre, double *part, size_t nwg, size_t R)
{
  __shared__ double red[LWAVES][LENT];
  __shared__ double reda[LWAVES][64], redb[LWAVES][64];
  __shared__ double redll[LWAVES][4];
  int ti = (int)blockIdx.y, tj = ti;
  if (!DIAG) {
    const int nu = nt * (nt - 1) / 2;
    int k = (int)blockIdx.y;
    const bool lower = k >= nu;
    if (lower) k -= nu;
    ti = 0;
    tj = k;
    while (tj >= nt - 1 - ti) {
      tj -= nt - 1 - ti;
      ++ti;
    }
    tj += ti + 1;
    if (lower) {
      const int s = ti;
      ti = tj;
      tj = s;
    }
  }
  const bool first = DIAG && blockIdx.y == 0;
  const size_t pair = DIAG ? blockIdx.y : (size_t)nt + blockIdx.y, S = 2 * (size_t)nt * LTILE + 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, rr = lane >> 4, cc = lane & 15;
  const int ca = ti * LTILE + cc, cb = tj * LTILE + cc;
  const bool oka = ca < np, okb = cb < np;  // a padded column is a column of zeros
  const int la = oka ? ca : 0, lb = okb ? cb : 0;
  const double ma = centre[la], mb = centre[lb], ml = centre[np];
  const size_t r1 = N;
  constexpr int G = lag_groups(W), NA = W == 1 ? 2 : W;  // (one lag: two accumulators in turn, as k_cov_tiles has them)
  lag_f64x4 acc[NA];
  double sa[W], sb[W], sl[W];
#pragma unroll
  for (int w = 0; w < NA; ++w) acc[w] = lag_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int w = 0; w < W; ++w) sa[w] = sb[w] = sl[w] = 0.0;
  for (size_t unit = blockIdx.x; unit < units; unit += nwg) {
    const size_t base = unit * lag_rows(W) + (size_t)wave * (G * 4);
    if (base >= r1) break;  // (the last unit's tail: every later unit of this wavefront lies beyond it too)
    float va[G], vla[G], vb[G][W], vlb[G][W];
    // every load of the G row groups and their W partners is issued before the first product (a row past the end or a
    // partner past the store: a row that exists, read again and masked)
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const size_t row = base + (size_t)(4 * u + rr);
      const size_t rc = row < r1 ? row : r1 - 1;
      va[u] = x[rc * (size_t)np + la];
      vla[u] = DIAG ? ly[rc] : 0.0f;
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const size_t rb = rc + (size_t)(t0 + w) * (size_t)nc;
        const size_t rbc = rb < N ? rb : rc;
        vb[u][w] = x[rbc * (size_t)np + lb];
        vlb[u][w] = DIAG ? ly[rbc] : 0.0f;
      }
    }
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const size_t row = base + (size_t)(4 * u + rr);
      const bool ok = row < r1;
      const double a = ok && oka ? (double)va[u] - ma : 0.0;
      const double l = DIAG && ok ? (double)vla[u] - ml : 0.0;
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const bool okw = ok && row + (size_t)(t0 + w) * (size_t)nc < N;  // the partner is a step of this range
        const double b = okw && okb ? (double)vb[u][w] - mb : 0.0;
        lag_f64x4 &d = acc[W == 1 ? (u & 1) : w];
        d = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, d, 0, 0, 0);
        if (DIAG) {
          const double lw = okw ? (double)vlb[u][w] - ml : 0.0;
          sa[w] = fma(a, lw, sa[w]);
          sb[w] = fma(l, b, sb[w]);
          if (first) sl[w] = fma(l, lw, sl[w]);
        }
      }
    }
  }
  const int t = threadIdx.x;
#pragma unroll
  for (int w = 0; w < W; ++w) {
    if (t0 + w > tmax) break;  // (uniform)
    double *slab = part + (size_t)w * R * nwg;
    if (w > 0) __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) red[wave][(rr + 4 * q) * LTILE + cc] = W == 1 ? acc[0][q] + acc[1][q] : acc[w][q];
    if (DIAG) {
      reda[wave][lane] = sa[w];
      redb[wave][lane] = sb[w];
      if (cc == 0) redll[wave][rr] = sl[w];
    }
    __syncthreads();
    slab[(S + pair * LENT + t) * nwg + blockIdx.x] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    if (DIAG && t < LTILE) {
      double s = 0.0, r = 0.0;
      for (int v = 0; v < LWAVES; ++v)
        for (int g = 0; g < 4; ++g) {
          s += reda[v][g * LTILE + t];
          r += redb[v][g * LTILE + t];
        }
      slab[((size_t)ti * LTILE + t) * nwg + blockIdx.x] = s;
      slab[((size_t)(nt + ti) * LTILE + t) * nwg + blockIdx.x] = r;
    }
    if (first && t == 0) {
      double s = 0.0;
      for (int v = 0; v < LWAVES; ++v)
        for (int g = 0; g < 4; ++g) s += redll[v][g];
      slab[(2 * (size_t)nt * LTILE) * nwg + blockIdx.x] = s;
    }
  }
}

static_assert(LWAVES == 4 && lag_rows(LW) == LROWS && lag_rows(1) <= 4 * LROWS && LW >= 4, "k_lagcov adds four wavefronts; LagGeometry's units are the windows'");

// G(t) [ncol][ncol] from a lag's reduced slab out: every entry as computed; at lag 0 the upper triangle, mirrored.  NaN in the
// row and column of a column that is not finite
void lag_matrix(const double *out, const LagGeometry &lg, const std::vector<char> &fin, int np, bool lag0, double N, double *G)
{
  const int ncol = np + 1, nt = lg.nt, nu = lg.nu;
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  auto put = [&](int i, int j, double s) {
    const double v = fin[i] && fin[j] ? s / N : qnan;
    G[(size_t)i * ncol + j] = v;
    if (lag0) G[(size_t)j * ncol + i] = v;
  };
  int k = 0;
  for (int ti = 0; ti < nt; ++ti)
    for (int tj = ti; tj < nt; ++tj) {
      const int pair = ti == tj ? ti : nt + k;
      const double *up = out + lg.S + (size_t)pair * LENT, *lo = ti == tj ? up : up + (size_t)nu * LENT;
      for (int i = 0; i < LTILE && ti * LTILE + i < np; ++i)
        for (int j = 0; j < LTILE && tj * LTILE + j < np; ++j) {
          if (lag0 && ti == tj && j < i) continue;
          put(ti * LTILE + i, tj * LTILE + j, up[i * LTILE + j]);
          if (!lag0 && ti != tj) put(tj * LTILE + j, ti * LTILE + i, lo[j * LTILE + i]);
        }
      if (ti != tj) ++k;
    }
  for (int c = 0; c < np; ++c) {
    put(c, np, out[c]);
    if (!lag0) put(np, c, out[(size_t)nt * LTILE + c]);
  }
  put(np, np, out[2 * (size_t)nt * LTILE]);
}

enum { LT_MOMENTS, LT_LAG0, LT_WINDOWS, LT_REDUCE, LT_TOTAL, LT_N };
static_assert(LT_N == MCX_LAGCOV_TIMES, "include/mcx.h lists the stages");

// one sweep: lags t0 .. t0 + nl - 1 into G (host), W = 1 for lag 0 and LW beyond
template <int W>
int lag_sweep(hipStream_t st, StageTimer &tm, const StoreView &v, const LagGeometry &lg, const double *ctr, double *part, double *out,
              int t0, int nl, const std::vector<char> &fin, std::vector<double> &G)
{
  const int np = v.np, nt = lg.nt, noff = t0 == 0 ? lg.nu : 2 * lg.nu, tmax = t0 + nl - 1;
  const size_t N = (size_t)v.N, rows = t0 == 0 ? lg.R0 : (size_t)nl * lg.R, nn = (size_t)v.ncol * v.ncol;
  const size_t units = lag_sweep_units(N, W), nwg = lag_sweep_workgroups(lg, N, W);
  MCXCHK(tm.run(t0 == 0 ? LT_LAG0 : LT_WINDOWS, [&]() -> int {
    hipLaunchKernelGGL((k_lagcov<true, W>), dim3((unsigned)nwg, (unsigned)nt), dim3(SB), 0, st, v.x, v.ly, np, nt, v.nc, N, units, t0,
                       tmax, ctr, part, nwg, lg.R);
    HIPCHK(hipGetLastError());
    if (noff > 0) {
      hipLaunchKernelGGL((k_lagcov<false, W>), dim3((unsigned)nwg, (unsigned)noff), dim3(SB), 0, st, v.x, v.ly, np, nt, v.nc, N, units,
                         t0, tmax, ctr, part, nwg, lg.R);
      HIPCHK(hipGetLastError());
    }
    return MCX_OK;
  }));
  MCXCHK(tm.run(LT_REDUCE, [&]() -> int {
    hipLaunchKernelGGL(k_sum_rows, dim3((unsigned)rows), dim3(SB), 0, st, (const double *)part, nwg, 1, 1, 1, nwg, nwg,
                       (const double *)nullptr, 0.0, out);
    HIPCHK(hipGetLastError());
    return MCX_OK;
  }));
  std::vector<double> h(rows);
  HIPCHK(hipMemcpyAsync(h.data(), out, rows * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  G.resize((size_t)(t0 + nl) * nn);
  for (int w = 0; w < nl; ++w) lag_matrix(h.data() + (size_t)w * lg.R, lg, fin, np, t0 + w == 0, (double)N, G.data() + (size_t)(t0 + w) * nn);
  return MCX_OK;
}

// the lags a call computes at the most, and its windows beyond lag 0
inline int last_lag(int64_t T, int max_lag) { return (int)std::min<int64_t>(T - 1, max_lag); }

// G(t), the walk and the numbers made of Sigma for a view on stream st.  ms (MCX_LAGCOV_TIMES doubles, or NULL): the stage times
int lagcov_device(hipStream_t st, DevBuf<double> *buf, const StoreView &v, const mcx_lagcov_spec &spec, mcx_lagcov_result *res,
                  mcx_col_lagcov *cols, double *sigma, double *gamma, double *ms)
{
  StageTimer tm{st, ms, LT_N, {}};
  const int nc = v.nc, np = v.np, ncol = v.ncol, L = last_lag(v.T, spec.max_lag);
  const size_t N = (size_t)v.N, nn = (size_t)ncol * ncol;
  const LagGeometry lg = lag_geometry(N, np);
  // device double scratch: hm[ncol][2][nc] | tot[ncol][nc] | colsum[ncol] | centre[ncol] | part[LW][R][nwg] | out[LW][R]
  const size_t o_hm = 0, o_tot = o_hm + (size_t)ncol * 2 * nc, o_cs = o_tot + (size_t)ncol * nc, o_ctr = o_cs + ncol,
               o_part = o_ctr + ncol, o_out = o_part + (size_t)LW * lg.R * lg.nwg, nd = o_out + (size_t)LW * lg.R;
  MCXCHK(buf->alloc(nd));
  double *D = buf->p;
  std::vector<double> G;
  std::vector<char> fin(ncol);
  std::vector<unsigned char> use(ncol);
  std::vector<int> cflags(ncol);
  std::vector<double> ess(ncol), mcse(ncol), mean(ncol), cs(ncol);
  H::Result hr{};
  int have = 0;
  MCXCHK(tm.run(LT_TOTAL, [&]() -> int {
    // ---- 1. column sums -> mean (the expression of mcx_samples_summary), flags
    MCXCHK(tm.run(LT_MOMENTS, [&]() -> int { return sweep_moments(st, v, D + o_hm, D + o_tot); }));
    MCXCHK(column_sums(st, v, D + o_tot, D + o_cs));
    HIPCHK(hipMemcpyAsync(cs.data(), D + o_cs, cs.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int c = 0; c < ncol; ++c) {
      fin[c] = std::isfinite(cs[c]) ? 1 : 0;
      mean[c] = fin[c] ? cs[c] / (double)N : std::numeric_limits<double>::quiet_NaN();  // (the centre: NaN for such a column)
      use[c] = fin[c] && (c < np || spec.with_ll);
    }
    HIPCHK(hipMemcpyAsync(D + o_ctr, mean.data(), mean.size() * sizeof(double), hipMemcpyHostToDevice, st));
    // ---- 2. lag 0, 3. windows while the walk asks for them
    MCXCHK((lag_sweep<1>(st, tm, v, lg, D + o_ctr, D + o_part, D + o_out, 0, 1, fin, G)));
    have = 1;
    // (the lags asked for are swept even beyond max_lag, which bounds the walk alone)
    const int Lc = std::max(L, spec.nlags_out - 1);
    int target = std::min(Lc + 1, std::max(spec.nlags_out, 1 + LW));
    for (;;) {
      while (have < target) {
        const int nl = std::min(LW, Lc + 1 - have);
        MCXCHK((lag_sweep<LW>(st, tm, v, lg, D + o_ctr, D + o_part, D + o_out, have, nl, fin, G)));
        have += nl;
      }
      const bool stopped = H::finish(ncol, std::min(have, L + 1), (long long)N, G.data(), use.data(), &hr, cflags.data(), ess.data(),
                                     mcse.data(), sigma);
      if (stopped || hr.p == 0 || have >= L + 1) break;  // (no column chosen: more lags decide nothing)
      target = std::min(L + 1, 1 + 2 * (have - 1));
    }
    return MCX_OK;
  }));
  MCXCHK(tm.collect());
  res->N = hr.N;
  res->p = hr.p;
  res->s = hr.s;
  res->k_used = hr.k_used;
  res->lags_used = hr.lags_used;
  res->lags_computed = have;
  res->flags = hr.flags;
  res->mess = hr.mess;
  res->logdet_lambda = hr.logdet_lambda;
  res->logdet_sigma = hr.logdet_sigma;
  for (int c = 0; c < ncol; ++c) {
    cols[c].mean = mean[c];
    cols[c].ess = ess[c];
    cols[c].mcse = mcse[c];
    cols[c].flags = fin[c] ? cflags[c] : MCX_SUMMARY_NONFINITE;
    cols[c].reserved = 0;
  }
  if (spec.nlags_out > 0) std::memcpy(gamma, G.data(), (size_t)spec.nlags_out * nn * sizeof(double));
  return MCX_OK;
}

// what every entry point refuses before a device is touched: the range and the spec, then with the outputs
int lagcov_range_args(int64_t nsteps, int nc, const mcx_lagcov_spec *spec)
{
  if (nsteps < 4) return fail(MCX_ERR_INVALID, "a lagged covariance needs nsteps >= 4, got %lld", (long long)nsteps);
  if (nc >= 1 && nsteps * nc < 2) return fail(MCX_ERR_INVALID, "a lagged covariance needs nsteps * nc >= 2 rows");
  if (spec->max_lag < 1) return fail(MCX_ERR_INVALID, "max_lag = %d: at least 1", spec->max_lag);
  if (spec->nlags_out < 0 || spec->nlags_out > nsteps)
    return fail(MCX_ERR_INVALID, "nlags_out = %d: 0 to nsteps = %lld lags", spec->nlags_out, (long long)nsteps);
  return MCX_OK;
}
int lagcov_args(int64_t nsteps, int nc, const mcx_lagcov_spec *spec, const mcx_lagcov_result *res, const mcx_col_lagcov *cols,
                const double *sigma, const double *gamma)
{
  if (!spec) return fail(MCX_ERR_INVALID, "spec is NULL");
  if (!res || !cols || !sigma) return fail(MCX_ERR_INVALID, "an output (res, cols or sigma) is NULL");
  MCXCHK(lagcov_range_args(nsteps, nc, spec));
  if (spec->nlags_out > 0 && !gamma) return fail(MCX_ERR_INVALID, "gamma is NULL and nlags_out = %d", spec->nlags_out);
  return MCX_OK;
}

}  // namespace

extern "C" int mcx_samples_lagcov(mcx_engine *e, int first_step, int nsteps, const mcx_lagcov_spec *spec, mcx_lagcov_result *res,
                                  mcx_col_lagcov *cols, double *sigma, double *gamma)
{
  return on_store(
      e, first_step, nsteps, [&] { return lagcov_args(nsteps, e->nchain, spec, res, cols, sigma, gamma); },
      [&](hipStream_t st, Bufs B, const StoreView &v) { return lagcov_device(st, B.d, v, *spec, res, cols, sigma, gamma, nullptr); });
}

extern "C" int mcx_rows_lagcov(const float *rows, int nsteps, int nc, int np, const mcx_lagcov_spec *spec, mcx_lagcov_result *res,
                               mcx_col_lagcov *cols, double *sigma, double *gamma)
{
  if (!rows) return fail(MCX_ERR_INVALID, "rows is NULL");
  if (nc < 1) return fail(MCX_ERR_INVALID, "nc = %d: at least one chain", nc);
  if (np < 1 || np > 256) return fail(MCX_ERR_INVALID, "np = %d: 1 to 256 parameters", np);
  MCXCHK(lagcov_args(nsteps, nc, spec, res, cols, sigma, gamma));
  return on_rows(rows, nsteps, nc, np, [&](hipStream_t st, Bufs B, const StoreView &v) {
    return lagcov_device(st, B.d, v, *spec, res, cols, sigma, gamma, nullptr);
  });
}

extern "C" int mcx_store_lagcov(mcx_store *s, const mcx_lagcov_spec *spec, mcx_lagcov_result *res, mcx_col_lagcov *cols, double *sigma,
                                double *gamma)
{
  if (!s) return fail(MCX_ERR_INVALID, "the store s is NULL");
  MCXCHK(lagcov_args(s->T, s->nc, spec, res, cols, sigma, gamma));
  HIPCHK(hipSetDevice(s->device));
  return lagcov_device(s->st, &s->d, StoreView(s->span()), *spec, res, cols, sigma, gamma, nullptr);
}

extern "C" int mcx_debug_lagcov_times(mcx_engine *e, int first_step, int nsteps, const mcx_lagcov_spec *spec, mcx_lagcov_result *res,
                                      double *ms)
{
  std::vector<mcx_col_lagcov> cols;
  std::vector<double> sigma, gamma;
  return on_store(
      e, first_step, nsteps,
      [&] {
        if (!ms) return fail(MCX_ERR_INVALID, "ms is NULL");
        if (!spec) return fail(MCX_ERR_INVALID, "spec is NULL");
        if (!res) return fail(MCX_ERR_INVALID, "res is NULL");
        MCXCHK(lagcov_range_args(nsteps, e->nchain, spec));
        const size_t ncol = (size_t)e->nparam + 1;  // (nothing is allocated before this line)
        cols.resize(ncol);
        sigma.resize(ncol * ncol);
        gamma.resize(ncol * ncol * (size_t)spec->nlags_out + 1);
        return (int)MCX_OK;
      },
      [&](hipStream_t st, Bufs B, const StoreView &v) {
        return lagcov_device(st, B.d, v, *spec, res, cols.data(), sigma.data(), gamma.data(), ms);
      });
}

// host only
extern "C" int mcx_mess_finish(int ncol, int nlags, long long N, const double *gamma, const unsigned char *use, mcx_lagcov_result *res,
                               mcx_col_lagcov *cols, double *sigma)
{
  if (!gamma || !res || !cols || !sigma) return fail(MCX_ERR_INVALID, "gamma or an output (res, cols or sigma) is NULL");
  if (ncol < 1 || ncol > 257) return fail(MCX_ERR_INVALID, "ncol = %d: 1 to 257 columns", ncol);
  if (nlags < 2) return fail(MCX_ERR_INVALID, "nlags = %d: lags 0 and 1 at least", nlags);
  if (N < 2) return fail(MCX_ERR_INVALID, "N = %lld: at least two rows", N);
  std::vector<unsigned char> all((size_t)ncol, 1);
  std::vector<int> cflags(ncol);
  std::vector<double> ess(ncol), mcse(ncol);
  H::Result hr{};
  H::finish(ncol, nlags, N, gamma, use ? use : all.data(), &hr, cflags.data(), ess.data(), mcse.data(), sigma);
  res->N = hr.N;
  res->p = hr.p;
  res->s = hr.s;
  res->k_used = hr.k_used;
  res->lags_used = hr.lags_used;
  res->lags_computed = nlags;
  res->flags = hr.flags;
  res->mess = hr.mess;
  res->logdet_lambda = hr.logdet_lambda;
  res->logdet_sigma = hr.logdet_sigma;
  for (int c = 0; c < ncol; ++c) {
    const double g = gamma[(size_t)c * ncol + c];
    cols[c].mean = std::numeric_limits<double>::quiet_NaN();  // (the matrices do not hold it)
    cols[c].ess = ess[c];
    cols[c].mcse = mcse[c];
    cols[c].flags = g != g ? MCX_SUMMARY_NONFINITE : cflags[c];
    cols[c].reserved = 0;
  }
  return MCX_OK;
}

// host only
extern "C" int mcx_debug_lagcov_geometry(int nsteps, int nc, int np, int nlags, mcx_lagcov_geometry *g)
{
  if (!g) return fail(MCX_ERR_INVALID, "g is NULL");
  if (nc < 1 || np < 1 || np > 256) return fail(MCX_ERR_INVALID, "nc = %d, np = %d: at least one chain, 1 to 256 parameters", nc, np);
  if (nsteps < 4) return fail(MCX_ERR_INVALID, "a lagged covariance needs nsteps >= 4, got %d", nsteps);
  if (nlags < 1 || nlags > nsteps) return fail(MCX_ERR_INVALID, "nlags = %d: 1 to nsteps = %d lags", nlags, nsteps);
  const size_t N = (size_t)nsteps * nc;
  const LagGeometry lg = lag_geometry(N, np);
  g->block = SB;
  g->window_lags = LW;
  g->rows_per_iteration = LROWS;
  g->units = (long long)lg.units;
  g->workgroups = (long long)lg.nwg;
  g->tiles = lg.nt;
  g->pairs_lag0 = lg.nt + lg.nu;
  g->pairs = (long long)lg.nt * lg.nt;
  g->slab_rows = (long long)lg.R;
  g->windows = (nlags - 1 + LW - 1) / LW;
  g->launches = 1 + g->windows;
  g->lags_computed = std::min<long long>(nsteps, 1 + g->windows * LW);
  g->scratch_bytes = 8 * ((long long)(np + 1) * (3LL * nc + 2) + (long long)LW * (long long)lg.R * (long long)(lg.nwg + 1));
  g->units_lag0 = (long long)lag_sweep_units(N, 1);
  g->workgroups_lag0 = (long long)lag_sweep_workgroups(lg, N, 1);
  return MCX_OK;
}
