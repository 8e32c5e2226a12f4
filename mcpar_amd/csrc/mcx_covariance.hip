// mcx_covariance.hip -- mcx_samples_covariance / mcx_rows_covariance: the (np + 1) x (np + 1) covariance of a step range of
// the sample store on the device, and mcx_proposal_from_cov, the host step from that matrix to the
// incov of the next run.
//
// The store is x[step][chain][np] plus ly[step][chain]: N = nsteps * nc rows of np contiguous floats, row r of x at
// r * np, its log L at ly[r].  Passes:
//   1. k_sum_moments + k_sum_rows   the column sums (mcx_summary_kernels.hpp: the bytes mcx_samples_summary's mean is made of)
//   2. k_cov_tiles                  one sweep over the rows: Xc^T Xc in fp64 on the matrix cores, Xc = the rows centred on
//                                   the mean of pass 1; grid = (workgroups over rows, pairs of 16-column tiles ti <= tj):
//                                   one launch for the nt diagonal pairs, one for the nt (nt - 1) / 2 others
//   3. k_sum_rows                   the workgroups' partials, [entry][workgroup] slabs, summed in a fixed order
// v_mfma_f64_16x16x4_f64 takes A (16 x 4) and B (4 x 16) as ONE double per lane, A[i = lane & 15][k = lane >> 4] and
// B[k = lane >> 4][j = lane & 15]: with a lane holding the centred x[row r0 + (lane >> 4)][column c0 + (lane & 15)] of a
// tile, that one register is A of the tile (transposed rows) and B of the tile at once, and D += A B adds four rows'
// outer products.  D: 4 doubles per lane, D[i = (lane >> 4) + 4 reg][j = lane & 15].  The log L column is not a tile: a
// diagonal tile pair adds one FMA per lane and row group (centred x times the row's centred log L), summed over the four
// lane >> 4 groups at the end.  No float atomics; a workgroup's four wavefronts are added in wavefront order.
#include "mcx_summary_kernels.hpp"

#include <limits>

namespace {

typedef double cov_f64x4 __attribute__((ext_vector_type(4)));

constexpr int CTILE = 16;                // columns per tile: the matrix-core shape
constexpr int CGRP = 8;                  // row groups (of 4 rows) a wavefront loads before it multiplies them
constexpr int CWAVES = SB / 64;          // wavefronts per workgroup
constexpr int CROWS = CWAVES * CGRP * 4;  // rows a workgroup takes per iteration
constexpr int CENT = CTILE * CTILE;      // entries of a tile pair

// part[row][workgroup], rows: [pair][CENT] | [tile][CTILE] (parameter x log L) | log L x log L; pair = tile t for the
// diagonal pair (t, t) (DIAG: blockIdx.y = t), nt + k for the k-th pair ti < tj, row by row of the strict upper triangle
// (!DIAG: blockIdx.y = k)
template <bool DIAG>
__global__ void __launch_bounds__(SB) k_cov_tiles(const float *x, const float *ly, int np, int nt, size_t N, size_t rpw,
                                                  const double *centre, double *part, size_t nwg)
{
  __shared__ double red[CWAVES][CENT];
  __shared__ double redl[CWAVES][64];
  __shared__ double redll[CWAVES][4];
  int ti = (int)blockIdx.y, tj = ti;
  if (!DIAG) {
    ti = 0;
    while (tj >= nt - 1 - ti) {
      tj -= nt - 1 - ti;
      ++ti;
    }
    tj += ti + 1;
  }
  constexpr bool diag = DIAG;
  const bool first = DIAG && blockIdx.y == 0;
  const size_t pair = DIAG ? blockIdx.y : (size_t)nt + blockIdx.y, npairs = (size_t)nt * (nt + 1) / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, rr = lane >> 4, cc = lane & 15;
  const int ca = ti * CTILE + cc, cb = tj * CTILE + cc;
  const bool oka = ca < np, okb = cb < np;  // a padded column is a column of zeros
  const int la = oka ? ca : 0, lb = okb ? cb : 0;
  const double ma = centre[la], mb = centre[lb], ml = centre[np];
  const size_t r0 = (size_t)blockIdx.x * rpw, r1 = r0 + rpw < N ? r0 + rpw : N;
  cov_f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
  double accl = 0.0, accll = 0.0;
  for (size_t base = r0 + (size_t)wave * (CGRP * 4); base < r1; base += CROWS) {
    float va[CGRP], vb[CGRP], vl[CGRP];
    bool ok[CGRP];
    // every load of the CGRP row groups is issued before the first product (rows past the end: the last row again, masked)
#pragma unroll
    for (int u = 0; u < CGRP; ++u) {
      const size_t row = base + (size_t)(4 * u + rr);
      ok[u] = row < r1;
      const size_t rc = ok[u] ? row : r1 - 1;
      va[u] = x[rc * (size_t)np + la];
      vb[u] = diag ? 0.0f : x[rc * (size_t)np + lb];
      vl[u] = diag ? ly[rc] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < CGRP; ++u) {
      const double a = ok[u] && oka ? (double)va[u] - ma : 0.0;
      const double b = diag ? a : (ok[u] && okb ? (double)vb[u] - mb : 0.0);
      if (u & 1) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc1, 0, 0, 0);
      else acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc0, 0, 0, 0);
      if (diag) {
        const double l = ok[u] ? (double)vl[u] - ml : 0.0;
        accl = fma(a, l, accl);
        if (first) accll = fma(l, l, accll);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) red[wave][(rr + 4 * q) * CTILE + cc] = acc0[q] + acc1[q];
  redl[wave][lane] = accl;
  if (cc == 0) redll[wave][rr] = accll;
  __syncthreads();
  const int t = threadIdx.x;
  part[(pair * CENT + t) * nwg + blockIdx.x] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
  if (diag && t < CTILE) {
    double s = 0.0;
    for (int w = 0; w < CWAVES; ++w)
      for (int g = 0; g < 4; ++g) s += redl[w][g * CTILE + t];
    part[(npairs * CENT + (size_t)ti * CTILE + t) * nwg + blockIdx.x] = s;
  }
  if (first && t == 0) {
    double s = 0.0;
    for (int w = 0; w < CWAVES; ++w)
      for (int g = 0; g < 4; ++g) s += redll[w][g];
    part[(npairs * CENT + (size_t)nt * CTILE) * nwg + blockIdx.x] = s;
  }
}

}  // namespace

static_assert(CWAVES == 4, "k_cov_tiles adds four wavefronts");

// the matrix from the reduced sums out (k_cov_tiles' row layout): the upper triangle as computed, mirrored; NaN in the row
// and column of a column that is not finite
static void cov_matrix(const std::vector<double> &out, const std::vector<char> &fin, int np, double dof, double *cov)
{
  const int ncol = np + 1, nt = (np + CTILE - 1) / CTILE, npairs = nt * (nt + 1) / 2;
  auto put = [&](int i, int j, double s) {
    const double v = fin[i] && fin[j] ? s / dof : std::numeric_limits<double>::quiet_NaN();
    cov[(size_t)i * ncol + j] = v;
    cov[(size_t)j * ncol + i] = v;
  };
  int off = nt;
  for (int ti = 0; ti < nt; ++ti)
    for (int tj = ti; tj < nt; ++tj) {
      const int pair = ti == tj ? ti : off++;
      for (int i = 0; i < CTILE && ti * CTILE + i < np; ++i)
        for (int j = ti == tj ? i : 0; j < CTILE && tj * CTILE + j < np; ++j)
          put(ti * CTILE + i, tj * CTILE + j, out[(size_t)pair * CENT + i * CTILE + j]);
    }
  for (int c = 0; c < np; ++c) put(c, np, out[(size_t)npairs * CENT + c]);
  put(np, np, out[(size_t)npairs * CENT + (size_t)nt * CTILE]);
}

// mean, covariance and flags of a view on stream st.  ms (mcx_debug_covariance_times, else NULL): ms[0] k_sum_moments,
// ms[1] k_cov_tiles, ms[2] the reducer of its partials; the column sums and the host round trip between them are not timed
static int covariance_device(hipStream_t st, DevBuf<double> *buf, const StoreView &v, double *mean, double *cov, int *flags,
                             double *ms)
{
  StageTimer tm{st, ms, 3, {}};
  const int nc = v.nc, np = v.np, ncol = v.ncol, nt = (np + CTILE - 1) / CTILE, npairs = nt * (nt + 1) / 2;
  const size_t N = (size_t)v.N;
  // workgroups over the rows: a function of N and np alone (the partials' order is part of the result's bytes)
  const size_t nwg_max = std::max<size_t>(128, 2048 / (size_t)npairs);
  const size_t rpw = ((N + nwg_max - 1) / nwg_max + CROWS - 1) / CROWS * CROWS, nwg = (N + rpw - 1) / rpw;
  const size_t R = (size_t)npairs * CENT + (size_t)nt * CTILE + 1;
  // device double scratch: hm[ncol][2][nc] | tot[ncol][nc] | colsum[ncol] | centre[ncol] | part[R][nwg] | out[R]
  const size_t o_hm = 0, o_tot = o_hm + (size_t)ncol * 2 * nc, o_cs = o_tot + (size_t)ncol * nc, o_ctr = o_cs + ncol,
               o_part = o_ctr + ncol, o_out = o_part + R * nwg, nd = o_out + R;
  MCXCHK(buf->alloc(nd));
  double *D = buf->p;

  // ---- 1. column sums -> mean (the expression of mcx_samples_summary), flags
  MCXCHK(tm.run(0, [&]() -> int { return sweep_moments(st, v, D + o_hm, D + o_tot); }));
  MCXCHK(column_sums(st, v, D + o_tot, D + o_cs));
  std::vector<double> cs(ncol), ctr(ncol);
  HIPCHK(hipMemcpyAsync(cs.data(), D + o_cs, cs.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  std::vector<char> fin(ncol);
  for (int c = 0; c < ncol; ++c) {
    fin[c] = std::isfinite(cs[c]) ? 1 : 0;
    mean[c] = fin[c] ? cs[c] / (double)N : qnan;
    ctr[c] = mean[c];  // a column that is not finite is centred on NaN: only its own row and column see it
    if (flags) flags[c] = fin[c] ? 0 : MCX_SUMMARY_NONFINITE;
  }
  HIPCHK(hipMemcpyAsync(D + o_ctr, ctr.data(), ctr.size() * sizeof(double), hipMemcpyHostToDevice, st));

  // ---- 2. the sweep, 3. its partials
  MCXCHK(tm.run(1, [&]() -> int {
    hipLaunchKernelGGL(k_cov_tiles<true>, dim3((unsigned)nwg, (unsigned)nt), dim3(SB), 0, st, v.x, v.ly, np, nt, N, rpw,
                       (const double *)(D + o_ctr), D + o_part, nwg);
    HIPCHK(hipGetLastError());
    if (npairs > nt) {
      hipLaunchKernelGGL(k_cov_tiles<false>, dim3((unsigned)nwg, (unsigned)(npairs - nt)), dim3(SB), 0, st, v.x, v.ly, np, nt, N, rpw,
                         (const double *)(D + o_ctr), D + o_part, nwg);
      HIPCHK(hipGetLastError());
    }
    return MCX_OK;
  }));
  MCXCHK(tm.run(2, [&]() -> int {
    hipLaunchKernelGGL(k_sum_rows, dim3((unsigned)R), dim3(SB), 0, st, D + o_part, nwg, 1, 1, 1, nwg, nwg, (const double *)nullptr,
                       0.0, D + o_out);
    HIPCHK(hipGetLastError());
    return MCX_OK;
  }));
  std::vector<double> out(R);
  HIPCHK(hipMemcpyAsync(out.data(), D + o_out, R * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));  // (ctr is read by the upload until here)
  MCXCHK(tm.collect());

  cov_matrix(out, fin, np, (double)(N - 1), cov);
  return MCX_OK;
}

static int covariance_args(int nsteps, int nc, const double *mean, const double *cov)
{
  if (!mean || !cov) return fail(MCX_ERR_INVALID, "mean or cov is NULL");
  if (nsteps < 1) return fail(MCX_ERR_INVALID, "a covariance needs nsteps >= 1, got %d", nsteps);
  if ((int64_t)nsteps * nc < 2) return fail(MCX_ERR_INVALID, "a covariance needs nsteps * nc >= 2 rows, got 1");
  return MCX_OK;
}

int covariance_span(hipStream_t st, Bufs B, const StoreSpan &s, double *mean, double *cov, int *flags)
{
  MCXCHK(covariance_args((int)s.T, s.nc, mean, cov));
  return covariance_device(st, B.d, StoreView(s), mean, cov, flags, nullptr);
}

extern "C" int mcx_samples_covariance(mcx_engine *e, int first_step, int nsteps, double *mean, double *cov, int *flags)
{
  return on_store(
      e, first_step, nsteps, [&] { return covariance_args(nsteps, e->nchain, mean, cov); },
      [&](hipStream_t st, Bufs B, const StoreView &v) { return covariance_device(st, B.d, v, mean, cov, flags, nullptr); });
}

extern "C" int mcx_debug_covariance_times(mcx_engine *e, int first_step, int nsteps, double *ms)
{
  std::vector<double> mean, cov;
  return on_store(
      e, first_step, nsteps,
      [&] {
        if (!ms) return fail(MCX_ERR_INVALID, "ms is NULL");
        mean.resize((size_t)e->nparam + 1);
        cov.resize(mean.size() * mean.size());
        return covariance_args(nsteps, e->nchain, mean.data(), cov.data());
      },
      [&](hipStream_t st, Bufs B, const StoreView &v) { return covariance_device(st, B.d, v, mean.data(), cov.data(), nullptr, ms); });
}

extern "C" int mcx_rows_covariance(const float *rows, int nsteps, int nc, int np, double *mean, double *cov, int *flags)
{
  if (nc < 1) return fail(MCX_ERR_INVALID, "bad arguments");
  MCXCHK(covariance_args(nsteps, nc, mean, cov));
  return on_rows(rows, nsteps, nc, np, [&](hipStream_t st, Bufs B, const StoreView &v) {
    return covariance_device(st, B.d, v, mean, cov, flags, nullptr);
  });
}

// host only
extern "C" int mcx_proposal_from_cov(int np, const double *cov, int ld, double scale, float *incov)
{
  if (np < 1 || np > 256 || !cov || !incov || ld < np) return fail(MCX_ERR_INVALID, "bad arguments");
  const double s = scale > 0.0 ? scale : 2.38 * 2.38 / (double)np;
  for (int i = 0; i < np; ++i)
    for (int j = i; j < np; ++j) {
      const double v = cov[(size_t)i * ld + j], w = cov[(size_t)j * ld + i];
      const float f = (float)(s * v);
      if (!std::isfinite(v) || !std::isfinite(w) || !std::isfinite(f))
        return fail(MCX_ERR_INVALID, "covariance entry (%d, %d) is not finite (column %d)", i, j, std::isfinite(cov[(size_t)i * ld + i]) ? j : i);
      incov[(size_t)i * np + j] = f;
      incov[(size_t)j * np + i] = f;
    }
  std::vector<float> c(incov, incov + (size_t)np * np);
  const int rc = cholesky_lower(np, c.data());
  if (rc != 0)
    return fail(MCX_ERR_INVALID, "the proposal covariance is not positive definite in float: pivot %d (column %d) is not > 0",
                rc - 1, rc - 1);
  return MCX_OK;
}
