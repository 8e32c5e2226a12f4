// mcx_summary.hip -- mcx_samples_summary / mcx_rows_summary: per-column statistics of a step range of the sample store on the
// device (DESIGN.md "Sample-store summaries"), and mcx_debug_summary_finish, the host step that turns the reduced sums into
// R-hat, ESS and quantiles.
//
// The store is x[step][chain][np] plus ly[step][chain].  Every kernel maps one thread to one (chain, column) SERIES of a
// column tile: a workgroup holds cg chains x ct adjacent columns (ct = 1 for the log L column), so one load of all its
// threads at a step reads one contiguous segment per chain.  Passes:
//   1. k_sum_moments    per series: sum of each half-chain and of all steps (fp64) -> [col][2][nc] means, [col][nc] sums
//   2. k_sum_hist x 4   radix select of the order statistics, 8 bits per pass: LDS histograms of the values whose key
//                       matches one of the column's target prefixes, integer-added to global
//   3. k_sum_acov       lag windows of 32: sum_i c_i c_{i+t} over both halves, t in [32k, 32k + 32), and (k = 0) the
//                       centred sum of squares about the column mean; only for the columns whose Geyer loop asks
// Every cross-chain sum goes through per-workgroup slabs and k_sum_rows (one workgroup per output, a fixed order): the bytes
// do not depend on scheduling.  No float atomics.
#include "mcx_summary_kernels.hpp"

#include <limits>

namespace {

constexpr int WLAG = 32;    // lags per window
constexpr int NQ = WLAG + 1;  // a window's outputs per column: 32 lag sums, then the centred sum of squares
constexpr int GMAX = 32;    // target prefixes per column per histogram launch
constexpr int64_t HIST_CHUNK = 1 << 16;  // steps per workgroup of a histogram pass (LDS counts stay below 2^32)

__device__ __forceinline__ uint32_t okey(float v)
{
  const uint32_t u = __float_as_uint(v);
  if (v != v) return 0xffffffffu;  // every NaN sorts last
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// pass 2: one radix digit.  grid = (nbc * ntiles, step chunks); LDS: counts[ct][gn][256], prefixes[ct][gn]
__global__ void __launch_bounds__(SB) k_sum_hist(TileSet t, int nc, int64_t T, int shift, const uint32_t *gpfx,
                                                 const int *gcnt, int G, int g0, int gn, unsigned long long *hist)
{
  extern __shared__ uint32_t lds[];
  uint32_t *cnt = lds, *pfx = lds + (size_t)t.ct * gn * 256;
  int *ng = (int *)(pfx + (size_t)t.ct * gn);
  const int tile = blockIdx.x % t.ntiles, bc = blockIdx.x / t.ntiles;
  for (int i = threadIdx.x; i < t.ct * gn * 256; i += SB) cnt[i] = 0;
  for (int i = threadIdx.x; i < t.ct * gn; i += SB) {
    const int j = i / gn, g = i - j * gn, lc = tile * t.ct + j;
    pfx[i] = lc < t.ncs && g0 + g < G ? gpfx[(size_t)(t.col0 + lc) * G + g0 + g] : 0u;
  }
  for (int j = threadIdx.x; j < t.ct; j += SB) {
    const int lc = tile * t.ct + j;
    ng[j] = lc < t.ncs ? min(gn, max(0, gcnt[t.col0 + lc] - g0)) : 0;
  }
  __syncthreads();
  const Lane l = lane_of(t, tile, bc, nc);
  const int m = l.ok ? ng[l.j] : 0;
  if (m > 0) {
    const uint32_t *mp = pfx + (size_t)l.j * gn;
    uint32_t *mc = cnt + (size_t)l.j * gn * 256;
    const float *p = t.src + (size_t)l.chain * t.cs + l.lcol;
    const int64_t s0 = (int64_t)blockIdx.y * HIST_CHUNK, s1 = min(T, s0 + HIST_CHUNK);
    const int dsh = shift - 8;
    for (int64_t s = s0; s < s1; ++s) {
      const uint32_t key = okey(p[s * t.rs]);
      const uint32_t kp = (uint32_t)((uint64_t)key >> shift);
      int lo = 0, hi = m;  // the column's prefixes are sorted and distinct: binary search
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (mp[mid] <= kp) lo = mid; else hi = mid;
      }
      if (mp[lo] == kp) atomicAdd(&mc[lo * 256 + ((key >> dsh) & 255u)], 1u);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < t.ct * gn * 256; i += SB) {
    const uint32_t c = cnt[i];
    if (!c) continue;
    const int j = i / (gn * 256), r = i - j * gn * 256, g = r >> 8, lc = tile * t.ct + j;
    if (lc < t.ncs && g0 + g < G)
      atomicAdd(&hist[((size_t)(t.col0 + lc) * G + g0 + g) * 256 + (r & 255)], (unsigned long long)c);
  }
}

// pass 3: lag windows k0 .. k0 + KW - 1.  grid = KW * ntiles * nbc, the window fastest (its workgroups read the same rows).
// part[((y * ncol + col) * NQ + q) * pstride + bc]
__global__ void __launch_bounds__(SB) k_sum_acov(TileSet t, int nc, int64_t T, int64_t n, int k0, int KW, int ncol,
                                                 const double *hm, const double *coltot, double Nd, const int *active,
                                                 double *part, size_t pstride)
{
  __shared__ double red[SB];
  const int y = blockIdx.x % KW, r = blockIdx.x / KW, tile = r % t.ntiles, bc = r / t.ntiles;
  const Lane l = lane_of(t, tile, bc, nc);
  const int col = t.col0 + l.lcol;
  const bool on = l.ok && active[col];
  const int64_t lag0 = (int64_t)(k0 + y) * WLAG;
  double acc[WLAG], ss = 0.0;
#pragma unroll
  for (int q = 0; q < WLAG; ++q) acc[q] = 0.0;
  if (on) {
    const float *p = t.src + (size_t)l.chain * t.cs + l.lcol;
    const double mu = coltot[col] / Nd;  // the reported mean: a constant column gives a zero sum
    for (int h = 0; h < 2; ++h) {
      const float *ph = p + (size_t)(h ? T - n : 0) * t.rs;
      const double m = hm[((size_t)col * 2 + h) * nc + l.chain];
      double ring[WLAG];
#pragma unroll
      for (int q = 0; q < WLAG; ++q) ring[q] = 0.0;
      for (int64_t i = 0; i < n; i += WLAG) {
#pragma unroll
        for (int u = 0; u < WLAG; ++u) {
          const int64_t a = i + u;
          double c = 0.0, dv = 0.0;
          if (a < n) {
            const double v = (double)ph[a * t.rs];
            c = v - m;
            if (lag0 == 0) {
              dv = c;
              ss = fma(v - mu, v - mu, ss);
            } else if (a >= lag0) {
              dv = (double)ph[(a - lag0) * t.rs] - m;
            }
          }
          ring[u] = dv;
#pragma unroll
          for (int q = 0; q < WLAG; ++q) acc[q] = fma(c, ring[(u - q) & (WLAG - 1)], acc[q]);
        }
      }
    }
    if (lag0 == 0 && T - 2 * n == 1) {
      const double v = (double)p[(size_t)n * t.rs];
      ss = fma(v - mu, v - mu, ss);
    }
  }
  // per column, across the workgroup's chains in chain order
  const bool writer = threadIdx.x < t.ct && tile * t.ct + (int)threadIdx.x < t.ncs;
  const int wcol = t.col0 + tile * t.ct + threadIdx.x;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    red[threadIdx.x] = q < WLAG ? acc[q < WLAG ? q : 0] : ss;
    __syncthreads();
    if (writer) {
      double s = 0.0;
      for (int k = 0; k < t.cg; ++k) s += red[k * t.ct + threadIdx.x];
      part[(((size_t)y * ncol + wcol) * NQ + q) * pstride + bc] = s;
    }
    __syncthreads();
  }
}

inline float key_float(uint32_t k)
{
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

}  // namespace

// the summary of x[T][nc][np], ly[T][nc] (device) on stream st.  force_lags > 0 (mcx_debug_rows_acov): every finite
// column takes windows until it holds force_lags lags instead of stopping where its Geyer loop does; the raw lag sums go to
// acov_out[ncol][force_lags] and the centred sums of squares to sumsq_out[ncol] (NaN for a column that is not finite),
// and cols / quantiles are not computed.  parts (SUMM_*) leaves out what a pass of mcx_samples_rank_summary does not need:
// without SUMM_OSTAT no order statistics (min, max and quantiles are not valid), without SUMM_ACOV no autocovariance
// windows (rhat, ess, ess_lag and mcse_mean are not valid); flags, mean and sd always are.
static int summary_device(hipStream_t st, Bufs B, const float *x, const float *ly, int nc, int np, int64_t T,
                          const double *probs, int nprobs, mcx_col_summary *cols, double *quantiles, int *nwin_out,
                          int force_lags = 0, double *acov_out = nullptr, double *sumsq_out = nullptr,
                          int parts = SUMM_OSTAT | SUMM_ACOV)
{
  const int ncol = np + 1;
  const int64_t n = T / 2, M = 2 * (int64_t)nc, N = T * (int64_t)nc;
  const TileSet tx = tiles_x(x, nc, np), tl = tiles_l(ly, nc, np);
  const size_t pstride = (size_t)std::max(tx.nbc, tl.nbc);
  const int KWMAX = 8;
  // device double scratch: hm[ncol][2][nc] | tot[ncol][nc] | colsum[3][ncol] | part[KWMAX][ncol][NQ][pstride] | win[KWMAX][ncol][NQ]
  const size_t o_hm = 0, o_tot = o_hm + (size_t)ncol * 2 * nc, o_cs = o_tot + (size_t)ncol * nc, o_part = o_cs + 3 * (size_t)ncol,
               o_win = o_part + (size_t)KWMAX * ncol * NQ * pstride, nd = o_win + (size_t)KWMAX * ncol * NQ;
  MCXCHK(B.d->alloc(nd));
  double *D = B.d->p;
  auto rows = [&](const double *in, size_t stride, int qper, size_t nrows, size_t lenx, size_t lenl, const double *center,
                  double cscale, double *out) -> int {
    hipLaunchKernelGGL(k_sum_rows, dim3((unsigned)nrows), dim3(SB), 0, st, in, stride, qper, ncol, np, lenx, lenl, center, cscale, out);
    HIPCHK(hipGetLastError());
    return MCX_OK;
  };

  // ---- 1. moments
  for (const TileSet *t : {&tx, &tl}) {
    hipLaunchKernelGGL(k_sum_moments, dim3((unsigned)(t->nbc * t->ntiles)), dim3(SB), 0, st, *t, nc, T, n, D + o_hm, D + o_tot);
    HIPCHK(hipGetLastError());
  }
  MCXCHK(rows(D + o_tot, nc, 1, ncol, nc, nc, nullptr, 0.0, D + o_cs));
  MCXCHK(rows(D + o_hm, 2 * (size_t)nc, 1, ncol, 2 * (size_t)nc, 2 * (size_t)nc, nullptr, 0.0, D + o_cs + ncol));
  MCXCHK(rows(D + o_hm, 2 * (size_t)nc, 1, ncol, 2 * (size_t)nc, 2 * (size_t)nc, D + o_cs + ncol, 1.0 / (double)M, D + o_cs + 2 * ncol));
  std::vector<double> cs(3 * (size_t)ncol);
  HIPCHK(hipMemcpyAsync(cs.data(), D + o_cs, cs.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));

  // ---- 2. order statistics: ranks 0, N-1, then lo, lo+1 of every probability
  const int nt = 2 + 2 * nprobs;
  std::vector<int64_t> rank(nt);
  rank[0] = 0;
  rank[1] = N - 1;
  for (int k = 0; k < nprobs; ++k) {
    const int64_t lo = (int64_t)std::floor((double)(N - 1) * probs[k]);
    rank[2 + 2 * k] = std::min(lo, N - 1);
    rank[3 + 2 * k] = std::min(lo + 1, N - 1);
  }
  std::vector<int64_t> rem((size_t)ncol * nt);      // rank within the current prefix
  std::vector<uint32_t> pre((size_t)ncol * nt, 0);  // key bits found so far
  for (int c = 0; c < ncol; ++c)
    for (int k = 0; k < nt; ++k) rem[(size_t)c * nt + k] = rank[k];
  std::vector<uint32_t> gp;
  std::vector<int> gc(ncol);
  std::vector<unsigned long long> hh;
  for (int pass = 0; pass < ((parts & SUMM_OSTAT) ? 4 : 0); ++pass) {
    const int shift = 32 - 8 * pass;
    // the distinct prefixes of each column's targets, sorted
    int G = 1;
    std::vector<std::vector<uint32_t>> lists(ncol);
    for (int c = 0; c < ncol; ++c) {
      auto &L = lists[c];
      for (int k = 0; k < nt; ++k) L.push_back(pass == 0 ? 0u : pre[(size_t)c * nt + k]);
      std::sort(L.begin(), L.end());
      L.erase(std::unique(L.begin(), L.end()), L.end());
      G = std::max(G, (int)L.size());
    }
    gp.assign((size_t)ncol * G, 0u);
    for (int c = 0; c < ncol; ++c) {
      std::copy(lists[c].begin(), lists[c].end(), gp.begin() + (size_t)c * G);
      gc[c] = (int)lists[c].size();
    }
    const size_t nh = (size_t)ncol * G * 256;
    MCXCHK(B.u->alloc(gp.size() + ncol));
    MCXCHK(B.h->alloc(nh));
    HIPCHK(hipMemcpyAsync(B.u->p, gp.data(), gp.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(B.u->p + gp.size(), gc.data(), (size_t)ncol * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(B.h->p, 0, nh * sizeof(unsigned long long), st));
    const unsigned chunks = (unsigned)((T + HIST_CHUNK - 1) / HIST_CHUNK);
    for (int g0 = 0; g0 < G; g0 += GMAX) {
      const int gn = std::min(GMAX, G - g0);
      for (const TileSet *t0 : {&tx, &tl}) {
        TileSet t = *t0;
        // keep the LDS counts within 32 KiB: narrower parameter tiles when a column has many target prefixes
        while (t.ct > 1 && (size_t)t.ct * gn * 256 * 4 > 32768) t.ct /= 2;
        t.cg = SB / t.ct; t.ntiles = (t.ncs + t.ct - 1) / t.ct; t.nbc = (nc + t.cg - 1) / t.cg;
        const size_t lds = (size_t)t.ct * gn * 257 * 4 + (size_t)t.ct * 4;
        hipLaunchKernelGGL(k_sum_hist, dim3((unsigned)(t.nbc * t.ntiles), chunks), dim3(SB), lds, st, t, nc, T, shift,
                           B.u->p, (const int *)(B.u->p + gp.size()), G, g0, gn, B.h->p);
        HIPCHK(hipGetLastError());
      }
    }
    hh.resize(nh);
    HIPCHK(hipMemcpyAsync(hh.data(), B.h->p, nh * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int c = 0; c < ncol; ++c)
      for (int k = 0; k < nt; ++k) {
        const uint32_t pf = pass == 0 ? 0u : pre[(size_t)c * nt + k];
        const int g = (int)(std::lower_bound(lists[c].begin(), lists[c].end(), pf) - lists[c].begin());
        const unsigned long long *h = hh.data() + ((size_t)c * G + g) * 256;
        int64_t r = rem[(size_t)c * nt + k];
        int b = 0;
        while (b < 255 && r >= (int64_t)h[b]) r -= (int64_t)h[b++];
        rem[(size_t)c * nt + k] = r;
        pre[(size_t)c * nt + k] = (pf << 8) | (uint32_t)b;
      }
  }

  // ---- 3. autocovariance windows, while some column's Geyer loop wants more lags
  std::vector<int> active(ncol), need(ncol, 0);
  std::vector<std::vector<double>> acov(ncol);  // sums over half-chains and steps of c_i c_{i+t}
  std::vector<double> ss(ncol, 0.0);
  for (int c = 0; c < ncol; ++c) active[c] = (parts & SUMM_ACOV) && std::isfinite(cs[c]) ? 1 : 0;
  const int nwin_max = (int)((n + WLAG - 1) / WLAG);
  int k0 = 0, KW = 2, nwin = 0;
  std::vector<float> os(nt);
  std::vector<double> win;
  for (;;) {
    bool any = false;
    for (int c = 0; c < ncol; ++c) any = any || active[c];
    if (!any || k0 >= nwin_max) break;
    KW = std::min({KW, KWMAX, nwin_max - k0});
    MCXCHK(B.u->alloc(ncol));
    HIPCHK(hipMemcpyAsync(B.u->p, active.data(), (size_t)ncol * 4, hipMemcpyHostToDevice, st));
    for (const TileSet *t : {&tx, &tl}) {
      hipLaunchKernelGGL(k_sum_acov, dim3((unsigned)(KW * t->ntiles * t->nbc)), dim3(SB), 0, st, *t, nc, T, n, k0, KW, ncol,
                         D + o_hm, D + o_cs, (double)N, (const int *)B.u->p, D + o_part, pstride);
      HIPCHK(hipGetLastError());
    }
    MCXCHK(rows(D + o_part, pstride, NQ, (size_t)KW * ncol * NQ, tx.nbc, tl.nbc, nullptr, 0.0, D + o_win));
    win.resize((size_t)KW * ncol * NQ);
    HIPCHK(hipMemcpyAsync(win.data(), D + o_win, win.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    nwin += KW;
    for (int c = 0; c < ncol; ++c) {
      if (!active[c]) continue;
      for (int y = 0; y < KW; ++y) {
        const double *w = win.data() + ((size_t)y * ncol + c) * NQ;
        for (int q = 0; q < WLAG && (int64_t)acov[c].size() < n; ++q) acov[c].push_back(w[q]);
        if (k0 + y == 0) ss[c] = w[WLAG];
      }
    }
    k0 += KW;
    KW *= 2;
    // which columns want more lags than they have
    for (int c = 0; c < ncol; ++c) {
      if (!active[c]) continue;
      if (force_lags > 0) {
        active[c] = (int64_t)acov[c].size() < force_lags ? 1 : 0;
        continue;
      }
      std::vector<double> a(acov[c].size());
      for (size_t t = 0; t < a.size(); ++t) a[t] = acov[c][t] / ((double)n * (double)M);
      mcx_col_summary tmp;
      std::fill(os.begin(), os.end(), 0.0f);
      const double mean = cs[c] / (double)N, vm = cs[2 * ncol + c] / (double)(M - 1), va = ss[c] / (double)(N - 1);
      MCXCHK(mcx_debug_summary_finish((int)n, (int)M, mean, va, vm, a.data(), (int)a.size(), os.data(), N, nullptr, 0, 0,
                                      &tmp, nullptr, &need[c]));
      active[c] = need[c] > 0 ? 1 : 0;
    }
  }
  if (nwin_out) *nwin_out = nwin;
  if (force_lags > 0) {
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    for (int c = 0; c < ncol; ++c) {
      const bool fin = std::isfinite(cs[c]);
      if (fin && (int64_t)acov[c].size() < force_lags)
        return fail(MCX_ERR_INVALID, "internal: column %d holds %d of %d lags", c, (int)acov[c].size(), force_lags);
      for (int t = 0; t < force_lags; ++t) acov_out[(size_t)c * force_lags + t] = fin ? acov[c][t] : qnan;
      sumsq_out[c] = fin ? ss[c] : qnan;
    }
    return MCX_OK;
  }

  // ---- 4. the host finish
  for (int c = 0; c < ncol; ++c) {
    for (int k = 0; k < nt; ++k) os[k] = key_float(pre[(size_t)c * nt + k]);
    const bool fin = std::isfinite(cs[c]);
    std::vector<double> a(acov[c].size());
    for (size_t t = 0; t < a.size(); ++t) a[t] = acov[c][t] / ((double)n * (double)M);
    const double mean = cs[c] / (double)N, vm = cs[2 * ncol + c] / (double)(M - 1), va = ss[c] / (double)(N - 1);
    int more = 0;
    MCXCHK(mcx_debug_summary_finish((int)n, (int)M, mean, va, vm, a.data(), (int)a.size(), os.data(), N, probs, nprobs,
                                    fin ? 0 : MCX_SUMMARY_NONFINITE, &cols[c], quantiles ? quantiles + (size_t)c * nprobs : nullptr,
                                    &more));
    if (more && (parts & SUMM_ACOV)) return fail(MCX_ERR_INVALID, "internal: column %d still wants %d lags", c, more);
  }
  return MCX_OK;
}

int summary_device_parts(hipStream_t st, DevBuf<double> *d, DevBuf<unsigned long long> *h, DevBuf<uint32_t> *u, const float *x,
                         const float *ly, int nc, int np, int64_t T, const double *probs, int nprobs, mcx_col_summary *cols,
                         double *quantiles, int parts)
{
  return summary_device(st, Bufs{d, h, u}, x, ly, nc, np, T, probs, nprobs, cols, quantiles, nullptr, 0, nullptr, nullptr, parts);
}

static int summary_args(int nsteps, const double *probs, int nprobs, const mcx_col_summary *cols, const double *quantiles)
{
  if (!cols) return fail(MCX_ERR_INVALID, "cols is NULL");
  if (nsteps < 4) return fail(MCX_ERR_INVALID, "a summary needs nsteps >= 4 (two half-chains of >= 2 steps), got %d", nsteps);
  if (nprobs < 0 || nprobs > 32) return fail(MCX_ERR_INVALID, "nprobs = %d: 0 to 32 probabilities", nprobs);
  if (nprobs > 0 && (!probs || !quantiles)) return fail(MCX_ERR_INVALID, "probs and quantiles are needed when nprobs > 0");
  for (int k = 0; k < nprobs; ++k)
    if (!(probs[k] >= 0.0 && probs[k] <= 1.0)) return fail(MCX_ERR_INVALID, "probs[%d] = %g is not in [0, 1]", k, probs[k]);
  return MCX_OK;
}

extern "C" int mcx_samples_summary(mcx_engine *e, int first_step, int nsteps, const double *probs, int nprobs,
                                   mcx_col_summary *cols, double *quantiles)
{
  if (!e) return fail(MCX_ERR_INVALID, "engine is NULL");
  MCXCHK(enter(e));
  MCXCHK(summary_args(nsteps, probs, nprobs, cols, quantiles));
  if (e->samp_steps == 0)
    return fail(MCX_ERR_INVALID, "the sample store is empty (no run yet, MCX_OPT_SAMPLES = 0, or a run into a sink)");
  if (first_step < 0 || (int64_t)first_step + nsteps > e->samp_steps)
    return fail(MCX_ERR_INVALID, "steps [%d,%lld) not in the sample store (%d steps)", first_step,
                (long long)first_step + nsteps, e->samp_steps);
  const size_t nc = (size_t)e->nchain, np = (size_t)e->nparam;
  return summary_device(e->stream, Bufs{&e->summ_d, &e->summ_h, &e->summ_u}, e->samp_x.p + (size_t)first_step * nc * np,
                        e->samp_ly.p + (size_t)first_step * nc, (int)nc, (int)np, nsteps, probs, nprobs, cols, quantiles,
                        nullptr);
}

extern "C" int mcx_rows_summary(const float *rows, int nsteps, int nc, int np, const double *probs, int nprobs,
                                mcx_col_summary *cols, double *quantiles)
{
  MCXCHK(summary_args(nsteps, probs, nprobs, cols, quantiles));
  return on_rows(rows, nsteps, nc, np, [&](hipStream_t st, Bufs B, const float *x, const float *ly) {
    return summary_device(st, B, x, ly, nc, np, nsteps, probs, nprobs, cols, quantiles, nullptr);
  });
}

extern "C" int mcx_debug_rows_acov(const float *rows, int nsteps, int nc, int np, int nlags, double *acov, double *sumsq)
{
  if (nsteps < 4) return fail(MCX_ERR_INVALID, "a summary needs nsteps >= 4 (two half-chains of >= 2 steps), got %d", nsteps);
  if (nlags < 1 || nlags > nsteps / 2 || !acov || !sumsq)
    return fail(MCX_ERR_INVALID, "nlags = %d: 1 to n = %d lags, acov and sumsq not NULL", nlags, nsteps / 2);
  return on_rows(rows, nsteps, nc, np, [&](hipStream_t st, Bufs B, const float *x, const float *ly) {
    return summary_device(st, B, x, ly, nc, np, nsteps, nullptr, 0, nullptr, nullptr, nullptr, nlags, acov, sumsq);
  });
}

extern "C" int mcx_debug_summary_windows(mcx_engine *e, int first_step, int nsteps, int *nwin)
{
  if (!e || !nwin) return fail(MCX_ERR_INVALID, "bad arguments");
  MCXCHK(enter(e));
  if (e->samp_steps == 0 || first_step < 0 || nsteps < 4 || (int64_t)first_step + nsteps > e->samp_steps)
    return fail(MCX_ERR_INVALID, "steps [%d,%lld) not in the sample store (%d steps)", first_step,
                (long long)first_step + nsteps, e->samp_steps);
  const size_t nc = (size_t)e->nchain, np = (size_t)e->nparam;
  std::vector<mcx_col_summary> cols(np + 1);
  return summary_device(e->stream, Bufs{&e->summ_d, &e->summ_h, &e->summ_u}, e->samp_x.p + (size_t)first_step * nc * np,
                        e->samp_ly.p + (size_t)first_step * nc, (int)nc, (int)np, nsteps, nullptr, 0, cols.data(), nullptr,
                        nwin);
}

// ---------------------------------------------------------------------------------------------------------------------
// host finish (no device calls): DESIGN.md "Sample-store summaries" restates every line
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int mcx_debug_summary_finish(int n, int M, double mean, double var_all, double var_means, const double *acov,
                                        int nlags, const float *ostat, long long N, const double *probs, int nprobs,
                                        int flags, mcx_col_summary *col, double *quantiles, int *need_lags)
{
  if (!col || !need_lags || !ostat || n < 2 || M < 2 || N < 1 || nlags < 0 || (nlags > 0 && !acov) ||
      (nprobs > 0 && (!probs || !quantiles)))
    return fail(MCX_ERR_INVALID, "bad arguments");
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  *need_lags = 0;
  col->flags = flags;
  col->min = ostat[0];
  col->max = ostat[1];
  const bool has_nan = std::isnan(ostat[1]);
  if (has_nan) col->min = ostat[1];
  for (int k = 0; k < nprobs; ++k) {
    const double h = (double)(N - 1) * probs[k], lo = std::floor(h), g = h - lo;
    const double a = ostat[2 + 2 * k], b = ostat[3 + 2 * k];
    quantiles[k] = has_nan ? qnan : (g == 0.0 || a == b) ? a : a + g * (b - a);
  }
  col->ess_lag = 0;
  if (flags & MCX_SUMMARY_NONFINITE) {
    col->mean = col->sd = col->rhat = col->ess = col->mcse_mean = qnan;
    return MCX_OK;
  }
  col->mean = mean;
  col->sd = std::sqrt(var_all);
  if (nlags < 2) {
    *need_lags = 2;
    return MCX_OK;
  }
  const double W = acov[0] * n / (n - 1.0), var_plus = acov[0] + var_means;
  col->rhat = std::sqrt(var_plus / W);
  if (!(W > 0.0)) {  // constant within every half-chain
    col->rhat = col->ess = col->mcse_mean = qnan;
    return MCX_OK;
  }
  auto R = [&](int64_t t) { return 1.0 - (W - acov[t]) / var_plus; };
  std::vector<double> rho((size_t)n + 2, 0.0);
  int64_t t = 0;
  double even = 1.0, odd = R(1);
  rho[0] = even;
  rho[1] = odd;
  while (t < (int64_t)n - 5 && !std::isnan(even + odd) && even + odd > 0.0) {
    if (t + 3 >= nlags) {
      *need_lags = (int)(t + 4);
      return MCX_OK;
    }
    t += 2;
    even = R(t);
    odd = R(t + 1);
    if (even + odd >= 0.0) {
      rho[t] = even;
      rho[t + 1] = odd;
    }
  }
  const int64_t max_t = t;
  if (even > 0.0) rho[max_t] = even;
  for (t = 0; t <= max_t - 4;) {  // Geyer's initial monotone sequence
    t += 2;
    if (rho[t] + rho[t + 1] > rho[t - 2] + rho[t - 1]) {
      rho[t] = (rho[t - 2] + rho[t - 1]) / 2.0;
      rho[t + 1] = rho[t];
    }
  }
  double sum = 0.0;
  for (t = 0; t < max_t; ++t) sum += rho[t];
  const double mn = (double)M * (double)n;
  const double tau = std::max(-1.0 + 2.0 * sum + rho[max_t], 1.0 / std::log10(mn));
  col->ess = mn / tau;
  col->ess_lag = (int)max_t;
  col->mcse_mean = col->sd / std::sqrt(col->ess);
  return MCX_OK;
}
