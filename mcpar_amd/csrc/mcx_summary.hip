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

// ---------------------------------------------------------------------------------------------------------------------
// the host pieces of the radix select (no HIP in them)
// ---------------------------------------------------------------------------------------------------------------------
// the target ranks of a column of N values: 0, N - 1, then lo, lo + 1 of every probability
std::vector<int64_t> target_ranks(int64_t N, const double *probs, int nprobs)
{
  std::vector<int64_t> rank(2 + 2 * (size_t)nprobs);
  rank[0] = 0;
  rank[1] = N - 1;
  for (int k = 0; k < nprobs; ++k) {
    const int64_t lo = (int64_t)std::floor((double)(N - 1) * probs[k]);
    rank[2 + 2 * k] = std::min(lo, N - 1);
    rank[3 + 2 * k] = std::min(lo + 1, N - 1);
  }
  return rank;
}

// the distinct prefixes of each column's nt targets, sorted; returns the longest list's length (1 at least)
int prefix_lists(const std::vector<uint32_t> &pre, int ncol, int nt, std::vector<std::vector<uint32_t>> &lists)
{
  int G = 1;
  lists.assign(ncol, {});
  for (int c = 0; c < ncol; ++c) {
    auto &L = lists[c];
    L.assign(pre.begin() + (size_t)c * nt, pre.begin() + (size_t)(c + 1) * nt);
    std::sort(L.begin(), L.end());
    L.erase(std::unique(L.begin(), L.end()), L.end());
    G = std::max(G, (int)L.size());
  }
  return G;
}

// one digit of one target: the digit b whose bucket of hist[256] holds rank rem of the values under the prefix, and the
// rank within that bucket.  The walk stops at 255 whatever the counts say: a rank past the end lands in the last bucket
int select_step(const unsigned long long *hist, int64_t rem, int64_t *rem_out)
{
  int b = 0;
  while (b < 255 && rem >= (int64_t)hist[b]) rem -= (int64_t)hist[b++];
  *rem_out = rem;
  return b;
}

// a tile set for a histogram launch of gn prefixes per column: the LDS counts stay within 32 KiB, by narrower parameter
// tiles when a column has many target prefixes
TileSet hist_tiles(TileSet t, int gn, int nc)
{
  while (t.ct > 1 && (size_t)t.ct * gn * 256 * 4 > 32768) t.ct /= 2;
  t.cg = SB / t.ct; t.ntiles = (t.ncs + t.ct - 1) / t.ct; t.nbc = (nc + t.cg - 1) / t.cg;
  return t;
}

// ---------------------------------------------------------------------------------------------------------------------
// one summary of a view: the context its phases share
// ---------------------------------------------------------------------------------------------------------------------
constexpr int KWMAX = 8;  // lag windows per k_sum_acov launch

struct SummaryPass {
  hipStream_t st;
  Bufs B;
  const StoreView &v;
  const double *probs;
  int nprobs, nt;  // nt = 2 + 2 nprobs order statistics per column: min, max, the two neighbours of every quantile
  // device double scratch: hm[ncol][2][nc] | tot[ncol][nc] | colsum[3][ncol] | part[KWMAX][ncol][NQ][pstride] | win[KWMAX][ncol][NQ]
  size_t pstride, o_hm, o_tot, o_cs, o_part, o_win, nd;
  double *D = nullptr;
  // host copies that later phases read
  std::vector<double> cs;                  // moments_pass: [3][ncol] sums of the values, of the half-chain means, of their centred squares
  std::vector<uint32_t> pre;               // order_stats_pass: [ncol][nt] keys of the order statistics (0 until it has run)
  std::vector<std::vector<double>> acov;   // acov_windows: per column, sums over half-chains and steps of c_i c_{i+t}
  std::vector<double> ss;                  // acov_windows: per column, the centred sum of squares
  int nwin = 0;                            // acov_windows: lag windows computed

  SummaryPass(hipStream_t st_, Bufs B_, const StoreView &v_, const double *probs_, int nprobs_)
      : st(st_), B(B_), v(v_), probs(probs_), nprobs(nprobs_), nt(2 + 2 * nprobs_), pstride((size_t)std::max(v_.tx.nbc, v_.tl.nbc)),
        pre((size_t)v_.ncol * nt, 0u), acov(v_.ncol), ss(v_.ncol, 0.0)
  {
    const size_t ncol = v.ncol, nc = v.nc;
    o_hm = 0; o_tot = o_hm + ncol * 2 * nc; o_cs = o_tot + ncol * nc; o_part = o_cs + 3 * ncol;
    o_win = o_part + (size_t)KWMAX * ncol * NQ * pstride; nd = o_win + (size_t)KWMAX * ncol * NQ;
  }
  int rows(const double *in, size_t stride, int qper, size_t nrows, size_t lenx, size_t lenl, const double *center, double cscale,
           double *out) const
  {
    hipLaunchKernelGGL(k_sum_rows, dim3((unsigned)nrows), dim3(SB), 0, st, in, stride, qper, v.ncol, v.np, lenx, lenl, center, cscale, out);
    HIPCHK(hipGetLastError());
    return MCX_OK;
  }
};

// ---- 1. moments -> cs
int moments_pass(SummaryPass &p)
{
  const StoreView &v = p.v;
  const int ncol = v.ncol;
  const size_t nc2 = 2 * (size_t)v.nc;
  MCXCHK(p.B.d->alloc(p.nd));
  double *D = p.D = p.B.d->p;
  MCXCHK(launch_moments(p.st, v, D + p.o_hm, D + p.o_tot, D + p.o_cs));
  MCXCHK(p.rows(D + p.o_hm, nc2, 1, ncol, nc2, nc2, nullptr, 0.0, D + p.o_cs + ncol));
  MCXCHK(p.rows(D + p.o_hm, nc2, 1, ncol, nc2, nc2, D + p.o_cs + ncol, 1.0 / (double)v.M, D + p.o_cs + 2 * ncol));
  p.cs.resize(3 * (size_t)ncol);
  HIPCHK(hipMemcpyAsync(p.cs.data(), D + p.o_cs, p.cs.size() * sizeof(double), hipMemcpyDeviceToHost, p.st));
  HIPCHK(hipStreamSynchronize(p.st));
  return MCX_OK;
}

// ---- 2. order statistics -> pre: a radix select of every column's target ranks, 8 bits per pass from the top
int order_stats_pass(SummaryPass &p)
{
  const StoreView &v = p.v;
  const int ncol = v.ncol, nt = p.nt;
  const std::vector<int64_t> rank = target_ranks(v.N, p.probs, p.nprobs);
  std::vector<int64_t> rem((size_t)ncol * nt);  // rank within the current prefix
  for (int c = 0; c < ncol; ++c) std::copy(rank.begin(), rank.end(), rem.begin() + (size_t)c * nt);
  std::vector<std::vector<uint32_t>> lists;
  std::vector<uint32_t> gp;
  std::vector<int> gc(ncol);
  std::vector<unsigned long long> hh;
  const unsigned chunks = (unsigned)((v.T + HIST_CHUNK - 1) / HIST_CHUNK);
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 32 - 8 * pass;
    const int G = prefix_lists(p.pre, ncol, nt, lists);
    gp.assign((size_t)ncol * G, 0u);
    for (int c = 0; c < ncol; ++c) {
      std::copy(lists[c].begin(), lists[c].end(), gp.begin() + (size_t)c * G);
      gc[c] = (int)lists[c].size();
    }
    const size_t nh = (size_t)ncol * G * 256;
    MCXCHK(p.B.u->alloc(gp.size() + ncol));
    MCXCHK(p.B.h->alloc(nh));
    HIPCHK(hipMemcpyAsync(p.B.u->p, gp.data(), gp.size() * 4, hipMemcpyHostToDevice, p.st));
    HIPCHK(hipMemcpyAsync(p.B.u->p + gp.size(), gc.data(), (size_t)ncol * 4, hipMemcpyHostToDevice, p.st));
    HIPCHK(hipMemsetAsync(p.B.h->p, 0, nh * sizeof(unsigned long long), p.st));
    for (int g0 = 0; g0 < G; g0 += GMAX) {
      const int gn = std::min(GMAX, G - g0);
      for (const TileSet *t0 : {&v.tx, &v.tl}) {
        const TileSet t = hist_tiles(*t0, gn, v.nc);
        const size_t lds = (size_t)t.ct * gn * 257 * 4 + (size_t)t.ct * 4;
        hipLaunchKernelGGL(k_sum_hist, dim3((unsigned)(t.nbc * t.ntiles), chunks), dim3(SB), lds, p.st, t, v.nc, v.T, shift,
                           p.B.u->p, (const int *)(p.B.u->p + gp.size()), G, g0, gn, p.B.h->p);
        HIPCHK(hipGetLastError());
      }
    }
    hh.resize(nh);
    HIPCHK(hipMemcpyAsync(hh.data(), p.B.h->p, nh * sizeof(unsigned long long), hipMemcpyDeviceToHost, p.st));
    HIPCHK(hipStreamSynchronize(p.st));
    for (int c = 0; c < ncol; ++c)
      for (int k = 0; k < nt; ++k) {
        const size_t i = (size_t)c * nt + k;
        const int g = (int)(std::lower_bound(lists[c].begin(), lists[c].end(), p.pre[i]) - lists[c].begin());
        const int b = select_step(hh.data() + ((size_t)c * G + g) * 256, rem[i], &rem[i]);
        p.pre[i] = (p.pre[i] << 8) | (uint32_t)b;
      }
  }
  return MCX_OK;
}

// The one place that turns column c's sums into mcx_debug_summary_finish's arguments.  os: the column's order statistics;
// need: how many lags its Geyer loop wants where it has too few (0: it is done)
int finish_column(const SummaryPass &p, int c, const float *os, int nprobs, mcx_col_summary *col, double *quantiles, int *need)
{
  const StoreView &v = p.v;
  std::vector<double> a(p.acov[c].size());
  for (size_t t = 0; t < a.size(); ++t) a[t] = p.acov[c][t] / ((double)v.n * (double)v.M);
  const double mean = p.cs[c] / (double)v.N, vm = p.cs[2 * v.ncol + c] / (double)(v.M - 1), va = p.ss[c] / (double)(v.N - 1);
  // (summary_thresholds on a range of fewer than four steps, for a clip, section 14: n < 2.  Without lags the finish reads
  // its n nowhere -- mean, sd, the order statistics and the quantiles -- and every caller with lags has nsteps >= 4)
  const int n = (int)std::max<int64_t>(v.n, 2);
  return mcx_debug_summary_finish(n, (int)v.M, mean, va, vm, a.data(), (int)a.size(), os, v.N, p.probs, nprobs,
                                  std::isfinite(p.cs[c]) ? 0 : MCX_SUMMARY_NONFINITE, col, quantiles, need);
}

// the normal rule of acov_windows: a column wants the lags its Geyer loop asks for
int geyer_wants(const SummaryPass &p, int c, int *more)
{
  const float os[2] = {0.0f, 0.0f};
  mcx_col_summary tmp;
  return finish_column(p, c, os, 0, &tmp, nullptr, more);
}

// ---- 3. autocovariance windows -> acov, ss, nwin: 2, 4, 8, ... windows a launch (KWMAX and the half-chain's length cap
// them) for the finite columns, while wants(p, c, &more) says that some column wants more lags than it holds.  kw0: the
// windows of the first launch (summary_spread wants window 0 alone: the centred sum of squares)
template <class W> int acov_windows(SummaryPass &p, W wants, int kw0 = 2)
{
  const StoreView &v = p.v;
  const int ncol = v.ncol;
  double *D = p.D;
  std::vector<int> active(ncol);
  for (int c = 0; c < ncol; ++c) active[c] = std::isfinite(p.cs[c]) ? 1 : 0;
  const int nwin_max = std::max(1, (int)((v.n + WLAG - 1) / WLAG));  // (window 0 also where a range of < 2 steps has no half-chain)
  int k0 = 0, KW = kw0;
  std::vector<double> win;
  while (k0 < nwin_max && std::count(active.begin(), active.end(), 1) > 0) {
    KW = std::min({KW, KWMAX, nwin_max - k0});
    MCXCHK(p.B.u->alloc(ncol));
    HIPCHK(hipMemcpyAsync(p.B.u->p, active.data(), (size_t)ncol * 4, hipMemcpyHostToDevice, p.st));
    for (const TileSet *t : {&v.tx, &v.tl}) {
      hipLaunchKernelGGL(k_sum_acov, dim3((unsigned)(KW * t->ntiles * t->nbc)), dim3(SB), 0, p.st, *t, v.nc, v.T, v.n, k0, KW, ncol,
                         D + p.o_hm, D + p.o_cs, (double)v.N, (const int *)p.B.u->p, D + p.o_part, p.pstride);
      HIPCHK(hipGetLastError());
    }
    MCXCHK(p.rows(D + p.o_part, p.pstride, NQ, (size_t)KW * ncol * NQ, v.tx.nbc, v.tl.nbc, nullptr, 0.0, D + p.o_win));
    win.resize((size_t)KW * ncol * NQ);
    HIPCHK(hipMemcpyAsync(win.data(), D + p.o_win, win.size() * sizeof(double), hipMemcpyDeviceToHost, p.st));
    HIPCHK(hipStreamSynchronize(p.st));
    p.nwin += KW;
    for (int c = 0; c < ncol; ++c) {
      if (!active[c]) continue;
      for (int y = 0; y < KW; ++y) {
        const double *w = win.data() + ((size_t)y * ncol + c) * NQ;
        for (int q = 0; q < WLAG && (int64_t)p.acov[c].size() < v.n; ++q) p.acov[c].push_back(w[q]);
        if (k0 + y == 0) p.ss[c] = w[WLAG];
      }
      int more = 0;
      MCXCHK(wants(p, c, &more));
      active[c] = more > 0 ? 1 : 0;
    }
    k0 += KW;
    KW *= 2;
  }
  for (int c = 0; c < ncol; ++c)
    if (active[c]) return fail(MCX_ERR_INVALID, "internal: column %d holds %d lags and still wants more", c, (int)p.acov[c].size());
  return MCX_OK;
}

// ---- 4. the host finish -> cols[ncol], quantiles[ncol][nprobs] (NULL when nprobs = 0)
int finish_columns(const SummaryPass &p, mcx_col_summary *cols, double *quantiles)
{
  std::vector<float> os(p.nt);
  for (int c = 0; c < p.v.ncol; ++c) {
    for (int k = 0; k < p.nt; ++k) os[k] = key_float(p.pre[(size_t)c * p.nt + k]);
    int more = 0;  // (acov_windows has seen to it where it ran; a pass without it reads no rhat or ess)
    MCXCHK(finish_column(p, c, os.data(), p.nprobs, &cols[c], quantiles ? quantiles + (size_t)c * p.nprobs : nullptr, &more));
  }
  return MCX_OK;
}

// mcx_samples_summary / mcx_rows_summary: every phase
int summary_full(SummaryPass &p, mcx_col_summary *cols, double *quantiles)
{
  MCXCHK(moments_pass(p));
  MCXCHK(order_stats_pass(p));
  MCXCHK(acov_windows(p, geyer_wants));
  return finish_columns(p, cols, quantiles);
}

int summary_args(int nsteps, const double *probs, int nprobs, const mcx_col_summary *cols, const double *quantiles)
{
  if (!cols) return fail(MCX_ERR_INVALID, "cols is NULL");
  MCXCHK(half_chain_args(nsteps));
  if (nprobs < 0 || nprobs > 32) return fail(MCX_ERR_INVALID, "nprobs = %d: 0 to 32 probabilities", nprobs);
  if (nprobs > 0 && (!probs || !quantiles)) return fail(MCX_ERR_INVALID, "probs and quantiles are needed when nprobs > 0");
  for (int k = 0; k < nprobs; ++k)
    if (!(probs[k] >= 0.0 && probs[k] <= 1.0)) return fail(MCX_ERR_INVALID, "probs[%d] = %g is not in [0, 1]", k, probs[k]);
  return MCX_OK;
}

}  // namespace

int summary_thresholds(hipStream_t st, Bufs B, const StoreSpan &s, const double *probs, int nprobs, mcx_col_summary *cols,
                       double *quantiles)
{
  const StoreView v(s);
  SummaryPass p(st, B, v, probs, nprobs);
  MCXCHK(moments_pass(p));
  MCXCHK(order_stats_pass(p));
  return finish_columns(p, cols, quantiles);
}

int summary_mixing(hipStream_t st, Bufs B, const StoreSpan &s, mcx_col_summary *cols)
{
  const StoreView v(s);
  SummaryPass p(st, B, v, nullptr, 0);
  MCXCHK(moments_pass(p));
  MCXCHK(acov_windows(p, geyer_wants));
  return finish_columns(p, cols, nullptr);
}

int summary_spread(hipStream_t st, Bufs B, const StoreSpan &s, const double *probs, int nprobs, mcx_col_summary *cols, double *quantiles)
{
  const StoreView v(s);
  SummaryPass p(st, B, v, probs, nprobs);
  MCXCHK(moments_pass(p));
  MCXCHK(order_stats_pass(p));
  MCXCHK(acov_windows(
      p,
      [](const SummaryPass &, int, int *more) {
        *more = 0;
        return MCX_OK;
      },
      1));
  // the finish without lags reads its n and M nowhere: mean, sd, the order statistics and the quantiles, by finish_column's
  // expressions, for any range of N >= 2 values
  std::vector<float> os(p.nt);
  for (int c = 0; c < v.ncol; ++c) {
    for (int k = 0; k < p.nt; ++k) os[k] = key_float(p.pre[(size_t)c * p.nt + k]);
    int more = 0;
    MCXCHK(mcx_debug_summary_finish(2, 2, p.cs[c] / (double)v.N, p.ss[c] / (double)(v.N - 1), 0.0, nullptr, 0, os.data(), v.N, probs, nprobs,
                                    std::isfinite(p.cs[c]) ? 0 : MCX_SUMMARY_NONFINITE, &cols[c], quantiles + (size_t)c * nprobs, &more));
  }
  return MCX_OK;
}

int summary_span(hipStream_t st, Bufs B, const StoreSpan &s, const double *probs, int nprobs, mcx_col_summary *cols, double *quantiles)
{
  MCXCHK(summary_args((int)s.T, probs, nprobs, cols, quantiles));
  const StoreView v(s);
  SummaryPass p(st, B, v, probs, nprobs);
  return summary_full(p, cols, quantiles);
}

extern "C" int mcx_samples_summary(mcx_engine *e, int first_step, int nsteps, const double *probs, int nprobs,
                                   mcx_col_summary *cols, double *quantiles)
{
  return on_store(
      e, first_step, nsteps, [&] { return summary_args(nsteps, probs, nprobs, cols, quantiles); },
      [&](hipStream_t st, Bufs B, const StoreView &v) {
        SummaryPass p(st, B, v, probs, nprobs);
        return summary_full(p, cols, quantiles);
      });
}

extern "C" int mcx_rows_summary(const float *rows, int nsteps, int nc, int np, const double *probs, int nprobs,
                                mcx_col_summary *cols, double *quantiles)
{
  MCXCHK(summary_args(nsteps, probs, nprobs, cols, quantiles));
  return on_rows(rows, nsteps, nc, np, [&](hipStream_t st, Bufs B, const StoreView &v) {
    SummaryPass p(st, B, v, probs, nprobs);
    return summary_full(p, cols, quantiles);
  });
}

// the raw sums of acov_windows, every finite column taking windows until it holds nlags lags (NaN for a column that is not)
extern "C" int mcx_debug_rows_acov(const float *rows, int nsteps, int nc, int np, int nlags, double *acov, double *sumsq)
{
  MCXCHK(half_chain_args(nsteps));
  if (nlags < 1 || nlags > nsteps / 2 || !acov || !sumsq)
    return fail(MCX_ERR_INVALID, "nlags = %d: 1 to n = %d lags, acov and sumsq not NULL", nlags, nsteps / 2);
  return on_rows(rows, nsteps, nc, np, [&](hipStream_t st, Bufs B, const StoreView &v) -> int {
    SummaryPass p(st, B, v, nullptr, 0);
    MCXCHK(moments_pass(p));
    MCXCHK(acov_windows(p, [&](const SummaryPass &q, int c, int *more) {
      *more = (int64_t)q.acov[c].size() < nlags ? 1 : 0;
      return MCX_OK;
    }));
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    for (int c = 0; c < v.ncol; ++c) {
      const bool fin = std::isfinite(p.cs[c]);
      for (int t = 0; t < nlags; ++t) acov[(size_t)c * nlags + t] = fin ? p.acov[c][t] : qnan;
      sumsq[c] = fin ? p.ss[c] : qnan;
    }
    return MCX_OK;
  });
}

extern "C" int mcx_debug_summary_windows(mcx_engine *e, int first_step, int nsteps, int *nwin)
{
  return on_store(
      e, first_step, nsteps,
      [&] {
        if (!nwin) return fail(MCX_ERR_INVALID, "nwin is NULL");
        return half_chain_args(nsteps);
      },
      [&](hipStream_t st, Bufs B, const StoreView &v) -> int {
        std::vector<mcx_col_summary> cols(v.ncol);
        SummaryPass p(st, B, v, nullptr, 0);
        MCXCHK(summary_full(p, cols.data(), nullptr));
        *nwin = p.nwin;
        return MCX_OK;
      });
}

extern "C" int mcx_debug_select_step(const unsigned long long hist[256], long long rem, int *digit, long long *rem_out)
{
  if (!hist || !digit || !rem_out || rem < 0) return fail(MCX_ERR_INVALID, "bad arguments");
  int64_t r = 0;
  *digit = select_step(hist, rem, &r);
  *rem_out = r;
  return MCX_OK;
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
