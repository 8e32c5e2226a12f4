// mcx_evidence.hip -- mcx_*_evidence: log Z of the sampled function by bridge sampling, with its error.
// The rows of a view carry log L; a proposal g (a mixture of up to 8 Gaussians, fitted by section 10 or the caller's) is drawn
// from and evaluated on both sides, and the iterative estimator of Meng & Wong runs on the two arrays of l = log L - log g.
//   1. covariance_span          section 10 on the first fit_steps steps -> the fitted proposal (host: mcx_evidence_host.hpp factors it)
//   2. k_ev_draw                a workgroup takes DR draws: the component from one uniform, the engine's normals of stream 8 into
//                               LDS, x~ = c + C z per coordinate in fp64, l ascending, no fused multiply-add -> floats
//   3. eval_device              log L of the draws by the likelihood's own device code (the callback for MCX_VL_HOST)
//   4. k_ev_logg x 2            the sweep, once over the rows and once over the draws: a tile of R rows in LDS, and per component its
//                               centre and W_k in chunks of rows beside it; 256 / R lanes per row share the outputs z_i = (W_k u)_i,
//                               Q_k and the log-sum-exp per row -> l (fp64) per row; the lowest row with a non-finite l through
//                               an integer atomicMin
//   5. summary_mixing           section 9 on the rows for neff, and later on the one-column store of f2 for ess_f2
//   6. k_ev_terms + k_sum_rows  one pass over l1 and l2 for a given r (or log Z): per-workgroup partial sums -> slabs -> the
//                               fixed-order reducer; the host loop reads two doubles per pass
// No float atomics, no kernel waits on another workgroup.  The call's buffers are its own and every one is written before it
// is read; the summary's and the covariance's scratch is the view's (Bufs).
#include "mcx_store.hpp"

#include "mcx_evidence_host.hpp"

#include <limits>

namespace {

namespace H = mcx_evidence_host;

constexpr int EV_MAX_WG = 4096;      // workgroups of a sweep: each takes tiles blockIdx.x, blockIdx.x + gridDim.x, ...
constexpr int TM_MAX_WG = 1024;      // workgroups of a terms pass per side
constexpr int64_t TM_CHUNK = 1024;   // values per workgroup of a terms pass at the least
constexpr uint32_t NO_ROW = 0xffffffffu;
enum { ET_FIT = 0, ET_DRAW, ET_LIK, ET_SWEEP_ROWS, ET_SWEEP_DRAWS, ET_ESS, ET_BRIDGE, ET_CALL, ET_N };
enum { LG_PLAIN = 0, LG_ROWS = 1, LG_DRAWS = 2 };  // what k_ev_logg writes
enum { TM_STATS = 0, TM_BRIDGE, TM_ERR1, TM_ERR2, TM_BYPRODUCTS };

// the proposal on the device: c[K][np] | W[K][np][np] | Cf[K][np][np] | lc[K], and the cumulative weights by value
struct PropDev {
  const double *c, *W, *Cf, *lc;
  int K;
  double cum[H::MAX_K];
};

constexpr int W_LDS = 2048;          // doubles of LDS for a chunk of rows of W_k
inline int tile_rows(int np) { return np <= 128 ? 64 : 32; }
// rows of W_k a chunk holds: all np when they fit, else as many as fit, a multiple of the SB / R lanes of a row
inline int w_chunk_rows(int np)
{
  const int S = SB / tile_rows(np), fit = W_LDS / np;
  return fit >= np ? np : std::max(S, fit / S * S);
}
// q[SB] | tk[MAX_K][64] | wl[W_LDS] | cl[256] doubles, nf[SB] ints, xs[R][np | 1] floats
inline size_t logg_lds(int np)
{
  return ((size_t)SB + (size_t)H::MAX_K * 64 + W_LDS + 256) * 8 + (size_t)SB * 4 + (size_t)tile_rows(np) * (size_t)(np | 1) * 4;
}
inline int64_t sweep_tiles_of(int64_t N, int np) { return (N + tile_rows(np) - 1) / tile_rows(np); }
inline unsigned sweep_wg(int64_t N, int np) { return (unsigned)std::min<int64_t>(EV_MAX_WG, std::max<int64_t>(1, sweep_tiles_of(N, np))); }
inline int draw_rows(int np) { return std::max(16, SB / np); }
inline int draw_zstride(int np) { return (np + 3) / 4 * 4 + 1; }
inline size_t draw_lds(int np) { return (size_t)draw_rows(np) * draw_zstride(np) * 4 + (size_t)draw_rows(np) * 4; }
inline unsigned draw_wg(int64_t n2, int np) { return (unsigned)((n2 + draw_rows(np) - 1) / draw_rows(np)); }
inline unsigned terms_wg(int64_t n) { return (unsigned)std::min<int64_t>(TM_MAX_WG, std::max<int64_t>(1, (n + TM_CHUNK - 1) / TM_CHUNK)); }

// 4. grid = sweep_wg.  x[N][np] floats; out[N]: log g (LG_PLAIN), ly - log g (LG_ROWS), or the same with ly = -inf or NaN giving
// -inf (LG_DRAWS: a draw with L = 0).  *bad = the lowest row whose l is not finite (LG_ROWS), is +inf or NaN (LG_DRAWS).
// A tile of R rows lies in LDS as floats; component by component the centre and a chunk of CH rows of W_k follow it there, so that
// every operand of z_i = sum_{l <= i} W_il (x_l - c_l) is an LDS read, W and c the same address for all lanes of a row slice (a
// broadcast).  Lane (r, s) of S = 256 / R takes the outputs i = i0 + s, i0 + s + S, ... of a chunk for row r; the slices' sums of
// z_i^2 meet in LDS in the order of s.
__global__ void __launch_bounds__(SB) k_ev_logg(const float *x, const float *ly, int64_t N, int np, int R, int CH, PropDev p, int what,
                                                double *out, uint32_t *bad)
{
  extern __shared__ double ev_lds[];
  double *q = ev_lds, *tk = q + SB, *wl = tk + H::MAX_K * 64, *cl = wl + W_LDS;
  int *nf = (int *)(cl + 256);
  float *xs = (float *)(nf + SB);
  const int tid = (int)threadIdx.x, S = SB / R, r = tid % R, s = tid / R, stride = np | 1, K = p.K;
  const int64_t ntiles = (N + R - 1) / R;
  const double pinf = __longlong_as_double(0x7ff0000000000000ll), qnan = __longlong_as_double(0x7ff8000000000000ll);
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * R;
    const int nrows = (int)min((int64_t)R, N - row0);
    __syncthreads();  // (the last tile's reads are over)
    const float *src = x + (size_t)row0 * np;
    for (int e = tid; e < nrows * np; e += SB) {
      const int rr = e / np, l = e - rr * np;
      xs[rr * stride + l] = src[e];
    }
    const float *xr = xs + r * stride;
    for (int k = 0; k < K; ++k) {
      __syncthreads();  // (the tile is staged; the last component's centre, chunk and sums have been read)
      for (int l = tid; l < np; l += SB) cl[l] = p.c[(size_t)k * np + l];
      const double *Wk = p.W + (size_t)k * np * np;
      double Q = 0.0;
      int nonfin = 0;
      for (int i0 = 0; i0 < np; i0 += CH) {
        const int nch = min(CH, np - i0);
        if (i0 > 0) __syncthreads();  // (the last chunk has been read)
        for (int e = tid; e < nch * np; e += SB) wl[e] = Wk[(size_t)i0 * np + e];
        __syncthreads();
        if (r < nrows)
          for (int i = i0 + s; i < i0 + nch; i += S) {
            const float xi = xr[i];
            nonfin |= (xi - xi != 0.0f) ? 1 : 0;  // inf or NaN
            const double *wi = wl + (i - i0) * np;
            double z = 0.0;
            for (int l = 0; l <= i; ++l) z += wi[l] * ((double)xr[l] - cl[l]);
            Q += z * z;
          }
      }
      q[s * R + r] = Q;
      if (k == 0) nf[s * R + r] = nonfin;
      __syncthreads();
      if (tid < nrows) {  // s = 0, r = tid: the row's sum over the slices in their order
        double a = 0.0;
        for (int ss = 0; ss < S; ++ss) a += q[ss * R + tid];
        tk[k * 64 + tid] = p.lc[k] - 0.5 * a;
      }
    }
    if (tid < nrows) {  // (tk[.][tid] and, behind the barriers above, nf are this lane's to read)
      int badrow = 0;
      for (int ss = 0; ss < S; ++ss) badrow |= nf[ss * R + tid];
      double mx = -pinf, se = 0.0;
      for (int k = 0; k < K; ++k) mx = fmax(mx, tk[k * 64 + tid]);
      for (int k = 0; k < K; ++k) se += exp(tk[k * 64 + tid] - mx);
      const double lg = badrow ? qnan : mx + log(se);
      const int64_t i = row0 + tid;
      double l = lg;
      if (what != LG_PLAIN) {
        const double v = (double)ly[i];
        if (what == LG_DRAWS && (v != v || v == -pinf)) l = -pinf;
        else {
          l = v - lg;
          if (l - l != 0.0) atomicMin(bad, (uint32_t)i);
        }
      }
      out[i] = l;
    }
  }
}

// 2. grid = draw_wg.  Draws base .. base + DR - 1 of a workgroup: xo[n2][np], comp[n2].  LDS: zs[DR][zstride] floats | cs[DR] ints
__global__ void __launch_bounds__(SB) k_ev_draw(PropDev p, int np, uint32_t seed, int64_t n2, int DR, int zstride, float *xo, int *comp)
{
  extern __shared__ double ev_lds[];
  float *zs = (float *)ev_lds;
  int *cs = (int *)(zs + (size_t)DR * zstride);
  const int tid = (int)threadIdx.x, nb = (np + 3) / 4;
  const int64_t base = (int64_t)blockIdx.x * DR;
  const int cnt = (int)min((int64_t)DR, n2 - base);
  for (int e = tid; e < cnt * nb; e += SB) {
    const int d = e / nb, b = e - d * nb;
    float z[4];
    normal4_from_words(philox4x32_10((uint32_t)(base + d), (uint32_t)b, 0u, 0u, seed, H::ST_EVIDENCE), z);
#pragma unroll
    for (int c = 0; c < 4; ++c) zs[d * zstride + 4 * b + c] = z[c];
  }
  for (int d = tid; d < cnt; d += SB) {
    const u32x4 w = philox4x32_10((uint32_t)(base + d), 0u, 1u, 0u, seed, H::ST_EVIDENCE);
    const int k = H::pick_component(H::uniform53(w.x, w.y), p.cum, p.K);
    cs[d] = k;
    comp[base + d] = k;
  }
  __syncthreads();
  for (int e = tid; e < cnt * np; e += SB) {
    const int d = e / np, i = e - d * np, k = cs[d];
    const double *Ci = p.Cf + ((size_t)k * np + i) * np;
    const float *zd = zs + d * zstride;
    double s = 0.0;
    for (int l = 0; l <= i; ++l) s = __dadd_rn(s, __dmul_rn(Ci[l], (double)zd[l]));
    xo[(size_t)(base + d) * np + i] = (float)__dadd_rn(p.c[(size_t)k * np + i], s);
  }
}

struct TermArgs {
  int mode;
  double r, lstar, s1, s2, logz, m1, m2, mf1, mf2;
};

// 6. grid = nwg1 + nwg2: the first nwg1 workgroups take the rows (l1), the others the draws (l2), each a stretch of chunk values;
// slab[0][w] = the rows' sum, slab[1][w] the draws' sum, slab[2][w] the rows' maximum, slab[3][w] the draws' (TM_STATS alone); slab
// rows are TM_MAX_WG apart.  TM_ERR1 also writes f2[n1] as floats
__global__ void __launch_bounds__(SB) k_ev_terms(TermArgs a, const double *l1, int64_t n1, unsigned nwg1, const double *l2, int64_t n2,
                                                 unsigned nwg2, double *slab, float *f2)
{
  __shared__ double red[SB], redm[SB];
  const int tid = (int)threadIdx.x;
  const bool rows = blockIdx.x < nwg1;
  const unsigned w = rows ? blockIdx.x : blockIdx.x - nwg1, nwg = rows ? nwg1 : nwg2;
  const int64_t n = rows ? n1 : n2, chunk = (n + nwg - 1) / nwg, i0 = (int64_t)w * chunk, i1 = min(n, i0 + chunk);
  const double *l = rows ? l1 : l2;
  const double ninf = -__longlong_as_double(0x7ff0000000000000ll);
  double s = 0.0, m = ninf;
  for (int64_t i = i0 + tid; i < i1; i += SB) {
    const double v = l[i];
    switch (a.mode) {
    case TM_STATS:
      if (rows) {
        s += v;
        m = fmax(m, -v);
      } else if (v == ninf) s += 1.0;
      else m = fmax(m, v);
      break;
    case TM_BRIDGE:
      s += rows ? H::term_den(v - a.lstar, a.r, a.s1, a.s2) : H::term_num(v - a.lstar, a.r, a.s1, a.s2);
      break;
    case TM_ERR1:
      if (rows) {
        const double f = H::term_f2(v - a.logz, a.s1, a.s2);
        f2[i] = (float)f;
        s += f;
      } else s += H::term_f1(v - a.logz, a.s1, a.s2);
      break;
    case TM_ERR2: {
      const double d = rows ? H::term_f2(v - a.logz, a.s1, a.s2) - a.mf2 : H::term_f1(v - a.logz, a.s1, a.s2) - a.mf1;
      s += d * d;
    } break;
    default:
      s += rows ? exp(-v - a.m1) : exp(v - a.m2);
      break;
    }
  }
  red[tid] = s;
  redm[tid] = m;
  __syncthreads();
  for (int h = SB / 2; h > 0; h >>= 1) {
    if (tid < h) {
      red[tid] += red[tid + h];
      redm[tid] = fmax(redm[tid], redm[tid + h]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    slab[(rows ? 0 : 1) * TM_MAX_WG + w] = red[0];
    if (a.mode == TM_STATS) slab[(rows ? 2 : 3) * TM_MAX_WG + w] = redm[0];
  }
}

// ---- what a call refuses before a device is touched, and what its defaults come to
struct Resolved {
  int fit = 0, K = 1, max_iter = H::MAX_ITER_DEFAULT;
  int64_t T1 = 0, N1 = 0, N2 = 0;
  bool fitted = true;
  std::vector<double> c, Cf, W, lc, cum;  // of a caller's proposal, factored on the host
};

int factor(int np, int K, const double *w, const double *c, const double *cov, double scale, Resolved &R)
{
  char msg[256];
  R.K = K;
  R.c.assign(c, c + (size_t)K * np);
  R.Cf.assign((size_t)K * np * np, 0.0);
  R.W.assign((size_t)K * np * np, 0.0);
  R.lc.assign((size_t)K, 0.0);
  if (H::proposal(np, K, w, c, cov, scale, R.Cf.data(), R.W.data(), R.lc.data(), msg, sizeof msg) != H::OK)
    return fail(MCX_ERR_INVALID, "evidence: %s", msg);
  R.cum.assign((size_t)K, 0.0);
  double s = 0.0;
  for (int k = 0; k < K; ++k) R.cum[k] = s += w[k];
  return MCX_OK;
}

int mixture_args(int np, const mcx_evidence_mixture *m)
{
  char msg[256];
  if (!m) return fail(MCX_ERR_INVALID, "the proposal m is NULL");
  if (H::mixture_check(np, m->k, m->weights, m->centres, m->covs, m->scale, msg, sizeof msg) != H::OK)
    return fail(MCX_ERR_INVALID, "evidence: %s", msg);
  return MCX_OK;
}

int evidence_args(int nsteps, int nc, int np, const mcx_vlfunc *L, bool need_L, const mcx_evidence_spec *spec, const mcx_evidence_mixture *m,
                  const mcx_evidence_result *res, Resolved &R)
{
  if (!spec) return fail(MCX_ERR_INVALID, "spec is NULL");
  if (!res) return fail(MCX_ERR_INVALID, "res is NULL");
  if (need_L && !L) return fail(MCX_ERR_INVALID, "the likelihood L is NULL");
  if (np < 1 || np > 256) return fail(MCX_ERR_INVALID, "np = %d: 1 to 256 parameters", np);
  if (nsteps < 1 || nc < 1) return fail(MCX_ERR_INVALID, "nsteps = %d, nc = %d: at least one step of one chain", nsteps, nc);
  if (L && L->d != np) return fail(MCX_ERR_INVALID, "evidence: L->d = %d but the rows have np = %d parameters", L->d, np);
  if (!(spec->tol >= 0.0)) return fail(MCX_ERR_INVALID, "tol = %g: not negative", spec->tol);
  if (spec->max_iter < 0) return fail(MCX_ERR_INVALID, "max_iter = %d: not negative (0 = %d)", spec->max_iter, H::MAX_ITER_DEFAULT);
  if (spec->ndraw < 0) return fail(MCX_ERR_INVALID, "ndraw = %lld: not negative (0 = min(N1, 2^20))", spec->ndraw);
  R.fitted = m == nullptr;
  R.max_iter = spec->max_iter > 0 ? spec->max_iter : H::MAX_ITER_DEFAULT;
  if (m) MCXCHK(mixture_args(np, m));
  else if (!(spec->scale > 0.0) || !std::isfinite(spec->scale)) return fail(MCX_ERR_INVALID, "scale = %g: finite and positive", spec->scale);
  if (spec->fit_steps < -1 || spec->fit_steps >= nsteps)
    return fail(MCX_ERR_INVALID, "fit_steps = %d: 0 to %d (nsteps - 1), or -1 for the default", spec->fit_steps, nsteps - 1);
  R.fit = spec->fit_steps >= 0 ? spec->fit_steps : (m ? 0 : nsteps / 2);
  if (!m && R.fit == 0) return fail(MCX_ERR_INVALID, "fit_steps = 0: a fitted proposal needs steps to fit on (nsteps = %d)", nsteps);
  if (!m && (int64_t)R.fit * nc < 2) return fail(MCX_ERR_INVALID, "a fitted proposal needs fit_steps * nc >= 2 rows, got 1");
  R.T1 = nsteps - R.fit;
  R.N1 = R.T1 * nc;
  R.N2 = spec->ndraw > 0 ? spec->ndraw : std::min<int64_t>(R.N1, H::NDRAW_DEFAULT_MAX);
  if (R.N1 >= H::NMAX || R.N2 >= H::NMAX)
    return fail(MCX_ERR_UNSUPPORTED, "evidence: %lld rows and %lld draws, fewer than 2^31 each are supported", (long long)R.N1, (long long)R.N2);
  if (m) MCXCHK(factor(np, m->k, m->weights, m->centres, m->covs, m->scale, R));
  return MCX_OK;
}

// the proposal of R uploaded on st: pd must outlive the kernels
int upload_proposal(hipStream_t st, int np, const Resolved &R, DevBuf<double> &pd, PropDev &p)
{
  const size_t K = (size_t)R.K, nn = (size_t)np * np;
  MCXCHK(pd.alloc(K * np + 2 * K * nn + K));
  double *c = pd.p, *W = c + K * np, *Cf = W + K * nn, *lc = Cf + K * nn;
  HIPCHK(hipMemcpyAsync(c, R.c.data(), K * np * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(W, R.W.data(), K * nn * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(Cf, R.Cf.data(), K * nn * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(lc, R.lc.data(), K * 8, hipMemcpyHostToDevice, st));
  p.c = c; p.W = W; p.Cf = Cf; p.lc = lc; p.K = R.K;
  for (int k = 0; k < H::MAX_K; ++k) p.cum[k] = k < R.K ? R.cum[k] : 0.0;
  return MCX_OK;
}

int launch_logg(hipStream_t st, const float *x, const float *ly, int64_t N, int np, const PropDev &p, int what, double *out, uint32_t *bad)
{
  hipLaunchKernelGGL(k_ev_logg, dim3(sweep_wg(N, np)), dim3(SB), logg_lds(np), st, x, ly, N, np, tile_rows(np), w_chunk_rows(np), p, what, out, bad);
  HIPCHK(hipGetLastError());
  return MCX_OK;
}

int launch_draw(hipStream_t st, const PropDev &p, int np, uint32_t seed, int64_t n2, float *xo, int *comp)
{
  hipLaunchKernelGGL(k_ev_draw, dim3(draw_wg(n2, np)), dim3(SB), draw_lds(np), st, p, np, seed, n2, draw_rows(np), draw_zstride(np), xo, comp);
  HIPCHK(hipGetLastError());
  return MCX_OK;
}

// log L of n draws x[n][np] on the device -> y[n], by the likelihood's own code
int eval_draws(hipStream_t st, const LikDev &L, const float *x, float *y, int64_t n, int np)
{
  if (L.kind == MCX_VL_HOST) {
    if (!L.fn) return fail(MCX_ERR_VLFUNC, "MCX_VL_HOST without a callback");
    std::vector<float> hx((size_t)n * np), hy((size_t)n);
    HIPCHK(hipMemcpyAsync(hx.data(), x, hx.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    (void)L.fn(L.ctx, (int)n, hx.data(), hy.data());
    HIPCHK(hipMemcpyAsync(y, hy.data(), hy.size() * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // (hy goes)
    return MCX_OK;
  }
  if (L.kind == MCX_VL_DEVICE) {
    int npset = (int)n;
    const float *xa = x;
    float *ya = y;
    void *args[] = {&npset, &xa, &ya};
    HIPCHK(hipModuleLaunchKernel((hipFunction_t)L.ctx, nblocks((size_t)n), 1, 1, BLOCK, 1, 1, 0, st, args, nullptr));
    return MCX_OK;
  }
  return eval_device(L, x, y, (int)n, np, st);
}

// one terms pass and its reducer: sums[0] the rows' sum, sums[1] the draws'
struct Terms {
  hipStream_t st;
  const double *l1, *l2;
  int64_t n1, n2;
  unsigned w1, w2;
  double *slab, *out;  // slab[4][TM_MAX_WG] | out[2]
  float *f2;
  int pass(const TermArgs &a, double sums[2], std::vector<double> *maxima = nullptr)
  {
    hipLaunchKernelGGL(k_ev_terms, dim3(w1 + w2), dim3(SB), 0, st, a, l1, n1, w1, l2, n2, w2, slab, f2);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_sum_rows, dim3(2), dim3(SB), 0, st, (const double *)slab, (size_t)TM_MAX_WG, 1, 2, 1, (size_t)w1, (size_t)w2,
                       (const double *)nullptr, 0.0, out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sums, out, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (maxima) {
      maxima->assign(2 * (size_t)TM_MAX_WG, 0.0);
      HIPCHK(hipMemcpyAsync(maxima->data(), slab + 2 * TM_MAX_WG, 2 * (size_t)TM_MAX_WG * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    return MCX_OK;
  }
};

// the call on a view.  l1o[N1], l2o[N2] (mcx_debug_evidence_l) and ms (mcx_debug_evidence_times) may be NULL
int evidence_device(hipStream_t st, Bufs B, const StoreView &v, const LikDev &lik, const mcx_evidence_spec *spec, Resolved &R,
                    mcx_evidence_result *res, double *l1o, double *l2o, double *ms)
{
  const auto t0 = std::chrono::steady_clock::now();
  const int np = v.np, nc = v.nc;
  const int64_t N1 = R.N1, N2 = R.N2;
  const double qnan = std::numeric_limits<double>::quiet_NaN(), ninf = -std::numeric_limits<double>::infinity();
  StageTimer tm{st, ms, ET_N, {}};
  DevBuf<double> pd, l1, l2, slab;
  DevBuf<float> xd, lld, f2;
  DevBuf<int> comp;
  DevBuf<uint32_t> bad;
  PropDev p;
  *res = mcx_evidence_result{};
  int flags = 0;
  double neff = (double)N1, ess_f2 = (double)N1;
  H::Bridge b;
  double sums[2], e1[2], e2[2], by[2], m1 = 0.0, m2 = 0.0;
  long long nzero = 0;
  const float *x1 = v.x + (size_t)R.fit * nc * np, *ly1 = v.ly + (size_t)R.fit * nc;
  auto run = [&]() -> int {
    // ---- 1. the fitted proposal
    if (R.fitted) {
      const int ncol = np + 1;
      std::vector<double> mean((size_t)ncol), cov((size_t)ncol * ncol), cc((size_t)np * np);
      MCXCHK(tm.run(ET_FIT, [&]() -> int { return covariance_span(st, B, StoreSpan{v.x, v.ly, nc, np, (int64_t)R.fit}, mean.data(), cov.data(), nullptr); }));
      for (int i = 0; i < np; ++i)
        for (int j = 0; j < np; ++j) cc[(size_t)i * np + j] = cov[(size_t)i * ncol + j];
      const double one = 1.0;
      MCXCHK(factor(np, 1, &one, mean.data(), cc.data(), spec->scale, R));
    }
    MCXCHK(upload_proposal(st, np, R, pd, p));
    MCXCHK(xd.alloc((size_t)N2 * np));
    MCXCHK(lld.alloc((size_t)N2));
    MCXCHK(comp.alloc((size_t)N2));
    MCXCHK(l1.alloc((size_t)N1));
    MCXCHK(l2.alloc((size_t)N2));
    MCXCHK(f2.alloc((size_t)N1));
    MCXCHK(slab.alloc(4 * (size_t)TM_MAX_WG + 2));
    MCXCHK(bad.alloc(2));
    HIPCHK(hipMemsetAsync(bad.p, 0xff, 2 * sizeof(uint32_t), st));
    // ---- 2. to 4.
    MCXCHK(tm.run(ET_DRAW, [&]() -> int { return launch_draw(st, p, np, spec->seed, N2, xd.p, comp.p); }));
    MCXCHK(tm.run(ET_LIK, [&]() -> int { return eval_draws(st, lik, xd.p, lld.p, N2, np); }));
    MCXCHK(tm.run(ET_SWEEP_ROWS, [&]() -> int { return launch_logg(st, x1, ly1, N1, np, p, LG_ROWS, l1.p, bad.p); }));
    MCXCHK(tm.run(ET_SWEEP_DRAWS, [&]() -> int { return launch_logg(st, xd.p, lld.p, N2, np, p, LG_DRAWS, l2.p, bad.p + 1); }));
    uint32_t hb[2];
    HIPCHK(hipMemcpyAsync(hb, bad.p, sizeof hb, hipMemcpyDeviceToHost, st));
    if (l1o) HIPCHK(hipMemcpyAsync(l1o, l1.p, (size_t)N1 * 8, hipMemcpyDeviceToHost, st));
    if (l2o) HIPCHK(hipMemcpyAsync(l2o, l2.p, (size_t)N2 * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (hb[0] != NO_ROW)
      return fail(MCX_ERR_INVALID, "evidence: log L - log g of row %u is not finite (the lowest such row; a stored log L of +-inf or NaN, or a parameter that is not finite)", hb[0]);
    if (hb[1] != NO_ROW) return fail(MCX_ERR_INVALID, "evidence: log L - log g of draw %u is +inf or NaN (the lowest such draw)", hb[1]);
    // ---- 5. neff
    if (spec->use_neff) {
      if (R.T1 < 4) flags |= MCX_EVIDENCE_NO_ESS;
      else {
        std::vector<mcx_col_summary> cs((size_t)np + 1);
        MCXCHK(tm.run(ET_ESS, [&]() -> int { return summary_mixing(st, B, StoreSpan{x1, ly1, nc, np, R.T1}, cs.data()); }));
        std::vector<double> ess((size_t)np);
        for (int c = 0; c < np; ++c) ess[c] = cs[c].ess;
        const double med = H::lower_median(ess);
        if (med == med && med > 0.0) neff = std::min(med, (double)N1);
        else flags |= MCX_EVIDENCE_NO_ESS;
      }
    }
    // ---- 6. the statistics of l, the loop, the error, the by-products
    Terms T{st, l1.p, l2.p, N1, N2, terms_wg(N1), terms_wg(N2), slab.p, slab.p + 4 * TM_MAX_WG, f2.p};
    return tm.run(ET_BRIDGE, [&]() -> int {
      TermArgs a{};
      std::vector<double> mx;
      a.mode = TM_STATS;
      MCXCHK(T.pass(a, sums, &mx));
      m1 = m2 = ninf;
      for (unsigned w = 0; w < T.w1; ++w) m1 = std::max(m1, mx[w]);
      for (unsigned w = 0; w < T.w2; ++w) m2 = std::max(m2, mx[(size_t)TM_MAX_WG + w]);
      nzero = (long long)sums[1];
      if (nzero == N2) return fail(MCX_ERR_INVALID, "evidence: every one of the %lld draws has L = 0: the proposal misses the sampled function", (long long)N2);
      b.begin(N1, N2, neff, sums[0] / (double)N1, spec->tol, R.max_iter);
      a.mode = TM_BRIDGE; a.lstar = b.lstar; a.s1 = b.s1; a.s2 = b.s2;
      for (;;) {
        a.r = b.r;
        MCXCHK(T.pass(a, sums));
        if (b.update(sums[1], sums[0])) break;
      }
      a.logz = b.log_z();
      a.mode = TM_ERR1;
      MCXCHK(T.pass(a, e1));
      a.mf2 = e1[0] / (double)N1; a.mf1 = e1[1] / (double)N2;
      a.mode = TM_ERR2;
      MCXCHK(T.pass(a, e2));
      a.m1 = m1; a.m2 = m2;
      a.mode = TM_BYPRODUCTS;
      return T.pass(a, by);
    });
  };
  int rc = run();
  if (rc == MCX_OK && R.T1 >= 4) {  // ess_f2: section 9 on the one-column store of f2 (its log L column is f2 again)
    std::vector<mcx_col_summary> cs(2);
    rc = tm.run(ET_ESS, [&]() -> int { return summary_mixing(st, B, StoreSpan{f2.p, f2.p, nc, 1, R.T1}, cs.data()); });
    if (rc == MCX_OK && cs[0].ess == cs[0].ess && cs[0].ess > 0.0) ess_f2 = cs[0].ess;
  }
  (void)hipStreamSynchronize(st);  // (before the call's buffers go)
  MCXCHK(rc);
  MCXCHK(tm.collect());
  res->n1 = N1; res->n2 = N2; res->k = R.K; res->fit_steps = R.fit;
  res->neff = neff; res->lstar = b.lstar; res->log_z = b.log_z();
  H::finish_error(e1[1], e2[1], N2, e1[0], e2[0], N1, ess_f2, &res->re2_draws, &res->re2_rows, &res->se);
  res->ess_f2 = ess_f2;
  res->log_z_is = H::finish_is(m2, by[1], N2);
  res->log_z_ris = H::finish_ris(m1, by[0], N1);
  res->ndraw_zero = nzero;
  res->iters = b.iters;
  res->flags = flags | b.flags;
  (void)qnan;
  if (ms) ms[ET_CALL] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return MCX_OK;
}

// a caller's likelihood set up on st for a call; the engine's own when L is NULL
struct LikOf {
  LikDev own;
  const LikDev *use = nullptr;
  int setup(const mcx_vlfunc *L, const LikDev *engines, int np, hipStream_t st)
  {
    if (!L) {
      if (!engines || engines->kind == 0) return fail(MCX_ERR_INVALID, "evidence: L is NULL and the engine has run no likelihood yet");
      use = engines;
      return MCX_OK;
    }
    MCXCHK(lik_setup(own, L, np, st));
    use = &own;
    return MCX_OK;
  }
};

int rows_call(const float *rows, int nsteps, int nc, int np, const mcx_vlfunc *L, const mcx_evidence_spec *spec, const mcx_evidence_mixture *m,
              mcx_evidence_result *res, double *l1, double *l2)
{
  Resolved R;
  if (!rows) return fail(MCX_ERR_INVALID, "rows is NULL");
  MCXCHK(evidence_args(nsteps, nc, np, L, true, spec, m, res, R));
  LikOf lk;  // (outlives the stream's work: on_rows waits before it returns)
  return on_rows(rows, nsteps, nc, np, [&](hipStream_t st, Bufs B, const StoreView &v) -> int {
    MCXCHK(lk.setup(L, nullptr, np, st));
    return evidence_device(st, B, v, *lk.use, spec, R, res, l1, l2, nullptr);
  });
}

int samples_call(mcx_engine *e, int first_step, int nsteps, const mcx_vlfunc *L, const mcx_evidence_spec *spec, const mcx_evidence_mixture *m,
                 mcx_evidence_result *res, double *ms)
{
  Resolved R;
  LikOf lk;
  const int rc = on_store(
      e, first_step, nsteps, [&]() -> int { return evidence_args(nsteps, e->nchain, e->nparam, L, false, spec, m, res, R); },
      [&](hipStream_t st, Bufs B, const StoreView &v) -> int {
        MCXCHK(lk.setup(L, &e->lik, v.np, st));
        return evidence_device(st, B, v, *lk.use, spec, R, res, nullptr, nullptr, ms);
      });
  if (e && lk.use == &lk.own) (void)hipStreamSynchronize(e->stream);  // (the parameter upload reads lk.own.host)
  return rc;
}

}  // namespace

extern "C" int mcx_samples_evidence(mcx_engine *e, int first_step, int nsteps, const mcx_vlfunc *L, const mcx_evidence_spec *spec,
                                    const mcx_evidence_mixture *proposal, mcx_evidence_result *res)
{
  return samples_call(e, first_step, nsteps, L, spec, proposal, res, nullptr);
}

extern "C" int mcx_debug_evidence_times(mcx_engine *e, int first_step, int nsteps, const mcx_vlfunc *L, const mcx_evidence_spec *spec,
                                        const mcx_evidence_mixture *proposal, mcx_evidence_result *res, double *ms)
{
  if (e && !ms) return fail(MCX_ERR_INVALID, "ms is NULL");
  return samples_call(e, first_step, nsteps, L, spec, proposal, res, ms);
}

extern "C" int mcx_rows_evidence(const float *rows, int nsteps, int nc, int np, const mcx_vlfunc *L, const mcx_evidence_spec *spec,
                                 const mcx_evidence_mixture *proposal, mcx_evidence_result *res)
{
  return rows_call(rows, nsteps, nc, np, L, spec, proposal, res, nullptr, nullptr);
}

extern "C" int mcx_debug_evidence_l(const float *rows, int nsteps, int nc, int np, const mcx_vlfunc *L, const mcx_evidence_spec *spec,
                                    const mcx_evidence_mixture *proposal, mcx_evidence_result *res, double *l1, double *l2)
{
  if (!l1 || !l2) return fail(MCX_ERR_INVALID, "l1 or l2 is NULL");
  return rows_call(rows, nsteps, nc, np, L, spec, proposal, res, l1, l2);
}

extern "C" int mcx_store_evidence(mcx_store *s, const mcx_vlfunc *L, const mcx_evidence_spec *spec, const mcx_evidence_mixture *proposal,
                                  mcx_evidence_result *res)
{
  if (!s) return fail(MCX_ERR_INVALID, "the store s is NULL");
  Resolved R;
  MCXCHK(evidence_args(s->T, s->nc, s->nout, L, true, spec, proposal, res, R));
  HIPCHK(hipSetDevice(s->device));
  LikOf lk;
  int rc = lk.setup(L, nullptr, s->nout, s->st);
  if (rc == MCX_OK) rc = evidence_device(s->st, s->bufs(), StoreView(s->span()), *lk.use, spec, R, res, nullptr, nullptr, nullptr);
  (void)hipStreamSynchronize(s->st);  // (the parameter upload reads lk.own.host)
  return rc;
}

// host only
extern "C" int mcx_evidence_proposal(int np, const mcx_evidence_mixture *m, double *C, double *W, double *lc)
{
  if (!lc) return fail(MCX_ERR_INVALID, "lc is NULL");
  MCXCHK(mixture_args(np, m));
  Resolved R;
  MCXCHK(factor(np, m->k, m->weights, m->centres, m->covs, m->scale, R));
  if (C) std::copy(R.Cf.begin(), R.Cf.end(), C);
  if (W) std::copy(R.W.begin(), R.W.end(), W);
  std::copy(R.lc.begin(), R.lc.end(), lc);
  return MCX_OK;
}

// host only
extern "C" int mcx_evidence_iterate(const double *l1, long long n1, const double *l2, long long n2, double neff, double tol, int max_iter,
                                    mcx_evidence_result *res)
{
  if (!l1 || !l2 || !res) return fail(MCX_ERR_INVALID, "l1, l2 or res is NULL");
  if (n1 < 1 || n2 < 1) return fail(MCX_ERR_INVALID, "n1 = %lld, n2 = %lld: at least one row and one draw", n1, n2);
  if (n1 >= H::NMAX || n2 >= H::NMAX) return fail(MCX_ERR_UNSUPPORTED, "n1 = %lld, n2 = %lld: fewer than 2^31 each are supported", n1, n2);
  if (!(tol >= 0.0)) return fail(MCX_ERR_INVALID, "tol = %g: not negative", tol);
  if (max_iter < 0) return fail(MCX_ERR_INVALID, "max_iter = %d: not negative (0 = %d)", max_iter, H::MAX_ITER_DEFAULT);
  if (!(neff > 0.0) || !std::isfinite(neff)) return fail(MCX_ERR_INVALID, "neff = %g: finite and positive", neff);
  char msg[256];
  H::IterateResult o;
  const double ne = std::min(neff, (double)n1);
  if (H::iterate(l1, n1, l2, n2, ne, (double)n1, tol, max_iter, &o, msg, sizeof msg) != H::OK) return fail(MCX_ERR_INVALID, "evidence: %s", msg);
  *res = mcx_evidence_result{};
  res->n1 = n1; res->n2 = n2; res->neff = ne; res->lstar = o.lstar; res->log_z = o.log_z; res->se = o.se;
  res->re2_draws = o.re2_draws; res->re2_rows = o.re2_rows; res->ess_f2 = (double)n1; res->log_z_is = o.log_z_is;
  res->log_z_ris = o.log_z_ris; res->ndraw_zero = o.ndraw_zero; res->iters = o.iters; res->flags = o.flags;
  return MCX_OK;
}

extern "C" int mcx_debug_evidence_logg(const float *x, long long n, int np, const mcx_evidence_mixture *m, double *lg)
{
  if (!x || !lg) return fail(MCX_ERR_INVALID, "x or lg is NULL");
  if (n < 1) return fail(MCX_ERR_INVALID, "n = %lld: at least one row", n);
  if (n >= H::NMAX) return fail(MCX_ERR_UNSUPPORTED, "n = %lld: fewer than 2^31 rows are supported", n);
  MCXCHK(mixture_args(np, m));
  Resolved R;
  MCXCHK(factor(np, m->k, m->weights, m->centres, m->covs, m->scale, R));
  MCXCHK(need_device());
  DevStream st;
  DevBuf<double> pd, out;
  DevBuf<float> xd;
  DevBuf<uint32_t> bad;
  PropDev p;
  auto run = [&]() -> int {
    MCXCHK(st.ensure(hipStreamNonBlocking));
    MCXCHK(upload_proposal(st, np, R, pd, p));
    MCXCHK(xd.alloc((size_t)n * np));
    MCXCHK(out.alloc((size_t)n));
    MCXCHK(bad.alloc(1));
    HIPCHK(hipMemcpyAsync(xd.p, x, (size_t)n * np * sizeof(float), hipMemcpyHostToDevice, st));
    MCXCHK(launch_logg(st, xd.p, nullptr, n, np, p, LG_PLAIN, out.p, bad.p));
    HIPCHK(hipMemcpyAsync(lg, out.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    return MCX_OK;
  };
  const int rc = run();
  if (st) (void)hipStreamSynchronize(st);
  return rc;
}

extern "C" int mcx_debug_evidence_draws(int np, const mcx_evidence_mixture *m, const mcx_vlfunc *L, uint32_t seed, long long ndraw, float *x,
                                        int *comp, double *lg, float *ll)
{
  if (ndraw < 1) return fail(MCX_ERR_INVALID, "ndraw = %lld: at least one draw", ndraw);
  if (ndraw >= H::NMAX) return fail(MCX_ERR_UNSUPPORTED, "ndraw = %lld: fewer than 2^31 draws are supported", ndraw);
  MCXCHK(mixture_args(np, m));
  if (ll && !L) return fail(MCX_ERR_INVALID, "ll asks for a likelihood and L is NULL");
  if (L && L->d != np) return fail(MCX_ERR_INVALID, "evidence: L->d = %d but the draws have np = %d parameters", L->d, np);
  Resolved R;
  MCXCHK(factor(np, m->k, m->weights, m->centres, m->covs, m->scale, R));
  MCXCHK(need_device());
  DevStream st;
  DevBuf<double> pd, out;
  DevBuf<float> xd, lld;
  DevBuf<int> cd;
  DevBuf<uint32_t> bad;
  PropDev p;
  LikOf lk;
  auto run = [&]() -> int {
    MCXCHK(st.ensure(hipStreamNonBlocking));
    MCXCHK(upload_proposal(st, np, R, pd, p));
    MCXCHK(xd.alloc((size_t)ndraw * np));
    MCXCHK(cd.alloc((size_t)ndraw));
    MCXCHK(out.alloc((size_t)ndraw));
    MCXCHK(lld.alloc((size_t)ndraw));
    MCXCHK(bad.alloc(1));
    MCXCHK(launch_draw(st, p, np, seed, ndraw, xd.p, cd.p));
    if (x) HIPCHK(hipMemcpyAsync(x, xd.p, (size_t)ndraw * np * sizeof(float), hipMemcpyDeviceToHost, st));
    if (comp) HIPCHK(hipMemcpyAsync(comp, cd.p, (size_t)ndraw * sizeof(int), hipMemcpyDeviceToHost, st));
    if (lg) {
      MCXCHK(launch_logg(st, xd.p, nullptr, ndraw, np, p, LG_PLAIN, out.p, bad.p));
      HIPCHK(hipMemcpyAsync(lg, out.p, (size_t)ndraw * 8, hipMemcpyDeviceToHost, st));
    }
    if (ll) {
      MCXCHK(lk.setup(L, nullptr, np, st));
      MCXCHK(eval_draws(st, *lk.use, xd.p, lld.p, ndraw, np));
      HIPCHK(hipMemcpyAsync(ll, lld.p, (size_t)ndraw * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    return MCX_OK;
  };
  const int rc = run();
  if (st) (void)hipStreamSynchronize(st);
  return rc;
}

// host only
extern "C" int mcx_debug_evidence_geometry(int np, long long n1, long long n2, int k, mcx_evidence_geometry *g)
{
  if (!g) return fail(MCX_ERR_INVALID, "g is NULL");
  if (np < 1 || np > 256) return fail(MCX_ERR_INVALID, "np = %d: 1 to 256 parameters", np);
  if (k < 1 || k > H::MAX_K) return fail(MCX_ERR_INVALID, "k = %d: 1 to %d components", k, H::MAX_K);
  if (n1 < 1 || n2 < 1) return fail(MCX_ERR_INVALID, "n1 = %lld, n2 = %lld: at least one row and one draw", n1, n2);
  if (n1 >= H::NMAX || n2 >= H::NMAX) return fail(MCX_ERR_UNSUPPORTED, "n1 = %lld, n2 = %lld: fewer than 2^31 each are supported", n1, n2);
  g->block = SB;
  g->tile_rows = tile_rows(np);
  g->slices = SB / tile_rows(np);
  g->sweep_tiles = sweep_tiles_of(n1, np);
  g->sweep_workgroups = sweep_wg(n1, np);
  g->sweep_max_workgroups = EV_MAX_WG;
  g->sweep_lds_bytes = (long long)logg_lds(np);
  g->use_mfma = 0;
  g->w_chunk_rows = w_chunk_rows(np);
  g->draw_rows = draw_rows(np);
  g->draw_workgroups = draw_wg(n2, np);
  g->draw_lds_bytes = (long long)draw_lds(np);
  g->terms_workgroups_rows = terms_wg(n1);
  g->terms_workgroups_draws = terms_wg(n2);
  const size_t nn = (size_t)np * np, K = (size_t)k;
  g->scratch_bytes = (long long)(8 * (K * np + 2 * K * nn + K) + 4 * (size_t)n2 * np + 4 * (size_t)n2 + 4 * (size_t)n2 + 8 * (size_t)n1 +
                                 8 * (size_t)n2 + 4 * (size_t)n1 + 8 * (4 * (size_t)TM_MAX_WG + 2) + 8);
  return MCX_OK;
}
