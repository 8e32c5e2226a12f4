// mcx_derive.hip -- derived columns and bootstrap draws of the sample store (the reference's
// mcparam.sample(mc.data, nsamp, func), src/anly/mcpar-analysis.R:30-47).
//   mcx_samples_derive / mcx_rows_derive   one sweep of the kernel of mcx_derive.hpp over a step range: a function of one row
//                                          (MCX_DERIVE_LINEAR, compiled here; MCX_DERIVE_SOURCE, a user's HIP text built around
//                                          the same body at run time) -> an mcx_store of the same shape, nout columns and log L
//   mcx_store_*                            the derived store as an object that owns its memory, a stream and its scratch: the
//                                          third way to a view beside on_store and on_rows.  Its three analyses are the passes
//                                          of mcx_summary.hip, mcx_ranks.hip and mcx_covariance.hip on a span of it
//   mcx_samples_draw / mcx_store_draw      rows drawn with replacement; the index of draw i is a function of (seed, i, N) only
#include "mcx_derive.hpp"

#include "mcx_store.hpp"

#include <map>

namespace {

// Philox stream of the draws.  The step kernels use streams 0-4 (mcx_numerics.hpp), so a draw never shares a block with a
// run of the same seed; the constant lives here because no step kernel has any business with it
constexpr uint32_t ST_DRAW = 5;

// index of draw i among N rows: w = philox(counter (i lo, i hi, 0, 0), key (seed, ST_DRAW)), r = w.x : w.y, (r N) >> 64
__host__ __device__ inline uint64_t draw_index(uint32_t seed, uint64_t i, uint64_t N)
{
  const u32x4 w = philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), 0u, 0u, seed, ST_DRAW);
  const uint64_t r = ((uint64_t)w.x << 32) | (uint64_t)w.y;
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(r, N);
#else
  return (uint64_t)(((unsigned __int128)r * (unsigned __int128)N) >> 64);
#endif
}

__global__ void __launch_bounds__(DERIVE_BLOCK) k_derive_linear(const DeriveArgs a) { derive_body(a, a.np, a.nout, DeriveLinear{}); }

// rows[k][0..np] = (x[j], ly[j]) of store row j = DRAW ? draw_index(seed, i0 + k, N) : i0 + k, for k < n: MCout layout.  A
// workgroup takes DERIVE_BLOCK rows; its threads write their (np + 1) * rows floats in order.  index (DRAW, may be NULL): j
template <bool DRAW>
__global__ void __launch_bounds__(DERIVE_BLOCK) k_gather_rows(const float *x, const float *ly, int np, uint64_t N, uint32_t seed,
                                                              uint64_t i0, uint64_t n, float *rows, long long *index)
{
  __shared__ uint64_t src[DERIVE_BLOCK];
  const uint64_t base = (uint64_t)blockIdx.x * DERIVE_BLOCK;
  const int cnt = n - base < (uint64_t)DERIVE_BLOCK ? (int)(n - base) : DERIVE_BLOCK, tid = (int)threadIdx.x;
  if (tid < cnt) {
    const uint64_t j = DRAW ? draw_index(seed, i0 + base + tid, N) : i0 + base + tid;
    src[tid] = j;
    if (DRAW && index) index[base + tid] = (long long)j;
  }
  __syncthreads();
  const int ncol = np + 1, total = cnt * ncol;
  float *out = rows + base * (uint64_t)ncol;
  for (int e = tid; e < total; e += DERIVE_BLOCK) {
    const int r = e / ncol, c = e - r * ncol;
    const uint64_t j = src[r];  // < N: the high half of r * N, or a row of the range
    out[e] = c < np ? x[j * (uint64_t)np + c] : ly[j];
  }
}

// rows[k][0..np] = (x[j], ly[j]) of store row j = floor(k N / n), k < n <= N: n rows evenly spaced in store order (section 28).
// k < 2^14 there, so k * N stays below 2^64
__global__ void __launch_bounds__(DERIVE_BLOCK) k_gather_spaced(const float *x, const float *ly, int np, uint64_t N, uint64_t n, float *rows)
{
  __shared__ uint64_t src[DERIVE_BLOCK];
  const uint64_t base = (uint64_t)blockIdx.x * DERIVE_BLOCK;
  const int cnt = n - base < (uint64_t)DERIVE_BLOCK ? (int)(n - base) : DERIVE_BLOCK, tid = (int)threadIdx.x;
  if (tid < cnt) src[tid] = (base + tid) * N / n;
  __syncthreads();
  const int ncol = np + 1, total = cnt * ncol;
  float *out = rows + base * (uint64_t)ncol;
  for (int e = tid; e < total; e += DERIVE_BLOCK) {
    const int r = e / ncol, c = e - r * ncol;
    const uint64_t j = src[r];  // < N: floor(k N / n) with k < n
    out[e] = c < np ? x[j * (uint64_t)np + c] : ly[j];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// the function of a row
// ---------------------------------------------------------------------------------------------------------------------
int derive_spec_args(const mcx_derive *f, int np, const void *out)
{
  if (!f) return fail(MCX_ERR_INVALID, "the derive spec f is NULL");
  if (!out) return fail(MCX_ERR_INVALID, "out is NULL");
  if (np < 1 || np > DERIVE_MAXW) return fail(MCX_ERR_INVALID, "np = %d: a derive takes rows of 1 to %d parameters", np, DERIVE_MAXW);
  if (f->kind != MCX_DERIVE_LINEAR && f->kind != MCX_DERIVE_SOURCE)
    return fail(MCX_ERR_INVALID, "kind = %d: MCX_DERIVE_LINEAR (1) or MCX_DERIVE_SOURCE (2)", f->kind);
  if (f->nout < 1 || f->nout > DERIVE_MAXW) return fail(MCX_ERR_INVALID, "nout = %d: 1 to %d outputs", f->nout, DERIVE_MAXW);
  if (f->npar < 0) return fail(MCX_ERR_INVALID, "npar = %d is negative", f->npar);
  if (f->kind == MCX_DERIVE_LINEAR && f->npar != f->nout * (np + 1))
    return fail(MCX_ERR_INVALID, "npar = %d: MCX_DERIVE_LINEAR takes A[nout][np] and b[nout], nout * (np + 1) = %d floats", f->npar,
                f->nout * (np + 1));
  if (f->npar > 0 && !f->par) return fail(MCX_ERR_INVALID, "par is NULL with npar = %d", f->npar);
  if (f->kind == MCX_DERIVE_SOURCE && (!f->source || !*f->source)) return fail(MCX_ERR_INVALID, "source is NULL or empty (MCX_DERIVE_SOURCE)");
  return MCX_OK;
}

// the run-time translation unit around a user's text: mcx_user_derive in the global namespace, the kernel body around it
const char *const DERIVE_TU_HEAD =
    "#include \"mcx_numerics.hpp\"\n"
    "#line 1 \"mcx_user_derive\"\n";
const char *const DERIVE_TU_TAIL =
    "\n#line 1 \"mcx_derive_kernel\"\n"
    "#include \"mcx_derive.hpp\"\n"
    "struct McxUserDerive {\n"
    "  __device__ __forceinline__ void operator()(const float *x, int d, float ly, const float *par, float *out, int nout) const\n"
    "  { mcx_user_derive(x, d, ly, par, out, nout); }\n"
    "};\n"
    "extern \"C\" __global__ __launch_bounds__(mcx::DERIVE_BLOCK) void mcx_derive_user(const mcx::DeriveArgs a)\n"
    "{ mcx::derive_body(a, MCX_DERIVE_NP, MCX_DERIVE_NOUT, McxUserDerive{}); }\n";

int derive_compile(const char *source, int np, int nout, std::vector<char> &code)
{
  std::string log;
  return rtc_compile(std::string(DERIVE_TU_HEAD) + source + DERIVE_TU_TAIL, "mcx_derive_user.hip",
                     {"-DMCX_DERIVE_NP=" + std::to_string(np), "-DMCX_DERIVE_NOUT=" + std::to_string(nout)}, code, log, "derive");
}

struct DeriveMod {
  hipModule_t mod = nullptr;
  hipFunction_t fn = nullptr;
};
// once per (device, text, np, nout) per process; never destroyed (at process exit the HIP runtime may be gone first)
std::map<std::string, DeriveMod> &g_derive_cache = *new std::map<std::string, DeriveMod>;

int derive_user_kernel(const char *source, int np, int nout, hipFunction_t *fn)
{
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(rtc_lock());
  // (the whole text is in the key: two texts never share an entry, and a module, once loaded, is never unloaded -- a
  // hipFunction_t handed out stays valid whatever other threads derive meanwhile)
  const std::string key = std::to_string(dev) + ":" + std::to_string(np) + ":" + std::to_string(nout) + ":" + source;
  auto it = g_derive_cache.find(key);
  if (it != g_derive_cache.end()) {
    *fn = it->second.fn;
    return MCX_OK;
  }
  std::vector<char> code;
  MCXCHK(derive_compile(source, np, nout, code));
  DeriveMod m;
  HIPCHK(hipModuleLoadData(&m.mod, code.data()));
  HIPCHK(hipModuleGetFunction(&m.fn, m.mod, "mcx_derive_user"));
  g_derive_cache[key] = m;
  *fn = m.fn;
  return MCX_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// the derived store
// ---------------------------------------------------------------------------------------------------------------------
// (struct mcx_store: mcx_store.hpp)
namespace {

// the sweep over a span on stream st (the span's own stream: what wrote it is ordered before) -> a new store.  ms
// (mcx_debug_derive_times, else NULL): the sweep runs twice into the same store and *ms is the second one's time, HIP events
int derive_span(hipStream_t st, const StoreSpan &s, const mcx_derive *f, mcx_store **out, double *ms = nullptr)
{
  const uint64_t N = (uint64_t)s.T * (uint64_t)s.nc;
  std::unique_ptr<mcx_store> o(new mcx_store);
  HIPCHK(hipGetDevice(&o->device));
  o->nc = s.nc; o->nout = f->nout; o->T = (int)s.T;
  DeriveArgs a;
  a.x = s.x; a.ly = s.ly; a.N = N; a.np = s.np; a.nout = f->nout; a.R = derive_rows(s.np, f->nout);
  const uint64_t nwg = sweep_tiles(N, a.R);
  if (nwg > 0x7fffffffull) return fail(MCX_ERR_UNSUPPORTED, "derive: %llu rows in tiles of %d are more workgroups than a grid holds", (unsigned long long)N, a.R);
  hipFunction_t ufn = nullptr;
  if (f->kind == MCX_DERIVE_SOURCE) MCXCHK(derive_user_kernel(f->source, s.np, f->nout, &ufn));
  MCXCHK(o->st.ensure(hipStreamNonBlocking));
  MCXCHK(o->x.alloc((size_t)N * f->nout));
  MCXCHK(o->ly.alloc((size_t)N));
  DevBuf<float> par;
  auto run = [&]() -> int {
    MCXCHK(par.alloc((size_t)f->npar));
    if (f->npar > 0) HIPCHK(hipMemcpyAsync(par.p, f->par, (size_t)f->npar * sizeof(float), hipMemcpyHostToDevice, st));
    a.xo = o->x.p; a.lyo = o->ly.p; a.par = par.p;
    const size_t lds = (size_t)derive_lds_floats(a.np, a.nout, a.R) * sizeof(float);
    auto sweep = [&]() -> int {
      if (ufn) {
        void *args[] = {&a};
        HIPCHK(hipModuleLaunchKernel(ufn, (unsigned)nwg, 1, 1, DERIVE_BLOCK, 1, 1, (unsigned)lds, st, args, nullptr));
      } else {
        hipLaunchKernelGGL(k_derive_linear, dim3((unsigned)nwg), dim3(DERIVE_BLOCK), lds, st, a);
        HIPCHK(hipGetLastError());
      }
      return MCX_OK;
    };
    MCXCHK(sweep());
    if (ms) {
      StageTimer tm{st, ms, 1, {}};
      MCXCHK(tm.run(0, sweep));
      return tm.collect();
    }
    HIPCHK(hipStreamSynchronize(st));
    return MCX_OK;
  };
  const int rc = run();
  if (rc != MCX_OK) (void)hipStreamSynchronize(st);  // (before par and the new store go)
  MCXCHK(rc);
  *out = o.release();  // (the unique_ptr's: the store is the caller's now)
  return MCX_OK;
}

// n rows of a span from row i0 on (DRAW: draws i0 .. i0 + n - 1 of seed) to the host in MCout layout, in chunks of 64 MiB
// through one device buffer
template <bool DRAW>
int gather_to_host(hipStream_t st, const StoreSpan &s, uint32_t seed, uint64_t i0, uint64_t n, float *rows, int64_t *index)
{
  if (n == 0) return MCX_OK;
  const uint64_t N = (uint64_t)s.T * (uint64_t)s.nc, ncol = (uint64_t)s.np + 1;
  const uint64_t chunk = gather_chunk_rows(n, ncol);
  DevBuf<float> dr;
  DevBuf<long long> di;
  auto run = [&]() -> int {
    MCXCHK(dr.alloc((size_t)(std::min(chunk, n) * ncol)));
    if (DRAW && index) MCXCHK(di.alloc((size_t)std::min(chunk, n)));
    for (uint64_t done = 0; done < n; done += chunk) {
      const uint64_t k = std::min(chunk, n - done);
      hipLaunchKernelGGL(k_gather_rows<DRAW>, dim3((unsigned)((k + DERIVE_BLOCK - 1) / DERIVE_BLOCK)), dim3(DERIVE_BLOCK), 0, st, s.x, s.ly,
                         s.np, N, seed, i0 + done, k, dr.p, DRAW && index ? di.p : (long long *)nullptr);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(rows + done * ncol, dr.p, (size_t)(k * ncol) * sizeof(float), hipMemcpyDeviceToHost, st));
      if (DRAW && index) HIPCHK(hipMemcpyAsync(index + done, di.p, (size_t)k * sizeof(long long), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));  // (one chunk buffer: the next launch overwrites it)
    }
    return MCX_OK;
  };
  const int rc = run();
  if (rc != MCX_OK) (void)hipStreamSynchronize(st);  // (before the chunk buffers go)
  return rc;
}

}  // namespace

uint64_t gather_chunk_rows(uint64_t n, uint64_t ncol)
{
  // (a test knob, as MCX_RANK_GROUP_COLS is: rows per chunk, so that a small store goes through several chunks)
  if (const char *cap = std::getenv("MCX_GATHER_CHUNK_ROWS")) return (uint64_t)std::max(1LL, std::atoll(cap));
  return std::max<uint64_t>(DERIVE_BLOCK, std::min<uint64_t>(n, ((uint64_t)64 << 20) / (ncol * sizeof(float))));
}

int gather_span(hipStream_t st, const StoreSpan &s, bool draw, uint32_t seed, uint64_t i0, uint64_t n, float *rows, int64_t *index)
{
  return draw ? gather_to_host<true>(st, s, seed, i0, n, rows, index) : gather_to_host<false>(st, s, 0u, i0, n, rows, nullptr);
}

int gather_spaced(hipStream_t st, const StoreSpan &s, uint64_t n, float *rows)
{
  const uint64_t N = (uint64_t)s.T * (uint64_t)s.nc, ncol = (uint64_t)s.np + 1;
  if (n == 0 || n > N || n > ((uint64_t)1 << 14)) return fail(MCX_ERR_INVALID, "gather_spaced: %llu rows of %llu", (unsigned long long)n, (unsigned long long)N);
  DevBuf<float> dr;
  auto run = [&]() -> int {
    MCXCHK(dr.alloc((size_t)(n * ncol)));
    hipLaunchKernelGGL(k_gather_spaced, dim3((unsigned)((n + DERIVE_BLOCK - 1) / DERIVE_BLOCK)), dim3(DERIVE_BLOCK), 0, st, s.x, s.ly, s.np, N, n,
                       dr.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rows, dr.p, (size_t)(n * ncol) * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MCX_OK;
  };
  const int rc = run();
  if (rc != MCX_OK) (void)hipStreamSynchronize(st);  // (before the buffer goes)
  return rc;
}

namespace {

int draw_args(int64_t ndraw, const float *rows)
{
  if (ndraw < 0) return fail(MCX_ERR_INVALID, "ndraw = %lld is negative", (long long)ndraw);
  if (ndraw > 0 && !rows) return fail(MCX_ERR_INVALID, "rows is NULL with ndraw = %lld", (long long)ndraw);
  return MCX_OK;
}

int range_args(int nsteps)
{
  if (nsteps < 1) return fail(MCX_ERR_INVALID, "nsteps = %d: a range of at least one step", nsteps);
  return MCX_OK;
}

int store_enter(const mcx_store *s)
{
  if (!s) return fail(MCX_ERR_INVALID, "the store s is NULL");
  HIPCHK(hipSetDevice(s->device));
  return MCX_OK;
}

}  // namespace

extern "C" int mcx_samples_derive(mcx_engine *e, int first_step, int nsteps, const mcx_derive *f, mcx_store **out)
{
  return on_store(
      e, first_step, nsteps,
      [&] {
        MCXCHK(derive_spec_args(f, e->nparam, out));
        return range_args(nsteps);
      },
      [&](hipStream_t st, Bufs, const StoreView &v) { return derive_span(st, v, f, out); });
}

// mcx_samples_derive with HIP events around the sweep, for tools/derive_bench.py; the store is let go
extern "C" int mcx_debug_derive_times(mcx_engine *e, int first_step, int nsteps, const mcx_derive *f, double *ms)
{
  mcx_store *o = nullptr;
  const int rc = on_store(
      e, first_step, nsteps,
      [&] {
        if (!ms) return fail(MCX_ERR_INVALID, "ms is NULL");
        MCXCHK(derive_spec_args(f, e->nparam, &o));
        return range_args(nsteps);
      },
      [&](hipStream_t st, Bufs, const StoreView &v) { return derive_span(st, v, f, &o, ms); });
  delete o;
  return rc;
}

extern "C" int mcx_rows_derive(const float *rows, int nsteps, int nc, int np, const mcx_derive *f, mcx_store **out)
{
  MCXCHK(derive_spec_args(f, np, out));
  MCXCHK(range_args(nsteps));
  return on_rows(rows, nsteps, nc, np, [&](hipStream_t st, Bufs, const StoreView &v) { return derive_span(st, v, f, out); });
}

extern "C" int mcx_store_destroy(mcx_store *s)
{
  if (!s) return MCX_OK;
  (void)hipSetDevice(s->device);
  delete s;
  return MCX_OK;
}

extern "C" int mcx_store_shape(const mcx_store *s, int *nsteps, int *nc, int *ncol)
{
  if (!s) return fail(MCX_ERR_INVALID, "the store s is NULL");
  if (nsteps) *nsteps = s->T;
  if (nc) *nc = s->nc;
  if (ncol) *ncol = s->nout + 1;
  return MCX_OK;
}

extern "C" int mcx_store_copy(mcx_store *s, int first_step, int nsteps, float *rows)
{
  MCXCHK(store_enter(s));
  if (!rows || nsteps < 0) return fail(MCX_ERR_INVALID, "rows is NULL or nsteps = %d is negative", nsteps);
  if (first_step < 0 || (int64_t)first_step + nsteps > s->T)
    return fail(MCX_ERR_INVALID, "steps [%d,%lld) not in the derived store (%d steps)", first_step, (long long)first_step + nsteps, s->T);
  return gather_to_host<false>(s->st, s->span(), 0u, (uint64_t)first_step * s->nc, (uint64_t)nsteps * s->nc, rows, nullptr);
}

extern "C" int mcx_store_summary(mcx_store *s, const double *probs, int nprobs, mcx_col_summary *cols, double *quantiles)
{
  MCXCHK(store_enter(s));
  return summary_span(s->st, s->bufs(), s->span(), probs, nprobs, cols, quantiles);
}

extern "C" int mcx_store_rank_summary(mcx_store *s, mcx_col_rank_summary *cols)
{
  MCXCHK(store_enter(s));
  return rank_span(s->st, s->bufs(), s->span(), cols);
}

extern "C" int mcx_store_covariance(mcx_store *s, double *mean, double *cov, int *flags)
{
  MCXCHK(store_enter(s));
  return covariance_span(s->st, s->bufs(), s->span(), mean, cov, flags);
}

extern "C" int mcx_store_density(mcx_store *s, const mcx_density_spec *spec, mcx_col_density *cols, double *x, double *y)
{
  MCXCHK(store_enter(s));
  return density_span(s->st, s->bufs(), s->span(), spec, cols, x, y);
}

extern "C" int mcx_store_density2d(mcx_store *s, const mcx_density2d_spec *spec, mcx_col_density *cols, double *axes,
                                   mcx_pair_density *pairs_out, double *z)
{
  MCXCHK(store_enter(s));
  return density2d_span(s->st, s->bufs(), s->span(), spec, cols, axes, pairs_out, z);
}

// mcx_store_density with its stages timed (mcx_debug_density_times' ms[4]), for tools/density_bench.py; the results are let go
extern "C" int mcx_debug_store_density_times(mcx_store *s, const mcx_density_spec *spec, double *ms)
{
  MCXCHK(store_enter(s));
  if (!ms || !spec) return fail(MCX_ERR_INVALID, "ms or the density spec is NULL");
  const size_t ncol = (size_t)s->nout + 1, n = (size_t)std::max(spec->n, 1);
  std::vector<mcx_col_density> cols(ncol);
  std::vector<double> x(ncol * n), y(ncol * n);
  return density_span(s->st, s->bufs(), s->span(), spec, cols.data(), x.data(), y.data(), ms);
}

extern "C" int mcx_samples_draw(mcx_engine *e, int first_step, int nsteps, uint32_t seed, int64_t ndraw, float *rows, int64_t *index)
{
  return on_store(
      e, first_step, nsteps,
      [&] {
        MCXCHK(draw_args(ndraw, rows));
        return range_args(nsteps);
      },
      [&](hipStream_t st, Bufs, const StoreView &v) { return gather_to_host<true>(st, v, seed, 0, (uint64_t)ndraw, rows, index); });
}

extern "C" int mcx_store_draw(mcx_store *s, uint32_t seed, int64_t ndraw, float *rows, int64_t *index)
{
  MCXCHK(store_enter(s));
  MCXCHK(draw_args(ndraw, rows));
  return gather_to_host<true>(s->st, s->span(), seed, 0, (uint64_t)ndraw, rows, index);
}

// host only
extern "C" int mcx_debug_draw_indices(uint32_t seed, uint64_t N, uint64_t first, int n, int64_t *index)
{
  if (N < 1 || n < 0 || (n > 0 && !index)) return fail(MCX_ERR_INVALID, "N = %llu, n = %d: N >= 1, n >= 0, index not NULL", (unsigned long long)N, n);
  if (N > (uint64_t)1 << 63) return fail(MCX_ERR_INVALID, "N = %llu: at most 2^63 rows (an index is an int64_t)", (unsigned long long)N);
  for (int k = 0; k < n; ++k) index[k] = (int64_t)draw_index(seed, first + (uint64_t)k, N);
  return MCX_OK;
}

// host only: the functions the launch code calls, on a shape
extern "C" int mcx_debug_store_geometry(int np, int nout, int nsteps, int nc, mcx_store_geometry *g)
{
  if (!g) return fail(MCX_ERR_INVALID, "g is NULL");
  if (np < 1 || np > DERIVE_MAXW) return fail(MCX_ERR_INVALID, "np = %d: 1 to %d parameters", np, DERIVE_MAXW);
  if (nout < 0 || nout > DERIVE_MAXW) return fail(MCX_ERR_INVALID, "nout = %d: 0 (no derive) to %d outputs", nout, DERIVE_MAXW);
  if (nsteps < 1 || nc < 1) return fail(MCX_ERR_INVALID, "nsteps = %d, nc = %d: at least one step of one chain", nsteps, nc);
  const uint64_t N = (uint64_t)nsteps * (uint64_t)nc;
  g->nrows = (long long)N;
  g->derive_rows = derive_rows(np, nout);
  g->derive_lds_bytes = (long long)derive_lds_floats(np, nout, (int)g->derive_rows) * (long long)sizeof(float);
  g->derive_workgroups = (long long)sweep_tiles(N, (int)g->derive_rows);
  const ClipGeometry c = clip_geometry(np, N);
  g->clip_rows = c.R;
  g->clip_mask_words = c.wpw;
  g->clip_lds_bytes = (long long)c.lds_bytes;
  g->clip_workgroups = (long long)c.nwg;
  g->clip_scan_blocks = (long long)c.nb;
  const RankGeometry r = rank_geometry(nsteps, (int64_t)N);
  g->rank_tiles = (long long)r.nblk;
  g->rank_step_chunk = (long long)r.rchunk;
  g->rank_grid_y = (long long)r.chunks;
  g->gather_chunk_rows = (long long)gather_chunk_rows(N, (uint64_t)np + 1);
  return MCX_OK;
}

// host only: DevBuf::alloc reads the setting (mcx_engine_internal.hpp)
extern "C" int mcx_debug_fill_allocations(int byte, unsigned long long *nfilled)
{
  if (byte < -1 || byte > 255) return fail(MCX_ERR_INVALID, "byte = %d: -1 (off) or 0 to 255", byte);
  g_alloc_fill.store(byte, std::memory_order_relaxed);
  const unsigned long long n = g_alloc_filled.exchange(0, std::memory_order_relaxed);
  if (nfilled) *nfilled = n;
  return MCX_OK;
}

// the analyses' scratch of an engine (summ_d, summ_h, summ_u) or of a store (d, h, u), to its capacity, on the owner's stream
extern "C" int mcx_debug_fill_scratch(mcx_engine *e, mcx_store *s, int byte, size_t bytes[3])
{
  if (!e == !s) return fail(MCX_ERR_INVALID, "exactly one of the engine e and the store s is given, not %s", e ? "both" : "neither");
  if (byte < 0 || byte > 255) return fail(MCX_ERR_INVALID, "byte = %d: 0 to 255", byte);
  if (e) MCXCHK(enter(e));
  else MCXCHK(store_enter(s));
  const hipStream_t st = e ? e->stream : (hipStream_t)s->st;
  const Bufs B = e ? Bufs{&e->summ_d, &e->summ_h, &e->summ_u} : s->bufs();
  void *const p[3] = {B.d->p, B.h->p, B.u->p};
  const size_t nb[3] = {B.d->p ? B.d->n * sizeof(double) : 0, B.h->p ? B.h->n * sizeof(unsigned long long) : 0,
                        B.u->p ? B.u->n * sizeof(uint32_t) : 0};
  for (int k = 0; k < 3; ++k) {
    if (nb[k]) HIPCHK(hipMemsetAsync(p[k], byte, nb[k], st));
    if (bytes) bytes[k] = nb[k];
  }
  HIPCHK(hipStreamSynchronize(st));
  return MCX_OK;
}

// the compile step alone (needs no GPU: hiprtc cross-compiles for gfx950)
extern "C" int mcx_debug_derive_compile(const char *source, int np, int nout, size_t *code_bytes)
{
  if (!source || !*source) return fail(MCX_ERR_INVALID, "source is NULL or empty");
  if (np < 1 || np > DERIVE_MAXW) return fail(MCX_ERR_INVALID, "np = %d: 1 to %d parameters", np, DERIVE_MAXW);
  if (nout < 1 || nout > DERIVE_MAXW) return fail(MCX_ERR_INVALID, "nout = %d: 1 to %d outputs", nout, DERIVE_MAXW);
  std::lock_guard<std::mutex> lk(rtc_lock());
  std::vector<char> code;
  MCXCHK(derive_compile(source, np, nout, code));
  if (code_bytes) *code_bytes = code.size();
  return MCX_OK;
}
