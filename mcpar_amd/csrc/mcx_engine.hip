// mcx_engine.hip -- host side of libmcx.so: the C ABI of include/mcx.h but mcx_run (mcx_run.hip): error plumbing, device
// information, create / destroy / options, likelihood and covariance set-up, getters, sample accessors, debug entry points.
//
// There is no CPU compute path in this file: every entry point that computes anything needs a
// HIP device and returns MCX_ERR_NO_DEVICE without one.
#include "mcx_engine_internal.hpp"


// ---------------------------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------------------------
static thread_local std::string g_err;

int fail(int code, const char *fmt, ...)
{
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

extern "C" const char *mcx_last_error(void) { return g_err.c_str(); }
extern "C" int mcx_abi_version(void) { return MCX_ABI_VERSION; }


int need_device()
{
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n < 1)
    return fail(MCX_ERR_NO_DEVICE, "no HIP device visible (%s); libmcx has no CPU fallback",
                e == hipSuccess ? "count = 0" : hipGetErrorString(e));
  return MCX_OK;
}

extern "C" int mcx_set_device(int device)
{
  MCXCHK(need_device());
  HIPCHK(hipSetDevice(device));
  return MCX_OK;
}

extern "C" int mcx_device_info(char *name, size_t namelen, int *cu_count, size_t *hbm_bytes)
{
  MCXCHK(need_device());
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  hipDeviceProp_t p;
  HIPCHK(hipGetDeviceProperties(&p, dev));
  if (name && namelen) snprintf(name, namelen, "%s (%s)", p.name, p.gcnArchName);
  if (cu_count) *cu_count = p.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = p.totalGlobalMem;
  return MCX_OK;
}

// ---------------------------------------------------------------------------------------------
// small helpers
// ---------------------------------------------------------------------------------------------
// Cholesky factor, lower, row-major, strict upper triangle zeroed: the role of spotrf('U') on the
// column-major view in MCPar::covar_setup (src/mcpar.cc:470-480).  Host side, np <= 32, once per run.  Returns 0, or
// 1 + the index of the pivot that is not > 0 (mcx_proposal_from_cov asks the same function for its verdict).
// mcx_lagcov_host.hpp has this function operation by operation in double (a log-determinant to nine digits, DESIGN.md section
// 24): a change to the loops or to the pivot test here belongs there too.
int cholesky_lower(int d, float *a)
{
  for (int i = 0; i < d; ++i) {
    for (int j = 0; j <= i; ++j) {
      float s = a[i * d + j];
      for (int k = 0; k < j; ++k) s = std::fmaf(-a[i * d + k], a[j * d + k], s);
      if (i == j) {
        if (!(s > 0.0f)) return i + 1;
        a[i * d + i] = std::sqrt(s);
      } else {
        a[i * d + j] = s / a[j * d + j];
      }
    }
    for (int j = i + 1; j < d; ++j) a[i * d + j] = 0.0f;
  }
  return 0;
}

// uploads asynchronously on st; the caller synchronises before L.host is touched again
int lik_setup(LikDev &L, const mcx_vlfunc *f, int np, hipStream_t st)
{
  if (!f) return fail(MCX_ERR_INVALID, "vlfunc is NULL");
  if (f->d != np) return fail(MCX_ERR_INVALID, "vlfunc.d = %d but engine np = %d", f->d, np);
  const int d = f->d;
  std::vector<float> h;
  L.fn = nullptr;
  L.ctx = nullptr;
  L.ncomp = 0;
  switch (f->kind) {
  case MCX_VL_ROSENBROCK1:
    if (d < 2 || (d & 1))  // src/rosenbrock.hh:13-16
      return fail(MCX_ERR_INVALID, "N for Rosenbrock1 must be even and >= 2");
    L.kind = LIK_ROSEN1;
    break;
  case MCX_VL_ROSENBROCK2:
    if (d < 2) return fail(MCX_ERR_INVALID, "N for Rosenbrock2 must be >= 2");  // src/rosenbrock.hh:27-30
    L.kind = LIK_ROSEN2;
    break;
  case MCX_VL_ROSENBROCK2_FIXED:
    if (d < 2) return fail(MCX_ERR_INVALID, "N for Rosenbrock2 must be >= 2");
    L.kind = LIK_ROSEN2F;
    break;
  case MCX_VL_GAUSSIAN:
    L.kind = LIK_GAUSS;
    h.resize(2 * (size_t)d);
    for (int k = 0; k < d; ++k) {  // src/rosenbrock.hh:44-47
      h[k] = f->params ? f->params[k] : 0.0f;
      h[d + k] = f->params ? 1.0f / f->params[d + k] : 1.0f;
    }
    break;
  case MCX_VL_DUALGAUSS: {
    if (d != 2) return fail(MCX_ERR_INVALID, "DualGaussian is two-dimensional");
    if (!f->params) return fail(MCX_ERR_INVALID, "DualGaussian needs params[0] = w");
    L.kind = LIK_MIX;
    L.ncomp = 2;
    const float m[4] = {0.0f, 0.0f, 5.0f, 5.0f};  // src/rosenbrock.cc:71-72
    h.assign(m, m + 4);
    h.push_back(logf_v1(f->params[0]));
    h.push_back(0.0f);
    break;
  }
  case MCX_VL_GAUSSMIX: {
    const int K = f->ncomp;
    if (K < 1 || K > 64 || !f->params) return fail(MCX_ERR_INVALID, "GAUSSMIX needs 1 <= K <= 64 and params");
    L.kind = LIK_MIX;
    L.ncomp = K;
    h.assign(f->params, f->params + (size_t)K * d);
    for (int c = 0; c < K; ++c) h.push_back(logf_v1(f->params[(size_t)K * d + c]));
    break;
  }
  case MCX_VL_HOST:
    if (!f->fn) return fail(MCX_ERR_VLFUNC, "MCX_VL_HOST without a callback");
    L.kind = MCX_VL_HOST;
    L.fn = f->fn;
    L.ctx = f->ctx;
    break;
  case MCX_VL_DEVICE:
    if (!f->ctx) return fail(MCX_ERR_VLFUNC, "MCX_VL_DEVICE without a kernel (hipFunction_t in ctx)");
    L.kind = MCX_VL_DEVICE;
    L.ctx = f->ctx;
    break;
  case MCX_VL_SOURCE: {
    if (f->ncomp < 0 || (f->ncomp > 0 && !f->params)) return fail(MCX_ERR_INVALID, "MCX_VL_SOURCE: ncomp floats of params expected");
    MCXCHK(user_lik_get(static_cast<const char *>(f->ctx), d, &L.user));  // (cached: compiled on first use)
    L.kind = LIK_USER;
    L.ncomp = f->ncomp;
    h.assign(f->params, f->params + (f->params ? f->ncomp : 0));
    if (h.empty()) h.push_back(0.0f);  // `par` is never a null pointer on the device
    break;
  }
  default:
    return fail(MCX_ERR_INVALID, "unknown vlfunc kind %d", f->kind);
  }
  if (L.params.p && h.size() == L.host.size() && (h.empty() || std::memcmp(h.data(), L.host.data(), h.size() * sizeof(float)) == 0))
    return MCX_OK;  // same parameters as the last call: they are on the device already
  HIPCHK(hipStreamSynchronize(st));  // (the last upload, or a run still in flight, may be reading L.host / L.params)
  L.host.swap(h);
  MCXCHK(L.params.alloc(L.host.size()));
  if (!L.host.empty())
    HIPCHK(hipMemcpyAsync(L.params.p, L.host.data(), L.host.size() * sizeof(float), hipMemcpyHostToDevice, st));
  return MCX_OK;
}

template <int LPC>
static int launch_eval(int lik, const float *x, float *y, int n, int d, const float *params,
                       int ncomp, int vec4, hipStream_t st)
{
  const dim3 grid(nblocks((size_t)n * LPC)), block(BLOCK);
  switch (lik) {
  case LIK_ROSEN1:
    hipLaunchKernelGGL((k_eval<LPC, LIK_ROSEN1>), grid, block, 0, st, x, y, n, d, params, ncomp, vec4);
    break;
  case LIK_GAUSS:
    hipLaunchKernelGGL((k_eval<LPC, LIK_GAUSS>), grid, block, 0, st, x, y, n, d, params, ncomp, vec4);
    break;
  case LIK_MIX:
    hipLaunchKernelGGL((k_eval<LPC, LIK_MIX>), grid, block, 0, st, x, y, n, d, params, ncomp, vec4);
    break;
  case LIK_ROSEN2F:
    hipLaunchKernelGGL((k_eval<LPC, LIK_ROSEN2F>), grid, block, 0, st, x, y, n, d, params, ncomp, vec4);
    break;
  case LIK_ROSEN2:
    hipLaunchKernelGGL(k_eval_rosen2, dim3(nblocks((size_t)n)), block, 0, st, x, y, n, d);
    break;
  default:
    return fail(MCX_ERR_INVALID, "likelihood %d has no device kernel", lik);
  }
  HIPCHK(hipGetLastError());
  return MCX_OK;
}

int eval_device(const LikDev &L, const float *x, float *y, int n, int d, hipStream_t st)
{
  if (L.kind == LIK_USER) return user_lik_launch_eval(*L.user, x, y, n, d, L.params.p, L.ncomp, st);
  const int lpc = lpc_for(d), vec4 = (d % 4 == 0);
  DISPATCH_LPC(lpc, MCXCHK((launch_eval<LPC_>(L.kind, x, y, n, d, L.params.p, L.ncomp, vec4, st))));
  return MCX_OK;
}

void prof_collect(mcx_engine *e)
{
  for (auto &p : e->evs) {
    float ms = 0.0f;
    (void)hipEventSynchronize(p.b);
    if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      e->prof.ms[p.kind] += ms;
      e->prof.launches[p.kind] += 1;
      e->prof.chain_steps[p.kind] += p.chain_steps;
    }
  }
  e->evs.clear();
}

extern "C" int mcx_create(mcx_engine **out, int np, int nc, int nshards, int shard, float pl,
                          float armin, float armax, float dfac, float ifac, int sync, uint32_t seed)
{
  if (!out) return fail(MCX_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (np < 1 || nc < 1 || nshards < 1 || shard < 0 || shard >= nshards || sync < 1)
    return fail(MCX_ERR_INVALID, "bad problem size np=%d nc=%d nshards=%d shard=%d sync=%d", np, nc,
                nshards, shard, sync);
  if (np > MAXD) return fail(MCX_ERR_UNSUPPORTED, "np = %d > %d is not supported", np, MAXD);
  if ((long long)nshards * nc > 0x7fffffffLL / (2LL * np))
    return fail(MCX_ERR_INVALID, "tchains*np*2 overflows int32 (the reference indexes musigall with int)");
  MCXCHK(need_device());
  mcx_engine *e = new mcx_engine();
  if (hipGetDevice(&e->device) != hipSuccess) e->device = 0;
  if (hipDeviceGetAttribute(&e->ncu, hipDeviceAttributeMultiprocessorCount, e->device) != hipSuccess) e->ncu = 0;
  e->nparam = np; e->nchain = nc; e->ntot = np * nc; e->ncov = np * np;
  e->size = nshards; e->rank = shard; e->tchains = nshards * nc;
  e->PLOCAL = pl; e->TGT_ARATE_MIN = armin; e->TGT_ARATE_MAX = armax;
  e->SCALE_DEC = dfac; e->SCALE_INC = ifac; e->SYNCSTEP = sync; e->seed = seed;
  e->lpc = lpc_for(np);
  e->vec4 = (np % 4 == 0);
  const size_t nt = (size_t)e->ntot, n = (size_t)nc;
  int st = MCX_OK;
  auto A = [&](int s) { if (st == MCX_OK) st = s; };
  A(e->pvals.alloc(nt)); A(e->ptrial.alloc(nt)); A(e->mu.alloc(nt)); A(e->sig.alloc(nt));
  A(e->psum2.alloc(nt)); A(e->mutrial.alloc(nt)); A(e->sigtrial.alloc(nt));
  A(e->musigall.alloc(2 * (size_t)e->tchains * np)); A(e->winvall.alloc(2 * (size_t)e->tchains * np));
  A(e->lylast.alloc(n)); A(e->lytrial.alloc(n)); A(e->cfac.alloc(n)); A(e->cmax.alloc(n));
  A(e->cov.alloc((size_t)e->ncov)); A(e->cov0.alloc((size_t)e->ncov)); A(e->trace.alloc(256)); A(e->acc_cnt.alloc(n));
  A(e->ctr.alloc((size_t)CTR_WORDS * CTR_RING + 2));  // (+ RunArgs::report_done, behind the ring)
  e->nslots = (int)(((size_t)nc * e->lpc + 63) / 64);
  A(e->acc_slots.alloc((size_t)e->nslots));
  A(e->tun_cells.alloc(TUN_CELLS + 1));
  if (st == MCX_OK && hipMemset(e->tun_cells.p, 0, (TUN_CELLS + 1) * sizeof(unsigned long long)) != hipSuccess)
    st = fail(MCX_ERR_HIP, "hipMemset failed");
  A(e->active0.alloc(n)); A(e->active1.alloc(n)); A(e->ntrace.alloc(1));
  A(e->nact.alloc(MurrayCounters::DEVICE_INTS));
  if (st == MCX_OK && hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess)
    st = fail(MCX_ERR_HIP, "hipStreamCreate failed");
  if (st != MCX_OK) { mcx_destroy(e); return st; }
  e->own_stream = true;
  (void)hipMemsetAsync(e->musigall.p, 0, 2 * (size_t)e->tchains * np * sizeof(float), e->stream);
  (void)hipMemsetAsync(e->mu.p, 0, nt * sizeof(float), e->stream);
  (void)hipMemsetAsync(e->sig.p, 0, nt * sizeof(float), e->stream);
  (void)hipMemsetAsync(e->psum2.p, 0, nt * sizeof(float), e->stream);
  (void)hipMemsetAsync(e->acc_cnt.p, 0, n * sizeof(uint32_t), e->stream);
  (void)hipMemsetAsync(e->acc_slots.p, 0, (size_t)e->nslots * sizeof(uint32_t), e->stream);  // (every run leaves them zero)
  (void)hipMemsetAsync(e->ntrace.p, 0, sizeof(int), e->stream);
  // identity factor until covar_setup / run installs one (src/mcpar.cc:460-467)
  std::vector<float> eye((size_t)e->ncov, 0.0f);
  for (int i = 0; i < np; ++i) eye[(size_t)i * (np + 1)] = 1.0f;
  (void)hipMemcpyAsync(e->cov.p, eye.data(), eye.size() * sizeof(float), hipMemcpyHostToDevice, e->stream);
  (void)hipMemcpyAsync(e->cov0.p, eye.data(), eye.size() * sizeof(float), hipMemcpyHostToDevice, e->stream);
  e->h_cov_dev = eye;
  (void)hipMemsetAsync(e->ctr.p, 0, ((size_t)CTR_WORDS * CTR_RING + 2) * sizeof(unsigned long long), e->stream);
  if (hipStreamSynchronize(e->stream) != hipSuccess) {
    mcx_destroy(e);
    return fail(MCX_ERR_HIP, "engine initialisation failed");
  }
  *out = e;
  return MCX_OK;
}

// Every buffer, stream and event of the engine is a member that releases itself: `delete e` gives them back.  What is
// left here is order alone: nothing may still be running on, or waiting for, what is about to go.
extern "C" int mcx_destroy(mcx_engine *e)
{
  if (!e) return MCX_OK;
  (void)hipSetDevice(e->device);
  e->tail_publish = 0;  // (nobody will look at the slot; the gather itself is waited for by mcx_exchange_rccl_destroy)
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  e->pend.active = false;  // (a run nobody waited for: over now; its results go with the engine)
  if (e->meet_held) { (void)flock(e->meet_fd, LOCK_UN); e->meet_held = false; }
  if (e->astream) (void)hipStreamSynchronize(e->astream);
  prof_collect(e);
  (void)mcx_exchange_rccl_destroy(e);  // (finish_tail needs a live stream)
  if (e->meet_fd >= 0) (void)close(e->meet_fd);
  if (e->own_stream && e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
  return MCX_OK;
}


extern "C" int mcx_set_exchange(mcx_engine *e, mcx_exchange_fn fn, void *ctx)
{
  if (!e) return fail(MCX_ERR_INVALID, "engine is NULL");
  if (e->pend.active) MCXCHK(enter(e));
  MCXCHK(finish_tail(e));  // (a gather of the exchange being replaced may still be in flight)
  e->xfn = fn;
  e->xctx = ctx;
  return MCX_OK;
}

extern "C" int mcx_set_output_hook(mcx_engine *e, mcx_output_fn fn, void *ctx)
{
  if (!e) return fail(MCX_ERR_INVALID, "engine is NULL");
  e->ofn = fn;
  e->octx = ctx;
  return MCX_OK;
}

extern "C" int mcx_set_option(mcx_engine *e, int opt, int64_t value)
{
  if (!e) return fail(MCX_ERR_INVALID, "engine is NULL");
  if (e->pend.active) MCXCHK(enter(e));  // (options apply to whole runs: the one in flight is finished first)
  switch (opt) {
  case MCX_OPT_SAMPLES: e->opt_samples = value ? 1 : 0; break;
  case MCX_OPT_SAMPLE_STRIDE:
    if (value < 1) return fail(MCX_ERR_INVALID, "SAMPLE_STRIDE must be >= 1");
    e->opt_stride = (int)std::min<int64_t>(value, 1 << 30);
    break;
  case MCX_OPT_ACCEPT_MASK: e->opt_mask = value ? 1 : 0; break;
  case MCX_OPT_FUSE: e->opt_fuse = value ? 1 : 0; break;
  case MCX_OPT_MAX_SEGMENT:
    if (value < 1) return fail(MCX_ERR_INVALID, "MAX_SEGMENT must be >= 1");
    e->opt_maxseg = (int)std::min<int64_t>(value, 1 << 20);
    break;
  case MCX_OPT_PROFILE: e->opt_profile = value ? 1 : 0; break;
  case MCX_OPT_EAGER_EXCHANGE: e->opt_eager = value ? 1 : 0; break;
  case MCX_OPT_SINK_TEXT: e->opt_sink_text = value ? 1 : 0; break;
  case MCX_OPT_ASYNC_TAIL: e->opt_async_tail = value == 2 ? 2 : (value ? 1 : 0); break;
  case MCX_OPT_SPLIT_RNG: e->opt_split = value < 0 ? -1 : (value ? 1 : 0); break;
  case MCX_OPT_PERSIST: e->opt_persist = value < 0 ? -1 : (value ? 1 : 0); break;
  case MCX_OPT_CULL: e->opt_cull = value < 0 ? -1 : ((value == 2 || value == 3) ? value : (value ? 1 : 0)); break;
  case MCX_OPT_BLOCKS_PER_LANE:
    if (value != 0 && value != 1 && value != 2 && value != 4) return fail(MCX_ERR_INVALID, "BLOCKS_PER_LANE must be 0 (auto), 1, 2 or 4");
    e->opt_bpl = (int)value;
    break;
  case MCX_OPT_MEET_TIMEOUT_MS:
    if (value < 1) return fail(MCX_ERR_INVALID, "MEET_TIMEOUT_MS must be >= 1");
    e->opt_meet_timeout_ms = (int)std::min<int64_t>(value, 600000);
    break;
  case MCX_OPT_ASYNC_RUN: e->opt_async_run = value ? 1 : 0; break;
  case MCX_OPT_REFERENCE_CALLS: e->opt_reference_calls = value ? 1 : 0; break;
  case MCX_OPT_SELF_REPORT: e->opt_self_report = value ? 1 : 0; break;
  case MCX_OPT_MURRAY_OVERLAP:
    if (value < 0 || value > 64) return fail(MCX_ERR_INVALID, "MURRAY_OVERLAP: 0 (off) or the number of column chunks, <= 64");
    e->opt_murray_overlap = (int)value;
    break;
  case MCX_OPT_MURRAY_MAX_PASSES:
    e->opt_murray_max_passes = value <= 0 ? MURRAY_MAX_PASSES_DEFAULT : (int)std::min<int64_t>(value, MURRAY_MAX_PASSES_DEFAULT);
    break;
  case MCX_OPT_MEET_UNDER_GATHER: e->opt_meet_under_gather = value < 0 ? -1 : (value ? 1 : 0); break;
  case MCX_OPT_DEBUG_MEET:
    e->opt_debug_meet = (int)std::max<int64_t>(0, std::min<int64_t>(value, 1 << 20));
    e->persist_broken = false;  // (a test switching the hook off again gets the one-launch kernel back)
    break;
  case MCX_OPT_STREAM:
    if (e->own_stream && e->stream) {
      (void)hipStreamSynchronize(e->stream);
      (void)hipStreamDestroy(e->stream);
    }
    e->stream = (hipStream_t)(uintptr_t)value;
    e->own_stream = false;
    break;
  default: return fail(MCX_ERR_INVALID, "unknown option %d", opt);
  }
  return MCX_OK;
}

// MCPar::covar_setup (src/mcpar.cc:454-484)
int covar_install(mcx_engine *e, const float *incov, float *cov_out, bool sync)
{
  const int d = e->nparam;
  std::vector<float> &c = e->h_cov;
  c.assign((size_t)e->ncov, 0.0f);
  if (incov) std::copy(incov, incov + e->ncov, c.begin());
  else
    for (int i = 0; i < d; ++i) c[(size_t)i * (d + 1)] = 1.0f;
  if (cholesky_lower(d, c.data()) != 0)
    return fail(MCX_ERR_INVALID, "covariance matrix is not positive definite");
  e->diag = true;
  for (int i = 0; i < d; ++i)
    for (int j = 0; j < i; ++j)
      if (c[(size_t)i * d + j] != 0.0f) e->diag = false;
  // cov0 keeps the factor as installed; cov (which the tuner rescales) is reset from it, on the device
  if (e->h_cov_dev != c) {
    if (!e->h_cov_dev.empty()) HIPCHK(hipStreamSynchronize(e->stream));  // the last upload may still read h_cov_dev
    e->h_cov_dev = c;
    HIPCHK(hipMemcpyAsync(e->cov0.p, e->h_cov_dev.data(), c.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
  }
  if (sync) {
    HIPCHK(hipMemcpyAsync(e->cov.p, e->cov0.p, c.size() * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->cov_pending = false;
    e->cov_offdiag = !e->diag;
  } else {
    e->cov_pending = true;  // the run resets it: k_run_small reads cov0 itself, every other path copies first
  }
  if (cov_out) std::copy(c.begin(), c.end(), cov_out);
  return MCX_OK;
}

extern "C" int mcx_covar_setup(mcx_engine *e, const float *incov, float *cov)
{
  MCXCHK(enter(e));
  if (!e) return fail(MCX_ERR_INVALID, "engine is NULL");
  return covar_install(e, incov, cov);
}

// Base pointers such that kept step r = isamp / stride of the run lives at base + r * rowsize: the whole-run
// store itself, or -- in sink mode -- the ring slot of isamp's block shifted back by the block's first row
// (kernels index rows of the run; a launch never straddles a block).
void samp_vbase(const mcx_engine *e, int isamp, float **px, float **pl)
{
  if (!e->run_sink) { *px = e->samp_x.p; *pl = e->samp_ly.p; return; }
  const long long b = isamp / e->run_sblock, slot = b % SINK_RING, shift = (slot - b) * (long long)e->run_kb;
  *px = e->samp_x.p + shift * (long long)e->ntot;
  *pl = e->samp_ly.p + shift * (long long)e->nchain;
}

// the one-launch small-n kernel's generator deal (mcxk_persist_deal) and steps per phase, for tests: host logic only
extern "C" int mcx_debug_persist_deal(int lpc2, int bpl, int own, int *rec, int *ksteps, uint32_t *tab, int max_words)
{
  if (lpc2 < 1 || lpc2 > 8 || (bpl != 1 && bpl != 2 && bpl != 4) || own < 1 || own > POWN_MAX || !rec || !ksteps || !tab ||
      max_words < MCXK_PERSIST_DEAL_WORDS)
    return fail(MCX_ERR_INVALID, "bad arguments");
  *rec = mcxk_persist_recorders(own, bpl) ? 1 : 0;
  *ksteps = mcxk_persist_ksteps(lpc2, bpl, own);
  mcxk_persist_deal(lpc2, bpl, own, *rec, *ksteps, tab);
  return MCX_OK;
}

extern "C" int mcx_debug_step_instances(mcx_engine *e, uint32_t *ids, int cap, int *n)
{
  if (!e || !n || cap < 0 || (cap > 0 && !ids)) return fail(MCX_ERR_INVALID, "bad arguments");
  if (e->steps.lost) return fail(MCX_ERR_UNSUPPORTED, "more than %d distinct step-kernel instances in one run", StepLedger::CAP);
  *n = e->steps.n;
  for (int i = 0; i < e->steps.n && i < cap; ++i) ids[i] = e->steps.ids[i];
  return MCX_OK;
}

// Every instance the launchers can launch: their own switches, driven over the whole small argument space with a dry
// ledger (mcx_launch.hpp), which makes each launcher return where it would launch.  No table is kept here: an
// instantiation added to a launcher shows up by itself.  No device call on the way.
extern "C" int mcx_debug_step_instance_list(uint32_t *ids, int cap, int *n)
{
  if (!n || cap < 0 || (cap > 0 && !ids)) return fail(MCX_ERR_INVALID, "bad arguments");
  std::vector<uint32_t> all;
  auto take = [&](StepLedger &l) {
    for (int i = 0; i < l.n; ++i)
      if (std::find(all.begin(), all.end(), l.ids[i]) == all.end()) all.push_back(l.ids[i]);
    l.n = 0;
  };
  static float somewhere[4];  // (never dereferenced: the launchers only ask whether rows / a trash row are wanted)
  StepLedger l;
  l.dry = true;
  for (int lpc = 1; lpc <= 64; lpc <<= 1) {
    for (int lik = 0; lik <= LIK_USER; ++lik)
      for (int main = 0; main < 2; ++main) {
        for (int rows = 0; rows < 2; ++rows)
          for (int stride = 1; stride <= 3; stride += 2) {
            SegArgs a{};
            a.n = 1; a.d = 4 * lpc; a.nsteps = 1;
            a.samp_x = a.samp_ly = rows ? somewhere : nullptr;
            a.samp_stride = stride;
            a.trash = somewhere;
            (void)mcxk_launch_fast(lpc, lik, main != 0, a, nullptr, &l);
            for (int bpl = 1; bpl <= 4; bpl <<= 1) (void)mcxk_launch_fastb(lpc, bpl, lik, main != 0, a, nullptr, &l);
            (void)mcxk_launch_fast_full(lpc, lik, main != 0, a, nullptr, &l);
            (void)mcxk_launch_fastb_full(lpc, lik, main != 0, a, nullptr, &l);
            (void)mcxk_launch_fast_pregen(lpc, lik, main != 0, a, nullptr, &l);
            (void)(main ? mcxk_launch_generic_main(lpc, lik, a, nullptr, &l) : mcxk_launch_generic_burn(lpc, lik, a, nullptr, &l));
            take(l);
          }
        for (int bpl = 1; bpl <= 4; bpl <<= 1)
          for (int own = 1; own <= 2; ++own)
            for (int rec = -1; rec <= 1; ++rec) {  // the launcher's own rule, and both forced choices (MCX_PERSIST_REC)
              RunArgs r{};
              r.n = 1; r.d = 4 * lpc; r.own = own; r.nown = own; r.nburn = main ? 0 : 1; r.nmain = main;
              l.force_rec = rec;
              (void)mcxk_launch_persist(lpc, bpl, lik, r, nullptr, &l);
              take(l);
            }
        l.force_rec = -1;
      }
    (void)mcxk_launch_gen(lpc, nullptr, nullptr, 1, 4 * lpc, 1, 0, 0, 0, nullptr, &l);
    take(l);
  }
  *n = (int)all.size();
  for (int i = 0; i < *n && i < cap; ++i) ids[i] = all[i];
  return MCX_OK;
}

extern "C" int mcx_device_count(int *n)
{
  if (!n) return fail(MCX_ERR_INVALID, "n is NULL");
  *n = 0;
  MCXCHK(need_device());
  HIPCHK(hipGetDeviceCount(n));
  return MCX_OK;
}

extern "C" int mcx_device_pci_bus_id(char *buf, size_t len)
{
  if (!buf || len < 16) return fail(MCX_ERR_INVALID, "buffer too small");
  MCXCHK(need_device());
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  HIPCHK(hipDeviceGetPCIBusId(buf, (int)len, dev));
  return MCX_OK;
}

extern "C" int mcx_stage_pinit(mcx_engine *e, const float *pinit)
{
  MCXCHK(enter(e));
  if (!e || !pinit) return fail(MCX_ERR_INVALID, "bad arguments");
  MCXCHK(e->pinit_dev.alloc((size_t)e->ntot));
  HIPCHK(hipMemcpyAsync(e->pinit_dev.p, pinit, (size_t)e->ntot * sizeof(float), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  e->pinit_staged = true;
  return MCX_OK;
}

// ---------------------------------------------------------------------------------------------
// standalone operators on host buffers
// ---------------------------------------------------------------------------------------------
extern "C" int mcx_vlfunc_eval(const mcx_vlfunc *f, int npset, const float *x, float *y)
{
  if (!f || npset < 0 || (npset > 0 && (!x || !y))) return fail(MCX_ERR_INVALID, "bad arguments");
  if (f->d < 1 || f->d > MAXD) return fail(MCX_ERR_UNSUPPORTED, "d = %d outside 1..%d", f->d, MAXD);
  if (f->kind == MCX_VL_HOST) {
    if (!f->fn) return fail(MCX_ERR_VLFUNC, "MCX_VL_HOST without a callback");
    return f->fn(f->ctx, npset, x, y);
  }
  MCXCHK(need_device());
  LikDev L;
  DevBuf<float> dx, dy;
  hipStream_t st = nullptr;
  auto run = [&]() -> int {
    MCXCHK(lik_setup(L, f, f->d, st));
    if (npset == 0) return MCX_OK;
    MCXCHK(dx.alloc((size_t)npset * f->d));
    MCXCHK(dy.alloc((size_t)npset));
    HIPCHK(hipMemcpy(dx.p, x, (size_t)npset * f->d * sizeof(float), hipMemcpyHostToDevice));
    if (L.kind == MCX_VL_DEVICE) {
      const float *xa = dx.p;
      float *ya = dy.p;
      void *args[] = {&npset, &xa, &ya};
      HIPCHK(hipModuleLaunchKernel((hipFunction_t)L.ctx, nblocks((size_t)npset), 1, 1, BLOCK, 1, 1, 0, st, args, nullptr));
    } else {
      MCXCHK(eval_device(L, dx.p, dy.p, npset, f->d, st));
    }
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(y, dy.p, (size_t)npset * sizeof(float), hipMemcpyDeviceToHost));
    return MCX_OK;
  };
  const int rc = run();
  (void)hipDeviceSynchronize();  // the parameter upload reads L.host, which goes with L
  return rc;
}

extern "C" int mcx_gen_local(mcx_engine *e, uint32_t t, const float *pvals, float *ptrial, float *cfac)
{
  MCXCHK(enter(e));
  if (!e || !pvals || !ptrial || !cfac) return fail(MCX_ERR_INVALID, "bad arguments");
  hipStream_t st = e->stream;
  DevBuf<float> x;
  MCXCHK(x.alloc((size_t)e->ntot));
  HIPCHK(hipMemcpyAsync(x.p, pvals, (size_t)e->ntot * sizeof(float), hipMemcpyHostToDevice, st));
  StepArgs a;
  fill_step(e, a, t, 0, false, 0, 0, 0);
  a.x = x.p;
  a.mask = nullptr;
  MCXCHK(launch_propose(e, a));
  HIPCHK(hipMemcpyAsync(ptrial, e->ptrial.p, (size_t)e->ntot * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(cfac, e->cfac.p, (size_t)e->nchain * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return MCX_OK;
}

extern "C" int mcx_gen_remote(mcx_engine *e, uint32_t t, const float *pvals, const float *musigall,
                              float *ptrial, float *cfac, float *mutrial, float *sigtrial, int *npass)
{
  MCXCHK(enter(e));
  if (!e || !pvals || !musigall || !ptrial || !cfac) return fail(MCX_ERR_INVALID, "bad arguments");
  hipStream_t st = e->stream;
  DevBuf<float> x, ms;
  MCXCHK(x.alloc((size_t)e->ntot));
  MCXCHK(ms.alloc(2 * (size_t)e->tchains * e->nparam));
  HIPCHK(hipMemcpyAsync(x.p, pvals, (size_t)e->ntot * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(ms.p, musigall, 2 * (size_t)e->tchains * e->nparam * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(e->cfac.p, 0, (size_t)e->nchain * sizeof(float), st));
  MCXCHK(remote_device(e, t, x.p, ms.p, e->ptrial.p, e->cfac.p, e->mutrial.p, e->sigtrial.p, npass));
  HIPCHK(hipMemcpyAsync(ptrial, e->ptrial.p, (size_t)e->ntot * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(cfac, e->cfac.p, (size_t)e->nchain * sizeof(float), hipMemcpyDeviceToHost, st));
  if (mutrial) HIPCHK(hipMemcpyAsync(mutrial, e->mutrial.p, (size_t)e->ntot * sizeof(float), hipMemcpyDeviceToHost, st));
  if (sigtrial) HIPCHK(hipMemcpyAsync(sigtrial, e->sigtrial.p, (size_t)e->ntot * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return MCX_OK;
}

// ---------------------------------------------------------------------------------------------
// getters
// ---------------------------------------------------------------------------------------------
template <typename T>
static int d2h(mcx_engine *e, T *dst, const T *src, size_t count)
{
  if (!e || !dst) return fail(MCX_ERR_INVALID, "bad arguments");
  MCXCHK(enter(e));  // (also: an asynchronous run in flight is finished first)
  HIPCHK(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return MCX_OK;
}

extern "C" int mcx_get_counters(mcx_engine *e, mcx_counters *c)
{
  if (!e || !c) return fail(MCX_ERR_INVALID, "bad arguments");
  if (e->pend.active) MCXCHK(enter(e));  // (an asynchronous run's counters exist once it is over)
  *c = e->cnt;
  c->meet_timeouts_total = e->meet_total;
  return MCX_OK;
}
extern "C" int mcx_get_state(mcx_engine *e, float *v) { return d2h(e, v, e ? e->pvals.p : nullptr, e ? (size_t)e->ntot : 0); }
extern "C" int mcx_get_loglike(mcx_engine *e, float *v) { return d2h(e, v, e ? e->lylast.p : nullptr, e ? (size_t)e->nchain : 0); }
extern "C" int mcx_get_mean(mcx_engine *e, float *v) { return d2h(e, v, e ? e->mu.p : nullptr, e ? (size_t)e->ntot : 0); }
extern "C" int mcx_get_var(mcx_engine *e, float *v) { return d2h(e, v, e ? e->sig.p : nullptr, e ? (size_t)e->ntot : 0); }
extern "C" int mcx_get_musigall(mcx_engine *e, float *v)
{
  MCXCHK(enter(e));
  MCXCHK(finish_tail(e));
  return d2h(e, v, e->musigall.p, 2 * (size_t)e->tchains * e->nparam);
}

extern "C" int mcx_synchronize(mcx_engine *e)
{
  MCXCHK(enter(e));
  MCXCHK(finish_tail(e));
  HIPCHK(hipStreamSynchronize(e->stream));
  return MCX_OK;
}
extern "C" int mcx_get_chol(mcx_engine *e, float *v) { return d2h(e, v, e ? e->cov.p : nullptr, e ? (size_t)e->ncov : 0); }
extern "C" int mcx_get_accept_counts(mcx_engine *e, uint32_t *v) { return d2h(e, v, e ? e->acc_cnt.p : nullptr, e ? (size_t)e->nchain : 0); }

extern "C" int mcx_get_accept_mask(mcx_engine *e, uint8_t *mask)
{
  MCXCHK(enter(e));
  if (!e || !mask) return fail(MCX_ERR_INVALID, "bad arguments");
  if (!e->have_run || !e->opt_mask || !e->mask.p) return fail(MCX_ERR_INVALID, "no accept mask recorded (MCX_OPT_ACCEPT_MASK)");
  return d2h(e, mask, e->mask.p, (size_t)(e->last_nburn + e->last_nsamp) * e->nchain);
}

extern "C" int mcx_get_tuner_trace(mcx_engine *e, float *scales, int maxn, int *n)
{
  MCXCHK(enter(e));
  if (!e || !n) return fail(MCX_ERR_INVALID, "bad arguments");
  int nt = 0;
  MCXCHK(d2h(e, &nt, e->ntrace.p, 1));
  *n = nt;
  const int k = std::min(std::min(nt, maxn), 256);
  if (k > 0 && scales) MCXCHK(d2h(e, scales, e->trace.p, (size_t)k));
  return MCX_OK;
}

extern "C" int mcx_samples_steps(mcx_engine *e, int *nsteps)
{
  if (!e || !nsteps) return fail(MCX_ERR_INVALID, "bad arguments");
  *nsteps = e->samp_steps;
  return MCX_OK;
}

// Rows are interleaved into MCout's (np+1)-column layout on the device, moved through two pinned
// staging buffers (the D2H of chunk k+1 overlaps the host copy of chunk k) and land in the caller's
// pageable buffer.  Off the hot path: this is the MCout::add / collect side of the boundary.
extern "C" int mcx_samples_copy(mcx_engine *e, int first_step, int nsteps, float *rows)
{
  MCXCHK(enter(e));
  if (!e || !rows || first_step < 0 || nsteps < 0) return fail(MCX_ERR_INVALID, "bad arguments");
  if (first_step + nsteps > e->samp_steps) return fail(MCX_ERR_INVALID, "steps [%d,%d) not in the sample store (%d steps)", first_step, first_step + nsteps, e->samp_steps);
  const size_t n = (size_t)e->nchain, d = (size_t)e->nparam, ncol = d + 1, nr = (size_t)nsteps * n;
  if (nr == 0) return MCX_OK;
  const size_t chunk_rows = std::max<size_t>(1, std::min<size_t>(nr, ((size_t)32 << 20) / (ncol * sizeof(float))));
  DevBuf<float> stage[2];
  PinBuf<float> pin[2];
  DevEvent done[2];
  auto run = [&]() -> int {
    for (int b = 0; b < 2; ++b) {
      MCXCHK(stage[b].alloc(chunk_rows * ncol));
      MCXCHK(pin[b].alloc(chunk_rows * ncol));
      MCXCHK(done[b].ensure(hipEventDisableTiming));
    }
    const float *sx = e->samp_x.p + (size_t)first_step * n * d, *sl = e->samp_ly.p + (size_t)first_step * n;
    size_t issued = 0, copied = 0;
    int ib = 0, cb = 0;
    size_t rows_in[2] = {0, 0};
    while (copied < nr) {
      while (issued < nr && issued - copied < 2 * chunk_rows) {  // keep both buffers in flight
        const size_t r = std::min(chunk_rows, nr - issued);
        hipLaunchKernelGGL(k_rows_interleave, dim3(nblocks(r * ncol)), dim3(BLOCK), 0, e->stream, sx + issued * d,
                           sl + issued, stage[ib].p, r, (int)d);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(pin[ib].p, stage[ib].p, r * ncol * sizeof(float), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipEventRecord(done[ib], e->stream));
        rows_in[ib] = r;
        issued += r;
        ib ^= 1;
      }
      HIPCHK(hipEventSynchronize(done[cb]));
      std::memcpy(rows + copied * ncol, pin[cb].p, rows_in[cb] * ncol * sizeof(float));
      copied += rows_in[cb];
      cb ^= 1;
    }
    return MCX_OK;
  };
  const int rc = run();
  (void)hipStreamSynchronize(e->stream);  // (the pinned buffers are the target of copies that may still be in flight)
  return rc;
}

extern "C" int mcx_samples_maxlike(mcx_engine *e, float *lmax, float *params)
{
  MCXCHK(enter(e));
  if (!e || !lmax || !params) return fail(MCX_ERR_INVALID, "bad arguments");
  const size_t n = (size_t)e->nchain, d = (size_t)e->nparam;
  if (!e->run_sink) {  // arg-max over the whole HBM-resident store, on the device (first strict maximum, src/mcout.cc:140)
    const size_t nr = (size_t)e->samp_steps * n;
    if (nr == 0) return fail(MCX_ERR_INVALID, "sample store is empty");
    if (nr > 0xfffffff0ull) return fail(MCX_ERR_UNSUPPORTED, "sample store too large for the arg-max key");
    MCXCHK(e->best_row.alloc(d + 1));
    MCXCHK(e->best_key.alloc(1));
    hipLaunchKernelGGL(k_best_reset, dim3(nblocks(d + 1)), dim3(BLOCK), 0, e->stream, e->best_row.p, (int)d, e->best_key.p);
    hipLaunchKernelGGL(k_argmax_first, dim3(std::min<unsigned>(nblocks(nr), 2048u)), dim3(BLOCK), 0, e->stream, e->samp_ly.p, nr, e->best_key.p);
    hipLaunchKernelGGL(k_best_update, dim3(1), dim3(BLOCK), 0, e->stream, e->best_key.p, e->samp_ly.p, e->samp_x.p, (int)d, e->best_row.p);
    HIPCHK(hipGetLastError());
  } else if (!e->have_run) {
    return fail(MCX_ERR_INVALID, "sample store is empty");
  }
  std::vector<float> h(d + 1);
  MCXCHK(d2h(e, h.data(), e->best_row.p, d + 1));
  *lmax = h[0];
  std::copy(h.begin() + 1, h.end(), params);
  return MCX_OK;
}

extern "C" int mcx_get_profile(mcx_engine *e, mcx_profile *p)
{
  if (!e || !p) return fail(MCX_ERR_INVALID, "bad arguments");
  prof_collect(e);
  *p = e->prof;
  return MCX_OK;
}

extern "C" int mcx_copy_to_host(void *dst_host, const void *src_dev, size_t bytes, void *stream)
{
  if (!dst_host || !src_dev) return fail(MCX_ERR_INVALID, "bad arguments");
  MCXCHK(need_device());
  HIPCHK(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return MCX_OK;
}

extern "C" int mcx_copy_to_device(void *dst_dev, const void *src_host, size_t bytes, void *stream)
{
  if (!dst_dev || !src_host) return fail(MCX_ERR_INVALID, "bad arguments");
  MCXCHK(need_device());
  HIPCHK(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return MCX_OK;
}

// ---------------------------------------------------------------------------------------------
// numerics test hooks
// ---------------------------------------------------------------------------------------------
extern "C" int mcx_debug_numerics(int what, int n, const uint32_t *in, uint32_t *out_bits)
{
  if (n < 0 || (n > 0 && (!in || !out_bits))) return fail(MCX_ERR_INVALID, "bad arguments");
  MCXCHK(need_device());
  if (n == 0) return MCX_OK;
  DevBuf<uint32_t> di, dout;
  MCXCHK(di.alloc((size_t)n));
  MCXCHK(dout.alloc((size_t)n));
  HIPCHK(hipMemcpy(di.p, in, (size_t)n * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_debug_numerics, dim3(nblocks((size_t)n)), dim3(BLOCK), 0, 0, what, n, di.p, dout.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out_bits, dout.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  return MCX_OK;
}

extern "C" int mcx_debug_copy_bandwidth(size_t bytes, int reps, double *gbps)
{
  if (!gbps || bytes == 0 || reps <= 0) return fail(MCX_ERR_INVALID, "copy bandwidth: bytes > 0, reps > 0, gbps != NULL");
  DevBuf<unsigned char> a, b;
  MCXCHK(a.alloc(bytes));
  MCXCHK(b.alloc(bytes));
  DevEvent t0, t1;
  int rc = MCX_OK;
  float ms = 0.0f;
  do {
    if (hipMemset(a.p, 1, bytes) != hipSuccess || t0.ensure(hipEventDefault) != MCX_OK || t1.ensure(hipEventDefault) != MCX_OK ||
        hipMemcpyAsync(b.p, a.p, bytes, hipMemcpyDeviceToDevice, nullptr) != hipSuccess ||  // warm
        hipEventRecord(t0, nullptr) != hipSuccess) { rc = MCX_ERR_HIP; break; }
    for (int r = 0; r < reps && rc == MCX_OK; ++r)
      if (hipMemcpyAsync(b.p, a.p, bytes, hipMemcpyDeviceToDevice, nullptr) != hipSuccess) rc = MCX_ERR_HIP;
    if (rc != MCX_OK) break;
    if (hipEventRecord(t1, nullptr) != hipSuccess || hipEventSynchronize(t1) != hipSuccess ||
        hipEventElapsedTime(&ms, t0, t1) != hipSuccess || !(ms > 0.0f)) rc = MCX_ERR_HIP;
  } while (0);
  if (rc != MCX_OK) return fail(rc, "copy bandwidth: %s", hipGetErrorString(hipGetLastError()));
  *gbps = 2.0 * (double)bytes * reps / (ms * 1e-3) / 1e9;
  return MCX_OK;
}

extern "C" int mcx_debug_sqrt_sweep(uint32_t lo_bits, uint32_t hi_bits, uint64_t *nbad, uint32_t *first_bad)
{
  if (!nbad || !first_bad || hi_bits < lo_bits) return fail(MCX_ERR_INVALID, "bad arguments");
  MCXCHK(need_device());
  DevBuf<unsigned long long> dn;
  DevBuf<uint32_t> df;
  MCXCHK(dn.alloc(1));
  MCXCHK(df.alloc(1));
  const uint32_t init = 0xffffffffu;
  HIPCHK(hipMemset(dn.p, 0, sizeof(unsigned long long)));
  HIPCHK(hipMemcpy(df.p, &init, 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_debug_sqrt_sweep, dim3(4096), dim3(BLOCK), 0, 0, lo_bits, hi_bits, dn.p, df.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  unsigned long long n = 0;
  HIPCHK(hipMemcpy(&n, dn.p, sizeof n, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(first_bad, df.p, 4, hipMemcpyDeviceToHost));
  *nbad = n;
  return MCX_OK;
}

extern "C" int mcx_debug_normals(uint32_t seed, uint32_t stream, uint32_t t, uint32_t g0, uint32_t a,
                                 uint32_t q, int n, float *out)
{
  if (n < 0 || (n > 0 && !out)) return fail(MCX_ERR_INVALID, "bad arguments");
  MCXCHK(need_device());
  if (n == 0) return MCX_OK;
  DevBuf<float> d;
  MCXCHK(d.alloc((size_t)n * 4));
  hipLaunchKernelGGL(k_debug_normals, dim3(nblocks((size_t)n)), dim3(BLOCK), 0, 0, seed, stream, t, g0, a, q, n, d.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out, d.p, (size_t)n * 16, hipMemcpyDeviceToHost));
  return MCX_OK;
}

// what the owners of mcx_engine_internal.hpp hold at this moment, process-wide; needs no device
extern "C" int mcx_debug_live_resources(uint64_t out[4])
{
  if (!out) return fail(MCX_ERR_INVALID, "out is NULL");
  for (int i = 0; i < 4; ++i) out[i] = g_live[i].load(std::memory_order_relaxed);
  return MCX_OK;
}
