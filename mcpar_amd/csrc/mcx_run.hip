// mcx_run.hip -- mcx_run: the step-loop control that replaces MCPar::run (src/mcpar.cc:17-214) by a schedule of gfx950
// kernel launches.  The launch helpers of the per-segment kernels, the meeting lock of the one-launch small-n kernel,
// run_once (the plan executor) and the ends of a run: synchronous, asynchronous (finish_pending), repeated.
#include "mcx_engine_internal.hpp"


// Launch one segment of consecutive local steps.  Small-n mode (MCX_OPT_SPLIT_RNG): with few chains the
// fused kernel is bound by the latency of a single wave's instruction stream, two thirds of it random
// numbers that do not depend on the chain state; they are then generated for 32..256 steps at a time
// by a fully parallel kernel on the otherwise idle SIMDs and streamed into the step kernel.
constexpr int SPLIT_CHUNK_MAX = 256;
constexpr size_t SPLIT_Z_BYTES = (size_t)32 << 20;  // keep a chunk's normals L2-resident (4 MiB per XCD)
constexpr size_t SPLIT_AUTO_MAX_WAVES = 640;

// Which fused kernel a segment gets: the one decision behind launch_fused (what is launched) and fused_takes_epilogue
// (what the plan executor may hand to the launch).
enum FusedKernel {
  FUSED_GENERIC,       // k_fused_generic
  FUSED_HOT,           // the hot path: k_fused_fast, or k_fused_fastb with bpl > 1 blocks per lane
  FUSED_HOT_FULLCOV,   // the hot path with a full covariance factor: one block per lane, or bpl = 2 mirrored ones
  FUSED_SPLIT          // small-n mode: generator kernel and k_fused_fast_pregen in turn
};
struct FusedChoice {
  FusedKernel kernel;
  int bpl;
};

static FusedChoice fused_choice(const mcx_engine *e, const SegArgs &a)
{
  const int lik = e->lik.kind, lpc = e->lpc;
  if (lik == LIK_USER) {  // MCX_VL_SOURCE has its own rule (mcx_user.hip): the user's hot-path kernels are k_fused_fast's body + epilogue
    const int v = user_lik_variant(lpc, a);
    return {v == 0 ? FUSED_HOT : v == 1 ? FUSED_HOT_FULLCOV : FUSED_GENERIC, 1};
  }
  const bool fast_lik = lik == LIK_ROSEN1 || lik == LIK_GAUSS || (lik == LIK_MIX && a.ncomp <= 8);
  const bool lanes_ok = lpc <= 8 && a.vec4 && !a.mask;
  // (the overlapping Rosenbrock has the plain hot-path kernel only: no small-n modes, no several blocks per lane)
  if (lanes_ok && a.diag && (fast_lik || lik == LIK_ROSEN2F)) {
    const size_t waves = ((size_t)a.n * lpc + 63) / 64;
    if (fast_lik && (e->opt_split > 0 || (e->opt_split < 0 && waves < SPLIT_AUTO_MAX_WAVES))) return {FUSED_SPLIT, 1};
    // blocks per lane of the hot-path kernel: MCX_OPT_BLOCKS_PER_LANE, or what was measured best (mcx_fastb.hpp)
    // Measured (tools/bpl_sweep.py, 65 536 chains): Rosenbrock1 / Gaussian 16-D 2.51 ms per job with one block per
    // lane, 2.67 with two, 2.81 with four -- the step is bound by the Philox / Box-Muller issue slots, which do not
    // care how the lanes are cut; the 32-D mixture 2.63 -> 1.97 ms with two -- its eight per-component reductions
    // over 8 lanes (DPP + row operations each) become reductions over 4.
    int bpl = e->opt_bpl;
    if (bpl == 0) bpl = (lik == LIK_MIX && lpc == 8) ? 2 : 1;
    while (bpl > lpc) bpl >>= 1;
    return {FUSED_HOT, fast_lik ? bpl : 1};
  }
  if (lanes_ok && !a.diag && fast_lik) {
    // full covariance: one block per lane, or two mirrored ones (mcx_fastb.hpp) -- bpl as MCX_OPT_BLOCKS_PER_LANE says,
    // else what tools/fullcov_ab.sh measured best per size (16-D: since the generator got cheaper the mirrored kernel wins
    // at 65 536 chains, 2.49 against 2.55 ms; it has half the wavefronts, so not below that)
    const bool mirrored = (lpc == 4 || lpc == 8) && (e->opt_bpl == 2 || (e->opt_bpl == 0 && (lpc == 8 || a.n >= 65536)));
    return {FUSED_HOT_FULLCOV, mirrored ? 2 : 1};
  }
  return {FUSED_GENERIC, 1};
}

// Does a segment run on one of the hot-path kernels that take the burn-in tuner and the start of the moments into
// the launch (SegArgs::tun, SegArgs::init_moments: k_fused_fast plain / full covariance, k_fused_fastb)?
static bool fused_takes_epilogue(const mcx_engine *e, const SegArgs &a)
{
  if ((unsigned long long)a.n * (unsigned long long)a.nsteps >= (1ull << 40)) return false;  // tuner_epilogue's 40-bit sums
  const FusedKernel k = fused_choice(e, a).kernel;
  return k == FUSED_HOT || k == FUSED_HOT_FULLCOV;
}

// The fused-kernel families are compiled in their own translation units (mcx_k_fast.hip,
// mcx_k_pregen.hip, mcx_k_generic_*.hip) so that the library builds in parallel; see mcx_launch.hpp.
static int launch_fused_plain(int lpc, int lik, bool main, const SegArgs &a, hipStream_t st, FusedChoice c, StepLedger *led)
{
  hipError_t err;
  switch (c.kernel) {
  case FUSED_HOT: err = c.bpl > 1 ? mcxk_launch_fastb(lpc, c.bpl, lik, main, a, st, led) : mcxk_launch_fast(lpc, lik, main, a, st, led); break;
  case FUSED_HOT_FULLCOV: err = c.bpl == 2 ? mcxk_launch_fastb_full(lpc, lik, main, a, st, led) : mcxk_launch_fast_full(lpc, lik, main, a, st, led); break;
  default: err = main ? mcxk_launch_generic_main(lpc, lik, a, st, led) : mcxk_launch_generic_burn(lpc, lik, a, st, led);
  }
  if (err == hipErrorInvalidValue) return fail(MCX_ERR_UNSUPPORTED, "no fused kernel for lanes/chain = %d, likelihood %d", lpc, lik);
  HIPCHK(err);
  return MCX_OK;
}

static int launch_fused(mcx_engine *e, bool main, const SegArgs &a, hipStream_t st)
{
  const int lik = e->lik.kind, lpc = e->lpc;
  if (lik == LIK_USER) return user_lik_launch_fused(*e->lik.user, main, a, st, &e->steps);  // MCX_VL_SOURCE: mcx_user.hip
  const FusedChoice c = fused_choice(e, a);
  if (c.kernel != FUSED_SPLIT) {
    if (c.kernel == FUSED_HOT && a.samp_x && a.d < 4 * lpc) {  // the plain hot-path kernel's lanes without parameters store their rows here
      MCXCHK(e->trash.alloc(4 * (size_t)a.n * lpc));
      SegArgs b = a;
      b.trash = e->trash.p;
      return launch_fused_plain(lpc, lik, main, b, st, c, &e->steps);
    }
    return launch_fused_plain(lpc, lik, main, a, st, c, &e->steps);
  }
  // generator and step kernel alternate on the engine's stream (overlapping them on two streams was
  // measured slower: the cross-stream event waits cost more than the generator, which is ~10 % of a chunk)
  const size_t per_step = (size_t)a.n * a.d * sizeof(float);
  const int SPLIT_CHUNK = (int)std::max<size_t>(32, std::min<size_t>(SPLIT_CHUNK_MAX, (SPLIT_Z_BYTES / per_step) & ~(size_t)7));
  constexpr int PAD = 16;  // the step kernel prefetches two 8-step batches ahead without bounds checks
  MCXCHK(e->zpre.alloc((size_t)(SPLIT_CHUNK + PAD) * a.n * a.d));
  MCXCHK(e->upre.alloc((size_t)(SPLIT_CHUNK + PAD) * a.n));
  MCXCHK(e->trash.alloc(4 * (size_t)a.n * lpc));
  for (int c0 = 0; c0 < a.nsteps; c0 += SPLIT_CHUNK) {
    const int ns = std::min(SPLIT_CHUNK, a.nsteps - c0);
    {
      ProfScope pg(e, MCX_K_GEN_NORMALS, (uint64_t)ns * (uint64_t)a.n);
      HIPCHK(mcxk_launch_gen(lpc, e->zpre.p, e->upre.p, a.n, a.d, ns, a.t0 + (uint32_t)c0, a.g0, a.seed, st, &e->steps));
    }
    SegArgs b = a;
    b.nsteps = ns;
    b.t0 = a.t0 + (uint32_t)c0;
    b.isamp0 = a.isamp0 + c0;
    b.snap_after = (a.snap_after >= c0 && a.snap_after < c0 + ns) ? a.snap_after - c0 : -1;
    if (b.samp_x && a.samp_stride <= 1) {
      b.samp_x += (size_t)c0 * a.n * a.d;
      b.samp_ly += (size_t)c0 * a.n;
    }
    b.zpre = e->zpre.p;
    b.upre = e->upre.p;
    b.trash = e->trash.p;
    HIPCHK(mcxk_launch_fast_pregen(lpc, lik, main, b, st, &e->steps));
    e->cnt.kernel_launches += 1;  // (the generator's scope counted itself)
  }
  return MCX_OK;
}

static int cov_reset(mcx_engine *e)
{
  if (!e->cov_pending) return MCX_OK;
  HIPCHK(hipMemcpyAsync(e->cov.p, e->cov0.p, (size_t)e->ncov * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
  e->cov_pending = false;
  e->cov_offdiag = !e->diag;
  return MCX_OK;
}

// VLFunc call on device-resident proposals; HOST kind goes device -> host -> device
static int eval_trials(mcx_engine *e, const float *x_dev, float *y_dev, uint64_t cs)
{
  const int n = e->nchain, d = e->nparam;
  if (e->lik.kind == MCX_VL_HOST) {
    MCXCHK(e->h_ptrial.alloc((size_t)e->ntot));
    MCXCHK(e->h_lytrial.alloc((size_t)n));
    HIPCHK(hipMemcpyAsync(e->h_ptrial.p, x_dev, (size_t)e->ntot * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    (void)e->lik.fn(e->lik.ctx, n, e->h_ptrial.p, e->h_lytrial.p);  // return code ignored like the reference
    // no second synchronisation: h_lytrial is pinned and is next written by the callback of the NEXT step, which
    // runs only after that step's D2H -- queued behind this copy on the same stream -- has been waited for
    HIPCHK(hipMemcpyAsync(y_dev, e->h_lytrial.p, (size_t)n * sizeof(float), hipMemcpyHostToDevice, e->stream));
    return MCX_OK;
  }
  ProfScope ps(e, MCX_K_EVAL, cs);
  if (e->lik.kind == MCX_VL_DEVICE) {  // the user's own kernel, VLFunc contract on device memory
    int npset = n;
    const float *xa = x_dev;
    float *ya = y_dev;
    void *args[] = {&npset, &xa, &ya};
    HIPCHK(hipModuleLaunchKernel((hipFunction_t)e->lik.ctx, nblocks((size_t)n), 1, 1, BLOCK, 1, 1, 0, e->stream, args, nullptr));
    return MCX_OK;
  }
  return eval_device(e->lik, x_dev, y_dev, n, d, e->stream);
}

// MCX_OPT_REFERENCE_CALLS: the reference evaluates L(1, pvals_j, &y) once per chain after every main-loop step and throws
// the result away (src/mcpar.cc:177-182).  A host functor with side effects -- a call counter, a cache, a log -- sees those
// calls there; here they are made only on request, for host functors (a device likelihood has no side effects to keep).
static int discarded_calls(mcx_engine *e)
{
  if (!e->opt_reference_calls || e->lik.kind != MCX_VL_HOST) return MCX_OK;
  const int n = e->nchain, d = e->nparam;
  MCXCHK(e->h_ptrial.alloc((size_t)e->ntot));
  HIPCHK(hipMemcpyAsync(e->h_ptrial.p, e->pvals.p, (size_t)e->ntot * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  float y = 0.0f;
  for (int j = 0; j < n; ++j) (void)e->lik.fn(e->lik.ctx, 1, e->h_ptrial.p + (size_t)j * d, &y);
  return MCX_OK;
}

void fill_step(mcx_engine *e, StepArgs &a, uint32_t t, int isamp, bool main, size_t maskrow,
                      int samprow, int remote)
{
  a.x = e->pvals.p; a.ly = e->lylast.p; a.mu = e->mu.p; a.psum2 = e->psum2.p;
  a.ptrial = e->ptrial.p; a.lytrial = e->lytrial.p; a.cfac = e->cfac.p;
  a.mutrial = e->mutrial.p; a.sigtrial = e->sigtrial.p;
  a.acc_cnt = e->acc_cnt.p;
  a.acc_slots = e->acc_slots.p;
  a.T = e->cov.p;
  const bool keep = main && e->opt_samples && samprow % e->opt_stride == 0;
  float *vx = nullptr, *vl = nullptr;
  if (keep) samp_vbase(e, samprow, &vx, &vl);
  a.samp_x = keep ? vx + (size_t)(samprow / e->opt_stride) * e->ntot : nullptr;
  a.samp_ly = keep ? vl + (size_t)(samprow / e->opt_stride) * e->nchain : nullptr;
  a.mask = e->opt_mask ? e->mask.p + maskrow * (size_t)e->nchain : nullptr;
  a.lik = e->lik.params.p; a.ncomp = e->lik.ncomp;
  a.n = e->nchain; a.d = e->nparam;
  a.g0 = (uint32_t)(e->rank * e->nchain); a.t = t; a.seed = e->seed;
  a.isamp = isamp; a.diag = e->diag ? 1 : 0; a.vec4 = e->vec4; a.remote = remote;
}

int launch_propose(mcx_engine *e, const StepArgs &a)
{
  ProfScope ps(e, MCX_K_PROPOSE, (uint64_t)e->nchain);
  const dim3 grid(nblocks((size_t)a.n * e->lpc)), block(BLOCK);
  DISPATCH_LPC(e->lpc, hipLaunchKernelGGL((k_propose_local<LPC_>), grid, block, 0, e->stream, a));
  HIPCHK(hipGetLastError());
  return MCX_OK;
}

static int launch_accept(mcx_engine *e, const StepArgs &a, bool main)
{
  ProfScope ps(e, MCX_K_ACCEPT, (uint64_t)e->nchain);
  const dim3 grid(nblocks((size_t)a.n * e->lpc)), block(BLOCK);
  if (main) { DISPATCH_LPC(e->lpc, hipLaunchKernelGGL((k_accept<LPC_, true>), grid, block, 0, e->stream, a)); }
  else { DISPATCH_LPC(e->lpc, hipLaunchKernelGGL((k_accept<LPC_, false>), grid, block, 0, e->stream, a)); }
  HIPCHK(hipGetLastError());
  return MCX_OK;
}

// ---------------------------------------------------------------------------------------------
// k_run_small's tuner events are meetings of ALL its workgroups at a device counter: every workgroup of the
// grid must be resident.  The grid is sized to fit the GPU on its own (one workgroup per CU), but two such
// kernels dispatched at the same time -- two engines of one process, or two processes sharing a GPU -- could
// each get part of the CUs and wait for the rest forever.  So a launch that contains meetings (burn-in steps)
// holds an exclusive advisory lock on a per-GPU lock file until it has completed; launches without meetings
// (main-loop steps only: workgroups are independent) need none.  flock() excludes both other processes and
// other engines of this process (each engine has its own open file description).
// ---------------------------------------------------------------------------------------------
// internal status of run_once(): a tuner meeting of k_run_small was abandoned (or its grid cannot be resident):
// mcx_run repeats the run on the per-segment kernels.  Never leaves this file.


// the launch that took the lock has completed (or is waited for here): let the next one in, and look at the
// launch's "abandoned" word -- before any of its results is used or shown to a hook
int meet_release(mcx_engine *e, bool stream_is_idle)
{
  if (!e->meet_held && !e->meet_check) return MCX_OK;
  hipError_t se = hipSuccess;
  if (!stream_is_idle) se = hipStreamSynchronize(e->stream);
  if (e->meet_held) {
    (void)flock(e->meet_fd, LOCK_UN);
    e->meet_held = false;
  }
  HIPCHK(se);
  if (e->meet_check) {
    e->meet_check = false;
    unsigned long long w = 0;
    HIPCHK(hipMemcpyAsync(&w, e->meet_word, sizeof w, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (w) return MCX_INTERNAL_MEET_ABANDONED;
  }
  return MCX_OK;
}

// One fixed path per GPU (PCI bus id), the same for every process and user whatever their TMPDIR: /dev/shm
// first (always local, never a per-job directory), /tmp second.  O_NOFOLLOW: a symbolic link planted under the
// name is not followed; the mode is widened only on the file this call created.
static bool meet_lock_open(mcx_engine *e)
{
  if (e->meet_fd >= 0) return true;
  char bus[64] = "gpu";
  (void)hipDeviceGetPCIBusId(bus, (int)sizeof bus, e->device);
  for (char *c = bus; *c; ++c)
    if (*c == ':' || *c == '/') *c = '_';
  const char *dirs[] = {"/dev/shm", "/tmp"};
  for (const char *d : dirs) {
    const std::string path = std::string(d) + "/mcx_meet_" + bus + ".lock";
    int fd = open(path.c_str(), O_RDWR | O_CREAT | O_EXCL | O_NOFOLLOW | O_CLOEXEC, 0666);
    if (fd >= 0) (void)fchmod(fd, 0666);  // created here: shared by every user of the GPU
    else fd = open(path.c_str(), O_RDWR | O_NOFOLLOW | O_CLOEXEC);
    if (fd < 0) fd = open(path.c_str(), O_RDONLY | O_NOFOLLOW | O_CLOEXEC);  // (another user's file: flock needs no write access)
    if (fd >= 0) {
      e->meet_fd = fd;
      return true;
    }
  }
  return false;
}

static int meet_lock_take(mcx_engine *e)
{
  int rc;
  do rc = flock(e->meet_fd, LOCK_EX);
  while (rc != 0 && errno == EINTR);
  if (rc != 0) return fail(MCX_ERR_HIP, "cannot lock the GPU's meeting lock file: %s", strerror(errno));
  e->meet_held = true;
  return MCX_OK;
}

// rerun: repeat the run that was just abandoned -- same likelihood and factor as installed (L and incov are not looked at),
// from the staged state or, when the run started from caller memory that may be gone by now, from the copy kept of it
static int run_once(mcx_engine *e, int nsamp, int nburn, const float *pinit, const mcx_vlfunc *L, const float *incov, bool rerun = false);
constexpr int PERSIST_RETRY_RUNS = 16;

// A tuner meeting of the one-launch small-n kernel was abandoned: some workgroup of its grid was not resident (CU mask,
// partitioned device, a foreign kernel on the CUs).  The launch wrote no state back: the run is repeated on the
// per-segment kernels (same bits), which the engine then keeps to for PERSIST_RETRY_RUNS runs.
static int repeat_abandoned_run(mcx_engine *e, int nsamp, int nburn, const float *pinit, const mcx_vlfunc *L, const float *incov, bool rerun)
{
  (void)hipStreamSynchronize(e->stream);
  e->persist_broken = true;
  e->runs_since_broken = 0;
  e->meet_total++;
  if (getenv("MCX_VERBOSE"))
    fprintf(stderr, "mcx: a tuner meeting of the one-launch small-n kernel was abandoned after %d ms (a workgroup of its grid "
                    "was not resident); the run is repeated on the per-segment kernels\n", e->opt_meet_timeout_ms);
  const int async = e->opt_async_run;
  e->opt_async_run = 0;  // (the repeat is waited for: whoever asked is about to look at its results)
  int rc = run_once(e, nsamp, nburn, pinit, L, incov, rerun);
  e->opt_async_run = async;
  if (rc == MCX_INTERNAL_MEET_ABANDONED) rc = fail(MCX_ERR_HIP, "internal: meeting abandoned without the one-launch kernel");
  e->cnt.meet_timeouts = 1;
  return rc;
}

static void never_leave_the_lock_behind(mcx_engine *e, int rc)
{
  if (rc == MCX_OK) return;
  if (e->meet_held) {
    (void)hipStreamSynchronize(e->stream);
    (void)flock(e->meet_fd, LOCK_UN);
    e->meet_held = false;
  }
  e->meet_check = false;
}

// A run whose last launch reports to its counter slot itself (RunArgs::report): has the serial number arrived?  Spins for
// at most `spin_us` -- jobs this is about take 0.3-0.5 ms; whoever waits for a longer one loses nothing by sleeping in
// hipStreamSynchronize instead -- and says whether it saw it.
// (mcx_murray.hip's wait_pass_counters waits for one pass and yields after 60 us: a different policy on purpose.)
static bool report_arrived(const unsigned long long *slot, unsigned long long serial, int spin_us)
{
  const auto t0 = std::chrono::steady_clock::now();
  for (int it = 0;; ++it) {
    if (__atomic_load_n(slot + 7, __ATOMIC_ACQUIRE) == serial) return true;
    if ((it & 63) == 63 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(spin_us)) return false;
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#endif
  }
}
constexpr int REPORT_SPIN_US = 1500;

// the books of runs that were queued asynchronously and never looked at (the next run was queued behind them): was one of
// their meetings abandoned?  Nobody saw their results -- nothing to repeat -- but the engine keeps to the per-segment kernels.
// all = every such run's counters have arrived (the caller waited for a later copy on the same stream); otherwise only those
// whose copy is over are looked at, the others next time
static void note_superseded(mcx_engine *e, bool all)
{
  for (int sl = 0; sl < mcx_engine::HSLOTS && e->superseded_mask; ++sl) {
    if (!(e->superseded_mask & (1u << sl))) continue;
    if (!all && e->slot_serial[sl]) {  // (it reports itself)
      if (__atomic_load_n(e->h_ctr.p + 8 * sl + 7, __ATOMIC_ACQUIRE) != e->slot_serial[sl]) continue;
    } else if (!all && e->copy_pending[sl]) {
      if (hipEventQuery(e->copy_ev[sl]) != hipSuccess) { (void)hipGetLastError(); continue; }
      e->copy_pending[sl] = false;
    }
    if (e->h_ctr.p[8 * sl + 5] != 0) {
      e->persist_broken = true;
      e->runs_since_broken = 0;
      e->meet_total++;
    }
    e->superseded_mask &= ~(1u << sl);
  }
}

// MCX_OPT_ASYNC_RUN: the end of the run that mcx_run queued and returned from.  Called by every entry point but mcx_run
// (enter(), mcx_engine_internal.hpp).
int finish_pending(mcx_engine *e)
{
  if (!e->pend.active) return MCX_OK;
  const mcx_engine::PendingRun p = e->pend;
  e->pend.active = false;
  hipError_t se = hipSuccess;
  if (!(p.serial && report_arrived(p.hctr, p.serial, REPORT_SPIN_US))) se = hipStreamSynchronize(e->stream);
  if (se == hipSuccess && p.serial && __atomic_load_n(p.hctr + 7, __ATOMIC_ACQUIRE) != p.serial)
    return fail(MCX_ERR_HIP, "internal: the run's last launch is over and has not reported");
  if (se == hipSuccess && e->copy_pending[p.slot]) se = hipEventSynchronize(e->copy_ev[p.slot]);  // (its counters: a stream of their own)
  if (se == hipSuccess)  // (the copies leave in order: every earlier run's counters are in as well)
    for (bool &cp : e->copy_pending) cp = false;
  for (bool &rq : e->run_queued) rq = false;
  const bool abandoned = p.meet_check && se == hipSuccess && p.hctr[5] != 0;
  e->meet_check = false;
  (void)meet_release(e, true);
  if (se == hipSuccess) note_superseded(e, true);
  HIPCHK(se);
  int rc = MCX_OK;
  if (abandoned) {
    e->tbase = p.tbase0;  // (the abandoned launch moved nothing but the step counter)
    rc = repeat_abandoned_run(e, p.nsamp, p.nburn, nullptr, nullptr, nullptr, true);
  } else {
    e->cnt.naccept_burn = p.hctr[3];
    e->cnt.naccept_main = p.hctr[4];
    xwait_collect(e);
    if (e->persist_broken && ++e->runs_since_broken >= PERSIST_RETRY_RUNS) e->persist_broken = false;
  }
  never_leave_the_lock_behind(e, rc);
  return rc;
}

extern "C" int mcx_run(mcx_engine *e, int nsamp, int nburn, const float *pinit, const mcx_vlfunc *L,
                       const float *incov)
{
  MCXCHK(enter_raw(e));
  if (e->pend.active) {
    // A run is still in flight.  With MCX_OPT_ASYNC_RUN the next one is queued right behind it: nobody has looked at its
    // results, and nobody will -- this run overwrites them -- so it needs no waiting for (launch and completion latency
    // of back-to-back small jobs overlap the jobs themselves); its counters are looked at later, for the books only.
    if (e->opt_async_run && hipStreamQuery(e->stream) == hipErrorNotReady) {
      (void)hipGetLastError();
      // at most TWO runs in flight: the one before the pending one must be over before this call queues another
      // (the host queues a small job in 15 us, the GPU takes 400: without a bound the queue would only grow).  Its KERNELS,
      // not its counters: their copy -- a kernel of the runtime's on the other stream -- gets no room beside the pending
      // run's grid and ends with it; waiting for it let the queue run dry after every second job (24 us between two jobs
      // where 7 is the dispatch alone, tools/queued_jobs_probe.py)
      const int before = (e->hctr_slot + mcx_engine::HSLOTS - 1) % mcx_engine::HSLOTS;
      if (e->run_queued[before]) {
        if (e->slot_serial[before]) {  // (it reports itself: no event behind it)
          if (!report_arrived(e->h_ctr.p + 8 * before, e->slot_serial[before], REPORT_SPIN_US)) {
            HIPCHK(hipStreamSynchronize(e->stream));  // a long job: no hurry then
            (void)hipGetLastError();
          }
        } else {
          HIPCHK(hipEventSynchronize(e->run_ev[before]));
        }
        e->run_queued[before] = false;
      }
      note_superseded(e, false);
      if (e->pend.meet_check) e->superseded_mask |= 1u << e->pend.slot;
      e->pend.active = false;
    } else {
      (void)hipGetLastError();
      MCXCHK(finish_pending(e));
    }
  }
  static const int verbose = getenv("MCX_VERBOSE") ? atoi(getenv("MCX_VERBOSE")) : 0;
  const auto ht0 = std::chrono::steady_clock::now();
  e->ht_mark[0] = e->ht_mark[1] = e->ht_mark[2] = ht0;
  e->steps.n = 0;  // the ledger of step-kernel instances (mcx_debug_step_instances) starts over
  e->steps.lost = false;
  int rc = run_once(e, nsamp, nburn, pinit, L, incov);
  if (verbose >= 2) {  // where the host's share of a run goes: set-up / queued everything / stream idle / done
    auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
      return std::chrono::duration<double, std::micro>(b - a).count();
    };
    const auto ht3 = std::chrono::steady_clock::now();
    fprintf(stderr, "mcx: run host timing: to first launch %.1f us, queueing %.1f us, waiting for the stream %.1f us, after %.1f us\n",
            us(ht0, e->ht_mark[0]), us(e->ht_mark[0], e->ht_mark[1]), us(e->ht_mark[1], e->ht_mark[2]), us(e->ht_mark[2], ht3));
  }
  uint64_t repeated = 0;
  if (rc == MCX_INTERNAL_MEET_ABANDONED) {
    repeated = 1;
    rc = repeat_abandoned_run(e, nsamp, nburn, pinit, L, incov, false);
  }
  if (!e->pend.active) {
    e->cnt.meet_timeouts = repeated;
    // whatever kept a workgroup out may be gone: the one-launch kernel is tried again after PERSIST_RETRY_RUNS runs
    if (e->persist_broken && !repeated && rc == MCX_OK && ++e->runs_since_broken >= PERSIST_RETRY_RUNS) e->persist_broken = false;
  }
  never_leave_the_lock_behind(e, rc);
  return rc;
}

// ---------------------------------------------------------------------------------------------
// run_once: one run, MCPar::run (src/mcpar.cc:17-214), as a sequence of phases over one context
// ---------------------------------------------------------------------------------------------
// What more than one phase of a run reads.  A parameter pack: filled by run_once and the phases in the order they are called.
struct Run {
  mcx_engine *e;
  int nsamp, nburn;
  const float *pinit;   // caller memory the run starts from, or nullptr:
  const float *staged;  // the state a run without `pinit` starts from (device)
  bool rerun;
  int n, d;
  hipStream_t st;
  uint32_t g0;
  int nkeep;  // kept steps: isamp % stride == 0
  bool sink;  // sink mode: a ring of SINK_RING blocks instead of the whole run (block length a multiple of the stride)
  int sblock;
  bool fused;
  // small-n mode, one launch per stretch of local steps (small_n_config)
  int pbpl, plpc2, nown;
  bool persist, lead;
  const char *trace_file;  // MCX_PERSIST_TRACE (a -DMCX_PERSIST_TRACE build writes it: tools/persist_trace.py), or nullptr
  unsigned long long *ctrp, *hctr;  // this run's counter block on the device / its slot of the pinned ring
  unsigned long long reported;      // serial of the launch that reports the run's end itself (RunArgs::report), if one does
  SegArgs sa;                       // what every segment's launch starts from (segment_template)
  bool init_pending;                // MCX_PLAN_INIT_MOMENTS handed to the next main segment's launch
  bool sig_done, slots_used;        // the variances are written / the accept slots want reducing at the end
  int sink_seq;
  std::vector<mcx_plan_item> plan;
};

// sample store, sink ring and its streams / events, best row, accept mask, the 1/pwgt table
static int prepare_outputs(Run &r)
{
  mcx_engine *e = r.e;
  const int n = r.n, d = r.d, nsamp = r.nsamp, nburn = r.nburn;
  hipStream_t st = r.st;
  // sample store: every chain, every main-loop step (src/mcpar.cc:31-40, 177-182), kept in HBM
  e->samp_steps = 0;
  r.nkeep = (nsamp + e->opt_stride - 1) / e->opt_stride;
  const bool sink = (e->sfn != nullptr || e->tfn != nullptr) && e->opt_samples && nsamp > 0;
  const int sblock = sink ? ((std::max(e->sink_block, 1) + e->opt_stride - 1) / e->opt_stride) * e->opt_stride : 0;
  const int kb = sink ? sblock / e->opt_stride : 0;
  r.sink = sink; r.sblock = sblock;
  e->run_sink = sink; e->run_sblock = sblock; e->run_kb = kb;
  e->run_sink_text = sink && e->sfn != nullptr && e->opt_sink_text != 0;
  if (e->opt_samples && nsamp > 0) {
    const size_t rows = sink ? (size_t)std::min<long long>((long long)SINK_RING * kb, r.nkeep + kb) : (size_t)r.nkeep;
    int s1 = e->samp_x.alloc(rows * e->ntot), s2 = e->samp_ly.alloc(rows * n);
    if (s1 != MCX_OK || s2 != MCX_OK)
      return fail(MCX_ERR_ALLOC, "Unable to allocate space for output samples (%zu bytes)",
                  rows * n * (d + 1) * sizeof(float));
  }
  if (sink) {
    for (int b = 0; b < 2; ++b) {
      MCXCHK(e->sink_stage[b].alloc((size_t)kb * n * (d + 1)));
      if (e->tfn || e->opt_sink_text) {
        MCXCHK(e->sink_text_wg[b].alloc(((size_t)kb * n * (d + 1) + BLOCK - 1) / BLOCK + 1));
        MCXCHK(e->sink_text_total[b].alloc(1));
      }
      if (!e->tfn) MCXCHK(e->sink_pin[b].alloc((size_t)kb * n * (d + 1)));
      MCXCHK(e->ev_steps[b].ensure(hipEventDisableTiming));
      MCXCHK(e->ev_copy[b].ensure(hipEventDisableTiming));
      MCXCHK(e->ev_write[b].ensure(hipEventDisableTiming));
    }
    MCXCHK(e->cstream.ensure(hipStreamNonBlocking));
    MCXCHK(e->tstream.ensure(hipStreamNonBlocking));
    MCXCHK(e->ev_text.ensure(hipEventDisableTiming));
  }
  MCXCHK(e->best_row.alloc((size_t)d + 1));
  MCXCHK(e->best_key.alloc(1));
  if (sink) {
    hipLaunchKernelGGL(k_best_reset, dim3(nblocks((size_t)d + 1)), dim3(BLOCK), 0, st, e->best_row.p, d, e->best_key.p);
    HIPCHK(hipGetLastError());
  }
  if (e->opt_mask) {
    MCXCHK(e->mask.alloc((size_t)(nburn + nsamp) * n));
    HIPCHK(hipMemsetAsync(e->mask.p, 0, (size_t)(nburn + nsamp) * n, st));
  }
  if ((size_t)nsamp > e->h_winv.size()) {  // 1/pwgt for every main-loop step (src/mcpar.cc:186-187),
    HIPCHK(hipStreamSynchronize(st));      // correctly rounded on the host; rebuilt only when it grows
    e->h_winv.resize((size_t)nsamp);
    for (int i = 0; i < nsamp; ++i) e->h_winv[(size_t)i] = 1.0f / (float)(i + 1);
    MCXCHK(e->winv_tab.alloc((size_t)nsamp + 16));  // + the small-n kernel's unchecked prefetch distance
    HIPCHK(hipMemcpyAsync(e->winv_tab.p, e->h_winv.data(), e->h_winv.size() * sizeof(float), hipMemcpyHostToDevice, st));
  }
  e->cnt = mcx_counters{};
  if (e->tail_publish) {  // the last run's final gather may still be in flight (finish_tail)
    if (nsamp > 0) e->tail_publish = 0;  // this run rewrites the slot -- after waiting for that gather -- before anything reads it
    else MCXCHK(finish_tail(e));
  }
  e->published_steps = 0;
  return MCX_OK;
}

// Small-n mode, one launch per stretch of local steps (mcx_persist.hpp): the whole burn-in with its tuner
// events, the start of the main loop and every run of consecutive local main-loop segments go to k_run_small
// when the chains fill at most POWN_MAX wavefronts per CU and the hot-path kernel applies.
static void small_n_config(Run &r)
{
  mcx_engine *e = r.e;
  // (with two 4-parameter blocks per lane where that takes a workgroup from two or more owner wavefronts towards one)
  r.pbpl = mcxk_persist_bpl(e->lpc, r.d, r.n, e->ncu, e->opt_bpl);
  r.plpc2 = e->lpc / r.pbpl;
  r.nown = (int)(((size_t)r.n * r.plpc2 + 63) / 64);
  const bool fast_lik = e->lik.kind == LIK_ROSEN1 || e->lik.kind == LIK_GAUSS || (e->lik.kind == LIK_MIX && e->lik.ncomp <= 8) ||
                        (e->lik.kind == LIK_USER && user_lik_small_ok(*e->lik.user));  // (a user's source in block form)
  const bool hot_path = r.fused && e->lpc <= 8 && fast_lik && e->diag && e->vec4 && !e->opt_mask;
  // (the mode is for chains that fill at most POWN_MAX wavefronts per CU at ONE block per lane: beyond that the per-segment
  // kernels are as fast or faster -- 65 536 x 16-D would fit the grid with two blocks per lane and run 35 % slower)
  const size_t nown_one_block = ((size_t)r.n * e->lpc + 63) / 64;
  const bool few_chains = e->ncu > 0 && nown_one_block <= (size_t)POWN_MAX * (size_t)e->ncu && r.nown <= POWN_MAX * e->ncu;
  const bool events_fit = r.nburn / 50 + 2 <= PEVENTS;  // the tuner events' meeting words of the counter block
  const int nwg = std::max(std::min(r.nown, e->ncu), 1);
  const bool lds_fits = hot_path && few_chains && mcxk_persist_lds_bytes(r.plpc2, r.pbpl, (r.nown + nwg - 1) / nwg) <= MCXK_PERSIST_LDS_LIMIT;
  const bool wanted = (e->opt_persist > 0 || (e->opt_persist < 0 && e->opt_split != 0)) && !e->persist_broken;
  // (launches with tuner meetings need the GPU's meeting lock: its file is opened last, only for a run that will take it)
  r.persist = hot_path && few_chains && events_fit && lds_fits && wanted && (r.nburn == 0 || meet_lock_open(e));
  // When the run opens with such a launch, the launch itself takes the initial state (and its likelihood,
  // src/mcpar.cc:47-53) and the factor as installed, and starts its counters afresh: no reset kernels at all.
  r.lead = r.persist && r.nburn + r.nsamp > 0;
}

// this run's counter block on the device and its slot of the pinned ring the counters end in
static int claim_counter_slots(Run &r)
{
  mcx_engine *e = r.e;
  // the counter block: a ring, zeroed as a whole when it wraps
  e->ctr_set = (e->ctr_set + 1) % CTR_RING;
  if (e->ctr_set == 0) {
    for (int sl = 0; sl < mcx_engine::HSLOTS; ++sl)  // (an asynchronous run's counters may still be on their way out of the ring)
      if (e->copy_pending[sl]) HIPCHK(hipStreamWaitEvent(r.st, e->copy_ev[sl], 0));
    HIPCHK(hipMemsetAsync(e->ctr.p, 0, (size_t)CTR_WORDS * CTR_RING * sizeof(unsigned long long), r.st));
  }
  r.ctrp = e->ctr.p + (size_t)e->ctr_set * CTR_WORDS;
  // ... and the slot (slots in turn: with MCX_OPT_ASYNC_RUN earlier runs' may not have been read yet)
  if (!e->h_ctr.p) {
    MCXCHK(e->h_ctr.alloc(8 * mcx_engine::HSLOTS));  // pinned: the copy queues behind the last kernel instead of staging through the runtime
    memset(e->h_ctr.p, 0, 8 * mcx_engine::HSLOTS * sizeof(unsigned long long));
  }
  e->hctr_slot = (e->hctr_slot + 1) % mcx_engine::HSLOTS;
  if (e->copy_pending[e->hctr_slot]) {  // four runs back: long over
    HIPCHK(hipEventSynchronize(e->copy_ev[e->hctr_slot]));
    e->copy_pending[e->hctr_slot] = false;
  }
  if (e->superseded_mask & (1u << e->hctr_slot)) note_superseded(e, false);  // (its word, before the slot is written again)
  e->superseded_mask &= ~(1u << e->hctr_slot);
  e->run_queued[e->hctr_slot] = false;
  e->slot_serial[e->hctr_slot] = 0;
  r.hctr = e->h_ctr.p + 8 * e->hctr_slot;
  r.reported = 0;
  return MCX_OK;
}

// the initial state and its likelihood (src/mcpar.cc:47-53), counters and factor reset -- unless the run's first launch does it all
static int reset_state(Run &r)
{
  mcx_engine *e = r.e;
  // pinit is pageable caller memory: the runtime stages it before hipMemcpyAsync returns
  if (r.pinit) HIPCHK(hipMemcpyAsync(e->pvals.p, r.pinit, (size_t)e->ntot * sizeof(float), hipMemcpyHostToDevice, r.st));  // :47-50
  if (r.lead) return MCX_OK;
  hipLaunchKernelGGL(k_run_reset, dim3(nblocks((size_t)e->ntot)), dim3(BLOCK), 0, r.st, e->acc_slots.p, (size_t)e->nslots,
                     e->acc_cnt.p, (size_t)r.n, e->ntrace.p, e->pvals.p, r.pinit ? (const float *)nullptr : r.staged,
                     (size_t)e->ntot, e->cov.p, e->cov_pending ? (const float *)e->cov0.p : (const float *)nullptr,
                     (size_t)e->ncov);
  HIPCHK(hipGetLastError());
  if (e->cov_pending) {  // (cov_reset's copy went with the reset kernel)
    e->cov_pending = false;
    e->cov_offdiag = !e->diag;
  }
  return eval_trials(e, e->pvals.p, e->lylast.p, 0);  // :53
}

static SegArgs segment_template(const Run &r)
{
  const mcx_engine *e = r.e;
  SegArgs sa;
  sa.x = e->pvals.p; sa.ly = e->lylast.p; sa.mu = e->mu.p; sa.psum2 = e->psum2.p;
  sa.acc_cnt = e->acc_cnt.p; sa.acc_slots = e->acc_slots.p; sa.T = e->cov.p; sa.lik = e->lik.params.p; sa.ncomp = e->lik.ncomp;
  sa.n = r.n; sa.d = r.d; sa.g0 = r.g0; sa.seed = e->seed; sa.diag = e->diag ? 1 : 0; sa.vec4 = e->vec4;
  sa.winv = e->winv_tab.p;
  sa.samp_stride = e->opt_stride;
  sa.musig_own = e->musigall.p + 2 * (size_t)e->rank * e->ntot;
  sa.snap_after = -1;
  sa.zpre = sa.upre = nullptr;
  sa.trash = nullptr;
  sa.init_moments = 0;
  sa.sig_out = nullptr;
  sa.tun = SegArgs::Tuner{};
  sa.tun.ncov = e->ncov; sa.tun.nslots = e->nslots; sa.tun.ctr = r.ctrp; sa.tun.T = e->cov.p; sa.tun.trace = e->trace.p;
  sa.tun.ntrace = e->ntrace.p; sa.tun.cells = e->tun_cells.p;
  sa.tun.armin = e->TGT_ARATE_MIN; sa.tun.armax = e->TGT_ARATE_MAX; sa.tun.dfac = e->SCALE_DEC; sa.tun.ifac = e->SCALE_INC;
  return sa;
}

// the kernel about to be launched rewrites this shard's slot: no gather may still be reading it
static int slot_rewritten(mcx_engine *e, int published_steps)
{
  MCXCHK(exchange_wait(e));
  e->published_steps = published_steps;
  return MCX_OK;
}

// who generates what in k_run_small (RunArgs::deal): rebuilt and uploaded only when the launch configuration changes
static int deal_table(Run &r, const RunArgs &ra)
{
  mcx_engine *e = r.e;
  const int prec = mcxk_persist_recorders(ra.own, r.pbpl) ? 1 : 0;
  const long long key = (((long long)r.plpc2 * 8 + r.pbpl) * 16 + ra.own) * 64 + ra.ksteps + 4096ll * 1024 * prec;
  if (key == e->deal_key) return MCX_OK;
  HIPCHK(hipStreamSynchronize(r.st));  // (an earlier launch may still read the table)
  e->h_deal.assign((size_t)MCXK_PERSIST_DEAL_WORDS, 0u);
  mcxk_persist_deal(r.plpc2, r.pbpl, ra.own, prec, ra.ksteps, e->h_deal.data());
  MCXCHK(e->deal_tab.alloc((size_t)MCXK_PERSIST_DEAL_WORDS));
  HIPCHK(hipMemcpyAsync(e->deal_tab.p, e->h_deal.data(), e->h_deal.size() * sizeof(uint32_t), hipMemcpyHostToDevice, r.st));
  e->deal_key = key;
  return MCX_OK;
}

// one launch of k_run_small for the stretch `s` of the plan (small_stretch, mcx_plan.hip)
static int launch_small_stretch(Run &r, const SmallStretch &s)
{
  mcx_engine *e = r.e;
  const int pb = s.burn, pm = s.main, is0 = s.first_main;
  hipStream_t st = r.st;
  RunArgs ra;
  ra.x = e->pvals.p; ra.ly = e->lylast.p; ra.mu = e->mu.p; ra.psum2 = e->psum2.p; ra.sig = e->sig.p;
  ra.acc_cnt = e->acc_cnt.p; ra.T = e->cov.p;
  ra.samp_x = ra.samp_ly = nullptr;
  if (e->opt_samples && pm > 0) samp_vbase(e, is0, &ra.samp_x, &ra.samp_ly);
  ra.samp_stride = e->opt_stride;
  MCXCHK(e->trash.alloc((size_t)PTRASH * (size_t)PBLOCK * (size_t)std::max(e->ncu, 1)));
  ra.trash = e->trash.p;
  ra.lik = e->lik.params.p; ra.ncomp = e->lik.ncomp; ra.n = r.n; ra.d = r.d; ra.g0 = r.g0; ra.seed = e->seed;
  ra.t0 = pb > 0 ? e->tbase : e->tbase + (uint32_t)r.nburn + (uint32_t)is0;
  ra.nburn = pb; ra.nmain = pm; ra.isamp0 = is0; ra.init_moments = s.init_moments;
  ra.winv = e->winv_tab.p; ra.musig_own = r.sa.musig_own; ra.snap_after = s.snap_after;
  ra.final_publish = (e->size == 1 && pm > 0 && is0 + pm == r.nsamp) ? 1 : 0;
  ra.armin = e->TGT_ARATE_MIN; ra.armax = e->TGT_ARATE_MAX; ra.dfac = e->SCALE_DEC; ra.ifac = e->SCALE_INC;
  ra.ctr = r.ctrp; ra.bar = r.ctrp + 8; ra.trace = e->trace.p; ra.ntrace = e->ntrace.p;
  // the run's first launch takes the state where it lies, evaluates it, and starts the counters afresh
  ra.x0 = r.lead ? (r.pinit ? e->pvals.p : r.staged) : nullptr;
  ra.T0 = e->cov_pending ? e->cov0.p : nullptr;
  ra.fresh = r.lead ? 1 : 0;
  if (e->cov_pending && e->cov_offdiag) {
    // the kernel writes back the diagonal only: a full factor left in cov by an earlier run must not
    // survive next to it (mcx_get_chol would return a mixture)
    HIPCHK(hipMemcpyAsync(e->cov.p, e->cov0.p, (size_t)e->ncov * sizeof(float), hipMemcpyDeviceToDevice, st));
    e->cov_offdiag = false;
  }
  e->cov_pending = false;
  r.lead = false;
  ra.nown = r.nown;
  const int nwg = std::min(r.nown, e->ncu);
  ra.own = (r.nown + nwg - 1) / nwg;
  ra.ksteps = mcxk_persist_ksteps(r.plpc2, r.pbpl, ra.own);
  MCXCHK(deal_table(r, ra));
  ra.deal = e->deal_tab.p;
  ra.trace_clk = nullptr;
  if (r.trace_file) {
    MCXCHK(e->trace_clk.alloc((size_t)PTRACE_WG * PWAVES * PTRACE_PH * 2));
    HIPCHK(hipMemsetAsync(e->trace_clk.p, 0, (size_t)PTRACE_WG * PWAVES * PTRACE_PH * 2 * sizeof(unsigned long long), st));
    ra.trace_clk = e->trace_clk.p;
  }
  ra.meet_timeout = (unsigned long long)e->opt_meet_timeout_ms * 100000ull;  // s_memrealtime: 100 MHz
  ra.meet_expect_extra = e->opt_debug_meet;
  // the launch that ends the run -- nothing of the plan left, variances and slot written by itself, accept counts its
  // own -- also tells the host: no counters' copy behind it
  ra.report = nullptr; ra.report_done = nullptr; ra.report_serial = 0;
  if (e->opt_self_report && s.plan_over && (ra.final_publish || r.nsamp == 0) && !r.slots_used && !r.sink && !e->ofn &&
      !e->opt_profile && e->size == 1) {
    r.reported = ++e->report_serial;
    ra.report = r.hctr;
    ra.report_done = reinterpret_cast<unsigned *>(e->ctr.p + (size_t)CTR_WORDS * CTR_RING);
    ra.report_serial = r.reported;
  }
  if (s.snap_after >= 0) MCXCHK(slot_rewritten(e, is0 + s.snap_after + 1));
  if (ra.final_publish) {
    MCXCHK(slot_rewritten(e, r.nsamp));
    r.sig_done = true;
  }
  // tuner events inside: exclusive on this GPU until the kernel has completed.  The lock is given back at
  // the run's next synchronisation with the stream -- before any user hook may block this thread, at the latest
  // at the end of the run
  if (pb > 0) MCXCHK(meet_lock_take(e));
  ProfScope ps(e, MCX_K_RUN_SMALL, (uint64_t)(pb + pm) * r.n);
  const hipError_t le = e->lik.kind == LIK_USER ? user_lik_launch_small(*e->lik.user, r.pbpl, ra, st, &e->steps)
                                                : mcxk_launch_persist(e->lpc, r.pbpl, e->lik.kind, ra, st, &e->steps);
  if (le != hipSuccess) (void)meet_release(e, true);
  if (le == hipErrorCooperativeLaunchTooLarge) {  // the grid cannot be resident at once on this device
    (void)hipGetLastError();
    return MCX_INTERNAL_MEET_ABANDONED;
  }
  HIPCHK(le);
  if (pb > 0) {  // looked at by meet_release, at the latest at the end of the run
    e->meet_check = true;
    e->meet_word = r.ctrp + 5;
  }
  e->cnt.small_n_launches++;
  e->cnt.small_n_blocks_per_lane = (uint64_t)r.pbpl;
  return MCX_OK;
}

// the per-step kernels (MCX_OPT_FUSE = 0, or a likelihood without a fused kernel): propose, evaluate, accept
static int run_unfused_steps(Run &r, bool main, int isamp, int steps)
{
  mcx_engine *e = r.e;
  const uint32_t t0 = e->tbase + (uint32_t)(main ? r.nburn : 0) + (uint32_t)isamp;
  r.slots_used = true;
  for (int s = 0; s < steps; ++s) {
    StepArgs a;
    if (main) fill_step(e, a, t0 + (uint32_t)s, isamp + s, true, (size_t)(r.nburn + isamp + s), isamp + s, 0);
    else fill_step(e, a, t0 + (uint32_t)s, 0, false, (size_t)(isamp + s), 0, 0);
    MCXCHK(launch_propose(e, a));
    MCXCHK(eval_trials(e, e->ptrial.p, e->lytrial.p, (uint64_t)r.n));
    MCXCHK(launch_accept(e, a, main));
    if (main) MCXCHK(discarded_calls(e));  // :177-182, on request
  }
  return MCX_OK;
}

// src/mcpar.cc:58-75; *folded: the MCX_PLAN_TUNER item behind the segment went into its launch
static int run_burn_segment(Run &r, size_t pi, bool *folded)
{
  mcx_engine *e = r.e;
  const mcx_plan_item &it = r.plan[pi];
  *folded = false;
  if (!r.fused) return run_unfused_steps(r, false, it.first, it.nsteps);
  SegArgs sa = r.sa;
  sa.samp_x = sa.samp_ly = nullptr;
  sa.mask = e->opt_mask ? e->mask.p + (size_t)it.first * r.n : nullptr;
  sa.nsteps = it.nsteps; sa.t0 = e->tbase + (uint32_t)it.first; sa.isamp0 = 0;
  // the tuner event that follows the segment: inside the launch where the kernel can (its last workgroup)
  const bool fold = pi + 1 < r.plan.size() && r.plan[pi + 1].kind == MCX_PLAN_TUNER && fused_takes_epilogue(e, sa);
  if (fold) {
    sa.tun.on = 1;
    sa.tun.check = r.plan[pi + 1].aux;
    sa.tun.add_trials = (unsigned long long)r.plan[pi + 1].nsteps * (unsigned long long)r.n;
  }
  {
    ProfScope ps(e, MCX_K_FUSED_BURN, (uint64_t)it.nsteps * r.n);
    MCXCHK(launch_fused(e, false, sa, r.st));
  }
  *folded = fold;
  if (!fold) r.slots_used = true;
  return MCX_OK;
}

// src/mcpar.cc:152-209 with genLocal
static int run_main_segment(Run &r, const mcx_plan_item &it)
{
  mcx_engine *e = r.e;
  const int isamp = it.first, steps = it.nsteps;
  if (!r.fused) return run_unfused_steps(r, true, isamp, steps);
  SegArgs sa = r.sa;
  const size_t row0 = e->opt_stride == 1 ? (size_t)isamp : 0;  // thinned: the kernel indexes from step 0
  float *vx = nullptr, *vl = nullptr;
  if (e->opt_samples) samp_vbase(e, isamp, &vx, &vl);
  sa.samp_x = e->opt_samples ? vx + row0 * e->ntot : nullptr;
  sa.samp_ly = e->opt_samples ? vl + row0 * r.n : nullptr;
  sa.mask = e->opt_mask ? e->mask.p + (size_t)(r.nburn + isamp) * r.n : nullptr;
  sa.nsteps = steps; sa.t0 = e->tbase + (uint32_t)r.nburn + (uint32_t)isamp; sa.isamp0 = isamp;
  sa.snap_after = it.aux;
  if (it.aux >= 0) MCXCHK(slot_rewritten(e, isamp + it.aux + 1));
  sa.init_moments = r.init_pending ? 1 : 0;
  r.init_pending = false;
  // hot-path kernels count their accepted proposals themselves (SegArgs::tun.on = 2), and the one that holds the
  // run's last step leaves the variances and this shard's slot behind (one shard: no gather may want the slot as
  // of the last sync point): no k_reduce_slots / k_variance / k_publish at the end of the run
  const bool self = fused_takes_epilogue(e, sa);
  sa.tun.on = self ? 2 : 0;
  if (self && e->size == 1 && isamp + steps == r.nsamp && it.aux < 0) {
    sa.snap_after = steps - 1;
    sa.sig_out = e->sig.p;
    e->published_steps = r.nsamp;
    r.sig_done = true;
  }
  {
    ProfScope ps(e, MCX_K_FUSED_MAIN, (uint64_t)steps * r.n);
    MCXCHK(launch_fused(e, true, sa, r.st));
  }
  if (!self) r.slots_used = true;
  return MCX_OK;
}

// src/mcpar.cc:152-175 with genRemote
static int run_remote_step(Run &r, int isamp)
{
  mcx_engine *e = r.e;
  MCXCHK(meet_release(e, false));  // (genRemote synchronises with the stream after every pass anyway)
  const uint32_t t = e->tbase + (uint32_t)r.nburn + (uint32_t)isamp;
  int npass = 0;
  MCXCHK(remote_device(e, t, e->pvals.p, e->musigall.p, e->ptrial.p, e->cfac.p, e->mutrial.p,
                       e->sigtrial.p, &npass));
  e->cnt.remote_steps++;
  e->cnt.remote_passes += (uint64_t)npass;
  MCXCHK(eval_trials(e, e->ptrial.p, e->lytrial.p, (uint64_t)r.n));  // :160
  StepArgs a;
  fill_step(e, a, t, isamp, true, (size_t)(r.nburn + isamp), isamp, 1);
  MCXCHK(launch_accept(e, a, true));
  MCXCHK(discarded_calls(e));  // :177-182, on request
  r.slots_used = true;
  return MCX_OK;
}

// the plan, item by item; in small-n mode stretch by stretch where one launch takes several items
static int execute_plan(Run &r)
{
  mcx_engine *e = r.e;
  const std::vector<mcx_plan_item> &plan = r.plan;
  for (size_t pi = 0; pi < plan.size(); ++pi) {
    const mcx_plan_item &it = plan[pi];
    if (r.persist) {
      if (e->xchg_pending && it.kind == MCX_PLAN_BURN_SEGMENT && e->opt_meet_under_gather <= 0) {
        // The last run's final gather is still in flight (finish_tail) and this launch has tuner meetings: every one
        // of its workgroups must become resident while the gather's kernel holds whatever it holds -- and that kernel
        // may itself be waiting for a peer GPU whose gather kernel cannot start beside the peer's small-n launch.  No
        // such cycle can form if the launch with meetings starts behind the gather: the step stream waits for it here
        // (MCX_OPT_MEET_UNDER_GATHER = 1 lets the burn-in run under the gather instead; the meetings' timeout is then
        // the net).  Launches without meetings have no workgroup waiting for another and need no such care.
        MCXCHK(exchange_wait(e));
      }
      const SmallStretch s = small_stretch(plan, pi, r.nsamp, e->xchg_pending);
      if (s.burn + s.main > 0) {
        MCXCHK(launch_small_stretch(r, s));
        pi = s.end - 1;
        continue;
      }
    }
    const int isamp = it.first, steps = it.nsteps;
    switch (it.kind) {
    case MCX_PLAN_BURN_SEGMENT: {
      bool folded = false;
      MCXCHK(run_burn_segment(r, pi, &folded));
      if (folded) ++pi;
      break;
    }
    case MCX_PLAN_TUNER: {  // src/mcpar.cc:77-96
      ProfScope ps(e, MCX_K_TUNER, 0);
      hipLaunchKernelGGL(k_tuner, dim3(1), dim3(BLOCK), 0, r.st, r.ctrp, e->cov.p, e->ncov,
                         (unsigned long long)steps * (unsigned long long)r.n, it.aux, e->TGT_ARATE_MIN,
                         e->TGT_ARATE_MAX, e->SCALE_DEC, e->SCALE_INC, e->trace.p, e->ntrace.p, e->acc_slots.p,
                         e->nslots);
      HIPCHK(hipGetLastError());
      break;
    }
    case MCX_PLAN_INIT_MOMENTS:  // src/mcpar.cc:99-104
      if (r.fused && pi + 1 < plan.size() && plan[pi + 1].kind == MCX_PLAN_MAIN_SEGMENT) {
        SegArgs probe = r.sa;
        probe.mask = e->opt_mask ? e->mask.p : nullptr;
        probe.nsteps = plan[pi + 1].nsteps;
        if (fused_takes_epilogue(e, probe)) {  // the segment's kernel starts from (0, FPEPS) instead of loading them
          r.init_pending = true;
          break;
        }
      }
      hipLaunchKernelGGL(k_init_moments, dim3(nblocks((size_t)e->ntot)), dim3(BLOCK), 0, r.st, e->mu.p,
                         e->psum2.p, (size_t)e->ntot);
      HIPCHK(hipGetLastError());
      break;
    case MCX_PLAN_OUTPUT:  // src/mcpar.cc:115-119
      HIPCHK(hipStreamSynchronize(r.st));
      MCXCHK(meet_release(e, true));
      e->samp_steps = e->opt_samples ? (isamp + e->opt_stride - 1) / e->opt_stride : 0;
      if (e->ofn(e->octx, isamp) != 0) return fail(MCX_ERR_INVALID, "output hook failed");
      break;
    case MCX_PLAN_SINK: MCXCHK(sink_block_done(e, isamp, steps, r.sink_seq++)); break;
    case MCX_PLAN_PUBLISH: MCXCHK(publish(e, isamp)); break;
    case MCX_PLAN_GATHER_BEGIN: MCXCHK(exchange_begin(e)); break;  // src/mcpar.cc:127-140
    case MCX_PLAN_GATHER_WAIT:
      if (isamp == r.nsamp && e->xchg_pending && exchange_tail_may_stay_in_flight(e) &&
          pi + 2 == plan.size() && plan[pi + 1].kind == MCX_PLAN_PUBLISH) {
        e->tail_publish = r.nsamp;  // finish_tail: the run's last gather stays in flight
        ++pi;
        break;
      }
      MCXCHK(exchange_wait(e));
      break;
    case MCX_PLAN_REMOTE_STEP: MCXCHK(run_remote_step(r, isamp)); break;
    case MCX_PLAN_MAIN_SEGMENT: MCXCHK(run_main_segment(r, it)); break;
    default: return fail(MCX_ERR_INVALID, "internal: unknown plan item %d", it.kind);
    }
  }
  return MCX_OK;
}

// what both ends of a run leave in the engine's books
static void note_run_done(Run &r, int samp_steps)
{
  mcx_engine *e = r.e;
  e->samp_steps = samp_steps;
  e->last_nsamp = r.nsamp;
  e->last_nburn = r.nburn;
  e->have_run = true;
  e->tbase += (uint32_t)(r.nburn + r.nsamp);
}

// MCX_OPT_ASYNC_RUN: everything is queued -- return.  Only runs whose end needs nothing from the host: one shard, no
// sink / output hook / host likelihood, no Murray step (a pass waits for its survivors' count), no profiling.
static bool may_end_async(const Run &r)
{
  const mcx_engine *e = r.e;
  bool go_async = e->opt_async_run && !r.rerun && e->size == 1 && !r.sink && !e->ofn && r.nsamp > 0 && e->lik.kind != MCX_VL_HOST &&
                  !e->opt_profile && !e->trace_clk.p;
  for (const mcx_plan_item &it : r.plan) go_async = go_async && it.kind != MCX_PLAN_REMOTE_STEP && it.kind != MCX_PLAN_OUTPUT;
  return go_async;
}

static int finish_async(Run &r)
{
  mcx_engine *e = r.e;
  hipStream_t st = r.st;
  if (r.pinit) {  // a repeat (abandoned meeting) must not need the caller's memory again
    MCXCHK(e->pinit_async.alloc((size_t)e->ntot));
    HIPCHK(hipMemcpyAsync(e->pinit_async.p, r.pinit, (size_t)e->ntot * sizeof(float), hipMemcpyHostToDevice, st));
  }
  // the counters' way to the host on a stream of its own, behind an event: on the step stream the copy would sit between
  // this run's last kernel and the next run's first one (5-8 us of every queued job)
  const int sl = e->hctr_slot;
  if (r.reported && !r.pinit) {  // (the run's last launch is the last thing on the stream and reports itself: nothing to add)
    e->slot_serial[sl] = r.reported;
    e->run_queued[sl] = true;
  } else {
    r.reported = 0;
    MCXCHK(e->astream.ensure(hipStreamNonBlocking));
    MCXCHK(e->run_ev[sl].ensure(hipEventDisableTiming));
    MCXCHK(e->copy_ev[sl].ensure(hipEventDisableTiming));
    HIPCHK(hipEventRecord(e->run_ev[sl], st));
    e->run_queued[sl] = true;
    HIPCHK(hipStreamWaitEvent(e->astream, e->run_ev[sl], 0));
    HIPCHK(hipMemcpyAsync(r.hctr, r.ctrp, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->astream));
    HIPCHK(hipEventRecord(e->copy_ev[sl], e->astream));
    e->copy_pending[sl] = true;
  }
  e->ht_mark[1] = std::chrono::steady_clock::now();
  e->pend.active = true;
  e->pend.slot = sl;
  e->pend.nsamp = r.nsamp; e->pend.nburn = r.nburn; e->pend.tbase0 = e->tbase;
  e->pend.meet_check = e->meet_check; e->pend.hctr = r.hctr; e->pend.host_pinit = r.pinit != nullptr;
  e->pend.serial = r.reported;
  e->meet_check = false;  // (finish_pending looks at the word itself)
  note_run_done(r, e->opt_samples ? r.nkeep : 0);
  return MCX_OK;
}

static int finish_sync(Run &r)
{
  mcx_engine *e = r.e;
  hipStream_t st = r.st;
  unsigned long long *const hctr = r.hctr;
  const unsigned long long reported = r.reported;
  if (!reported) HIPCHK(hipMemcpyAsync(hctr, r.ctrp, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  e->ht_mark[1] = std::chrono::steady_clock::now();
  {
    hipError_t se = hipSuccess;
    // (spinning only for runs of the length the last one had: whoever runs 10 ms jobs sleeps as ever)
    const auto w0 = std::chrono::steady_clock::now();
    if (!(reported && e->report_wait_us < (double)REPORT_SPIN_US && report_arrived(hctr, reported, REPORT_SPIN_US))) se = hipStreamSynchronize(st);
    if (reported) e->report_wait_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - w0).count();
    if (se == hipSuccess && reported && __atomic_load_n(hctr + 7, __ATOMIC_ACQUIRE) != reported) {
      (void)meet_release(e, true);
      return fail(MCX_ERR_HIP, "internal: the run's last launch is over and has not reported");
    }
    e->ht_mark[2] = std::chrono::steady_clock::now();
    const bool abandoned = e->meet_check && se == hipSuccess && hctr[5] != 0;  // (the word came with the counters)
    e->meet_check = false;
    (void)meet_release(e, true);
    HIPCHK(se);
    if (abandoned) return MCX_INTERNAL_MEET_ABANDONED;
  }
  e->cnt.naccept_burn = hctr[3];
  e->cnt.naccept_main = hctr[4];
  xwait_collect(e);
  if (e->trace_clk.p && r.trace_file) {  // debug: the phase clocks of the run's last small-n launch, as raw u64 words
    std::vector<unsigned long long> h((size_t)PTRACE_WG * PWAVES * PTRACE_PH * 2);
    HIPCHK(hipMemcpy(h.data(), e->trace_clk.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (FILE *f = fopen(r.trace_file, "wb")) {
      (void)fwrite(h.data(), sizeof(unsigned long long), h.size(), f);
      fclose(f);
    }
  }
  if (r.sink) MCXCHK(sink_drain(e, r.sink_seq));
  note_run_done(r, (e->opt_samples && !r.sink) ? r.nkeep : 0);
  prof_collect(e);
  if (e->ofn && e->ofn(e->octx, r.nsamp) != 0) return fail(MCX_ERR_INVALID, "output hook failed");  // :212
  return MCX_OK;  // :213
}

static int run_once(mcx_engine *e, int nsamp, int nburn, const float *pinit, const mcx_vlfunc *L, const float *incov, bool rerun)
{
  if (nsamp < 0 || nburn < 0) return fail(MCX_ERR_INVALID, "bad run arguments");
  Run r;
  r.e = e; r.nsamp = nsamp; r.nburn = nburn; r.rerun = rerun;
  // the state a run without `pinit` starts from: what mcx_stage_pinit put there, or (the repeat of an asynchronous run
  // that started from caller memory) the copy kept of that memory
  r.staged = (rerun && e->pend.host_pinit) ? e->pinit_async.p : e->pinit_dev.p;
  r.pinit = rerun ? nullptr : pinit;
  if (!pinit && !rerun && !e->pinit_staged) return fail(MCX_ERR_INVALID, "pinit is NULL and no state was staged (mcx_stage_pinit)");
  if (e->size > 1 && !e->xfn) return fail(MCX_ERR_EXCHANGE, "nshards > 1 needs mcx_set_exchange()");
  r.n = e->nchain; r.d = e->nparam; r.st = e->stream;
  if (!rerun) {
    MCXCHK(lik_setup(e->lik, L, r.d, r.st));
    MCXCHK(covar_install(e, incov, nullptr, false));  // src/mcpar.cc:20
  } else {
    e->cov_pending = true;  // the factor as installed (cov0), rescaled by nothing yet
  }
  e->cull_skip[0] = e->cull_skip[1] = 0;  // a new job starts from pinit: what the last one's Murray sweeps found useless is no guide
  MCXCHK(prepare_outputs(r));
  r.fused = e->opt_fuse && e->lik.fusable();
  r.g0 = (uint32_t)(e->rank * r.n);
  const char *tf = getenv("MCX_PERSIST_TRACE");
  r.trace_file = (tf && *tf) ? tf : nullptr;
  small_n_config(r);
  MCXCHK(claim_counter_slots(r));
  MCXCHK(reset_state(r));

  e->ht_mark[0] = std::chrono::steady_clock::now();
  r.sa = segment_template(r);
  r.init_pending = r.sig_done = r.slots_used = false;
  r.sink_seq = 0;
  const PlanCfg cfg = {nsamp, nburn, e->SYNCSTEP, e->PLOCAL, e->seed, e->tbase, e->size > 1, e->opt_eager != 0,
                       r.fused, e->ofn != nullptr, e->opt_maxseg, r.sink ? r.sblock : 0};
  r.plan = build_plan(cfg);
  MCXCHK(execute_plan(r));

  e->cnt.nsteps_burn = (uint64_t)nburn;
  e->cnt.nsteps_main = (uint64_t)nsamp;
  if (nsamp > 0 && !r.sig_done) {
    hipLaunchKernelGGL(k_variance, dim3(nblocks((size_t)e->ntot)), dim3(BLOCK), 0, r.st, e->psum2.p,
                       e->sig.p, (size_t)e->ntot, 1.0f / (float)nsamp);
    HIPCHK(hipGetLastError());
  }
  if (r.slots_used) {
    hipLaunchKernelGGL(k_reduce_slots, dim3(1), dim3(BLOCK), 0, r.st, e->acc_slots.p, e->nslots, r.ctrp + 4);
    HIPCHK(hipGetLastError());
  }
  MCXCHK(cov_reset(e));  // (a run without any step)
  return may_end_async(r) ? finish_async(r) : finish_sync(r);
}
