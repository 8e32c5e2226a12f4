/*
 * mcx.h -- C ABI of the MI355X-native parallel Metropolis-Hastings engine (libmcx.so).
 *
 * This is the drop-in boundary for the chain-step hot path of rplzzz/mcpar.  The reference has
 * no C ABI of its own (its plug-in mechanism is a C++ abstract class linked into the same
 * executable), so each entry point below cites the C++ member of the reference it replaces; the
 * reference-compatible C++ classes (include/mcpar/{vlfunc,mcpar,mcout,rosenbrock}.hh) are thin
 * shims over these functions.  See INTEGRATION.md for the binding a maintainer would add.
 *
 * Plain pointers and sizes only.  Unless a parameter says "device", pointers are host memory.
 * All arithmetic is float32 ("MCX arithmetic v3"); accept decisions are bit-exact
 * against oracle/mcx_oracle.c for a fixed seed.
 *
 * Every function returns MCX_OK (0) or an mcx_status; mcx_last_error() gives the message.
 * There is no CPU fallback: without a gfx950 device every compute entry point fails with
 * MCX_ERR_NO_DEVICE.
 */
#ifndef MCX_H_
#define MCX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCX_ABI_VERSION 5

typedef enum mcx_status {
  MCX_OK = 0,
  MCX_ERR_INVALID = 1,     /* bad argument (the reference throws a string literal: src/mcpar.cc:268) */
  MCX_ERR_NO_DEVICE = 2,   /* no HIP device / not gfx950 */
  MCX_ERR_HIP = 3,         /* a HIP call failed (the reference abort()s on VSL errors: src/mcpar.hh:93) */
  MCX_ERR_UNSUPPORTED = 4, /* np > 256 */
  MCX_ERR_ALLOC = 5,       /* sample store does not fit (reference: exit(2), src/mcpar.cc:34-40) */
  MCX_ERR_EXCHANGE = 6,    /* exchange hook failed / missing (reference: MPI_Abort, src/mcpar.cc:133-137) */
  MCX_ERR_VLFUNC = 7,      /* host likelihood callback missing */
  /* ABI 5 */
  MCX_ERR_NONFINITE = 8    /* a Murray step could not end: a NaN among the gathered per-chain moments, or chains still rejected
                              after MCX_OPT_MURRAY_MAX_PASSES passes (the reference loops for ever, src/mcpar.cc:443).
                              mcx_last_error names the step and the global chain; the run stops before that step: state,
                              log L, moments and sample rows are those of the steps before it */
} mcx_status;

/* ---- likelihood plug-in: replaces class VLFunc (src/vlfunc.hh:9-12) ---------------------- */
enum {
  MCX_VL_ROSENBROCK1 = 1, /* Rosenbrock1::operator()  src/rosenbrock.cc:4-21   (fused on device) */
  MCX_VL_ROSENBROCK2 = 2, /* Rosenbrock2::operator()  src/rosenbrock.cc:25-41  as written (device, unfused) */
  MCX_VL_GAUSSIAN = 3,    /* Gaussian::operator()     src/rosenbrock.cc:44-61  any d      (fused) */
  MCX_VL_DUALGAUSS = 4,   /* DualGaussian::operator() src/rosenbrock.cc:63-78             (fused) */
  MCX_VL_GAUSSMIX = 5,    /* N-D K-component unit-variance mixture (BASELINE config 5)    (fused) */
  MCX_VL_ROSENBROCK2_FIXED = 6, /* NOT reference behaviour, a flagged variant: the overlapping Rosenbrock function made
                             well-posed -- src/rosenbrock.cc:25-41 with '+' on the second term (the '-' at :38 leaves
                             log L unbounded above) and the loop kept inside each parameter set:
                             - sum_{k < d-1} (1 - x_k)^2 + 100 (x_{k+1} - x_k^2)^2                      (fused) */
  MCX_VL_HOST = 100,      /* any user VLFunc subclass: device -> host callback -> device  */
  MCX_VL_DEVICE = 101,    /* user likelihood as a GPU kernel: stays on the device (see mcx_vlfunc.ctx) */
  MCX_VL_SOURCE = 102     /* user likelihood as HIP SOURCE of device functions, compiled into the engine's fused step
                             kernels at run time (hiprtc): one launch per segment like the built-ins (see below) */
};

/* MCX_VL_SOURCE -- the VLFunc contract (src/vlfunc.hh:9-12) for ONE parameter set, as device code the engine inlines into
 * its own step kernels.  ctx = the NUL-terminated source text, params / ncomp = `ncomp` floats handed to the functions as
 * `par` (copied to the device by mcx_run).  The text defines, in the global namespace, EITHER
 *
 *     __device__ float mcx_user_loglike(const float *x, int d, const float *par);      // log L of x[0..d-1]
 *
 * (x points to on-chip memory; every call sees one whole parameter set) OR, for likelihoods that are a sum over
 * blocks of four consecutive parameters -- the engine's own decomposition, one GPU lane per block --
 *
 *     #define MCX_USER_BLOCK_FORM
 *     __device__ float mcx_user_block(const float xb[4], int nv, int k0, int d, const float *par);
 *         // partial of parameters k0 .. k0+nv-1 (nv = 4 except in the last block when d % 4 != 0)
 *     #define MCX_USER_FINISH                                                            // optional
 *     __device__ float mcx_user_finish(float sum, int d, const float *par);             // log L from the sum (default: sum)
 *
 * The partials are added in the order of the built-ins, so a restatement of a built-in returns
 * its bits.  MCX_USER_NP (= np) and MCX_USER_LPC (= the number of 4-parameter blocks, rounded up to a power of two) are
 * defined when the text is compiled: loops over them unroll, small arrays stay in registers.  In the whole-vector form a
 * chain of np <= 16 is held by ONE lane (four blocks per lane) and the function runs once per chain; above that by
 * np / 16 lanes, each of which evaluates it.  "mcx_numerics.hpp" is already included: mcx::logf_v1, mcx::expf_v2, ... are the engine's (and the CPU
 * oracle's) own transcendentals.  Compiled with -O3 -ffp-contract=off (write fma explicitly: __builtin_fmaf), once per
 * (text, np) per process; a text that does not compile fails mcx_run with MCX_ERR_VLFUNC and the compiler's messages
 * in mcx_last_error().  Without libhiprtc: MCX_ERR_UNSUPPORTED (MCX_VL_DEVICE and MCX_VL_HOST remain).  A text in block form
 * also gets the one-launch small-n kernel (few chains: burn-in, tuner meetings and main loop in ONE launch), built when a
 * run first qualifies for it. */
int mcx_user_source_available(void); /* 1 / 0 (mcx_last_error says why not) */
/* the compile step alone, for a chain of np parameters (needs no GPU): MCX_OK and the code object's size, or MCX_ERR_VLFUNC */
int mcx_debug_user_source_compile(const char *source, int np, size_t *code_bytes);
/* the same for the one-launch small-n kernel (few chains: the whole run in one launch), which takes the block form only and is
 * built when a run first wants it: bpl = 1 or 2 blocks per lane, rec = with recorder wavefronts */
int mcx_debug_user_source_compile_small(const char *source, int np, int bpl, int rec, size_t *code_bytes);
/* For MCX_VL_DEVICE without a compiler at hand: source of a whole kernel
 *   extern "C" __global__ void f(int npset, const float *x, float *y)   -> *function = its hipFunction_t (for mcx_vlfunc.ctx) */
int mcx_user_kernel_compile(const char *source, const char *symbol, void **function);

/* same contract as VLFunc::operator()(int npset, const float *x, float *restrict y): x is
 * row-major [npset][d], y is [npset]; the return code is ignored like the reference's
 * (doc/userguide.tex:146-149).  Called on the thread that called mcx_run. */
typedef int (*mcx_host_fn)(void *ctx, int npset, const float *x, float *y);

typedef struct mcx_vlfunc {
  int kind;            /* MCX_VL_* */
  int d;               /* parameters per set; must equal the engine's np */
  int ncomp;           /* GAUSSMIX: number of components K (<= 64); SOURCE: number of floats in params */
  const float *params; /* GAUSSIAN: mu[d], sig2[d] (NULL = standard normal); DUALGAUSS: w;
                          GAUSSMIX: means[K*d], weights[K]; SOURCE: the user's `par`.  Copied by mcx_run. */
  mcx_host_fn fn;      /* HOST */
  void *ctx;           /* HOST: passed to fn.  SOURCE: const char *, the source text.  DEVICE: a hipFunction_t (from the caller's own code object,
                          hipModuleGetFunction) of a kernel with the VLFunc contract on device memory,
                            extern "C" __global__ void f(int npset, const float *x, float *y);
                          launched with 256-thread blocks, ceil(npset / 256) blocks, on the engine's
                          stream; thread i evaluates parameter set i (or any mapping covering all sets). */
} mcx_vlfunc;

/* batched likelihood on host buffers: the VLFunc call itself, runs the device kernel */
int mcx_vlfunc_eval(const mcx_vlfunc *f, int npset, const float *x, float *y);

/* ---- engine: replaces class MCPar (src/mcpar.hh:10-91) ------------------------------------ */
typedef struct mcx_engine mcx_engine;

/* MCPar::MCPar(np, nc, mpisiz, mpirank, pl, armin, armax, dfac, ifac, sync) src/mcpar.hh:32-33,
 * src/mcpar.cc:216-272.  nshards/shard replace mpisiz/mpirank (one shard per GPU/process; this
 * shard owns global chains [shard*nc, (shard+1)*nc)).  seed replaces the literal 8675309 of
 * src/mcpar.cc:271.  Runs on the current HIP device of the calling thread. */
int mcx_create(mcx_engine **out, int np, int nc, int nshards, int shard, float pl, float armin,
               float armax, float dfac, float ifac, int sync, uint32_t seed);
/* MCPar::~MCPar  src/mcpar.cc:274-299 */
int mcx_destroy(mcx_engine *e);

/* MCPar::run(nsamp, nburn, pinit, L, outsamples, incov)  src/mcpar.hh:36-37, src/mcpar.cc:17-214.
 * pinit[nc*np] and incov[np*np] (or NULL = identity) are copied.  Samples go to the engine's
 * HBM-resident sample store (mcx_samples_*), which plays the role of MCout's vector. */
int mcx_run(mcx_engine *e, int nsamp, int nburn, const float *pinit, const mcx_vlfunc *L,
            const float *incov);
/* Stage the initial chain state pinit[nc*np] in HBM ahead of time; a later mcx_run(..., pinit = NULL,
 * ...) starts from the staged copy (device-to-device) instead of reading host memory. */
int mcx_stage_pinit(mcx_engine *e, const float *pinit);

/* MCPar::genLocal(pvals, ptrial, cfac)  src/mcpar.hh:40, src/mcpar.cc:302-312.  t is the RNG
 * step index; host buffers [nc*np], [nc*np], [nc].  Uses the engine's current
 * Cholesky factor (mcx_covar_setup / last run). */
int mcx_gen_local(mcx_engine *e, uint32_t t, const float *pvals, float *ptrial, float *cfac);
/* MCPar::genRemote(pvals, musigall, ptrial, cfac)  src/mcpar.hh:41-42, src/mcpar.cc:315-451.
 * musigall[nshards*nc*np*2] interleaved (mu, sig^2).  mutrial/sigtrial[nc*np] are the side
 * outputs the reference keeps in members (sigtrial returned squared, :447-448); npass = number
 * of rejection passes.  MCX_ERR_NONFINITE: see mcx_status. */
int mcx_gen_remote(mcx_engine *e, uint32_t t, const float *pvals, const float *musigall,
                   float *ptrial, float *cfac, float *mutrial, float *sigtrial, int *npass);
/* MCPar::covar_setup(incov, cov)  src/mcpar.hh:38, src/mcpar.cc:454-484: cov[np*np] in/out,
 * identity if incov == NULL; also installs the factor in the engine. */
int mcx_covar_setup(mcx_engine *e, const float *incov, float *cov);

/* ---- inter-shard exchange: replaces MPI_Allgather(IN_PLACE, musigall) src/mcpar.cc:127-140 --
 * phase MCX_XCHG_BEGIN: start an in-place all-gather of musigall (device pointer, nshards slots
 * of slot_floats floats; this shard's slot is filled) ordered after the work already queued on
 * `stream` (a hipStream_t).  phase MCX_XCHG_WAIT: make `stream` wait for that gather.  A hook may
 * do all the work in BEGIN.  Required when nshards > 1. */
enum { MCX_XCHG_BEGIN = 0, MCX_XCHG_WAIT = 1 };
typedef int (*mcx_exchange_fn)(void *ctx, int phase, void *musigall_dev, size_t slot_floats,
                               int shard, int nshards, void *stream);
int mcx_set_exchange(mcx_engine *e, mcx_exchange_fn fn, void *ctx);

/* The exchange the library ships: an in-place ncclAllGather (RCCL over xGMI) of the musigall slots --
 * sendbuff = musigall + shard*2*ntot, 2*ntot floats per shard, the slot layout of src/mcpar.cc:206 -- on a
 * side stream, BEGIN = enqueue behind the engine's stream, WAIT = the engine's stream waits for it.
 * One process (or thread) per GPU, communicator rank = shard.  librccl.so.1 is loaded on first use.
 *   rank 0:     mcx_rccl_unique_id(id);  ship the MCX_RCCL_ID_BYTES bytes to every rank (MPI_Bcast, ...)
 *   every rank: mcx_exchange_rccl_init(e, id);     collective, like MPI_Comm_dup at src/mcpar.cc:228
 * or hand over a communicator the caller already has (ncclComm_t, rank == shard, nranks == nshards). */
#define MCX_RCCL_ID_BYTES 128
int mcx_rccl_available(void); /* 1 / 0 (mcx_last_error says why not) */
int mcx_rccl_unique_id(void *id);
int mcx_exchange_rccl_init(mcx_engine *e, const void *id);
int mcx_exchange_rccl_adopt(mcx_engine *e, void *nccl_comm);
int mcx_exchange_rccl_destroy(mcx_engine *e); /* also done by mcx_destroy */
/* what the installed RCCL exchange sees: ncclCommCount / ncclCommUserRank of its communicator (a launcher's
 * start-up check that every rank really joined); MCX_ERR_EXCHANGE when no RCCL exchange is installed */
int mcx_exchange_rccl_info(mcx_engine *e, int *nranks, int *rank);
/* run the installed exchange hook once, now (BEGIN, WAIT, drain): start-up self-check / tests */
int mcx_debug_exchange(mcx_engine *e);
/* fill this shard's musigall slot with `value` (start-up self-check of an exchange: every shard fills its slot with
 * its own number, mcx_debug_exchange, then mcx_get_musigall must show slot r full of shard r's number) */
int mcx_debug_fill_slot(mcx_engine *e, float value);

/* called where the reference dumps output (isamp % outstep == 0 && isamp > 0, and after the
 * last step: src/mcpar.cc:110-119,212) with the number of main-loop steps completed. */
typedef int (*mcx_output_fn)(void *ctx, int steps_done);
int mcx_set_output_hook(mcx_engine *e, mcx_output_fn fn, void *ctx);

/* Streaming sample sink: the role of MCout as the reference fills it (src/mcpar.cc:176-182) and dumps it every
 * outstep steps (:110-119), for runs whose samples should not all stay in HBM.  With a sink installed the
 * engine keeps only a ring of 4 blocks of `block_steps` main-loop steps on the device; when a block is complete
 * its rows -- MCout layout, np+1 columns, step-major then chain -- are interleaved on the device and copied to
 * pinned host memory on a second stream while the step stream goes on with the next blocks, and fn is called on
 * the thread that called mcx_run with rows valid for the duration of the call (first_step / nsteps count KEPT
 * steps, see MCX_OPT_SAMPLE_STRIDE).  nsamp is then bounded by nothing but the int32 range; mcx_samples_copy
 * serves only what the ring still holds, mcx_samples_maxlike keeps its running maximum on the device.
 * fn == NULL removes the sink.  block_steps is rounded up to a multiple of the sample stride. */
typedef int (*mcx_sink_fn)(void *ctx, int first_step, int nsteps, const float *rows);
int mcx_set_sink(mcx_engine *e, mcx_sink_fn fn, void *ctx, int block_steps);
/* The same sink, but every block arrives as the TEXT MCout::output prints for its rows (src/mcout.cc:41-45; see
 * mcx_samples_text), formatted on the device: nbytes characters, no terminating 0, valid during the call.  One of the
 * two sinks at a time: setting one removes the other. */
typedef int (*mcx_text_sink_fn)(void *ctx, int first_step, int nsteps, const char *text, size_t nbytes);
int mcx_set_text_sink(mcx_engine *e, mcx_text_sink_fn fn, void *ctx, int block_steps);
/* inside a row sink's callback of a run with MCX_OPT_SINK_TEXT: the same block as text (valid during the callback) */
int mcx_sink_text(mcx_engine *e, const char **text, size_t *nbytes);

/* ---- options ------------------------------------------------------------------------------ */
enum {
  MCX_OPT_SAMPLES = 1,     /* 0 none, 1 keep every (step, chain) row in HBM (reference semantics,
                              src/mcpar.cc:177-182) [default 1] */
  MCX_OPT_ACCEPT_MASK = 2, /* 1: record one byte per (step, chain), burn-in and main [default 0] */
  MCX_OPT_FUSE = 3,        /* 1: multi-step fused kernel for local steps [default 1]; 0: one
                              propose/eval/accept kernel triple per step (same bits) */
  MCX_OPT_MAX_SEGMENT = 4, /* upper bound on steps per fused launch [default 256] */
  MCX_OPT_PROFILE = 5,     /* 1: bracket every kernel launch with HIP events (slower) */
  MCX_OPT_STREAM = 6,      /* value = hipStream_t to run on (default: engine-owned stream) */
  MCX_OPT_SAMPLE_STRIDE = 8, /* k >= 1: keep only main-loop steps with isamp % k == 0 in the sample store
                              (thinning; the reference keeps every step, k = 1) [default 1] */
  MCX_OPT_SPLIT_RNG = 9,   /* small-n mode: random numbers of 32-256 steps at a time from a separate, fully parallel
                              kernel, streamed into the step kernel (same bits).  -1 auto [default: when the
                              chains fill fewer than 640 wavefronts], 0 off, 1 on */
  MCX_OPT_PERSIST = 10,    /* small-n mode, one launch per stretch of local steps: the burn-in with its tuner, the start of
                              the main loop and the local main-loop steps run in ONE kernel whose owner wavefronts keep
                              the chains while the other wavefronts of each CU generate their random numbers into LDS
                              (same bits).  -1 auto [default: when the chains fill at most 8 wavefronts per CU and
                              SPLIT_RNG is not 0], 0 off, 1 on */
  MCX_OPT_EAGER_EXCHANGE = 7, /* 0 [default]: gather the latest sync-point snapshot only when a Murray step (or
                              the end of the run) will read it -- bit-identical to 1: gather at every sync
                              point like the reference (src/mcpar.cc:127-140), overlapped with compute */
  MCX_OPT_MEET_TIMEOUT_MS = 11, /* small-n mode: how long a tuner meeting of the one-launch kernel may wait for a
                              workgroup that is not resident (CU mask, partitioned device, foreign kernel) before
                              the launch is abandoned and the run repeated on the per-segment kernels (same bits;
                              mcx_counters.meet_timeouts counts it, MCX_VERBOSE=1 in the environment prints it; the engine
                              keeps to the per-segment kernels for 16 runs, then tries again) [default 50: a healthy
                              launch is 0.3-1.3 ms long and its meetings wait microseconds] */
  MCX_OPT_CULL = 13,       /* Murray sweeps: exclude, exactly, the Gaussians that are too far from all 128 chains of a
                              wavefront to matter (the chains are sorted spatially first; same bits).  Three screens:
                              (3) a lower bound of arg for every (chain, Gaussian) PAIR on the matrix cores -- a bf16
                              product with its rounding bounded rigorously, reduced over the 128 chains
                              (mcx_screen.hpp): leaves 6 % of C3-murray's pairs and 54 % of C5's; (1) boxes of four
                              coordinates around the 128 chains (33 % / 100 %); (2) one direction -- the chains' first
                              principal axis -- with a Cauchy-Schwarz bound along it (for targets stretched along a
                              line; on BASELINE's shapes it excludes less than the boxes).  -1 auto [default: the
                              per-pair bound, with np = 16 or 32, >= 4096 chains still rejected, >= 4096 Gaussians],
                              0 off, 1 / 2 / 3: that screen whenever np allows */
  MCX_OPT_BLOCKS_PER_LANE = 14, /* hot-path kernel: consecutive 4-parameter blocks of a chain held by one lane -- 1: one
                              (np/4 lanes per chain), 2 or 4: fewer lanes per chain, the per-chain work (acceptance test,
                              selects, counters) paid once per 2 / 4 blocks (same bits).  0 auto [default] */
  MCX_OPT_ASYNC_TAIL = 15,   /* sharded runs on the library's RCCL exchange: mcx_run returns while the run's LAST all-gather
                              (which nothing inside the run reads) is still in flight on its side stream; whatever looks
                              at the gathered slots next -- mcx_get_musigall, the next run's first gather or publish,
                              mcx_synchronize, mcx_destroy -- waits for it.  1 [default]: on a communicator the library made
                              itself (mcx_exchange_rccl_init); not on an adopted one, where the caller's own collectives
                              could overtake the pending gather on some ranks.  0: mcx_run always waits itself.  2: also with
                              an adopted communicator or a caller's exchange hook (whose MCX_XCHG_WAIT call then comes after
                              mcx_run has returned): call mcx_synchronize before anything else touches the communicator */
  MCX_OPT_SINK_TEXT = 16,    /* a row sink (mcx_set_sink) also gets every block as text: inside the callback, mcx_sink_text
                              returns the characters MCout::output would print for the block's rows [default 0] */
  MCX_OPT_ASYNC_RUN = 19,    /* 1: mcx_run returns as soon as the run is QUEUED (one shard, no sink / output hook / host likelihood,
                              no Murray step, samples > 0; other runs are waited for as ever).  Every other entry point -- the
                              getters, mcx_samples_*, mcx_get_counters, mcx_synchronize, mcx_set_option, mcx_destroy -- first
                              finishes it (waits, takes its counters, repeats a run whose tuner meeting was abandoned), so results
                              are what a synchronous run gives.  Calling mcx_run again before looking queues the next run behind
                              it (at most two in flight): launch and completion latency of back-to-back small jobs overlap the
                              jobs; the overtaken run's results are never seen (the next run overwrites them, as ever) and its
                              counters are not reported.  pinit / incov / the vlfunc are copied during the call as ever.
                              [default 0] */
  MCX_OPT_REFERENCE_CALLS = 20, /* 1: after every main-loop step call a HOST functor once per chain on (1, pvals_j, &y) and discard the
                              result, as the reference does (src/mcpar.cc:177-182): for functors whose side effects -- a call
                              counter, a cache -- must see the calls they see there.  Results do not change.  [default 0] */
  MCX_OPT_SELF_REPORT = 21, /* a run that ends with a launch of the one-launch small-n kernel (few chains, one shard, no sink or
                              output hook): 1: that launch's last workgroup writes the run's counters and a serial number to
                              pinned host memory and mcx_run spins on the word (for at most 1.5 ms, then sleeps in
                              hipStreamSynchronize as ever) -- nothing is queued behind the kernel: 6 us less per job of
                              0.3-0.5 ms waited for.  0: the counters come by a copy behind the kernel.  Same results.  [default 1] */
  MCX_OPT_MURRAY_OVERLAP = 18, /* Murray passes over many chains (np = 16 or 32, the per-pair screen): cut the Gaussians into this
                              many column chunks and screen chunk c + 1 (matrix cores, step stream) while chunk c is swept
                              (vector units, a side stream).  Same bits.  0 / 1: one screen, then one sweep */
  MCX_OPT_MURRAY_MAX_PASSES = 22, /* a Murray step (genRemote call) gives up with MCX_ERR_NONFINITE when chains are still rejected
                              after this many rejection passes: a backstop for moments no proposal can come from (sig^2 = +inf
                              from an overflowed variance, a negative sig^2 handed to mcx_gen_remote), not a tuned value
                              [default 10 000 000: DESIGN.md section 3; the longest call measured took 3 217]; <= 0: the default */
  MCX_OPT_MEET_UNDER_GATHER = 17 /* small-n mode, sharded runs: may a launch with tuner meetings -- whose workgroups must all
                              be resident at once -- start while this engine's own last gather is still in flight
                              (MCX_OPT_ASYNC_TAIL)?  0: no, the step stream waits for the gather first: no cycle of a
                              half-resident launch, its GPU's gather kernel and a peer's can form.  1: yes, the next
                              run's burn-in runs under the gather; MCX_OPT_MEET_TIMEOUT_MS is then the net.  -1 auto
                              [default] = 0 */
  /* (12 is taken by a test hook that is not part of this header) */
};
int mcx_set_option(mcx_engine *e, int opt, int64_t value);

/* ---- results ------------------------------------------------------------------------------ */
typedef struct mcx_counters {
  uint64_t naccept_burn, naccept_main; /* accepted proposals (the reference's float naccept, :43-44) */
  uint64_t nsteps_burn, nsteps_main;
  uint64_t remote_steps, remote_passes; /* genRemote calls / rejection passes */
  uint64_t exchanges;
  uint64_t kernel_launches;
  uint64_t remote_pairs; /* (chain, Q_i) pairs of the Murray sweeps as the reference loops over them: sum over
                            passes of n_active * N, plus n * N per genRemote call for the cfac numerator
                            (src/mcpar.cc:367-395, 421-437) */
  uint64_t remote_pairs_evaluated; /* the pairs whose arg the sweep kernels actually started to accumulate: the
                            rest were excluded by an exact bound (their Q_i is exactly 0, or cannot lower the running
                            minimum) before any per-pair work.  The late passes over a few hundred chains sweep the
                            next four passes' proposals at once (same results, same pass count): proposals a chain
                            then did not need are counted here and not in remote_pairs, so without a screen the
                            ratio of the two is a little above 1 */
  uint64_t meet_timeouts; /* runs repeated on the per-segment kernels because a tuner meeting of the one-launch
                            small-n kernel was abandoned (MCX_OPT_MEET_TIMEOUT_MS) */
  /* ABI 4 */
  uint64_t meet_timeouts_total; /* the same, over the engine's life (meet_timeouts is the last run's) */
  uint64_t small_n_launches;    /* launches of the one-launch small-n kernel in the last run (0: per-segment kernels) */
  uint64_t small_n_blocks_per_lane; /* 4-parameter blocks per lane those launches ran with (0 when there were none) */
  uint64_t exchange_waits;      /* times the step stream was made to wait for a gather (src/mcpar.cc:127-140) that had
                                   been begun earlier: the last run's waits, including a wait for the run before's tail */
  uint64_t exchange_wait_ns;    /* device time the step stream spent in those waits (HIP events around each wait) */
} mcx_counters;
int mcx_get_counters(mcx_engine *e, mcx_counters *c);

int mcx_get_state(mcx_engine *e, float *pvals);       /* [nc*np]  MCPar::pvals   */
int mcx_get_loglike(mcx_engine *e, float *ly);        /* [nc]     MCPar::lylast  */
int mcx_get_mean(mcx_engine *e, float *mu);           /* [nc*np]  MCPar::mu      */
int mcx_get_var(mcx_engine *e, float *sig);           /* [nc*np]  MCPar::sig (population variance) */
int mcx_get_musigall(mcx_engine *e, float *musigall); /* [nshards*nc*np*2] MCPar::musigall */
/* Wait for everything the last mcx_run left in flight on the device (MCX_OPT_ASYNC_TAIL: the last all-gather of a
 * sharded run and the slot's final publish behind it).  A launcher that times runs calls it before stopping the clock. */
int mcx_synchronize(mcx_engine *e);
int mcx_get_chol(mcx_engine *e, float *cov);          /* [np*np]  MCPar::cov after tuning */
int mcx_get_accept_counts(mcx_engine *e, uint32_t *counts); /* [nc] per chain, burn + main */
int mcx_get_accept_mask(mcx_engine *e, uint8_t *mask);      /* [(nburn+nsamp)*nc] of the last run */
int mcx_get_tuner_trace(mcx_engine *e, float *scales, int maxn, int *n); /* cov[0] after each check */

/* sample store of the last run, in MCout row format: (np+1) columns, step-major then chain
 * (src/mcout.cc:129-145).  rows = steps*nc. */
int mcx_samples_steps(mcx_engine *e, int *nsteps);
int mcx_samples_copy(mcx_engine *e, int first_step, int nsteps, float *rows);
/* The same rows as the text MCout::output prints for them (src/mcout.cc:41-45: every field as `ostream << float` with
 * the stream defaults, i.e. printf("%g"), two blanks behind it, a newline behind a row's last column), formatted on the
 * device -- that conversion is 65-87 % of the reference's wall time.  *nbytes = bytes of the text (no terminating 0);
 * text == NULL, capacity == 0: the size only.  A C3-sized block of 25 steps is ~270 MB of text: ask step ranges. */
int mcx_samples_text(mcx_engine *e, int first_step, int nsteps, char *text, size_t capacity, size_t *nbytes);
/* the same for any rows on the host (ncol columns each, e.g. what a sink was given): uploaded, formatted, copied back */
int mcx_format_rows(const float *rows, size_t nrows, int ncol, char *text, size_t capacity, size_t *nbytes);
/* running maximum-likelihood sample of this shard (MCout::add's maxlval, src/mcout.cc:140-144) */
int mcx_samples_maxlike(mcx_engine *e, float *lmax, float *params);

/* ---- summaries of the sample store, on the device (DESIGN.md "Sample-store summaries") ----
 * Per column (the np parameters, then log L) over N = nsteps * nc values.  Split chains: each chain's nsteps values
 * are cut into two halves of n = floor(nsteps / 2) (odd nsteps: the middle step is dropped), M = 2 nc half-chains.
 *   mean, sd   over all N values, sd with divisor N - 1
 *   min, max   exact, in float order (-inf < finite < +inf; -0 before +0); a NaN anywhere makes min, max and every
 *              quantile NaN (a NaN, payload unspecified)
 *   rhat       split R-hat: W = mean of the half-chain variances (divisor n - 1), B/n = variance of the half-chain means
 *              (divisor M - 1), var+ = (n - 1)/n W + B/n, rhat = sqrt(var+ / W)
 *   ess        split "basic" ESS (Geyer's initial positive and monotone sequences on the chain-averaged biased
 *              autocovariance, no rank normalisation), ess_lag the last lag its sum used; mcse_mean = sd / sqrt(ess)
 *   quantiles  R type 7 / numpy "linear" from exact order statistics: h = (N - 1) p, x(lo) + (h - lo)(x(lo+1) - x(lo))
 * A column holding an inf or NaN has MCX_SUMMARY_NONFINITE and NaN mean, sd, rhat, ess and mcse_mean.  A column that is
 * constant within every half-chain (W = 0) has NaN rhat, ess and mcse_mean. */
enum { MCX_SUMMARY_NONFINITE = 1 }; /* the column holds an inf or NaN */
typedef struct mcx_col_summary {
  double mean, sd;  /* over all N = nsteps*nc values of the column; sd with divisor N - 1 */
  float min, max;   /* exact */
  double rhat;      /* split R-hat */
  double ess;       /* split "basic" ESS, no rank normalisation */
  double mcse_mean; /* sd / sqrt(ess) */
  int ess_lag;      /* max_t of the ESS sum: the last lag it used */
  int flags;        /* MCX_SUMMARY_* */
} mcx_col_summary;
/* Steps [first_step, first_step + nsteps) of the store (kept steps, as mcx_samples_copy counts them), nsteps >= 4.
 * cols[np + 1]; quantiles[(np + 1) * nprobs], row = column (may be NULL when nprobs == 0); probs in [0, 1], nprobs <= 32.
 * MCX_ERR_INVALID when the store does not hold the range (no run yet, MCX_OPT_SAMPLES = 0, a run into a sink).  Works on
 * the engine's stream after a queued MCX_OPT_ASYNC_RUN run is finished; the same store and arguments give the same bytes. */
int mcx_samples_summary(mcx_engine *e, int first_step, int nsteps, const double *probs, int nprobs,
                        mcx_col_summary *cols, double *quantiles);
/* the same for rows on the host in MCout layout (np + 1 columns, step-major then chain, nsteps * nc rows), e.g. what
 * MCout collected from a sink: uploaded to a scratch store, summarised there */
int mcx_rows_summary(const float *rows, int nsteps, int nc, int np, const double *probs, int nprobs,
                     mcx_col_summary *cols, double *quantiles);

/* ---- rank-normalised summaries of the sample store, on the device ----
 * Vehtari, Gelman, Simpson, Carpenter & Buerkner (2021).  Columns, split chains, R-hat and ESS as above; N = nsteps * nc.
 *   ranks      r(v) = the 1-based position of v among all N values of the column in ascending order, equal values (-0 and
 *              +0 are equal) sharing the average of their positions; every step is ranked, the middle step of an odd
 *              nsteps included
 *   z(v)       = float(PPND16((r(v) - 0.375) / (N + 0.25))), Wichura's AS 241 in fp64
 *   q05, median, q95   the type-7 quantiles of the column: mcx_samples_summary's for probs (0.05, 0.5, 0.95), bit for bit
 *   rhat_bulk, ess_bulk, ess_bulk_lag   rhat, ess, ess_lag of the store of z(x)
 *   rhat_folded   rhat of the store of z(f), f = float(|x - median|);  rhat = max(rhat_bulk, rhat_folded)
 *   ess_q05, ess_q95   ess of the stores of the indicators x <= q05, x <= q95 (1.0f / 0.0f);  ess_tail = their min
 * A max or min over a NaN is NaN.  A column holding an inf or NaN has MCX_SUMMARY_NONFINITE and NaN in every double,
 * thresholds included; a transformed column that is constant within every half-chain gives NaN for what is built on it. */
typedef struct mcx_col_rank_summary {
  double rhat, rhat_bulk, rhat_folded;
  double ess_bulk, ess_tail, ess_q05, ess_q95;
  double q05, median, q95;      /* the thresholds used */
  int ess_bulk_lag, flags;      /* MCX_SUMMARY_* */
} mcx_col_rank_summary;
/* Steps [first_step, first_step + nsteps) of the store, nsteps >= 4, cols[np + 1].  MCX_ERR_INVALID in the cases
 * mcx_samples_summary refuses; MCX_ERR_ALLOC, with the bytes needed in mcx_last_error, when the scratch (4 N (np + 1) bytes
 * of transformed store and 8 N bytes of keys per column sorted at a time) does not fit even one column at a time;
 * MCX_ERR_UNSUPPORTED for N >= 2^31.  Works on the engine's stream after a queued MCX_OPT_ASYNC_RUN run is finished; the
 * same store and arguments give the same bytes. */
int mcx_samples_rank_summary(mcx_engine *e, int first_step, int nsteps, mcx_col_rank_summary *cols);
/* the same for host rows in MCout layout (np + 1 columns, step-major then chain, nsteps * nc rows) */
int mcx_rows_rank_summary(const float *rows, int nsteps, int nc, int np, mcx_col_rank_summary *cols);

/* ---- covariance of the sample store, on the device -----------------
 * Columns as above (the np parameters, then log L), N = nsteps * nc rows, nsteps >= 1 and N >= 2.
 *   mean[c]    = column sum / N: the number mcx_samples_summary reports, bit for bit
 *   cov[i][j]  = sum over the rows of (x_i - mean[i]) (x_j - mean[j]) / (N - 1), fp64 throughout, centred (two passes);
 *                the full symmetric matrix, row-major, cov[i][j] and cov[j][i] the same bits
 * A column holding an inf or NaN has MCX_SUMMARY_NONFINITE in flags[c], NaN mean[c] and NaN in row and column c of cov;
 * every other entry is what it would be without that column.  MCX_ERR_INVALID in the cases mcx_samples_summary refuses
 * (the store does not hold the range).  The same store and arguments give the same bytes.
 * mean[np+1], cov[(np+1)*(np+1)] row-major, flags[np+1] (MCX_SUMMARY_*; may be NULL) */
int mcx_samples_covariance(mcx_engine *e, int first_step, int nsteps, double *mean, double *cov, int *flags);
/* the same for host rows in MCout layout (what a sink / MCout collected): uploaded, computed on the device */
int mcx_rows_covariance(const float *rows, int nsteps, int nc, int np, double *mean, double *cov, int *flags);
/* host only, no device: the np x np parameter block of cov (leading dimension ld >= np), times scale
 * (scale <= 0: 2.38^2 / np, the Gaussian-target optimum of Gelman, Roberts & Gilks), rounded to float and made exactly
 * symmetric -> incov[np*np], ready for mcx_run / mcx_covar_setup / MCPar::run.  MCX_ERR_INVALID, with the column or
 * pivot named in mcx_last_error, when an entry is not finite or the float Cholesky mcx_covar_setup uses rejects it. */
int mcx_proposal_from_cov(int np, const double *cov, int ld, double scale, float *incov);

/* ---- derived columns and bootstrap draws of the sample store, on the device ----
 * The reference's mcparam.sample(mc.data, nsamp, func) (src/anly/mcpar-analysis.R:30-47).  A function f maps one row
 * (x[0..np-1], ly) to nout floats, 1 <= nout <= 256.  One sweep over a step range applies it to every row and writes a store
 * of the same shape: nout derived columns, then log L, copied, as the last column.  The same store and arguments give the
 * same bytes.
 *   MCX_DERIVE_LINEAR  par = A[nout][np] row-major, then b[nout]: npar = nout * (np + 1).  out[j]: acc = b[j], then for
 *                      k = 0 .. np-1 in that order acc = acc + A[j][k] * x[k], the product and the sum each rounded to
 *                      float32 (not an fma chain).  Compiled into the library: needs no hiprtc.
 *   MCX_DERIVE_SOURCE  source = NUL-terminated HIP text that defines, in the global namespace,
 *
 *     __device__ void mcx_user_derive(const float *x, int d, float ly, const float *par, float *out, int nout);
 *
 *                      par = the npar floats of the spec (may be 0 / NULL).  x and out point to on-chip memory: x[0..d-1]
 *                      is one row, out[0..nout-1] is written by the function (what it leaves unwritten is unspecified).
 *                      The function is called for rows of the range only, never for a lane without a row: it never sees
 *                      values that no run produced.  "mcx_numerics.hpp" is already included; MCX_DERIVE_NP (= np) and
 *                      MCX_DERIVE_NOUT (= nout) are defined.  Compiled like an MCX_VL_SOURCE text (-O3 -ffp-contract=off),
 *                      once per (text, np, nout) per process; a text that does not compile gives MCX_ERR_VLFUNC with the
 *                      compiler's messages under the text's own line numbers ("mcx_user_derive:LINE") in
 *                      mcx_last_error(); without libhiprtc MCX_ERR_UNSUPPORTED. */
enum { MCX_DERIVE_LINEAR = 1, MCX_DERIVE_SOURCE = 2 };
typedef struct mcx_derive {
  int kind;           /* MCX_DERIVE_* */
  int nout;           /* outputs per row, 1 to 256 */
  int npar;           /* floats in par */
  const float *par;   /* copied by the call */
  const char *source; /* SOURCE: the text */
} mcx_derive;
/* A derived store: it owns its device memory, a stream and the scratch of its analyses, and does not depend on the engine
 * it was derived from -- a later mcx_run or mcx_destroy of that engine leaves it intact.  One thread at a time per store. */
typedef struct mcx_store mcx_store;
/* Steps [first_step, first_step + nsteps) of the engine's store, nsteps >= 1: refused as mcx_samples_summary refuses a
 * range the store does not hold; a queued MCX_OPT_ASYNC_RUN run is finished first. */
int mcx_samples_derive(mcx_engine *e, int first_step, int nsteps, const mcx_derive *f, mcx_store **out);
/* the same for host rows in MCout layout (np + 1 columns, step-major then chain, nsteps * nc rows), np <= 256 */
int mcx_rows_derive(const float *rows, int nsteps, int nc, int np, const mcx_derive *f, mcx_store **out);
int mcx_store_destroy(mcx_store *s);
int mcx_store_shape(const mcx_store *s, int *nsteps, int *nc, int *ncol);      /* ncol = nout + 1 */
int mcx_store_copy(mcx_store *s, int first_step, int nsteps, float *rows);     /* MCout layout: rows[nsteps * nc][ncol] */
/* mcx_samples_summary, mcx_samples_rank_summary and mcx_samples_covariance of the whole derived store: the same device
 * passes under the same rules (nsteps >= 4 for the first two, nsteps * nc >= 2 for the third, MCX_SUMMARY_NONFINITE for
 * a column in which f produced an inf or NaN); cols[ncol], quantiles[ncol * nprobs], mean[ncol], cov[ncol * ncol] */
int mcx_store_summary(mcx_store *s, const double *probs, int nprobs, mcx_col_summary *cols, double *quantiles);
int mcx_store_rank_summary(mcx_store *s, mcx_col_rank_summary *cols);
int mcx_store_covariance(mcx_store *s, double *mean, double *cov, int *flags);
/* the compile step of an MCX_DERIVE_SOURCE text alone (needs no GPU): MCX_OK and the code object's size, or MCX_ERR_VLFUNC */
int mcx_debug_derive_compile(const char *source, int np, int nout, size_t *code_bytes);

/* Bootstrap draws: ndraw rows of the range (of the derived store), with replacement, as the reference's
 * sample.int(..., replace = TRUE).  The row of draw i among the N = nsteps * nc rows depends on (seed, i, N) only:
 *   w = Philox4x32-10(counter = (i & 0xffffffff, i >> 32, 0, 0), key = (seed, 5)), r = (w.x << 32) | w.y,
 *   index = (r * N) >> 64 (the high half of the 128-bit product); row index is step index / nc, chain index % nc.
 * (Stream 5: a run uses streams 0 to 4 of its seed.)  So mcx_samples_draw on a range and mcx_store_draw on the store derived
 * from that range pick the same rows: the derived draws are f of the draws.  rows[ndraw][ncol] in MCout layout, gathered on
 * the device; index[ndraw] may be NULL; ndraw = 0 is allowed. */
int mcx_samples_draw(mcx_engine *e, int first_step, int nsteps, uint32_t seed, int64_t ndraw, float *rows, int64_t *index);
int mcx_store_draw(mcx_store *s, uint32_t seed, int64_t ndraw, float *rows, int64_t *index);
/* host only: index[k] = the row of draw first + k among N rows, k < n */
int mcx_debug_draw_indices(uint32_t seed, uint64_t N, uint64_t first, int n, int64_t *index);

/* ---- densities of the sample store, on the device -------------------
 * The reference's mcparam.density (src/anly/mcpar-analysis.R:22-28): per column (the parameters, then log L; of a derived
 * store the nout outputs, then log L) the binned Gaussian kernel density estimate of R's density.default, which is what
 * geom_density evaluates.  N = nsteps * nc >= 2 values per column, a grid of n_g = 512 points, n output points.
 *   mean, sd, min, max, q25, q75   mcx_samples_summary's numbers (its type-7 quantiles for probs 0.25 and 0.75), bit for bit
 *   bw         bw.nrd0: hi = sd, lo_ = min(hi, (q75 - q25) / 1.34), or hi where that is 0, or |min|, or 1;
 *              bw = adjust * 0.9 * lo_ * N^(-1/5).  A positive finite spec->bw[c] replaces it (adjust is not applied)
 *   from, to   min and max; with clip other than (0, 1) the type-7 quantiles of clip_lo and clip_hi, except that the last
 *              column, log L, keeps to = max (the exception of mcparam.clip.tails); finite spec->from[c] / to[c] override
 *   lo, up     from - 4 bw, to + 4 bw;  delta = (up - lo) / 511,  inv = 511 / (up - lo)
 *   binning    every value v: xpos = (double(v) - lo) * inv, ix = floor(xpos), w = floor((xpos - ix) * 2^24); for
 *              -1 <= ix <= 511 slot ix + 1 gets cnt += 1 and frac += w (both u64); every other value is dropped;
 *              nbinned = the sum of cnt over the slots 1 .. 512
 *   masses     y[k] = (cnt[k+1] - frac[k+1] / 2^24 + frac[k] / 2^24) / N for k < 512, 0 for 512 <= k < 1024
 *   kernel     K[m] = exp(-(k_m / bw)^2 / 2) / (bw sqrt(2 pi)), k_m = m delta for m <= 512, -(1024 - m) delta above
 *   d[j]       = max(0, sum over m of y[m] K[(m - j) mod 1024]), j < 512: a plain fp64 sum on the host
 *   x[j]       = from + j (to - from) / (n - 1), x[n-1] = to;  y[j] = the linear interpolation of (lo + k delta, d[k]) at x[j]
 * The sweep adds integers only: the same store and arguments give the same bytes.  A column holding an inf or NaN has
 * MCX_SUMMARY_NONFINITE, NaN in every double of its record and of its x and y, and nbinned = 0; every other column is what
 * it would be without that column. */
typedef struct mcx_density_spec {
  int n;                    /* output points per column, 2..512 */
  double adjust;            /* > 0; multiplies the nrd0 bandwidth */
  double clip_lo, clip_hi;  /* 0, 1 = the data's range; else 0 <= clip_lo < clip_hi <= 1 */
  const double *bw, *from, *to; /* NULL, or [ncol]; a NaN entry = the default of that column */
} mcx_density_spec;
typedef struct mcx_col_density {
  double bw, from, to, lo, up, mean, sd;
  long long nvalues, nbinned;
  int flags;                /* MCX_SUMMARY_* */
} mcx_col_density;
/* Steps [first_step, first_step + nsteps) of the store; cols[np + 1], x and y [np + 1][n].  MCX_ERR_INVALID in the cases
 * mcx_samples_summary refuses (but any nsteps >= 1 with nsteps * nc >= 2 will do), and for n outside 2..512, adjust <= 0 or
 * not finite, clip probabilities out of order, a given bw <= 0 or from > to: the spec is checked before a device is
 * touched.  A queued MCX_OPT_ASYNC_RUN run is finished first. */
int mcx_samples_density(mcx_engine *e, int first_step, int nsteps, const mcx_density_spec *spec, mcx_col_density *cols,
                        double *x, double *y);
/* the same for host rows in MCout layout (np + 1 columns, step-major then chain, nsteps * nc rows), and for a derived store */
int mcx_rows_density(const float *rows, int nsteps, int nc, int np, const mcx_density_spec *spec, mcx_col_density *cols,
                     double *x, double *y);
int mcx_store_density(mcx_store *s, const mcx_density_spec *spec, mcx_col_density *cols, double *x, double *y);
/* The two host steps of a density call for one column (no device): the record of column `col` (the index into the spec's
 * arrays) from its statistics -- qclip_* are read only with a clip pair --, nbinned left 0; and x[n], y[n] from the record
 * and the column's slots[513][2] = (cnt, frac).  The product path calls these very functions. */
int mcx_debug_density_grid(long long N, double mean, double sd, float min, float max, double q25, double q75,
                           double qclip_lo, double qclip_hi, int is_last_col, int col, const mcx_density_spec *spec,
                           mcx_col_density *out);
int mcx_debug_density_finish(const mcx_col_density *col, const unsigned long long *slots, int n, double *x, double *y);
/* the device sweep alone on given grids lo[np + 1] < up[np + 1]: slots[np + 1][513][2] */
int mcx_debug_rows_density_bins(const float *rows, int nsteps, int nc, int np, const double *lo, const double *up,
                                unsigned long long *slots);
/* one mcx_samples_density call, its results let go: ms[0] the statistics passes (wall clock), ms[1] the binning sweep
 * (HIP events), ms[2] the host grid and finish (wall clock), ms[3] the whole call (wall clock) */
int mcx_debug_density_times(mcx_engine *e, int first_step, int nsteps, const mcx_density_spec *spec, double *ms);
int mcx_debug_store_density_times(mcx_store *s, const mcx_density_spec *spec, double *ms); /* the same of a derived store */

/* ---- pair densities of the sample store, on the device --------------
 * The corner plot: per pair (a, b) of columns, a != b, the binned product-Gaussian kernel density estimate of MASS::kde2d
 * with bandwidth.nrd, which is what geom_density_2d evaluates, on the g x g nodes of the two columns' grids.  N = nsteps * nc
 * rows, 2 <= N < 2^31; 8 <= g <= 64; F = 4096.
 *   per column (the same in every pair the column is in)
 *   mean, sd, min, max, q25, q75, from, to   as in section 13 above (clip, log L's upper end, spec->from / to)
 *   bw         s = min(sd, (q75 - q25) / 1.34), or sd where that is 0, or |min|, or 1;  h = adjust * 1.06 * s * N^(-1/5)
 *              (bandwidth.nrd / 4, as kde2d divides it).  A positive finite spec->bw[c] replaces it (adjust is not applied)
 *   lo, up     from - 4 h, to + 4 h;  delta = (up - lo) / (g - 1),  inv = (g - 1) / (up - lo);  axis[c][j] = lo + j delta
 *   a value v  xpos = (double(v) - lo) * inv; on the grid iff -1 <= xpos < g (a NaN is not);
 *              s(v) = floor(xpos) + 1 in [0, g],  w(v) = floor((xpos - floor(xpos)) * F) in [0, F]
 *   per pair
 *   slots      a row whose two values are both on their grids adds to slot [s_a][s_b] of (g + 1) x (g + 1) slots the u64 sums
 *              cnt += 1, Sa += w_a, Sb += w_b, Sab += w_a w_b; every other row is dropped from this pair only;
 *              nbinned = the sum of cnt
 *   masses     num[j][k] = (F^2 cnt - F Sa - F Sb + Sab)[j+1][k+1] + (F Sa - Sab)[j][k+1] + (F Sb - Sab)[j+1][k] + Sab[j][k],
 *              an exact integer; mass[j][k] = double(num[j][k]) / (F^2 double(N)),  0 <= j, k < g
 *   kernel     K_c[i] = exp(-(i delta_c / h_c)^2 / 2) / (h_c sqrt(2 pi)), i < g
 *   z[j][k]    = sum over l of t[j][l] K_b[|l - k|],  t[j][l] = sum over m of mass[m][l] K_a[|m - j|], both ascending, plain
 *              fp64 sums on the host; z is the density at (axis[a][j], axis[b][k]).  For a > b the pair is summed as (b, a) and
 *              turned, so that z of (b, a) is the transpose of z of (a, b) bit for bit
 * The sweeps add integers only: the same store and arguments give the same bytes.  A pair with a column that holds an inf or
 * NaN has MCX_SUMMARY_NONFINITE, NaN in its z and nbinned = 0 (that column's record and axis are NaN, as in section 13); every
 * other pair is what it would be without that column. */
typedef struct mcx_density2d_spec {
  int g;                    /* grid nodes per axis, 8..64 */
  double adjust;            /* > 0; multiplies the bandwidth */
  double clip_lo, clip_hi;  /* 0, 1 = the data's range; else 0 <= clip_lo < clip_hi <= 1 */
  const double *bw, *from, *to; /* NULL, or [ncol]; a NaN entry = the default of that column */
  int npairs;               /* 1..1024; not read when pairs is NULL */
  const int *pairs;         /* [npairs][2] columns (a, b); NULL = every a < b in ascending order (at most 45 columns) */
} mcx_density2d_spec;
typedef struct mcx_pair_density {
  int a, b;
  long long nbinned;
  int flags;                /* MCX_SUMMARY_* */
} mcx_pair_density;
/* Steps [first_step, first_step + nsteps) of the store; cols[ncol] (mcx_col_density with nbinned left 0), axes[ncol][g],
 * pairs_out[npairs] and z[npairs][g][g], npairs = ncol (ncol - 1) / 2 when spec->pairs is NULL.  MCX_ERR_INVALID, before a
 * device is touched, in the cases mcx_samples_density refuses and for g outside 8..64, a == b, a column outside [0, ncol),
 * npairs outside 1..1024 (the default of more than 45 columns too: name the pairs); MCX_ERR_UNSUPPORTED for N >= 2^31;
 * MCX_ERR_ALLOC with the bytes needed in mcx_last_error when the scratch does not fit.  A queued MCX_OPT_ASYNC_RUN run is
 * finished first. */
int mcx_samples_density2d(mcx_engine *e, int first_step, int nsteps, const mcx_density2d_spec *spec, mcx_col_density *cols,
                          double *axes, mcx_pair_density *pairs_out, double *z);
/* the same for host rows in MCout layout, and for a derived store (a clip's mcx_rowset_store too) */
int mcx_rows_density2d(const float *rows, int nsteps, int nc, int np, const mcx_density2d_spec *spec, mcx_col_density *cols,
                       double *axes, mcx_pair_density *pairs_out, double *z);
int mcx_store_density2d(mcx_store *s, const mcx_density2d_spec *spec, mcx_col_density *cols, double *axes,
                        mcx_pair_density *pairs_out, double *z);
/* The two host steps (no device): the record of column `col` from its statistics, as mcx_debug_density_grid; and z[g][g] of
 * one pair from its two records and slots[(g + 1)^2][4] = (cnt, Sa, Sb, Sab), b_first != 0 for the sums of a > b.  The
 * product path calls these very functions. */
int mcx_debug_density2d_grid(long long N, double mean, double sd, float min, float max, double q25, double q75,
                             double qclip_lo, double qclip_hi, int is_last_col, int col, const mcx_density2d_spec *spec,
                             mcx_col_density *out);
int mcx_debug_density2d_finish(const mcx_col_density *ca, const mcx_col_density *cb, int g, const unsigned long long *slots,
                               int b_first, double *z);
/* the device sweeps alone on given grids lo[np + 1] < up[np + 1]: slots[npairs][(g + 1)^2][4]; pairs as in the spec */
int mcx_debug_rows_density2d_bins(const float *rows, int nsteps, int nc, int np, const double *lo, const double *up, int g,
                                  int npairs, const int *pairs, unsigned long long *slots);
/* one mcx_samples_density2d call, its results let go: ms[0] the statistics passes (wall clock), ms[1] k_density2d_codes,
 * ms[2] k_density2d_pairs, ms[3] k_density2d_reduce (HIP events), ms[4] the host grids and finish (wall clock), ms[5] the
 * whole call (wall clock) */
int mcx_debug_density2d_times(mcx_engine *e, int first_step, int nsteps, const mcx_density2d_spec *spec, double *ms);

/* ---- tail-clipped rows of the sample store, on the device -----------
 * The reference's mcparam.clip.tails (src/anly/mcpar-analysis.R:60-78): every row that lies in the tail of any column is
 * dropped, jointly, and the remaining rows are handed on.  The source is a step range of an engine's store, host rows in
 * MCout layout, or a derived store: N = nsteps * nc >= 1 rows of ncol columns (the parameters or derived columns, then
 * log L); row r is step r / nc, chain r % nc.
 *   thresholds  per column c doubles lo[c], hi[c]: by default mcx_samples_summary's type-7 quantiles of the column for the
 *               probabilities qlo and qhi, bit for bit.  The last column's upper threshold is ll_hi when that is not NaN
 *               (the reference: the literal 0.0, "its theoretical maximum"; +inf: no upper clip; NaN: the qhi quantile,
 *               like any other column).  A non-NaN spec->lo[c] / spec->hi[c] replaces the default of that column and side
 *               (+-inf: that side is not clipped), for the last column also ll_hi.  With both bounds of every column given
 *               no quantile pass runs and every flags is 0
 *   predicate   a row is kept iff for every column (double)v[c] > lo[c] && (double)v[c] < hi[c]: strict, as in R.  A NaN
 *               value or a NaN threshold fails both comparisons: a column whose default quantiles are NaN (a NaN among
 *               its values) drops every row unless both its bounds are given.  +-inf values compare as IEEE says
 *   row set     the K kept rows in source order, compacted on the device as x'[K][np], ly'[K], and with each its source
 *               row index r (int64, ascending).  K = 0 is a valid row set
 *   per column  nbelow[c] = the rows with !(v > lo[c]), nabove[c] = the rows with !(v < hi[c]), each counted whatever the
 *               row's other columns say (a NaN value counts in both); flags[c] = MCX_SUMMARY_NONFINITE from the quantile pass
 * Only integers are added and every kept row has one position: the same source and arguments give the same bytes. */
typedef struct mcx_clip_spec {
  double qlo, qhi;       /* 0 <= qlo < qhi <= 1 */
  double ll_hi;          /* upper threshold of log L; NaN = its qhi quantile; the reference: 0.0 */
  const double *lo, *hi; /* NULL, or [ncol]; a NaN entry = the default of that column and side */
} mcx_clip_spec;
typedef struct mcx_col_clip {
  double lo, hi;         /* the thresholds used */
  long long nbelow, nabove;
  int flags;             /* MCX_SUMMARY_* */
} mcx_col_clip;
/* A row set: it owns its device memory and a stream, and depends neither on the engine nor on the store it came from -- a
 * later mcx_run or mcx_destroy of that engine, or mcx_store_destroy of that store, leaves it intact.  One thread at a time
 * per row set. */
typedef struct mcx_rowset mcx_rowset;
/* Steps [first_step, first_step + nsteps) of the engine's store, nsteps >= 1; cols[np + 1], *nkept = K.  out == NULL: the
 * thresholds, the counts and K only, nothing is compacted or allocated.  MCX_ERR_INVALID for a NULL spec, cols or nkept
 * and for probabilities out of order or outside [0, 1] (checked before a device is touched), and in the cases
 * mcx_samples_summary refuses (the store does not hold the range); MCX_ERR_UNSUPPORTED for more rows than a grid of
 * workgroups covers (2^31 - 1 tiles of 32 to 256 rows).  A queued MCX_OPT_ASYNC_RUN run is finished first. */
int mcx_samples_clip(mcx_engine *e, int first_step, int nsteps, const mcx_clip_spec *spec, mcx_col_clip *cols, long long *nkept,
                     mcx_rowset **out);
/* the same for host rows in MCout layout (np + 1 columns, step-major then chain, nsteps * nc rows), and for a derived store */
int mcx_rows_clip(const float *rows, int nsteps, int nc, int np, const mcx_clip_spec *spec, mcx_col_clip *cols, long long *nkept,
                  mcx_rowset **out);
int mcx_store_clip(mcx_store *s, const mcx_clip_spec *spec, mcx_col_clip *cols, long long *nkept, mcx_rowset **out);
int mcx_rowset_destroy(mcx_rowset *r);
int mcx_rowset_shape(const mcx_rowset *r, long long *nrows, int *ncol, long long *nsource); /* K, ncol, N */
/* kept rows [first_row, first_row + nrows) in MCout layout, rows[nrows][ncol], and their source row indices */
int mcx_rowset_copy(mcx_rowset *r, long long first_row, long long nrows, float *rows);
int mcx_rowset_index(mcx_rowset *r, long long first_row, long long nrows, long long *index);
/* mcx_samples_draw's rule with N = K: draw i is kept row (r * K) >> 64, so this is mcparam.sample(mcparam.clip.tails(d)).
 * index[ndraw] (may be NULL): the position in the row set.  ndraw > 0 with K = 0 is MCX_ERR_INVALID. */
int mcx_rowset_draw(mcx_rowset *r, uint32_t seed, int64_t ndraw, float *rows, int64_t *index);
/* How the analyses of sections 9 to 13 reach the kept rows: they work on series of chains, and a flat row set has none.  So
 * the caller names a shape: kept rows [first_row, first_row + nsteps * nc) are copied, device to device, into a new store of
 * nsteps steps of nc pseudo-chains (the flat layouts are identical).  mean, sd, min, max, quantiles, covariance, density
 * and draws of that store are those of exactly these rows; its R-hat and ESS are of pseudo-chains and mean nothing.  The
 * caller chooses nc and leaves out at most nc - 1 rows, knowingly.  MCX_ERR_INVALID when the range is not inside the row
 * set or nsteps or nc < 1.  The store is the caller's (mcx_store_destroy) and outlives the row set. */
int mcx_rowset_store(mcx_rowset *r, long long first_row, int nsteps, int nc, mcx_store **out);
/* host only, no device: lo[ncol], hi[ncol] from q[ncol][2], the columns' (qlo, qhi) quantiles (NULL: all NaN), and the
 * spec by the rule above.  The product path calls this very function. */
int mcx_debug_clip_thresholds(int ncol, const double *q, const mcx_clip_spec *spec, double *lo, double *hi);
/* one mcx_samples_clip call with a row set, its results let go: ms[0] the thresholds (the quantile passes; wall clock),
 * ms[1] the mark sweep, ms[2] the scan, ms[3] the scatter sweep (HIP events), ms[4] the whole call (wall clock) */
int mcx_debug_clip_times(mcx_engine *e, int first_step, int nsteps, const mcx_clip_spec *spec, double *ms);

/* host only, no device: the launch geometry of the store analyses of sections 11, 12 and 14 for a store of nsteps steps of
 * nc chains of np parameters and a derive to nout outputs (nout = 0: none; the derive fields are then the clip's), N =
 * nsteps * nc rows.  Every field comes from the function or constant the launch code itself uses, so a test can assert
 * that its shape lies on the side of a size switch it is there for.  MCX_ERR_INVALID for np outside 1..256, nout outside
 * 0..256, nsteps or nc < 1, or g NULL. */
typedef struct mcx_store_geometry {
  long long nrows;              /* N */
  long long derive_rows;        /* rows per workgroup of the derive sweep: 256, 128, 64, 32 or 16 */
  long long derive_lds_bytes;   /* of its two tiles, at most 40 960 */
  long long derive_workgroups;
  long long clip_rows;          /* rows per workgroup of the clip's mark and scatter sweeps: 256 down to 32 */
  long long clip_mask_words;    /* 64-bit keep-mask words per workgroup, ceil(clip_rows / 64) */
  long long clip_lds_bytes;
  long long clip_workgroups;
  long long clip_scan_blocks;   /* blocks of 256 workgroup counts; the top level of the scan carries over steps of 256 blocks */
  long long rank_tiles;         /* sort tiles of 8192 keys per column; the scan of a (column, digit) row carries over steps of 256 */
  long long rank_step_chunk;    /* steps per workgroup of the key and transform sweeps */
  long long rank_grid_y;        /* their grid.y, ceil(nsteps / rank_step_chunk) */
  long long gather_chunk_rows;  /* rows of np + 1 floats that one chunk of a copy of N rows to the host holds */
} mcx_store_geometry;
int mcx_debug_store_geometry(int np, int nout, int nsteps, int nc, mcx_store_geometry *g);

/* Two test hooks for the rule that no store analysis depends on what its scratch held before the call (DESIGN.md "Scratch and
 * its history"; tests/test_gpu_scratch_history.py).
 * mcx_debug_fill_allocations: host only, touches no device.  byte = -1 (off, the default) or 0..255: while on, every device
 * allocation the library really makes (a buffer that is large enough is not allocated again) is filled with that byte before
 * the allocating call goes on.  *nfilled (may be NULL): the allocations filled under the setting this call ends.  Process-wide.
 * MCX_ERR_INVALID for any other byte; the setting then stays as it was.
 * mcx_debug_fill_scratch: exactly one of e and s is not NULL; the three scratch buffers the analyses of that engine or store
 * share (doubles, 64-bit words, 32-bit words) are filled with byte = 0..255 up to their present capacity, on the owner's stream,
 * and the call waits for it.  bytes (may be NULL): the bytes filled per buffer, 0 for one that no analysis has allocated yet.
 * MCX_ERR_INVALID, before any device is touched, for both or neither of e and s or a byte outside 0..255. */
int mcx_debug_fill_allocations(int byte, unsigned long long *nfilled);
int mcx_debug_fill_scratch(mcx_engine *e, mcx_store *s, int byte, size_t bytes[3]);

/* ---- the per-chain table of the sample store, and stores of chosen chains, on the device ----
 * The one analysis whose unit is the chain: what every chain of a step range did, a rule that names the chains to drop, and a
 * store of the chains that stay, for every analysis above.  The source is a step range of an engine's store, host rows in
 * MCout layout, or a derived store: T = nsteps >= 1 steps of nc chains (indices local to the shard) and ncol = np + 1 columns
 * (the parameters or derived columns, then log L).
 *   per (chain, column) series x_0 .. x_{T-1}, fp64 throughout, centred (two passes):
 *     mean       = the sum over the steps / T
 *     sd         = sqrt(sum c_i^2 / (T - 1)), c_i = x_i - mean; NaN at T = 1
 *     rho1       = sum_{i < T-1} c_i c_{i+1} / sum_i c_i^2, the lag-1 autocorrelation; NaN when T < 2 or the series is constant
 *     a series holding an inf or NaN has NaN in all three
 *   per chain:
 *     moves         the steps t in [1, T) whose row differs from step t - 1's in the bits of any of its ncol floats (-0 and +0
 *                   differ, one NaN pattern equals itself, a change in log L alone is a move)
 *     longest_stay  the steps of the longest run of bit-identical consecutive rows: 1 when no row repeats, T when none moved
 *     ll_max, ll_max_step   the largest log L in float order (-inf < finite < +inf, -0 before +0) and the first step of the
 *                   range, counted from 0, that holds it; NaN and -1 when the chain's log L holds a NaN
 *     flags         MCX_SUMMARY_NONFINITE when any series of the chain holds an inf or NaN
 * Every number has one writer and a fixed order of operations: the same source and arguments give the same bytes. */
typedef struct mcx_chain_col { double mean, sd, rho1; } mcx_chain_col;
typedef struct mcx_chain_row {
  long long moves, longest_stay;
  float ll_max;
  int ll_max_step;
  int flags;            /* MCX_SUMMARY_* */
} mcx_chain_row;
/* Steps [first_step, first_step + nsteps) of the engine's store, nsteps >= 1; cols[nc][np + 1], chains[nc].  MCX_ERR_INVALID
 * for a NULL cols or chains (checked before a device is touched) and in the cases mcx_samples_summary refuses (the store
 * does not hold the range).  A queued MCX_OPT_ASYNC_RUN run is finished first. */
int mcx_samples_chain_table(mcx_engine *e, int first_step, int nsteps, mcx_chain_col *cols, mcx_chain_row *chains);
/* the same for host rows in MCout layout (np + 1 columns, step-major then chain, nsteps * nc rows), and for a derived store */
int mcx_rows_chain_table(const float *rows, int nsteps, int nc, int np, mcx_chain_col *cols, mcx_chain_row *chains);
int mcx_store_chain_table(mcx_store *s, mcx_chain_col *cols, mcx_chain_row *chains);

/* host only, no device: which chains of a table to keep.  Per column that takes part, over the chains whose mean of that
 * column is finite: med = the median of the chain means (the mean of the two middle values of an even count), mad = the
 * median of |mean - med|, scale = 1.4826 mad.
 *   MCX_CHAIN_NONFINITE  flags has MCX_SUMMARY_NONFINITE (or a mean of the chain is not finite); such a chain gets this alone
 *   MCX_CHAIN_STUCK      moves < min_moves, or max_stay > 0 and longest_stay > max_stay
 *   MCX_CHAIN_OUTLIER    |mean - med| > z scale in a column that takes part: strict, so scale = 0 names exactly the chains
 *                        whose mean differs from med; z = +inf: no outlier test
 * reasons[nc], 0 = kept; centre[ncol][2] = (med, scale), NaN for a column that takes no part (may be NULL); *nkept = the
 * chains kept.  MCX_ERR_INVALID for nc or ncol < 1, a NULL cols, chains, rule, reasons or nkept, and z <= 0 or NaN.  The
 * product path (mcpar-run --chain-keep, the Python binding's keep_chains) calls this very function. */
enum { MCX_CHAIN_NONFINITE = 1, MCX_CHAIN_STUCK = 2, MCX_CHAIN_OUTLIER = 4 };
typedef struct mcx_chain_rule {
  double z;                      /* > 0 and finite, or +inf: no outlier test */
  long long min_moves, max_stay; /* STUCK when moves < min_moves, or max_stay > 0 && longest_stay > max_stay */
  const unsigned char *use_col;  /* NULL = every column; else [ncol], non-zero = the column takes part in the outlier test */
} mcx_chain_rule;
int mcx_chains_keep(int nc, int ncol, const mcx_chain_col *cols, const mcx_chain_row *chains, const mcx_chain_rule *rule,
                    int *reasons, double *centre, int *nkept);

/* A store of chosen chains: out[t][k][:] = in[t][chains[k]][:] for the T steps of the range, log L likewise -- nsel >= 1
 * chains in any order and with repeats (chains resampled with replacement are the bootstrap of an ensemble), nsel may exceed
 * nc.  The result is an ordinary mcx_store of T steps of nsel chains and the same columns: it owns its memory and a stream,
 * outlives its source, and every analysis above works on it.  These are real chains: its R-hat and ESS mean what they say.
 * MCX_ERR_INVALID, before a device is touched and with nothing allocated, for a NULL chains or out, nsel < 1 and an index
 * outside [0, nc), the entry named in mcx_last_error; MCX_ERR_UNSUPPORTED for more elements than one grid copies (2^31 - 1
 * workgroups of 256 quads or floats).  The same source and arguments give the same bytes. */
int mcx_samples_select_chains(mcx_engine *e, int first_step, int nsteps, const int *chains, int nsel, mcx_store **out);
int mcx_rows_select_chains(const float *rows, int nsteps, int nc, int np, const int *chains, int nsel, mcx_store **out);
int mcx_store_select_chains(mcx_store *s, const int *chains, int nsel, mcx_store **out);

/* host only, no device: the launch geometry of the three sweeps of this section for a store of nsteps steps of nc chains of np
 * parameters and a selection of nsel chains, every field from the function the launch code itself uses.  MCX_ERR_INVALID for
 * np outside 1..256, nsteps, nc or nsel < 1, or g NULL. */
typedef struct mcx_chains_geometry {
  long long block;                 /* threads per workgroup of the three sweeps: 256 */
  long long lds_bytes;             /* of each: 0, every sweep works in registers */
  long long series_tile_cols;      /* series sweep: adjacent parameter columns per tile, min(np, 16) */
  long long series_tile_chains;    /* chains per tile, 256 / series_tile_cols */
  long long series_col_tiles;      /* ceil(np / series_tile_cols) */
  long long series_workgroups;     /* of the parameter columns: series_col_tiles * ceil(nc / series_tile_chains) */
  long long series_ll_workgroups;  /* of log L, one lane per chain: ceil(nc / 256) */
  long long rows_lanes_per_chain;  /* row sweep: min(64, the power of two >= np + 1) */
  long long rows_values_per_lane;  /* ceil((np + 1) / rows_lanes_per_chain): 1 to 5 */
  long long rows_chains_per_workgroup; /* 256 / rows_lanes_per_chain */
  long long rows_workgroups;
  long long select_vec4;           /* the gather's path when its bases are 16-byte aligned: 1 = 16 bytes per lane (np % 4 == 0), 0 = 4 */
  long long select_items;          /* one per lane: the quads or floats of x', then the nsteps * nsel values of log L */
  long long select_workgroups;
} mcx_chains_geometry;
int mcx_debug_chains_geometry(int np, int nsteps, int nc, int nsel, mcx_chains_geometry *g);
/* one mcx_samples_chain_table call, its results let go: ms[0] the series sweep, ms[1] the row sweep (HIP events), ms[2] the
 * whole call (wall clock) */
int mcx_debug_chain_table_times(mcx_engine *e, int first_step, int nsteps, double *ms);

/* ---- the per-step table of the sample store on the device, and where the ensemble settled ----
 * The one analysis whose unit is the step: what the ensemble of nc chains looked like at every kept step, and a rule that
 * names the step from which it no longer drifts.  The source is a step range of an engine's store, host rows in MCout layout,
 * or a derived store (of mcx_*_derive, mcx_rowset_store or mcx_*_select_chains): T = nsteps >= 1 steps of nc >= 1 chains
 * (indices local to the shard) and ncol = np + 1 columns (the parameters or derived columns, then log L).
 *   per (step t, column c), over the nc values x_0 .. x_{nc-1} of that step: cols[t * ncol + c]
 *     mean       = the sum over the chains / nc, fp64
 *     sd         = sqrt(sum (x_i - mean)^2 / (nc - 1)), fp64, centred (a second pass); NaN at nc = 1
 *     min, max   exact, in float order (-inf < finite < +inf; -0 before +0)
 *     quantiles  q[(t * ncol + c) * nprobs + k], R type 7 / numpy "linear" from exact order statistics with N = nc:
 *                h = (nc - 1) p_k, lo = floor(h), g = h - lo; x(lo) when g = 0 or x(lo) = x(lo+1), else
 *                x(lo) + g (x(lo+1) - x(lo)), fp64
 *     a NaN among the nc values makes min, max and every quantile NaN (a NaN, payload unspecified); an inf or NaN among them
 *     (the fp64 sum is not finite) sets flags = MCX_SUMMARY_NONFINITE and makes mean and sd NaN
 *   per step t: steps[t]
 *     moved         the chains whose row at step t differs from their row at step t - 1 in the bits of any of its ncol floats
 *                   (-0 and +0 differ, one NaN pattern equals itself, a change in log L alone counts): the realised acceptance
 *                   count of the step; -1 for the first step of the range
 *     ll_max, ll_max_chain   the largest log L of the step in float order and the lowest chain index that holds it; NaN and
 *                   -1 when the step's log L holds a NaN
 *     flags         MCX_SUMMARY_NONFINITE when any column of the step has it
 * No float atomics; every float sum is a fixed slot and a fixed-order tree; counts are integers: the same source and
 * arguments give the same bytes. */
enum { MCX_STEP_MAX_PROBS = 8 };
typedef struct mcx_step_col {
  double mean, sd;
  float min, max;
  int flags;            /* MCX_SUMMARY_* */
  int reserved;         /* 0 */
} mcx_step_col;
typedef struct mcx_step_row {
  int moved;            /* -1 for the first step of the range */
  float ll_max;
  int ll_max_chain;
  int flags;            /* MCX_SUMMARY_* */
} mcx_step_row;
/* Steps [first_step, first_step + nsteps) of the engine's store, nsteps >= 1.  cols[nsteps * (np + 1)], steps[nsteps],
 * quantiles[nsteps * (np + 1) * nprobs] (may be NULL only when nprobs == 0); probs[nprobs] in [0, 1], 0 <= nprobs <=
 * MCX_STEP_MAX_PROBS.  MCX_ERR_INVALID, before a device is touched and with nothing allocated, for a NULL cols or steps, a
 * NULL probs or quantiles with nprobs > 0, nsteps < 1, nprobs outside [0, 8] and a p that is NaN or outside [0, 1], the entry
 * named in mcx_last_error; and in the cases mcx_samples_summary refuses (the store does not hold the range).
 * MCX_ERR_UNSUPPORTED for more (step, column tile) pairs than one grid holds (2^31 - 1).  A queued MCX_OPT_ASYNC_RUN run is
 * finished first. */
int mcx_samples_step_table(mcx_engine *e, int first_step, int nsteps, const double *probs, int nprobs, mcx_step_col *cols,
                           mcx_step_row *steps, double *quantiles);
/* the same for host rows in MCout layout (np + 1 columns, step-major then chain, nsteps * nc rows), and for a derived store */
int mcx_rows_step_table(const float *rows, int nsteps, int nc, int np, const double *probs, int nprobs, mcx_step_col *cols,
                        mcx_step_row *steps, double *quantiles);
int mcx_store_step_table(mcx_store *s, const double *probs, int nprobs, mcx_step_col *cols, mcx_step_row *steps, double *quantiles);

/* host only, no device: from which step on the ensemble of a step table no longer drifts.  The reference window is the last
 * R = max(1, ceil(ref_frac T)) steps of the T = nsteps of the table.  Per column that takes part, fp64, summed in step order:
 *   m_ref = the mean of the window's step means; s_ref = sqrt(the mean of the window's sd^2)
 * Step t is in band when, for every column that takes part, |mean_t - m_ref| <= tol_mean s_ref and |sd_t - s_ref| <= tol_sd
 * s_ref; a step with a non-finite mean or sd in such a column is out of band.
 *   out_cols[ncol]: m_ref, s_ref; last_out = the last step out of band in that column alone, -1 if none; max_dev_mean =
 *     max_t |mean_t - m_ref| / s_ref and max_dev_sd = max_t |sd_t - s_ref| / s_ref over the steps whose mean and sd are
 *     finite, NaN when s_ref is 0 or not finite; a column that takes no part has NaN in the four doubles and last_out = -1
 *   *settled_step = 1 + the last out-of-band step; 0 when every step is in band; -1, not settled, when that step lies inside
 *     the reference window (1 + it > T - R), or when a column that takes part has s_ref = 0 or not finite -- a table of one
 *     chain, whose every sd is NaN, is such a table
 * MCX_ERR_INVALID for nsteps or ncol < 1, a NULL cols, rule, out_cols or settled_step, a tol_mean or tol_sd that is negative
 * or NaN, a ref_frac outside (0, 1] or NaN, and a use_col that names no column.  The product path (mcpar-run --settle, the
 * Python binding's settle_steps) calls this very function. */
typedef struct mcx_step_rule {
  double tol_mean, tol_sd;       /* in units of s_ref; the defaults of the driver and the binding: 0.1, 0.1 */
  double ref_frac;               /* the share of the steps, from the end, that make the reference window; default 0.5 */
  const unsigned char *use_col;  /* NULL = every column; else [ncol], non-zero = the column takes part */
} mcx_step_rule;
typedef struct mcx_step_settle_col {
  double m_ref, s_ref, max_dev_mean, max_dev_sd;
  int last_out;
  int reserved;                  /* 0 */
} mcx_step_settle_col;
int mcx_steps_settle(int nsteps, int ncol, const mcx_step_col *cols, const mcx_step_rule *rule, mcx_step_settle_col *out_cols,
                     int *settled_step);

/* host only, no device: the launch geometry of the three sweeps of this section for a table of nsteps steps of nc chains of np
 * parameters and nprobs probabilities, every field from the function the launch code itself uses.  MCX_ERR_INVALID for np
 * outside 1..256, nsteps or nc < 1, nprobs outside [0, 8], or g NULL. */
typedef struct mcx_steptable_geometry {
  long long block;                  /* threads per workgroup of the three sweeps: 256 */
  long long moments_tile_cols;      /* moments sweep: adjacent parameter columns per tile, min(np, 16) */
  long long moments_stride_chains;  /* chains one stride of such a tile covers, 256 / moments_tile_cols (log L: 256) */
  long long moments_col_tiles;      /* ceil(np / moments_tile_cols), and one more tile for log L */
  long long moments_workgroups;     /* nsteps * (moments_col_tiles + 1) */
  long long moments_lds_bytes;
  long long select_slots;           /* histograms per column: the target ranks, 2 nprobs */
  long long select_tile_cols;       /* select sweep: min(np, 16, 63 / select_slots); 0 when nprobs = 0 (no launch) */
  long long select_stride_chains;   /* 256 / select_tile_cols */
  long long select_col_tiles;       /* ceil(np / select_tile_cols), and one more tile for log L */
  long long select_workgroups;      /* nsteps * (select_col_tiles + 1); 0 when nprobs = 0 */
  long long select_lds_bytes;       /* select_tile_cols * select_slots KiB of bins and 1 KiB of state: at most 64 KiB */
  long long rows_lanes_per_chain;   /* row sweep: section 16's grouping, min(64, the power of two >= np + 1) */
  long long rows_values_per_lane;   /* ceil((np + 1) / rows_lanes_per_chain): 1 to 5 */
  long long rows_chains_per_pass;   /* 256 / rows_lanes_per_chain */
  long long rows_chunks;            /* workgroups per step: min(32, ceil(nc / rows_chains_per_pass)) */
  long long rows_workgroups;        /* nsteps * rows_chunks */
  long long scratch_doubles;        /* nsteps * (np + 1) * (4 + nprobs) */
  long long scratch_words;          /* nsteps * 2 * (rows_chunks + 1) */
} mcx_steptable_geometry;
int mcx_debug_steptable_geometry(int np, int nsteps, int nc, int nprobs, mcx_steptable_geometry *g);
/* one mcx_samples_step_table call, its results let go: ms[0] the moments sweep, ms[1] the select sweep, ms[2] the row sweep and
 * its reducer (HIP events), ms[3] the whole call (wall clock) */
int mcx_debug_step_table_times(mcx_engine *e, int first_step, int nsteps, const double *probs, int nprobs, double *ms);

/* ---- sample text read back, on the device ---------------------------
 * The reference's read.mc.data (src/anly/mcpar-analysis.R: read.table(filename)) for the text MCout::output prints
 * (src/mcout.cc:41-45), which mcx_samples_text, mcx_format_rows and the reference's own drivers write: lines of ncol numbers.
 *   token      a maximal run of bytes other than blank, tab, \r and \n:
 *              [+-]? ( D+ ( . D* )? | . D+ ) ( [eE] [+-]? D+ )?,  or  [+-]? inf | infinity | nan  in any letter case.
 *              Nothing else is a number: hex floats, NA, 1e, nan(...) are refused.
 *   value      the bits of glibc's strtof in the "C" locale: correctly rounded, ties to even, +-inf above the range, +-0
 *              below 2^-150, denormals between, -0 kept; a nan token gives a NaN of unspecified sign and payload.  Converted on
 *              the device, in integer arithmetic, for every token of at most 40 bytes and 19 digits from its first non-zero
 *              one on; any other token of the grammar is converted by strtof on the host and counted in nfallback.
 *   lines      end with \n (\r\n is accepted; the last line needs none); a line of separators only is skipped and not
 *              counted as a row; every other line must hold exactly ncol tokens.
 *   rows       row r of the text is (step r / nc, chain r % nc): the order of mcx_samples_text.  The result is an ordinary
 *              mcx_store of ncol - 1 columns, then the last column as log L, T = nrows / nc: every mcx_store_* and
 *              mcx_rowset_* entry point works on it.
 *   pieces     the text goes to the device in pieces of at most piece_bytes bytes, each cut behind the last line end that
 *              fits (the rest of the text, if it fits, is the last piece); the result does not depend on piece_bytes.
 * MCX_ERR_INVALID, nothing left allocated and *out NULL: a NULL argument; ncol outside 2..257; nc < 1; a line with another
 * number of tokens ("line L: K fields, expected ncol": L counts from 1 in the whole text, skipped and empty lines included; of
 * several wrong lines the first is named, and its field count before its tokens); a token outside the grammar ("line L, field
 * F"); no rows, or a number of rows that is no multiple of nc; a line longer than a piece.  MCX_ERR_ALLOC, with the bytes
 * needed in mcx_last_error: the store (4 bytes per number, for as many rows as the text has lines) and three piece_bytes of
 * text and token offsets do not fit.  The same text and arguments give the same bytes. */
#define MCX_TEXT_FALLBACK_CAPACITY 1024 /* tokens of one piece the device hands to the host one by one; a piece with more of them
                                           is tokenised on the host (same result, same nfallback) */
typedef struct mcx_text_spec {
  int ncol;            /* columns per line; 0: the token count of the first kept line that has any */
  int nc;              /* chains: rows must be a multiple; step-major then chain, the order of mcx_samples_text */
  int64_t skip_lines;  /* leading lines ignored, whatever they hold (read.table's skip): "nsamp = ..." of the reference's drivers */
  int64_t max_rows;    /* < 0: to the end; else stop after that many rows (read.table's nrows): trailing "max likelihood" lines */
  size_t piece_bytes;  /* 0: default (32 MiB); 64 to 2^30; must hold the longest line with its line end */
} mcx_text_spec;
typedef struct mcx_text_report {
  int64_t nrows;       /* rows stored */
  int64_t nlines;      /* lines read, the skipped and the empty ones included (with max_rows: to the end of the last piece read) */
  int64_t ntokens;     /* nrows * ncol */
  int64_t nfallback;   /* tokens converted by strtof on the host */
  int64_t npieces;
  int ncol;
} mcx_text_report;
int mcx_text_store(const char *text, size_t nbytes, const mcx_text_spec *spec, mcx_store **out, mcx_text_report *rep);
/* the rows on the host, MCout layout rows[nrows][ncol]; MCX_ERR_INVALID when capacity_rows < nrows.  rows == NULL: the report only */
int mcx_text_rows(const char *text, size_t nbytes, const mcx_text_spec *spec, float *rows, int64_t capacity_rows,
                  mcx_text_report *rep);
/* the same of a file, read in pieces (once to count its lines, once to parse): the file need not fit host memory */
int mcx_file_store(const char *path, const mcx_text_spec *spec, mcx_store **out, mcx_text_report *rep);
/* host only, no device: one token through parse_g.hpp as compiled into the library.  *status = 0 converted, 1 not a number,
 * 2 of the grammar but left to the host: *bits is then strtof's, as in the store */
int mcx_debug_parse_token(const char *tok, size_t len, uint32_t *bits, int *status);
/* mcx_text_store with its stages timed, for tools/parse_bench.py; the store is let go.  ms[8]: the upload, the mark sweep, the
 * scan, the scatter of the token starts, the parse sweep (HIP events, summed over the pieces), the host's line count, its
 * staging of the pieces in pinned memory, the whole call (wall clock) */
int mcx_debug_text_times(const char *text, size_t nbytes, const mcx_text_spec *spec, mcx_text_report *rep, double *ms);

/* ---- two sample stores compared, on the device ----------------------
 * Do stores A and B sample the same distribution?  Per column (the parameters, then log L; both stores have the same number of
 * columns, any nc and nsteps on either side): na = nsteps_a * nc_a and nb = nsteps_b * nc_b values, each in [1, 2^31).
 * Values are ordered by the key of the rank summary: -0 and +0 are one point, -inf and +inf ordinary end points, every NaN
 * one point that sorts last.  cA(x), cB(x) = the number of values <= x in that order.
 *   ks_plus_num   = max over the distinct values x of A of cA(x) nb - cB(x) na   (int64, >= 0, < 2^62)
 *   ks_minus_num  = max over the distinct values x of B of cB(x) na - cA(x) nb
 *   ks_plus_x, ks_minus_x   the smallest x that attains each maximum
 *   ks            = (double)max(ks_plus_num, ks_minus_num) / ((double)na * (double)nb): the two-sample Kolmogorov-Smirnov
 *                   distance, exact in integers up to that one division
 *   w1            = the Wasserstein-1 distance, the area between the two ECDFs in the column's units: over the pooled distinct
 *                   values x_0 < ... < x_m, sum_{k<m} |cA(x_k) nb - cB(x_k) na| (x_{k+1} - x_k) / (na nb), fp64, fixed order
 *   mean_*, sd_*, ess_*   mcx_samples_summary's numbers of each side when that side has nsteps >= 4 and MCX_COMPARE_IID is
 *                   not set; else ess = n, mean and sd (divisor n - 1; NaN for n = 1) as the summary gives them
 *   z_mean        = (mean_a - mean_b) / sqrt(sd_a^2 / ess_a + sd_b^2 / ess_b)
 *   ks_neff, ks_p mcx_ks_prob(ks, ess_a, ess_b): not an exact test -- the asymptotic Kolmogorov law with the ESS in the place
 *                   of the sample sizes
 * A side whose fp64 column sum is not finite has MCX_COMPARE_NONFINITE_A / _B: the KS fields stay (the order defines them);
 * w1, mean_*, sd_*, ess_*, z_mean, ks_neff and ks_p of that column are NaN.  The same stores and arguments give the same
 * bytes; the same store on both sides gives zeros and ks_p = 1.  MCX_ERR_INVALID before anything is allocated: a NULL store,
 * rows or cols, unknown flags, different column counts, the two stores on different devices; MCX_ERR_UNSUPPORTED: 2^31 or more
 * values on a side.  spec == NULL: flags = 0.  The call runs on A's stream with A's scratch after B's stream is idle. */
enum { MCX_COMPARE_IID = 1 };                                   /* mcx_compare_spec.flags: treat every value as an independent draw */
enum { MCX_COMPARE_NONFINITE_A = 1, MCX_COMPARE_NONFINITE_B = 2 }; /* mcx_col_compare.flags */
typedef struct mcx_compare_spec {
  int flags;
} mcx_compare_spec;
typedef struct mcx_col_compare {
  long long ks_plus_num, ks_minus_num;
  double ks_plus_x, ks_minus_x;
  double ks, w1;
  double mean_a, sd_a, ess_a;
  double mean_b, sd_b, ess_b;
  double z_mean, ks_neff, ks_p;
  long long na, nb;
  int flags, reserved;
} mcx_col_compare;
/* cols[ncol] */
int mcx_store_compare(mcx_store *a, mcx_store *b, const mcx_compare_spec *spec, mcx_col_compare *cols);
/* host rows in MCout layout on both sides (np + 1 columns) */
int mcx_rows_compare(const float *rows_a, int nsteps_a, int nc_a, const float *rows_b, int nsteps_b, int nc_b, int np,
                     const mcx_compare_spec *spec, mcx_col_compare *cols);
/* two step ranges of one engine's store (they may overlap), and a range against a store.  MCX_ERR_INVALID in the cases
 * mcx_samples_summary refuses; a queued MCX_OPT_ASYNC_RUN run is finished first */
int mcx_samples_compare(mcx_engine *e, int first_a, int nsteps_a, int first_b, int nsteps_b, const mcx_compare_spec *spec,
                        mcx_col_compare *cols);
int mcx_samples_compare_store(mcx_engine *e, int first_step, int nsteps, mcx_store *b, const mcx_compare_spec *spec,
                              mcx_col_compare *cols);
/* host only: *neff = ess_a ess_b / (ess_a + ess_b), *p = Q((sqrt(neff) + 0.12 + 0.11 / sqrt(neff)) ks), Q the survival
 * function of Kolmogorov's distribution.  MCX_ERR_INVALID: ks outside [0, 1], an ess <= 0, a NULL output; NaN in, NaN out */
int mcx_ks_prob(double ks, double ess_a, double ess_b, double *neff, double *p);
/* host only: the launch geometry of a comparison of na against nb values per column of ncol columns */
typedef struct mcx_compare_geometry {
  long long block, tile_keys;        /* threads per workgroup; keys per sort and sweep tile */
  long long tiles_a, tiles_b;        /* sweep tiles per column of each side */
  long long window_lds_keys;         /* a tile whose window of the other side has at most this many keys searches it in LDS */
  long long lds_bytes;               /* of a sweep workgroup */
  long long group_cols;              /* columns sorted and swept at a time before any halving for memory (MCX_COMPARE_GROUP_COLS caps it) */
  long long scratch_bytes_per_col;   /* per-call scratch of one column of a group */
  long long sort_tiles_a, sort_tiles_b;               /* sort tiles per column of each side: above 256 the scans of the sort carry */
  long long bounds_workgroups_a, bounds_workgroups_b; /* grid.x of k_cmp_bounds, a lane per tile: ceil(tiles / block) */
  long long step_chunk_a, step_chunk_b;               /* steps per workgroup of k_cmp_keys: max(64, ceil(nsteps / 32768)) */
  long long grid_y_a, grid_y_b;                       /* and its grid.y; these four are 0 from the entry that is given na and nb alone */
} mcx_compare_geometry;
int mcx_debug_compare_geometry(long long na, long long nb, int ncol, mcx_compare_geometry *g);
/* the same for na = nsteps_a * nc_a against nb = nsteps_b * nc_b values, with the step chunks of the key sweeps */
int mcx_debug_compare_store_geometry(int nsteps_a, int nc_a, int nsteps_b, int nc_b, int ncol, mcx_compare_geometry *g);
/* one mcx_samples_compare call, its results let go, ms[10] by HIP events: 0 the two sides' summaries, 1 A's keys, 2 A's sort,
 * 3 B's keys, 4 B's sort, 5 the bounds, 6 the sweep with self = A, 7 with self = B, 8 the reducer, 9 the whole call */
int mcx_debug_compare_times(mcx_engine *e, int first_a, int nsteps_a, int first_b, int nsteps_b, const mcx_compare_spec *spec,
                            double *ms);

/* ---- two sample stores compared jointly, on the device -------------
 * The energy distance (Szekely & Rizzo) between rows of stores A and B as points in column space, with a permutation test.
 * Both stores have the same columns and any nc and nsteps; NA = nsteps_a * nc_a and NB rows in MCout order.  The columns
 * used are the parameters (a derived store's outputs); MCX_ENERGY_WITH_LL adds the last column.
 *   rows of a side  spec.n_a (n_b) > 0: that many draws with replacement by section 12's rule -- draw i of A is draw i of
 *                   mcx_debug_draw_indices(seed, NA, ...), draw i of B is draw n_a + i of (seed, NB); 0: min(rows, 2048)
 *                   draws; -1: every row of the side in store order.  2 <= n <= MCX_ENERGY_MAX_SIDE a side, 0 <= nperm <= 4095
 *   scale[c]        the standard deviation of column c over the N = n_a + n_b pooled rows (A's, then B's): fp64, centred
 *                   two-pass, divisor N - 1.  A used column with a value that is not finite has MCX_ENERGY_COL_NONFINITE, one
 *                   with scale 0 MCX_ENERGY_COL_CONSTANT: both are left out of the distance.  MCX_ENERGY_RAW: scale = 1, only
 *                   the first rule applies.  The last column without MCX_ENERGY_WITH_LL: MCX_ENERGY_COL_UNUSED, scale NaN
 *   d_ij            sqrt(sum_c (z_ic - z_jc)^2), z_ic = (double)x_ic / scale[c], every difference formed directly, fp64
 *   sums            for a label vector l in {0,1}^N with n_a ones: S = sum_ij d_ij, S_A = sum_i l_i sum_j d_ij,
 *                   S_AA = sum_ij l_i l_j d_ij (ordered pairs); S_AB = S_A - S_AA, S_BB = S - 2 S_A + S_AA,
 *                   E(l) = 2 S_AB / (n_a n_b) - S_AA / n_a^2 - S_BB / n_b^2
 *   e, mean_*, h    E and the three normalised sums of l_0 = the first n_a rows; h = e / (2 mean_ab) (NaN at mean_ab = 0)
 *   perm_e[p - 1]   E(l_p), p = 1 ... nperm: l_p is mcx_debug_energy_labels' vector (Philox stream 6)
 *   nge, p_value    #{p : perm_e >= e} and (1 + nge) / (1 + nperm) (NaN at nperm = 0)
 * If no column is left every statistic is NaN, nused = 0 and the call returns MCX_OK.  The permutation law is exact for
 * exchangeable rows; the rows of a store are autocorrelated, so draw far fewer rows than the smallest column ESS that
 * mcx_*_compare reports, or read the p-value as anticonservative (the result carries n_a, n_b, na_rows, nb_rows to judge by).
 * The same stores and arguments give the same bytes.  MCX_ERR_INVALID before anything is allocated: a NULL store, rows or
 * res, unknown flags, different column counts, stores on different devices, sizes outside the limits.  cols[ncol] and
 * perm_e[nperm] may be NULL; spec == NULL is {0, 0, 999, 0, 0}.  While it makes the label vectors a call runs up to 15 threads of
 * its own beside the caller's (at most one per block of 16 label vectors and per hardware thread), all joined before it returns. */
enum { MCX_ENERGY_WITH_LL = 1, MCX_ENERGY_RAW = 2 };                                         /* mcx_energy_spec.flags */
enum { MCX_ENERGY_COL_NONFINITE = 1, MCX_ENERGY_COL_CONSTANT = 2, MCX_ENERGY_COL_UNUSED = 4 }; /* mcx_energy_col.flags */
enum { MCX_ENERGY_MAX_SIDE = 16384, MCX_ENERGY_MAX_PERM = 4095 };
typedef struct mcx_energy_spec {
  int n_a, n_b, nperm;
  uint32_t seed;
  unsigned flags;
} mcx_energy_spec;
typedef struct mcx_energy_result {
  double e, h, mean_ab, mean_aa, mean_bb, p_value;
  long long nge;
  int n_a, n_b, nperm, nused;
  long long na_rows, nb_rows;
} mcx_energy_result;
typedef struct mcx_energy_col {
  double scale;
  int flags;
} mcx_energy_col;
int mcx_store_energy(mcx_store *a, mcx_store *b, const mcx_energy_spec *spec, mcx_energy_result *res, mcx_energy_col *cols,
                     double *perm_e);
/* host rows in MCout layout on both sides (np + 1 columns) */
int mcx_rows_energy(const float *rows_a, int nsteps_a, int nc_a, const float *rows_b, int nsteps_b, int nc_b, int np,
                    const mcx_energy_spec *spec, mcx_energy_result *res, mcx_energy_col *cols, double *perm_e);
/* two step ranges of one engine's store (they may overlap), and a range against a store.  MCX_ERR_INVALID in the cases
 * mcx_samples_compare refuses; a queued MCX_OPT_ASYNC_RUN run is finished first */
int mcx_samples_energy(mcx_engine *e, int first_a, int nsteps_a, int first_b, int nsteps_b, const mcx_energy_spec *spec,
                       mcx_energy_result *res, mcx_energy_col *cols, double *perm_e);
int mcx_samples_energy_store(mcx_engine *e, int first_step, int nsteps, mcx_store *b, const mcx_energy_spec *spec,
                             mcx_energy_result *res, mcx_energy_col *cols, double *perm_e);
/* host only: labels[n_a + n_b] of permutation p (0: the first n_a rows; 1 ... MCX_ENERGY_MAX_PERM: a partial Fisher-Yates on
 * idx = [0, N) -- for i < n_a, w = philox4x32_10(counter (i, p, 0, 0), key (seed, 6)), r = w.x : w.y, j = i + ((r (N - i)) >> 64),
 * swap idx[i] and idx[j], labels[idx[i]] = 1) */
int mcx_debug_energy_labels(uint32_t seed, int n_a, int n_b, int p, uint8_t *labels);
/* mcx_rows_energy's device sums: sums[0] = S, then (S_A, S_AA) of l_0 ... l_nperm, 3 + 2 nperm doubles (all NaN if no column
 * is left) */
int mcx_debug_energy_sums(const float *rows_a, int nsteps_a, int nc_a, const float *rows_b, int nsteps_b, int nc_b, int np,
                          const mcx_energy_spec *spec, double *sums);
/* host only: the launch geometry of n_a against n_b rows of nused columns with nperm permutations.  k_energy_pairs has a grid
 * of (tiles, slabs, chunks) workgroups: tile_rows rows i each, against the slab_rows rows j of a slab (the last one shorter;
 * MCX_ENERGY_SLAB_ROWS, a multiple of 64, lowers the default: a knob for tests only, since the partials grow as the slabs
 * shrink -- about 17 GB at 64 rows and the largest call), for chunk_blocks blocks of 16 label columns (the
 * power of two that holds label_blocks, 16 at most; the last chunk may hold fewer).  label_cols = nperm + 2: a column of ones,
 * l_0, l_1 ... l_nperm */
typedef struct mcx_energy_geometry {
  long long block, tile_rows, tiles;
  long long slab_rows, slabs;
  long long label_cols, label_blocks, chunk_blocks, chunks;
  long long col_chunk;      /* columns of z staged at a time */
  long long workgroups;
  long long lds_bytes;      /* of a k_energy_pairs workgroup */
  long long scratch_bytes;  /* z, the packed labels, the partials and the sums */
} mcx_energy_geometry;
int mcx_debug_energy_geometry(int n_a, int n_b, int nused, int nperm, mcx_energy_geometry *g);
/* one mcx_samples_energy call, its results let go, ms[7]: 0 the gather of both sides, 3 the uploads, 4 k_energy_pairs, 5 the
 * reducer and its copy (HIP events); 1 scale and flags, 2 the label vectors, 6 the whole call (the host's clock) */
int mcx_debug_energy_times(mcx_engine *e, int first_a, int nsteps_a, int first_b, int nsteps_b, const mcx_energy_spec *spec,
                           double *ms);

/* ---- importance weights on a store ----------------------------------
 * The rows of a store reweighted to a posterior close to the sampled one, without a rerun.  N = nsteps * nc rows in row order
 * (step-major, the chain within the step), 1 <= N < 2^31 (MCX_ERR_UNSUPPORTED from 2^31 on); any nsteps >= 1.
 * The weight source gives a value v_i per row:
 *   MCX_WEIGHT_HOST   logw[i], a host array of N floats, uploaded once
 *   MCX_WEIGHT_STORE  column col of store (same nsteps and nc, same device; col = ncol - 1 is its log L column), usually a
 *                     derived store whose function computes a log-ratio
 *   MCX_WEIGHT_LL     the view's own log L column (scale = beta - 1: the power posterior L^beta)
 * lw_i = scale * (double)v_i (scale finite; 0 and negative values are allowed).  lw = -inf is an ordinary zero weight; a NaN or
 * +inf in any lw_i, or every lw_i at -inf, is MCX_ERR_INVALID, and mcx_last_error names the lowest such row.
 * Fixed-point weights: lwmax = max lw_i, q_i = (uint32)rint(2^31 exp(lw_i - lwmax)) in fp64, ties to even: 0 <= q_i <= 2^31,
 * and some row has 2^31.  A row below 2^-32 of the largest weight has q = 0 and takes part in nothing: the mass left out is
 * below N 2^-32 of the largest weight.  Everything else is integer sums of q or fp64 sums in a fixed order: the same store and
 * arguments give the same bytes in every entry point.
 *   n, nzero         rows, and rows with q = 0
 *   sumq             Q = sum q_i (< 2^62);  sumq2_hi : sumq2_lo = sum q_i^2, exact in 128 bits
 *   ess_kish         Q^2 / sum q_i^2, Kish's effective size
 *   log_mean_w       lwmax + log(Q / (2^31 N)): the log of the average weight -- the log-ratio of the two normalising constants
 *                    when the weights are a ratio of unnormalised densities
 *   tail_m, khat, tail_sigma   the M = min(floor(N / 5), ceil(3 sqrt(N))) largest q over their cutoff (the (M + 1)-th largest),
 *                    x = (q - cutoff) / 2^31, fitted by mcx_khat_of_tail: the Pareto tail index of Vehtari et al.  The weights are
 *                    not smoothed (no PSIS): khat is reported, the raw weights are used
 *   flags            MCX_REWEIGHT_NO_TAIL (khat and tail_sigma are NaN: M < 5, or ties at the cutoff reach a quarter into the
 *                    tail, e.g. constant weights), MCX_REWEIGHT_KHAT_HIGH (khat > 0.7: do not trust the estimates)
 * Per column, over the rows with q > 0 only (a q = 0 row is never multiplied in):
 *   mean             sum q x / Q;  sd = sqrt(sum q (x - mean)^2 / Q), two passes
 *   mcse_mean        sqrt(sum q^2 (x - mean)^2) / Q: the delta-method error of the self-normalised estimate.  It ignores the
 *                    autocorrelation of the rows
 *   min, max         the smallest and largest value among rows with q > 0, in mcx_samples_summary's key order (NaN last, -0
 *                    before +0)
 *   quantiles[col * nprobs + k]   the smallest value x of the column with C(x) >= t, C(x) the q of the rows whose key is at most
 *                    x's, t = min(Q, max(1, ceil(probs[k] (double)Q))): the weighted inverse ECDF (R type 1), always a float of
 *                    the column, no interpolation; numpy.quantile(method="inverted_cdf") at equal weights
 *   flags            MCX_REWEIGHT_NONFINITE: a row with q > 0 holds an inf or NaN in the column; mean, sd and mcse_mean are NaN,
 *                    min, max and the quantiles stay defined by the order
 * MCX_ERR_INVALID before anything is allocated: a NULL store, rows, w, res or cols, an unknown kind, a NULL logw or weight
 * store, a weight store of another shape or device, col outside it, a scale that is not finite, nprobs outside [0,
 * MCX_REWEIGHT_MAX_PROBS], a probability outside [0, 1], probs or quantiles NULL with nprobs > 0. */
enum { MCX_WEIGHT_HOST = 1, MCX_WEIGHT_STORE = 2, MCX_WEIGHT_LL = 3 };  /* mcx_weights.kind */
enum { MCX_REWEIGHT_NO_TAIL = 1, MCX_REWEIGHT_KHAT_HIGH = 2 };          /* mcx_reweight_result.flags */
enum { MCX_REWEIGHT_NONFINITE = 1 };                                    /* mcx_col_reweight.flags */
enum { MCX_REWEIGHT_MAX_PROBS = 64 };
typedef struct mcx_weights {
  int kind;
  const float *logw; /* MCX_WEIGHT_HOST */
  mcx_store *store;  /* MCX_WEIGHT_STORE */
  int col;
  double scale;
} mcx_weights;
typedef struct mcx_reweight_result {
  long long n, nzero;
  double lwmax;
  long long sumq;
  unsigned long long sumq2_hi, sumq2_lo;
  double ess_kish, log_mean_w;
  long long tail_m;
  double khat, tail_sigma;
  int flags, reserved;
} mcx_reweight_result;
typedef struct mcx_col_reweight {
  double mean, sd, mcse_mean;
  float min, max;
  int flags, reserved;
} mcx_col_reweight;
int mcx_store_reweight(mcx_store *s, const mcx_weights *w, const double *probs, int nprobs, mcx_reweight_result *res,
                       mcx_col_reweight *cols, double *quantiles);
/* steps [first_step, first_step + nsteps) of an engine's store, cols[np + 1]; a queued MCX_OPT_ASYNC_RUN run is finished first */
int mcx_samples_reweight(mcx_engine *e, int first_step, int nsteps, const mcx_weights *w, const double *probs, int nprobs,
                         mcx_reweight_result *res, mcx_col_reweight *cols, double *quantiles);
/* host rows in MCout layout (np + 1 columns) */
int mcx_rows_reweight(const float *rows, int nsteps, int nc, int np, const mcx_weights *w, const double *probs, int nprobs,
                      mcx_reweight_result *res, mcx_col_reweight *cols, double *quantiles);
/* Sampling-importance-resampling: K = nsteps_out * nc_out rows drawn with replacement in proportion to q, 1 <= K < 2^31, as a
 * store of shape (nsteps_out, nc_out, ncol).  Draw k of seed uses mcx_samples_draw's r (Philox key (seed, 5), counter k):
 * u = (r Q) >> 64, and the row is the smallest j with q_0 + ... + q_j > u, in row order; row k of the new store is a copy of
 * that row, and index[k] (may be NULL) is j.  A q = 0 row is never drawn; with equal weights index[k] is mcx_store_draw's.
 * The "chains" of the new store are not chains: its rows are exchangeable draws, so the density, pair density, covariance,
 * clip and draws mean something on it, and compare / energy in their iid forms; R-hat and the ESS of its summary do not.
 * MCX_ERR_INVALID as above, and for out NULL or nsteps_out or nc_out < 1. */
int mcx_store_resample(mcx_store *s, const mcx_weights *w, uint32_t seed, int nsteps_out, int nc_out, mcx_store **out,
                       int64_t *index);
int mcx_samples_resample(mcx_engine *e, int first_step, int nsteps, const mcx_weights *w, uint32_t seed, int nsteps_out,
                         int nc_out, mcx_store **out, int64_t *index);
int mcx_rows_resample(const float *rows, int nsteps, int nc, int np, const mcx_weights *w, uint32_t seed, int nsteps_out,
                      int nc_out, mcx_store **out, int64_t *index);
/* host only: the generalised Pareto fit of a tail.  x[0] <= ... <= x[n - 1] >= 0 are the exceedances over the cutoff.  Zhang and
 * Stephens' estimator with the weak prior of Vehtari et al., in fp64, every sum in index order: m = 30 + floor(sqrt(n)),
 * xstar = x[floor(n / 4 + 0.5) - 1]; theta_j = 1 / x[n - 1] + (1 - sqrt(m / (j - 0.5))) / (3 xstar), k_j = mean log1p(-theta_j x),
 * l_j = n (log(-theta_j / k_j) - k_j - 1) for j = 1 ... m; w_j = 1 / sum_i exp(l_i - l_j); theta = sum theta_j w_j,
 * k = mean log1p(-theta x), *sigma = -k / theta, *khat = (k n + 5) / (n + 10).  *flags: MCX_REWEIGHT_NO_TAIL with NaN in both
 * when n < 5, xstar = 0 or x[n - 1] = 0; MCX_REWEIGHT_KHAT_HIGH when khat > 0.7 */
int mcx_khat_of_tail(const double *x, long long n, double *khat, double *sigma, int *flags);
/* tests only: the fixed-point weights q[nsteps * nc] and lwmax of the rows of a store (rows == NULL) or of host rows in MCout
 * layout (s == NULL); exactly one of the two is given */
int mcx_debug_reweight_q(mcx_store *s, const float *rows, int nsteps, int nc, int np, const mcx_weights *w, uint32_t *q,
                         double *lwmax);
/* host only: the launch geometry for N rows of ncol columns, nprobs probabilities and K draws (K = 0: no resample), computed by
 * the functions the passes call.  k_rw_max and k_rw_q give a workgroup one scan tile of scan_tile_rows rows; the histogram
 * passes take hist_prefixes target prefixes a launch on parameter tiles hist_tile_cols wide, their 64-bit bins within
 * hist_lds_budget bytes of LDS (two workgroups and more per compute unit); k_rw_draw gives a lane one draw */
typedef struct mcx_reweight_geometry {
  long long block, scan_tile_rows, scan_tiles;
  long long hist_targets, hist_prefixes, hist_launches, hist_tile_cols, hist_lds_bytes, hist_lds_budget;
  long long tail_m, sort_tiles;
  long long draw_workgroups;
  long long scratch_bytes; /* of a reweight call, or of a resample call when K > 0 */
  long long scan_tiles_per_lane; /* consecutive scan tiles a lane of k_rw_scan owns: ceil(scan_tiles / block) */
  long long hist_step_chunks;    /* grid.y of the histogram passes, ceil(nsteps / 65536); 0 from the entry that is given N alone */
} mcx_reweight_geometry;
int mcx_debug_reweight_geometry(long long N, int ncol, int nprobs, long long K, mcx_reweight_geometry *g);
/* the same for N = nsteps * nc rows, with hist_step_chunks, which depends on how N splits into steps and chains */
int mcx_debug_reweight_store_geometry(int nsteps, int nc, int ncol, int nprobs, long long K, mcx_reweight_geometry *g);
/* one mcx_samples_reweight call and, when nsteps_out * nc_out > 0, one mcx_samples_resample call, their results let go.  ms[8],
 * HIP events: 0 k_rw_max and its reducer, 1 k_rw_q and the scan, 2 the two moment passes, 3 the four histogram passes, 4 the
 * sort of q, 5 k_rw_draw, 6 the whole reweight call, 7 the whole resample call */
int mcx_debug_reweight_times(mcx_engine *e, int first_step, int nsteps, const mcx_weights *w, const double *probs, int nprobs,
                             uint32_t seed, int nsteps_out, int nc_out, double *ms);

/* ---- interval estimates of the sample store, on the device ----------
 * What the table of posterior::summarise_draws / arviz.summary holds beyond mcx_samples_summary.  Columns as there (the np
 * parameters, then log L), N = nsteps * nc values per column, nsteps >= 4.  s(0) <= ... <= s(N - 1) are the column's floats in
 * the key order of the rank summary: -0 and +0 are one value (reported as +0), every NaN sorts last.
 *   HDI of mass p, 0 < p < 1 (arviz's hdi): span m = min(floor(p N), N - 1); w(i) = double(s(i + m)) - double(s(i)) for 0 <= i <
 *              N - m; index = the smallest i with the smallest w; lo = s(index), hi = s(index + m), width = w(index)
 *   ess_sd, mcse_sd (posterior's): c2 = float((double(x) - mean)^2), ess_sd and ess_sd_lag the ess and ess_lag of the store of
 *              c2 as mcx_samples_summary defines them; mcse_sd = sqrt((N - 1) / N sd_c2^2 / ess_sd / mean_c2 / 4)
 *   ess_q, mcse_q of a probability p (posterior's ess_quantile, mcse_quantile): q = mcx_samples_summary's type-7 quantile, bit
 *              for bit; ess_q and ess_q_lag those of the store of the indicators double(x) <= q (1.0f / 0.0f); u_lo, u_hi = the
 *              quantiles of 0.1586553 and 0.8413447 of the beta law (ess_q p + 1, ess_q (1 - p) + 1), by mcx_beta_quantile;
 *              k_lo = max(floor(u_lo N), 1) - 1, k_hi = min(ceil(u_hi N), N) - 1; s_lo = s(k_lo), s_hi = s(k_hi);
 *              mcse_q = (double(s_hi) - double(s_lo)) / 2
 * A column holding an inf or NaN has MCX_SUMMARY_NONFINITE, NaN in every double and float and -1 in index, k_lo and k_hi (span
 * stays m).  A transformed column that is constant within every half-chain gives NaN ess and mcse, NaN u and s and -1 ranks for
 * what is built on it.  A constant column's HDI is lo = hi, width 0, index 0. */
enum { MCX_INTERVAL_MAX_MASSES = 8, MCX_INTERVAL_MAX_PROBS = 8, MCX_INTERVAL_TIMES = 12 };
typedef struct mcx_interval_spec {
  int nmass;           /* 0 to MCX_INTERVAL_MAX_MASSES */
  int nprobs;          /* 0 to MCX_INTERVAL_MAX_PROBS */
  const double *mass;  /* nmass masses in (0, 1) */
  const double *probs; /* nprobs probabilities in [0, 1] */
} mcx_interval_spec;
typedef struct mcx_col_intervals {
  double mean, sd;         /* mcx_samples_summary's */
  double ess_sd, mcse_sd;
  int ess_sd_lag, flags;   /* MCX_SUMMARY_* */
} mcx_col_intervals;
typedef struct mcx_col_hdi {
  double width;
  long long index, span;
  float lo, hi;
} mcx_col_hdi;
typedef struct mcx_col_quantile_se {
  double q, ess_q, u_lo, u_hi, mcse_q;
  long long k_lo, k_hi;
  float s_lo, s_hi;
  int ess_q_lag, reserved;
} mcx_col_quantile_se;
/* Steps [first_step, first_step + nsteps) of the store.  cols[np + 1]; hdi[(np + 1) * nmass] and qse[(np + 1) * nprobs], row =
 * column (each may be NULL when its count is 0).  MCX_ERR_INVALID, before a device is touched, for nsteps < 4, a mass outside
 * (0, 1), a probability outside [0, 1], a count outside its range and a NULL output, and in the cases mcx_samples_summary
 * refuses; MCX_ERR_UNSUPPORTED for N >= 2^31; MCX_ERR_ALLOC, with the bytes needed in mcx_last_error, when the scratch (4 N (np +
 * 1) bytes of transformed store, then 8 N bytes of keys per column sorted at a time) does not fit even one column at a time.
 * The same store and arguments give the same bytes. */
int mcx_samples_intervals(mcx_engine *e, int first_step, int nsteps, const mcx_interval_spec *spec, mcx_col_intervals *cols,
                          mcx_col_hdi *hdi, mcx_col_quantile_se *qse);
/* the same for host rows in MCout layout (np + 1 columns, step-major then chain, nsteps * nc rows) */
int mcx_rows_intervals(const float *rows, int nsteps, int nc, int np, const mcx_interval_spec *spec, mcx_col_intervals *cols,
                       mcx_col_hdi *hdi, mcx_col_quantile_se *qse);
/* and for the whole of a derived store */
int mcx_store_intervals(mcx_store *s, const mcx_interval_spec *spec, mcx_col_intervals *cols, mcx_col_hdi *hdi,
                        mcx_col_quantile_se *qse);
/* host only: *x = the quantile of probability p of the beta law (a, b), the inverse of the regularised incomplete beta function
 * in fp64, for 0 <= p <= 1 and finite a >= 1, b >= 1 (MCX_ERR_INVALID and NaN otherwise) */
int mcx_beta_quantile(double p, double a, double b, double *x);
/* host only: u_lo, u_hi, k_lo, k_hi of the definition above for N values, a probability and an effective size; an ess that is
 * not a positive finite number gives NaN and -1 */
int mcx_intervals_quantile_ranks(long long N, double prob, double ess, double *u_lo, double *u_hi, long long *k_lo, long long *k_hi);
/* tests only, host only: the launch geometry of an intervals call, from the function the launches use */
typedef struct mcx_intervals_geometry {
  long long block;                 /* threads per workgroup */
  long long window_tile;           /* window starts per workgroup of k_hdi_windows */
  long long window_tiles;          /* its grid.x, ceil(N / window_tile); grid.y = the columns of a group */
  long long slab_entries;          /* (w, i) pairs per column between k_hdi_windows and k_hdi_reduce: nmass * window_tiles */
  long long slab_bytes;            /* 16 bytes each */
  long long reduce_workgroups;     /* of k_hdi_reduce per column: nmass */
  long long pick_ranks;            /* ranks per column read by k_iv_pick: 2 nprobs */
  long long transforms;            /* k_iv_transform sweeps, each followed by the summary's mixing passes: 1 + nprobs */
  long long sort_tiles;            /* sort tiles of 8192 keys per column */
  long long step_chunk, grid_y;    /* steps per workgroup of the transform and key sweeps, and their grid.y */
  long long group_cols, groups;    /* columns sorted at a time at most (MCX_RANK_GROUP_COLS caps it), and the groups that makes */
  long long store_scratch_bytes;   /* the transformed store */
  long long scratch_bytes_per_col; /* keys, counts, slab and outputs of one column of a group */
} mcx_intervals_geometry;
int mcx_debug_intervals_geometry(int nsteps, int nc, int np, int nmass, int nprobs, mcx_intervals_geometry *g);
/* mcx_samples_intervals with HIP events around its stages, for tools/intervals_bench.py.  ms[MCX_INTERVAL_TIMES]: 0 the
 * summary's spread passes, 1 the k_iv_transform sweeps, 2 the mixing passes behind them, 3 k_iv_keys, 4 .. 7 the sort passes,
 * 8 k_hdi_windows, 9 k_hdi_reduce, 10 k_iv_pick, 11 the whole call */
int mcx_debug_intervals_times(mcx_engine *e, int first_step, int nsteps, const mcx_interval_spec *spec, double *ms);

/* ---- lagged covariance of the sample store and the multivariate ESS, on the device ----------
 * Columns as in mcx_samples_summary (the np parameters, then log L; ncol = np + 1), T = nsteps kept steps of nc chains, N = T nc
 * rows, m the column means (mcx_samples_summary's bits).  For 0 <= t <= T - 1
 *   G(t)[i][j] = (1 / N) sum over chains c and steps s <= T - 1 - t of (x[c, s, i] - m_i) (x[c, s + t, j] - m_j)
 * in fp64, two passes: the globally centred, biased estimator for replicated chains.  G(t)[j][i] is the lag -t entry; G(0) is
 * symmetric in its bits, and G(0) N / (N - 1) is mcx_samples_covariance's matrix within its bound.
 * On the chosen columns -- the finite, non-constant parameters, and log L when with_ll is set -- with S(t) = (G(t) + G(t)^T) / 2,
 * P(k) = S(2k) + S(2k + 1), Sigma_k = -S(0) + 2 sum_{i <= k} P(i) and K = floor((min(T - 1, max_lag) - 1) / 2):
 *   s       the smallest k <= K at which Sigma_k is positive definite (every pivot of a double Cholesky factorisation > 0);
 *           none: MCX_MESS_NOT_PD, k_used = s = -1, Sigma, mess, ess and mcse NaN
 *   k_used  the last k of s, s + 1, ... <= K at which Sigma_k is still positive definite and log det Sigma_k > log det Sigma_{k-1};
 *           Sigma = Sigma_k_used, lags_used = 2 k_used + 2; MCX_MESS_TRUNCATED when k reached K with no test failed
 *   mess = N exp((log det Lambda - log det Sigma) / p), Lambda = G(0) N / (N - 1) on the p chosen columns (not positive definite:
 *           MCX_MESS_LAMBDA_SINGULAR and a NaN mess); ess_j = N Lambda_jj / Sigma_jj; mcse_j = sqrt(Sigma_jj / N); Sigma / N is
 *           the covariance of the Monte-Carlo error of the mean vector
 * A column holding an inf or NaN has MCX_SUMMARY_NONFINITE, a NaN mean, and NaN in its row and column of every G(t); every other
 * entry is what it would be without that column.  A constant column (G(0)_jj = 0) has MCX_LAGCOV_CONSTANT.  Both are left out of
 * Sigma and the determinants (their rows and columns of sigma, their ess and mcse are NaN).  Lags are computed a window at a
 * time, only as far as the walk (and nlags_out) needs them: lags_computed says how many.  Every lag computed is kept on the host
 * until the call returns, 8 ncol^2 bytes each: on a long unmixed range, where the walk runs to the end, max_lag is the cap. */
enum { MCX_LAGCOV_CONSTANT = 2 }; /* mcx_col_lagcov.flags, beside MCX_SUMMARY_NONFINITE */
enum { MCX_MESS_NOT_PD = 1, MCX_MESS_TRUNCATED = 2, MCX_MESS_LAMBDA_SINGULAR = 4, MCX_LAGCOV_TIMES = 5 };
typedef struct mcx_lagcov_spec {
  int max_lag;   /* >= 1; lags beyond T - 1 do not exist: pass nsteps - 1 for all */
  int nlags_out; /* G(0) .. G(nlags_out - 1) are returned in gamma, 0 <= nlags_out <= nsteps: also beyond max_lag, which bounds
                    the walk alone */
  int with_ll;   /* log L among the chosen columns */
} mcx_lagcov_spec;
typedef struct mcx_lagcov_result {
  long long N;
  int p, s, k_used, lags_used, lags_computed, flags; /* flags: MCX_MESS_* */
  double mess, logdet_lambda, logdet_sigma;
} mcx_lagcov_result;
typedef struct mcx_col_lagcov {
  double mean, ess, mcse;
  int flags, reserved;
} mcx_col_lagcov;
/* Steps [first_step, first_step + nsteps) of the store.  cols[ncol]; sigma[ncol][ncol], NaN outside the chosen columns;
 * gamma[nlags_out][ncol][ncol] (may be NULL when nlags_out is 0).  MCX_ERR_INVALID, before a device is touched and with nothing
 * allocated, for nsteps < 4, N < 2, a NULL spec or output, max_lag < 1 and nlags_out outside [0, nsteps], and in the cases
 * mcx_samples_summary refuses.  The same store and arguments give the same bytes. */
int mcx_samples_lagcov(mcx_engine *e, int first_step, int nsteps, const mcx_lagcov_spec *spec, mcx_lagcov_result *res,
                       mcx_col_lagcov *cols, double *sigma, double *gamma);
/* the same for host rows in MCout layout (np + 1 columns, step-major then chain, nsteps * nc rows) */
int mcx_rows_lagcov(const float *rows, int nsteps, int nc, int np, const mcx_lagcov_spec *spec, mcx_lagcov_result *res,
                    mcx_col_lagcov *cols, double *sigma, double *gamma);
/* and for the whole of a derived store */
int mcx_store_lagcov(mcx_store *s, const mcx_lagcov_spec *spec, mcx_lagcov_result *res, mcx_col_lagcov *cols, double *sigma,
                     double *gamma);
/* host only: the walk and the numbers made of Sigma on given matrices gamma[nlags][ncol][ncol] = G(0) .. G(nlags - 1) of N rows
 * (so K = floor((nlags - 2) / 2)); use[ncol]: the chosen columns (NULL: all).  cols[c].mean is NaN (the matrices do not hold it),
 * a NaN G(0)_cc gives MCX_SUMMARY_NONFINITE; lags_computed = nlags.  MCX_ERR_INVALID for nlags < 2, N < 2, ncol outside
 * [1, 257] and a NULL pointer other than use. */
int mcx_mess_finish(int ncol, int nlags, long long N, const double *gamma, const unsigned char *use, mcx_lagcov_result *res,
                    mcx_col_lagcov *cols, double *sigma);
/* tests only, host only: the launch geometry of a lagcov call that computes lags 0 .. nlags - 1 of nsteps steps */
typedef struct mcx_lagcov_geometry {
  long long block;              /* threads per workgroup */
  long long window_lags;        /* W: lags per sweep beyond lag 0 */
  long long rows_per_iteration; /* rows of a unit: what a workgroup loads before it multiplies */
  long long units;              /* ceil(N / rows_per_iteration) */
  long long workgroups;         /* grid.x = min(units, max(32, 512 / tiles^2)): workgroup g takes units g, g + workgroups, ...; a
                                   function of N and np */
  long long tiles;              /* 16-column tiles of the parameters */
  long long pairs_lag0;         /* tile pairs swept at lag 0: tiles (tiles + 1) / 2 */
  long long pairs;              /* at every other lag: tiles^2 */
  long long slab_rows;          /* partial sums per lag and workgroup */
  long long windows;            /* sweeps of W lags: ceil((nlags - 1) / W) */
  long long launches;           /* sweeps in all: 1 + windows */
  long long lags_computed;      /* min(nsteps, 1 + windows W) */
  long long scratch_bytes;
  long long units_lag0;         /* the lag-0 sweep alone takes larger units: ceil(N / (4 rows_per_iteration)) */
  long long workgroups_lag0;    /* and its grid.x = min(units_lag0, 4 max(32, 512 / tiles^2)) */
} mcx_lagcov_geometry;
int mcx_debug_lagcov_geometry(int nsteps, int nc, int np, int nlags, mcx_lagcov_geometry *g);
/* mcx_samples_lagcov with HIP events around its stages, for tools/lagcov_bench.py (sigma, the columns and gamma are dropped).
 * ms[MCX_LAGCOV_TIMES]: 0 the column-sum sweep, 1 the sweep of lag 0, 2 the window sweeps, 3 the reducers, 4 the whole call */
int mcx_debug_lagcov_times(mcx_engine *e, int first_step, int nsteps, const mcx_lagcov_spec *spec, mcx_lagcov_result *res, double *ms);

/* ---- modes of the sample store: k-means on the device, the mode table, chain hops ----------
 * The N = T nc rows of a range are partitioned into K clusters by Lloyd's k-means on the p = np parameters; log L takes no
 * part in a distance.
 *   scale     s_j = 1 / sd_j of mcx_samples_summary's sd of the range (spec->scale != 0), else 1; a column whose sd is 0 or
 *             not finite has s_j = 0 and takes no part
 *   distance  u_ij = (double)x_ij s_j; d2(i, k): over j = 0 .. p - 1 in that order e = u_ij - c_kj, acc = acc + e e, every
 *             subtraction, product and sum rounded on its own (no fused multiply-add); columns with s_j = 0 are skipped.
 *             Centres are held scaled, in fp64
 *   label     the lowest k that attains the least d2; a row with an inf or NaN parameter gets MCX_MODE_NONE, is counted in
 *             n_nonfinite and enters no sum.  Given centres, the labels are a function of the definition alone
 *   a pass    labels, n_changed (rows whose label differs from the pass before; before the first pass every label is
 *             MCX_MODE_NONE), n_k and S_kj = sum of u_ij over the members of k in fp64; then c_k <- S_k / n_k on the host.  A
 *             cluster with n_k = 0 keeps its centre and sets MCX_MODES_EMPTY
 *   stopping  n_changed == 0: MCX_MODES_CONVERGED; after max_iter passes: MCX_MODES_NOT_CONVERGED.  The centres returned are
 *             those the returned labels are the argmin of
 *   seeding   spec->centres ([k][np], unscaled) when given; else mcx_modes_seed on M = min(N, seed_rows) rows: every row when
 *             N <= seed_rows, else draws 0 .. M - 1 of (spec->seed, the range) as mcx_samples_draw makes them
 *   table     one more sweep with the final centres and labels: per mode n, weight = n / (N - n_nonfinite), per column the
 *             mean of its members (= the centre at convergence) and the within-mode sd sqrt(sum (u - mean)^2 / (n - 1)) / s_j,
 *             inertia = sum d2, ll_mean in fp64 (NaN when a member's log L is not finite), ll_max in float order with the
 *             first source row that holds it (NaN and -1 when a member's log L is NaN; an empty mode: NaN everywhere, -1)
 * No float atomics: float sums go through one-writer accumulators, per-workgroup slabs and a fixed-order reducer, counts are
 * integers.  The same source and arguments give the same bytes. */
enum { MCX_MODES_MAX_K = 32, MCX_MODE_NONE = 255 };
enum { MCX_MODES_CONVERGED = 1, MCX_MODES_NOT_CONVERGED = 2, MCX_MODES_EMPTY = 4, MCX_MODES_TIMES = 8 };
typedef struct mcx_modes_spec {
  int k;                 /* 1 .. MCX_MODES_MAX_K */
  int max_iter;          /* >= 1 (the wrappers' default: 50) */
  int scale;             /* non-zero: s_j = 1 / sd_j; 0: s_j = 1 */
  int seed_rows;         /* >= 1 (the wrappers' default: 16 384) */
  uint32_t seed;
  const double *centres; /* NULL, or [k][np] unscaled, all finite: replaces the seeding */
} mcx_modes_spec;
typedef struct mcx_modes_result {
  int k, iters, flags; /* flags: MCX_MODES_* */
  int reserved;        /* 0 */
  long long n, n_nonfinite, n_changed; /* rows of the range; rows labelled MCX_MODE_NONE; of the last pass */
  double inertia;      /* the sum of the modes' */
} mcx_modes_result;
typedef struct mcx_mode_row {
  long long n, ll_max_row;
  double weight, inertia, ll_mean;
  float ll_max;
  int flags; /* MCX_MODES_EMPTY for a mode without rows */
} mcx_mode_row;
typedef struct mcx_mode_chain {
  long long hops;           /* steps t >= 1 at which l_t and l_{t-1} are both valid and differ */
  long long dominant_steps; /* visits of the dominant mode */
  int dominant;             /* the mode the chain visits most, the lowest on ties; MCX_MODE_NONE when no label is valid */
  int first_label, last_label; /* at steps 0 and T - 1 */
  int reserved;             /* 0 */
} mcx_mode_chain;
/* The labels of a call: it owns a byte per row on the device and a stream, and remembers (T, nc, ncol, k) of its source but
 * not the rows.  It depends neither on the engine nor on the store it came from.  One thread at a time per handle. */
typedef struct mcx_modes mcx_modes;
/* Steps [first_step, first_step + nsteps) of the engine's store (a queued asynchronous run is finished first), nsteps >= 1,
 * N >= 2 when spec->scale is set.  table[k]; centres_scaled, centres, means, sds [k][np] (centres, means and sds unscaled; NaN
 * in a column that takes no part, and for an empty mode's means and sds); scale[np].  out may be NULL (the labels are let go).
 * MCX_ERR_INVALID, before a device is touched and with nothing allocated, for a NULL pointer other than out and
 * spec->centres, k outside [1, MCX_MODES_MAX_K] or greater than N, max_iter < 1, seed_rows < 1, np outside [1, 256], N < 2 with
 * spec->scale set and a centre that is not finite (the entry is named); after the seed sample is fetched, for k greater than its rows with finite parameters; and in the
 * cases mcx_samples_summary refuses (the store does not hold the range).  MCX_ERR_ALLOC names the bytes. */
int mcx_samples_modes(mcx_engine *e, int first_step, int nsteps, const mcx_modes_spec *spec, mcx_modes_result *res,
                      mcx_mode_row *table, double *centres_scaled, double *centres, double *means, double *sds, double *scale,
                      mcx_modes **out);
/* the same for host rows in MCout layout (np + 1 columns, step-major then chain, nsteps * nc rows) */
int mcx_rows_modes(const float *rows, int nsteps, int nc, int np, const mcx_modes_spec *spec, mcx_modes_result *res,
                   mcx_mode_row *table, double *centres_scaled, double *centres, double *means, double *sds, double *scale,
                   mcx_modes **out);
/* and for the whole of a derived store */
int mcx_store_modes(mcx_store *s, const mcx_modes_spec *spec, mcx_modes_result *res, mcx_mode_row *table, double *centres_scaled,
                    double *centres, double *means, double *sds, double *scale, mcx_modes **out);
int mcx_modes_destroy(mcx_modes *m); /* NULL is fine */
/* any of the four may be NULL */
int mcx_modes_shape(const mcx_modes *m, int *nsteps, int *nc, int *ncol, int *k);
/* labels[nrows] of source rows [first_row, first_row + nrows), row = step * nc + chain */
int mcx_modes_labels(mcx_modes *m, long long first_row, long long nrows, unsigned char *labels);
/* Integers from the labels alone; any output may be NULL.  chains[nc]; visits[nc][k]: the steps chain c spends in mode k;
 * trans[k][k]: the pairs (l_{t-1}, l_t) with both valid over all chains and steps t >= 1, a = b included; occupancy[T][k]: the
 * chains in mode k at step t.  One lane walks a chain's T labels: many steps of few chains are slow, as in section 16. */
int mcx_modes_chain_table(mcx_modes *m, mcx_mode_chain *chains, long long *visits, long long *trans, long long *occupancy);
/* A store of T steps of nc chains with k columns, column j = 1.0f where the row's label is j and 0.0f elsewhere (a row
 * labelled MCX_MODE_NONE is all zero), and log L = 0 (the handle does not hold the source's): mcx_store_summary of it gives
 * every mode's weight as the mean, with its MCSE, R-hat and ESS. */
int mcx_modes_indicator_store(mcx_modes *m, mcx_store **out);
/* The rows of mode k of the source the handle was made from (or of any source of the same shape), in source order, as a
 * row set (section 14).  MCX_ERR_INVALID for a source whose (nsteps, nc, np + 1) is not the handle's and k outside [0, m's k). */
int mcx_samples_mode_rows(mcx_engine *e, int first_step, int nsteps, mcx_modes *m, int k, mcx_rowset **out);
int mcx_rows_mode_rows(const float *rows, int nsteps, int nc, int np, mcx_modes *m, int k, mcx_rowset **out);
int mcx_store_mode_rows(mcx_store *s, mcx_modes *m, int k, mcx_rowset **out);
/* host only: k-means++ on rows[nrows][np + 1] (MCout layout) with the scale s[np] -> index[k], the seed rows.
 *   centre 0  the row of the largest log L, first on ties (a NaN log L counts as -inf), among the rows with finite parameters
 *   centre j  D_i = the least d2 of row i from centres 0 .. j - 1 (0 for a row that is not finite), cum_i their running sum
 *             in index order in fp64; the first i with cum_i > u cum_{nrows-1}, u = the top 53 bits of words x : y of Philox
 *             block (j, 0, 0, 0) under key (seed, 7) times 2^-53 (stream 7 is this unit's alone).  When every row sits on a
 *             centre: the first finite row not yet taken
 * MCX_ERR_INVALID for NULL pointers, np outside [1, 256], k outside [1, MCX_MODES_MAX_K] and fewer than k finite rows. */
int mcx_modes_seed(const float *rows, long long nrows, int np, int k, uint32_t seed, const double *s, long long *index);
/* tests only: one pass over host rows with given scaled centres[k][np] and scale s[np] (a column with s = 0 takes no part,
 * whatever the centres hold there) -> labels[N], d2[N] of the winner (NaN for MCX_MODE_NONE), n[k], S[k][np]; any output may be
 * NULL */
int mcx_debug_modes_assign(const float *rows, int nsteps, int nc, int np, int k, const double *centres_scaled, const double *s,
                           unsigned char *labels, double *d2, long long *n, double *S);
/* tests only, host only: the launch geometry of a modes call */
typedef struct mcx_modes_geometry {
  long long block;           /* threads per workgroup */
  long long rows_per_tile;   /* R = clip_rows of section 14: a workgroup stages R consecutive rows of all np columns */
  long long tiles;           /* ceil(N / R) */
  long long workgroups;      /* min(tiles, 1024): workgroup g takes tiles g, g + workgroups, ... */
  long long lane_groups;     /* 256 / R: a row's centre blocks are dealt among this many lanes */
  long long centre_blocks;   /* ceil(k / 8): eight running distances per lane at a time */
  long long uniform_centres; /* 1 when R >= 64: a wavefront's centres are one scalar load */
  long long sum_subgroups;   /* of the assign pass: the lane groups that share the tile's rows, min(256 / np, 2048 / (k np)), 1 at least */
  long long table_columns;   /* of the table pass: np + 2 (the squares, d2, log L) */
  long long table_subgroups; /* min(256 / min(np + 2, 256), 2048 / (k (np + 2))), 1 at least */
  long long assign_lds_bytes, table_lds_bytes;
  long long mark_workgroups, mark_mask_words; /* of mode_rows: section 14's geometry */
  long long chains_workgroups, steps_workgroups;
  long long scratch_bytes;   /* of the call's three scratch buffers */
} mcx_modes_geometry;
int mcx_debug_modes_geometry(int np, int nsteps, int nc, int k, mcx_modes_geometry *g);
/* mcx_samples_modes with HIP events around its stages, for tools/modes_bench.py (the tables and labels are let go).
 * ms[MCX_MODES_TIMES]: 0 the scale (summary passes), 1 the seed sample and seeding (wall clock), 2 the assign passes in all,
 * 3 their reducers, 4 the table pass and its reducer (2 to 4: HIP events), 5 and 6 reserved (0), 7 the whole call (wall clock) */
int mcx_debug_modes_times(mcx_engine *e, int first_step, int nsteps, const mcx_modes_spec *spec, mcx_modes_result *res, double *ms);

/* ---- evidence of a run: log Z by bridge sampling, with its error -------------------------------------
 * log Z = log of the integral of the sampled function L, from the rows of a view (their log L is in the store) and draws from
 * a proposal g, a mixture of 1 <= k <= MCX_EVIDENCE_MAX_K Gaussians with full covariances, by the iterative bridge estimator of
 * Meng & Wong with the relative error of Fruehwirth-Schnatter.  All of it is fp64 on the device through slabs and a
 * fixed-order reducer: the same arguments give the same bytes.
 *   proposal   mcx_evidence_mixture: weights[k] > 0, centres[k][np], covs[k][np][np] (row-major, the lower triangle is read),
 *              scale > 0 multiplies every component's standard deviations.  NULL: k = 1, centre and covariance are section 10's
 *              mean and covariance of the parameters over the first fit_steps steps of the view (default nsteps / 2), which are
 *              then left out of the bridge; spec->scale scales it.  With a caller's proposal fit_steps defaults to 0.
 *   log g(x)   u = (double)x - c_k, z = W_k u with W_k the inverse of the lower Cholesky factor C_k of scale^2 covs[k],
 *              t_k = lc_k - sum z_i^2 / 2, lc_k = log(w_k / sum w) - sum log diag C_k - (np / 2) log 2 pi, log-sum-exp over k;
 *              NaN for a row with a non-finite parameter
 *   rows       N1 = (nsteps - fit_steps) * nc, l1_i = log L_i - log g(x_i); a non-finite l1 is MCX_ERR_INVALID naming the lowest
 *              such row
 *   draws      N2 = spec->ndraw (0: min(N1, 2^20)), Philox stream 8: the component of draw j from the uniform of block
 *              (j, 0, 1, 0), its normals z[4b .. 4b+3] those of mcx_debug_normals(seed, 8, j, b, 0, 0), x~_i = (float)(c_i + sum_{l
 *              <= i} C_il (double)z_l), l ascending, no fused multiply-add; log L of the draws by L's device code (the callback
 *              for MCX_VL_HOST); l2_j = log L - log g(x~_j); log L = -inf or NaN counts as L = 0 (ndraw_zero), +inf is
 *              MCX_ERR_INVALID, and so are draws that all have L = 0
 *   bridge     neff = the lower median over the parameters of mcx_samples_summary's ess on the N1 rows, at most N1 (N1 itself
 *              with use_neff = 0, or with MCX_EVIDENCE_NO_ESS when fewer than 4 steps remain or an ess is NaN); s1 = neff / (neff
 *              + N2), s2 = N2 / (neff + N2); l* = mean l1; r <- (mean over draws of num) / (mean over rows of den) from r = 1 until
 *              |delta log r| <= tol or max_iter passes (MCX_EVIDENCE_NOT_CONVERGED); log_z = log r + l*
 *   error      f1 = p / (s1 p + s2) over the draws, f2 = 1 / (s1 p + s2) over the rows, p = e^(l - log_z); re2_draws = Var f1 /
 *              (mean(f1)^2 N2), re2_rows = Var f2 / (mean(f2)^2 ess_f2) (variances with divisor n - 1), ess_f2 = the summary's ess
 *              of the series f2 as a one-column store of floats (N1 when that is NaN or the range too short); se = sqrt of their sum
 *   log_z_is   log mean e^(l2), importance sampling from g alone; log_z_ris = -log mean e^(-l1), the reciprocal estimator
 * L: the sampled function (L->d = np); NULL for mcx_samples_evidence = the last run's.  mcx_store_evidence is for stores whose
 * columns are the parameters (a text read back, chosen chains, a row set's store).
 * MCX_ERR_INVALID before a device is touched: a NULL argument, k outside 1 .. 8, a weight <= 0, a scale that is not finite and
 * positive, fit_steps outside [0, nsteps) (-1 = the default), a fitted proposal with fit_steps = 0, L->d != np, tol < 0 or NaN,
 * max_iter < 0, ndraw < 0, a covariance that is not positive definite (the message names the component and the pivot).
 * MCX_ERR_UNSUPPORTED: N1 or N2 >= 2^31. */
enum { MCX_EVIDENCE_MAX_K = 8 };
enum { MCX_EVIDENCE_NOT_CONVERGED = 1, MCX_EVIDENCE_NO_ESS = 2 };
typedef struct mcx_evidence_mixture {
  int k;                 /* 1 .. MCX_EVIDENCE_MAX_K */
  int reserved;          /* 0 */
  const double *weights; /* [k] */
  const double *centres; /* [k][np] */
  const double *covs;    /* [k][np][np] */
  double scale;          /* > 0 */
} mcx_evidence_mixture;
typedef struct mcx_evidence_spec {
  long long ndraw; /* 0: min(N1, 2^20) */
  uint32_t seed;
  int fit_steps;   /* -1: nsteps / 2 for a fitted proposal, 0 for a caller's */
  int use_neff;    /* 0: neff = N1 */
  int max_iter;    /* 0: 1000 */
  double tol;      /* >= 0; 1e-10 is what the drivers use */
  double scale;    /* of the fitted proposal, > 0 */
} mcx_evidence_spec;
typedef struct mcx_evidence_result {
  long long n1, n2;
  int k, fit_steps;
  double neff, lstar, log_z, se, re2_draws, re2_rows, ess_f2, log_z_is, log_z_ris;
  long long ndraw_zero;
  int iters, flags; /* MCX_EVIDENCE_* */
} mcx_evidence_result;
int mcx_samples_evidence(mcx_engine *e, int first_step, int nsteps, const mcx_vlfunc *L, const mcx_evidence_spec *spec,
                         const mcx_evidence_mixture *proposal, mcx_evidence_result *res);
int mcx_rows_evidence(const float *rows, int nsteps, int nc, int np, const mcx_vlfunc *L, const mcx_evidence_spec *spec,
                      const mcx_evidence_mixture *proposal, mcx_evidence_result *res);
int mcx_store_evidence(mcx_store *s, const mcx_vlfunc *L, const mcx_evidence_spec *spec, const mcx_evidence_mixture *proposal,
                       mcx_evidence_result *res);
/* host only, no device: the factors of a proposal.  C[k][np][np] the lower Cholesky factors of scale^2 covs (may be NULL),
 * W[k][np][np] their inverses (may be NULL), lc[k] */
int mcx_evidence_proposal(int np, const mcx_evidence_mixture *m, double *C, double *W, double *lc);
/* host only, no device: the estimator on host arrays l1[n1] and l2[n2] (an l2 of -inf is a draw with L = 0), by the update and
 * finish functions of the device path with sums in index order.  The host has no spectral estimate: ess_f2 = n1.  Fills lstar,
 * log_z, se, re2_draws, re2_rows, ess_f2, log_z_is, log_z_ris, ndraw_zero, iters, flags, n1, n2, neff of res (k = fit_steps = 0). */
int mcx_evidence_iterate(const double *l1, long long n1, const double *l2, long long n2, double neff, double tol, int max_iter,
                         mcx_evidence_result *res);
/* tests only: log g of n host rows x[n][np] (parameters alone) under a proposal -> lg[n], by the sweep kernel of the calls */
int mcx_debug_evidence_logg(const float *x, long long n, int np, const mcx_evidence_mixture *m, double *lg);
/* tests only: the first ndraw draws of (seed, proposal): x[ndraw][np], comp[ndraw], lg[ndraw] = log g of the rounded rows, and with
 * L not NULL ll[ndraw] = their log L as the calls evaluate it (any of the four may be NULL) */
int mcx_debug_evidence_draws(int np, const mcx_evidence_mixture *m, const mcx_vlfunc *L, uint32_t seed, long long ndraw, float *x,
                             int *comp, double *lg, float *ll);
/* tests only: mcx_rows_evidence that also returns l1[N1] and l2[N2] as the bridge passes read them */
int mcx_debug_evidence_l(const float *rows, int nsteps, int nc, int np, const mcx_vlfunc *L, const mcx_evidence_spec *spec,
                         const mcx_evidence_mixture *proposal, mcx_evidence_result *res, double *l1, double *l2);
/* host only, no device: the launch geometry of a call on n1 rows and n2 draws of np parameters */
typedef struct mcx_evidence_geometry {
  long long block;          /* threads per workgroup: 256 */
  long long tile_rows;      /* R: rows per tile of the sweep, 64 up to np = 128 and 32 above */
  long long slices;         /* 256 / R lanes per row, lane s taking the outputs i = s, s + slices, ... */
  long long sweep_tiles, sweep_workgroups; /* tiles of n1 rows; workgroups, at most sweep_max_workgroups (each takes tiles in turn) */
  long long sweep_max_workgroups;
  long long sweep_lds_bytes;
  long long use_mfma;       /* 0: the product runs on the vector unit at every np */
  long long w_chunk_rows;   /* rows of W_k staged in LDS at a time: np when 2048 / np >= np, else 2048 / np rounded down to slices */
  long long draw_rows;      /* draws per workgroup of the draw kernel: max(16, 256 / np) */
  long long draw_workgroups, draw_lds_bytes;
  long long terms_workgroups_rows, terms_workgroups_draws; /* of a bridge pass: ceil(n / 1024), at most 1024 each */
  long long scratch_bytes;  /* of the call's own device buffers, without the likelihood's and the summary's */
} mcx_evidence_geometry;
int mcx_debug_evidence_geometry(int np, long long n1, long long n2, int k, mcx_evidence_geometry *g);
/* mcx_samples_evidence with HIP events around its stages, for tools/evidence_bench.py.  ms[MCX_EVIDENCE_TIMES]: 0 the fit
 * (section 10), 1 the draws, 2 the likelihood of the draws, 3 the sweep of the rows (k_ev_logg), 4 the sweep of the draws, 5 neff and
 * ess_f2 (the summary passes), 6 all bridge passes with their reducers, 7 the whole call (wall clock) */
enum { MCX_EVIDENCE_TIMES = 8 };
int mcx_debug_evidence_times(mcx_engine *e, int first_step, int nsteps, const mcx_vlfunc *L, const mcx_evidence_spec *spec,
                             const mcx_evidence_mixture *proposal, mcx_evidence_result *res, double *ms);

/* ---- profile likelihoods of a store: per parameter, per pair, with intervals --------------------------
 * pl_c(x) = max { log L(row) : the row's column c in the bin of x } - max log L, over the N = nsteps * nc rows of a view, 2 <= N <
 * 2^32 (MCX_ERR_UNSUPPORTED from 2^32 on).  The columns profiled are the np parameters (of a derived store the nout outputs), not
 * log L.  Integer maxima and integer adds on the device, serial host steps: the same arguments give the same bytes.
 *   order      log L in section 9's float order as a u32 key k(l) = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000): -0 before
 *              +0, a NaN counted as -inf.  The key of row r is K(r) = k(l_r) << 32 | (0xFFFFFFFF - r): its maximum is the largest
 *              log L, the first row on ties; 0 is "empty"
 *   grid       from / to: the column's min / max; with a clip pair other than (0, 1) its type-7 quantiles; the spec's from[c] /
 *              to[c] over both where not NaN.  n bins, inv = n / (to - from); a value v goes to bin floor(((double)v - from) inv)
 *              (no fused multiply-add), v == to to bin n - 1, anything else outside [0, n) is dropped; with to == from the
 *              values equal to it go to bin 0
 *   bin        cnt; the maximum key of its rows -> lmax (the row's log L as stored, -inf for a NaN), row; xat = the column's value
 *              in that row, the abscissa of the curve; path = the whole row, log L last.  An empty bin has row -1, lmax -inf,
 *              NaN xat, pl -inf, NaN plh and path
 *   fit        lhat / row_hat: the maximum key of all N rows, binned or not; xhat the column's value there.  pl = (double)lmax -
 *              (double)lhat.  A lhat that is not finite sets MCX_PROFILE_LL_NONFINITE and makes every pl, plh and interval NaN
 *   hull       plh: the least concave majorant of the points (xat, pl) of the non-empty bins, evaluated at xat (Andrew's monotone
 *              chain, a point popped on a cross product >= 0; between two vertices the chord, never below pl).  A non-empty bin at
 *              pl = -inf takes no part and keeps -inf
 *   intervals  per level p: drop = z^2 / 2, z the normal quantile of (1 + p) / 2 (levels_are_drops: the entries are drops); on
 *              the raw curve and on the hull each, jl / jh the first / last non-empty bins with y >= -drop, the end the linear
 *              interpolation at -drop towards the nearest non-empty bin outside (xat[jl] itself when that bin is at -inf), or
 *              xat[jl] with MCX_PROFILE_OPEN_LO (MCX_PROFILE_HULL_OPEN_LO) when there is none; the upper end alike; NaN ends with
 *              MCX_PROFILE_NO_BIN when no bin reaches the level.  nseg: the maximal runs of non-empty bins with pl >= -drop
 *   pairs      cell (ia, ib) of pair (a, b), a != b, from each column's own grid at n = g, 8 <= g <= 64; a row counts when both
 *              values are binned; z = lmax - lhat; levels by drop = -log(1 - p); nlevel = the non-empty cells with z >= -drop
 * A column holding an inf or NaN has MCX_SUMMARY_NONFINITE, bins nothing and has NaN in every double of its record, curves and
 * intervals (of its pairs: in z); every other column is what it would be without it. */
enum { MCX_PROFILE_MAX_LEVELS = 8 };
enum { MCX_PROFILE_LL_NONFINITE = 2, MCX_PROFILE_OPEN_LO = 4, MCX_PROFILE_OPEN_HI = 8, MCX_PROFILE_NO_BIN = 16,
       MCX_PROFILE_HULL_OPEN_LO = 32, MCX_PROFILE_HULL_OPEN_HI = 64 };
typedef struct mcx_profile_spec {
  int n;                   /* bins per column, 2 .. 512 */
  double clip_lo, clip_hi; /* (0, 1): from min to max */
  const double *from, *to; /* [np], NaN for a column's default; may be NULL */
  int nlevels;             /* 0: the levels 0.6827 and 0.9545; at most MCX_PROFILE_MAX_LEVELS */
  const double *levels;    /* [nlevels] confidence levels in (0, 1), or drops of log L > 0 */
  int levels_are_drops;
} mcx_profile_spec;
typedef struct mcx_col_profile {
  double from, to, lhat, xhat;
  long long row_hat, nvalues, nbinned, ndropped;
  int nempty, flags; /* MCX_SUMMARY_NONFINITE, MCX_PROFILE_LL_NONFINITE */
} mcx_col_profile;
typedef struct mcx_profile_interval_t {
  double p, drop, lo, hi, lo_hull, hi_hull; /* p is NaN where the spec gave drops */
  int nseg, flags;                          /* MCX_PROFILE_OPEN_*, MCX_PROFILE_HULL_OPEN_*, MCX_PROFILE_NO_BIN, MCX_SUMMARY_NONFINITE */
} mcx_profile_interval_t;
/* Steps [first_step, first_step + nsteps) of the store; cols[np]; cnt, lmax, row, xat, pl, plh [np][n]; intervals[np][L], L =
 * nlevels, or 2 for the defaults; path[np][n][np + 1] or NULL.  MCX_ERR_INVALID, before a device is touched, in the cases
 * mcx_samples_density refuses (n outside 2 .. 512 for its n) and for nlevels outside 0 .. 8, a level outside (0, 1), a drop that is
 * not positive and finite; MCX_ERR_ALLOC with the bytes needed in mcx_last_error when the scratch does not fit.  A queued
 * MCX_OPT_ASYNC_RUN run is finished first. */
int mcx_samples_profile(mcx_engine *e, int first_step, int nsteps, const mcx_profile_spec *spec, mcx_col_profile *cols,
                        unsigned long long *cnt, float *lmax, long long *row, float *xat, double *pl, double *plh,
                        mcx_profile_interval_t *intervals, float *path);
/* the same of rows [nsteps * nc][np + 1] on the host (MCout layout), and of a derived store (its nout outputs) */
int mcx_rows_profile(const float *rows, int nsteps, int nc, int np, const mcx_profile_spec *spec, mcx_col_profile *cols,
                     unsigned long long *cnt, float *lmax, long long *row, float *xat, double *pl, double *plh,
                     mcx_profile_interval_t *intervals, float *path);
int mcx_store_profile(mcx_store *s, const mcx_profile_spec *spec, mcx_col_profile *cols, unsigned long long *cnt, float *lmax,
                      long long *row, float *xat, double *pl, double *plh, mcx_profile_interval_t *intervals, float *path);
typedef struct mcx_profile2d_spec {
  int g;                   /* nodes per axis, 8 .. 64 */
  double clip_lo, clip_hi;
  const double *from, *to;
  int npairs;              /* of pairs; not read when pairs is NULL */
  const int *pairs;        /* [npairs][2] columns, or NULL: every a < b in ascending order */
  int nlevels;
  const double *levels;
  int levels_are_drops;
} mcx_profile2d_spec;
typedef struct mcx_pair_profile {
  int a, b;
  long long nbinned; /* rows with both values binned */
  int nempty, flags; /* MCX_SUMMARY_NONFINITE (one of the two columns), MCX_PROFILE_LL_NONFINITE */
} mcx_pair_profile;
/* cols[np] (from, to at n = g, lhat, xhat, row_hat, nvalues, flags; the counts are 0); pairs_out[npairs]; cnt, lmax, row, xat_a,
 * xat_b, z [npairs][g][g], cell (ia, ib) at ia * g + ib; nlevel[npairs][L].  npairs = np (np - 1) / 2 when spec->pairs is NULL.
 * The refusals of mcx_samples_profile and of mcx_samples_density2d's pair list over the np columns */
int mcx_samples_profile2d(mcx_engine *e, int first_step, int nsteps, const mcx_profile2d_spec *spec, mcx_col_profile *cols,
                          mcx_pair_profile *pairs_out, unsigned long long *cnt, float *lmax, long long *row, float *xat_a, float *xat_b,
                          double *z, long long *nlevel);
int mcx_rows_profile2d(const float *rows, int nsteps, int nc, int np, const mcx_profile2d_spec *spec, mcx_col_profile *cols,
                       mcx_pair_profile *pairs_out, unsigned long long *cnt, float *lmax, long long *row, float *xat_a, float *xat_b,
                       double *z, long long *nlevel);
int mcx_store_profile2d(mcx_store *s, const mcx_profile2d_spec *spec, mcx_col_profile *cols, mcx_pair_profile *pairs_out,
                        unsigned long long *cnt, float *lmax, long long *row, float *xat_a, float *xat_b, double *z, long long *nlevel);
/* host only, no device: one curve -> one interval.  x[n] ascending over the non-empty bins and NaN for an empty one, y[n] the
 * curve, drop > 0 -> lo, hi, nseg, flags (MCX_PROFILE_OPEN_LO / _OPEN_HI / _NO_BIN) */
int mcx_profile_interval(int n, const double *x, const double *y, double drop, double *lo, double *hi, int *nseg, int *flags);
/* host only: the drop of log L of a confidence level p for nparams = 1 (z^2 / 2) or 2 (-log(1 - p)) */
int mcx_profile_drop(double p, int nparams, double *drop);
/* host only: one column from its swept keys[n], cnt[n], xat[n] and the maximum key of all rows, by the functions of the calls */
int mcx_debug_profile_finish(int n, const unsigned long long *keys, const unsigned long long *cnt, const float *xat, unsigned long long hat,
                             int nlevels, const double *levels, int levels_are_drops, float *lmax, long long *row, double *pl, double *plh,
                             mcx_profile_interval_t *intervals, long long *nbinned, int *nempty, int *flags);
/* tests only: the sweep alone over host rows on given grids from[np] <= to[np] -> keys, cnt [np][n], hat[1] */
int mcx_debug_rows_profile_bins(const float *rows, int nsteps, int nc, int np, int n, const double *from, const double *to,
                                unsigned long long *keys, unsigned long long *cnt, unsigned long long *hat);
/* host only, no device: the launch geometry of the sweeps of a call */
typedef struct mcx_profile_geometry {
  long long block;                /* threads per workgroup of k_profile_bins: 256 */
  long long tile_columns;         /* ct = min(np, 8) adjacent columns per workgroup */
  long long chains_per_workgroup; /* 256 / ct */
  long long column_tiles, chain_blocks;
  long long chunk_steps;          /* steps per workgroup: 2^16 / chains_per_workgroup, so that a bin's count stays a u32 */
  long long chunks, workgroups;
  long long lds_bytes;            /* 12 ct n */
  long long unroll;               /* steps whose loads are issued together */
  long long pair_block, pair_chunk_rows, pair_chunks, pair_workgroups, pair_lds_bytes; /* k_profile_pairs: 12 g^2 bytes */
  long long scratch_bytes;        /* of a profile call without a path, behind the statistics' */
  long long keys_workgroups;      /* k_profile_keys: min(ceil(N / block), keys_max_workgroups), a lane per row or a grid stride */
  long long keys_max_workgroups;  /* 4096 */
} mcx_profile_geometry;
int mcx_debug_profile_geometry(int np, int nsteps, int nc, int n, int g, int npairs, mcx_profile_geometry *geom);
/* one call with its results let go, for tools/profile_bench.py.  Profile: ms[0] the statistics passes (wall clock), ms[1]
 * k_profile_bins (HIP events), ms[2] the host grids and finish (wall clock), ms[3] the whole call.  Pairs: ms[0] the statistics,
 * ms[1] k_profile_codes and k_profile_keys, ms[2] k_profile_pairs, ms[3] k_profile_at (HIP events), ms[4] the host, ms[5] the call */
int mcx_debug_profile_times(mcx_engine *e, int first_step, int nsteps, const mcx_profile_spec *spec, double *ms);
int mcx_debug_store_profile_times(mcx_store *s, const mcx_profile_spec *spec, double *ms);
int mcx_debug_profile2d_times(mcx_engine *e, int first_step, int nsteps, const mcx_profile2d_spec *spec, double *ms);

/* ---- mutual information between columns of a store, on the device -------------------------------------
 * Which columns depend on each other at all, and how strongly: the k-nearest-neighbour estimate of Kraskov, Stoegbauer and
 * Grassberger (algorithm 1) of the mutual information of every column pair, in nats, with a permutation null.  Covariance and
 * correlation (sections 10, 24) are blind to a curved valley or to several modes; this is not.  A store view has N = nsteps * nc
 * rows in MCout order; the columns used are the parameters (a derived store's outputs), MCX_MUTINFO_WITH_LL adds the last one.
 *   rows            spec.n > 0: the n rows floor(i N / n), i < n, evenly spaced in store order (n <= N); 0: n = min(N, 4096);
 *                   -1: every row (N <= MCX_MUTINFO_MAX_ROWS).  2 <= n <= MCX_MUTINFO_MAX_ROWS
 *   scale[c], flags section 21's, over the n selected rows: fp64, centred two-pass, divisor n - 1; a value that is not finite gives
 *                   MCX_MUTINFO_COL_NONFINITE, scale 0 MCX_MUTINFO_COL_CONSTANT, the last column without MCX_MUTINFO_WITH_LL
 *                   MCX_MUTINFO_COL_UNUSED and scale NaN; MCX_MUTINFO_RAW: scale = 1.  A pair with a flagged column has
 *                   MCX_MUTINFO_PAIR_UNUSED and NaN everywhere
 *   repeated rows   a rejected step repeats its row, and a repeated point is a neighbour at distance 0, which wrecks the estimate.
 *                   A selected row is dropped when an earlier selected row equals it (float ==) in every column without a flag:
 *                   m = n - ndup points are left, in selection order.  Dropping thins the cloud where the acceptance is low: the
 *                   estimate then describes a cloud that is not quite the posterior's.  A large ndup says that the rows are too
 *                   close in time: take fewer.  m <= k: every pair has MCX_MUTINFO_PAIR_FEW and NaN, and the call returns MCX_OK
 *   z               z_ic = (double)x_ic / scale[c]
 *   permutations    pi_0 the identity; p >= 1: a Fisher-Yates shuffle of [0, m) -- for i = 0 ... m - 2, w = philox4x32_10(counter
 *                   (i, p, 0, 0), key (seed, 9)), r = w.x : w.y, j = i + ((r (m - i)) >> 64), swap.  One pi_p serves every pair
 *   a pair under p  u_i = z_ia, v_i = z_{pi_p(i) b}; da_ij = |u_i - u_j|, db_ij = |v_i - v_j|, d_ij = max(da_ij, db_ij), every
 *                   difference formed directly in fp64; eps_i the k-th smallest of {d_ij : j != i} with multiplicity (spec.k = 0: 3);
 *                   na_i = #{j != i : da_ij < eps_i}, nb_i likewise (strict);
 *                   mi_p = psi(k) + psi(m) - (1 / m) sum_i [psi(na_i + 1) + psi(nb_i + 1)], psi(q) = H_{q-1} - gamma from the table
 *                   H_0 = 0, H_q = H_{q-1} + 1 / q
 *   per pair        mi = mi_0; r_info = sqrt(1 - exp(-2 max(mi, 0))) (Linfoot: |rho| of a Gaussian pair); pearson over the m points
 *                   (fp64, two-pass, on the host); nzero = #{i : eps_i = 0} at p = 0, above 0: MCX_MUTINFO_PAIR_TIES (an indicator
 *                   column, say); perm_mean, perm_sd (divisor nperm - 1), nge = #{p >= 1 : mi_p >= mi}, p_value = (1 + nge) /
 *                   (1 + nperm): NaN at nperm = 0 (perm_sd below 2)
 *   pairs           spec.pairs == NULL: every a < b among the used columns, flagged ones included (more than 45 used columns:
 *                   MCX_ERR_INVALID, name the pairs); else spec.pairs[npairs][2], 1 <= npairs <= MCX_MUTINFO_MAX_PAIRS, a != b, both
 *                   used columns.  pairs[npairs] and perm_mi[npairs][nperm] come in that order
 * The same store and arguments give the same bytes.  MCX_ERR_INVALID before anything is allocated: a NULL store, rows, res or
 * pairs, unknown flags, sizes outside the limits.  cols[ncol] and perm_mi may be NULL; spec == NULL is all zeros.  The estimate
 * assumes independent points: rows of a chain are not, which is why the default takes rows far apart.  Not built: an fp32 or
 * packed form of the distances (the contract is fp64), more than two dimensions, rank coordinates. */
enum { MCX_MUTINFO_WITH_LL = 1, MCX_MUTINFO_RAW = 2 };                                             /* mcx_mutinfo_spec.flags */
enum { MCX_MUTINFO_COL_NONFINITE = 1, MCX_MUTINFO_COL_CONSTANT = 2, MCX_MUTINFO_COL_UNUSED = 4 };   /* mcx_mutinfo_col.flags */
enum { MCX_MUTINFO_PAIR_UNUSED = 1, MCX_MUTINFO_PAIR_FEW = 2, MCX_MUTINFO_PAIR_TIES = 4 };          /* mcx_mutinfo_pair.flags */
enum { MCX_MUTINFO_MAX_ROWS = 16384, MCX_MUTINFO_MAX_PERM = 999, MCX_MUTINFO_MAX_K = 8, MCX_MUTINFO_MAX_PAIRS = 1024 };
typedef struct mcx_mutinfo_spec {
  int n, k, nperm;
  uint32_t seed;
  unsigned flags;
  int npairs;        /* with pairs: how many */
  const int *pairs;  /* [npairs][2] or NULL */
} mcx_mutinfo_spec;
typedef struct mcx_mutinfo_result {
  long long n_rows;  /* N */
  int n_sel, ndup, m, k, npairs, nperm, nused;
} mcx_mutinfo_result;
typedef struct mcx_mutinfo_col {
  double scale;
  int flags;
} mcx_mutinfo_col;
typedef struct mcx_mutinfo_pair {
  int a, b;
  double mi, r_info, pearson, perm_mean, perm_sd, p_value;
  long long nge, nzero;
  int flags;
} mcx_mutinfo_pair;
int mcx_store_mutinfo(mcx_store *s, const mcx_mutinfo_spec *spec, mcx_mutinfo_result *res, mcx_mutinfo_col *cols, mcx_mutinfo_pair *pairs,
                      double *perm_mi);
int mcx_rows_mutinfo(const float *rows, int nsteps, int nc, int np, const mcx_mutinfo_spec *spec, mcx_mutinfo_result *res,
                     mcx_mutinfo_col *cols, mcx_mutinfo_pair *pairs, double *perm_mi);
/* a step range of an engine's store; a queued MCX_OPT_ASYNC_RUN run is finished first */
int mcx_samples_mutinfo(mcx_engine *e, int first_step, int nsteps, const mcx_mutinfo_spec *spec, mcx_mutinfo_result *res,
                        mcx_mutinfo_col *cols, mcx_mutinfo_pair *pairs, double *perm_mi);
/* host only, no device touched.  index[n]: the rows floor(i N / n) of the rule above, 1 <= n <= min(N, MCX_MUTINFO_MAX_ROWS) */
int mcx_debug_mutinfo_rows(long long N, int n, long long *index);
/* perm[m] = pi_p, 1 <= m <= MCX_MUTINFO_MAX_ROWS, 0 <= p <= MCX_MUTINFO_MAX_PERM */
int mcx_debug_mutinfo_perm(uint32_t seed, int m, int p, int *perm);
/* table[q - 1] = psi(q), q = 1 ... q_max <= MCX_MUTINFO_MAX_ROWS: what a call uploads */
int mcx_debug_mutinfo_psi(int q_max, double *table);
/* eps, na, nb [m] of one pair under one permutation -> mi (the sum over i in index order, a point's two table values added first)
 * and nzero; k < m <= MCX_MUTINFO_MAX_ROWS, 1 <= k <= MCX_MUTINFO_MAX_K, 0 <= na, nb < m */
int mcx_mutinfo_finish(const double *eps, const int *na, const int *nb, int m, int k, double *mi, long long *nzero);
/* the whole host half on host rows: res (n_rows, n_sel, ndup, m, k, nperm, nused; npairs as the call would have it), index[n_sel]
 * the selected rows, kept[n_sel] (0: dropped as a repeat), cols[np + 1], z[np + 1][m] (column-major, the m kept points in order;
 * a flagged column's stretch is 0; room for [np + 1][n_sel]).  Each output may be NULL */
int mcx_debug_mutinfo_points(const float *rows, int nsteps, int nc, int np, const mcx_mutinfo_spec *spec, mcx_mutinfo_result *res,
                             long long *index, unsigned char *kept, mcx_mutinfo_col *cols, double *z);
/* the launch geometry of m points, npairs pairs, nperm permutations: k_mi_pairs has a grid of (tiles, pairs, 1 + nperm)
 * workgroups of block threads, each lane with queries_per_lane queries, the m points streamed through LDS stage_rows at a time
 * (MCX_MUTINFO_STAGE_ROWS lowers the stage to a multiple of 64: a knob for tests only) */
typedef struct mcx_mutinfo_geometry {
  long long block, queries_per_lane, tile_rows, stage_rows, stages, tiles, workgroups;
  long long lds_bytes;      /* of a k_mi_pairs workgroup */
  long long scratch_bytes;  /* the permutations, the table, the pair list, the partials and the sums; z takes 8 m bytes a column */
} mcx_mutinfo_geometry;
int mcx_debug_mutinfo_geometry(int m, int npairs, int nperm, int k, mcx_mutinfo_geometry *g);
/* on the device: eps, na, nb [m] of pair `pair` of the call's list under permutation p, written by k_mi_pairs itself (the same
 * kernel with an output pointer).  MCX_ERR_INVALID for a pair that has MCX_MUTINFO_PAIR_UNUSED or _FEW */
int mcx_debug_mutinfo_counts(const float *rows, int nsteps, int nc, int np, const mcx_mutinfo_spec *spec, int pair, int p, double *eps,
                             int *na, int *nb);
/* one mcx_samples_mutinfo call, its results let go, ms[8]: 0 the gather, 3 the uploads, 4 k_mi_pairs, 5 the reducer and its copy
 * (HIP events); 1 scale, flags, repeats and z, 2 the permutations and the table, 6 pearson and the null, 7 the whole call (the
 * host's clock) */
int mcx_debug_mutinfo_times(mcx_engine *e, int first_step, int nsteps, const mcx_mutinfo_spec *spec, double *ms);

/* ---- the schedule of one run (host logic only, no device needed) --------------------------
 * mcx_run cuts MCPar::run's two loops (src/mcpar.cc:55-97, 99-210) into device launches between the
 * events it knows in advance: tuner checks, output dumps, exchanges and -- because the local/remote
 * coin is counter-based -- Murray steps.  mcx_plan returns exactly the item list mcx_run executes. */
enum {
  MCX_PLAN_BURN_SEGMENT = 1, /* first, nsteps: consecutive burn-in steps in one launch */
  MCX_PLAN_TUNER = 2,        /* first = last step of the segment, nsteps, aux = 1 if the tuner decides here */
  MCX_PLAN_INIT_MOMENTS = 3,
  MCX_PLAN_OUTPUT = 4,       /* first = main-loop steps completed (output hook) */
  MCX_PLAN_PUBLISH = 5,      /* first = steps completed: write this shard's (mu, sig^2) slot */
  MCX_PLAN_GATHER_BEGIN = 6, /* exchange hook, MCX_XCHG_BEGIN */
  MCX_PLAN_GATHER_WAIT = 7,  /* exchange hook, MCX_XCHG_WAIT */
  MCX_PLAN_REMOTE_STEP = 8,  /* first = isamp of a Murray (genRemote) step */
  MCX_PLAN_MAIN_SEGMENT = 9, /* first, nsteps: consecutive local main-loop steps in one launch;
                                aux = local step after which the kernel snapshots the slot, or -1 */
  MCX_PLAN_SINK = 10         /* first = main-loop steps completed, nsteps = steps of the block that just ended:
                                hand the block to the sample sink (mcx_set_sink) */
};
typedef struct mcx_plan_item {
  int kind, first, nsteps, aux;
} mcx_plan_item;
/* tbase = steps consumed by earlier runs of the engine (0 for a fresh one).  items may be NULL to
 * query the count. */
int mcx_plan(int nsamp, int nburn, int sync, float pl, uint32_t seed, uint32_t tbase, int nshards,
             int eager, int fused, int max_segment, int has_output_hook, int sink_block_steps,
             mcx_plan_item *items, int max_items, int *nitems);

/* ---- profiling (MCX_OPT_PROFILE) ---------------------------------------------------------- */
enum { MCX_K_FUSED_BURN = 0, MCX_K_FUSED_MAIN, MCX_K_PROPOSE, MCX_K_EVAL, MCX_K_ACCEPT,
       MCX_K_REMOTE,       /* a whole genRemote call: draws, sweeps, decisions and the host's survivor counts */
       MCX_K_TUNER, MCX_K_MISC,
       MCX_K_REMOTE_SWEEP, /* the all-pairs sweep kernels alone (inside MCX_K_REMOTE); chain_steps = pairs */
       MCX_K_GEN_NORMALS,  /* small-n mode: the random-number generator kernel (inside MCX_K_FUSED_*) */
       MCX_K_RUN_SMALL,    /* small-n mode: k_run_small, burn-in and main-loop steps of one launch together */
       MCX_K_REMOTE_SCREEN,/* the per-pair screen's matrix-core kernel alone (inside MCX_K_REMOTE); chain_steps = pairs */
       MCX_K_COUNT = 12 };
typedef struct mcx_profile {
  double ms[MCX_K_COUNT];
  uint64_t launches[MCX_K_COUNT];
  uint64_t chain_steps[MCX_K_COUNT];
} mcx_profile;
int mcx_get_profile(mcx_engine *e, mcx_profile *p);

/* ---- helpers for exchange / output hooks written in a host language ------------------------ */
/* copies ordered after the work queued on `stream` (NULL = the default stream); both block until done */
int mcx_copy_to_host(void *dst_host, const void *src_dev, size_t bytes, void *stream);
int mcx_copy_to_device(void *dst_dev, const void *src_host, size_t bytes, void *stream);

/* ---- misc --------------------------------------------------------------------------------- */
const char *mcx_last_error(void);
int mcx_abi_version(void);
int mcx_device_info(char *name, size_t namelen, int *cu_count, size_t *hbm_bytes);
int mcx_set_device(int device);
int mcx_device_count(int *n);
/* PCI bus id of the calling thread's current device ("0000:05:00.0"): lets a multi-process launcher see
 * whether two ranks share a GPU (RCCL refuses such a communicator) */
int mcx_device_pci_bus_id(char *buf, size_t len);
/* measured device-copy bandwidth of the current device: `reps` device-to-device copies of `bytes` bytes, timed with
 * HIP events; *gbps = (bytes read + bytes written) / time in GB/s.  What bench.py reports the HBM figures against
 * next to the nominal 8 TB/s. */
int mcx_debug_copy_bandwidth(size_t bytes, int reps, double *gbps);
/* what the library holds at this moment, process-wide (no device; fails only on NULL): out[0] device allocations, out[1]
 * pinned host allocations, out[2] streams, out[3] events -- every engine, derived store and call in flight together.  All
 * four are zero once every engine and store is destroyed and no call is running.  An engine's main stream is not counted
 * (it may be the caller's, MCX_OPT_STREAM), nor are the modules of run-time compiled sources, which stay for the process. */
int mcx_debug_live_resources(uint64_t out[4]);
/* host logic of the one-launch small-n kernel, for tests (no device): recorders yes/no and steps per phase for `own` owner
 * wavefronts per workgroup of lpc2 lanes per chain x bpl blocks per lane, and who generates what: tab[3][16][24] item
 * codes (0xffffffff ends a wavefront's list; kind << 14 | step pair << 4 | (owner, block)) */
int mcx_debug_persist_deal(int lpc2, int bpl, int own, int *rec, int *ksteps, uint32_t *tab, int max_words);
/* The step-kernel template instances.  An id packs what the launcher's own template arguments say, formed next to the
 * launch: bits 0-3 family (1 k_fused_fast, 2 k_fused_fastb, 3 k_fused_fast full covariance, 4 k_fused_fastb full
 * covariance (mirrored), 5 k_fused_fast with pre-generated normals, 6 k_gen_normals, 7 k_fused_steps, 8 k_run_small, 9 a
 * user's source compiled at run time), bits 4-10 lanes per chain (LPC or LPC2), 11-13 blocks per lane, 14-17 the likelihood
 * (LikKind; 0 none), 18 MAIN, 19-20 EmitMode (0 where the instance has no such argument), 21 REC.
 * mcx_debug_step_instances: the distinct instances launched since the last mcx_run began, in order of first launch (*n of
 * them, the first `cap` in ids).  Kept on the host in a fixed array of the engine: no device call, nothing launched differently.
 * mcx_debug_step_instance_list: every instance the launchers can launch (no device, like mcx_plan): their own dispatch
 * code run over lanes 1..64, blocks per lane 1/2/4, every likelihood, both loops, rows or none, stride 1 or 3, one or two
 * owner wavefronts and either recorder choice, stopping where it would launch. */
int mcx_debug_step_instances(mcx_engine *e, uint32_t *ids, int cap, int *n);
int mcx_debug_step_instance_list(uint32_t *ids, int cap, int *n);
/* host logic of mcx_run in small-n mode, for tests (no device): the stretch of a plan (mcx_plan) that one launch of the
 * one-launch kernel takes when the executor stands at items[index] -- items [index, *end) -- and out5 = its burn-in steps,
 * main-loop steps, 1 if it starts the moments, its first main-loop step, and the step of its main loop after which the
 * kernel snapshots the slot (or -1).  Zero steps and *end = index: nothing to merge there, the item is executed by itself.
 * gather_in_flight: the last run's final gather has not been waited for yet. */
int mcx_debug_small_stretch(const mcx_plan_item *items, int nitems, int index, int nsamp, int gather_in_flight,
                            int *end, int *out5);
/* the per-pair screen of the Murray sweeps alone (mcx_screen.hpp; np = 16 or 32), for tests: nact chains x[nact][d], in
 * groups of 128 as given, against N Gaussians musig[N][d][2] = (mu, sig2); sums != 0: the sum sweeps' bound (176), else
 * the min-arg sweep's (chain j's own Gaussian is own0 + j).  masks[(N + 63) / 64][(nact + 127) / 128]: bit b of word w
 * for group g set = Gaussian 64 w + b may matter to some chain of the group. */
int mcx_debug_murray_screen(int d, int nact, int N, const float *x, const float *musig, int own0, int sums,
                            unsigned long long *masks);
/* host logic of a Murray step, for tests (no device): what the counter block of one kernel turn says.  words[nwords >= 132],
 * 64-bit: [0] the two survivor counters (turn `it` counted in the low half when `it` is even, in the high half when odd),
 * [1, 65) the cells of the pairs kept by the min-arg sweep's screen, [65, 129) those of the sum sweeps' screens, [129] a
 * word of the kernels' own, [130, 132) tried[4] as 32-bit words: chains that came as far as candidate c of a turn over
 * candidates (multi != 0).  nact_before chains went into the turn, against N Gaussians.  out5 = the survivors, the
 * passes of the reference the turn stood for, the pairs those passes swept, the pairs kept by the min-arg screen and by
 * the sum screens so far (both 0 unless cull_can != 0). */
int mcx_debug_murray_decode(const unsigned long long *words, int nwords, int it, int multi, int cull_can,
                            int nact_before, int N, unsigned long long *out5);
/* device evaluation of the arithmetic primitives for bit-exactness tests:
 * what = 0 logf(bits), 1 expf(bits), 2 sin(2 pi w/2^32), 3 cos(...), 4 u24, 5 uopen,
 * 6 philox word 0 of ctr=(w,0,0,0) key=(0,0), 7 the kernels' lean sqrt, 8 IEEE sqrtf,
 * 9/10 packed expf lane 0/1, 11 packed logf, 12/13 packed/scalar sincos hash, 14/15 scalar/packed log of
 * the acceptance draw */
int mcx_debug_numerics(int what, int n, const uint32_t *in, uint32_t *out_bits);
/* number of float bit patterns in [lo_bits, hi_bits) where the kernels' lean sqrt (valid for +-0 and
 * positive normal floats) differs from IEEE sqrtf, and the smallest such pattern */
int mcx_debug_sqrt_sweep(uint32_t lo_bits, uint32_t hi_bits, uint64_t *nbad, uint32_t *first_bad);
/* the host step of mcx_samples_summary for one column (no device): n, M half-chains of n steps, N values; mean, var_all
 * (divisor N - 1) and var_means (B/n, divisor M - 1); acov[nlags] = the mean over half-chains of the biased autocovariance
 * (1/n) sum_{i<n-t} (x_i - m_c)(x_{i+t} - m_c); ostat = [min, max, then x(lo), x(lo+1) of every probability] as floats;
 * flags as given (MCX_SUMMARY_NONFINITE: only min, max and quantiles are computed).  *need_lags = 0 when col is complete,
 * else the number of lags the ESS sum needs (more than nlags; col's R-hat / ESS fields are then not final). */
int mcx_debug_summary_finish(int n, int M, double mean, double var_all, double var_means, const double *acov, int nlags,
                             const float *ostat, long long N, const double *probs, int nprobs, int flags,
                             mcx_col_summary *col, double *quantiles, int *need_lags);
/* mcx_samples_summary without quantiles, reporting the number of 32-lag autocovariance windows it computed */
int mcx_debug_summary_windows(mcx_engine *e, int first_step, int nsteps, int *nwin);
/* host only, no device: one digit of mcx_samples_summary's radix select for one target.  hist[256] counts, by their next 8
 * bits, the keys under the prefix found so far; rem is the target's rank among them.  *digit = the bucket that holds it (the
 * walk stops at 255 whatever the counts say), *rem_out = its rank within that bucket. */
int mcx_debug_select_step(const unsigned long long hist[256], long long rem, int *digit, long long *rem_out);
/* the autocovariance sums of mcx_rows_summary's device passes, for tests: the same kernels and launches, but every finite
 * column takes lag windows until it holds nlags lags (1 <= nlags <= n) instead of stopping where its Geyer loop does.
 * acov[(np + 1) * nlags], row = column: sum over the M half-chains of sum_{i<n-t} c_i c_{i+t}, c = the half-chain centred
 * on its mean (n M times the acov of mcx_debug_summary_finish); sumsq[np + 1]: sum over all N values of (x - mean)^2.
 * A column that is not finite gets NaN in both. */
int mcx_debug_rows_acov(const float *rows, int nsteps, int nc, int np, int nlags, double *acov, double *sumsq);
/* mcx_samples_derive with HIP events around the sweep, for tools/derive_bench.py: the sweep runs twice into the same derived
 * store, ms[0] = the time of the second in ms; the store is let go */
int mcx_debug_derive_times(mcx_engine *e, int first_step, int nsteps, const mcx_derive *f, double *ms);
/* mcx_samples_covariance with HIP events around its device passes, for tools/covariance_bench.py: ms[0] the column-sum
 * sweep (k_sum_moments, the pass mcx_samples_summary shares), ms[1] the covariance sweep, ms[2] the reducer of its partials */
int mcx_debug_covariance_times(mcx_engine *e, int first_step, int nsteps, double *ms);
/* tests only: one transformed store of mcx_rows_rank_summary back on the host, in MCout layout (out_rows[nsteps * nc * (np + 1)]).
 * what = 0: z(x), 1: z(f), 2: the indicator x <= q05, 3: x <= q95.  ranks (may be NULL; only for what 0 / 1) receives the
 * average ranks as doubles, in the same layout. */
int mcx_debug_rows_rank_transform(const float *rows, int nsteps, int nc, int np, int what, double *ranks, float *out_rows);
/* host only, no device: z[i] = PPND16(p[i]), the normal quantile function the device uses (NaN outside (0, 1)) */
int mcx_debug_normal_quantile(const double *p, int n, double *z);
/* mcx_samples_rank_summary with HIP events around its stages, for tools/rank_summary_bench.py.  ms[20]: for s = 0 (values)
 * and 1 (folded): ms[7 s] key extraction, ms[7 s + 1 .. 7 s + 4] the sort passes, ms[7 s + 5] rank look-up and transform,
 * ms[7 s + 6] the summary passes of the transformed store; ms[14], ms[15] the q05 indicator and its summary passes, ms[16],
 * ms[17] the same for q95; ms[18] the thresholds (the order-statistics passes); ms[19] the whole call */
int mcx_debug_rank_summary_times(mcx_engine *e, int first_step, int nsteps, double *ms);
/* normals of stream `stream`, counter (t, g0+i, a, q) for i < n: out[n*4] */
int mcx_debug_normals(uint32_t seed, uint32_t stream, uint32_t t, uint32_t g0, uint32_t a,
                      uint32_t q, int n, float *out);

#ifdef __cplusplus
}
#endif
#endif /* MCX_H_ */
