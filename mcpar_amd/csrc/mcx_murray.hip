// mcx_murray.hip -- MCPar::genRemote (src/mcpar.cc:315-451) on device buffers: the schedule of draws, all-pairs sweeps and
// decisions over the kernels of mcx_remote.hpp, with the exact screens that let a sweep skip rows (boxes of four
// coordinates: mcx_remote.hpp; one direction: mcx_cull_proj.hpp; the per-pair bound: mcx_screen.hpp).  A translation unit
// of its own: its kernels are the largest of the library after the step kernels.
// One call is one MurrayStep context through remote_device: murray_scratch and murray_open, min_arg_sweep, murray_passes
// (a kernel turn is pass_big, pass_multi or pass_plain over fill_remote_args; then wait_pass_counters, decode_pass and
// note_pass), murray_close.  screen_pass chooses and launches the screen of a sweep and sweep_pass the sweep behind it;
// srow_grid is the one decision on the row-by-row sweep kernel and its grid.
#include <atomic>

#include "mcx_engine_internal.hpp"
#include <sched.h>
#include "mcx_remote.hpp"
#include "mcx_cull_proj.hpp"
#include "mcx_screen.hpp"

static_assert(NACT_CULL_CELLS == CULL_NCOUNT, "mcx_engine::nact is sized for the screens' counter cells");

constexpr int SROW_UNMASKED_MAX_CHAINS = 8192;  // see srow_grid
constexpr int SROW_MAX_BLOCKS_PER_WAVE = 8;
// Few chains left (the late rejection passes: a few hundred chains, then tens, then a handful -- three or four passes per
// Murray step that cost 60-75 us each whatever they sweep, launches and one wait for the host): MULTI_K passes at once.
// The proposal and the test of pass p for chain j are functions of (step, j, p) and of sums over all Gaussians, not of
// what other chains or earlier passes did, so the next MULTI_K proposals of every remaining chain are drawn, swept and
// tested together and each chain takes the first that passes: same proposals, same tests, same order -- same bits, and
// the pass count the reference would have reached.
constexpr int MULTI_MAX_CHAINS = 1024, MULTI_K = 4;  // (from 128 / 448 / 1024 / 2048 chains: C3-murray 15.66 / 15.47 / 15.45 /
                                                     // 15.47 ms, C5 23.10 / 22.15 / 21.93 / 22.12; never: 16.7 / 23.9)
static_assert(MULTI_K == MurrayCounters::TRIED, "the counter block has a tried[] word per candidate");

// Does the row-by-row kernel take this sweep (np = 16 or 32 only), and in what grid: blocks of Gaussians per wavefront, grid y.
// 16-D masked, or over few chains: every wavefront reads its own rows through the scalar cache (no LDS, no
// barriers); unmasked over many chains the rows are better staged once per 512 chains (4.3 GB through L2 otherwise).
// 32-D: masked only (a row is two scalar fetches there) -- and then whatever share of the rows the masks leave: C5 25.5 ms
// per job so, 26.0-26.8 with the LDS kernel taking over from 15 / 30 / 50 % of the rows kept or everywhere.
// Masked min-arg sweep: several blocks per wavefront while 8192 wavefronts (eight per SIMD) remain -- 310 -> 72 us
// per 65 536 x 65 536 sweep at 1 % of the rows.  The sum sweep has no own-Gaussian args to redo per block and
// its surviving rows are many more in some groups than in others: eight blocks per wavefront 508 -> 600 us.
struct SrowGrid {
  bool use;
  int bpw, gy;
};
template <int DM, bool SUMS>
static SrowGrid srow_grid(int cnt, const unsigned long long *excl, int ngroups, int S)
{
  if constexpr (DM == 16 || DM == 32) {
    if (excl || (DM == 16 && cnt <= SROW_UNMASKED_MAX_CHAINS)) {
      int bpw = (excl && !SUMS) ? (int)(((long long)ngroups * S) / 8192) : 1;
      bpw = bpw < 1 ? 1 : (bpw > SROW_MAX_BLOCKS_PER_WAVE ? SROW_MAX_BLOCKS_PER_WAVE : bpw);
      return {true, bpw, (S + bpw - 1) / bpw};
    }
  }
  return {false, 1, S};
}

// rows [y0, y0 + ny) of the row-by-row sweep's grid (the whole sweep, or a column chunk of a pass), on stream st
template <int DM, bool SUMS>
static void launch_srow_range(const float *x, const int *list, int cnt, const float *qpar, float *psum, float *pmax, int N, int own0,
                              const unsigned long long *excl, int ngroups, int bpw, int y0, int ny, hipStream_t st)
{
  if constexpr (DM == 16 || DM == 32)
    hipLaunchKernelGGL((k_remote_sweep_srow<DM, SUMS>), dim3((unsigned)((ngroups + BLOCK / 64 - 1) / (BLOCK / 64)), (unsigned)ny), dim3(BLOCK), 0, st,
                       x, list, cnt, qpar, psum, pmax, N, own0, excl, ngroups, bpw, y0);
}

// the all-pairs sweep over chains whose np is a power of two (d == DMAX): one or two chains per lane (SWEEP_CPL).
// Workgroups of 512 / 1024 threads (fewer copies of a block's Gaussians staged through LDS) were measured on the
// two-chain kernels: C3 R-murray 39.2 ms with 256 threads, 40.0 with 512, 49.4 with 1024; the 32-D mixture 43.4 / 42.7
// / 42.7 -- the staging is not what a sweep waits for.
// Returns the number of entries per chain the sweep leaves in pmax for k_remote_cmax_combine (!SUMS): the blocks, or
// fewer where a wavefront carries its minimum through several of them.
template <int DM, bool SUMS>
static int launch_sweep_exact(const float *x, const int *list, int cnt, const float *qpar, float *psum, float *pmax,
                              int N, int own0, const unsigned long long *excl, int ngroups, int S, hipStream_t st)
{
  constexpr int CPL = SWEEP_CPL(DM);
  const SrowGrid g = srow_grid<DM, SUMS>(cnt, excl, ngroups, S);
  if (g.use) {
    launch_srow_range<DM, SUMS>(x, list, cnt, qpar, psum, pmax, N, own0, excl, ngroups, g.bpw, 0, g.gy, st);
    return SUMS ? S : g.gy;
  }
  hipLaunchKernelGGL((k_remote_sweep<DM, SUMS, true, CPL>), dim3(nblocks(((size_t)cnt + CPL - 1) / CPL), S), dim3(BLOCK), 0, st, x,
                     list, cnt, qpar, psum, pmax, DM, N, own0, excl, ngroups);
  return S;
}


constexpr int CULL_MIN_CHAINS = 4096, CULL_MIN_GAUSSIANS = 4096;
// the per-pair screen: any number of chains (a late rejection pass over a few hundred costs 60-160 us unscreened -- every
// one of them against every Gaussian, on a fraction of the chip -- and has 20-30 of them per job), sorted only where there
// are enough of them for neighbours to be near
constexpr int SCREEN_MIN_CHAINS = 1, SCREEN_SORT_MIN_CHAINS = 2048;

// Sort the active chains by their spatial key, box every group of CULL_W of them and test every (group, Q_i)
// pair (mcx_remote.hpp, "Exact exclusion of far Gaussians").  Leaves the sorted list in e->cull_sorted and the
// masks in e->cull_excl ([group][words]); the pairs kept are added to the device counter behind e->nact.
template <int DMAX>
static int cull_prepare(mcx_engine *e, const float *xrows, const int *ain, int nact, bool sums, int own0, hipStream_t st)
{
  const int d = e->nparam, N = e->tchains;
  const int ng = (nact + CULL_W - 1) / CULL_W, nw = (N + 63) / 64;
  // (the sums and the histogram are zero here: zeroed when allocated, and again by every k_cull_boxes)
  hipLaunchKernelGGL(k_cull_stats, dim3(nblocks((size_t)nact)), dim3(BLOCK), 0, st, xrows, ain, nact, d, e->cull_stats.p);
  hipLaunchKernelGGL(k_cull_keys, dim3(nblocks((size_t)nact)), dim3(BLOCK), 0, st, xrows, ain, nact, d, e->cull_stats.p,
                     e->cull_keys.p, e->cull_hist.p);
  hipLaunchKernelGGL(k_cull_scan, dim3(1), dim3(1024), 0, st, e->cull_hist.p);
  hipLaunchKernelGGL(k_cull_scatter, dim3(nblocks((size_t)nact)), dim3(BLOCK), 0, st, ain, e->cull_keys.p, nact, e->cull_hist.p,
                     e->cull_sorted.p);
  const dim3 gb((unsigned)((ng + BLOCK / 64 - 1) / (BLOCK / 64)));
  if (sums)
    hipLaunchKernelGGL((k_cull_boxes<DMAX, true>), gb, dim3(BLOCK), 0, st, xrows, (const int *)e->cull_sorted.p, nact,
                       (const float *)e->winvall.p, own0, e->cull_box.p, e->cull_lim.p, e->cull_stats.p, e->cull_hist.p);
  else
    hipLaunchKernelGGL((k_cull_boxes<DMAX, false>), gb, dim3(BLOCK), 0, st, xrows, (const int *)e->cull_sorted.p, nact,
                       (const float *)e->winvall.p, own0, e->cull_box.p, e->cull_lim.p, e->cull_stats.p, e->cull_hist.p);
  const int gchunk = 64;  // (every chunk re-reads the Gaussians' key dimensions: 74 us per 65 536 x 65 536 test with 16, 35 with 64)
  hipLaunchKernelGGL((k_cull_test<DMAX>), dim3((unsigned)((nw + BLOCK / 64 - 1) / (BLOCK / 64)), (unsigned)((ng + gchunk - 1) / gchunk)),
                     dim3(BLOCK), 0, st, (const float *)e->winvall.p, N, (const float *)e->cull_box.p, (const float *)e->cull_lim.p, ng, nact,
                     gchunk, e->cull_excl.p, nw, MurrayCounters::kept(e->nact.p, sums));
  HIPCHK(hipGetLastError());
  e->cnt.kernel_launches += 6;
  return MCX_OK;
}

// The same with the chains sorted along ONE direction and every (group, Q_i) row bounded by Cauchy-Schwarz along it
// (mcx_cull_proj.hpp): for chain clouds no box of a few coordinates separates.
template <int DMAX>
static int cull_prepare_proj(mcx_engine *e, const float *xrows, const int *ain, int nact, bool sums, int own0, hipStream_t st)
{
  const int N = e->tchains;
  const int ng = (nact + CULL_W - 1) / CULL_W, nw = (N + 63) / 64;
  double *acc0 = e->proj_acc.p, *acc1 = e->proj_acc.p + PROJ_ACC;
  // (acc0 and the histogram are zero here: zeroed when allocated, and again by every k_proj_groups; acc1 is zeroed now)
  HIPCHK(hipMemsetAsync(acc1, 0, PROJ_ACC * sizeof(double), st));
  hipLaunchKernelGGL((k_proj_moments<DMAX>), dim3(nblocks((size_t)nact)), dim3(BLOCK), 0, st, xrows, ain, nact, (const double *)acc0, 0, acc0);
  hipLaunchKernelGGL((k_proj_moments<DMAX>), dim3(nblocks((size_t)nact)), dim3(BLOCK), 0, st, xrows, ain, nact, (const double *)acc0, 1, acc1);
  hipLaunchKernelGGL((k_proj_keys<DMAX>), dim3(nblocks((size_t)nact)), dim3(BLOCK), 0, st, xrows, ain, nact, (const double *)acc1,
                     e->proj_p.p, e->cull_keys.p, e->cull_hist.p);
  hipLaunchKernelGGL(k_cull_scan, dim3(1), dim3(1024), 0, st, e->cull_hist.p);
  hipLaunchKernelGGL(k_cull_scatter, dim3(nblocks((size_t)nact)), dim3(BLOCK), 0, st, ain, e->cull_keys.p, nact, e->cull_hist.p,
                     e->cull_sorted.p);
  const dim3 gb((unsigned)((ng + BLOCK / 64 - 1) / (BLOCK / 64)));
  if (sums)
    hipLaunchKernelGGL((k_proj_groups<DMAX, true>), gb, dim3(BLOCK), 0, st, xrows, (const int *)e->cull_sorted.p, nact,
                       (const float *)e->winvall.p, own0, (const double *)e->proj_p.p, e->proj_lohi.p, e->cull_lim.p, acc0, e->cull_hist.p);
  else
    hipLaunchKernelGGL((k_proj_groups<DMAX, false>), gb, dim3(BLOCK), 0, st, xrows, (const int *)e->cull_sorted.p, nact,
                       (const float *)e->winvall.p, own0, (const double *)e->proj_p.p, e->proj_lohi.p, e->cull_lim.p, acc0, e->cull_hist.p);
  const int gchunk = 64;
  hipLaunchKernelGGL((k_proj_test<DMAX>), dim3((unsigned)((nw + BLOCK / 64 - 1) / (BLOCK / 64)), (unsigned)((ng + gchunk - 1) / gchunk)),
                     dim3(BLOCK), 0, st, (const float *)e->winvall.p, N, (const double *)acc1, (const double *)e->proj_lohi.p,
                     (const float *)e->cull_lim.p, ng, nact, gchunk, e->cull_excl.p, nw, MurrayCounters::kept(e->nact.p, sums));
  HIPCHK(hipGetLastError());
  e->cnt.kernel_launches += 8;
  return MCX_OK;
}

// What the per-pair screen's launches touch (mcx_screen.hpp): the engine's buffers in a genRemote call, local ones in
// mcx_debug_murray_screen.
struct ScreenView {
  const float *winv;        // the Gaussians as (mu, 1/sig2) pairs
  float *centre;            // their centre
  unsigned short *a, *b;    // A' per position of the chains' list, B' per Gaussian (bf16)
  float *stats;             // the sort's sums and the histogram: k_screen_prep_x leaves them zero for the next sort
  unsigned *hist;
  unsigned long long *excl, *nkept;  // the masks, and the cells that count the pairs they keep
};
static ScreenView screen_view(mcx_engine *e, bool sums)
{
  return {e->winvall.p, e->scr_centre.p, e->scr_a.p, e->scr_b.p, e->cull_stats.p, e->cull_hist.p, e->cull_excl.p,
          MurrayCounters::kept(e->nact.p, sums)};
}

// the Gaussians' side of the screen: their centre and B'.  Once per genRemote call.
template <int DMAX>
static void screen_launch_q(const ScreenView &v, int N, int d, hipStream_t st)
{
  const int nblk = (N + SCR_BLK - 1) / SCR_BLK;
  hipLaunchKernelGGL(k_screen_centre, dim3(1), dim3(1024), 0, st, v.winv, N, d, v.centre);
  hipLaunchKernelGGL((k_screen_prep_q<DMAX>), dim3(nblocks((size_t)nblk * SCR_BLK)), dim3(BLOCK), 0, st, v.winv, N, nblk * SCR_BLK,
                     (const float *)v.centre, v.b);
}

// the chains' side: A' of the nact chains in `order` (null = index order), in whole groups of CULL_W
template <int DMAX>
static void screen_launch_x(const ScreenView &v, const float *xrows, const int *order, int nact, bool sums, int own0, hipStream_t st)
{
  const int ng = (nact + CULL_W - 1) / CULL_W;
  const dim3 gp(nblocks((size_t)ng * CULL_W));
  if (sums)
    hipLaunchKernelGGL((k_screen_prep_x<DMAX, true>), gp, dim3(BLOCK), 0, st, xrows, order, nact, ng * CULL_W, v.winv, own0,
                       (const float *)v.centre, v.a, v.stats, v.hist);
  else
    hipLaunchKernelGGL((k_screen_prep_x<DMAX, false>), gp, dim3(BLOCK), 0, st, xrows, order, nact, ng * CULL_W, v.winv, own0,
                       (const float *)v.centre, v.a, v.stats, v.hist);
}

// the screen's matrix-core kernel over the Gaussians' blocks [blk0, blk1), `bchunk` of them per workgroup: as
// screen_prepare sizes it, kept for launching by column chunks
struct ScreenLaunch {
  int gx = 0, bchunk = 1, nblk = 0, nact = 0, N = 0, ng = 0, nw = 0;
};
static ScreenLaunch screen_launch_shape(int nact, int N, int bchunk)
{
  ScreenLaunch L;
  L.ng = (nact + CULL_W - 1) / CULL_W; L.nw = (N + 63) / 64; L.nblk = (N + SCR_BLK - 1) / SCR_BLK;
  L.gx = (L.ng + SCR_WAVES - 1) / SCR_WAVES; L.bchunk = bchunk; L.nact = nact; L.N = N;
  return L;
}

template <int DMAX>
static void screen_gemm_go(const ScreenView &v, const ScreenLaunch &L, int blk0, int blk1, hipStream_t st)
{
  hipLaunchKernelGGL((k_screen_gemm<DMAX>), dim3((unsigned)L.gx, (unsigned)((blk1 - blk0 + L.bchunk - 1) / L.bchunk)), dim3(SCR_WAVES * 64), 0, st,
                     (const unsigned short *)v.a, (const unsigned short *)v.b, L.nact, L.N, L.ng, L.bchunk, v.excl, L.nw, v.nkept, blk0, blk1);
}

// The same sort as cull_prepare's, then the per-pair bound on the matrix cores (mcx_screen.hpp) in place of the boxes.
// `fresh_q`: the Gaussians' side (centre, B') has not been built for this genRemote call yet.  *order_out: the list the
// masks' groups are cut from (the sorted list, or `ain` itself -- null = every chain in index order -- where nothing was
// sorted).  `defer`: the matrix-core kernel is not launched but described there, its grid sized for `chunks` column chunks.
template <int DMAX>
static int screen_prepare(mcx_engine *e, const float *xrows, const int *ain, int nact, bool sums, int own0, bool *fresh_q,
                          const int **order_out, hipStream_t st, bool may_sort = true, ScreenLaunch *defer = nullptr, int chunks = 1)
{
  const int d = e->nparam, N = e->tchains;
  const ScreenView v = screen_view(e, sums);
  if (*fresh_q) {
    screen_launch_q<DMAX>(v, N, d, st);
    e->cnt.kernel_launches += 2;
    *fresh_q = false;
  }
  const int *order = ain;  // (few chains: in the order they come)
  if (may_sort && nact >= SCREEN_SORT_MIN_CHAINS) {
    hipLaunchKernelGGL(k_cull_stats, dim3(nblocks((size_t)nact)), dim3(BLOCK), 0, st, xrows, ain, nact, d, e->cull_stats.p);
    hipLaunchKernelGGL(k_cull_keys, dim3(nblocks((size_t)nact)), dim3(BLOCK), 0, st, xrows, ain, nact, d, e->cull_stats.p,
                       e->cull_keys.p, e->cull_hist.p);
    hipLaunchKernelGGL(k_cull_scan, dim3(1), dim3(1024), 0, st, e->cull_hist.p);
    hipLaunchKernelGGL(k_cull_scatter, dim3(nblocks((size_t)nact)), dim3(BLOCK), 0, st, ain, e->cull_keys.p, nact, e->cull_hist.p,
                       e->cull_sorted.p);
    order = e->cull_sorted.p;
    e->cnt.kernel_launches += 4;
  }
  *order_out = order;
  screen_launch_x<DMAX>(v, xrows, order, nact, sums, own0, st);
  // The Gaussians' blocks are cut into chunks so that the grid is two chipfuls of workgroups (the kernel's own occupancy
  // x the CUs; one to four chipfuls, or 4096 workgroups whatever the chip holds: the same time within 2 %)
  constexpr int rounds = 2;
  static std::atomic<int> blocks_per_cu{0};  // (per instantiation; engines on several threads may ask at once: the same answer)
  int nb = blocks_per_cu.load(std::memory_order_relaxed);
  if (!nb) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_screen_gemm<DMAX>, SCR_WAVES * 64, 0) != hipSuccess || nb < 1) nb = 2;
    blocks_per_cu.store(nb, std::memory_order_relaxed);
  }
  const int resident = nb * (e->ncu > 0 ? e->ncu : 256);
  ScreenLaunch L = screen_launch_shape(nact, N, 1);
  const int per_launch = (L.nblk + chunks - 1) / chunks;  // (by column chunks: every chunk's grid is sized like a whole screen's)
  const int gy_want = std::max(1, (rounds * resident) / L.gx);
  L.bchunk = std::max(1, (per_launch + gy_want - 1) / gy_want);
  if (defer) {
    *defer = L;
    HIPCHK(hipGetLastError());
    return MCX_OK;
  }
  {
    ProfScope sg(e, MCX_K_REMOTE_SCREEN, (uint64_t)nact * (uint64_t)N);
    screen_gemm_go<DMAX>(v, L, 0, L.nblk, st);
  }
  HIPCHK(hipGetLastError());
  e->cnt.kernel_launches += 1;  // (+1: the screen's own scope)
  return MCX_OK;
}

// A pass over many chains with the per-pair screen, its Gaussians cut into `chunks` column chunks: chunk c + 1 is screened
// on the step stream (matrix cores) while chunk c is swept on a side stream (vector units) -- the two kernels alternated
// before, each leaving the other's pipe idle (screen 36 % + sweep 36 % of C3-murray's job).  Nothing about
// the sums changes: block partials are per block of QBLOCK Gaussians and combined in index order as ever.  *done stays false
// (nothing launched, or the preparation alone) where the pass does not cut evenly or is not the row-by-row kernel's.
constexpr int OVERLAP_MIN_CHAINS = 8192;
template <int DM, bool SUMS>
static int screen_sweep_chunked(mcx_engine *e, const float *xrows, const int *ain, int nact, int own0, bool *fresh_q, const int **order_out,
                                float *psum, float *pmax, int S, int chunks, int *entries_out, bool *done, hipStream_t st)
{
  *done = false;
  const int N = e->tchains, ng = (nact + CULL_W - 1) / CULL_W;
  const SrowGrid g = srow_grid<DM, SUMS>(nact, e->cull_excl.p, ng, S);
  if (!g.use) return MCX_OK;
  // a chunk = gy / chunks rows of the sweep's grid = bpw * QBLOCK Gaussians each = whole blocks of the screen
  static_assert(QBLOCK % SCR_BLK == 0, "a sweep block is a whole number of screen blocks");
  while (chunks > 1 && (g.gy % chunks != 0 || N % QBLOCK != 0)) chunks >>= 1;
  if (chunks < 2) return MCX_OK;
  const int ny = g.gy / chunks, blk_per = ny * g.bpw * (QBLOCK / SCR_BLK);
  ScreenLaunch L;
  MCXCHK((screen_prepare<DM>(e, xrows, ain, nact, SUMS, own0, fresh_q, order_out, st, true, &L, chunks)));
  const ScreenView v = screen_view(e, SUMS);
  MCXCHK(e->mstream.ensure(hipStreamNonBlocking));
  while ((int)e->mev.size() < chunks + 1) {
    DevEvent ev;
    MCXCHK(ev.ensure(hipEventDisableTiming));
    e->mev.push_back(std::move(ev));
  }
  {
    // (profile: the phase as a whole counts as the sweep -- the screen has no time of its own any more)
    ProfScope sw(e, MCX_K_REMOTE_SWEEP, (uint64_t)nact * (uint64_t)N);
    for (int c = 0; c < chunks; ++c) {
      const int b0 = c * blk_per, b1 = std::min(L.nblk, b0 + blk_per);
      screen_gemm_go<DM>(v, L, b0, b1, st);
      HIPCHK(hipEventRecord(e->mev[c], st));
      HIPCHK(hipStreamWaitEvent(e->mstream, e->mev[c], 0));
      launch_srow_range<DM, SUMS>(xrows, *order_out, nact, e->winvall.p, psum, pmax, N, own0, e->cull_excl.p, ng, g.bpw, c * ny, ny, e->mstream);
    }
    HIPCHK(hipEventRecord(e->mev[chunks], e->mstream));
    HIPCHK(hipStreamWaitEvent(st, e->mev[chunks], 0));
  }
  HIPCHK(hipGetLastError());
  e->cnt.kernel_launches += 2 * chunks - 1;
  *entries_out = SUMS ? S : g.gy;
  *done = true;
  return MCX_OK;
}

// ---------------------------------------------------------------------------------------------
// one genRemote call
// ---------------------------------------------------------------------------------------------
// auto mode gives a screen up where it excludes too little to pay for itself (the 32-D mixture: per-chain Gaussians too
// broad for any 128-chain box), per kind of sweep: within a call once a pass keeps more than this share of its pairs,
// and for the next seven calls (mcx_engine::cull_skip) where the call as a whole did -- it is tried again every eighth
constexpr double CULL_USELESS = 0.85;
constexpr int CULL_SKIP_CALLS = 7;

// what is fixed for one genRemote call, and its books
struct MurrayStep {
  mcx_engine *e;
  hipStream_t st;
  uint32_t t;
  int n, d, N, dm, S, own0;
  bool big;  // chain vector in registers up to np = 64, re-read from memory above
  // exclusion of far Gaussians: the two-chains-per-lane sweeps (np = 16, 32) over enough chains and Gaussians to
  // pay for the sort and the tests (or whenever possible: MCX_OPT_CULL = 1, for the tests)
  bool cull_can;
  // which exact screen: the per-pair bound (auto mode, 3), boxes of four coordinates (1), or -- on request only -- one
  // direction (2, mcx_cull_proj.hpp).  Measured in round 4: on C3's shape the direction keeps 0.58 of the pairs where the
  // boxes keep 0.41; on C5's mixture it keeps 0.999 like the boxes -- there a pair is dead because the chain is far from the
  // Gaussian in the 31 directions ACROSS the mixture's axis (the per-chain Gaussians are still narrow), which no bound for
  // 128 chains at once can see.
  bool gemm, proj;
  int overlap;  // column chunks of a big pass: the next chunk's screen beside this chunk's sweep (0 / 1: off)
  const float *pvals, *musigall;
  float *ptrial, *cfac, *mutrial, *sigtrial;
  // the books
  bool fresh_q = true;                       // the per-pair screen's Gaussian side is yet to be built
  bool cull_min = true, cull_sums = true;    // the min-arg sweep / the sum sweeps are (still) screened in this call
  uint64_t tested_min = 0, tested_sums = 0;  // pairs that went through a screen
  unsigned long long kept_min = 0, kept_sums = 0;  // and those it kept
  uint64_t evaluated_host = 0;               // pairs of the sweeps that ran without an exclusion test
  // the rejection passes' state: chains left, passes done, kernel turns done (a turn over candidates stands for
  // several passes), the active lists in turn
  int nact, pass = 0, it = 0;
  int *ain = nullptr, *aout;

  bool cull_now(int na) const
  {
    return cull_can && (e->opt_cull > 0 || (na >= (gemm ? SCREEN_MIN_CHAINS : CULL_MIN_CHAINS) && N >= CULL_MIN_GAUSSIANS));
  }
};

// the scratch buffers of the sweeps and the screens: sized on the first call, zeroed where a kernel expects zeros
static int murray_scratch(MurrayStep &c)
{
  mcx_engine *e = c.e;
  const int n = c.n, d = c.d, N = c.N, S = c.S;
  hipStream_t st = c.st;
  const size_t rows_max = std::max<size_t>((size_t)n, (size_t)MULTI_MAX_CHAINS * MULTI_K);  // chains, or candidates of few chains
  if (!c.big) {
    MCXCHK(e->psum.alloc(rows_max * S));
    MCXCHK(e->pmax.alloc(rows_max * S));
    MCXCHK(e->racpt.alloc((size_t)n));
    MCXCHK(e->cand.alloc((size_t)MULTI_MAX_CHAINS * MULTI_K * (3 * (size_t)d + 1)));
  }
  if (c.cull_can) {
    const size_t ngmax = (rows_max + CULL_W - 1) / CULL_W, nw = ((size_t)N + 63) / 64;
    const bool fresh = !e->cull_hist.p || !e->cull_stats.p;
    MCXCHK(e->cull_keys.alloc(rows_max)); MCXCHK(e->cull_hist.alloc(CULL_BINS)); MCXCHK(e->cull_sorted.alloc(rows_max));
    MCXCHK(e->cull_stats.alloc(2 * CULL_KD));
    if (fresh) {  // (k_cull_boxes leaves them zero for the next sort)
      HIPCHK(hipMemsetAsync(e->cull_stats.p, 0, 2 * CULL_KD * sizeof(float), st));
      HIPCHK(hipMemsetAsync(e->cull_hist.p, 0, CULL_BINS * sizeof(unsigned), st));
    }
    MCXCHK(e->cull_box.alloc(ngmax * 2 * CULL_KD)); MCXCHK(e->cull_lim.alloc(ngmax));
    MCXCHK(e->cull_excl.alloc(ngmax * nw));
    const bool fresh_p = !e->proj_acc.p;
    MCXCHK(e->proj_acc.alloc(2 * PROJ_ACC)); MCXCHK(e->proj_p.alloc(rows_max)); MCXCHK(e->proj_lohi.alloc(2 * ngmax));
    if (fresh_p) HIPCHK(hipMemsetAsync(e->proj_acc.p, 0, 2 * PROJ_ACC * sizeof(double), st));
    MCXCHK(e->scr_centre.alloc(64)); MCXCHK(e->scr_a.alloc(ngmax * CULL_W * scr_k(c.dm)));
    MCXCHK(e->scr_b.alloc((((size_t)N + SCR_BLK - 1) / SCR_BLK) * SCR_BLK * scr_k(c.dm)));
  }
  return MCX_OK;
}

// the call's start: the counter block's per-call part zeroed, and auto mode's skipped calls counted down
static int murray_open(MurrayStep &c)
{
  mcx_engine *e = c.e;
  HIPCHK(hipMemsetAsync(MurrayCounters::call_zero_from(e->nact.p), 0, MurrayCounters::CALL_ZERO_BYTES, c.st));
  if (e->opt_cull < 0) {
    if (e->cull_skip[0] > 0) { c.cull_min = false; e->cull_skip[0]--; }
    if (e->cull_skip[1] > 0) { c.cull_sums = false; e->cull_skip[1]--; }
  }
  return MCX_OK;
}

// what screen_pass leaves for the sweep behind it and for the kernels that read the sweep's results
struct Screened {
  const int *list;                 // the order of the chains in psum / pmax: the caller's list, or the screen's
  const unsigned long long *excl;  // the masks, or null: every pair is swept
  bool swept;                      // the sweep went out with the screen, by column chunks
  int entries;                     // entries per chain a min-arg sweep left for the combining kernel
};

template <int DM, bool SUMS>
static int screen_pass_dm(MurrayStep &c, const float *rows, const int *ain, int cnt, int own0, bool may_sort, Screened *r)
{
  mcx_engine *e = c.e;
  if (may_sort && c.gemm && c.overlap > 1 && cnt >= OVERLAP_MIN_CHAINS)
    MCXCHK((screen_sweep_chunked<DM, SUMS>(e, rows, ain, cnt, own0, &c.fresh_q, &r->list, SUMS ? e->psum.p : nullptr, e->pmax.p, c.S,
                                           c.overlap, &r->entries, &r->swept, c.st)));
  if (r->swept) return MCX_OK;
  // (boxes for the min-arg sweep and the per-pair bound for the sums only: C3-murray 18.1 -> 25.6 ms, C5 26.0 -> 38.8)
  if (c.gemm) return screen_prepare<DM>(e, rows, ain, cnt, SUMS, own0, &c.fresh_q, &r->list, c.st, may_sort);
  if (c.proj) return cull_prepare_proj<DM>(e, rows, ain, cnt, SUMS, own0, c.st);
  return cull_prepare<DM>(e, rows, ain, cnt, SUMS, own0, c.st);
}

// The screen of one sweep, where one applies: over the `cnt` chains of `ain` (null = all in index order) with rows `rows`,
// for the min-arg sweep (!SUMS; chain j's own Gaussian is own0 + j) or a sum sweep.  Chooses among the four kinds --
// per-pair bound by column chunks with the sweep beside it, per-pair bound, one direction, boxes -- and keeps the books
// of pairs tested / swept untested.  may_sort = false: the rows must keep their positions (candidates: a chain's four are
// a quad of lanes), which only the per-pair bound can do.
template <bool SUMS>
static int screen_pass(MurrayStep &c, const float *rows, const int *ain, int cnt, int own0, bool may_sort, Screened *r)
{
  *r = {ain, nullptr, false, c.S};
  const bool cull = (may_sort || c.gemm) && c.cull_now(cnt) && (SUMS ? c.cull_sums : c.cull_min);
  if (!cull) {
    c.evaluated_host += (uint64_t)cnt * (uint64_t)c.N;
    return MCX_OK;
  }
  if (!SUMS) c.tested_min = (uint64_t)cnt * (uint64_t)c.N;  // (the sums' share is known once the pass's counters are back: note_pass)
  r->list = c.e->cull_sorted.p;
  r->excl = c.e->cull_excl.p;
  // (cull_can: np = 16 or 32, the instantiations the screens have)
  return c.dm == 16 ? screen_pass_dm<16, SUMS>(c, rows, ain, cnt, own0, may_sort, r)
                    : screen_pass_dm<32, SUMS>(c, rows, ain, cnt, own0, may_sort, r);
}

// The all-pairs sweep behind screen_pass, unless that sent it out already: the kernels for np a power of two, or the
// generic one (unmasked: no screen runs there).  Returns in r->entries what launch_sweep_exact says.
template <bool SUMS>
static int sweep_pass(MurrayStep &c, const float *rows, int cnt, int own0, Screened *r)
{
  mcx_engine *e = c.e;
  if (r->swept) return MCX_OK;
  float *const psum = SUMS ? e->psum.p : nullptr;
  ProfScope sw(e, MCX_K_REMOTE_SWEEP, (uint64_t)cnt * (uint64_t)c.N);
  if (c.d == c.dm) {
    DISPATCH_DMAX(c.dm, (r->entries = launch_sweep_exact<DMAX_, SUMS>(rows, r->list, cnt, e->winvall.p, psum, e->pmax.p, c.N, own0, r->excl,
                                                                     (cnt + CULL_W - 1) / CULL_W, c.S, c.st)));
  } else {
    DISPATCH_DMAX(c.dm, hipLaunchKernelGGL((k_remote_sweep<DMAX_, SUMS, false>), dim3(nblocks((size_t)cnt), c.S), dim3(BLOCK), 0, c.st, rows,
                                           r->list, cnt, (const float *)e->winvall.p, psum, e->pmax.p, c.d, c.N, own0,
                                           (const unsigned long long *)nullptr, 0));
  }
  return MCX_OK;
}

// The Gaussians prepared as (mu, 1/sig2) pairs, then cmax[j] = max_i Q_i(pvals_j) as its exponent, cfac's numerator
// (src/mcpar.cc:412-437): for every chain, before the passes, since any of them may accept it
static int min_arg_sweep(MurrayStep &c)
{
  mcx_engine *e = c.e;
  const int n = c.n, d = c.d, N = c.N;
  hipStream_t st = c.st;
  hipLaunchKernelGGL(k_remote_prep, dim3(nblocks((size_t)N * d)), dim3(BLOCK), 0, st, c.musigall, e->winvall.p, (size_t)N * d, d, N,
                     MurrayCounters::nonfinite(e->nact.p));
  if (c.big) {
    hipLaunchKernelGGL(k_remote_cmax_big, dim3(nblocks((size_t)n)), dim3(BLOCK), 0, st, c.pvals, e->winvall.p, e->cmax.p, n, d, N);
    c.evaluated_host += (uint64_t)n * (uint64_t)N;
  } else {
    Screened r;
    MCXCHK(screen_pass<false>(c, c.pvals, nullptr, n, c.own0, true, &r));
    MCXCHK(sweep_pass<false>(c, c.pvals, n, c.own0, &r));
    hipLaunchKernelGGL(k_remote_cmax_combine, dim3(nblocks((size_t)n)), dim3(BLOCK), 0, st, e->pmax.p, e->cmax.p, n, r.entries, r.list);
  }
  HIPCHK(hipGetLastError());
  e->cnt.remote_pairs += (uint64_t)n * (uint64_t)N;
  return MCX_OK;
}

// the arguments of kernel turn c.it, which starts at pass c.pass of the reference, over the chains of c.ain
static RemoteArgs fill_remote_args(const MurrayStep &c, bool multi)
{
  const int it = c.it, pass = c.pass;
  mcx_engine *e = c.e;
  const int d = c.d;
  RemoteArgs a;
  // two survivor counters in turn: a pass counts in one and zeroes the other for the next pass (the first pass's
  // draw zeroes its own) -- no fill between the passes
  a.active_in = c.ain; a.nact = c.nact; a.active_out = c.aout; a.nact_out = MurrayCounters::survivors(e->nact.p, it);
  a.nact_zero = c.big ? nullptr : MurrayCounters::survivors(e->nact.p, it + 1);
  a.musigall = c.musigall; a.winv = e->winvall.p; a.cmax = e->cmax.p;
  a.ptrial = c.ptrial; a.mutrial = c.mutrial; a.sigtrial = c.sigtrial; a.cfac = c.cfac;
  a.racpt = e->racpt.p; a.psum = e->psum.p; a.pmax = e->pmax.p;
  a.n = c.n; a.d = d; a.N = c.N; a.pass = pass; a.S = c.S;
  a.g0 = (uint32_t)(e->rank * e->nchain); a.t = c.t; a.seed = e->seed;
  a.counts = MurrayCounters::words(e->nact.p);
  a.counts_host = c.big ? nullptr : e->h_nact.p;  // (np > 64: no k_remote_decide; pass_big's copy)
  a.done = MurrayCounters::done(e->nact.p);
  a.ncounts = multi ? MurrayCounters::WORDS : (c.cull_can ? MurrayCounters::WORDS_SCREENS : 1);
  a.nflag = MurrayCounters::W_SERIAL;  // (a word of its own whatever ncounts is: serial numbers only ever grow there)
  a.serial = ++e->remote_serial;
  a.nonfinite = it == 0 ? MurrayCounters::nonfinite(e->nact.p) : nullptr;  // (the call's first turn brings k_remote_prep's flag home)
  a.ncand = MULTI_K;
  a.cand_p = e->cand.p;
  a.cand_mu = a.cand_p + (size_t)MULTI_MAX_CHAINS * MULTI_K * d;
  a.cand_sig = a.cand_mu + (size_t)MULTI_MAX_CHAINS * MULTI_K * d;
  a.cand_racpt = a.cand_sig + (size_t)MULTI_MAX_CHAINS * MULTI_K * d;
  a.tried = MurrayCounters::tried(e->nact.p);
  return a;
}

// np > 64: draw, sweep and decision of a pass in one kernel, its survivor count by copy
static int pass_big(MurrayStep &c, RemoteArgs &a)
{
  mcx_engine *e = c.e;
  HIPCHK(hipMemsetAsync(a.nact_out, 0, sizeof(int), c.st));
  hipLaunchKernelGGL(k_remote_pass_big, dim3(nblocks((size_t)c.nact)), dim3(BLOCK), 0, c.st, a);
  HIPCHK(hipGetLastError());
  e->cnt.kernel_launches += 1;
  c.evaluated_host += (uint64_t)c.nact * (uint64_t)c.N;
  HIPCHK(hipMemcpyAsync(e->h_nact.p, e->nact.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, c.st));
  if (a.nonfinite)  // (the low half of a word whose high half is never written)
    HIPCHK(hipMemcpyAsync(e->h_nact.p + MurrayCounters::W_NONFINITE, a.nonfinite, sizeof(unsigned), hipMemcpyDeviceToHost, c.st));
  HIPCHK(hipStreamSynchronize(c.st));
  return MCX_OK;
}

// few chains left: their next MULTI_K proposals drawn, swept and decided together (see MULTI_K)
static int pass_multi(MurrayStep &c, RemoteArgs &a)
{
  mcx_engine *e = c.e;
  const int nv = c.nact * MULTI_K;
  hipLaunchKernelGGL(k_remote_draw_multi, dim3(nblocks((size_t)nv)), dim3(BLOCK), 0, c.st, a);
  Screened r;
  MCXCHK(screen_pass<true>(c, a.cand_p, nullptr, nv, -1, false, &r));
  MCXCHK(sweep_pass<true>(c, a.cand_p, nv, -1, &r));
  static_assert(MULTI_K == 4, "k_remote_decide_multi: a chain's candidates are a quad of lanes");
  hipLaunchKernelGGL(k_remote_decide_multi, dim3(nblocks((size_t)nv)), dim3(BLOCK), 0, c.st, a);
  HIPCHK(hipGetLastError());
  e->cnt.kernel_launches += 1;  // (the draw and the decision count as one, as they always have: the books are compared across versions)
  return MCX_OK;
}

// a pass of its own: the proposals of the still-rejected chains swept and decided
static int pass_plain(MurrayStep &c, RemoteArgs &a)
{
  mcx_engine *e = c.e;
  // (later passes: the k_remote_decide that rejected a chain has drawn its next proposal already)
  if (c.pass == 0) {
    DISPATCH_DMAX(c.dm, hipLaunchKernelGGL((k_remote_draw<DMAX_>), dim3(nblocks((size_t)c.nact)), dim3(BLOCK), 0, c.st, a));
    e->cnt.kernel_launches += 1;
  }
  Screened r;
  MCXCHK(screen_pass<true>(c, c.ptrial, c.ain, c.nact, -1, true, &r));  // the proposals have just been drawn: sort, bound and test them
  if (r.excl) a.active_in = r.list;  // positions of psum / pmax are positions of the screen's list
  MCXCHK(sweep_pass<true>(c, c.ptrial, c.nact, -1, &r));
  hipLaunchKernelGGL(k_remote_decide, dim3(nblocks((size_t)c.nact)), dim3(BLOCK), 0, c.st, a);
  HIPCHK(hipGetLastError());
  e->cnt.kernel_launches += 1;
  return MCX_OK;
}

// k_remote_decide's last workgroup writes the counters, then the pass's serial number: spinning on that word
// instead of a copy kernel and a wait for the stream (once per pass, 30-50 passes per job; against the copy and
// the wait on one box: C3-murray 16.2 -> 16.1 ms, C5 23.6 -> 23.4: the counters' way over PCIe is 6-11 us of the
// kernel now, what the copy kernel and its launch were) -- with a look at the stream now and then, so that a
// launch that failed or a device that is gone ends the wait
// The busy wait is BOUNDED: a short pass answers within tens of microseconds and is worth a core's
// attention; past SPIN_US the thread yields between looks (8 ranks + their MCout formatting threads + MPI progress
// on 16 cores: a spinning waiter must not hold a core from the work it waits for), and past YIELD_US it sleeps in
// hipStreamSynchronize like any other wait.
// (mcx_run.hip's report_arrived waits for a whole run's counters and never yields: a different policy on purpose.)
static int wait_pass_counters(volatile unsigned long long *flag, unsigned long long serial, hipStream_t st)
{
  constexpr long SPIN_US = 60, YIELD_US = 2000;
  const auto t_wait = std::chrono::steady_clock::now();
  bool polite = false;
  for (unsigned spins = 0; __atomic_load_n(const_cast<unsigned long long *>(flag), __ATOMIC_ACQUIRE) != serial; ++spins) {
    if (!polite) {
#if defined(__x86_64__) || defined(__i386__)
      __builtin_ia32_pause();  // (the sibling hyperthread gets the core's issue slots)
#endif
    } else {
      sched_yield();
    }
    if ((spins & 0xffu) == 0xffu || polite) {
      const long us = (long)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_wait).count();
      if (us > YIELD_US) break;  // (the blocking wait below)
      polite = us > SPIN_US;
    }
    if ((spins & 0xfffu) == 0xfffu) {
      const hipError_t q = hipStreamQuery(st);
      if (q == hipSuccess) break;  // the stream is empty: the word is there (or never will be: checked below)
      if (q != hipErrorNotReady) return fail(MCX_ERR_HIP, "Murray pass: %s", hipGetErrorString(q));
    }
  }
  if (__atomic_load_n(const_cast<unsigned long long *>(flag), __ATOMIC_ACQUIRE) != serial) {
    HIPCHK(hipStreamSynchronize(st));
    if (__atomic_load_n(const_cast<unsigned long long *>(flag), __ATOMIC_ACQUIRE) != serial)
      return fail(MCX_ERR_HIP, "Murray pass: the pass's counters did not arrive");
  }
  return MCX_OK;
}

// What the counter block `back` (MurrayCounters, host side) says after kernel turn `it` over nact_before chains against N
// Gaussians.  Pure host logic.
PassOutcome decode_pass(const unsigned long long *back, int it, bool multi, bool cull_can, int nact_before, int N)
{
  PassOutcome o = {0, 1, (unsigned long long)nact_before * (unsigned long long)N, 0, 0};
  const unsigned long long s = back[MurrayCounters::W_SURVIVORS];
  o.survivors = (int)(unsigned)((it & 1) ? s >> 32 : s & 0xffffffffull);
  if (multi) {
    // tried[c] chains came as far as candidate c: pass + c would have swept them.  Survivors tried them all.
    const unsigned *tried = MurrayCounters::tried(back);
    o.passes = 0;
    o.pairs = 0;
    for (int c = 0; c < MULTI_K; ++c)
      if (tried[c]) {
        o.passes = c + 1;
        o.pairs += (unsigned long long)tried[c] * (unsigned long long)N;
      }
    if (o.survivors > 0) o.passes = MULTI_K;
  }
  if (cull_can)
    for (int c = 0; c < CULL_NCOUNT; ++c) {
      o.kept_min += back[MurrayCounters::W_KEPT_MIN + c];
      o.kept_sums += back[MurrayCounters::W_KEPT_SUMS + c];
    }
  return o;
}

// the books after a kernel turn over `pairs_now` pairs, and the state of the next one
static void note_pass(MurrayStep &c, const PassOutcome &o, uint64_t pairs_now)
{
  mcx_engine *e = c.e;
  const unsigned long long before = c.kept_sums;
  e->cnt.remote_pairs += o.pairs;
  c.kept_min = o.kept_min; c.kept_sums = o.kept_sums;
  if (pairs_now && c.kept_sums > before) {  // this pass was tested
    c.tested_sums += pairs_now;
    if (e->opt_cull < 0 && (double)(c.kept_sums - before) > CULL_USELESS * (double)pairs_now) c.cull_sums = false;
  }
  c.nact = o.survivors;
  c.ain = c.aout;
  c.aout = (c.aout == e->active0.p) ? e->active1.p : e->active0.p;
  c.pass += o.passes;
  ++c.it;
}

// The call gives up ("Non-finite values"): nothing of it is left in flight, and the run it belongs to
// stops before this step.  `left` chains were still rejected after `passes` passes; `list`: their list on the device, if any.
static int murray_gave_up(MurrayStep &c, int left, int passes, const int *list)
{
  HIPCHK(hipStreamSynchronize(c.st));
  int j = -1;
  if (list && hipMemcpy(&j, list, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) j = -1;
  if (j >= 0)
    return fail(MCX_ERR_NONFINITE, "Murray step %u: %d chains still rejected after %d passes (MCX_OPT_MURRAY_MAX_PASSES), global chain %d among them",
                (unsigned)c.t, left, passes, c.own0 + j);
  return fail(MCX_ERR_NONFINITE, "Murray step %u: %d chains still rejected after %d passes (MCX_OPT_MURRAY_MAX_PASSES)", (unsigned)c.t, left, passes);
}

// the rejection passes (src/mcpar.cc:337-449): kernel turns until no chain is left -- or the call gives up: after its first
// turn when k_remote_prep found a NaN among the moments, and when chains are left after MCX_OPT_MURRAY_MAX_PASSES passes
static int murray_passes(MurrayStep &c)
{
  mcx_engine *e = c.e;
  if (!e->h_nact.p) {  // pinned and mapped: k_remote_decide writes the pass's counters and serial there
    MCXCHK(e->h_nact.alloc(MurrayCounters::HOST_WORDS));
    memset(e->h_nact.p, 0, MurrayCounters::HOST_WORDS * sizeof(unsigned long long));
  }
  const int maxp = e->opt_murray_max_passes;
  while (c.nact > 0) {
    if (c.pass >= maxp) return murray_gave_up(c, c.nact, c.pass, c.ain);
    const bool multi = !c.big && c.pass > 0 && c.nact <= MULTI_MAX_CHAINS;
    RemoteArgs a = fill_remote_args(c, multi);
    if (c.big) {
      MCXCHK(pass_big(c, a));
    } else {
      MCXCHK(multi ? pass_multi(c, a) : pass_plain(c, a));
      MCXCHK(wait_pass_counters(e->h_nact.p + a.nflag, a.serial, c.st));
    }
    if (c.it == 0) {
      const unsigned bad = (unsigned)__atomic_load_n(e->h_nact.p + MurrayCounters::W_NONFINITE, __ATOMIC_RELAXED);
      if (bad) {
        HIPCHK(hipStreamSynchronize(c.st));
        return fail(MCX_ERR_NONFINITE, "Murray step %u: the moments of global chain %d hold a NaN", (unsigned)c.t, c.N - (int)bad);
      }
    }
    // a turn over candidates stands for passes c.pass .. c.pass + MULTI_K - 1: chains that came as far as the candidate of
    // pass `maxp` were still rejected after maxp passes
    if (multi && maxp - c.pass < MULTI_K) {
      const unsigned beyond = MurrayCounters::tried(e->h_nact.p)[maxp - c.pass];
      if (beyond) return murray_gave_up(c, (int)beyond, maxp, nullptr);
    }
    const uint64_t pairs_now = (uint64_t)c.nact * (uint64_t)c.N * (multi ? MULTI_K : 1);
    note_pass(c, decode_pass(e->h_nact.p, c.it, multi, c.cull_can, c.nact, c.N), pairs_now);
  }
  return MCX_OK;
}

// the call's end: the pairs really evaluated, auto mode's verdict on either screen, sigtrial squared
static int murray_close(MurrayStep &c, int *npass_out)
{
  mcx_engine *e = c.e;
  e->cnt.remote_pairs_evaluated += c.evaluated_host + (uint64_t)c.kept_min + (uint64_t)c.kept_sums;
  if (e->opt_cull < 0) {
    if (c.tested_min && (double)c.kept_min > CULL_USELESS * (double)c.tested_min) e->cull_skip[0] = CULL_SKIP_CALLS;
    if (c.tested_sums && (double)c.kept_sums > CULL_USELESS * (double)c.tested_sums) e->cull_skip[1] = CULL_SKIP_CALLS;
  }
  hipLaunchKernelGGL(k_square, dim3(nblocks((size_t)e->ntot)), dim3(BLOCK), 0, c.st, c.sigtrial, (size_t)e->ntot);
  HIPCHK(hipGetLastError());
  if (npass_out) *npass_out = c.pass;
  return MCX_OK;
}

// MCPar::genRemote on device buffers (src/mcpar.cc:315-451)
int remote_device(mcx_engine *e, uint32_t t, const float *pvals, const float *musigall,
                         float *ptrial, float *cfac, float *mutrial, float *sigtrial, int *npass_out)
{
  MurrayStep c;
  c.e = e; c.st = e->stream; c.t = t;
  c.n = e->nchain; c.d = e->nparam; c.N = e->tchains;
  c.big = c.d > 64;
  c.dm = c.big ? 64 : dmax_for(c.d);
  c.S = (c.N + QBLOCK - 1) / QBLOCK;
  c.own0 = e->rank * e->nchain;
  if (!c.big && c.S > 65535)  // blocks of Gaussians go in gridDim.y
    return fail(MCX_ERR_UNSUPPORTED, "Murray proposals over %d chains in all: at most %d", c.N, 65535 * QBLOCK);
  c.cull_can = !c.big && c.d == c.dm && SWEEP_CPL(c.dm) == 2 && e->opt_cull != 0;
  c.gemm = e->opt_cull == 3 || e->opt_cull < 0;
  c.proj = e->opt_cull == 2;
  c.overlap = e->opt_murray_overlap;
  c.pvals = pvals; c.musigall = musigall;
  c.ptrial = ptrial; c.cfac = cfac; c.mutrial = mutrial; c.sigtrial = sigtrial;
  c.nact = c.n; c.aout = e->active0.p;
  ProfScope ps(e, MCX_K_REMOTE, (uint64_t)c.n);
  MCXCHK(murray_scratch(c));
  MCXCHK(murray_open(c));
  MCXCHK(min_arg_sweep(c));
  MCXCHK(murray_passes(c));
  return murray_close(c, npass_out);
}

extern "C" int mcx_debug_murray_decode(const unsigned long long *words, int nwords, int it, int multi, int cull_can,
                                       int nact_before, int N, unsigned long long *out5)
{
  if (!words || nwords < MurrayCounters::WORDS || it < 0 || nact_before < 0 || N < 0 || !out5) return fail(MCX_ERR_INVALID, "bad arguments");
  const PassOutcome o = decode_pass(words, it, multi != 0, cull_can != 0, nact_before, N);
  out5[0] = (unsigned long long)o.survivors; out5[1] = (unsigned long long)o.passes; out5[2] = o.pairs;
  out5[3] = o.kept_min; out5[4] = o.kept_sums;
  return MCX_OK;
}

// The per-pair screen alone, for tests: masks[word][group] (mcx_screen.hpp's layout; group = 128 consecutive chains, in
// the order given) of nact chains against N Gaussians given as (mu, sig2) pairs.  The launches are screen_prepare's, over
// buffers of its own; one block of Gaussians per workgroup.
template <int DM>
static int debug_screen(int nact, int N, const float *x, const float *musig, int own0, bool sums, unsigned long long *masks)
{
  const int d = DM;
  const ScreenLaunch L = screen_launch_shape(nact, N, 1);
  const size_t K = (size_t)scr_k(d), nmask = (size_t)L.ng * L.nw;
  struct Bufs {
    DevBuf<float> dx, dms, q, centre, stats;
    DevBuf<unsigned> hist;
    DevBuf<unsigned short> A, B;
    DevBuf<unsigned long long> excl, kept;
  } b;
  MCXCHK(b.dx.alloc((size_t)nact * d)); MCXCHK(b.dms.alloc((size_t)N * d * 2)); MCXCHK(b.q.alloc((size_t)N * d * 2));
  MCXCHK(b.centre.alloc(64)); MCXCHK(b.stats.alloc(2 * CULL_KD)); MCXCHK(b.hist.alloc(CULL_BINS));
  MCXCHK(b.A.alloc((size_t)L.ng * CULL_W * K)); MCXCHK(b.B.alloc((size_t)L.nblk * SCR_BLK * K));
  MCXCHK(b.excl.alloc(nmask)); MCXCHK(b.kept.alloc(CULL_NCOUNT));
  HIPCHK(hipMemcpy(b.dx.p, x, (size_t)nact * d * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b.dms.p, musig, (size_t)N * d * 2 * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipMemset(b.kept.p, 0, CULL_NCOUNT * sizeof(unsigned long long)));
  HIPCHK(hipMemset(b.excl.p, 0, nmask * sizeof(unsigned long long)));
  hipStream_t st = nullptr;
  const ScreenView v = {b.q.p, b.centre.p, b.A.p, b.B.p, b.stats.p, b.hist.p, b.excl.p, b.kept.p};
  hipLaunchKernelGGL(k_remote_prep, dim3(nblocks((size_t)N * d)), dim3(BLOCK), 0, st, (const float *)b.dms.p, b.q.p, (size_t)N * d, d, N,
                     (unsigned *)nullptr);
  screen_launch_q<DM>(v, N, d, st);
  screen_launch_x<DM>(v, b.dx.p, nullptr, nact, sums, sums ? -1 : own0, st);
  screen_gemm_go<DM>(v, L, 0, L.nblk, st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(masks, b.excl.p, nmask * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return MCX_OK;
}

extern "C" int mcx_debug_murray_screen(int d, int nact, int N, const float *x, const float *musig, int own0, int sums,
                                       unsigned long long *masks)
{
  if ((d != 16 && d != 32) || nact < 1 || N < 1 || !x || !musig || !masks) return fail(MCX_ERR_INVALID, "mcx_debug_murray_screen: np = 16 or 32");
  if (!sums && (own0 < 0 || own0 + nact > N)) return fail(MCX_ERR_INVALID, "mcx_debug_murray_screen: own Gaussians outside the N");
  return d == 16 ? debug_screen<16>(nact, N, x, musig, own0, sums != 0, masks) : debug_screen<32>(nact, N, x, musig, own0, sums != 0, masks);
}
