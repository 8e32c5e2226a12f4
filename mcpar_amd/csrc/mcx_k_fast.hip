// mcx_k_fast.hip -- instantiations of the hot-path kernel k_fused_fast<LPC, MAIN, LIK, ..., EMIT> (mcx_device.hpp)
#include "mcx_launch.hpp"

using namespace mcx;

// the sample rows' mode (EmitMode) is chosen here, per launch: burn-in and main segments without rows EMIT_NONE,
// rows every step EMIT_EVERY, thinned EMIT_THIN -- the only main-loop instances the engine can ask for
template <int LPC, int LIK>
static hipError_t go(bool main, const SegArgs &a, hipStream_t st, StepLedger *led)
{
  const dim3 grid((unsigned)(((size_t)a.n * LPC + BLOCK - 1) / BLOCK)), block(BLOCK);
  if (a.samp_x && a.d < 4 * LPC && !a.trash) return hipErrorInvalidValue;  // idle lanes store to a.trash
  if (!main) {
    MCX_STEP_NOTE(led, SF_FAST, LPC, 1, LIK, false, EMIT_NONE, false);
    hipLaunchKernelGGL((k_fused_fast<LPC, false, LIK, false, false, EMIT_NONE>), grid, block, 0, st, a);
  } else if (!a.samp_x) {
    MCX_STEP_NOTE(led, SF_FAST, LPC, 1, LIK, true, EMIT_NONE, false);
    hipLaunchKernelGGL((k_fused_fast<LPC, true, LIK, false, false, EMIT_NONE>), grid, block, 0, st, a);
  } else if (a.samp_stride <= 1) {
    MCX_STEP_NOTE(led, SF_FAST, LPC, 1, LIK, true, EMIT_EVERY, false);
    hipLaunchKernelGGL((k_fused_fast<LPC, true, LIK, false, false, EMIT_EVERY>), grid, block, 0, st, a);
  } else {
    MCX_STEP_NOTE(led, SF_FAST, LPC, 1, LIK, true, EMIT_THIN, false);
    hipLaunchKernelGGL((k_fused_fast<LPC, true, LIK, false, false, EMIT_THIN>), grid, block, 0, st, a);
  }
  return hipGetLastError();
}

template <int LPC>
static hipError_t by_lik(int lik, bool main, const SegArgs &a, hipStream_t st, StepLedger *led)
{
  switch (lik) {
  case LIK_ROSEN1: return go<LPC, LIK_ROSEN1>(main, a, st, led);
  case LIK_GAUSS: return go<LPC, LIK_GAUSS>(main, a, st, led);
  case LIK_MIX: return go<LPC, LIK_MIX>(main, a, st, led);
  case LIK_ROSEN2F: return go<LPC, LIK_ROSEN2F>(main, a, st, led);
  default: return hipErrorInvalidValue;
  }
}

hipError_t mcxk_launch_fast(int lpc, int lik, bool main, const SegArgs &a, hipStream_t st, StepLedger *led)
{
  switch (lpc) {
  case 1: return by_lik<1>(lik, main, a, st, led);
  case 2: return by_lik<2>(lik, main, a, st, led);
  case 4: return by_lik<4>(lik, main, a, st, led);
  case 8: return by_lik<8>(lik, main, a, st, led);
  default: return hipErrorInvalidValue;
  }
}
