// mcx_k_generic_main.hip -- instantiations of the generic fused kernel k_fused_steps<LPC, LIK, true>
// (mcx_device.hpp): any np <= 256, full covariance, accept-mask recording, every fusable likelihood
#include "mcx_launch.hpp"

using namespace mcx;

template <int LPC>
static hipError_t by_lik(int lik, const SegArgs &a, hipStream_t st, StepLedger *led)
{
  const dim3 grid((unsigned)(((size_t)a.n * LPC + BLOCK - 1) / BLOCK)), block(BLOCK);
  switch (lik) {
  case LIK_ROSEN1:
    MCX_STEP_NOTE(led, SF_GENERIC, LPC, 1, LIK_ROSEN1, true, EMIT_ANY, false);
    hipLaunchKernelGGL((k_fused_steps<LPC, LIK_ROSEN1, true>), grid, block, 0, st, a);
    break;
  case LIK_GAUSS:
    MCX_STEP_NOTE(led, SF_GENERIC, LPC, 1, LIK_GAUSS, true, EMIT_ANY, false);
    hipLaunchKernelGGL((k_fused_steps<LPC, LIK_GAUSS, true>), grid, block, 0, st, a);
    break;
  case LIK_MIX:
    MCX_STEP_NOTE(led, SF_GENERIC, LPC, 1, LIK_MIX, true, EMIT_ANY, false);
    hipLaunchKernelGGL((k_fused_steps<LPC, LIK_MIX, true>), grid, block, 0, st, a);
    break;
  case LIK_ROSEN2F:
    MCX_STEP_NOTE(led, SF_GENERIC, LPC, 1, LIK_ROSEN2F, true, EMIT_ANY, false);
    hipLaunchKernelGGL((k_fused_steps<LPC, LIK_ROSEN2F, true>), grid, block, 0, st, a);
    break;
  default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t mcxk_launch_generic_main(int lpc, int lik, const SegArgs &a, hipStream_t st, StepLedger *led)
{
  switch (lpc) {
  case 1: return by_lik<1>(lik, a, st, led);
  case 2: return by_lik<2>(lik, a, st, led);
  case 4: return by_lik<4>(lik, a, st, led);
  case 8: return by_lik<8>(lik, a, st, led);
  case 16: return by_lik<16>(lik, a, st, led);
  case 32: return by_lik<32>(lik, a, st, led);
  case 64: return by_lik<64>(lik, a, st, led);
  default: return hipErrorInvalidValue;
  }
}
