#!/bin/bash
# Full-covariance kernels A/B on one box (tools/fullcov_probe.py, 65 536 chains, 500 + 1000 steps):
#   blocks per lane (MCX_OPT_BLOCKS_PER_LANE): 1 = k_fused_fast<LPC, .., FULL> (one block per lane; up to 16-D the lane's rows
#   of the factor in registers), 2 = k_fused_fastb<LPC/2, 2, .., FULL> (two mirrored blocks per lane: mcx_fastb.hpp), 0 = the
#   engine's choice.  (The fourth leg -- the factor in LDS at every size, as in rounds 2-4 -- went with its compile-time switch:
#   EXPERIMENTS.md keeps what it measured.)
# usage: tools/fullcov_ab.sh   (from the repository root)
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
for bpl in 0 1 2; do
  echo "== blocks per lane $bpl (0 = engine's choice)"
  MCX_PROBE_BPL=$bpl python3 $ROOT/tools/fullcov_probe.py 2>&1 | grep -E "again" 
done
