#!/bin/bash
# Tool-only builds of the 256 x 320 phase-interleaved tile (csrc/gemm_conv8p.hip): one library per "-D..." argument set,
#   bash tools/ab8p.sh v1 "-DES8P_SCHED=1"   -> edgestyle_amd/lib/ablate/libes_8p_v1.so
set -e
NAME=$1; shift
bash "$(dirname "$0")/build_variant.sh" 8p_$NAME gemm_conv8p.hip "$*"
