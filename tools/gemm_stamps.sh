#!/bin/bash
# Tool-only: gemm_conv.hip with in-kernel stamps (tools/gemm_stamps.py) -> edgestyle_amd/lib/ablate/libes_gemm_stamps.so
set -e
bash "$(dirname "$0")/build_variant.sh" gemm_stamps gemm_conv.hip -DES_STAMPS=1
