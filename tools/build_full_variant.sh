#!/bin/bash
# Tool-only: the WHOLE library rebuilt with extra compiler flags -> edgestyle_amd/lib/ablate/libes_<name>.so
#   bash tools/build_full_variant.sh <name> "<extra flags>" [sources (without .hip) to apply the flags to (default: all)]
set -e
name=$1; flags=$2; shift; shift
make -C "$(dirname "$0")/../edgestyle_amd/csrc" -j4 OUT=../lib/ablate/libes_${name}.so VARIANT_DIR=../lib/ablate/full_${name} ${1:+ONLY="$*"} EXTRA="$flags"
echo "built edgestyle_amd/lib/ablate/libes_${name}.so"
