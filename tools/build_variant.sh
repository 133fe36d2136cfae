#!/bin/bash
# Tool-only library variants: rebuild ONE source with extra flags (added to its product flags) and link it with the product objects.
#   bash tools/build_variant.sh <name> <source.hip> "<extra flags>"   -> edgestyle_amd/lib/ablate/libes_<name>.so
set -e
name=$1; src=$2; flags=$3
make -C "$(dirname "$0")/../edgestyle_amd/csrc" -j4 OUT=../lib/ablate/libes_${name}.so VARIANT_DIR=../lib/ablate/obj_${name} ONLY="$(basename $src .hip)" EXTRA="$flags"
echo "built edgestyle_amd/lib/ablate/libes_${name}.so"
