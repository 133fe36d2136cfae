#!/bin/bash
# Builds ablated variants of the library (linear_xs.hip with XS_ABLATE=n, on top of the flags the product builds that file with) next to
# the product one -> edgestyle_amd/lib/ablate/libes_xs_<n>.so
set -e
for a in ${XS_VARIANTS:-0 1 2 4 8 16 32 3 7 35 39 63}; do
  bash "$(dirname "$0")/build_variant.sh" xs_$a linear_xs.hip -DXS_ABLATE=$a
done
