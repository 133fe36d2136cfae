#!/bin/bash
# Tool-only builds of attention.hip (static priority forms and ablations) -> edgestyle_amd/lib/ablate/libes_attn_<tag>.so
#   bash tools/attn_ablate.sh           (in the container; then on the GPU box: python tools/attn_ablate_run.py)
set -e
for v in ${ATTN_VARIANTS:-p0:-DATTN_PRIO=0 p3:-DATTN_PRIO=3}; do
  bash "$(dirname "$0")/build_variant.sh" attn_${v%%:*} attention.hip "${v#*:}"
done
ls -la "$(dirname "$0")"/../edgestyle_amd/lib/ablate/libes_attn_*.so
