// Host check of csrc/gn_index.h, the division-free index arithmetic of the GroupNorm kernels (tests/test_group_norm_index_cpu.py builds
// and runs it): every value the functions can return for the arguments the kernels pass, against the integer division they replace.
#include <cstdio>
#include "../edgestyle_amd/csrc/gn_index.h"

int main() {
  long long checked = 0, bad = 0;
  auto fail = [&](const char* what, int a, int d, int got, int want) {
    if (bad++ < 10) std::printf("%s: a = %d, d = %d: %d, a / d = %d\n", what, a, d, got, want);
  };
  // gn_div: every divisor a kernel can have (a channel, chunk or item count up to 8192) against every dividend below 2^14
  for (int d = 1; d <= 8192; ++d) {
    const float inv = 1.0f / (float)d;
    for (int a = 0; a < (1 << 14); ++a, ++checked)
      if (gn_div(a, d, inv) != a / d) fail("gn_div", a, d, gn_div(a, d, inv), a / d);
  }
  // ... and sparsely up to the 2^22 its comment proves
  for (int d = 1; d <= 8192; d += 7) {
    const float inv = 1.0f / (float)d;
    for (int a = (1 << 22) - 1; a >= 0; a -= 1021, ++checked)
      if (gn_div(a, d, inv) != a / d) fail("gn_div (large)", a, d, gn_div(a, d, inv), a / d);
  }
  // gn_chunk_groups: every 8-channel chunk of every C <= 2560 (a multiple of 8) for every group count 1 .. 32 that divides C
  for (int C = 8; C <= 2560; C += 8)
    for (int groups = 1; groups <= 32; ++groups) {
      if (C % groups) continue;
      const int cpg = C / groups;
      for (int c0 = 0; c0 < C; c0 += 8) {
        int lg[8];
        gn_chunk_groups(c0, cpg, lg);
        for (int e = 0; e < 8; ++e, ++checked)
          if (lg[e] != (c0 + e) / cpg) fail("gn_chunk_groups", c0 + e, cpg, lg[e], (c0 + e) / cpg);
      }
    }
  std::printf("checked %lld, bad %lld\n", checked, bad);
  return bad ? 1 : 0;
}
