// Index arithmetic of the GroupNorm kernels (norm.hip) without integer division, as functions a host program can compile too:
// tests/gn_index_check.cpp runs them against `/` over every argument the kernels can pass (tests/test_group_norm_index_cpu.py).
#pragma once

#if defined(__HIPCC__)
#define GN_HD __host__ __device__ __forceinline__
#else
#define GN_HD inline
#endif

// a / d for 0 <= a < 2^22 and 1 <= d, with inv = 1.0f / (float)d: (float)a is exact, inv and the product are each within 2^-24
// relative of their true values, so the product is within a * 2^-23 / d < 1/2 of a / d and its truncation is a / d or one off
// either way - the remainder test puts that right.  (The kernels pass a < 2^14: a thread, an LDS item or a channel index.)
GN_HD int gn_div(const int a, const int d, const float inv) {
  int q = (int)((float)a * inv);
  const int r = a - q * d;
  q += (r >= d) - (r < 0);
  return q;
}

// The group of each of the 8 consecutive channels c0 .. c0 + 7, cpg channels per group: lg[e] == (c0 + e) / cpg.  One reciprocal
// division for the first channel, then an index that steps whenever the channel crosses into the next group (cpg may be below 8).
GN_HD void gn_chunk_groups(const int c0, const int cpg, int lg[8]) {
  int g = gn_div(c0, cpg, 1.0f / (float)cpg);
  int r = c0 - g * cpg;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    lg[e] = g;
    if (++r == cpg) { r = 0; ++g; }
  }
}
