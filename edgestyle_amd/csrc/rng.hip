// Seeded normal noise at the edge of the C ABI (gfx950): the stream of torch's device generator, restated.
//
// Both of the reference's callers draw their initial latents from torch.Generator(device).manual_seed(42)
// (test_text2image_pretrained_openpose.py:274, app.py:119) and the VAE conditioning sample from the device's default generator
// (model/controllora.py:39).  That generator is Philox4x32-10, counter based: element `li` of a draw of `numel` floats is a pure
// function of (seed, offset, li) and of the launch shape torch would have chosen (ATen/native/hip/DistributionTemplates.h:
// calc_execution_policy + distribution_elementwise_grid_stride_kernel, unroll 4):
//   blocks = min(block_cap, ceil(numel / 256)), T = 256 * blocks threads, each with its own subsequence;
//   li -> iteration i = li / 4T, lane word ii = (li % 4T) / T, thread t = li % T;
//   value = component ii of the four normals of counter {offset / 4 + i, subsequence t}, key {seed lo, seed hi};
//   the draw moves the generator on by ((numel - 1) / 4T + 1) * 4.
// The four normals are two Box-Muller pairs (words x, y -> elements 0, 1; words z, w -> elements 2, 3), the transform the
// vendor's normal4 applies (rocrand_normal.h box_muller), restated here: nothing is included from or linked against a vendor
// math library.  The integer layer, the layout, the rounding and the scatter are written once (__host__ __device__) and shared
// by the kernel and es_randn_host.  The float step has a device and a host form, as the vendor header's has:
//   device: what torch's build of that header executes (read off the disassembly of its float normal kernel for gfx950): u and v
//           are single fused multiply-adds (written as __fmaf_rn here, no flag decides it), logf is v_log_f32 with its two-constant
//           ln 2 tail whose last step is a plain add, sqrtf is the correctly rounded form, __sinf / __cosf are the hardware's (what
//           __sincosf is), and sin * s, cos * s are plain products.  The file is built with -ffp-contract=off (csrc/Makefile): with
//           the library's -ffp-contract=fast the compiler fuses the last add of logf's tail into an FMA, and about one value in
//           seven moves by an ulp or two;
//   host:   separately rounded product and sum, libm's logf / sinf / cosf - what plain float arithmetic gives without an FMA
//           unit; within a few ulp of the device form, never bit-equal to it.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>

#include "../../include/edgestyle_hip.h"
#include "plan.h"

extern "C" void es_set_error(const char* msg);

namespace {

constexpr uint32_t kMulA = 0xD2511F53u, kMulB = 0xCD9E8D57u;      // Philox4x32 multipliers
constexpr uint32_t kWeylA = 0x9E3779B9u, kWeylB = 0xBB67AE85u;    // key schedule (golden ratio, sqrt(3) - 1)
constexpr float k2Pow32Inv = 2.3283064e-10f;                      // 2^-32
constexpr float k2Pow32Inv2Pi = 1.46291807e-09f;                  // 2 pi * 2^-32
constexpr int kThreads = 256;

struct U4 { uint32_t x, y, z, w; };

__host__ __device__ inline U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)kMulA * c.x, p1 = (uint64_t)kMulB * c.z;
    c = U4{(uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0};
    k0 += kWeylA;
    k1 += kWeylB;
  }
  return c;
}

// one Box-Muller pair from two 32-bit words (see the head of the file for the two forms)
__host__ __device__ inline void box_muller(uint32_t x, uint32_t y, float* a, float* b) {
#ifdef __HIP_DEVICE_COMPILE__
  const float u = __fmaf_rn((float)x, k2Pow32Inv, k2Pow32Inv);
  const float v = __fmaf_rn((float)y, k2Pow32Inv2Pi, k2Pow32Inv2Pi);
  const float s = sqrtf(-2.0f * logf(u));
  *a = __sinf(v) * s;
  *b = __cosf(v) * s;
#else
  volatile float px = (float)x * k2Pow32Inv, py = (float)y * k2Pow32Inv2Pi;     // volatile: a rounded product, then a rounded sum
  const float u = k2Pow32Inv + px;
  const float v = k2Pow32Inv2Pi + py;
  const float s = sqrtf(-2.0f * logf(u));
  *a = sinf(v) * s;
  *b = cosf(v) * s;
#endif
}

// round to the nearest fp16 value (ties to even, subnormals and overflow included) and widen again: torch's float -> half cast
__host__ __device__ inline float round_f16(float x) {
  union { float f; uint32_t u; } v;
  v.f = x;
  const uint32_t mag = v.u & 0x7fffffffu;
  if (mag > 0x7f800000u) return x;                                   // NaN (never drawn)
  if (mag < 0x38800000u) return rintf(x * 16777216.0f) * 5.9604644775390625e-08f;     // below 2^-14: multiples of 2^-24
  v.u += 0xfffu + ((v.u >> 13) & 1u);
  v.u &= 0xffffe000u;
  if ((v.u & 0x7fffffffu) >= 0x47800000u) v.u = (v.u & 0x80000000u) | 0x7f800000u;    // 65520 and above round to infinity
  return v.f;
}

__host__ __device__ inline float round_bf16(float x) {               // round to nearest even, as torch's float -> bfloat16 cast
  union { float f; uint32_t u; } v;
  v.f = x;
  if ((v.u & 0x7fffffffu) > 0x7f800000u) return x;                   // NaN (never drawn)
  v.u += 0x7fffu + ((v.u >> 16) & 1u);
  v.u &= 0xffff0000u;
  return v.f;
}

struct Draw {
  float* out;
  uint64_t seed, ctr0;             // ctr0 = offset / 4
  long long numel, T;              // T = 256 * blocks: torch's thread count, the stride between a counter's four elements
  long long C, HW, Cstride;        // C == 0: linear write; otherwise li over [N,C,HW] lands at [n, p, c] of [N,HW,Cstride]
  float scale;
  int round_dtype;
};

// torch's transform (z * std + mean with std 1, mean 0: a -0 becomes +0), its cast to the tensor's dtype, then the scale
__host__ __device__ inline float finish(float z, const Draw& d) {
  z = z + 0.0f;
  if (d.round_dtype == ES_F16) z = round_f16(z);
  else if (d.round_dtype == ES_BF16) z = round_bf16(z);
  return z * d.scale;
}

__host__ __device__ inline void put(const Draw& d, long long li, float z) {
  if (li >= d.numel) return;
  long long at = li;
  if (d.C) {
    const long long p = li % d.HW, nc = li / d.HW;
    const long long n = nc / d.C, c = nc - n * d.C;
    at = (n * d.HW + p) * d.Cstride + c;
  }
  d.out[at] = finish(z, d);
}

// counter g of the draw: iteration g / T, thread g % T; its four elements lie T apart
__host__ __device__ inline void draw_counter(const Draw& d, long long g) {
  const long long i = g / d.T, t = g - i * d.T;
  const long long li = i * 4 * d.T + t;
  if (li >= d.numel) return;
  const uint64_t ctr = d.ctr0 + (uint64_t)i;
  const U4 r = philox4x32_10(U4{(uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)t, (uint32_t)((uint64_t)t >> 32)},
                             (uint32_t)d.seed, (uint32_t)(d.seed >> 32));
  float z0, z1, z2, z3;
  box_muller(r.x, r.y, &z0, &z1);
  box_muller(r.z, r.w, &z2, &z3);
  put(d, li, z0);
  put(d, li + d.T, z1);
  put(d, li + 2 * d.T, z2);
  put(d, li + 3 * d.T, z3);
}

// One thread per counter: consecutive threads are consecutive subsequences, so each of a wave's four stores is one run of
// consecutive elements (linear write) or of consecutive pixels of one channel (permuted write).
__global__ __launch_bounds__(kThreads) void randn_kernel(const Draw d, long long counters) {
  const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (g < counters) draw_counter(d, g);
}

thread_local char g_msg[224];
int fail(const char* who, const char* what) {
  snprintf(g_msg, sizeof(g_msg), "%s: %s", who, what);
  es_set_error(g_msg);
  return -1;
}
const char* const kRecording = "a plan is recording on this thread; the noise calls are never part of a plan";

long long blocks_of(long long numel, long long cap) {
  const long long b = (numel + kThreads - 1) / kThreads;
  return b < cap ? b : cap;
}
long long advance_of(long long numel, long long blocks) { return ((numel - 1) / (4 * kThreads * blocks) + 1) * 4; }

int cap_of(const char* who, int device) {
  static int cached[64];           // 0 = not asked yet; a device's properties do not change
  if (device < 0 && hipGetDevice(&device) != hipSuccess) { fail(who, "no current HIP device"); return -2; }
  if (device < 64 && cached[device]) return cached[device];
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, device) != hipSuccess) { fail(who, "hipGetDeviceProperties failed (device)"); return -2; }
  const int cap = p.multiProcessorCount * (p.maxThreadsPerMultiProcessor / kThreads);
  if (cap < 1) { fail(who, "the device reports no block capacity"); return -2; }
  if (device < 64) cached[device] = cap;
  return cap;
}

// every check that needs no GPU; fills `w` (blocks still as given: 0 = derive)
int check_desc(const char* who, const float* out, const es_randn_desc* d, Draw& w) {
  if (!d) return fail(who, "null pointer (descriptor)");
  if (!out) return fail(who, "null pointer (out)");
  if (es_plan_recording()) return fail(who, kRecording);
  if (d->numel < 1) return fail(who, "numel < 1");
  if (d->blocks < 0) return fail(who, "blocks < 0");
  if (d->round_dtype != ES_F16 && d->round_dtype != ES_BF16 && d->round_dtype != ES_F32) return fail(who, "unknown round_dtype (ES_F32 | ES_F16 | ES_BF16)");
  if (d->offset % 4) return fail(who, "offset is not a multiple of 4");
  if (d->N || d->C || d->HW || d->Cstride) {
    if (d->N < 1 || d->C < 1 || d->HW < 1) return fail(who, "permutation: N, C and HW must all be >= 1 (or all four fields 0)");
    if (d->N > d->numel || d->C > d->numel / d->N || d->HW > d->numel || d->N * d->C * d->HW != d->numel) return fail(who, "permutation: N*C*HW != numel");
    if (d->Cstride < d->C) return fail(who, "permutation: Cstride < C");
  }
  w.out = const_cast<float*>(out);
  w.seed = d->seed; w.ctr0 = d->offset / 4;
  w.numel = d->numel; w.T = 0;
  w.C = d->C; w.HW = d->HW; w.Cstride = d->Cstride;
  w.scale = d->scale; w.round_dtype = d->round_dtype;
  return 0;
}

}  // namespace

// library-internal (plan.hip: es_ctx_draw_latents / es_ctx_draw_cond_noise): es_randn under the caller's name; *advance (may be
// null) = by how much the draw moves the generator's offset on
int es_randn_impl(const char* who, float* out, const es_randn_desc* d, void* stream, unsigned long long* advance) {
  Draw w;
  if (check_desc(who, out, d, w)) return -1;
  long long blocks = d->blocks;
  if (!blocks) {
    const int cap = cap_of(who, -1);
    if (cap < 0) return cap;
    blocks = blocks_of(d->numel, cap);
  }
  w.T = kThreads * blocks;
  const long long counters = ((d->numel - 1) / (4 * w.T) + 1) * w.T;
  if (counters / kThreads > 0x7fffffffll) return fail(who, "too many elements for one launch");
  hipLaunchKernelGGL(randn_kernel, dim3((unsigned)(counters / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, w, counters);
  if (hipGetLastError() != hipSuccess) { fail(who, "launch failed"); return -2; }
  if (advance) *advance = (unsigned long long)advance_of(d->numel, blocks);
  return 0;
}

extern "C" int es_randn(float* out, const es_randn_desc* d, void* stream) { return es_randn_impl("es_randn", out, d, stream, nullptr); }

extern "C" int es_randn_host(float* out, const es_randn_desc* d) {
  Draw w;
  if (check_desc("es_randn_host", out, d, w)) return -1;
  if (!d->blocks) return fail("es_randn_host", "blocks must be given (there is no device to derive it from)");
  w.T = (long long)kThreads * d->blocks;
  const long long counters = ((d->numel - 1) / (4 * w.T) + 1) * w.T;
  for (long long g = 0; g < counters; ++g) draw_counter(w, g);
  return 0;
}

extern "C" int es_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  if (!ctr || !key || !out) return fail("es_philox4x32_10", "null pointer");
  if (es_plan_recording()) return fail("es_philox4x32_10", kRecording);
  const U4 r = philox4x32_10(U4{ctr[0], ctr[1], ctr[2], ctr[3]}, key[0], key[1]);
  out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
  return 0;
}

extern "C" int es_philox_block_cap(int device) {
  if (es_plan_recording()) return fail("es_philox_block_cap", kRecording);
  if (device < 0) return fail("es_philox_block_cap", "device < 0");
  return cap_of("es_philox_block_cap", device);
}

extern "C" int es_philox_blocks(int64_t numel, int block_cap) {
  if (es_plan_recording()) return fail("es_philox_blocks", kRecording);
  if (numel < 1) return fail("es_philox_blocks", "numel < 1");
  if (block_cap < 1) return fail("es_philox_blocks", "block_cap < 1");
  return (int)blocks_of(numel, block_cap);
}

extern "C" int64_t es_philox_advance(int64_t numel, int blocks) {
  if (es_plan_recording()) return fail("es_philox_advance", kRecording);
  if (numel < 1) return fail("es_philox_advance", "numel < 1");
  if (blocks < 1) return fail("es_philox_advance", "blocks < 1");
  return advance_of(numel, blocks);
}
