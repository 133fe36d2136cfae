// Pose rendering (gfx950) and the host logic around it: 18 body key points -> the pose condition image, which the reference draws on
// the host with controlnet_aux's draw_bodypose (cv2.ellipse2Poly + fillConvexPoly per limb, cv2.circle per point) after
// create_openpose's filters (extract_dataset.py:222-295).  The two detector networks are not restated; this is the deterministic half.
//
// Which pixels a shape covers is this library's own rule (include/edgestyle_hip.h states it in full): every shape is an ellipse in
// integers - a limb has semi-axes int(length / 2) + 1/2 along and 4 + 1/2 across, a point is the disc of radius 4 with its rim - whose
// axes are turned by a whole number of degrees through a 2^-30 fixed-point sine table, and the inside test runs in 64-bit integers.
// The truncated angle is found by exact integer comparisons against that table, the truncated half-length by an integer square
// root: no atan2, sqrt, sin or cos is evaluated, so es_pose_draw_host (the same __host__ __device__ code) and the kernel agree bit
// for bit.  The only floating-point steps are single IEEE double products, sums and one division by 2 of the widened fp32 inputs;
// the file is built with -ffp-contract=off so that none of them fuses.
//
// Kernel: one launch for the whole batch.  A workgroup of 256 threads owns a tile of 64 x 16 pixels of one image; its first 35 lanes
// derive the 17 limb and 18 point records of that image into LDS; every thread then walks the records in draw order (the last writer
// wins) for its four horizontally adjacent pixels and stores 12 bytes as three dwords.  A record whose bounding box misses the tile
// is skipped by a scalar branch (the box is read from LDS at one address for the whole wave and made uniform with readfirstlane).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../../include/edgestyle_hip.h"
#include "plan.h"

extern "C" void es_set_error(const char* msg);

namespace {

constexpr int kLimbs = 17, kPoints = 18, kRecords = kLimbs + kPoints;
constexpr int kStick = 4;                       // draw_bodypose's stickwidth, and the radius of its circles
constexpr double kCoordLimit = 65536.0;         // a key point further out than this many pixels is not drawn
constexpr int kTileW = 64, kTileH = 16;

struct Tables {
  int32_t sin_q[91];                            // round(sin(t degrees) * 2^30), t = 0 .. 90
  uint8_t limb[kLimbs][2];                      // controlnet_aux's limbSeq, 0-based
  uint8_t colour[kPoints][3];
};
// (a function-local constant aggregate: the host and the device build each get their own read-only copy of the same literals)
#define ES_POSE_TABLES                                                                                                                  \
  {{0, 18739379, 37473049, 56195305, 74900443, 93582766, 112236583, 130856211, 149435979, 167970228, 186453311, 204879599, 223243478,    \
    241539355, 259761657, 277904834, 295963357, 313931728, 331804471, 349576144, 367241333, 384794656, 402230767, 419544355, 436730145,  \
    453782903, 470697435, 487468587, 504091252, 520560366, 536870912, 553017922, 568996477, 584801711, 600428808, 615873009, 631129609,  \
    646193961, 661061475, 675727625, 690187940, 704438018, 718473518, 732290163, 745883746, 759250125, 772385229, 785285058, 797945680,  \
    810363241, 822533958, 834454122, 846120104, 857528349, 868675383, 879557810, 890172315, 900515665, 910584710, 920376381, 929887697,  \
    939115760, 948057759, 956710970, 965072759, 973140576, 980911966, 988384560, 995556083, 1002424350, 1008987269, 1015242840,          \
    1021189159, 1026824413, 1032146887, 1037154959, 1041847103, 1046221891, 1050277989, 1054014162, 1057429273, 1060522280, 1063292242,  \
    1065738315, 1067859754, 1069655912, 1071126243, 1072270298, 1073087729, 1073578288, 1073741824},                                     \
   {{1, 2}, {1, 5}, {2, 3}, {3, 4}, {5, 6}, {6, 7}, {1, 8}, {8, 9}, {9, 10}, {1, 11}, {11, 12}, {12, 13}, {1, 0}, {0, 14}, {14, 16},     \
    {0, 15}, {15, 17}},                                                                                                                  \
   {{255, 0, 0}, {255, 85, 0}, {255, 170, 0}, {255, 255, 0}, {170, 255, 0}, {85, 255, 0}, {0, 255, 0}, {0, 255, 85}, {0, 255, 170},      \
    {0, 255, 255}, {0, 170, 255}, {0, 85, 255}, {0, 0, 255}, {85, 0, 255}, {170, 0, 255}, {255, 0, 255}, {255, 0, 170}, {255, 0, 85}}}

__host__ __device__ inline long long sin_q(const Tables& tb, int t) {        // t in [0, 360)
  if (t <= 90) return tb.sin_q[t];
  if (t <= 180) return tb.sin_q[180 - t];
  if (t <= 270) return -(long long)tb.sin_q[t - 180];
  return -(long long)tb.sin_q[360 - t];
}
__host__ __device__ inline long long cos_q(const Tables& tb, int t) { return sin_q(tb, t + 90 >= 360 ? t - 270 : t + 90); }

// One shape: the ellipse of semi-axes A / 2 along (c, s) and B / 2 across it, centred on pixel (cx, cy).  A == 0: nothing to draw.
// (hx, hy): half extents of a box around it, for skipping only - the inside test alone decides a pixel.
struct Rec { int32_t cx, cy, c, s, A, B, hx, hy; uint32_t rgb; };

__host__ __device__ inline bool present(const float* p, int H, int W) {      // NaN fails every comparison: absent
  return p[2] > 0.0f && fabs((double)p[0] * (double)W) < kCoordLimit && fabs((double)p[1] * (double)H) < kCoordLimit;
}

__host__ __device__ inline long long isqrt64(long long v) {                  // floor(sqrt(v)), v < 2^62
  long long r = 0;
  for (long long bit = 1ll << 60; bit; bit >>= 2) {
    if (v >= r + bit) { v -= r + bit; r = (r >> 1) + bit; }
    else r >>= 1;
  }
  return r;
}

__host__ __device__ inline void finish(Rec& r) {
  const long long ac = r.c < 0 ? -(long long)r.c : r.c, as = r.s < 0 ? -(long long)r.s : r.s;
  r.hx = (int32_t)((ac * r.A + as * r.B) >> 31) + 2;
  r.hy = (int32_t)((as * r.A + ac * r.B) >> 31) + 2;
}

// record `slot` of one pose (0 .. 16: the limbs, 17 .. 34: the points), kp = [18][3]
__host__ __device__ inline void derive(const float* kp, int H, int W, int slot, Rec& r) {
  const Tables tb = ES_POSE_TABLES;
  r = Rec{0, 0, 1 << 30, 0, 0, 0, 0, 0, 0};
  if (slot >= kLimbs) {
    const int i = slot - kLimbs;
    const float* p = kp + 3 * i;
    if (!present(p, H, W)) return;
    r.cx = (int32_t)((double)p[0] * (double)W);
    r.cy = (int32_t)((double)p[1] * (double)H);
    r.A = r.B = 2 * kStick;
    r.rgb = tb.colour[i][0] | tb.colour[i][1] << 8 | tb.colour[i][2] << 16;
    finish(r);
    return;
  }
  const float *p = kp + 3 * tb.limb[slot][0], *q = kp + 3 * tb.limb[slot][1];
  if (!present(p, H, W) || !present(q, H, W)) return;
  const double xp = (double)p[0] * (double)W, yp = (double)p[1] * (double)H, xq = (double)q[0] * (double)W, yq = (double)q[1] * (double)H;
  r.cx = (int32_t)((xp + xq) / 2.0);
  r.cy = (int32_t)((yp + yq) / 2.0);
  const long long qx = (long long)((xp - xq) * 256.0), qy = (long long)((yp - yq) * 256.0);      // 1/256 pixel, |.| < 2^25
  const int a = (int)(isqrt64(qx * qx + qy * qy) >> 9);                                           // int(length / 2)
  const long long ay = qy < 0 ? -qy : qy;
  int t = 0;                                    // int(degrees(atan2(|dy|, dx))): the last whole degree not past the limb's direction
  while (t < 180 && cos_q(tb, t + 1) * ay - sin_q(tb, t + 1) * qx >= 0) ++t;
  r.c = (int32_t)cos_q(tb, t);
  r.s = (int32_t)(qy < 0 ? -sin_q(tb, t) : sin_q(tb, t));                    // the angle -t: same cosine, the sine's sign turned
  r.A = 2 * a + 1;
  r.B = 2 * kStick + 1;
  const int i = slot;
  auto dim = [](int v) { return (uint32_t)(v == 255 ? 153 : v == 170 ? 102 : v == 85 ? 51 : 0); };   // int(v * 0.6)
  r.rgb = dim(tb.colour[i][0]) | dim(tb.colour[i][1]) << 8 | dim(tb.colour[i][2]) << 16;
  finish(r);
}

__host__ __device__ inline bool covers(int cx, int cy, long long c, long long s, long long A, long long B, int px, int py) {
  const long long u = px - cx, v = py - cy;
  long long al = (u * c + v * s + (1ll << 21)) >> 22;       // along and across the limb in 1/256 pixel (an arithmetic shift: floor)
  long long ac = (v * c - u * s + (1ll << 21)) >> 22;
  if (al < 0) al = -al;
  if (ac < 0) ac = -ac;
  if (al > 128 * A || ac > 128 * B) return false;           // (also what keeps the squares below inside 64 bits)
  return al * al * (B * B) + ac * ac * (A * A) <= 16384 * A * A * B * B;
}

__global__ __launch_bounds__(256) void pose_draw_kernel(const float* __restrict__ kp, uint8_t* __restrict__ out, int H, int W, int vec) {
  __shared__ Rec recs[kRecords];
  const int img = blockIdx.z;
  if (threadIdx.x < kRecords) derive(kp + (size_t)img * kPoints * 3, H, W, threadIdx.x, recs[threadIdx.x]);
  __syncthreads();
  const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
  const int px0 = tx0 + (threadIdx.x & 15) * 4, py = ty0 + (threadIdx.x >> 4);
  uint32_t col[4] = {0u, 0u, 0u, 0u};
  for (int i = 0; i < kRecords; ++i) {
    const int A = __builtin_amdgcn_readfirstlane(recs[i].A);
    if (A == 0) continue;
    const int cx = __builtin_amdgcn_readfirstlane(recs[i].cx), cy = __builtin_amdgcn_readfirstlane(recs[i].cy);
    const int hx = __builtin_amdgcn_readfirstlane(recs[i].hx), hy = __builtin_amdgcn_readfirstlane(recs[i].hy);
    if (cx + hx < tx0 || cx - hx >= tx0 + kTileW || cy + hy < ty0 || cy - hy >= ty0 + kTileH) continue;
    const int c = __builtin_amdgcn_readfirstlane(recs[i].c), s = __builtin_amdgcn_readfirstlane(recs[i].s);
    const int B = __builtin_amdgcn_readfirstlane(recs[i].B);
    const uint32_t rgb = (uint32_t)__builtin_amdgcn_readfirstlane((int)recs[i].rgb);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (covers(cx, cy, c, s, A, B, px0 + q, py)) col[q] = rgb;
  }
  if (py >= H || px0 >= W) return;
  uint8_t* dst = out + (((size_t)img * H + py) * W + px0) * 3;
  if (vec) {                                    // W % 4 == 0 and a 4-byte aligned canvas: the four pixels are whole and aligned
    uint32_t* d32 = (uint32_t*)dst;
    d32[0] = col[0] | col[1] << 24;
    d32[1] = col[1] >> 8 | col[2] << 16;
    d32[2] = col[2] >> 16 | col[3] << 8;
  } else {
    const int m = W - px0 < 4 ? W - px0 : 4;
    for (int q = 0; q < m; ++q) {
      dst[3 * q] = (uint8_t)col[q];
      dst[3 * q + 1] = (uint8_t)(col[q] >> 8);
      dst[3 * q + 2] = (uint8_t)(col[q] >> 16);
    }
  }
}

thread_local char g_msg[224];
int fail(const char* who, const char* what) {
  snprintf(g_msg, sizeof(g_msg), "%s: %s", who, what);
  es_set_error(g_msg);
  return -1;
}

int check_canvas(const char* who, const void* kp, const void* out, int count, int H, int W) {
  if (!kp || !out) return fail(who, "null pointer");
  if (count < 1) return fail(who, "count < 1");
  if (count > 65535) return fail(who, "count > 65535");
  if (H < 1 || W < 1) return fail(who, "height or width < 1");
  if (H > 16384 || W > 16384) return fail(who, "height or width > 16384");
  return 0;
}

inline bool has(const float* kp, int i) { return kp[3 * i + 2] > 0.0f; }

}  // namespace

extern "C" int es_pose_draw(const float* kp, uint8_t* out, int count, int H, int W, void* stream) {
  const char* who = "es_pose_draw";
  if (check_canvas(who, kp, out, count, H, W)) return -1;
  if (es_plan_recording()) return fail(who, "a plan is recording on this thread; the pose calls are never part of a plan");
  const int vec = W % 4 == 0 && (uintptr_t)out % 4 == 0;
  const dim3 grid((unsigned)((W + kTileW - 1) / kTileW), (unsigned)((H + kTileH - 1) / kTileH), (unsigned)count);
  hipLaunchKernelGGL(pose_draw_kernel, grid, dim3(256), 0, (hipStream_t)stream, kp, out, H, W, vec);
  if (hipGetLastError() != hipSuccess) { fail(who, "launch failed"); return -2; }
  return 0;
}

extern "C" int es_pose_draw_host(const float* kp, uint8_t* out, int count, int H, int W) {
  if (check_canvas("es_pose_draw_host", kp, out, count, H, W)) return -1;
  memset(out, 0, (size_t)count * H * W * 3);
  for (int n = 0; n < count; ++n) {
    uint8_t* img = out + (size_t)n * H * W * 3;
    for (int slot = 0; slot < kRecords; ++slot) {
      Rec r;
      derive(kp + (size_t)n * kPoints * 3, H, W, slot, r);
      if (r.A == 0) continue;
      const int y0 = r.cy - r.hy < 0 ? 0 : r.cy - r.hy, y1 = r.cy + r.hy > H - 1 ? H - 1 : r.cy + r.hy;
      const int x0 = r.cx - r.hx < 0 ? 0 : r.cx - r.hx, x1 = r.cx + r.hx > W - 1 ? W - 1 : r.cx + r.hx;
      for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x)
          if (covers(r.cx, r.cy, r.c, r.s, r.A, r.B, x, y)) {
            uint8_t* px = img + ((size_t)y * W + x) * 3;
            px[0] = (uint8_t)r.rgb; px[1] = (uint8_t)(r.rgb >> 8); px[2] = (uint8_t)(r.rgb >> 16);
          }
    }
  }
  return 0;
}

extern "C" int es_pose_select_host(const float* kps, const double* total_score, const double* total_parts, int n) {
  if (n < 0 || (n > 0 && (!kps || !total_score || !total_parts))) { fail("es_pose_select_host", "null pointer or n < 0"); return -2; }
  int best = -1;
  double best_area = 0.0;
  for (int i = 0; i < n; ++i) {
    const float* kp = kps + (size_t)i * kPoints * 3;
    if (!(total_score[i] > 10.0) || !(total_parts[i] > 5.0)) continue;
    if (!(has(kp, 0) || has(kp, 1) || has(kp, 14) || has(kp, 15) || has(kp, 16) || has(kp, 17))) continue;     // no head at all
    if (!(has(kp, 2) || has(kp, 5))) continue;                                                                     // no shoulder
    if (!(has(kp, 8) || has(kp, 11))) continue;                                                                    // no hip
    double x0 = 0, x1 = 0, y0 = 0, y1 = 0;       // compute_area: the box around the present points (there are some: the tests above)
    bool first = true;
    for (int k = 0; k < kPoints; ++k) {
      if (!has(kp, k)) continue;
      const double x = kp[3 * k], y = kp[3 * k + 1];
      if (first) { x0 = x1 = x; y0 = y1 = y; first = false; }
      else { x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1; y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1; }
    }
    const double area = (x1 - x0) * (y1 - y0);
    if (best < 0 || area > best_area) { best = i; best_area = area; }       // a stable descending sort's first: ties keep input order
  }
  return best;
}

extern "C" int es_pose_points_host(const float* kp, int W, int H, float* out) {
  if (!kp || !out) return fail("es_pose_points_host", "null pointer");
  if (H < 1 || W < 1) return fail("es_pose_points_host", "height or width < 1");
  int n = 0;
  for (int k = 0; k < kPoints; ++k) {
    if (!has(kp, k)) continue;
    out[2 * n] = (float)((double)kp[3 * k] * (double)W);
    out[2 * n + 1] = (float)((double)kp[3 * k + 1] * (double)H);
    ++n;
  }
  return n;
}
