// SAM prompt encoder and mask decoder pieces (gfx950): the kernels between es_sam_encode_u8's embedding and es_sam_compose's masks that
// are not a big GEMM.  Each is an entry point of its own (include/edgestyle_hip.h has the semantics):
//
//   es_sam_prompt_tokens      PromptEncoder._embed_points / _embed_boxes + the decoder's output tokens: the token matrix and query_pe
//   es_linear_tokens          act(x W^T + b) (+ residual) for at most 32 rows per sample: the token side of the TwoWayTransformer
//   es_sam_upscale_masks      MaskDecoder.output_upscaling behind its first transposed convolution + the hypernetwork product, one launch
//   es_sam_postprocess_masks  EfficientViTSam.postprocess_masks (two bilinear resamplings and the crop between them) + `> 0`, one launch
//   es_mask_bbox              getBox: the bounding box of a mask with a margin, as fp32 on the device - the box prompt of the next decode
//
// Nothing here uses a float atomic, allocates or reads back: results do not depend on the order of execution, image i of a batch equals the
// image alone bit for bit, and every call accepts a capturing stream.  None is ever part of a plan.
//
// es_linear_tokens streams the weights once per block of 8 rows and is bound by latency, not by arithmetic: 2048 x 256 weights are 1 MB, a
// sample has a handful of rows.  A wave takes 64 / L output columns at a time, L = min(64, largest power of two <= K / 8) lanes per column;
// a lane owns the 8-element chunks L apart of its column's weight row (one 16-byte load each), multiplies them with the same chunk of every
// row of x (a broadcast load: all columns of the wave read the same address) into one fp32 fma chain per row, and the L partial sums are
// folded by a butterfly.  The order of summation depends on K alone.  MFMA would pad 5-7 rows to 16 and still wait for the same bytes.
//
// es_sam_decoder (the end of this file) is the object that walks the TwoWayTransformer over these kernels and es_conv_gemm, es_attention,
// es_layer_norm and es_add in one arena; its image-side GEMMs take the tile the launch policy gives for ONE image (as sam.hip does).
//
// The three position / resampling functions are __host__ __device__ and have host twins (es_sam_prompt_tokens_host,
// es_sam_postprocess_masks_host, es_mask_bbox_host) that run THE SAME code on the CPU, for hosts that want to check an index without a GPU.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/edgestyle_hip.h"
#include "common.h"
#include "encoder.h"
#include "plan.h"

extern "C" void es_set_error(const char* msg);

namespace {

constexpr int kMaxSide = 4096, kMaxCount = 4096, kMaxTokens = 32, kMaxDim = 2048, kRowBlock = 8;

// ---- prompt tokens ------------------------------------------------------------------------------------------------------------------
struct PromptArgs {
  const float *gauss, *point_emb, *not_a_point, *iou_token, *mask_tokens, *points, *boxes;
  const int32_t* labels;
  void *tokens, *query_pe;
  double sx, sy;                     // apply_coords: new_w / old_w and new_h / old_h, formed in double on the host
  float frame;
  int32_t P, E, n_mask_tokens, T;
};

// PositionEmbeddingRandom._pe_encoding of one point in the prompt frame, value j of E: [sin | cos] of 2 pi ((2 c - 1) @ G)
__host__ __device__ inline float pe_value(const float* G, float x, float y, float frame, int j, int E) {
  const int h = E >> 1, jj = j < h ? j : j - h;
  float cx = (x + 0.5f) / frame, cy = (y + 0.5f) / frame;
  cx = 2.0f * cx - 1.0f;
  cy = 2.0f * cy - 1.0f;
  const float t = 6.283185307179586f * (cx * G[jj] + cy * G[h + jj]);
  return j < h ? sinf(t) : cosf(t);
}

// value j of sparse token t of one image: its points in order, then the box corners, or one padding point where there is no box
__host__ __device__ inline float sparse_value(const PromptArgs& a, const float* pts, const int32_t* labels, const float* box, int t, int j) {
  int label;
  float x = 0.f, y = 0.f;
  bool corner = false;
  if (t < a.P) {
    label = labels[t]; x = pts[2 * t]; y = pts[2 * t + 1];
  } else if (box) {
    const int c = t - a.P;
    label = 2 + c; x = box[2 * c]; y = box[2 * c + 1]; corner = true;
  } else {
    label = -1;
  }
  if (label == -1) return a.not_a_point[j];
  x = (float)((double)x * a.sx);
  y = (float)((double)y * a.sy);
  const float pe = pe_value(a.gauss, x, y, a.frame, j, a.E);
  if (corner || label == 0 || label == 1) return pe + a.point_emb[label * a.E + j];
  return pe;                                                               // a label the prompt encoder has no embedding for
}

__host__ __device__ inline float token_value(const PromptArgs& a, int img, int row, int j) {
  if (row == 0) return a.iou_token[j];
  if (row <= a.n_mask_tokens) return a.mask_tokens[(row - 1) * a.E + j];
  return sparse_value(a, a.points ? a.points + (size_t)img * a.P * 2 : nullptr, a.labels ? a.labels + (size_t)img * a.P : nullptr,
                      a.boxes ? a.boxes + (size_t)img * 4 : nullptr, row - 1 - a.n_mask_tokens, j);
}

// grid (rows, n), 256 threads over the E values of a token
template <typename T>
__global__ __launch_bounds__(256) void prompt_tokens_kernel(const PromptArgs a) {
  const int row = blockIdx.x, img = blockIdx.y, rows = 1 + a.n_mask_tokens + a.T;
  const size_t at = ((size_t)img * rows + row) * a.E;
  for (int j = threadIdx.x; j < a.E; j += 256) {
    const T v = from_f32<T>(token_value(a, img, row, j));
    ((T*)a.tokens)[at + j] = v;
    if (a.query_pe) ((T*)a.query_pe)[at + j] = v;
  }
}

// ---- linear over a few rows ---------------------------------------------------------------------------------------------------------
struct LinArgs {
  const void *x, *w, *residual;
  const float* bias;
  void* out;
  long long bsx, bsr, bso;
  int32_t rows, K, N, ldx, ldr, ldo, per_row, relu, lpc, lpc_log2;
};

// grid (ceil(N / (4 * 64 / lpc)), n, ceil(rows / 8)), 256 threads = 4 waves
template <typename T>
__global__ __launch_bounds__(256) void linear_tokens_kernel(const LinArgs a) {
  typedef typename Traits<T>::vec8 vec8;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane & (a.lpc - 1), cpw = 64 >> a.lpc_log2;
  const int col = (blockIdx.x * 4 + wave) * cpw + (lane >> a.lpc_log2);
  const int img = blockIdx.y, r0 = blockIdx.z * kRowBlock;
  const bool colok = col < a.N;
  const T* xb = (const T*)a.x + (size_t)img * a.bsx;
  const T* wb = (const T*)a.w;
  float acc[kRowBlock];
#pragma unroll
  for (int r = 0; r < kRowBlock; ++r) acc[r] = 0.f;
  for (int k = sub * 8; k < a.K; k += a.lpc * 8) {
    vec8 wv = {};
    if (!a.per_row && colok) wv = *(const vec8*)(wb + (size_t)col * a.K + k);
#pragma unroll
    for (int r = 0; r < kRowBlock; ++r) {
      if (r0 + r < a.rows) {                                               // uniform over the block
        if (a.per_row && colok) wv = *(const vec8*)(wb + ((size_t)(r0 + r) * a.N + col) * a.K + k);
        const vec8 xv = *(const vec8*)(xb + (size_t)(r0 + r) * a.ldx + k);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[r] = __builtin_fmaf(to_f32(wv[e]), to_f32(xv[e]), acc[r]);
      }
    }
  }
  for (int off = a.lpc >> 1; off >= 1; off >>= 1) {                        // every lane takes part: the guards sit on the memory accesses only
#pragma unroll
    for (int r = 0; r < kRowBlock; ++r) acc[r] += __shfl_xor(acc[r], off);
  }
  if (sub != 0 || !colok) return;
#pragma unroll
  for (int r = 0; r < kRowBlock; ++r) {
    const int row = r0 + r;
    if (row >= a.rows) break;
    float v = acc[r];
    if (a.bias) v += a.bias[(a.per_row ? (size_t)row * a.N : 0) + col];
    if (a.relu) v = fmaxf(v, 0.f);
    if (a.residual) v += to_f32(((const T*)a.residual)[(size_t)img * a.bsr + (size_t)row * a.ldr + col]);
    ((T*)a.out)[(size_t)img * a.bso + (size_t)row * a.ldo + col] = from_f32<T>(v);
  }
}

// ---- the fused upscaling tail -------------------------------------------------------------------------------------------------------
// One wave per 16 rows of ConvT1's GEMM output, a row = (source pixel, sub-pixel) with C1 = 32 KS channels.  The row's channels sit in
// the four lanes l, l ^ 16, l ^ 32, l ^ 48 exactly as the A operand of mfma_f32_16x16x32 wants them (lane l: row l & 15, k = 8 (l >> 4) + j),
// so LayerNorm (two passes, two butterfly steps each) and the erf-GELU run on the operand's own registers and it is rounded once.
// ConvT2 is 4 KS tiles of 16 columns, column = sub-pixel2 * C2 + c2; the accumulator (column on the lane, rows in the registers) takes
// the bias and the erf-GELU and is multiplied with the lane's hyper[m, c2] in fp32; four butterfly steps fold the 16 lanes of a group.
struct UpArgs {
  const void *g, *wp, *hyper;
  const float *ln_g, *ln_b, *bias2;
  float* out;
  long long bsh;
  int32_t Gh, Gw, M, ldh;
  float eps;
};

__device__ inline float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }

template <typename T, int KS>
__global__ __launch_bounds__(256) void upscale_kernel(const UpArgs a) {
  typedef typename Traits<T>::vec8 vec8;
  constexpr int C1 = 32 * KS;
  const int lane = threadIdx.x & 63, quad = lane >> 4, l15 = lane & 15;
  const int tile = blockIdx.x * 4 + (threadIdx.x >> 6), img = blockIdx.y;
  const int HW = a.Gh * a.Gw, rows_img = HW * 4;
  if (tile * 16 >= rows_img) return;                                       // the whole wave leaves
  int arow = tile * 16 + l15;
  if (arow > rows_img - 1) arow = rows_img - 1;                            // a ragged last tile reads its last row again and stores nothing for it
  const T* gp = (const T*)a.g + ((size_t)img * rows_img + arow) * C1 + 8 * quad;
  float x[KS][8];
  float sum = 0.f;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const vec8 v = *(const vec8*)(gp + 32 * s);
#pragma unroll
    for (int j = 0; j < 8; ++j) { x[s][j] = to_f32(v[j]); sum += x[s][j]; }
  }
  sum += __shfl_xor(sum, 16);
  sum += __shfl_xor(sum, 32);
  const float mean = sum * (1.0f / C1);
  float sq = 0.f;
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float d = x[s][j] - mean; sq = __builtin_fmaf(d, d, sq); }
  sq += __shfl_xor(sq, 16);
  sq += __shfl_xor(sq, 32);
  const float rstd = 1.0f / sqrtf(sq * (1.0f / C1) + a.eps);
  vec8 af[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = 32 * s + 8 * quad + j;
      af[s][j] = from_f32<T>(gelu_erf((x[s][j] - mean) * rstd * a.ln_g[c] + a.ln_b[c]));
    }
  float h[4][KS], b2[KS];
#pragma unroll
  for (int tt = 0; tt < KS; ++tt) {
    b2[tt] = a.bias2[tt * 16 + l15];
#pragma unroll
    for (int m = 0; m < 4; ++m)
      h[m][tt] = m < a.M ? to_f32(((const T*)a.hyper)[(size_t)img * a.bsh + (size_t)m * a.ldh + tt * 16 + l15]) : 0.f;
  }
  const T* wp = (const T*)a.wp + (size_t)lane * 8;
  const int W4 = 4 * a.Gw;
  const size_t plane = (size_t)16 * HW;
#pragma unroll
  for (int s2 = 0; s2 < 4; ++s2) {
    float part[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) part[m][r] = 0.f;
#pragma unroll
    for (int tt = 0; tt < KS; ++tt) {
      const int t = s2 * KS + tt;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s) acc = mfma16(af[s], *(const vec8*)(wp + (size_t)(t * KS + s) * 512), acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float u = gelu_erf(acc[r] + b2[tt]);
#pragma unroll
        for (int m = 0; m < 4; ++m) part[m][r] = __builtin_fmaf(u, h[m][tt], part[m][r]);
      }
    }
#pragma unroll
    for (int off = 1; off < 16; off <<= 1)
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[m][r] += __shfl_xor(part[m][r], off);
    if (l15 == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = tile * 16 + quad * 4 + r;
        if (row < rows_img) {
          const int p = row >> 2, s = row & 3, py = p / a.Gw, px = p - py * a.Gw;
          const int Y = 4 * py + 2 * (s >> 1) + (s2 >> 1), X = 4 * px + 2 * (s & 1) + (s2 & 1);
#pragma unroll
          for (int m = 0; m < 4; ++m)
            if (m < a.M) a.out[((size_t)img * a.M + m) * plane + (size_t)Y * W4 + X] = part[m][r];
        }
      }
    }
  }
}

// ---- postprocess_masks --------------------------------------------------------------------------------------------------------------
struct Tap { int i0, i1; float w0, w1; };
// torch's upsample_bilinear2d source index for align_corners=False in fp32: scale = in / out, src = scale (dst + 0.5) - 0.5 clamped at 0
__host__ __device__ inline Tap tap_of(int dst, float scale, int in) {
  float s = scale * ((float)dst + 0.5f) - 0.5f;
  if (s < 0.f) s = 0.f;
  int i0 = (int)s;
  if (i0 > in - 1) i0 = in - 1;
  Tap t;
  t.i0 = i0;
  t.i1 = i0 + (i0 < in - 1 ? 1 : 0);
  t.w1 = s - (float)i0;
  t.w0 = 1.0f - t.w1;
  return t;
}
__host__ __device__ inline float blend(const Tap& a, const Tap& b, float v00, float v01, float v10, float v11) {
  return a.w0 * (b.w0 * v00 + b.w1 * v01) + a.w1 * (b.w0 * v10 + b.w1 * v11);
}
// pixel (cy, cx) of the S x S canvas: the first resampling, never stored
__host__ __device__ inline float canvas_at(const float* lg, int L, float s1, int cy, int cx) {
  const Tap a = tap_of(cy, s1, L), b = tap_of(cx, s1, L);
  return blend(a, b, lg[a.i0 * L + b.i0], lg[a.i0 * L + b.i1], lg[a.i1 * L + b.i0], lg[a.i1 * L + b.i1]);
}
// pixel (y, x) of the H x W result: the second resampling over the canvas' top left new_h x new_w pixels
__host__ __device__ inline float post_at(const float* lg, int L, int S, int new_h, int new_w, int H, int W, int y, int x) {
  const float s1 = (float)L / (float)S;
  const Tap a = tap_of(y, (float)new_h / (float)H, new_h), b = tap_of(x, (float)new_w / (float)W, new_w);
  return blend(a, b, canvas_at(lg, L, s1, a.i0, b.i0), canvas_at(lg, L, s1, a.i0, b.i1), canvas_at(lg, L, s1, a.i1, b.i0),
               canvas_at(lg, L, s1, a.i1, b.i1));
}

// grid (ceil(H W / 256), count)
__global__ __launch_bounds__(256) void postprocess_kernel(const float* __restrict__ logits, float* __restrict__ out_f32, uint8_t* __restrict__ out_u8,
                                                          int L, int S, int new_h, int new_w, int H, int W) {
  const size_t HW = (size_t)H * W, pix = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (pix >= HW) return;
  const int m = blockIdx.y, y = (int)(pix / W), x = (int)(pix - (size_t)y * W);
  const float v = post_at(logits + (size_t)m * L * L, L, S, new_h, new_w, H, W, y, x);
  if (out_f32) out_f32[m * HW + pix] = v;
  if (out_u8) out_u8[m * HW + pix] = v > 0.f ? 1 : 0;
}

// ---- getBox -------------------------------------------------------------------------------------------------------------------------
// the box buffer holds int32 {xmin, ymin, xmax, ymax} between the launches and fp32 after the last
__global__ void bbox_init_kernel(int32_t* b, int count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  b[4 * i] = INT_MAX; b[4 * i + 1] = INT_MAX; b[4 * i + 2] = -1; b[4 * i + 3] = -1;
}

constexpr int kBoxPixelsPerThread = 8;
// grid (ceil(H W / 2048), count): one integer atomic per wave and bound, only from waves that saw a true pixel
__global__ __launch_bounds__(256) void bbox_reduce_kernel(const uint8_t* __restrict__ masks, int32_t* __restrict__ b, int H, int W) {
  const size_t HW = (size_t)H * W;
  const uint8_t* m = masks + blockIdx.y * HW;
  int x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
  const size_t base = (size_t)blockIdx.x * 256 * kBoxPixelsPerThread;
  for (int i = 0; i < kBoxPixelsPerThread; ++i) {
    const size_t pix = base + (size_t)i * 256 + threadIdx.x;
    if (pix < HW && m[pix] != 0) {
      const int y = (int)(pix / W), x = (int)(pix - (size_t)y * W);
      x0 = min(x0, x); y0 = min(y0, y); x1 = max(x1, x); y1 = max(y1, y);
    }
  }
  for (int d = 32; d >= 1; d >>= 1) {
    x0 = min(x0, __shfl_xor(x0, d)); y0 = min(y0, __shfl_xor(y0, d));
    x1 = max(x1, __shfl_xor(x1, d)); y1 = max(y1, __shfl_xor(y1, d));
  }
  if ((threadIdx.x & 63) == 0 && x1 >= 0) {
    int32_t* o = b + 4 * blockIdx.y;
    atomicMin(o, x0); atomicMin(o + 1, y0); atomicMax(o + 2, x1); atomicMax(o + 3, y1);
  }
}

__host__ __device__ inline void box_of(int x0, int y0, int x1, int y1, int H, int W, int margin, float out[4]) {
  if (x1 < 0) { out[0] = out[1] = out[2] = out[3] = 0.f; return; }
  out[0] = (float)(x0 - margin > 0 ? x0 - margin : 0);
  out[1] = (float)(y0 - margin > 0 ? y0 - margin : 0);
  out[2] = (float)(x1 + margin < W ? x1 + margin : W);
  out[3] = (float)(y1 + margin < H ? y1 + margin : H);
}

__global__ void bbox_finish_kernel(int32_t* b, int count, int H, int W, int margin) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const int x0 = b[4 * i], y0 = b[4 * i + 1], x1 = b[4 * i + 2], y1 = b[4 * i + 3];
  float o[4];
  box_of(x0, y0, x1, y1, H, W, margin, o);
  float* f = (float*)b + 4 * i;
  f[0] = o[0]; f[1] = o[1]; f[2] = o[2]; f[3] = o[3];
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
thread_local char g_msg[224];
int fail(const char* who, const char* what) {
  snprintf(g_msg, sizeof(g_msg), "%s: %s", who, what);
  es_set_error(g_msg);
  return -1;
}
int launched(const char* who) {
  if (hipGetLastError() != hipSuccess) { fail(who, "launch failed"); return -2; }
  return 0;
}
const char* kNoPlan = "a plan is recording on this thread; the SAM decoder calls are never part of a plan";

// checks a prompt descriptor and fills the kernel's arguments; device: the storage dtype and the outputs are checked too
int prompt_args(const char* who, const es_sam_prompt_desc* d, bool device, PromptArgs* a) {
  if (!d) return fail(who, "null pointer (desc)");
  if (!d->gauss || !d->point_embeddings || !d->not_a_point || !d->iou_token || !d->mask_tokens) return fail(who, "null pointer (a weight)");
  if (d->n < 1 || d->n > kMaxCount) return fail(who, "n must be in 1..4096");
  if (d->embed_dim < 2 || d->embed_dim > kMaxDim || d->embed_dim % 2) return fail(who, "embed_dim must be even and in 2..2048");
  if (d->n_mask_tokens < 1 || d->n_mask_tokens > 8) return fail(who, "n_mask_tokens must be in 1..8");
  if (d->P < 0) return fail(who, "P < 0");
  if (d->P > 0 && (!d->points || !d->labels)) return fail(who, "null pointer (points or labels with P > 0)");
  if (d->P == 0 && !d->boxes) return fail(who, "no prompt: neither points nor a box");
  const int T = es_sam_prompt_token_count(d->P, d->boxes != nullptr);
  if (1 + d->n_mask_tokens + T > kMaxTokens) return fail(who, "more than 32 tokens");
  if (d->frame < 1 || d->orig_h < 1 || d->orig_w < 1) return fail(who, "frame, orig_h and orig_w must be >= 1");
  if (device && d->dtype != ES_F16 && d->dtype != ES_BF16) return fail(who, "dtype must be ES_F16 or ES_BF16");
  if (device && !d->tokens) return fail(who, "null pointer (tokens)");
  int32_t hw[2];
  es_sam_resize_shape(d->orig_h, d->orig_w, d->frame, hw);
  a->gauss = d->gauss; a->point_emb = d->point_embeddings; a->not_a_point = d->not_a_point; a->iou_token = d->iou_token;
  a->mask_tokens = d->mask_tokens; a->points = d->P > 0 ? d->points : nullptr; a->labels = d->P > 0 ? d->labels : nullptr; a->boxes = d->boxes;
  a->tokens = d->tokens; a->query_pe = d->query_pe;
  a->sx = (double)hw[1] / (double)d->orig_w;
  a->sy = (double)hw[0] / (double)d->orig_h;
  a->frame = (float)d->frame;
  a->P = d->P; a->E = d->embed_dim; a->n_mask_tokens = d->n_mask_tokens; a->T = T;
  return 0;
}

int check_post(const char* who, const float* logits, int count, int L, int S, int new_h, int new_w, int H, int W, const void* o1, const void* o2) {
  if (!logits) return fail(who, "null pointer (logits)");
  if (!o1 && !o2) return fail(who, "null pointer (both outputs)");
  if (count < 1 || count > kMaxCount) return fail(who, "count must be in 1..4096");
  if (L < 1 || L > kMaxSide || S < 1 || S > kMaxSide) return fail(who, "L and S must be in 1..4096");
  if (new_h < 1 || new_w < 1 || new_h > S || new_w > S) return fail(who, "new_h and new_w must be in 1..S");
  if (H < 1 || W < 1 || H > kMaxSide || W > kMaxSide) return fail(who, "H and W must be in 1..4096");
  return 0;
}

int check_bbox(const char* who, const void* masks, const void* boxes, int count, int H, int W, int margin) {
  if (!masks || !boxes) return fail(who, "null pointer");
  if (count < 1 || count > kMaxCount) return fail(who, "count must be in 1..4096");
  if (H < 1 || W < 1 || H > kMaxSide || W > kMaxSide) return fail(who, "H and W must be in 1..4096");
  if (margin < 0 || margin > kMaxSide) return fail(who, "margin must be in 0..4096");
  return 0;
}

}  // namespace

extern "C" int es_sam_prompt_token_count(int P, int has_box) {
  if (P < 0) return -1;
  return P + (has_box ? 2 : (P > 0 ? 1 : 0));
}

extern "C" int es_sam_prompt_tokens(const es_sam_prompt_desc* d, void* stream) {
  const char* who = "es_sam_prompt_tokens";
  PromptArgs a;
  if (prompt_args(who, d, true, &a)) return -1;
  if (es_plan_recording()) return fail(who, kNoPlan);
  const dim3 grid((unsigned)(1 + a.n_mask_tokens + a.T), (unsigned)d->n);
  if (d->dtype == ES_F16) hipLaunchKernelGGL(prompt_tokens_kernel<f16>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(prompt_tokens_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, a);
  return launched(who);
}

extern "C" int es_sam_prompt_tokens_host(const es_sam_prompt_desc* d, float* tokens_f32) {
  const char* who = "es_sam_prompt_tokens_host";
  PromptArgs a;
  if (prompt_args(who, d, false, &a)) return -1;
  if (!tokens_f32) return fail(who, "null pointer (tokens_f32)");
  const int rows = 1 + a.n_mask_tokens + a.T;
  for (int img = 0; img < d->n; ++img)
    for (int row = 0; row < rows; ++row)
      for (int j = 0; j < a.E; ++j) tokens_f32[((size_t)img * rows + row) * a.E + j] = token_value(a, img, row, j);
  return 0;
}

extern "C" int es_linear_tokens(const es_linear_tokens_desc* d, void* stream) {
  const char* who = "es_linear_tokens";
  if (!d) return fail(who, "null pointer (desc)");
  if (!d->x || !d->w || !d->out) return fail(who, "null pointer");
  if (d->dtype != ES_F16 && d->dtype != ES_BF16) return fail(who, "dtype must be ES_F16 or ES_BF16");
  if (d->n < 1 || d->n > kMaxCount) return fail(who, "n must be in 1..4096");
  if (d->rows < 1 || d->rows > kMaxTokens) return fail(who, "rows must be in 1..32");
  if (d->K < 8 || d->K > kMaxDim || d->K % 8) return fail(who, "K must be a multiple of 8 in 8..2048");
  if (d->N < 4 || d->N > kMaxDim || d->N % 4) return fail(who, "N must be a multiple of 4 in 4..2048");
  LinArgs a = {};
  a.x = d->x; a.w = d->w; a.bias = d->bias; a.residual = d->residual; a.out = d->out;
  a.rows = d->rows; a.K = d->K; a.N = d->N;
  a.ldx = d->ldx ? d->ldx : d->K; a.ldr = d->ldr ? d->ldr : d->N; a.ldo = d->ldo ? d->ldo : d->N;
  if (a.ldx < d->K || a.ldx % 8) return fail(who, "ldx must be a multiple of 8 and >= K");
  if (a.ldr < d->N || a.ldo < d->N) return fail(who, "ldr and ldo must be >= N");
  a.bsx = d->bsx ? d->bsx : (long long)d->rows * a.ldx;
  a.bsr = d->bsr ? d->bsr : (long long)d->rows * a.ldr;
  a.bso = d->bso ? d->bso : (long long)d->rows * a.ldo;
  if (a.bsx < 0 || a.bsr < 0 || a.bso < 0 || a.bsx % 8) return fail(who, "sample strides must be >= 0, that of x a multiple of 8");
  if (((uintptr_t)d->x | (uintptr_t)d->w) % 16) return fail(who, "x and w must be 16-byte aligned");
  if (es_plan_recording()) return fail(who, kNoPlan);
  a.per_row = d->per_row_weights ? 1 : 0;
  a.relu = d->relu ? 1 : 0;
  int lg = 0;
  while (lg < 6 && (2 << lg) <= d->K / 8) ++lg;
  a.lpc = 1 << lg; a.lpc_log2 = lg;
  const int cols_per_block = 4 * (64 >> lg);
  const dim3 grid((unsigned)((d->N + cols_per_block - 1) / cols_per_block), (unsigned)d->n, (unsigned)((d->rows + kRowBlock - 1) / kRowBlock));
  if (d->dtype == ES_F16) hipLaunchKernelGGL(linear_tokens_kernel<f16>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(linear_tokens_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, a);
  return launched(who);
}

extern "C" int es_sam_upscale_pack(const float* w, int C1, int dtype, void* out) {
  const char* who = "es_sam_upscale_pack";
  if (!w || !out) return fail(who, "null pointer");
  if (C1 != 32 && C1 != 64) return fail(who, "C1 must be 32 or 64");
  if (dtype != ES_F16 && dtype != ES_BF16) return fail(who, "dtype must be ES_F16 or ES_BF16");
  const int KS = C1 / 32, C2 = C1 / 2;
  for (int t = 0; t < 4 * KS; ++t)
    for (int s = 0; s < KS; ++s)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
          const int k = 32 * s + 8 * (lane >> 4) + j, col = 16 * t + (lane & 15), s2 = col / C2, c2 = col - s2 * C2;
          const float v = w[((size_t)k * C2 + c2) * 4 + s2];                // [C1, C2, 2, 2]: s2 = 2 dy + dx
          const size_t at = ((size_t)(t * KS + s) * 64 + lane) * 8 + j;
          if (dtype == ES_F16) ((f16*)out)[at] = (f16)v;
          else ((bf16*)out)[at] = (bf16)v;
        }
  return 0;
}

extern "C" int es_sam_upscale_masks(const es_sam_upscale_desc* d, void* stream) {
  const char* who = "es_sam_upscale_masks";
  if (!d) return fail(who, "null pointer (desc)");
  if (!d->g || !d->w_packed || !d->ln_gamma || !d->ln_beta || !d->bias2 || !d->hyper || !d->out) return fail(who, "null pointer");
  if (d->dtype != ES_F16 && d->dtype != ES_BF16) return fail(who, "dtype must be ES_F16 or ES_BF16");
  if (d->n < 1 || d->n > kMaxCount) return fail(who, "n must be in 1..4096");
  if (d->grid_h < 1 || d->grid_w < 1 || d->grid_h > 256 || d->grid_w > 256) return fail(who, "grid_h and grid_w must be in 1..256");
  if (d->C1 != 32 && d->C1 != 64) return fail(who, "C1 must be 32 or 64 (embed_dim 128 or 256)");
  if (d->M < 1 || d->M > 4) return fail(who, "M must be in 1..4");
  if (((uintptr_t)d->g | (uintptr_t)d->w_packed) % 16) return fail(who, "g and w_packed must be 16-byte aligned");
  UpArgs a = {};
  a.g = d->g; a.wp = d->w_packed; a.hyper = d->hyper; a.ln_g = d->ln_gamma; a.ln_b = d->ln_beta; a.bias2 = d->bias2; a.out = d->out;
  a.Gh = d->grid_h; a.Gw = d->grid_w; a.M = d->M; a.eps = d->ln_eps;
  a.ldh = d->ldh ? d->ldh : d->C1 / 2;
  a.bsh = d->bsh ? d->bsh : (long long)d->M * a.ldh;
  if (a.ldh < d->C1 / 2 || a.bsh < 0) return fail(who, "ldh must be >= C1 / 2 and bsh >= 0");
  if (es_plan_recording()) return fail(who, kNoPlan);
  const int tiles = (d->grid_h * d->grid_w * 4 + 15) / 16;
  const dim3 grid((unsigned)((tiles + 3) / 4), (unsigned)d->n);
  hipStream_t st = (hipStream_t)stream;
  if (d->dtype == ES_F16) {
    if (d->C1 == 64) hipLaunchKernelGGL((upscale_kernel<f16, 2>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((upscale_kernel<f16, 1>), grid, dim3(256), 0, st, a);
  } else {
    if (d->C1 == 64) hipLaunchKernelGGL((upscale_kernel<bf16, 2>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((upscale_kernel<bf16, 1>), grid, dim3(256), 0, st, a);
  }
  return launched(who);
}

extern "C" int es_sam_postprocess_masks(const float* logits, int count, int L, int S, int new_h, int new_w, int H, int W, float* out_f32,
                                        uint8_t* out_u8, void* stream) {
  const char* who = "es_sam_postprocess_masks";
  if (check_post(who, logits, count, L, S, new_h, new_w, H, W, out_f32, out_u8)) return -1;
  if (es_plan_recording()) return fail(who, kNoPlan);
  const dim3 grid((unsigned)(((size_t)H * W + 255) / 256), (unsigned)count);
  hipLaunchKernelGGL(postprocess_kernel, grid, dim3(256), 0, (hipStream_t)stream, logits, out_f32, out_u8, L, S, new_h, new_w, H, W);
  return launched(who);
}

extern "C" int es_sam_postprocess_masks_host(const float* logits, int count, int L, int S, int new_h, int new_w, int H, int W, float* out_f32,
                                             uint8_t* out_u8) {
  const char* who = "es_sam_postprocess_masks_host";
  if (check_post(who, logits, count, L, S, new_h, new_w, H, W, out_f32, out_u8)) return -1;
  for (int m = 0; m < count; ++m)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const float v = post_at(logits + (size_t)m * L * L, L, S, new_h, new_w, H, W, y, x);
        const size_t at = ((size_t)m * H + y) * W + x;
        if (out_f32) out_f32[at] = v;
        if (out_u8) out_u8[at] = v > 0.f ? 1 : 0;
      }
  return 0;
}

extern "C" int es_mask_bbox(const uint8_t* masks, float* boxes, int count, int H, int W, int margin, void* stream) {
  const char* who = "es_mask_bbox";
  if (check_bbox(who, masks, boxes, count, H, W, margin)) return -1;
  if ((uintptr_t)boxes % 4) return fail(who, "boxes must be 4-byte aligned");
  if (es_plan_recording()) return fail(who, kNoPlan);
  hipStream_t st = (hipStream_t)stream;
  const dim3 per_mask((unsigned)((count + 255) / 256));
  const size_t per_block = (size_t)256 * kBoxPixelsPerThread;
  hipLaunchKernelGGL(bbox_init_kernel, per_mask, dim3(256), 0, st, (int32_t*)boxes, count);
  if (launched(who)) return -2;
  hipLaunchKernelGGL(bbox_reduce_kernel, dim3((unsigned)(((size_t)H * W + per_block - 1) / per_block), (unsigned)count), dim3(256), 0, st, masks,
                     (int32_t*)boxes, H, W);
  if (launched(who)) return -2;
  hipLaunchKernelGGL(bbox_finish_kernel, per_mask, dim3(256), 0, st, (int32_t*)boxes, count, H, W, margin);
  return launched(who);
}

extern "C" int es_mask_bbox_host(const uint8_t* masks, float* boxes, int count, int H, int W, int margin) {
  const char* who = "es_mask_bbox_host";
  if (check_bbox(who, masks, boxes, count, H, W, margin)) return -1;
  for (int m = 0; m < count; ++m) {
    int x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x)
        if (masks[((size_t)m * H + y) * W + x]) {
          x0 = x < x0 ? x : x0; y0 = y < y0 ? y : y0; x1 = x > x1 ? x : x1; y1 = y > y1 ? y : y1;
        }
    box_of(x0, y0, x1, y1, H, W, margin, boxes + 4 * m);
  }
  return 0;
}


// =====================================================================================================================================
// es_sam_decoder: state dict -> one arena (weights, per-decoder constants, activations of max_n images) and the walk
// =====================================================================================================================================
namespace {

using es_enc::EncBuilder;
using es_enc::Lin;

struct TokLin { size_t w = 0, bias = 0; int N = 0, K = 0; };
// one Attention block: each projection lives on the token side (es_linear_tokens) or on the image side (es_conv_gemm)
struct Attn { TokLin tq, tk, tv, to; Lin iq, ik, iv, io; };
struct DecLayer { Attn self_attn, t2i, i2t; TokLin lin1, lin2; size_t ng[4], nb[4]; };

template <typename T>
__global__ void iou_out_kernel(const T* __restrict__ src, float* __restrict__ dst, int total, int nm, int r0, int M) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int img = i / M, m = i - img * M;
  dst[i] = to_f32(src[(size_t)img * nm + r0 + m]);
}

int dfail(int rc, const char* who, const std::string& what) { return es_enc::fail(rc, who, what); }

}  // namespace

struct es_sam_decoder {
  es_sam_decoder_config cfg;
  int dtype = ES_F16, max_n = 0, max_points = 0, device = -1, Ci = 0, Rmax = 0;
  size_t arena_bytes = 0, ws_bytes = 0, ws = 0;
  char* arena = nullptr;
  es_launch_knobs knobs;
  std::vector<DecLayer> layers;
  Attn final_attn;
  size_t nfg = 0, nfb = 0;
  std::vector<TokLin> hyper, iou;                     // hyper[k]: n_mask_tokens weight sets of layer k, [nm][N][K]
  Lin convt1;
  size_t up_w = 0, up_b = 0, up_g = 0, up_beta = 0;
  size_t gauss = 0, pemb = 0, nap = 0, iou_tok = 0, mask_tok = 0, key_pe = 0, dense = 0;      // constants
  size_t tok = 0, qpe = 0, Q = 0, TT = 0, QP = 0, PQ = 0, PK = 0, PV = 0, ATT = 0, HID = 0, HA = 0, HB = 0, HO = 0, IA = 0, IB = 0;      // token side
  size_t KEYS = 0, KEYS2 = 0, IK = 0, IPA = 0, IPB = 0, IATT = 0, LOW = 0;                                                         // image side
  std::vector<std::pair<const Lin*, bool>> img_lins;  // every image-side projection and whether it runs with a residual (workspace sizing)
};

namespace {

const char* const kAttnWidths = "8, 16, 24, 32, 40, 48, 64, 80, 128, 160, 512";
bool attn_width_ok(int d) {
  for (int w : {8, 16, 24, 32, 40, 48, 64, 80, 128, 160, 512}) if (d == w) return true;
  return false;
}

bool tok_lin(EncBuilder& b, const std::string& key, int N, int K, TokLin* o) {
  std::vector<float> w = b.get(key + ".weight", N, K);
  if (w.empty()) return false;
  std::vector<float> bias = b.get(key + ".bias", N);
  if (bias.empty()) return false;
  o->N = N; o->K = K;
  o->w = b.alloc((size_t)N * K * 2);
  uint16_t* d = (uint16_t*)b.staged(o->w, (size_t)N * K * 2);
  for (size_t i = 0; i < w.size(); ++i) d[i] = b.enc(w[i]);
  o->bias = b.upload_f32(std::move(bias));
  return true;
}
bool img_lin(EncBuilder& b, const std::string& key, int N, int K, Lin* o) {
  std::vector<float> w = b.get(key + ".weight", N, K);
  if (w.empty()) return false;
  std::vector<float> bias = b.get(key + ".bias", N);
  if (bias.empty()) return false;
  *o = b.pack(w, bias, N, K, nullptr, nullptr, 1.0);
  return true;
}
// sides: t | i for q, k, v, out; internal: the width between the projections
bool pack_attn(EncBuilder& b, const std::string& key, const char* sides, int E, int internal, Attn* a) {
  const char* names[4] = {"q_proj", "k_proj", "v_proj", "out_proj"};
  TokLin* t[4] = {&a->tq, &a->tk, &a->tv, &a->to};
  Lin* im[4] = {&a->iq, &a->ik, &a->iv, &a->io};
  for (int i = 0; i < 4; ++i) {
    const int N = i < 3 ? internal : E, K = i < 3 ? E : internal;
    const std::string k = key + "." + names[i];
    if (sides[i] == 't' ? !tok_lin(b, k, N, K, t[i]) : !img_lin(b, k, N, K, im[i])) return false;
  }
  return true;
}
bool ln_params(EncBuilder& b, const std::string& key, int C, size_t* g, size_t* beta) {
  std::vector<float> w = b.get(key + ".weight", C);
  if (w.empty()) return false;
  std::vector<float> bb = b.get(key + ".bias", C);
  if (bb.empty()) return false;
  *g = b.upload_f32(std::move(w)); *beta = b.upload_f32(std::move(bb));
  return true;
}

// an image-side projection over n images: the tile of ONE image's launch, whatever n is
int img_linear(const char* who, es_sam_decoder* e, const Lin& L, const void* x, void* out, const void* residual, int n, hipStream_t st) {
  const int HW = e->cfg.grid * e->cfg.grid;
  es_launch_choice ch;
  if (!es_enc::choose(e, L, HW, ES_ACT_NONE, 1.f, residual != nullptr, &ch)) return dfail(-1, who, std::string("the launch policy has no tile for a projection: ") + es_last_error());
  es_gemm_desc d = es_enc::gemm_desc(e, L, n * HW, ES_ACT_NONE, 1.f, ch);
  d.x = x; d.out = out; d.residual = residual;
  d.w = e->arena + L.w; d.bias = (const float*)(e->arena + L.bias);
  if (ch.splitk > 1) {
    if (es_conv_gemm_workspace_bytes(&d) > e->ws_bytes) return dfail(-1, who, "split-K workspace smaller than the launch needs");
    d.workspace = (float*)(e->arena + e->ws);
  }
  return es_conv_gemm(&d, st);
}

int tok_linear(es_sam_decoder* e, const TokLin& L, const void* x, long long bsx, void* out, const void* residual, int n, int rows, bool relu,
               void* stream, int per_row = 0, int first_set = 0) {
  es_linear_tokens_desc d;
  memset(&d, 0, sizeof(d));
  d.x = x; d.out = out; d.residual = residual;
  d.w = e->arena + L.w + (size_t)first_set * L.N * L.K * 2;
  d.bias = (const float*)(e->arena + L.bias) + (size_t)first_set * L.N;
  d.n = n; d.rows = rows; d.K = L.K; d.N = L.N; d.bsx = bsx; d.per_row_weights = per_row; d.relu = relu; d.dtype = e->dtype;
  return es_linear_tokens(&d, stream);
}

int attend(es_sam_decoder* e, const void* q, int Sq, const void* k, const void* v, int Skv, void* o, int width, int n, void* stream) {
  es_attn_desc a;
  memset(&a, 0, sizeof(a));
  a.q = q; a.k = k; a.v = v; a.o = o;
  a.N = n; a.heads = e->cfg.heads; a.Sq = Sq; a.Skv = Skv; a.d = width / e->cfg.heads;
  a.ldq = a.ldk = a.ldv = a.ldo = width;
  a.bsq = a.bso = (int64_t)Sq * width; a.bsk = a.bsv = (int64_t)Skv * width;
  a.scale = (float)(1.0 / sqrt((double)a.d)); a.dtype = e->dtype;
  return es_attention(&a, stream);
}

const char* const kDry = "this decoder is a dry build (es_sam_decoder_create device -1): it holds no device memory and cannot run";

#define ES_RC(call) do { if ((rc = (call))) return rc; } while (0)

// token-to-image attention block (a layer's or the final one): Q <- LN(Q + out(attn(Q + pe, keys + key_pe, keys))); IK is left = keys + key_pe
int token_to_image(const char* who, es_sam_decoder* e, const Attn& a, size_t g, size_t beta, int n, int R, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  char* A = e->arena;
  const int E = e->cfg.embed_dim, HW = e->cfg.grid * e->cfg.grid, Ci = e->Ci;
  int rc;
  ES_RC(es_add(A + e->Q, A + e->qpe, A + e->QP, (int64_t)n * R * E, e->dtype, stream));
  ES_RC(es_add(A + e->KEYS, A + e->key_pe, A + e->IK, (int64_t)n * HW * E, e->dtype, stream));
  ES_RC(tok_linear(e, a.tq, A + e->QP, 0, A + e->PQ, nullptr, n, R, false, stream));
  ES_RC(img_linear(who, e, a.ik, A + e->IK, A + e->IPA, nullptr, n, st));
  ES_RC(img_linear(who, e, a.iv, A + e->KEYS, A + e->IPB, nullptr, n, st));
  ES_RC(attend(e, A + e->PQ, R, A + e->IPA, A + e->IPB, HW, A + e->ATT, Ci, n, stream));
  ES_RC(tok_linear(e, a.to, A + e->ATT, 0, A + e->TT, A + e->Q, n, R, false, stream));
  return es_layer_norm(A + e->TT, A + e->Q, (const float*)(A + g), (const float*)(A + beta), n * R, E, e->cfg.ln_eps, e->dtype, stream);
}

int check_call(const char* who, es_sam_decoder* e, const float* emb, const es_sam_prompts* p, int n, const float* iou) {
  if (!e || !emb || !p || !iou) return dfail(-1, who, "null pointer");
  if (es_plan_recording()) return dfail(-1, who, kNoPlan);
  if (p->mask_input) return dfail(-1, who, "mask_input is not supported (the reference never passes one)");
  if (n < 1 || n > e->max_n) return dfail(-1, who, "n = " + std::to_string(n) + " is outside 1..max_n = " + std::to_string(e->max_n));
  if (p->P < 0 || p->P > e->max_points) return dfail(-1, who, "P = " + std::to_string(p->P) + " is outside 0..max_points = " + std::to_string(e->max_points));
  if (p->P > 0 && (!p->points || !p->labels)) return dfail(-1, who, "null pointer (points or labels with P > 0)");
  if (p->P == 0 && !p->boxes) return dfail(-1, who, "no prompt: neither points nor a box");
  if (p->orig_h < 1 || p->orig_w < 1 || p->orig_h > kMaxSide || p->orig_w > kMaxSide) return dfail(-1, who, "orig_h and orig_w must be in 1..4096");
  if (!e->arena) return dfail(-1, who, kDry);
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev != e->device) return dfail(-1, who, "the current device is not the one the decoder was built on");
  return 0;
}

int decode(const char* who, es_sam_decoder* e, const float* emb, const es_sam_prompts* p, int n, int multimask, float* low_res, float* iou,
           void* stream) {
  hipStream_t st = (hipStream_t)stream;
  char* A = e->arena;
  const es_sam_decoder_config& c = e->cfg;
  const int E = c.embed_dim, HW = c.grid * c.grid, Ci = e->Ci, nm = c.n_mask_tokens;
  const int R = 1 + nm + es_sam_prompt_token_count(p->P, p->boxes != nullptr);
  int rc;
  es_sam_prompt_desc pd;
  memset(&pd, 0, sizeof(pd));
  pd.gauss = (const float*)(A + e->gauss); pd.point_embeddings = (const float*)(A + e->pemb); pd.not_a_point = (const float*)(A + e->nap);
  pd.iou_token = (const float*)(A + e->iou_tok); pd.mask_tokens = (const float*)(A + e->mask_tok);
  pd.points = p->points; pd.labels = p->labels; pd.boxes = p->boxes; pd.tokens = A + e->Q; pd.query_pe = A + e->qpe;
  pd.n = n; pd.P = p->P; pd.embed_dim = E; pd.n_mask_tokens = nm; pd.frame = c.frame; pd.orig_h = p->orig_h; pd.orig_w = p->orig_w; pd.dtype = e->dtype;
  ES_RC(es_sam_prompt_tokens(&pd, stream));
  ES_RC(es_nchw_f32_to_nhwc(emb, A + e->KEYS2, n, E, HW, E, e->dtype, stream));
  ES_RC(es_add(A + e->KEYS2, A + e->dense, A + e->KEYS, (int64_t)n * HW * E, e->dtype, stream));
  for (size_t li = 0; li < e->layers.size(); ++li) {
    const DecLayer& L = e->layers[li];
    const Attn& s = L.self_attn;
    const void* qin = A + e->Q;
    if (li) {
      ES_RC(es_add(A + e->Q, A + e->qpe, A + e->QP, (int64_t)n * R * E, e->dtype, stream));
      qin = A + e->QP;
    }
    ES_RC(tok_linear(e, s.tq, qin, 0, A + e->PQ, nullptr, n, R, false, stream));
    ES_RC(tok_linear(e, s.tk, qin, 0, A + e->PK, nullptr, n, R, false, stream));
    ES_RC(tok_linear(e, s.tv, A + e->Q, 0, A + e->PV, nullptr, n, R, false, stream));
    ES_RC(attend(e, A + e->PQ, R, A + e->PK, A + e->PV, R, A + e->ATT, E, n, stream));
    ES_RC(tok_linear(e, s.to, A + e->ATT, 0, A + e->TT, li ? A + e->Q : nullptr, n, R, false, stream));
    ES_RC(es_layer_norm(A + e->TT, A + e->Q, (const float*)(A + L.ng[0]), (const float*)(A + L.nb[0]), n * R, E, c.ln_eps, e->dtype, stream));
    ES_RC(token_to_image(who, e, L.t2i, L.ng[1], L.nb[1], n, R, stream));
    ES_RC(tok_linear(e, L.lin1, A + e->Q, 0, A + e->HID, nullptr, n, R, true, stream));
    ES_RC(tok_linear(e, L.lin2, A + e->HID, 0, A + e->TT, A + e->Q, n, R, false, stream));
    ES_RC(es_layer_norm(A + e->TT, A + e->Q, (const float*)(A + L.ng[2]), (const float*)(A + L.nb[2]), n * R, E, c.ln_eps, e->dtype, stream));
    // image to token: q = keys + key_pe (IK still holds it: the keys have not changed since), k = queries + pe, v = queries
    const Attn& t = L.i2t;
    ES_RC(es_add(A + e->Q, A + e->qpe, A + e->QP, (int64_t)n * R * E, e->dtype, stream));
    ES_RC(img_linear(who, e, t.iq, A + e->IK, A + e->IPA, nullptr, n, st));
    ES_RC(tok_linear(e, t.tk, A + e->QP, 0, A + e->PK, nullptr, n, R, false, stream));
    ES_RC(tok_linear(e, t.tv, A + e->Q, 0, A + e->PV, nullptr, n, R, false, stream));
    ES_RC(attend(e, A + e->IPA, HW, A + e->PK, A + e->PV, R, A + e->IATT, Ci, n, stream));
    ES_RC(img_linear(who, e, t.io, A + e->IATT, A + e->KEYS2, A + e->KEYS, n, st));
    ES_RC(es_layer_norm(A + e->KEYS2, A + e->KEYS, (const float*)(A + L.ng[3]), (const float*)(A + L.nb[3]), n * HW, E, c.ln_eps, e->dtype, stream));
  }
  ES_RC(token_to_image(who, e, e->final_attn, e->nfg, e->nfb, n, R, stream));
  // heads: only the rows that are returned
  const int r0 = multimask ? 1 : 0, M = multimask ? nm - 1 : 1, C1 = E / 4;
  const char* x = A + e->Q + (size_t)(1 + r0) * E * 2;
  ES_RC(tok_linear(e, e->hyper[0], x, (long long)R * E, A + e->HA, nullptr, n, M, true, stream, 1, r0));
  ES_RC(tok_linear(e, e->hyper[1], A + e->HA, 0, A + e->HB, nullptr, n, M, true, stream, 1, r0));
  ES_RC(tok_linear(e, e->hyper[2], A + e->HB, 0, A + e->HO, nullptr, n, M, false, stream, 1, r0));
  const void* ix = A + e->Q;
  long long ibs = (long long)R * E;
  for (size_t k = 0; k < e->iou.size(); ++k) {
    void* io = A + (k & 1 ? e->IB : e->IA);
    ES_RC(tok_linear(e, e->iou[k], ix, ibs, io, nullptr, n, 1, k + 1 < e->iou.size(), stream));
    ix = io; ibs = 0;
  }
  const int total = n * M;
  if (e->dtype == ES_F16) hipLaunchKernelGGL(iou_out_kernel<f16>, dim3((total + 255) / 256), dim3(256), 0, st, (const f16*)ix, iou, total, nm, r0, M);
  else hipLaunchKernelGGL(iou_out_kernel<bf16>, dim3((total + 255) / 256), dim3(256), 0, st, (const bf16*)ix, iou, total, nm, r0, M);
  if (hipGetLastError() != hipSuccess) return dfail(-2, who, "launch failed");
  ES_RC(img_linear(who, e, e->convt1, A + e->KEYS, A + e->IK, nullptr, n, st));
  es_sam_upscale_desc u;
  memset(&u, 0, sizeof(u));
  u.g = A + e->IK; u.w_packed = A + e->up_w; u.ln_gamma = (const float*)(A + e->up_g); u.ln_beta = (const float*)(A + e->up_beta);
  u.bias2 = (const float*)(A + e->up_b); u.hyper = A + e->HO; u.out = low_res;
  u.n = n; u.grid_h = c.grid; u.grid_w = c.grid; u.C1 = C1; u.M = M; u.ln_eps = c.ln2d_eps; u.dtype = e->dtype;
  return es_sam_upscale_masks(&u, stream);
}

}  // namespace

extern "C" void es_sam_decoder_destroy(es_sam_decoder* e) {
  if (!e) return;
  if (e->arena) (void)hipFree(e->arena);
  delete e;
}

extern "C" size_t es_sam_decoder_arena_bytes(const es_sam_decoder* e) { return e ? e->arena_bytes : 0; }

extern "C" int es_sam_decoder_create(const es_state_dict* sd, const es_sam_decoder_config* cfg, int dtype, int max_n, int max_points, int device,
                                     es_sam_decoder** out) {
  const char* who = "es_sam_decoder_create";
  if (out) *out = nullptr;
  if (!sd || !cfg || !out) return dfail(-1, who, "null pointer");
  if (es_plan_recording()) return dfail(-1, who, kNoPlan);
  if (dtype != ES_F16 && dtype != ES_BF16) return dfail(-1, who, "dtype must be ES_F16 or ES_BF16");
  if (device < -1) return dfail(-1, who, "device must be >= 0, or -1 for a dry build");
  const int E = cfg->embed_dim, nm = cfg->n_mask_tokens, G = cfg->grid;
  if (E < 64 || E % 64) return dfail(-1, who, "embed_dim must be a multiple of 64");
  if (E != 128 && E != 256) return dfail(-1, who, "embed_dim must be 128 or 256 (es_sam_upscale_masks has 32 or 64 channels behind ConvT1)");
  if (cfg->heads < 1 || cfg->attn_downsample < 1 || E % cfg->heads || E % cfg->attn_downsample || (E / cfg->attn_downsample) % cfg->heads)
    return dfail(-1, who, "heads must divide embed_dim and embed_dim / attn_downsample");
  const int Ci = E / cfg->attn_downsample;
  if (!attn_width_ok(E / cfg->heads) || !attn_width_ok(Ci / cfg->heads))
    return dfail(-1, who, "head widths " + std::to_string(E / cfg->heads) + " and " + std::to_string(Ci / cfg->heads) + " must be among es_attention's (" + kAttnWidths + ")");
  if (Ci % 8) return dfail(-1, who, "embed_dim / attn_downsample must be a multiple of 8");
  if (cfg->mlp_dim < 8 || cfg->mlp_dim > kMaxDim || cfg->mlp_dim % 8) return dfail(-1, who, "mlp_dim must be a multiple of 8 in 8..2048");
  if (cfg->iou_hidden < 8 || cfg->iou_hidden > kMaxDim || cfg->iou_hidden % 8) return dfail(-1, who, "iou_hidden must be a multiple of 8 in 8..2048");
  if (cfg->depth < 1 || cfg->depth > 16 || cfg->iou_depth < 2 || cfg->iou_depth > 8) return dfail(-1, who, "depth must be in 1..16 and iou_depth in 2..8");
  if (nm != 4) return dfail(-1, who, "n_mask_tokens must be 4 (the IoU head's last layer is read as 4 columns)");
  if (G < 1 || G > 64) return dfail(-1, who, "grid must be in 1..64");
  if (cfg->frame < 1 || cfg->frame > kMaxSide) return dfail(-1, who, "frame must be in 1..4096");
  if (max_n < 1 || max_n > 64) return dfail(-1, who, "max_n must be in 1..64");
  if (max_points < 0) return dfail(-1, who, "max_points must be >= 0");
  const int Rmax = 1 + nm + max_points + 2;
  if (Rmax > kMaxTokens) return dfail(-1, who, "more than 32 tokens: 1 + n_mask_tokens + max_points + 2 = " + std::to_string(Rmax));
  if (!(cfg->ln_eps > 0.f) || !(cfg->ln2d_eps > 0.f)) return dfail(-1, who, "ln_eps and ln2d_eps must be positive");

  // the prefix in front of "prompt_encoder.": found from the one key every state dict has
  const std::string first = "prompt_encoder.pe_layer.positional_encoding_gaussian_matrix";
  std::string prefix;
  bool found = false;
  for (int i = 0; sd->tensors && i < sd->count && !found; ++i) {
    const std::string k = sd->tensors[i].key ? sd->tensors[i].key : "";
    if (k.size() >= first.size() && k.compare(k.size() - first.size(), first.size(), first) == 0) { prefix = k.substr(0, k.size() - first.size()); found = true; }
  }
  if (!found) return dfail(-1, who, "missing key '" + first + "'");
  EncBuilder b;
  b.dt = dtype;
  if (!b.init(sd, prefix.c_str())) return dfail(-1, who, b.err);
  std::unique_ptr<es_sam_decoder, void (*)(es_sam_decoder*)> e(new es_sam_decoder, es_sam_decoder_destroy);
  e->cfg = *cfg; e->dtype = dtype; e->max_n = max_n; e->max_points = max_points; e->device = device; e->Ci = Ci; e->Rmax = Rmax;
  es_enc::default_knobs(&e->knobs);

#define ES_GET(var, ...) std::vector<float> var = b.get(__VA_ARGS__); if (var.empty()) return dfail(-1, who, b.err)
#define ES_OK(call) do { if (!(call)) return dfail(-1, who, b.err); } while (0)
  const size_t HW = (size_t)G * G, N = (size_t)max_n;
  {
    ES_GET(gauss, first, 2, E / 2);
    // get_dense_pe, once: pe of the grid points ((j + 0.5) / grid, (i + 0.5) / grid), rounded to the storage dtype, for max_n images
    e->key_pe = b.alloc(N * HW * E * 2);
    uint16_t* kp = (uint16_t*)b.staged(e->key_pe, N * HW * E * 2);
    const int h = E / 2;
    for (int i = 0; i < G; ++i)
      for (int j = 0; j < G; ++j) {
        const float cx = 2.0f * (((float)j + 0.5f) / (float)G) - 1.0f, cy = 2.0f * (((float)i + 0.5f) / (float)G) - 1.0f;
        for (int k = 0; k < h; ++k) {
          const float t = 6.283185307179586f * (cx * gauss[k] + cy * gauss[h + k]);
          kp[((size_t)i * G + j) * E + k] = b.enc(sinf(t));
          kp[((size_t)i * G + j) * E + h + k] = b.enc(cosf(t));
        }
      }
    for (size_t r = 1; r < N; ++r) memcpy(kp + r * HW * E, kp, HW * E * 2);
    e->gauss = b.upload_f32(std::move(gauss));
    std::vector<float> pemb;
    for (int i = 0; i < 4; ++i) {
      ES_GET(pi, "prompt_encoder.point_embeddings." + std::to_string(i) + ".weight", 1, E);
      pemb.insert(pemb.end(), pi.begin(), pi.end());
    }
    e->pemb = b.upload_f32(std::move(pemb));
    ES_GET(nap, "prompt_encoder.not_a_point_embed.weight", 1, E);
    e->nap = b.upload_f32(std::move(nap));
    ES_GET(nomask, "prompt_encoder.no_mask_embed.weight", 1, E);
    e->dense = b.alloc(N * HW * E * 2);
    uint16_t* dn = (uint16_t*)b.staged(e->dense, N * HW * E * 2);
    for (size_t r = 0; r < N * HW; ++r)
      for (int k = 0; k < E; ++k) dn[r * E + k] = b.enc(nomask[k]);
    ES_GET(it, "mask_decoder.iou_token.weight", 1, E);
    e->iou_tok = b.upload_f32(std::move(it));
    ES_GET(mt, "mask_decoder.mask_tokens.weight", nm, E);
    e->mask_tok = b.upload_f32(std::move(mt));
  }
  const std::string T = "mask_decoder.transformer.";
  e->layers.resize(cfg->depth);
  for (int li = 0; li < cfg->depth; ++li) {
    const std::string p = T + "layers." + std::to_string(li) + ".";
    DecLayer& L = e->layers[li];
    ES_OK(pack_attn(b, p + "self_attn", "tttt", E, E, &L.self_attn));
    ES_OK(pack_attn(b, p + "cross_attn_token_to_image", "tiit", E, Ci, &L.t2i));
    ES_OK(pack_attn(b, p + "cross_attn_image_to_token", "itti", E, Ci, &L.i2t));
    ES_OK(tok_lin(b, p + "mlp.lin1", cfg->mlp_dim, E, &L.lin1));
    ES_OK(tok_lin(b, p + "mlp.lin2", E, cfg->mlp_dim, &L.lin2));
    for (int k = 0; k < 4; ++k) ES_OK(ln_params(b, p + "norm" + std::to_string(k + 1), E, &L.ng[k], &L.nb[k]));
  }
  ES_OK(pack_attn(b, T + "final_attn_token_to_image", "tiit", E, Ci, &e->final_attn));
  ES_OK(ln_params(b, T + "norm_final_attn", E, &e->nfg, &e->nfb));
  const int C1 = E / 4, C2 = E / 8;
  e->hyper.resize(3);
  for (int k = 0; k < 3; ++k) {                            // the nm MLPs' layer k as one [nm][N][K] block: es_linear_tokens per_row_weights
    const int Nk = k < 2 ? E : C2;
    TokLin& H = e->hyper[k];
    H.N = Nk; H.K = E;
    H.w = b.alloc((size_t)nm * Nk * E * 2);
    uint16_t* dw = (uint16_t*)b.staged(H.w, (size_t)nm * Nk * E * 2);
    std::vector<float> bias;
    for (int i = 0; i < nm; ++i) {
      const std::string key = "mask_decoder.output_hypernetworks_mlps." + std::to_string(i) + ".layers." + std::to_string(k);
      ES_GET(w, key + ".weight", Nk, E);
      ES_GET(bi, key + ".bias", Nk);
      for (size_t j = 0; j < w.size(); ++j) dw[(size_t)i * Nk * E + j] = b.enc(w[j]);
      bias.insert(bias.end(), bi.begin(), bi.end());
    }
    H.bias = b.upload_f32(std::move(bias));
  }
  e->iou.resize(cfg->iou_depth);
  for (int k = 0; k < cfg->iou_depth; ++k)
    ES_OK(tok_lin(b, "mask_decoder.iou_prediction_head.layers." + std::to_string(k), k + 1 < cfg->iou_depth ? cfg->iou_hidden : nm,
                  k ? cfg->iou_hidden : E, &e->iou[k]));
  {
    const std::string u = "mask_decoder.output_upscaling.";
    ES_GET(w1, u + "0.weight", E, C1, 2, 2);
    ES_GET(b1, u + "0.bias", C1);
    std::vector<float> wg((size_t)4 * C1 * E), bg((size_t)4 * C1);
    for (int s = 0; s < 4; ++s)
      for (int cc = 0; cc < C1; ++cc) {
        bg[(size_t)s * C1 + cc] = b1[cc];
        for (int ci = 0; ci < E; ++ci) wg[((size_t)s * C1 + cc) * E + ci] = w1[((size_t)ci * C1 + cc) * 4 + s];
      }
    e->convt1 = b.pack(wg, bg, 4 * C1, E, nullptr, nullptr, 1.0);
    ES_OK(ln_params(b, u + "1", C1, &e->up_g, &e->up_beta));
    ES_GET(w2, u + "3.weight", C1, C2, 2, 2);
    ES_GET(b2, u + "3.bias", C2);
    e->up_w = b.alloc((size_t)2 * C1 * C1 * 2);
    if (es_sam_upscale_pack(w2.data(), C1, dtype, b.staged(e->up_w, (size_t)2 * C1 * C1 * 2))) return -1;
    e->up_b = b.upload_f32(std::move(b2));
  }
#undef ES_GET
#undef ES_OK

  // activations for max_n images
  const size_t tokE = N * Rmax * E * 2;
  for (size_t* o : {&e->tok, &e->qpe, &e->Q, &e->TT, &e->QP, &e->PQ, &e->PK, &e->PV, &e->ATT}) *o = b.alloc(tokE);
  e->HID = b.alloc(N * Rmax * cfg->mlp_dim * 2);
  e->HA = b.alloc(N * nm * E * 2); e->HB = b.alloc(N * nm * E * 2); e->HO = b.alloc(N * nm * C2 * 2);
  const size_t iw = (size_t)std::max(cfg->iou_hidden, 8);
  e->IA = b.alloc(N * iw * 2); e->IB = b.alloc(N * iw * 2);
  for (size_t* o : {&e->KEYS, &e->KEYS2, &e->IK}) *o = b.alloc(N * HW * E * 2);
  for (size_t* o : {&e->IPA, &e->IPB, &e->IATT}) *o = b.alloc(N * HW * Ci * 2);
  e->LOW = b.alloc(N * nm * 16 * HW * 4);
  // the largest split-K workspace the policy asks for (the tile is one image's at every n: only M grows)
  for (DecLayer& L : e->layers)
    for (auto pr : {std::make_pair(&L.t2i.ik, false), std::make_pair(&L.t2i.iv, false), std::make_pair(&L.i2t.iq, false), std::make_pair(&L.i2t.io, true)})
      e->img_lins.push_back(pr);
  e->img_lins.push_back({&e->final_attn.ik, false}); e->img_lins.push_back({&e->final_attn.iv, false}); e->img_lins.push_back({&e->convt1, false});
  for (auto& pr : e->img_lins) {
    es_launch_choice ch;
    if (!es_enc::choose(e.get(), *pr.first, (int)HW, ES_ACT_NONE, 1.f, pr.second, &ch))
      return dfail(-1, who, std::string("the launch policy has no tile for a projection: ") + es_last_error());
    if (ch.route != ES_ROUTE_CONV_GEMM) return dfail(-1, who, "the launch policy routed a projection away from es_conv_gemm");
    if (ch.splitk > 1) e->ws_bytes = std::max(e->ws_bytes, (size_t)ch.splitk * N * HW * pr.first->rows_padded * 4);
  }
  e->ws = b.alloc(e->ws_bytes);
  e->arena_bytes = b.top;
  if (device < 0) { *out = e.release(); return 0; }      // dry build: everything but the allocation and the upload

  int prev = 0;
  if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(device) != hipSuccess) return dfail(-2, who, "cannot select the device");
  bool ok = es_enc::upload_arena(b, &e->arena, e->arena_bytes);
  ok = ok && hipDeviceSynchronize() == hipSuccess;
  (void)hipSetDevice(prev);
  if (!ok) { (void)hipGetLastError(); return dfail(-2, who, "device allocation or upload failed"); }
  *out = e.release();
  return 0;
}

extern "C" int es_sam_decode(es_sam_decoder* e, const float* emb_nchw, const es_sam_prompts* prompts, int n, int multimask, float* low_res,
                             float* iou, void* stream) {
  const char* who = "es_sam_decode";
  if (!low_res) return dfail(-1, who, "null pointer (low_res)");
  if (check_call(who, e, emb_nchw, prompts, n, iou)) return -1;
  return decode(who, e, emb_nchw, prompts, n, multimask, low_res, iou, stream);
}

extern "C" int es_sam_predict(es_sam_decoder* e, const float* emb_nchw, const es_sam_prompts* prompts, int n, int multimask, float* low_res,
                              float* iou, uint8_t* masks, float* mask_logits, void* stream) {
  const char* who = "es_sam_predict";
  if (!masks && !mask_logits) return dfail(-1, who, "null pointer (both mask outputs)");
  if (check_call(who, e, emb_nchw, prompts, n, iou)) return -1;
  float* low = low_res ? low_res : (float*)(e->arena + e->LOW);
  int rc = decode(who, e, emb_nchw, prompts, n, multimask, low, iou, stream);
  if (rc) return rc;
  int32_t hw[2];
  es_sam_resize_shape(prompts->orig_h, prompts->orig_w, e->cfg.frame, hw);
  const int M = multimask ? e->cfg.n_mask_tokens - 1 : 1;
  return es_sam_postprocess_masks(low, n * M, 4 * e->cfg.grid, e->cfg.frame, hw[0], hw[1], prompts->orig_h, prompts->orig_w, mask_logits, masks, stream);
}
