// The CLIP prompt picker at the C ABI (gfx950): garment bytes in, the best words of the caller's vocabularies out.
//
// Replaces BestEmbeddings (model/utils.py:647-684), which the reference's try_on runs inside every request (app.py:161-165) through
// transformers on the host: CLIPProcessor -> CLIPModel (ViT image tower, text tower over the words) -> logits_per_image -> softmax ->
// the two best words of each list.  The pieces here:
//   es_clip_patchify     uint8 HWC -> normalised rows of the patch-embedding GEMM (the unfold of a Conv2d with kernel = stride = p)
//   es_clip_embed        class token + position table + pre_layrnorm, one launch, one wave per token row
//   es_clip_vision       builder and forward of the image tower on the library's kernels: the text encoder's layer (encoder.h) with
//                        es_attention instead of the causal kernel
//   es_clip_bank         fp32 unit rows of the words' text_embeds; es_clip_text_pool fills it from an es_text_encoder's output
//   es_clip_score        L2 norm, logits, per-vocabulary softmax and top-k, fp32 throughout, one workgroup per image
//   es_clip_pick         bicubic resize (image_io.hip) -> tower -> score
// None of these calls is ever part of a plan: while a plan records on the calling thread they return -1.
#include "encoder.h"

using namespace es_enc;

namespace {

const char* const kRecording = "a plan is recording on this thread; the prompt-picker calls are never part of a plan";
constexpr int kMaxTokens = 1025, kMaxWords = 4096, kMaxProj = 4096, kMaxSeg = 4, kMaxK = 8;

// ---- patchify ---------------------------------------------------------------------------------------------------------------------
struct Norm3 { float mean[3], std[3]; };

// one thread per 8 columns of an output row: 8 scattered byte loads, one 16-byte store (the pad columns store zeros)
template <typename T>
__global__ __launch_bounds__(256) void patchify_kernel(const uint8_t* __restrict__ in, T* __restrict__ out, float* __restrict__ nchw,
                                                       const long long total8, const int R, const int p, const int G, const int K, const int K8,
                                                       const Norm3 nm) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total8) return;
  const long long row = i / K8;
  const int c8 = (int)(i - row * K8);
  const int P = G * G, pp = p * p;
  const int n = (int)(row / P), pr = (int)(row - (long long)n * P);
  const int py = pr / G, px = pr - py * G;
  typename Traits<T>::vec8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = c8 * 8 + e;
    float f = 0.f;
    if (k < K) {
      const int c = k / pp, r = k - c * pp;
      const int ky = r / p, kx = r - ky * p;
      const int y = py * p + ky, x = px * p + kx;
      const uint8_t b = in[(((size_t)n * R + y) * R + x) * 3 + c];
      f = __fdiv_rn(__fdiv_rn((float)b, 255.0f) - nm.mean[c], nm.std[c]);
      if (nchw) nchw[(((size_t)n * 3 + c) * R + y) * R + x] = f;
    }
    v[e] = from_f32<T>(f);
  }
  if (out) *(u32x4*)(out + (size_t)i * 8) = __builtin_bit_cast(u32x4, v);
}

// ---- class token + positions + pre_layrnorm -----------------------------------------------------------------------------------------
// One wave per token row, 4 rows per workgroup (no barrier, no LDS): lane l holds the 16-byte chunks l, l + 64, ... of the row (at most 8:
// 4096 channels) in registers, so the row is read once; mean and variance are the two-pass forms over the ROUNDED sums (what the
// reference's LayerNorm sees), reduced with the DPP / permlane wave_sum.
template <typename T>
__global__ __launch_bounds__(256) void clip_embed_kernel(const T* __restrict__ patch, const float* __restrict__ cls, const float* __restrict__ pos,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta, T* __restrict__ out,
                                                         const int rows, const int P, const int C, const float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;               // wave-uniform
  const int T1 = P + 1, C8 = C >> 3;
  const int n = row / T1, t = row - n * T1;
  const float* prow = pos + (size_t)t * C;
  const T* src = t ? patch + ((size_t)n * P + (t - 1)) * C : nullptr;
  float x[8][8];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = lane + 64 * j;
#pragma unroll
    for (int e = 0; e < 8; ++e) x[j][e] = 0.f;
    if (c < C8) {
      const f32x4 p0 = *(const f32x4*)(prow + c * 8), p1 = *(const f32x4*)(prow + c * 8 + 4);
      float a[8];
      if (src) {
        const auto pv = as_vec8<T>(*(const u32x4*)(src + c * 8));
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = to_f32(pv[e]);
      } else {
        const f32x4 c0 = *(const f32x4*)(cls + c * 8), c1 = *(const f32x4*)(cls + c * 8 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { a[e] = c0[e]; a[4 + e] = c1[e]; }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        x[j][e] = to_f32(from_f32<T>(a[e] + (e < 4 ? p0[e] : p1[e - 4])));      // the embedding, rounded once
        s += x[j][e];
      }
    }
  }
  const float mean = wave_sum(s) / (float)C;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (lane + 64 * j < C8) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = x[j][e] - mean; q = __builtin_fmaf(d, d, q); }
    }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
  T* dst = out + (size_t)row * C;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = lane + 64 * j;
    if (c < C8) {
      const f32x4 g0 = *(const f32x4*)(gamma + c * 8), g1 = *(const f32x4*)(gamma + c * 8 + 4);
      const f32x4 b0 = *(const f32x4*)(beta + c * 8), b1 = *(const f32x4*)(beta + c * 8 + 4);
      typename Traits<T>::vec8 v;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = from_f32<T>((x[j][e] - mean) * rstd * (e < 4 ? g0[e] : g1[e - 4]) + (e < 4 ? b0[e] : b1[e - 4]));
      *(u32x4*)(dst + c * 8) = __builtin_bit_cast(u32x4, v);
    }
  }
}

// ---- unit rows, logits, softmax, top-k ---------------------------------------------------------------------------------------------
template <typename T> ES_DEVICE float load_f32(const T* p, int i) { return to_f32(p[i]); }
template <> ES_DEVICE float load_f32<float>(const float* p, int i) { return p[i]; }

// 1 / |row|_2 in fp32 for the whole 256-thread workgroup (every thread gets it): per-thread partial sums of squares over a strided walk,
// wave_sum, then the four wave results through `red` (LDS, 4 floats) in a fixed order.  Ends behind a barrier: `red` may be reused.
// This is the norm of BOTH sides of the logits: the bank's rows (unit_rows_kernel) and the image embeddings (score_kernel).
template <typename T>
ES_DEVICE float row_inv_norm(const T* row, const int len, float* red) {
  float ss = 0.f;
  for (int i = threadIdx.x; i < len; i += 256) { const float v = load_f32(row, i); ss = __builtin_fmaf(v, v, ss); }
  ss = wave_sum(ss);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
  __syncthreads();
  const float tot = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return 1.0f / sqrtf(tot);
}

// out[r] = in[r] / |in[r]|, fp32 out; one workgroup per row.  in == out is allowed for T = float (the bank's raw rows, normalised where
// they lie): a thread reads element i for the norm, then reads it again and writes it - no other thread touches it.  No __restrict__.
template <typename T>
__global__ __launch_bounds__(256) void unit_rows_kernel(const T* in, float* out, const int len) {
  __shared__ float red[4];
  const T* row = in + (size_t)blockIdx.x * len;
  const float inv = row_inv_norm(row, len, red);
  for (int i = threadIdx.x; i < len; i += 256) out[(size_t)blockIdx.x * len + i] = load_f32(row, i) * inv;
}

struct Segs { int32_t end[kMaxSeg]; int32_t nseg; };

// One workgroup per image.  LDS: the unit embedding (proj floats), then the logits (W floats).  Phase 1: the norm.  Phase 2: wave w takes
// words w, w + 4, ...: lanes walk the row in float4 steps, wave_sum.  Phase 3: wave s owns segment s - maximum, sum of exponentials,
// probabilities, then k rounds of (wave_max of the remaining logits, lowest index among the lanes that hold it), the winner struck out
// in LDS by the lane that owns it.  Indices are below 2^24: exact as floats, so the index minimum rides on wave_max too.
template <typename T>
__global__ __launch_bounds__(256) void score_kernel(const T* __restrict__ pooled, const float* __restrict__ bank, const int W, const int proj,
                                                    const float scale, const Segs segs, const int k, float* __restrict__ logits,
                                                    float* __restrict__ probs, int32_t* __restrict__ topk) {
  extern __shared__ float lds[];
  __shared__ float red[4];
  float* emb = lds;                  // [proj]
  float* lg = lds + proj;            // [W]
  const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T* row = pooled + (size_t)n * proj;
  const float inv = row_inv_norm(row, proj, red);
  for (int i = threadIdx.x; i < proj; i += 256) emb[i] = load_f32(row, i) * inv;
  __syncthreads();
  const int p4 = proj >> 2;
  for (int w = wave; w < W; w += 4) {
    const f32x4* b = (const f32x4*)(bank + (size_t)w * proj);
    float acc = 0.f;
    for (int i = lane; i < p4; i += 64) {
      const f32x4 bv = b[i], ev = *(const f32x4*)(emb + 4 * i);
      acc = __builtin_fmaf(bv[0], ev[0], acc); acc = __builtin_fmaf(bv[1], ev[1], acc);
      acc = __builtin_fmaf(bv[2], ev[2], acc); acc = __builtin_fmaf(bv[3], ev[3], acc);
    }
    acc = wave_sum(acc) * scale;
    if (lane == 0) { lg[w] = acc; if (logits) logits[(size_t)n * W + w] = acc; }
  }
  __syncthreads();
  if (wave >= segs.nseg) return;     // wave-uniform, behind the last barrier
  const int a = wave ? segs.end[wave - 1] : 0, e = segs.end[wave];
  float mx = -INFINITY;
  for (int w = a + lane; w < e; w += 64) mx = fmaxf(mx, lg[w]);
  mx = wave_max(mx);
  float sum = 0.f;
  for (int w = a + lane; w < e; w += 64) sum += expf(lg[w] - mx);
  sum = wave_sum(sum);
  if (probs)
    for (int w = a + lane; w < e; w += 64) probs[(size_t)n * W + w] = expf(lg[w] - mx) / sum;
  if (!topk) return;
  for (int r = 0; r < k; ++r) {
    float best = -INFINITY;
    int bi = 0x00FFFFFF;
    for (int w = a + lane; w < e; w += 64) {
      const float v = lg[w];
      if (v > best) { best = v; bi = w; }          // strictly greater: the lane keeps its lowest index among equals
    }
    const float top = wave_max(best);
    const float cand = (best == top && bi != 0x00FFFFFF) ? -(float)bi : -16777216.0f;
    const int win = (int)(-wave_max(cand));
    if (lane == 0) topk[((size_t)n * segs.nseg + wave) * k + r] = win < e ? win - a : -1;     // -1: nothing left to rank (NaN logits only)
    if (win < e && ((win - a) & 63) == lane) lg[win] = -INFINITY;
    // the strike and the next round's reads are LDS accesses of one wave in program order: no barrier is needed
  }
}

struct Gather { int32_t pos[64]; };
// out[i, :] = ehs[first + i, pos[i], :], 16 bytes per thread
__global__ __launch_bounds__(256) void gather_rows_kernel(const uint16_t* __restrict__ ehs, uint16_t* __restrict__ out, const Gather g, const int count,
                                                          const int S, const int C8) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count * C8) return;
  const int r = i / C8, c = i - r * C8;
  *(u32x4*)(out + ((size_t)r * C8 + c) * 8) = *(const u32x4*)(ehs + (((size_t)r * S + g.pos[r]) * C8 + c) * 8);
}

bool on_device(int device) {
  int dev = -1;
  return hipGetDevice(&dev) == hipSuccess && dev == device;
}

}  // namespace

struct es_clip_bank {
  struct { float ln_eps; } cfg = {1e-5f};      // linear() reads cfg.ln_eps; no LayerNorm is folded here
  int dtype = ES_F16, device = -1, proj = 0, hidden = 0, capacity = 0, max_n = 0, rows = 0;
  bool text = false;
  size_t arena_bytes = 0, ws_bytes = 0;
  char* arena = nullptr;
  Lin tproj;
  size_t data = 0, gathered = 0, projected = 0, ws = 0;
  es_launch_knobs knobs;
};

struct es_clip_vision {
  es_clip_vision_config cfg;
  int dtype = ES_F16, max_n = 0, device = -1;
  int G = 0, P = 0, T = 0, K = 0, Kpad = 0;
  size_t arena_bytes = 0, ws_bytes = 0;
  char* arena = nullptr;
  std::vector<Layer> layers;
  Lin patch, proj;
  size_t cls = 0, pos = 0, pre_g = 0, pre_b = 0, post_g = 0, post_b = 0;       // arena offsets
  size_t rows = 0, pe = 0, xa = 0, xb = 0, qkv = 0, att = 0, hid = 0, ct = 0, ctn = 0, ws = 0;
  es_launch_knobs knobs;
};

extern "C" int es_clip_patchify(const uint8_t* in, void* out_rows, float* out_nchw, int n, int R, int p, const float* mean, const float* std,
                                int dtype, void* stream) {
  const char* who = "es_clip_patchify";
  if (es_plan_recording()) return fail(-1, who, kRecording);
  if (!in || !mean || !std || (!out_rows && !out_nchw)) return fail(-1, who, "null pointer");
  if (dtype != ES_F16 && dtype != ES_BF16) return fail(-1, who, "dtype must be ES_F16 or ES_BF16");
  if (n < 1 || p < 1 || R < p || R > 16384) return fail(-1, who, "n >= 1, 1 <= p <= R <= 16384");
  if (R % p) return fail(-1, who, "image_size must be a multiple of patch_size");
  if ((uintptr_t)out_rows & 15) return fail(-1, who, "out_rows must be 16-byte aligned");
  Norm3 nm;
  for (int c = 0; c < 3; ++c) {
    nm.mean[c] = mean[c]; nm.std[c] = std[c];
    if (!(std[c] > 0.f)) return fail(-1, who, "std must be positive");
  }
  const int G = R / p, K = 3 * p * p, Kpad = round_up(K, BK);
  const long long total8 = (long long)n * G * G * (Kpad / 8);
  if ((total8 + 255) / 256 > 0x7fffffffll || (long long)n * R * R * 3 >= (1ll << 40)) return fail(-1, who, "too many elements for one launch");
  const dim3 grid((unsigned)((total8 + 255) / 256));
  if (dtype == ES_F16) hipLaunchKernelGGL(patchify_kernel<f16>, grid, dim3(256), 0, (hipStream_t)stream, in, (f16*)out_rows, out_nchw, total8, R, p, G, K, Kpad / 8, nm);
  else hipLaunchKernelGGL(patchify_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, in, (bf16*)out_rows, out_nchw, total8, R, p, G, K, Kpad / 8, nm);
  if (ES_CHECK_LAUNCH()) return fail(-2, who, "launch failed");
  return 0;
}

extern "C" int es_clip_embed(const void* patch, const float* cls, const float* pos, const float* gamma, const float* beta, void* out, int n, int P,
                             int hidden, float eps, int dtype, void* stream) {
  const char* who = "es_clip_embed";
  if (es_plan_recording()) return fail(-1, who, kRecording);
  if (!patch || !cls || !pos || !gamma || !beta || !out) return fail(-1, who, "null pointer");
  if (dtype != ES_F16 && dtype != ES_BF16) return fail(-1, who, "dtype must be ES_F16 or ES_BF16");
  if (n < 1 || P < 1 || P + 1 > kMaxTokens) return fail(-1, who, "n >= 1 and 1 <= patches <= 1024");
  if (hidden < 8 || hidden % 8 || hidden > 4096) return fail(-1, who, "hidden must be a multiple of 8, at most 4096 (a row is held in one wave's registers)");
  if (!(eps > 0.f)) return fail(-1, who, "eps must be positive");
  if (((uintptr_t)patch | (uintptr_t)cls | (uintptr_t)pos | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out) & 15) return fail(-1, who, "every operand must be 16-byte aligned");
  const long long rows = (long long)n * (P + 1);
  if (rows > (1 << 24)) return fail(-1, who, "more than 2^24 token rows");
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (dtype == ES_F16) hipLaunchKernelGGL(clip_embed_kernel<f16>, grid, dim3(256), 0, (hipStream_t)stream, (const f16*)patch, cls, pos, gamma, beta, (f16*)out, (int)rows, P, hidden, eps);
  else hipLaunchKernelGGL(clip_embed_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)patch, cls, pos, gamma, beta, (bf16*)out, (int)rows, P, hidden, eps);
  if (ES_CHECK_LAUNCH()) return fail(-2, who, "launch failed");
  return 0;
}

extern "C" int es_clip_score(const void* pooled, int pooled_dtype, const float* bank, int n, int W, int proj, float logit_scale_exp,
                             const int32_t* seg_ends, int nseg, int k, float* logits, float* probs, int32_t* topk, void* stream) {
  const char* who = "es_clip_score";
  if (es_plan_recording()) return fail(-1, who, kRecording);
  if (!pooled || !bank || !seg_ends) return fail(-1, who, "null pointer");
  if (pooled_dtype != ES_F16 && pooled_dtype != ES_BF16 && pooled_dtype != ES_F32) return fail(-1, who, "pooled_dtype must be ES_F16, ES_BF16 or ES_F32");
  if (n < 1 || n > 65535) return fail(-1, who, "n must be in 1..65535");
  if (W < 1 || W > kMaxWords) return fail(-1, who, "W must be in 1..4096 (the logits of an image are kept on chip)");
  if (proj < 4 || proj % 4 || proj > kMaxProj) return fail(-1, who, "proj must be a multiple of 4, at most 4096");
  if (nseg < 1 || nseg > kMaxSeg) return fail(-1, who, "nseg must be in 1..4");
  if (k < 1 || k > kMaxK) return fail(-1, who, "k must be in 1..8");
  if (((uintptr_t)bank | (uintptr_t)pooled) & 15) return fail(-1, who, "pooled and bank must be 16-byte aligned");
  Segs sg = {};
  sg.nseg = nseg;
  int prev = 0;
  for (int s = 0; s < nseg; ++s) {
    if (seg_ends[s] <= prev) return fail(-1, who, "seg_ends must be increasing and start above 0");
    sg.end[s] = prev = seg_ends[s];
  }
  if (prev != W) return fail(-1, who, "the last segment must end at W");
  const size_t lds = (size_t)(proj + W) * 4;        // at most 32 KB
  hipStream_t st = (hipStream_t)stream;
  if (pooled_dtype == ES_F16) hipLaunchKernelGGL(score_kernel<f16>, dim3(n), dim3(256), lds, st, (const f16*)pooled, bank, W, proj, logit_scale_exp, sg, k, logits, probs, topk);
  else if (pooled_dtype == ES_BF16) hipLaunchKernelGGL(score_kernel<bf16>, dim3(n), dim3(256), lds, st, (const bf16*)pooled, bank, W, proj, logit_scale_exp, sg, k, logits, probs, topk);
  else hipLaunchKernelGGL(score_kernel<float>, dim3(n), dim3(256), lds, st, (const float*)pooled, bank, W, proj, logit_scale_exp, sg, k, logits, probs, topk);
  if (ES_CHECK_LAUNCH()) return fail(-2, who, "launch failed");
  return 0;
}

// ---- the bank -----------------------------------------------------------------------------------------------------------------------
extern "C" void es_clip_bank_destroy(es_clip_bank* b) {
  if (!b) return;
  if (b->arena) (void)hipFree(b->arena);
  delete b;
}
extern "C" int es_clip_bank_rows(const es_clip_bank* b) { return b ? b->rows : 0; }
extern "C" const float* es_clip_bank_data(const es_clip_bank* b) { return b && b->arena ? (const float*)(b->arena + b->data) : nullptr; }
extern "C" int es_clip_bank_create(const es_state_dict* text_sd, int text_hidden, int proj, int capacity, int max_n, int dtype, int device,
                                   es_clip_bank** out) {
  const char* who = "es_clip_bank_create";
  if (out) *out = nullptr;
  if (!out) return fail(-1, who, "null pointer");
  if (es_plan_recording()) return fail(-1, who, kRecording);
  if (dtype != ES_F16 && dtype != ES_BF16) return fail(-1, who, "dtype must be ES_F16 or ES_BF16");
  if (device < 0) return fail(-1, who, "device must be >= 0 (a bank is device memory: there is no dry build)");
  if (proj < 4 || proj % 4 || proj > kMaxProj) return fail(-1, who, "proj must be a multiple of 4, at most 4096");
  if (capacity < 1 || capacity > kMaxWords) return fail(-1, who, "capacity must be in 1..4096");
  if (text_sd && (text_hidden < 64 || text_hidden % 64 || text_hidden > 4096)) return fail(-1, who, "text_hidden must be a multiple of 64, at most 4096");
  if (text_sd && (max_n < 1 || max_n > 4096)) return fail(-1, who, "max_n must be in 1..4096");
  EncBuilder bd;
  bd.dt = dtype;
  std::unique_ptr<es_clip_bank, void (*)(es_clip_bank*)> b(new es_clip_bank, es_clip_bank_destroy);
  b->dtype = dtype; b->device = device; b->proj = proj; b->capacity = capacity;
  default_knobs(&b->knobs);
  b->data = bd.alloc((size_t)capacity * proj * 4);
  if (text_sd) {
    if (!bd.init(text_sd, "")) return fail(-1, who, bd.err);
    std::vector<float> w = bd.get("text_projection.weight", proj, text_hidden);
    if (w.empty()) return fail(-1, who, bd.err);
    b->text = true; b->hidden = text_hidden; b->max_n = max_n;
    b->tproj = bd.pack(w, std::vector<float>((size_t)proj, 0.f), proj, text_hidden, nullptr, nullptr, 1.0);
    b->gathered = bd.alloc((size_t)max_n * text_hidden * 2);
    b->projected = bd.alloc((size_t)max_n * proj * 2);
    for (int n = 1; n <= max_n; ++n)
      if (!size_workspace(who, b.get(), b->tproj, n, ES_ACT_NONE, 1.f, false)) return -1;
    b->ws = bd.alloc(b->ws_bytes);
  }
  b->arena_bytes = bd.top;
  int prev = 0;
  if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(device) != hipSuccess) return fail(-2, who, "cannot select the device");
  bool ok = upload_arena(bd, &b->arena, b->arena_bytes);
  ok = ok && hipDeviceSynchronize() == hipSuccess;
  (void)hipSetDevice(prev);
  if (!ok) { (void)hipGetLastError(); return fail(-2, who, "device allocation or upload failed"); }
  *out = b.release();
  return 0;
}

extern "C" int es_clip_bank_append(es_clip_bank* b, const float* rows_host, int count, void* stream) {
  const char* who = "es_clip_bank_append";
  if (!b || !rows_host) return fail(-1, who, "null pointer");
  if (es_plan_recording()) return fail(-1, who, kRecording);
  if (count < 1 || b->rows + count > b->capacity) return fail(-1, who, "count = " + std::to_string(count) + " rows do not fit: " + std::to_string(b->rows) + " of " + std::to_string(b->capacity) + " are taken");
  if (!on_device(b->device)) return fail(-1, who, "the current device is not the one the bank was built on");
  hipStream_t st = (hipStream_t)stream;
  if (capturing(st)) return fail(-1, who, "the stream is capturing; this entry point copies from host memory and cannot be captured");
  float* dst = (float*)(b->arena + b->data) + (size_t)b->rows * b->proj;
  if (hipMemcpyAsync(dst, rows_host, (size_t)count * b->proj * 4, hipMemcpyHostToDevice, st) != hipSuccess) return fail(-2, who, "copy of the rows failed");
  hipLaunchKernelGGL(unit_rows_kernel<float>, dim3(count), dim3(256), 0, st, (const float*)dst, dst, b->proj);
  if (ES_CHECK_LAUNCH()) return fail(-2, who, "launch failed");
  b->rows += count;
  return 0;
}

extern "C" int es_clip_text_pool(es_clip_bank* b, const void* ehs, const int32_t* eos_pos, int n, int S, void* stream) {
  const char* who = "es_clip_text_pool";
  if (!b || !ehs || !eos_pos) return fail(-1, who, "null pointer");
  if (es_plan_recording()) return fail(-1, who, kRecording);
  if (!b->text) return fail(-1, who, "this bank was created without a text_projection (es_clip_bank_create text_sd NULL)");
  if (n < 1 || n > b->max_n) return fail(-1, who, "n = " + std::to_string(n) + " is outside 1..max_n = " + std::to_string(b->max_n));
  if (S < 1 || S > (1 << 20)) return fail(-1, who, "S must be in 1..2^20");
  if (b->rows + n > b->capacity) return fail(-1, who, "n = " + std::to_string(n) + " rows do not fit: " + std::to_string(b->rows) + " of " + std::to_string(b->capacity) + " are taken");
  for (int i = 0; i < n; ++i)
    if (eos_pos[i] < 0 || eos_pos[i] >= S) return fail(-1, who, "eos_pos[" + std::to_string(i) + "] = " + std::to_string(eos_pos[i]) + " is outside [0, " + std::to_string(S) + ")");
  if ((uintptr_t)ehs & 15) return fail(-1, who, "ehs must be 16-byte aligned");
  if (!on_device(b->device)) return fail(-1, who, "the current device is not the one the bank was built on");
  hipStream_t st = (hipStream_t)stream;
  char* A = b->arena;
  const int C8 = b->hidden / 8;
  for (int first = 0; first < n; first += 64) {
    Gather g = {};
    const int cnt = n - first < 64 ? n - first : 64;
    for (int i = 0; i < cnt; ++i) g.pos[i] = eos_pos[first + i];
    hipLaunchKernelGGL(gather_rows_kernel, dim3((cnt * C8 + 255) / 256), dim3(256), 0, st, (const uint16_t*)ehs + (size_t)first * S * b->hidden,
                       (uint16_t*)(A + b->gathered) + (size_t)first * b->hidden, g, cnt, S, C8);
  }
  if (ES_CHECK_LAUNCH()) return fail(-2, who, "launch failed");
  int rc = linear(who, b, b->tproj, A + b->gathered, A + b->projected, nullptr, n, ES_ACT_NONE, 1.f, st);
  if (rc) return rc;
  float* dst = (float*)(A + b->data) + (size_t)b->rows * b->proj;
  if (b->dtype == ES_F16) hipLaunchKernelGGL(unit_rows_kernel<f16>, dim3(n), dim3(256), 0, st, (const f16*)(A + b->projected), dst, b->proj);
  else hipLaunchKernelGGL(unit_rows_kernel<bf16>, dim3(n), dim3(256), 0, st, (const bf16*)(A + b->projected), dst, b->proj);
  if (ES_CHECK_LAUNCH()) return fail(-2, who, "launch failed");
  b->rows += n;
  return 0;
}

// ---- the image tower ------------------------------------------------------------------------------------------------------------------
extern "C" void es_clip_vision_destroy(es_clip_vision* e) {
  if (!e) return;
  if (e->arena) (void)hipFree(e->arena);
  delete e;
}
extern "C" size_t es_clip_vision_arena_bytes(const es_clip_vision* e) { return e ? e->arena_bytes : 0; }

extern "C" int es_clip_vision_create(const es_state_dict* sd, const es_clip_vision_config* cfg, int dtype, int max_n, int device, es_clip_vision** out) {
  const char* who = "es_clip_vision_create";
  if (out) *out = nullptr;
  if (!sd || !cfg || !out) return fail(-1, who, "null pointer");
  if (es_plan_recording()) return fail(-1, who, kRecording);
  if (dtype != ES_F16 && dtype != ES_BF16) return fail(-1, who, "dtype must be ES_F16 or ES_BF16");
  if (device < -1) return fail(-1, who, "device must be >= 0, or -1 for a dry build");
  const int C = cfg->hidden, I = cfg->intermediate, NL = cfg->layers, R = cfg->image_size, p = cfg->patch_size, D = cfg->projection_dim;
  if (cfg->act != 0) return fail(-1, who, "act must be 0 (quick_gelu); other activations are not implemented");
  if (C < 64 || C % 64) return fail(-1, who, "hidden must be a multiple of 64 (LayerNorm fold of the projections)");
  if (C > 4096) return fail(-1, who, "hidden above 4096 (es_layer_norm, es_clip_embed)");
  if (cfg->heads < 1 || C % cfg->heads || (C / cfg->heads != 32 && C / cfg->heads != 64)) return fail(-1, who, "hidden / heads must be 32 or 64");
  if (p < 1 || R < p || R > 16384 || R % p) return fail(-1, who, "image_size must be a multiple of patch_size (and at most 16384)");
  const int G = R / p;
  if ((long long)G * G + 1 > kMaxTokens) return fail(-1, who, "more than 1025 tokens ((image_size / patch_size)^2 + 1)");
  if (I < 64 || I % 64) return fail(-1, who, "intermediate must be a multiple of 64");
  if (NL < 1 || NL > 256) return fail(-1, who, "1 <= layers <= 256");
  if (D < 4 || D % 4 || D > kMaxProj) return fail(-1, who, "projection_dim must be a multiple of 4, at most 4096");
  if (max_n < 1 || max_n > 4096) return fail(-1, who, "max_n must be in 1..4096");
  if (!(cfg->ln_eps > 0.f)) return fail(-1, who, "ln_eps must be positive");
  for (int c = 0; c < 3; ++c)
    if (!(cfg->image_std[c] > 0.f)) return fail(-1, who, "image_std must be positive");

  EncBuilder b;
  b.dt = dtype;
  if (!b.init(sd, "vision_model.")) return fail(-1, who, b.err);
  std::unique_ptr<es_clip_vision, void (*)(es_clip_vision*)> e(new es_clip_vision, es_clip_vision_destroy);
  e->cfg = *cfg; e->dtype = dtype; e->max_n = max_n; e->device = device;
  e->G = G; e->P = G * G; e->T = e->P + 1; e->K = 3 * p * p; e->Kpad = round_up(e->K, BK);
  default_knobs(&e->knobs);
  const int P = e->P, T = e->T, K = e->K, Kpad = e->Kpad;

#define ES_GET(var, ...) std::vector<float> var = b.get(__VA_ARGS__); if (var.empty()) return fail(-1, who, b.err)
  {
    ES_GET(cls, "embeddings.class_embedding", C);
    e->cls = b.upload_f32(std::move(cls));
    ES_GET(pos, "embeddings.position_embedding.weight", T, C);
    e->pos = b.upload_f32(std::move(pos));
    ES_GET(pw, "embeddings.patch_embedding.weight", C, 3, p, p);
    // [hidden][3 p^2] -> [hidden][Kpad]: the GEMM runs over K = Kpad, the pad columns meet the zeros es_clip_patchify writes
    std::vector<float> wpad((size_t)C * Kpad, 0.f);
    for (int r = 0; r < C; ++r) memcpy(&wpad[(size_t)r * Kpad], &pw[(size_t)r * K], (size_t)K * 4);
    e->patch = b.pack(wpad, std::vector<float>((size_t)C, 0.f), C, Kpad, nullptr, nullptr, 1.0);
    ES_GET(g, "pre_layrnorm.weight", C); ES_GET(bt, "pre_layrnorm.bias", C);
    e->pre_g = b.upload_f32(std::move(g)); e->pre_b = b.upload_f32(std::move(bt));
  }
  for (int li = 0; li < NL; ++li) {
    Layer L;
    if (!b.pack_layer("encoder.layers." + std::to_string(li) + ".", C, I, &L)) return fail(-1, who, b.err);
    e->layers.push_back(L);
  }
  {
    ES_GET(g, "post_layernorm.weight", C); ES_GET(bt, "post_layernorm.bias", C);
    e->post_g = b.upload_f32(std::move(g)); e->post_b = b.upload_f32(std::move(bt));
    ES_GET(vp, "visual_projection.weight", D, C);
    e->proj = b.pack(vp, std::vector<float>((size_t)D, 0.f), D, C, nullptr, nullptr, 1.0);
  }
#undef ES_GET

  // activations for max_n images, and the largest split-K workspace the policy asks for at any n <= max_n
  const size_t Mp = (size_t)max_n * P, Mt = (size_t)max_n * T;
  e->rows = b.alloc(Mp * Kpad * 2); e->pe = b.alloc(Mp * C * 2);
  e->xa = b.alloc(Mt * C * 2); e->xb = b.alloc(Mt * C * 2);
  e->qkv = b.alloc(Mt * 3 * C * 2); e->att = b.alloc(Mt * C * 2); e->hid = b.alloc(Mt * I * 2);
  e->ct = b.alloc((size_t)max_n * C * 2); e->ctn = b.alloc((size_t)max_n * C * 2);
  const Layer& L0 = e->layers[0];
  for (int n = 1; n <= max_n; ++n) {
    struct { const Lin* L; int M, act; float sc; bool res; } g[6] = {
        {&e->patch, n * P, ES_ACT_NONE, 1.f, false}, {&L0.qkv, n * T, ES_ACT_NONE, 1.f, false}, {&L0.out, n * T, ES_ACT_NONE, 1.f, true},
        {&L0.fc1, n * T, ES_ACT_SILU, 1.f / QUICK_GELU, false}, {&L0.fc2, n * T, ES_ACT_NONE, 1.f, true}, {&e->proj, n, ES_ACT_NONE, 1.f, false}};
    for (auto& x : g)
      if (!size_workspace(who, e.get(), *x.L, x.M, x.act, x.sc, x.res)) return -1;
  }
  e->ws = b.alloc(e->ws_bytes);
  e->arena_bytes = b.top;
  if (device < 0) { *out = e.release(); return 0; }      // dry build: everything but the allocation and the upload

  int prev = 0;
  if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(device) != hipSuccess) return fail(-2, who, "cannot select the device");
  bool ok = upload_arena(b, &e->arena, e->arena_bytes);
  ok = ok && hipDeviceSynchronize() == hipSuccess;
  (void)hipSetDevice(prev);
  if (!ok) { (void)hipGetLastError(); return fail(-2, who, "device allocation or upload failed"); }
  *out = e.release();
  return 0;
}

extern "C" int es_clip_vision_encode(es_clip_vision* e, const uint8_t* images, int n, void* out_pooled, void* stream) {
  const char* who = "es_clip_vision_encode";
  if (!e || !images || !out_pooled) return fail(-1, who, "null pointer");
  if (es_plan_recording()) return fail(-1, who, kRecording);
  if (n < 1 || n > e->max_n) return fail(-1, who, "n = " + std::to_string(n) + " is outside 1..max_n = " + std::to_string(e->max_n));
  if (!e->arena) return fail(-1, who, "this tower is a dry build (es_clip_vision_create device -1): it holds no device memory and cannot run");
  if (!on_device(e->device)) return fail(-1, who, "the current device is not the one the tower was built on");
  const es_clip_vision_config& c = e->cfg;
  const int C = c.hidden, P = e->P, T = e->T, M = n * T;
  hipStream_t st = (hipStream_t)stream;
  char* A = e->arena;
  int rc = es_clip_patchify(images, A + e->rows, nullptr, n, c.image_size, c.patch_size, c.image_mean, c.image_std, e->dtype, stream);
  if (rc) return rc;
  if ((rc = linear(who, e, e->patch, A + e->rows, A + e->pe, nullptr, n * P, ES_ACT_NONE, 1.f, st))) return rc;
  if ((rc = es_clip_embed(A + e->pe, (const float*)(A + e->cls), (const float*)(A + e->pos), (const float*)(A + e->pre_g), (const float*)(A + e->pre_b),
                          A + e->xa, n, P, C, c.ln_eps, e->dtype, stream))) return rc;
  const int dh = C / c.heads;
  es_attn_desc a;
  memset(&a, 0, sizeof(a));
  a.q = A + e->qkv; a.k = A + e->qkv + (size_t)C * 2; a.v = A + e->qkv + (size_t)2 * C * 2; a.o = A + e->att;
  a.N = n; a.heads = c.heads; a.Sq = T; a.Skv = T; a.d = dh;
  a.ldq = a.ldk = a.ldv = 3 * C; a.ldo = C;
  a.bsq = a.bsk = a.bsv = (int64_t)T * 3 * C; a.bso = (int64_t)T * C;
  a.scale = (float)(1.0 / sqrt((double)dh)); a.dtype = e->dtype;
  for (const Layer& L : e->layers) {      // the stream lives in xa at the top of every layer
    if ((rc = linear(who, e, L.qkv, A + e->xa, A + e->qkv, nullptr, M, ES_ACT_NONE, 1.f, st))) return rc;
    if ((rc = es_attention(&a, stream))) return rc;
    if ((rc = linear(who, e, L.out, A + e->att, A + e->xb, A + e->xa, M, ES_ACT_NONE, 1.f, st))) return rc;
    if ((rc = linear(who, e, L.fc1, A + e->xb, A + e->hid, nullptr, M, ES_ACT_SILU, 1.f / QUICK_GELU, st))) return rc;
    if ((rc = linear(who, e, L.fc2, A + e->hid, A + e->xa, A + e->xb, M, ES_ACT_NONE, 1.f, st))) return rc;
  }
  // pooled_output = post_layernorm(last_hidden_state[:, 0]); image_embeds = visual_projection(pooled_output)
  if ((rc = es_memcpy2d(A + e->ct, (size_t)C * 2, A + e->xa, (size_t)T * C * 2, (size_t)C * 2, (size_t)n, stream))) return rc;
  if ((rc = es_layer_norm(A + e->ct, A + e->ctn, (const float*)(A + e->post_g), (const float*)(A + e->post_b), n, C, c.ln_eps, e->dtype, stream))) return rc;
  return linear(who, e, e->proj, A + e->ctn, out_pooled, nullptr, n, ES_ACT_NONE, 1.f, st);
}

// workspace of es_clip_pick: [resized bytes | pooled embeddings | the resize's own scratch], each part 256-byte aligned
static size_t pick_layout(const es_clip_vision* e, int count, size_t* pooled_off, size_t* scratch_off) {
  const size_t R = (size_t)e->cfg.image_size;
  size_t top = ((size_t)count * R * R * 3 + 255) & ~(size_t)255;
  *pooled_off = top;
  top += ((size_t)count * e->cfg.projection_dim * 2 + 255) & ~(size_t)255;
  *scratch_off = top;
  return top;
}

extern "C" size_t es_clip_pick_workspace_bytes(const es_clip_vision* e, const es_image_u8* imgs, int count) {
  const char* who = "es_clip_pick_workspace_bytes";
  if (!e || !imgs) { fail(-1, who, "null pointer"); return 0; }
  if (count < 1 || count > e->max_n) { fail(-1, who, "count = " + std::to_string(count) + " is outside 1..max_n = " + std::to_string(e->max_n)); return 0; }
  for (int i = 0; i < count; ++i)
    if (imgs[i].height < 1 || imgs[i].width < 1) { fail(-1, who, "image " + std::to_string(i) + ": height or width < 1"); return 0; }
  size_t po, so;
  const size_t fixed = pick_layout(e, count, &po, &so);
  return fixed + es_image_resize_workspace_bytes_ex(imgs, count, e->cfg.image_size, ES_FILTER_BICUBIC, ES_CROP_TRANSFORMERS);
}

extern "C" int es_clip_pick(es_clip_vision* e, const es_clip_bank* bank, const es_image_u8* imgs, int count, float logit_scale_exp,
                            const int32_t* seg_ends, int nseg, int k, float* logits, float* probs, int32_t* topk, void* workspace,
                            size_t workspace_bytes, void* stream) {
  const char* who = "es_clip_pick";
  if (!e || !bank || !imgs || !seg_ends || !workspace) return fail(-1, who, "null pointer");
  if (es_plan_recording()) return fail(-1, who, kRecording);
  if (count < 1 || count > e->max_n) return fail(-1, who, "count = " + std::to_string(count) + " is outside 1..max_n = " + std::to_string(e->max_n));
  if (!e->arena) return fail(-1, who, "this tower is a dry build (es_clip_vision_create device -1): it holds no device memory and cannot run");
  if (bank->proj != e->cfg.projection_dim) return fail(-1, who, "the bank's rows have " + std::to_string(bank->proj) + " columns, the tower projects to " + std::to_string(e->cfg.projection_dim));
  if (bank->device != e->device) return fail(-1, who, "the bank and the tower live on different devices");
  if (bank->rows < 1) return fail(-1, who, "the bank is empty");
  if ((uintptr_t)workspace & 255) return fail(-1, who, "workspace must be 256-byte aligned");
  size_t po, so;
  const size_t fixed = pick_layout(e, count, &po, &so);
  if (workspace_bytes < fixed) return fail(-1, who, "workspace too small: " + std::to_string(workspace_bytes) + " bytes given (es_clip_pick_workspace_bytes)");
  char* ws = (char*)workspace;
  int rc = es_image_resize_impl_ex(who, imgs, count, (uint8_t*)ws, nullptr, nullptr, e->cfg.image_size, ES_FILTER_BICUBIC, ES_CROP_TRANSFORMERS,
                                   ws + so, workspace_bytes - fixed, stream);
  if (rc) return rc;
  if ((rc = es_clip_vision_encode(e, (const uint8_t*)ws, count, ws + po, stream))) return rc;
  return es_clip_score(ws + po, e->dtype, es_clip_bank_data(bank), count, bank->rows, bank->proj, logit_scale_exp, seg_ends, nseg, k, logits, probs, topk, stream);
}
