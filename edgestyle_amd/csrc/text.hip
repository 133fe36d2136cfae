// The CLIP text encoder at the C ABI (gfx950): token ids in, the text states `ehs` of es_denoise_step / es_denoise_loop out.
//
// Replaces transformers' CLIPTextModel forward that the reference runs once per request (app.py:163-176: the prompt and the
// negative prompt; model/edgestyle_pipeline.py encode_prompt) - last_hidden_state of a pre-LN transformer with a causal mask:
//   x = token_embedding[ids] + position_embedding
//   per layer:  x += out_proj(attn_causal(q, k, v of LayerNorm1(x)));   x += fc2(quick_gelu(fc1(LayerNorm2(x))))
//   out = final_layer_norm(x)
// Three pieces live here:
//   es_attention_causal  softmax_{j <= i}(Q_i K_j scale) V_j for S <= 128 keys: all of K and V of one head sit in LDS (128 x 64 x 2 B x 2
//                        = 32 KB), so there is no online softmax - one pass of QK^T on MFMA 16x16x32 into registers, mask, row max, exp2,
//                        row sum, PV.  Orientation and fragment maps are attention.hip's generic kernel's (S^T = K Q^T: a lane owns one
//                        query column, its accumulators are keys; P^T is the B operand of O^T = V^T P^T; V is read with the transposed
//                        LDS read).  A wave only computes the 16-key fragments at or below its 16 queries.
//   es_text_embed        out[r] = round(tok[ids[r]] + pos[r % S]), both tables fp32 (nn.Embedding stays fp32 under autocast), one rounding.
//   es_text_encoder      the builder (state dict -> packed weights in one arena; its pieces are encoder.h's, shared with clip.hip) and the
//                        forward, on the kernels the library already has:
//                        es_conv_gemm through the shared launch policy (es_launch_choose) for the four GEMMs of a layer - q|k|v as one
//                        GEMM of 3C columns with LayerNorm1 folded in (ln_colsum), out_proj and fc2 with the residual add in the epilogue,
//                        fc1 with LayerNorm2 folded in - and es_layer_norm for the final norm.
// quick_gelu without a new GEMM epilogue: x sigmoid(1.702 x) = silu(1.702 x) / 1.702, so fc1 is packed as 1.702 W, 1.702 b and launched with
// ES_ACT_SILU and out_scale = 1 / 1.702.
// None of these calls is ever part of a plan: while a plan records on the calling thread they return -1.
#include "encoder.h"

using namespace es_enc;

namespace {

constexpr int S_MAX = 128;
constexpr float NEG = -3.0e38f;

// ---- causal attention ---------------------------------------------------------------------------------------------------------
// grid (ceil(S / 64), heads, N), 4 waves: wave w owns queries q0 = 64 * blockIdx.x + 16 * w .. + 15.  Keys 0 .. kend - 1, kend = min(S,
// 64 * blockIdx.x + 64), are staged once, padded with ZERO rows to a multiple of 32 (a PV k-step): rows >= S are out of the buffer
// resource's range (hardware zero-fill) and are zeroed explicitly as well - a masked probability is exactly 0, but 0 x NaN is NaN in a
// matrix product, so what the pad rows of V hold matters.
template <typename T, int KS /* head_dim = 32 * KS */>
__global__ __launch_bounds__(256) void attention_causal_kernel(const es_attn_desc p) {
  constexpr int D = 32 * KS, DF = 2 * KS;
  constexpr int ROW = D * 2 + 16;       // bytes per K / V row in LDS (+16 B pad)
  constexpr int CH = D / 8;             // 16-byte chunks per row
  __shared__ __attribute__((aligned(16))) char ks_[S_MAX * ROW];
  __shared__ __attribute__((aligned(16))) char vs_[S_MAX * ROW];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, n = blockIdx.z, S = p.Sq;
  const int qb0 = blockIdx.x * 64, q0 = qb0 + wave * 16;
  const int kend = S < qb0 + 64 ? S : qb0 + 64;
  const int kpad = (kend + 31) & ~31;   // <= 128

  const T* Q = (const T*)p.q + (size_t)n * p.bsq + (size_t)h * D;
  const T* K = (const T*)p.k + (size_t)n * p.bsk + (size_t)h * D;
  const T* V = (const T*)p.v + (size_t)n * p.bsv + (size_t)h * D;
  T* O = (T*)p.o + (size_t)n * p.bso + (size_t)h * D;

  const auto rK = __builtin_amdgcn_make_buffer_rsrc((void*)K, (short)0, (int)(((size_t)(S - 1) * p.ldk + D) * 2), 0x00020000);
  const auto rV = __builtin_amdgcn_make_buffer_rsrc((void*)V, (short)0, (int)(((size_t)(S - 1) * p.ldv + D) * 2), 0x00020000);
  for (int i = tid; i < kpad * CH; i += 256) {
    const int r = i / CH, c = i - r * CH;
    u32x4 kv = __builtin_amdgcn_raw_buffer_load_b128(rK, (r * p.ldk + c * 8) * 2, 0, 0);
    u32x4 vv = __builtin_amdgcn_raw_buffer_load_b128(rV, (r * p.ldv + c * 8) * 2, 0, 0);
    if (r >= S) { kv = u32x4{0u, 0u, 0u, 0u}; vv = u32x4{0u, 0u, 0u, 0u}; }
    *(u32x4*)(ks_ + r * ROW + c * 16) = kv;
    *(u32x4*)(vs_ + r * ROW + c * 16) = vv;
  }
  __syncthreads();
  if (q0 >= S) return;                  // wave-uniform, behind the only barrier

  // Q^T fragments (B operand): lane holds Q[query = col][32 * s + 8 * g .. + 7]; rows past S re-read row S - 1 and are never stored
  const int qi = q0 + col;
  const int qr = qi < S ? qi : S - 1;
  typename Traits<T>::vec8 qf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) qf[s] = as_vec8<T>(*(const u32x4*)(Q + (size_t)qr * p.ldq + (4 * s + g) * 8));

  // ---- S^T = K Q^T, scaled to the exp2 domain in fp32; the mask goes in BEFORE the row maximum and the row sum are taken ----
  const float sl2 = p.scale * 1.4426950408889634f;
  const int nkf = (q0 >> 4) + 1;        // 16-key fragments at or below this wave's queries (q0 < S: all inside the staged rows)
  f32x4 s[S_MAX / 16];
#pragma unroll
  for (int kf = 0; kf < S_MAX / 16; ++kf) {
    s[kf] = f32x4{NEG, NEG, NEG, NEG};
    if (kf < nkf) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ksx = 0; ksx < KS; ++ksx) {
        const auto ka = as_vec8<T>(*(const u32x4*)(ks_ + (kf * 16 + col) * ROW + (4 * ksx + g) * 16));
        acc = mfma16(ka, qf[ksx], acc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kf * 16 + g * 4 + r;
        s[kf][r] = (key > qi || key >= S) ? NEG : acc[r] * sl2;
      }
    }
  }
  float mx = NEG;                       // key 0 is valid for every query: the maximum is finite
#pragma unroll
  for (int kf = 0; kf < S_MAX / 16; ++kf) {
    mx = fmaxf(fmaxf(mx, s[kf][0]), s[kf][1]);
    mx = fmaxf(fmaxf(mx, s[kf][2]), s[kf][3]);
  }
  mx = xor32_max(xor16_max(mx));        // lanes l, l^16, l^32, l^48 hold the four key groups of one query
  float rs = 0.f;
#pragma unroll
  for (int kf = 0; kf < S_MAX / 16; ++kf)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float e = s[kf][r] <= -1.0e38f ? 0.f : __builtin_amdgcn_exp2f(s[kf][r] - mx);     // masked: exactly 0
      s[kf][r] = e;
      rs += e;
    }
  const float l = xor32_sum(xor16_sum(rs));

  // ---- O^T = V^T P^T ----  P^T as B operand: k index 8g + j <-> key 32 * sx + 16 * (j >> 2) + 4g + (j & 3)
  f32x4 o[DF];
#pragma unroll
  for (int j = 0; j < DF; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nsx = (nkf + 1) >> 1;       // 32 * nsx <= kpad
#pragma unroll
  for (int sx = 0; sx < S_MAX / 32; ++sx) {
    if (sx < nsx) {
      typename Traits<T>::vec8 b;
#pragma unroll
      for (int j = 0; j < 8; ++j) b[j] = from_f32<T>(s[2 * sx + (j >> 2)][j & 3]);
#pragma unroll
      for (int j = 0; j < DF; ++j) {
        // lane 4q + pp of each 16-lane group supplies row q, columns 4pp .. 4pp + 3 of its 4 x 16 block
        const int q = col >> 2, pp = col & 3;
        const char* base = vs_ + (32 * sx + 4 * g + q) * ROW + (j * 16 + 4 * pp) * 2;
        const u32x2 lo = lds_read_tr16(base);
        const u32x2 hi = lds_read_tr16(base + 16 * ROW);
        const u32x4 av = {lo[0], lo[1], hi[0], hi[1]};
        o[j] = mfma16(as_vec8<T>(av), b, o[j]);
      }
    }
  }

  if (qi < S) {
    const float inv = 1.0f / l;
#pragma unroll
    for (int j = 0; j < DF; ++j) {
      typename Traits<T>::vec4 pk;
#pragma unroll
      for (int r = 0; r < 4; ++r) pk[r] = from_f32<T>(o[j][r] * inv);
      *(u32x2*)(O + (size_t)qi * p.ldo + j * 16 + g * 4) = __builtin_bit_cast(u32x2, pk);
    }
  }
}

template <typename T>
int launch_causal(const es_attn_desc& d, hipStream_t st) {
  const dim3 grid((d.Sq + 63) / 64, d.heads, d.N);
  if (d.d == 64) hipLaunchKernelGGL((attention_causal_kernel<T, 2>), grid, dim3(256), 0, st, d);
  else hipLaunchKernelGGL((attention_causal_kernel<T, 1>), grid, dim3(256), 0, st, d);
  return ES_CHECK_LAUNCH();
}

// ---- embedding ----------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void text_embed_kernel(const int32_t* __restrict__ ids, const float* __restrict__ tok, const float* __restrict__ pos,
                                                         T* __restrict__ out, const long long total8, const int S, const int C8, const int vocab) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total8) return;
  const long long r = i / C8;
  const int c = (int)(i - r * C8);
  int id = ids[r];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);        // a bad id never reads outside the table (the host entry refuses it first)
  const f32x4* t = (const f32x4*)(tok + ((size_t)id * C8 + c) * 8);
  const f32x4* q = (const f32x4*)(pos + ((size_t)(r % S) * C8 + c) * 8);
  const f32x4 a0 = t[0] + q[0], a1 = t[1] + q[1];
  typename Traits<T>::vec8 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[e] = from_f32<T>(a0[e]); v[4 + e] = from_f32<T>(a1[e]); }
  *(u32x4*)(out + (size_t)i * 8) = __builtin_bit_cast(u32x4, v);
}

const char* const kRecording = "a plan is recording on this thread; the text-encoder calls are never part of a plan";

}  // namespace

struct es_text_encoder {
  es_text_config cfg;
  int dtype = ES_F16, max_n = 0, device = -1;
  size_t arena_bytes = 0, ws_bytes = 0;
  char* arena = nullptr;
  int32_t* ids_pinned = nullptr;
  hipEvent_t staged = nullptr;
  std::vector<Layer> layers;
  size_t tok = 0, pos = 0, fln_g = 0, fln_b = 0;                 // arena offsets
  size_t ids = 0, xa = 0, xb = 0, qkv = 0, att = 0, hid = 0, ws = 0;
  es_launch_knobs knobs;
};

extern "C" int es_attention_causal(const es_attn_desc* d, void* stream) {
  const char* who = "es_attention_causal";
  if (!d) return fail(-1, who, "null pointer (descriptor)");
  if (es_plan_recording()) return fail(-1, who, kRecording);
  if (!d->q || !d->k || !d->v || !d->o) return fail(-1, who, "null pointer");
  if (d->dtype != ES_F16 && d->dtype != ES_BF16) return fail(-1, who, "dtype must be ES_F16 or ES_BF16");
  if (d->N < 1 || d->heads < 1 || d->N > 65535 || d->heads > 65535) return fail(-1, who, "N and heads must be in 1..65535");
  if (d->Sq != d->Skv) return fail(-1, who, "Sq != Skv: the causal kernel is self-attention over one sequence");
  if (d->Sq < 1 || d->Sq > S_MAX) return fail(-1, who, "S must be in 1..128 (all keys of a head are kept on chip)");
  if (d->d != 32 && d->d != 64) return fail(-1, who, "unsupported head_dim (32, 64)");
  if (d->ldq % 8 || d->ldk % 8 || d->ldv % 8 || d->ldo % 4 || d->bsq % 8 || d->bsk % 8 || d->bsv % 8 || d->bso % 4)
    return fail(-1, who, "row and batch strides must be multiples of 8 elements (4 for o)");
  const long long need = (long long)d->heads * d->d;
  if (d->ldq < need || d->ldk < need || d->ldv < need || d->ldo < need) return fail(-1, who, "a row stride below heads * head_dim");
  if (d->bsq < 0 || d->bsk < 0 || d->bsv < 0 || d->bso < 0) return fail(-1, who, "negative batch stride");
  if (((uintptr_t)d->q | (uintptr_t)d->k | (uintptr_t)d->v) & 15 || ((uintptr_t)d->o & 7)) return fail(-1, who, "q, k, v must be 16-byte aligned, o 8-byte aligned");
  if ((long long)S_MAX * d->ldk * 2 >= (1ll << 31) || (long long)S_MAX * d->ldv * 2 >= (1ll << 31)) return fail(-1, who, "k / v row stride too long for 32-bit buffer offsets");
  const int rc = d->dtype == ES_F16 ? launch_causal<f16>(*d, (hipStream_t)stream) : launch_causal<bf16>(*d, (hipStream_t)stream);
  if (rc) return fail(rc, who, "launch failed");
  return 0;
}

extern "C" int es_text_embed(const int32_t* ids, const float* tok, const float* pos, void* out, int rows, int S, int hidden, int vocab, int dtype, void* stream) {
  const char* who = "es_text_embed";
  if (es_plan_recording()) return fail(-1, who, kRecording);
  if (!ids || !tok || !pos || !out) return fail(-1, who, "null pointer");
  if (dtype != ES_F16 && dtype != ES_BF16) return fail(-1, who, "dtype must be ES_F16 or ES_BF16");
  if (rows < 1 || S < 1 || vocab < 1 || hidden < 8 || hidden % 8) return fail(-1, who, "rows, S, vocab >= 1 and hidden a multiple of 8");
  if (((uintptr_t)tok | (uintptr_t)pos | (uintptr_t)out) & 15) return fail(-1, who, "tok, pos and out must be 16-byte aligned");
  const long long total8 = (long long)rows * (hidden / 8);
  if ((total8 + 255) / 256 > 0x7fffffffll) return fail(-1, who, "too many elements for one launch");
  const dim3 grid((unsigned)((total8 + 255) / 256));
  if (dtype == ES_F16) hipLaunchKernelGGL(text_embed_kernel<f16>, grid, dim3(256), 0, (hipStream_t)stream, ids, tok, pos, (f16*)out, total8, S, hidden / 8, vocab);
  else hipLaunchKernelGGL(text_embed_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, ids, tok, pos, (bf16*)out, total8, S, hidden / 8, vocab);
  if (ES_CHECK_LAUNCH()) return fail(-2, who, "launch failed");
  return 0;
}

extern "C" void es_text_encoder_destroy(es_text_encoder* e) {
  if (!e) return;
  if (e->staged) { (void)hipEventSynchronize(e->staged); (void)hipEventDestroy(e->staged); }
  if (e->ids_pinned) (void)hipHostFree(e->ids_pinned);
  if (e->arena) (void)hipFree(e->arena);
  delete e;
}

extern "C" size_t es_text_encoder_arena_bytes(const es_text_encoder* e) { return e ? e->arena_bytes : 0; }

extern "C" int es_text_encoder_create(const es_state_dict* sd, const es_text_config* cfg, int dtype, int max_n, int device, es_text_encoder** out) {
  const char* who = "es_text_encoder_create";
  if (out) *out = nullptr;
  if (!sd || !cfg || !out) return fail(-1, who, "null pointer");
  if (es_plan_recording()) return fail(-1, who, kRecording);
  if (dtype != ES_F16 && dtype != ES_BF16) return fail(-1, who, "dtype must be ES_F16 or ES_BF16");
  if (device < -1) return fail(-1, who, "device must be >= 0, or -1 for a dry build");
  const int C = cfg->hidden, I = cfg->intermediate, S = cfg->max_positions, V = cfg->vocab_size, NL = cfg->layers;
  if (cfg->act != 0) return fail(-1, who, "act must be 0 (quick_gelu); other activations are not implemented");
  if (C < 64 || C % 64) return fail(-1, who, "hidden must be a multiple of 64 (LayerNorm fold of the projections)");
  if (C > 4096) return fail(-1, who, "hidden above 4096 (es_layer_norm)");
  if (cfg->heads < 1 || C % cfg->heads || (C / cfg->heads != 32 && C / cfg->heads != 64)) return fail(-1, who, "hidden / heads must be 32 or 64 (es_attention_causal)");
  if (S < 1 || S > S_MAX) return fail(-1, who, "max_positions must be in 1..128 (es_attention_causal keeps all keys on chip)");
  if (I < 64 || I % 64) return fail(-1, who, "intermediate must be a multiple of 64");
  if (V < 1 || NL < 1 || NL > 256) return fail(-1, who, "vocab_size >= 1 and 1 <= layers <= 256");
  if (max_n < 1 || (long long)max_n * S > (1 << 24)) return fail(-1, who, "max_n must be >= 1 (and max_n * max_positions <= 2^24)");
  if (!(cfg->ln_eps > 0.f)) return fail(-1, who, "ln_eps must be positive");

  EncBuilder b;
  b.dt = dtype;
  if (!b.init(sd, "text_model.")) return fail(-1, who, b.err);
  std::unique_ptr<es_text_encoder, void (*)(es_text_encoder*)> e(new es_text_encoder, es_text_encoder_destroy);
  e->cfg = *cfg; e->dtype = dtype; e->max_n = max_n; e->device = device;
  default_knobs(&e->knobs);

#define ES_GET(var, ...) std::vector<float> var = b.get(__VA_ARGS__); if (var.empty()) return fail(-1, who, b.err)
  {
    ES_GET(tok, "embeddings.token_embedding.weight", V, C);
    e->tok = b.upload_f32(std::move(tok));
    ES_GET(pos, "embeddings.position_embedding.weight", S, C);
    e->pos = b.upload_f32(std::move(pos));
  }
  for (int li = 0; li < NL; ++li) {
    const std::string p = "encoder.layers." + std::to_string(li) + ".";
    Layer L;
    if (!b.pack_layer(p, C, I, &L)) return fail(-1, who, b.err);
    e->layers.push_back(L);
  }
  {
    ES_GET(g, "final_layer_norm.weight", C); ES_GET(bt, "final_layer_norm.bias", C);
    e->fln_g = b.upload_f32(std::move(g)); e->fln_b = b.upload_f32(std::move(bt));
  }
#undef ES_GET

  // activations for max_n prompts, and the largest split-K workspace the policy asks for at any n <= max_n
  const size_t Mmax = (size_t)max_n * S;
  e->ids = b.alloc(Mmax * 4);
  e->xa = b.alloc(Mmax * C * 2); e->xb = b.alloc(Mmax * C * 2);
  e->qkv = b.alloc(Mmax * 3 * C * 2); e->att = b.alloc(Mmax * C * 2); e->hid = b.alloc(Mmax * I * 2);
  const Layer& L0 = e->layers[0];
  for (int n = 1; n <= max_n; ++n) {
    const int M = n * S;
    struct { const Lin* L; int act; float sc; bool res; } g[4] = {{&L0.qkv, ES_ACT_NONE, 1.f, false}, {&L0.out, ES_ACT_NONE, 1.f, true},
                                                                   {&L0.fc1, ES_ACT_SILU, 1.f / QUICK_GELU, false}, {&L0.fc2, ES_ACT_NONE, 1.f, true}};
    for (auto& x : g)
      if (!size_workspace(who, e.get(), *x.L, M, x.act, x.sc, x.res)) return -1;
  }
  e->ws = b.alloc(e->ws_bytes);
  e->arena_bytes = b.top;
  if (device < 0) { *out = e.release(); return 0; }      // dry build: everything but the allocation and the upload

  int prev = 0;
  if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(device) != hipSuccess) return fail(-2, who, "cannot select the device");
  bool ok = upload_arena(b, &e->arena, e->arena_bytes);
  ok = ok && hipHostMalloc((void**)&e->ids_pinned, Mmax * 4, hipHostMallocDefault) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&e->staged, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipDeviceSynchronize() == hipSuccess;
  (void)hipSetDevice(prev);
  if (!ok) { (void)hipGetLastError(); return fail(-2, who, "device allocation or upload failed"); }
  *out = e.release();
  return 0;
}

// the forward from ids on the device: what es_text_encode and es_text_encode_dev share
static int forward(const char* who, es_text_encoder* e, const int32_t* ids_dev, int n, void* out_ehs, void* stream) {
  const int C = e->cfg.hidden, S = e->cfg.max_positions, V = e->cfg.vocab_size, M = n * S;
  hipStream_t st = (hipStream_t)stream;
  char* A = e->arena;
  int rc = es_text_embed(ids_dev, (const float*)(A + e->tok), (const float*)(A + e->pos), A + e->xa, M, S, C, V, e->dtype, stream);
  if (rc) return rc;
  const int dh = C / e->cfg.heads;
  es_attn_desc a;
  memset(&a, 0, sizeof(a));
  a.q = A + e->qkv; a.k = A + e->qkv + (size_t)C * 2; a.v = A + e->qkv + (size_t)2 * C * 2; a.o = A + e->att;
  a.N = n; a.heads = e->cfg.heads; a.Sq = S; a.Skv = S; a.d = dh;
  a.ldq = a.ldk = a.ldv = 3 * C; a.ldo = C;
  a.bsq = a.bsk = a.bsv = (int64_t)S * 3 * C; a.bso = (int64_t)S * C;
  a.scale = (float)(1.0 / sqrt((double)dh)); a.dtype = e->dtype;
  for (const Layer& L : e->layers) {      // the stream lives in xa at the top of every layer
    if ((rc = linear(who, e, L.qkv, A + e->xa, A + e->qkv, nullptr, M, ES_ACT_NONE, 1.f, st))) return rc;
    if ((rc = es_attention_causal(&a, stream))) return rc;
    if ((rc = linear(who, e, L.out, A + e->att, A + e->xb, A + e->xa, M, ES_ACT_NONE, 1.f, st))) return rc;
    if ((rc = linear(who, e, L.fc1, A + e->xb, A + e->hid, nullptr, M, ES_ACT_SILU, 1.f / QUICK_GELU, st))) return rc;
    if ((rc = linear(who, e, L.fc2, A + e->hid, A + e->xa, A + e->xb, M, ES_ACT_NONE, 1.f, st))) return rc;
  }
  return es_layer_norm(A + e->xa, out_ehs, (const float*)(A + e->fln_g), (const float*)(A + e->fln_b), M, C, e->cfg.ln_eps, e->dtype, stream);
}

extern "C" int es_text_encode(es_text_encoder* e, const int32_t* ids_host, int n, void* out_ehs, void* stream) {
  const char* who = "es_text_encode";
  if (!e || !ids_host || !out_ehs) return fail(-1, who, "null pointer");
  if (es_plan_recording()) return fail(-1, who, kRecording);
  if (n < 1 || n > e->max_n) return fail(-1, who, "n = " + std::to_string(n) + " is outside 1..max_n = " + std::to_string(e->max_n));
  if (!e->arena) return fail(-1, who, "this encoder is a dry build (es_text_encoder_create device -1): it holds no device memory and cannot run");
  const int S = e->cfg.max_positions, V = e->cfg.vocab_size, M = n * S;
  for (int i = 0; i < M; ++i)
    if (ids_host[i] < 0 || ids_host[i] >= V)
      return fail(-1, who, "token id " + std::to_string(ids_host[i]) + " at row " + std::to_string(i / S) + ", position " + std::to_string(i % S) + " is outside [0, " + std::to_string(V) + ")");
  hipStream_t st = (hipStream_t)stream;
  if (capturing(st)) return fail(-1, who, "the stream is capturing; this entry point stages the token ids through pinned memory and cannot be captured");
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev != e->device) return fail(-1, who, "the current device is not the one the encoder was built on");
  if (hipEventSynchronize(e->staged) != hipSuccess) return fail(-2, who, "hipEventSynchronize failed");      // the previous call's copy has completed
  memcpy(e->ids_pinned, ids_host, (size_t)M * 4);
  char* A = e->arena;
  if (hipMemcpyAsync(A + e->ids, e->ids_pinned, (size_t)M * 4, hipMemcpyHostToDevice, st) != hipSuccess) return fail(-2, who, "copy of the token ids failed");
  if (hipEventRecord(e->staged, st) != hipSuccess) return fail(-2, who, "hipEventRecord failed");
  return forward(who, e, (const int32_t*)(A + e->ids), n, out_ehs, stream);
}

// es_text_encode with the ids already on the device: no pinned staging, nothing allocated - capturable.  Everything after the id copy
// is es_text_encode's own code (forward), so the two agree bit for bit; an id outside the vocabulary is clamped by the embed kernel.
extern "C" int es_text_encode_dev(es_text_encoder* e, const int32_t* ids_dev, int n, void* out_ehs, void* stream) {
  const char* who = "es_text_encode_dev";
  if (!e || !ids_dev || !out_ehs) return fail(-1, who, "null pointer");
  if (es_plan_recording()) return fail(-1, who, kRecording);
  if (n < 1 || n > e->max_n) return fail(-1, who, "n = " + std::to_string(n) + " is outside 1..max_n = " + std::to_string(e->max_n));
  if (!e->arena) return fail(-1, who, "this encoder is a dry build (es_text_encoder_create device -1): it holds no device memory and cannot run");
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev != e->device) return fail(-1, who, "the current device is not the one the encoder was built on");
  return forward(who, e, ids_dev, n, out_ehs, stream);
}
