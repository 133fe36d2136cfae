// The EfficientViT-SAM image encoder at the C ABI (gfx950): the reference's normalised photo tensor in, the 64 x 64 image embedding of a SAM
// mask decoder out.
//
// Replaces EfficientViTSamImageEncoder.forward (efficientvit/models/efficientvit/sam.py:174-190) that EfficientViTSamPredictor.set_image runs
// once per photo AND per predictor (extract_dataset.py:371-425: five predictors, whose fine-tuned models share one frozen image encoder):
//   EfficientViTLargeBackbone  stage0  conv3x3 s2 + BN + gelu; ResBlocks (3x3 + BN + gelu, 3x3 + BN, + x)
//                              stage1, stage2  FusedMBConv (3x3 + BN + gelu, 1x1 + BN; + x on the stride-1 blocks)
//                              stage3  MBConv (1x1 + bias + gelu, depthwise 3x3 + bias + gelu, 1x1 + BN)
//                              stage4  MBConv, then EfficientViTBlocks = LiteMLA + MBConv, both residual
//   SamNeck                    1x1 + BN of stage4 / stage3 / stage2 -> bicubic to 64 x 64 -> sum -> FusedMBConv blocks -> 1x1 + bias
//   LayerNorm2d                over the channels of each pixel
// gelu is nn.GELU(approximate="tanh").  Activations are NHWC in the storage dtype.  What is new here:
//   es_dwconv                 depthwise 3x3 (stride 1 | 2) and 5x5: bandwidth-bound; a thread owns 8 channels (one 16-byte load per tap) of
//                             1, 2 or 4 neighbouring output pixels of a row, so the input row segment it loads serves every tap of all of
//                             them; neighbouring threads re-read their overlap from L1 / L2, never from HBM
//   es_relu_linear_attention  LiteMLA.relu_linear_att: a workgroup per (32 tokens, group, image) sums kv = relu(k)^T [v | 1] over ALL tokens
//                             in fp32 (64-token tiles through LDS; 33 x 32 accumulators across 256 threads), then applies it to its 32
//                             queries: HW / 32 x groups workgroups at n = 1 instead of `groups`, at the price of re-summing kv (2 HW 32 33
//                             MACs: nothing) - and no second launch, no kv round trip through memory
//   es_sam_neck_merge         the three projected maps resampled with torch's bicubic and summed, one rounding
//   es_sam_encoder            the builder (state dict -> BatchNorm folded in fp64 -> weights packed for es_conv_gemm, one arena) and the
//                             forward.  Every dense convolution is es_conv_gemm with the tile es_launch_choose gives for ONE image's
//                             launch, whatever the batch: the K order of every output element is then the same at every batch size, so
//                             image i of a batch equals the image encoded alone bit for bit.  tanh-GELU and the identity shortcuts are
//                             the GEMM's epilogue (ES_ACT_GELU_TANH, `residual`).  The grouped 1x1 of LiteMLA.aggreg is a block-diagonal
//                             dense weight (exact zeros) on es_conv_gemm.
// None of these calls is ever part of a plan: while a plan records on the calling thread they return -1.
#include "encoder.h"

using namespace es_enc;

namespace {

const char* const kRecording = "a plan is recording on this thread; the SAM encoder calls are never part of a plan";
constexpr int NECK = 64;          // SamNeck's UpSampleLayer(size=(64, 64)), sam.py:127
constexpr int QD = 32;            // qkv_dim

template <typename T> ES_DEVICE void unpack8(const u32x4 v, float* f) {
  const auto h = as_vec8<T>(v);
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = to_f32(h[e]);
}

// ---- depthwise convolution ------------------------------------------------------------------------------------------------------
// item = (n, oy, group of TW output columns, 8 channels); consecutive threads take consecutive channel octets: every load and the store
// of a wave are contiguous runs of C * 2 bytes.  Taps outside the image add an exact 0; rows outside it are skipped.
template <typename T, int K, int S, int TW>
__global__ __launch_bounds__(256) void dwconv_kernel(const T* __restrict__ x, const T* __restrict__ w, const float* __restrict__ bias, T* __restrict__ out,
                                                     const int H, const int W, const int C, const int Ho, const int Wo, const int wt,
                                                     const long long total, const int act) {
  constexpr int P = K / 2, NI = (TW - 1) * S + K;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int C8 = C >> 3;
  const int c8 = (int)(idx % C8);
  long long r = idx / C8;
  const int xt = (int)(r % wt); r /= wt;
  const int oy = (int)(r % Ho);
  const long long n = r / Ho;
  const int ox0 = xt * TW;
  float acc[TW][8];
#pragma unroll
  for (int t = 0; t < TW; ++t)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[t][e] = 0.f;
#pragma unroll
  for (int ky = 0; ky < K; ++ky) {
    const int iy = oy * S + ky - P;
    if (iy < 0 || iy >= H) continue;
    const T* row = x + ((size_t)(n * H + iy) * W) * C + (size_t)c8 * 8;
    u32x4 in[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int ix = ox0 * S - P + i;
      in[i] = (ix >= 0 && ix < W) ? *(const u32x4*)(row + (size_t)ix * C) : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int kx = 0; kx < K; ++kx) {
      float wf[8];
      unpack8<T>(*(const u32x4*)(w + (size_t)(ky * K + kx) * C + (size_t)c8 * 8), wf);
#pragma unroll
      for (int t = 0; t < TW; ++t) {
        float v[8];
        unpack8<T>(in[t * S + kx], v);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[t][e] = __builtin_fmaf(v[e], wf[e], acc[t][e]);
      }
    }
  }
  float bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (bias) {
    const f32x4 b0 = *(const f32x4*)(bias + (size_t)c8 * 8), b1 = *(const f32x4*)(bias + (size_t)c8 * 8 + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { bv[e] = b0[e]; bv[4 + e] = b1[e]; }
  }
#pragma unroll
  for (int t = 0; t < TW; ++t) {
    if (ox0 + t >= Wo) break;
    typename Traits<T>::vec8 pk;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float y = acc[t][e] + bv[e];
      if (act == ES_ACT_GELU_TANH) y = gelu_tanh_f(y);
      pk[e] = from_f32<T>(y);
    }
    *(u32x4*)(out + (((size_t)(n * Ho + oy) * Wo + ox0 + t) * C + (size_t)c8 * 8)) = __builtin_bit_cast(u32x4, pk);
  }
}

template <typename T, int K, int S>
int launch_dwconv(const void* x, const void* w, const float* bias, void* out, int N, int H, int W, int C, int act, hipStream_t st) {
  const int Ho = (H + 2 * (K / 2) - K) / S + 1, Wo = (W + 2 * (K / 2) - K) / S + 1;
  const long long rows = (long long)N * Ho * (C / 8);
  // 4 columns per thread while that still fills the chip four times over, else 2, else 1 (the result does not depend on it)
  int tw = 4;
  if (rows * ((Wo + 3) / 4) < 4 * 256 * 256) tw = 2;
  if (tw == 2 && rows * ((Wo + 1) / 2) < 2 * 256 * 256) tw = 1;
  const int wt = (Wo + tw - 1) / tw;
  const long long total = rows * wt;
  if ((total + 255) / 256 > 0x7fffffffll) return -3;
  const dim3 grid((unsigned)((total + 255) / 256));
#define ES_DW(TW) hipLaunchKernelGGL((dwconv_kernel<T, K, S, TW>), grid, dim3(256), 0, st, (const T*)x, (const T*)w, bias, (T*)out, H, W, C, Ho, Wo, wt, total, act)
  if (tw == 4) ES_DW(4); else if (tw == 2) ES_DW(2); else ES_DW(1);
#undef ES_DW
  return ES_CHECK_LAUNCH();
}

template <typename T>
int dwconv_dispatch(const void* x, const void* w, const float* bias, void* out, int N, int H, int W, int C, int k, int stride, int act, hipStream_t st) {
  if (k == 3 && stride == 1) return launch_dwconv<T, 3, 1>(x, w, bias, out, N, H, W, C, act, st);
  if (k == 3) return launch_dwconv<T, 3, 2>(x, w, bias, out, N, H, W, C, act, st);
  return launch_dwconv<T, 5, 1>(x, w, bias, out, N, H, W, C, act, st);
}

// ---- ReLU linear attention --------------------------------------------------------------------------------------------------------
// grid (ceil(HW / 32), 2 * heads, N), 256 threads.  Phase 1, thread (i = tid / 8, jb = tid % 8): kv[i][4 jb .. 4 jb + 3] and ksum[i] over the
// tokens IN ORDER (the same order in every workgroup and at every batch size).  Phase 2, thread (token tid / 8, jb): 4 outputs.
template <typename T>
__global__ __launch_bounds__(256) void relu_att_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ out, const int HW, const int heads) {
  constexpr int TT = 64;
  __shared__ __attribute__((aligned(16))) float ks[TT][QD];
  __shared__ __attribute__((aligned(16))) float vs[TT][QD];
  __shared__ __attribute__((aligned(16))) float kvs[QD][QD + 4];     // [i][0..31] kv, [i][32] the sum of relu(k_i)
  __shared__ __attribute__((aligned(16))) float qs[32][QD + 1];
  const int tid = threadIdx.x, g = blockIdx.y;
  const size_t n = blockIdx.z;
  const int C3 = 3 * heads * QD;
  const T* src = (g < heads ? a : b) + n * (size_t)HW * C3 + (size_t)(g < heads ? g : g - heads) * 3 * QD;
  const int i = tid >> 3, jb = tid & 7;
  float acc[4] = {0.f, 0.f, 0.f, 0.f}, ksum = 0.f;
  for (int t0 = 0; t0 < HW; t0 += TT) {
    for (int it = tid; it < TT * 8; it += 256) {          // k: chunks 0..3 of channels 32..63, v: chunks 4..7 of channels 64..95
      const int tt = it >> 3, ch = it & 7, t = t0 + tt;
      float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (t < HW) unpack8<T>(*(const u32x4*)(src + (size_t)t * C3 + QD + ch * 8), f);
      float* dst = ch < 4 ? &ks[tt][ch * 8] : &vs[tt][(ch - 4) * 8];
#pragma unroll
      for (int e = 0; e < 8; ++e) dst[e] = ch < 4 ? fmaxf(f[e], 0.f) : f[e];
    }
    __syncthreads();
    const int tend = HW - t0 < TT ? HW - t0 : TT;
    for (int tt = 0; tt < tend; ++tt) {
      const float kk = ks[tt][i];
      const f32x4 v4 = *(const f32x4*)&vs[tt][jb * 4];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(kk, v4[e], acc[e]);
      ksum += kk;
    }
    __syncthreads();
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) kvs[i][jb * 4 + e] = acc[e];
  if (jb == 0) kvs[i][QD] = ksum;
  const int tq0 = blockIdx.x * 32;
  if (tid < 128) {
    const int tt = tid >> 2, ch = tid & 3, t = tq0 + tt;
    float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (t < HW) unpack8<T>(*(const u32x4*)(src + (size_t)t * C3 + ch * 8), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) qs[tt][ch * 8 + e] = fmaxf(f[e], 0.f);
  }
  __syncthreads();
  const int t = tq0 + i;            // (i: this thread's token of the 32)
  float o[4] = {0.f, 0.f, 0.f, 0.f}, den = 0.f;
#pragma unroll 8
  for (int c = 0; c < QD; ++c) {
    const float qq = qs[i][c];
    const f32x4 k4 = *(const f32x4*)&kvs[c][jb * 4];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = __builtin_fmaf(qq, k4[e], o[e]);
    den = __builtin_fmaf(qq, kvs[c][QD], den);
  }
  if (t < HW) {
    const float d = den + 1.0e-15f;
    typename Traits<T>::vec4 pk;
#pragma unroll
    for (int e = 0; e < 4; ++e) pk[e] = from_f32<T>(o[e] / d);
    *(u32x2*)(out + (n * HW + t) * (size_t)(2 * heads * QD) + (size_t)g * QD + jb * 4) = __builtin_bit_cast(u32x2, pk);
  }
}

// ---- neck merge -------------------------------------------------------------------------------------------------------------------
struct NeckDesc { const void* m[3]; int32_t h[3], w[3], count; };

// torch's upsample_bicubic2d, align_corners = False: source coordinate scale * (o + 0.5) - 0.5 (not clamped), the Keys kernel with A = -0.75
ES_DEVICE void cubic_coeffs(const int o, const int in, int* i0, float c[4]) {
  const float scale = (float)in / (float)NECK;
  const float real = scale * ((float)o + 0.5f) - 0.5f;
  const float fl = floorf(real);
  const float t = real - fl;
  constexpr float A = -0.75f;
  const float x0 = t + 1.0f, x1 = t, x2 = 1.0f - t, x3 = 2.0f - t;
  c[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
  c[1] = ((A + 2.0f) * x1 - (A + 3.0f)) * x1 * x1 + 1.0f;
  c[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
  c[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
  *i0 = (int)fl - 1;
}

template <typename T>
__global__ __launch_bounds__(256) void neck_merge_kernel(const NeckDesc d, T* __restrict__ out, const int C, const long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int C8 = C >> 3;
  const int c8 = (int)(idx % C8);
  const long long pix = idx / C8;
  const int ox = (int)(pix % NECK), oy = (int)((pix / NECK) % NECK);
  const size_t n = (size_t)(pix / (NECK * NECK));
  float val[3][8];
#pragma unroll
  for (int s = 0; s < 3; ++s) {
#pragma unroll
    for (int e = 0; e < 8; ++e) val[s][e] = 0.f;
    if (s >= d.count) continue;
    const int h = d.h[s], w = d.w[s];
    const T* base = (const T*)d.m[s] + n * (size_t)h * w * C + (size_t)c8 * 8;
    if (h == NECK && w == NECK) {
      unpack8<T>(*(const u32x4*)(base + ((size_t)oy * NECK + ox) * C), val[s]);
      continue;
    }
    int y0, x0;
    float cy[4], cx[4];
    cubic_coeffs(oy, h, &y0, cy);
    cubic_coeffs(ox, w, &x0, cx);
#pragma unroll
    for (int ky = 0; ky < 4; ++ky) {
      int yy = y0 + ky;
      yy = yy < 0 ? 0 : (yy > h - 1 ? h - 1 : yy);
      float rowv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kx = 0; kx < 4; ++kx) {
        int xx = x0 + kx;
        xx = xx < 0 ? 0 : (xx > w - 1 ? w - 1 : xx);
        float f[8];
        unpack8<T>(*(const u32x4*)(base + ((size_t)yy * w + xx) * C), f);
#pragma unroll
        for (int e = 0; e < 8; ++e) rowv[e] = __builtin_fmaf(cx[kx], f[e], rowv[e]);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) val[s][e] = __builtin_fmaf(cy[ky], rowv[e], val[s][e]);
    }
  }
  typename Traits<T>::vec8 pk;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    // list_sum (efficientvit/models/utils/list.py:16-17): x[0] + (x[1] + x[2])
    const float sum = d.count == 1 ? val[0][e] : (d.count == 2 ? val[0][e] + val[1][e] : val[0][e] + (val[1][e] + val[2][e]));
    pk[e] = from_f32<T>(sum);
  }
  *(u32x4*)(out + (size_t)idx * 8) = __builtin_bit_cast(u32x4, pk);
}

// ---- the builder's records ----------------------------------------------------------------------------------------------------------
struct Conv { size_t w = 0, bias = 0; int cout = 0, cin = 0, k = 1, stride = 1, rows_padded = 0, kpad = 0; };      // dense, packed for es_conv_gemm
struct DW { size_t w = 0, bias = 0; int c = 0, k = 3, stride = 1; };                                                 // depthwise: [k * k][C] dtype
struct ResB { Conv c1, c2; };
struct FMB { Conv spatial, point; bool shortcut = false; };
struct MB { Conv inverted, point; DW depth; bool shortcut = false; };
struct MLA { Conv qkv, group, proj; DW agg; };
struct VitBlock { MLA att; MB local; };

}  // namespace

struct es_sam_encoder {
  es_sam_config cfg;
  int dtype = ES_F16, max_n = 0, device = -1;
  size_t arena_bytes = 0, ws_bytes = 0;
  char* arena = nullptr;
  es_launch_knobs knobs;
  bool sizing = false;              // the forward only asks the launch policy (es_sam_encoder_create: the split-K workspace)
  Conv stem;
  std::vector<ResB> stage0;
  std::vector<FMB> stage12[2];
  std::vector<MB> stage3;
  MB stage4_first;
  std::vector<VitBlock> stage4;
  Conv neck_in[3], neck_out;
  std::vector<FMB> neck_mid;
  size_t ln_g = 0, ln_b = 0;
  // activations (arena offsets)
  size_t xin = 0, s[2] = {0, 0}, m[2] = {0, 0}, stage[3] = {0, 0, 0} /* stage2, stage3, stage4 */, qkv = 0, agg0 = 0, agg = 0, att = 0;
  size_t np[3] = {0, 0, 0}, nk[2] = {0, 0}, nm = 0, no = 0, nl = 0, ws = 0;
};

namespace {

struct SamBuilder : EncBuilder {
  double bn_eps = 1e-6;
  bool has(const std::string& k) const { return m.count(k) != 0; }
  // weight [cout][cin_g][k][k] and bias [cout] of ConvLayer `p` (raw: a bare Conv2d, keys p.weight / p.bias) with its BatchNorm, where it has
  // one, folded in, in fp64: W gamma / sqrt(var + eps), beta + (b - mean) gamma / sqrt(var + eps)
  bool load(const std::string& p, bool raw, int cout, int cin_g, int k, std::vector<double>* w, std::vector<double>* b) {
    const std::string wk = p + (raw ? ".weight" : ".conv.weight"), bk = p + (raw ? ".bias" : ".conv.bias"), nk = p + ".norm.";
    std::vector<float> wf = get(wk, cout, cin_g, k, k);
    if (wf.empty()) return false;
    w->assign(wf.begin(), wf.end());
    b->assign((size_t)cout, 0.0);
    if (has(bk)) {
      std::vector<float> bf = get(bk, cout);
      if (bf.empty()) return false;
      for (int r = 0; r < cout; ++r) (*b)[r] = bf[r];
    }
    if (!raw && (has(nk + "weight") || has(nk + "running_var") || has(nk + "running_mean") || has(nk + "bias"))) {
      std::vector<float> g = get(nk + "weight", cout); if (g.empty()) return false;
      std::vector<float> bt = get(nk + "bias", cout); if (bt.empty()) return false;
      std::vector<float> mu = get(nk + "running_mean", cout); if (mu.empty()) return false;
      std::vector<float> var = get(nk + "running_var", cout); if (var.empty()) return false;
      const size_t per = (size_t)cin_g * k * k;
      for (int r = 0; r < cout; ++r) {
        if (!((double)var[r] + bn_eps > 0.0)) { err = "'" + nk + "running_var' + eps is not positive"; return false; }
        const double sc = (double)g[r] / sqrt((double)var[r] + bn_eps);
        for (size_t j = 0; j < per; ++j) (*w)[(size_t)r * per + j] *= sc;
        (*b)[r] = (double)bt[r] + ((*b)[r] - (double)mu[r]) * sc;
      }
    }
    return true;
  }
  // w [cout][cin][k][k] -> [rows_padded][kpad], K tap-major over cin padded to cp channels; the bias is always there (zeros where the layer has none)
  Conv pack_dense(const std::vector<double>& w, const std::vector<double>& b, int cout, int cin, int k, int stride, int cp) {
    Conv L;
    L.cout = cout; L.cin = cp; L.k = k; L.stride = stride;
    L.rows_padded = round_up(cout, es_policy::choose_bn(cout)); L.kpad = round_up(k * k * cp, BK);
    L.w = alloc((size_t)L.rows_padded * L.kpad * 2);
    uint16_t* dw = (uint16_t*)staged(L.w, (size_t)L.rows_padded * L.kpad * 2);
    L.bias = alloc((size_t)L.rows_padded * 4);
    float* db = (float*)staged(L.bias, (size_t)L.rows_padded * 4);
    for (int r = 0; r < cout; ++r) {
      for (int t = 0; t < k * k; ++t)
        for (int ci = 0; ci < cin; ++ci) dw[(size_t)r * L.kpad + (size_t)t * cp + ci] = enc((float)w[((size_t)r * cin + ci) * k * k + t]);
      db[r] = (float)b[r];
    }
    return L;
  }
  bool conv(const std::string& p, int cin, int cout, int k, int stride, Conv* out) {
    std::vector<double> w, b;
    if (!load(p, false, cout, cin, k, &w, &b)) return false;
    *out = pack_dense(w, b, cout, cin, k, stride, round_up(cin, 8));
    return true;
  }
  bool dwconv(const std::string& p, bool raw, int c, int k, int stride, DW* out) {
    std::vector<double> w, b;
    if (!load(p, raw, c, 1, k, &w, &b)) return false;
    out->c = c; out->k = k; out->stride = stride;
    out->w = alloc((size_t)k * k * c * 2);
    uint16_t* dw = (uint16_t*)staged(out->w, (size_t)k * k * c * 2);
    for (int ch = 0; ch < c; ++ch)
      for (int t = 0; t < k * k; ++t) dw[(size_t)t * c + ch] = enc((float)w[(size_t)ch * k * k + t]);
    std::vector<float> bf(b.begin(), b.end());
    out->bias = upload_f32(std::move(bf));
    return true;
  }
  // nn.Conv2d(c, c, 1, groups = c / 32) as a block-diagonal dense weight
  bool grouped(const std::string& p, int c, Conv* out) {
    std::vector<double> w, b;
    if (!load(p, true, c, QD, 1, &w, &b)) return false;
    std::vector<double> dense((size_t)c * c, 0.0);
    for (int r = 0; r < c; ++r)
      for (int j = 0; j < QD; ++j) dense[(size_t)r * c + (size_t)(r / QD) * QD + j] = w[(size_t)r * QD + j];
    *out = pack_dense(dense, b, c, c, 1, 1, c);
    return true;
  }
  bool fmb(const std::string& p, int cin, int cout, int stride, int expand, bool shortcut, FMB* out) {
    out->shortcut = shortcut;
    return conv(p + ".main.spatial_conv", cin, cin * expand, 3, stride, &out->spatial) && conv(p + ".main.point_conv", cin * expand, cout, 1, 1, &out->point);
  }
  bool mb(const std::string& p, int cin, int cout, int stride, int expand, bool shortcut, MB* out) {
    out->shortcut = shortcut;
    return conv(p + ".main.inverted_conv", cin, cin * expand, 1, 1, &out->inverted) && dwconv(p + ".main.depth_conv", false, cin * expand, 3, stride, &out->depth) &&
           conv(p + ".main.point_conv", cin * expand, cout, 1, 1, &out->point);
  }
};

int out_size(int h, int k, int stride) { return (h + 2 * (k / 2) - k) / stride + 1; }

// one dense convolution over n images of H x W: the tile is the launch policy's answer for ONE image (see the head of this file)
int conv(const char* who, es_sam_encoder* e, const Conv& L, const void* x, int n, int H, int W, void* out, const void* residual, int act, hipStream_t st) {
  const int Ho = out_size(H, L.k, L.stride), Wo = out_size(W, L.k, L.stride);
  es_launch_query q;
  memset(&q, 0, sizeof(q));
  q.M = (long long)Ho * Wo; q.hw = q.M; q.w_numel = (long long)L.rows_padded * L.kpad; q.src_numel = (long long)H * W * L.cin;
  q.ksize = L.k; q.stride = L.stride; q.C1 = L.cin; q.rows_padded = L.rows_padded; q.kpad = L.kpad; q.cin = L.cin; q.cout = L.cout;
  q.act = act; q.has_residual = residual != nullptr; q.residual_dense = 1; q.unit_scale = 1; q.x_rep = 1; q.dtype = e->dtype;
  es_launch_choice ch;
  if (es_launch_choose(&q, &e->knobs, &ch)) return fail(-1, who, std::string("the launch policy has no tile for a convolution: ") + es_last_error());
  if (ch.route != ES_ROUTE_CONV_GEMM) return fail(-1, who, "the launch policy routed a convolution away from es_conv_gemm");
  const size_t M = (size_t)n * Ho * Wo;
  if (e->sizing) {
    if (ch.splitk > 1) e->ws_bytes = std::max(e->ws_bytes, (size_t)ch.splitk * M * L.rows_padded * 4);
    return 0;
  }
  es_gemm_desc d;
  memset(&d, 0, sizeof(d));
  d.x = x; d.out = out; d.residual = residual; d.w = e->arena + L.w; d.bias = (const float*)(e->arena + L.bias);
  d.N = n; d.Hsrc = H; d.Wsrc = W; d.C1 = L.cin; d.Hout = Ho; d.Wout = Wo; d.Cout = L.cout;
  d.rows_padded = L.rows_padded; d.Kpad = L.kpad; d.ksize = L.k; d.stride = L.stride; d.pad = L.k / 2;
  d.act = act; d.splitk = ch.splitk; d.bn = ch.bn; d.dtype = e->dtype; d.out_scale = 1.f; d.stages = ch.stages;
  d.waves = ch.waves; d.xcd_m_fastest = ch.xcd_m_fastest;
  if (ch.splitk > 1) {
    if (es_conv_gemm_workspace_bytes(&d) > e->ws_bytes) return fail(-1, who, "split-K workspace smaller than the launch needs");
    d.workspace = (float*)(e->arena + e->ws);
  }
  return es_conv_gemm(&d, st);
}

int dw(es_sam_encoder* e, const DW& L, const void* x, int n, int H, int W, void* out, int act, hipStream_t st) {
  if (e->sizing) return 0;
  return es_dwconv(x, e->arena + L.w, (const float*)(e->arena + L.bias), out, n, H, W, L.c, L.k, L.stride, act, e->dtype, st);
}

// the whole network from the stem's NHWC input in e->xin; out_nchw may be NULL (sizing)
int forward(const char* who, es_sam_encoder* e, int n, float* out_nchw, hipStream_t st) {
  char* A = e->arena;
  const es_sam_config& c = e->cfg;
  int H = c.image_size, rc;
  const int G = ES_ACT_GELU_TANH, NA = ES_ACT_NONE;
  auto other = [&](const char* cur) { return cur == A + e->s[0] ? A + e->s[1] : A + e->s[0]; };
  char *m0 = A + e->m[0], *m1 = A + e->m[1];
#define ES_RUN(call) do { if ((rc = (call))) return rc; } while (0)
  char* cur = A + e->s[0];
  ES_RUN(conv(who, e, e->stem, A + e->xin, n, H, H, cur, nullptr, G, st));
  H /= 2;
  for (const ResB& b : e->stage0) {
    char* dst = other(cur);
    ES_RUN(conv(who, e, b.c1, cur, n, H, H, m0, nullptr, G, st));
    ES_RUN(conv(who, e, b.c2, m0, n, H, H, dst, cur, NA, st));
    cur = dst;
  }
  auto run_fmb = [&](const FMB& b, char* dst) {
    int r = conv(who, e, b.spatial, cur, n, H, H, m0, nullptr, G, st);
    const int Ho = out_size(H, 3, b.spatial.stride);
    if (!r) r = conv(who, e, b.point, m0, n, Ho, Ho, dst, b.shortcut ? cur : nullptr, NA, st);
    H = Ho; cur = dst;
    return r;
  };
  auto run_mb = [&](const MB& b, char* dst) {
    int r = conv(who, e, b.inverted, cur, n, H, H, m0, nullptr, G, st);
    if (!r) r = dw(e, b.depth, m0, n, H, H, m1, G, st);
    const int Ho = out_size(H, 3, b.depth.stride);
    if (!r) r = conv(who, e, b.point, m1, n, Ho, Ho, dst, b.shortcut ? cur : nullptr, NA, st);
    H = Ho; cur = dst;
    return r;
  };
  for (int s = 0; s < 2; ++s)
    for (size_t i = 0; i < e->stage12[s].size(); ++i)
      ES_RUN(run_fmb(e->stage12[s][i], (s == 1 && i + 1 == e->stage12[s].size()) ? A + e->stage[0] : other(cur)));
  const int H2 = H;
  for (size_t i = 0; i < e->stage3.size(); ++i) ES_RUN(run_mb(e->stage3[i], i + 1 == e->stage3.size() ? A + e->stage[1] : other(cur)));
  const int H3 = H;
  ES_RUN(run_mb(e->stage4_first, e->stage4.empty() ? A + e->stage[2] : other(cur)));
  const int H4 = H, HW4 = H * H, heads = c.width[4] / QD;
  for (size_t i = 0; i < e->stage4.size(); ++i) {
    const VitBlock& b = e->stage4[i];
    char* dst = other(cur);
    ES_RUN(conv(who, e, b.att.qkv, cur, n, H, H, A + e->qkv, nullptr, NA, st));
    ES_RUN(dw(e, b.att.agg, A + e->qkv, n, H, H, A + e->agg0, NA, st));
    ES_RUN(conv(who, e, b.att.group, A + e->agg0, n, H, H, A + e->agg, nullptr, NA, st));
    if (!e->sizing) ES_RUN(es_relu_linear_attention(A + e->qkv, A + e->agg, A + e->att, n, HW4, heads, e->dtype, st));
    ES_RUN(conv(who, e, b.att.proj, A + e->att, n, H, H, dst, cur, NA, st));
    cur = dst;
    ES_RUN(run_mb(b.local, i + 1 == e->stage4.size() ? A + e->stage[2] : other(cur)));
  }
  // neck
  const int hs[3] = {H4, H3, H2};
  for (int j = 0; j < 3; ++j) ES_RUN(conv(who, e, e->neck_in[j], A + e->stage[2 - j], n, hs[j], hs[j], A + e->np[j], nullptr, NA, st));
  cur = A + e->nk[0];
  if (!e->sizing) {
    const void* maps[3] = {A + e->np[0], A + e->np[1], A + e->np[2]};
    ES_RUN(es_sam_neck_merge(maps, hs, hs, 3, cur, n, c.head_width, e->dtype, st));
  }
  for (const FMB& b : e->neck_mid) {
    char* dst = cur == A + e->nk[0] ? A + e->nk[1] : A + e->nk[0];
    ES_RUN(conv(who, e, b.spatial, cur, n, NECK, NECK, A + e->nm, nullptr, G, st));
    ES_RUN(conv(who, e, b.point, A + e->nm, n, NECK, NECK, dst, cur, NA, st));
    cur = dst;
  }
  ES_RUN(conv(who, e, e->neck_out, cur, n, NECK, NECK, A + e->no, nullptr, NA, st));
  if (e->sizing) return 0;
  ES_RUN(es_layer_norm(A + e->no, A + e->nl, (const float*)(A + e->ln_g), (const float*)(A + e->ln_b), n * NECK * NECK, c.out_dim, c.ln_eps, e->dtype, st));
  return es_nhwc_to_nchw_f32(A + e->nl, out_nchw, n, c.out_dim, NECK * NECK, c.out_dim, 1.f, 0.f, 0, e->dtype, st);
#undef ES_RUN
}

int ready(const char* who, const es_sam_encoder* e, int n) {
  if (es_plan_recording()) return fail(-1, who, kRecording);
  if (n < 1 || n > e->max_n) return fail(-1, who, "n = " + std::to_string(n) + " is outside 1..max_n = " + std::to_string(e->max_n));
  if (!e->arena) return fail(-1, who, "this encoder is a dry build (es_sam_encoder_create device -1): it holds no device memory and cannot run");
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev != e->device) return fail(-1, who, "the current device is not the one the encoder was built on");
  return 0;
}

}  // namespace

extern "C" int es_dwconv(const void* x, const void* w, const float* bias, void* out, int N, int H, int W, int C, int k, int stride, int act, int dtype, void* stream) {
  const char* who = "es_dwconv";
  if (es_plan_recording()) return fail(-1, who, kRecording);
  if (!x || !w || !out) return fail(-1, who, "null pointer");
  if (dtype != ES_F16 && dtype != ES_BF16) return fail(-1, who, "dtype must be ES_F16 or ES_BF16");
  if (!((k == 3 && (stride == 1 || stride == 2)) || (k == 5 && stride == 1))) return fail(-1, who, "k = 3 with stride 1 | 2, or k = 5 with stride 1");
  if (act != ES_ACT_NONE && act != ES_ACT_GELU_TANH) return fail(-1, who, "act must be ES_ACT_NONE or ES_ACT_GELU_TANH");
  if (N < 1 || H < 1 || W < 1 || C < 8 || C % 8) return fail(-1, who, "N, H, W >= 1 and C a positive multiple of 8");
  if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)out | (uintptr_t)bias) & 15) return fail(-1, who, "x, w, bias and out must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int rc = dtype == ES_F16 ? dwconv_dispatch<f16>(x, w, bias, out, N, H, W, C, k, stride, act, st) : dwconv_dispatch<bf16>(x, w, bias, out, N, H, W, C, k, stride, act, st);
  if (rc == -3) return fail(-1, who, "too many elements for one launch");
  if (rc) return fail(-2, who, "launch failed");
  return 0;
}

extern "C" int es_relu_linear_attention(const void* a, const void* b, void* out, int N, int HW, int heads, int dtype, void* stream) {
  const char* who = "es_relu_linear_attention";
  if (es_plan_recording()) return fail(-1, who, kRecording);
  if (!a || !b || !out) return fail(-1, who, "null pointer");
  if (dtype != ES_F16 && dtype != ES_BF16) return fail(-1, who, "dtype must be ES_F16 or ES_BF16");
  if (N < 1 || N > 65535 || HW < 1 || HW > (1 << 24) || heads < 1 || heads > 1024) return fail(-1, who, "N in 1..65535, HW in 1..2^24, heads in 1..1024");
  if (((uintptr_t)a | (uintptr_t)b) & 15 || ((uintptr_t)out & 7)) return fail(-1, who, "a and b must be 16-byte aligned, out 8-byte aligned");
  const dim3 grid((unsigned)((HW + 31) / 32), (unsigned)(2 * heads), (unsigned)N);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == ES_F16) hipLaunchKernelGGL(relu_att_kernel<f16>, grid, dim3(256), 0, st, (const f16*)a, (const f16*)b, (f16*)out, HW, heads);
  else hipLaunchKernelGGL(relu_att_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)a, (const bf16*)b, (bf16*)out, HW, heads);
  if (ES_CHECK_LAUNCH()) return fail(-2, who, "launch failed");
  return 0;
}

extern "C" int es_sam_neck_merge(const void* const* maps, const int32_t* hs, const int32_t* ws, int count, void* out, int N, int C, int dtype, void* stream) {
  const char* who = "es_sam_neck_merge";
  if (es_plan_recording()) return fail(-1, who, kRecording);
  if (!maps || !hs || !ws || !out) return fail(-1, who, "null pointer");
  if (dtype != ES_F16 && dtype != ES_BF16) return fail(-1, who, "dtype must be ES_F16 or ES_BF16");
  if (count < 1 || count > 3) return fail(-1, who, "count must be 1, 2 or 3 maps");
  if (N < 1 || C < 8 || C % 8) return fail(-1, who, "N >= 1 and C a positive multiple of 8");
  NeckDesc d;
  memset(&d, 0, sizeof(d));
  d.count = count;
  for (int i = 0; i < count; ++i) {
    if (!maps[i] || ((uintptr_t)maps[i] & 15)) return fail(-1, who, "a map is null or not 16-byte aligned");
    if (hs[i] < 1 || ws[i] < 1 || hs[i] > NECK || ws[i] > NECK) return fail(-1, who, "a map's height and width must be in 1..64");
    d.m[i] = maps[i]; d.h[i] = hs[i]; d.w[i] = ws[i];
  }
  if ((uintptr_t)out & 15) return fail(-1, who, "out must be 16-byte aligned");
  const long long total = (long long)N * NECK * NECK * (C / 8);
  if ((total + 255) / 256 > 0x7fffffffll) return fail(-1, who, "too many elements for one launch");
  const dim3 grid((unsigned)((total + 255) / 256));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == ES_F16) hipLaunchKernelGGL(neck_merge_kernel<f16>, grid, dim3(256), 0, st, d, (f16*)out, C, total);
  else hipLaunchKernelGGL(neck_merge_kernel<bf16>, grid, dim3(256), 0, st, d, (bf16*)out, C, total);
  if (ES_CHECK_LAUNCH()) return fail(-2, who, "launch failed");
  return 0;
}

extern "C" void es_sam_encoder_destroy(es_sam_encoder* e) {
  if (!e) return;
  if (e->arena) (void)hipFree(e->arena);
  delete e;
}

extern "C" size_t es_sam_encoder_arena_bytes(const es_sam_encoder* e) { return e ? e->arena_bytes : 0; }

extern "C" int es_sam_encoder_create(const es_state_dict* sd, const es_sam_config* cfg, int dtype, int max_n, int device, es_sam_encoder** out) {
  const char* who = "es_sam_encoder_create";
  if (out) *out = nullptr;
  if (!sd || !cfg || !out) return fail(-1, who, "null pointer");
  if (es_plan_recording()) return fail(-1, who, kRecording);
  if (dtype != ES_F16 && dtype != ES_BF16) return fail(-1, who, "dtype must be ES_F16 or ES_BF16");
  if (device < -1) return fail(-1, who, "device must be >= 0, or -1 for a dry build");
  const int S = cfg->image_size;
  const int* w = cfg->width;
  for (int i = 0; i < 5; ++i) {
    if (w[i] < 32 || w[i] % 32 || w[i] > 2048) return fail(-1, who, "width[" + std::to_string(i) + "] = " + std::to_string(w[i]) + " must be a multiple of 32 in 32..2048");
    if (cfg->depth[i] < 0 || cfg->depth[i] > 64) return fail(-1, who, "depth[" + std::to_string(i) + "] must be in 0..64");
  }
  if (cfg->qkv_dim != QD) return fail(-1, who, "qkv_dim must be 32 (es_relu_linear_attention)");
  if (S < 64 || S > 512 || S % 32) return fail(-1, who, "image_size = " + std::to_string(S) + " must be a multiple of 32 in 64..512 (the neck's output is 64 x 64 whatever the input: sam.py:127)");
  if (cfg->head_width < 8 || cfg->head_width % 8 || cfg->head_width > 4096) return fail(-1, who, "head_width must be a multiple of 8 in 8..4096");
  if (cfg->head_depth < 0 || cfg->head_depth > 64) return fail(-1, who, "head_depth must be in 0..64");
  if (cfg->out_dim < 8 || cfg->out_dim % 8 || cfg->out_dim > 4096) return fail(-1, who, "out_dim must be a multiple of 8 in 8..4096 (es_layer_norm)");
  if (max_n < 1 || max_n > 1024) return fail(-1, who, "max_n must be in 1..1024");
  if (!(cfg->bn_eps > 0.f) || !(cfg->ln_eps > 0.f)) return fail(-1, who, "bn_eps and ln_eps must be positive");
  for (int i = 0; i < 3; ++i) if (!(cfg->pixel_std[i] > 0.f)) return fail(-1, who, "pixel_std must be positive");

  SamBuilder b;
  b.dt = dtype; b.bn_eps = (double)cfg->bn_eps;
  if (!b.init(sd, "image_encoder.")) return fail(-1, who, b.err);
  std::unique_ptr<es_sam_encoder, void (*)(es_sam_encoder*)> e(new es_sam_encoder, es_sam_encoder_destroy);
  e->cfg = *cfg; e->dtype = dtype; e->max_n = max_n; e->device = device;
  default_knobs(&e->knobs);

#define ES_NEED(call) do { if (!(call)) return fail(-1, who, b.err); } while (0)
  {
    std::vector<double> sw, sb;                     // the stem reads the 3 colour planes as an 8-channel NHWC tensor (channels 3..7 are zero)
    ES_NEED(b.load("backbone.stages.0.op_list.0", false, w[0], 3, 3, &sw, &sb));
    e->stem = b.pack_dense(sw, sb, w[0], 3, 3, 2, 8);
  }
  for (int i = 0; i < cfg->depth[0]; ++i) {
    const std::string p = "backbone.stages.0.op_list." + std::to_string(1 + i);
    ResB r;
    ES_NEED(b.conv(p + ".main.conv1", w[0], w[0], 3, 1, &r.c1));
    ES_NEED(b.conv(p + ".main.conv2", w[0], w[0], 3, 1, &r.c2));
    e->stage0.push_back(r);
  }
  int cin = w[0];
  for (int s = 1; s <= 3; ++s) {
    for (int i = 0; i < cfg->depth[s] + 1; ++i) {
      const std::string p = "backbone.stages." + std::to_string(s) + ".op_list." + std::to_string(i);
      const int stride = i == 0 ? 2 : 1, expand = i == 0 ? 16 : 4;
      if (s <= 2) { FMB f; ES_NEED(b.fmb(p, cin, w[s], stride, expand, stride == 1, &f)); e->stage12[s - 1].push_back(f); }
      else { MB f; ES_NEED(b.mb(p, cin, w[s], stride, expand, stride == 1, &f)); e->stage3.push_back(f); }
      cin = w[s];
    }
  }
  ES_NEED(b.mb("backbone.stages.4.op_list.0", cin, w[4], 2, 24, false, &e->stage4_first));
  for (int i = 0; i < cfg->depth[4]; ++i) {
    const std::string p = "backbone.stages.4.op_list." + std::to_string(1 + i);
    const std::string a = p + ".context_module.main";
    VitBlock v;
    ES_NEED(b.conv(a + ".qkv", w[4], 3 * w[4], 1, 1, &v.att.qkv));
    ES_NEED(b.dwconv(a + ".aggreg.0.0", true, 3 * w[4], 5, 1, &v.att.agg));
    ES_NEED(b.grouped(a + ".aggreg.0.1", 3 * w[4], &v.att.group));
    ES_NEED(b.conv(a + ".proj", 2 * w[4], w[4], 1, 1, &v.att.proj));
    ES_NEED(b.mb(p + ".local_module", w[4], w[4], 1, 6, true, &v.local));
    e->stage4.push_back(v);
  }
  const int hwid = cfg->head_width;
  for (int j = 0; j < 3; ++j) ES_NEED(b.conv("neck.input_ops." + std::to_string(j) + ".op_list.0", w[4 - j], hwid, 1, 1, &e->neck_in[j]));
  for (int i = 0; i < cfg->head_depth; ++i) {
    FMB f;
    ES_NEED(b.fmb("neck.middle.op_list." + std::to_string(i), hwid, hwid, 1, 1, true, &f));
    e->neck_mid.push_back(f);
  }
  ES_NEED(b.conv("neck.output_ops.0.op_list.0", hwid, cfg->out_dim, 1, 1, &e->neck_out));
  {
    std::vector<float> g = b.get("norm.weight", cfg->out_dim); if (g.empty()) return fail(-1, who, b.err);
    std::vector<float> bt = b.get("norm.bias", cfg->out_dim); if (bt.empty()) return fail(-1, who, b.err);
    e->ln_g = b.upload_f32(std::move(g)); e->ln_b = b.upload_f32(std::move(bt));
  }
#undef ES_NEED

  // activations for max_n images (elements of one image; two bytes each): the stream ping-pong, the expanded tensors of a block (before and
  // after its depthwise convolution), the three stage maps the neck reads, LiteMLA's four tensors, the neck's
  const size_t N = (size_t)max_n;
  auto sq = [&](int div) { return (size_t)(S / div) * (S / div); };
  const size_t stream = std::max({sq(2) * w[0], sq(4) * w[1], sq(8) * w[2], sq(16) * w[3], sq(32) * w[4]});
  const size_t mid = std::max({sq(2) * w[0], sq(4) * 16 * w[0], sq(4) * 4 * w[1], sq(8) * 16 * w[1], sq(8) * 4 * w[2], sq(8) * 16 * w[2], sq(16) * 4 * w[3],
                               sq(16) * 24 * w[3], sq(32) * 6 * w[4]});
  e->xin = b.alloc(N * sq(1) * 8 * 2);
  for (int i = 0; i < 2; ++i) { e->s[i] = b.alloc(N * stream * 2); e->m[i] = b.alloc(N * mid * 2); }
  e->stage[0] = b.alloc(N * sq(8) * w[2] * 2); e->stage[1] = b.alloc(N * sq(16) * w[3] * 2); e->stage[2] = b.alloc(N * sq(32) * w[4] * 2);
  e->qkv = b.alloc(N * sq(32) * 3 * w[4] * 2); e->agg0 = b.alloc(N * sq(32) * 3 * w[4] * 2); e->agg = b.alloc(N * sq(32) * 3 * w[4] * 2);
  e->att = b.alloc(N * sq(32) * 2 * w[4] * 2);
  const int divs[3] = {32, 16, 8};
  for (int j = 0; j < 3; ++j) e->np[j] = b.alloc(N * sq(divs[j]) * hwid * 2);
  const size_t npx = (size_t)NECK * NECK;
  e->nk[0] = b.alloc(N * npx * hwid * 2); e->nk[1] = b.alloc(N * npx * hwid * 2); e->nm = b.alloc(N * npx * hwid * 2);
  e->no = b.alloc(N * npx * cfg->out_dim * 2); e->nl = b.alloc(N * npx * cfg->out_dim * 2);
  // the largest split-K workspace the policy asks for at any n <= max_n (the tile is one image's at every n: only M grows)
  e->sizing = true;
  const int rc = forward(who, e.get(), max_n, nullptr, nullptr);
  e->sizing = false;
  if (rc) return rc;
  e->ws = b.alloc(e->ws_bytes);
  e->arena_bytes = b.top;
  if (device < 0) { *out = e.release(); return 0; }

  int prev = 0;
  if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(device) != hipSuccess) return fail(-2, who, "cannot select the device");
  bool ok = upload_arena(b, &e->arena, e->arena_bytes);
  ok = ok && hipDeviceSynchronize() == hipSuccess;
  (void)hipSetDevice(prev);
  if (!ok) { (void)hipGetLastError(); return fail(-2, who, "device allocation or upload failed"); }
  *out = e.release();
  return 0;
}

extern "C" int es_sam_encode(es_sam_encoder* e, const float* x_nchw, int n, float* out_nchw, void* stream) {
  const char* who = "es_sam_encode";
  if (!e || !x_nchw || !out_nchw) return fail(-1, who, "null pointer");
  if (int rc = ready(who, e, n)) return rc;
  const int S = e->cfg.image_size;
  if (int rc = es_nchw_f32_to_nhwc(x_nchw, e->arena + e->xin, n, 3, S * S, 8, e->dtype, stream)) return rc;
  return forward(who, e, n, out_nchw, (hipStream_t)stream);
}

extern "C" int es_sam_encoder_stage(es_sam_encoder* e, int stage, int n, float* out_nchw, void* stream) {
  const char* who = "es_sam_encoder_stage";
  if (!e || !out_nchw) return fail(-1, who, "null pointer");
  if (stage < 2 || stage > 4) return fail(-1, who, "stage must be 2, 3 or 4");
  if (int rc = ready(who, e, n)) return rc;
  const int side = e->cfg.image_size >> (stage + 1), C = e->cfg.width[stage];
  return es_nhwc_to_nchw_f32(e->arena + e->stage[stage - 2], out_nchw, n, C, side * side, C, 1.f, 0.f, 0, e->dtype, stream);
}

extern "C" size_t es_sam_encode_u8_workspace_bytes(const es_sam_encoder* e, const es_image_u8* imgs, int count) {
  if (!e) { fail(-1, "es_sam_encode_u8_workspace_bytes", "null pointer"); return 0; }
  return es_sam_preprocess_u8_workspace_bytes(imgs, count, e->cfg.image_size);
}

extern "C" int es_sam_encode_u8(es_sam_encoder* e, const es_image_u8* imgs, int count, float* out_nchw, int32_t* input_hw, void* workspace,
                                size_t workspace_bytes, void* stream) {
  const char* who = "es_sam_encode_u8";
  if (!e || !imgs || !out_nchw) return fail(-1, who, "null pointer");
  if (int rc = ready(who, e, count)) return rc;
  if (int rc = es_sam_preprocess_u8(imgs, count, e->cfg.image_size, e->cfg.pixel_mean, e->cfg.pixel_std, e->dtype, e->arena + e->xin, nullptr, nullptr,
                                    input_hw, workspace, workspace_bytes, stream)) return rc;
  return forward(who, e, count, out_nchw, (hipStream_t)stream);
}
