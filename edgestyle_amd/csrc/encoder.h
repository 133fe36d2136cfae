// What the two CLIP towers share on the host (text.hip: es_text_encoder, clip.hip: es_clip_vision and the text side of es_clip_bank):
// one packed linear layer (Lin), the state-dict reader and packer (EncBuilder) and the launch of a
// linear layer through the shared launch policy.  Header-only, included by those two files; the launch helpers are templates over
// the owning object, which must have the members dtype, cfg.ln_eps, knobs, arena, ws and ws_bytes.
#pragma once
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "../../include/edgestyle_hip.h"
#include "host_util.h"
#include "launch_policy.h"
#include "plan.h"

extern "C" void es_set_error(const char* msg);

namespace es_enc {

using namespace es_host;
using es_policy::BK;
constexpr float QUICK_GELU = 1.702f;

inline int fail(int rc, const char* who, const std::string& what) {
  static thread_local char msg[320];
  snprintf(msg, sizeof(msg), "%s: %s", who, what.c_str());
  es_set_error(msg);
  return rc;
}

inline bool capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

struct Lin {                      // one packed linear layer: [rows_padded][kpad] dtype, bias fp32 [rows_padded], optional LayerNorm fold
  size_t w = 0, bias = 0, colsum = 0;
  bool ln = false;
  int cout = 0, cin = 0, rows_padded = 0, kpad = 0;
};
struct Layer { Lin qkv, out, fc1, fc2; };

struct Upload { size_t off; const void* src; size_t bytes; std::vector<char> own; };

struct EncBuilder {
  std::unordered_map<std::string, const es_tensor*> m;
  std::vector<Upload> uploads;
  size_t top = 0;
  int dt = ES_F16;
  std::string err;

  size_t alloc(size_t bytes) { const size_t off = top; top += (bytes + 255) & ~(size_t)255; return off; }
  char* staged(size_t off, size_t bytes) {
    uploads.push_back(Upload{off, nullptr, bytes, std::vector<char>(bytes, 0)});
    return uploads.back().own.data();
  }
  uint16_t enc(float f) const { return dt == ES_F16 ? f32_to_f16(f) : f32_to_bf16(f); }
  float dec(uint16_t u) const { return dt == ES_F16 ? f16_to_f32(u) : bf16_to_f32(u); }

  // `prefix`: stripped from the keys that carry it ("text_model." - SD1.5 checkpoints spell the keys with it, transformers 5 without;
  // "vision_model." - CLIPModel's spelling of what a bare CLIPVisionModel leaves out)
  bool init(const es_state_dict* sd, const char* prefix) {
    if (!sd || sd->count < 0 || (sd->count > 0 && !sd->tensors)) { err = "the state dict has a count but no tensors"; return false; }
    const size_t pl = strlen(prefix);
    for (int i = 0; i < sd->count; ++i) {
      const es_tensor& t = sd->tensors[i];
      if (!t.key || !t.data || t.ndim < 1 || t.ndim > 4 || t.dtype < 0 || t.dtype > ES_F32) { err = "malformed tensor descriptor #" + std::to_string(i); return false; }
      std::string k = t.key;
      if (pl && k.compare(0, pl, prefix) == 0) k = k.substr(pl);
      m[k] = &t;
    }
    return true;
  }
  // fp32 copy of tensor `key` with exactly this shape (1 to 4 dimensions); empty (and err set) otherwise
  std::vector<float> get(const std::string& key, long long d0, long long d1 = -1, long long d2 = -1, long long d3 = -1) {
    auto it = m.find(key);
    if (it == m.end()) { err = "missing key '" + key + "'"; return {}; }
    const es_tensor* t = it->second;
    const long long want[4] = {d0, d1, d2, d3};
    int nd = 1;
    while (nd < 4 && want[nd] >= 0) ++nd;
    bool same = t->ndim == nd;
    for (int j = 0; same && j < nd; ++j) same = t->shape[j] == want[j];
    if (!same) {
      std::string s = "size mismatch for '" + key + "': (";
      for (int j = 0; j < t->ndim; ++j) s += std::to_string(t->shape[j]) + (j + 1 < t->ndim ? "," : "");
      s += ") vs (";
      for (int j = 0; j < nd; ++j) s += std::to_string(want[j]) + (j + 1 < nd ? "," : "");
      err = s + ")";
      return {};
    }
    std::vector<float> v;
    if (!tensor_to_f32(t, &v)) { err = "cannot read '" + key + "' from the device"; return {}; }
    return v;
  }
  size_t upload_f32(std::vector<float>&& v) {
    const size_t off = alloc(v.size() * 4);
    memcpy(staged(off, v.size() * 4), v.data(), v.size() * 4);
    return off;
  }
  // w [cout][cin], b [cout]; gamma / beta: the LayerNorm in front, folded in as es_gemm_desc.ln_colsum asks (w gamma, W beta + b, column sums of
  // the ROUNDED weights); `mul` scales weights and bias (quick_gelu's 1.702)
  Lin pack(const std::vector<float>& w, const std::vector<float>& b, int cout, int cin, const std::vector<float>* gamma, const std::vector<float>* beta, double mul) {
    Lin L;
    L.cout = cout; L.cin = cin;
    const int bn = es_policy::choose_bn(cout);
    L.rows_padded = round_up(cout, bn); L.kpad = round_up(cin, BK);
    L.w = alloc((size_t)L.rows_padded * L.kpad * 2);
    uint16_t* dw = (uint16_t*)staged(L.w, (size_t)L.rows_padded * L.kpad * 2);
    L.bias = alloc((size_t)L.rows_padded * 4);
    float* db = (float*)staged(L.bias, (size_t)L.rows_padded * 4);
    std::vector<float> cs;
    if (gamma) { L.ln = true; cs.assign((size_t)L.rows_padded, 0.f); }
    for (int r = 0; r < cout; ++r) {
      double acc = (double)b[r], sum = 0.0;
      for (int j = 0; j < cin; ++j) {
        const double wv = (double)w[(size_t)r * cin + j];
        const uint16_t q = enc((float)(wv * (gamma ? (double)(*gamma)[j] : 1.0) * mul));
        dw[(size_t)r * L.kpad + j] = q;
        if (gamma) { acc += wv * (double)(*beta)[j]; sum += (double)dec(q); }
      }
      db[r] = (float)(acc * mul);
      if (gamma) cs[r] = (float)sum;
    }
    if (gamma) L.colsum = upload_f32(std::move(cs));
    return L;
  }
  // the four projections of one pre-LN transformer layer under `p` ("encoder.layers.{i}."): q|k|v as one GEMM with LayerNorm1 folded in,
  // out_proj, fc1 with LayerNorm2 folded in and quick_gelu's factor, fc2.  false (and err set) on a missing key or a wrong shape
  bool pack_layer(const std::string& p, int C, int I, Layer* out) {
#define ES_ENC_GET(var, ...) std::vector<float> var = get(__VA_ARGS__); if (var.empty()) return false
    ES_ENC_GET(g1, p + "layer_norm1.weight", C); ES_ENC_GET(b1, p + "layer_norm1.bias", C);
    ES_ENC_GET(g2, p + "layer_norm2.weight", C); ES_ENC_GET(b2, p + "layer_norm2.bias", C);
    std::vector<float> w, bias;
    for (const char* nm : {"q_proj", "k_proj", "v_proj"}) {
      ES_ENC_GET(wi, p + "self_attn." + nm + ".weight", C, C); ES_ENC_GET(bi, p + "self_attn." + nm + ".bias", C);
      w.insert(w.end(), wi.begin(), wi.end()); bias.insert(bias.end(), bi.begin(), bi.end());
    }
    out->qkv = pack(w, bias, 3 * C, C, &g1, &b1, 1.0);
    ES_ENC_GET(wo, p + "self_attn.out_proj.weight", C, C); ES_ENC_GET(bo, p + "self_attn.out_proj.bias", C);
    out->out = pack(wo, bo, C, C, nullptr, nullptr, 1.0);
    ES_ENC_GET(w1, p + "mlp.fc1.weight", I, C); ES_ENC_GET(bb1, p + "mlp.fc1.bias", I);
    out->fc1 = pack(w1, bb1, I, C, &g2, &b2, (double)QUICK_GELU);
    ES_ENC_GET(w2, p + "mlp.fc2.weight", C, I); ES_ENC_GET(bb2, p + "mlp.fc2.bias", C);
    out->fc2 = pack(w2, bb2, C, I, nullptr, nullptr, 1.0);
#undef ES_ENC_GET
    return true;
  }
};

// the policy's defaults with es_linear_xs off: that kernel serves K = 320 | 640 from 8192 rows on, and an encoder batch is a few hundred
// rows of K = hidden
inline void default_knobs(es_launch_knobs* k) {
  es_policy::launch_default_knobs(k);
  k->xs_enabled = 0;
}

template <typename E>
es_gemm_desc gemm_desc(const E* e, const Lin& L, int M, int act, float out_scale, const es_launch_choice& ch) {
  es_gemm_desc d;
  memset(&d, 0, sizeof(d));
  d.N = M; d.Hsrc = 1; d.Wsrc = 1; d.C1 = L.cin; d.Hout = 1; d.Wout = 1; d.Cout = L.cout;
  d.rows_padded = L.rows_padded; d.Kpad = L.kpad; d.ksize = 1; d.stride = 1; d.pad = 0;
  d.act = act; d.splitk = ch.splitk; d.bn = ch.bn; d.dtype = e->dtype; d.out_scale = out_scale; d.stages = ch.stages;
  d.waves = ch.waves; d.xcd_m_fastest = ch.xcd_m_fastest;
  d.ln_eps = e->cfg.ln_eps;
  return d;
}
// the launch policy's answer for one linear layer over M rows (the questions Builder::conv_gemm of builder.hip asks)
template <typename E>
bool choose(const E* e, const Lin& L, int M, int act, float out_scale, bool residual, es_launch_choice* ch) {
  es_launch_query q;
  memset(&q, 0, sizeof(q));
  q.M = M; q.hw = 1; q.w_numel = (long long)L.rows_padded * L.kpad; q.src_numel = (long long)M * L.cin;
  q.ksize = 1; q.stride = 1; q.C1 = L.cin; q.rows_padded = L.rows_padded; q.kpad = L.kpad; q.cin = L.cin; q.cout = L.cout;
  q.has_ln = L.ln; q.act = act; q.has_residual = residual; q.residual_dense = 1; q.unit_scale = out_scale == 1.f; q.x_rep = 1; q.dtype = e->dtype;
  es_launch_knobs k = e->knobs;
  if (act != ES_ACT_NONE) k.big_tile_256 = 0;       // the 256 x 256 tile has no SiLU epilogue form
  return es_launch_choose(&q, &k, ch) == 0;
}

template <typename E>
int linear(const char* who, E* e, const Lin& L, const void* x, void* out, const void* residual, int M, int act, float out_scale, hipStream_t st) {
  es_launch_choice ch;
  if (!choose(e, L, M, act, out_scale, residual != nullptr, &ch)) return -1;
  es_gemm_desc d = gemm_desc(e, L, M, act, out_scale, ch);
  d.x = x; d.out = out; d.residual = residual;
  d.w = e->arena + L.w; d.bias = (const float*)(e->arena + L.bias);
  if (L.ln) d.ln_colsum = (const float*)(e->arena + L.colsum);
  if (ch.splitk > 1) {
    if (es_conv_gemm_workspace_bytes(&d) > e->ws_bytes) return fail(-1, who, "split-K workspace smaller than the launch needs");
    d.workspace = (float*)(e->arena + e->ws);
  }
  return es_conv_gemm(&d, st);
}

// grows e->ws_bytes to the largest split-K workspace the policy asks for when `L` runs over M rows; false (error set) where the policy has no
// es_conv_gemm tile for it
template <typename E>
bool size_workspace(const char* who, E* e, const Lin& L, int M, int act, float out_scale, bool residual) {
  es_launch_choice ch;
  if (!choose(e, L, M, act, out_scale, residual, &ch)) { fail(-1, who, std::string("the launch policy has no tile for a projection: ") + es_last_error()); return false; }
  if (ch.route != ES_ROUTE_CONV_GEMM) { fail(-1, who, "the launch policy routed a projection away from es_conv_gemm"); return false; }
  if (ch.splitk > 1) e->ws_bytes = std::max(e->ws_bytes, (size_t)ch.splitk * M * L.rows_padded * 4);
  return true;
}

// the arena of a built object: one allocation, zeroed, then the staged uploads
inline bool upload_arena(const EncBuilder& b, char** arena, size_t bytes) {
  bool ok = hipMalloc((void**)arena, bytes) == hipSuccess;
  ok = ok && hipMemset(*arena, 0, bytes) == hipSuccess;
  for (const Upload& u : b.uploads) ok = ok && hipMemcpy(*arena + u.off, u.own.data(), u.bytes, hipMemcpyHostToDevice) == hipSuccess;
  return ok;
}

}  // namespace es_enc
