// Leaf code the two native builders share on the host (builder.hip: es_load_weights; encoder.h: the CLIP towers): the 16-bit storage
// conversions, round_up, and the read of an es_tensor - which may live on a device - into fp32.  Header-only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/edgestyle_hip.h"

namespace es_host {

inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

// ---- 16-bit storage types, round to nearest even like torch's .to(dtype) ------------------------------------------------
inline uint16_t f32_to_f16(float f) { _Float16 h = (_Float16)f; uint16_t u; memcpy(&u, &h, 2); return u; }
inline float f16_to_f32(uint16_t u) { _Float16 h; memcpy(&h, &u, 2); return (float)h; }
inline uint16_t f32_to_bf16(float f) {
  uint32_t u; memcpy(&u, &f, 4);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40);      // NaN stays NaN
  return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
inline float bf16_to_f32(uint16_t h) { uint32_t u = (uint32_t)h << 16; float f; memcpy(&f, &u, 4); return f; }

// the source tensors may live on a device as well (a host that already holds the checkpoint there): copied to the host first
inline bool on_device(const void* p) {
  hipPointerAttribute_t a;
  const bool dev = hipPointerGetAttributes(&a, p) == hipSuccess && a.type == hipMemoryTypeDevice;
  (void)hipGetLastError();
  return dev;
}
// every element of `t` as fp32; false when the copy from the device fails (the caller names the tensor)
inline bool tensor_to_f32(const es_tensor* t, std::vector<float>* out) {
  size_t n = 1;
  for (int i = 0; i < t->ndim; ++i) n *= (size_t)t->shape[i];
  std::vector<float>& v = *out;
  v.resize(n);
  const void* src = t->data;
  std::vector<char> tmp;
  if (on_device(src)) {
    tmp.resize(n * (t->dtype == ES_F32 ? 4 : 2));
    if (hipMemcpy(tmp.data(), src, tmp.size(), hipMemcpyDeviceToHost) != hipSuccess) return false;
    src = tmp.data();
  }
  if (t->dtype == ES_F32) memcpy(v.data(), src, n * 4);
  else if (t->dtype == ES_F16) { const uint16_t* s = (const uint16_t*)src; for (size_t i = 0; i < n; ++i) v[i] = f16_to_f32(s[i]); }
  else { const uint16_t* s = (const uint16_t*)src; for (size_t i = 0; i < n; ++i) v[i] = bf16_to_f32(s[i]); }
  return true;
}

}  // namespace es_host
