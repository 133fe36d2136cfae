// JPEG reconstruction (gfx950): quantised DCT coefficients -> RGB bytes, the device half of the decoder whose host half (marker parser,
// Huffman decoder) and per-sample integer rules are csrc/jpeg.h.  include/edgestyle_hip.h states format, limits and arithmetic.
//
// Two launches per 16 images, grid.y = image (images of different sizes share a launch; the blocks past a smaller image's end leave
// at once):
//  1. jpeg_idct_kernel: a workgroup of 256 threads takes 32 consecutive 8x8 blocks of one image (the coefficient buffer is block-major,
//     component after component, so a block's number is its address), eight lanes per block.  Lane j loads row j of the coefficients and
//     of the component's table as one 16-byte load each (a wave reads 1 KiB of consecutive coefficients), dequantises into an LDS tile
//     (rows padded to 9 words), runs the column pass on column j, writes the column back, runs the row pass on row j and stores its
//     8 samples as one 8-byte store into the component's uint8 plane in the workspace (planes are padded to whole blocks).
//  2. jpeg_colour_kernel: a workgroup owns 64 x 16 pixels, a thread four horizontally adjacent ones: one 4-byte luma load, the triangle
//     filter on the chroma planes (esjpeg::upsampled, the host twin's own function), YCbCr -> RGB, and 12 bytes stored as three dwords
//     where the destination is 4-byte aligned and the four pixels are whole, else byte by byte: nothing past width * 3 of a row is written.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include "jpeg.h"
#include "plan.h"

extern "C" void es_set_error(const char* msg);

namespace {

using namespace esjpeg;

constexpr int kImgPerLaunch = 16;
constexpr int kMaxDecode = 64;                    // es_jpeg_decode_u8 keeps its headers on the stack
constexpr size_t kQtableBytes = 3 * 64 * sizeof(uint16_t);

struct ImgDesc {
  const int16_t* coef;
  const uint16_t* q;
  uint8_t* plane[3];      // uint8 planes, rows of blocks_w * 8 bytes
  uint8_t* out;
  long long out_stride;
  uint32_t nblk[3];       // blocks per component
  int32_t blocks_w[3];
  int32_t width, height, components, mode;
  int32_t dw, dh;         // real chroma samples
};
struct Batch { ImgDesc d[kImgPerLaunch]; };

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const Batch b) {
  __shared__ uint32_t tile[32][8][9];
  const ImgDesc& d = b.d[blockIdx.y];
  const uint32_t n0 = d.nblk[0], n01 = n0 + d.nblk[1], total = n01 + d.nblk[2];
  if (blockIdx.x * 32u >= total) return;          // (the whole workgroup: no barrier is left behind)
  const int sub = threadIdx.x >> 3, j = threadIdx.x & 7;
  const uint32_t g = blockIdx.x * 32u + sub;
  const bool live = g < total;
  const int c = g < n0 ? 0 : g < n01 ? 1 : 2;
  if (live) {
    const uint4 cw = *reinterpret_cast<const uint4*>(d.coef + (size_t)g * 64 + j * 8);
    const uint4 qw = *reinterpret_cast<const uint4*>(d.q + c * 64 + j * 8);
    const uint32_t cv[4] = {cw.x, cw.y, cw.z, cw.w}, qv[4] = {qw.x, qw.y, qw.z, qw.w};
#pragma unroll
    for (int k = 0; k < 8; ++k)
      tile[sub][j][k] = dequant((int16_t)(cv[k >> 1] >> (16 * (k & 1))), (uint16_t)(qv[k >> 1] >> (16 * (k & 1))));
  }
  __syncthreads();
  uint32_t in[8], o[8];
  if (live) {                                     // column j: read and written by this lane alone
#pragma unroll
    for (int k = 0; k < 8; ++k) in[k] = tile[sub][k][j];
    idct_1d(in, o);
#pragma unroll
    for (int k = 0; k < 8; ++k) tile[sub][k][j] = descale_column(o[k]);
  }
  __syncthreads();
  if (!live) return;
#pragma unroll
  for (int k = 0; k < 8; ++k) in[k] = tile[sub][j][k];
  idct_1d(in, o);
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    lo |= (uint32_t)descale_sample(o[k]) << (8 * k);
    hi |= (uint32_t)descale_sample(o[4 + k]) << (8 * k);
  }
  const uint32_t lb = g - (c == 0 ? 0u : c == 1 ? n0 : n01);
  const uint32_t bw = (uint32_t)(c == 0 ? d.blocks_w[0] : c == 1 ? d.blocks_w[1] : d.blocks_w[2]);
  uint8_t* plane = c == 0 ? d.plane[0] : c == 1 ? d.plane[1] : d.plane[2];
  const uint32_t by = lb / bw, bx = lb - by * bw;
  *reinterpret_cast<uint2*>(plane + ((size_t)by * 8 + j) * ((size_t)bw * 8) + (size_t)bx * 8) = make_uint2(lo, hi);
}

__global__ __launch_bounds__(256) void jpeg_colour_kernel(const Batch b) {
  const ImgDesc& d = b.d[blockIdx.y];
  const uint32_t tiles_x = (uint32_t)(d.width + 63) / 64u;
  const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const long long yy = (long long)ty * 16 + (threadIdx.x >> 4);
  const int x0 = (int)tx * 64 + (threadIdx.x & 15) * 4;
  if (yy >= d.height || x0 >= d.width) return;
  const int y = (int)yy;
  const size_t s0 = (size_t)d.blocks_w[0] * 8;
  const uint32_t luma = *reinterpret_cast<const uint32_t*>(d.plane[0] + (size_t)y * s0 + x0);     // the plane is padded to whole blocks
  const int m = d.width - x0 < 4 ? d.width - x0 : 4;
  uint8_t px[12];
  if (d.components == 1) {
#pragma unroll
    for (int q = 0; q < 4; ++q) px[3 * q] = px[3 * q + 1] = px[3 * q + 2] = (uint8_t)(luma >> (8 * q));
  } else {
    const size_t s1 = (size_t)d.blocks_w[1] * 8, s2 = (size_t)d.blocks_w[2] * 8;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int x = x0 + q < d.width ? x0 + q : d.width - 1;
      ycc_to_rgb((int)((luma >> (8 * q)) & 255u), upsampled(d.plane[1], s1, d.dw, d.dh, d.mode, x, y),
                 upsampled(d.plane[2], s2, d.dw, d.dh, d.mode, x, y), px + 3 * q);
    }
  }
  uint8_t* dst = d.out + (size_t)y * (size_t)d.out_stride + (size_t)x0 * 3;
  if (m == 4 && ((uintptr_t)dst & 3) == 0) {
    uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
    d32[0] = px[0] | px[1] << 8 | px[2] << 16 | (uint32_t)px[3] << 24;
    d32[1] = px[4] | px[5] << 8 | px[6] << 16 | (uint32_t)px[7] << 24;
    d32[2] = px[8] | px[9] << 8 | px[10] << 16 | (uint32_t)px[11] << 24;
  } else {
    for (int i = 0; i < 3 * m; ++i) dst[i] = px[i];
  }
}

thread_local char g_msg[256];
int fail(const char* who, const char* what) {
  snprintf(g_msg, sizeof(g_msg), "%s: %s", who, what);
  es_set_error(g_msg);
  return -1;
}

const char* check_infos(const es_jpeg_info* infos, int count) {
  if (!infos) return "null pointer";
  if (count < 1) return "count < 1";
  const char* why = nullptr;
  for (int i = 0; i < count; ++i)
    if (!info_ok(infos + i, &why)) return why;
  return nullptr;
}
const char* check_out(const es_jpeg_info& I, const es_image_u8& o) {
  if (!o.data) return "an output image without memory";
  if (o.height != I.height || o.width != I.width) return "an output image whose size is not the file's";
  if (o.channels != 3) return "an output image must have 3 channels";
  if (o.row_stride < (int64_t)I.width * 3) return "an output row stride below width * 3";
  return nullptr;
}
inline size_t staging_bytes_one(const es_jpeg_info& I) { return coeff_count(I) * sizeof(int16_t) + kQtableBytes; }

}  // namespace

extern "C" int es_jpeg_info_host(const uint8_t* bytes, size_t n, es_jpeg_info* info) {
  if (!bytes || !info) return fail("es_jpeg_info_host", "null pointer");
  Header H;
  const char* why = nullptr;
  if (!parse_header(bytes, n, H, &why)) return fail("es_jpeg_info_host", why);
  *info = H.info;
  return 0;
}

extern "C" size_t es_jpeg_coeff_count(const es_jpeg_info* info) {
  const char* why = nullptr;
  if (!info_ok(info, &why)) { fail("es_jpeg_coeff_count", why); return 0; }
  return coeff_count(*info);
}

extern "C" int es_jpeg_entropy_decode_host(const uint8_t* bytes, size_t n, const es_jpeg_info* info, int16_t* coeffs, uint16_t* qtables) {
  const char* who = "es_jpeg_entropy_decode_host";
  if (!bytes || !info || !coeffs || !qtables) return fail(who, "null pointer");
  Header H;
  const char* why = nullptr;
  if (!parse_header(bytes, n, H, &why)) return fail(who, why);
  if (memcmp(&H.info, info, sizeof(H.info)) != 0) return fail(who, "the info is not what es_jpeg_info_host gives for these bytes");
  if (!entropy_decode(bytes, n, H, coeffs, &why)) return fail(who, why);
  component_qtables(H, qtables);
  return 0;
}

extern "C" size_t es_jpeg_reconstruct_workspace_bytes(const es_jpeg_info* infos, int count) {
  if (const char* why = check_infos(infos, count)) { fail("es_jpeg_reconstruct_workspace_bytes", why); return 0; }
  size_t total = 16;                              // room to start the planes on a 16-byte boundary
  for (int i = 0; i < count; ++i) total += coeff_count(infos[i]);      // one byte per coefficient: planes padded to whole blocks
  return total;
}

extern "C" int es_jpeg_reconstruct(const es_jpeg_info* infos, int count, const int16_t* const* coeffs_dev, const uint16_t* const* qtables_dev,
                                   const es_image_u8* out, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "es_jpeg_reconstruct";
  if (!coeffs_dev || !qtables_dev || !out || !workspace) return fail(who, "null pointer");
  if (const char* why = check_infos(infos, count)) return fail(who, why);
  if (es_plan_recording()) return fail(who, "a plan is recording on this thread; the JPEG calls are never part of a plan");
  size_t need = 16;
  for (int i = 0; i < count; ++i) {
    if (const char* why = check_out(infos[i], out[i])) return fail(who, why);
    if (!coeffs_dev[i] || !qtables_dev[i]) return fail(who, "null pointer");
    if ((uintptr_t)coeffs_dev[i] % 16 || (uintptr_t)qtables_dev[i] % 16) return fail(who, "coefficients and tables must be 16-byte aligned");
    need += coeff_count(infos[i]);
  }
  if (workspace_bytes < need) return fail(who, "workspace too small (es_jpeg_reconstruct_workspace_bytes)");
  uint8_t* ws = (uint8_t*)(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  for (int first = 0; first < count; first += kImgPerLaunch) {
    const int n = count - first < kImgPerLaunch ? count - first : kImgPerLaunch;
    Batch b;
    memset(&b, 0, sizeof(b));
    uint32_t max_groups = 0, max_tiles = 0;
    for (int i = 0; i < n; ++i) {
      const es_jpeg_info& I = infos[first + i];
      ImgDesc& d = b.d[i];
      d.coef = coeffs_dev[first + i];
      d.q = qtables_dev[first + i];
      uint32_t blocks = 0;
      for (int c = 0; c < I.components; ++c) {
        d.plane[c] = ws;
        d.nblk[c] = (uint32_t)component_blocks(I, c);            // at most 8192 * 8192 each
        d.blocks_w[c] = I.blocks_w[c];
        ws += component_blocks(I, c) * 64;
        blocks += d.nblk[c];
      }
      d.out = const_cast<uint8_t*>(out[first + i].data);
      d.out_stride = out[first + i].row_stride;
      d.width = I.width; d.height = I.height; d.components = I.components;
      d.mode = up_mode(I.hmax, I.vmax);
      d.dw = I.components == 3 ? comp_w(I, 1) : 0;
      d.dh = I.components == 3 ? comp_h(I, 1) : 0;
      const uint32_t groups = (blocks + 31) / 32;
      const uint32_t tiles = (uint32_t)((I.width + 63) / 64) * (uint32_t)((I.height + 15) / 16);
      max_groups = groups > max_groups ? groups : max_groups;
      max_tiles = tiles > max_tiles ? tiles : max_tiles;
    }
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(max_groups, (unsigned)n), dim3(256), 0, (hipStream_t)stream, b);
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3(max_tiles, (unsigned)n), dim3(256), 0, (hipStream_t)stream, b);
    if (hipGetLastError() != hipSuccess) { fail(who, "launch failed"); return -2; }
  }
  return 0;
}

extern "C" int es_jpeg_reconstruct_host(const es_jpeg_info* infos, int count, const int16_t* const* coeffs, const uint16_t* const* qtables,
                                        const es_image_u8* out) {
  const char* who = "es_jpeg_reconstruct_host";
  if (!coeffs || !qtables || !out) return fail(who, "null pointer");
  if (const char* why = check_infos(infos, count)) return fail(who, why);
  for (int i = 0; i < count; ++i) {
    if (const char* why = check_out(infos[i], out[i])) return fail(who, why);
    if (!coeffs[i] || !qtables[i]) return fail(who, "null pointer");
  }
  for (int i = 0; i < count; ++i) reconstruct(infos[i], coeffs[i], qtables[i], const_cast<uint8_t*>(out[i].data), (size_t)out[i].row_stride);
  return 0;
}

extern "C" size_t es_jpeg_decode_staging_bytes(const es_jpeg_info* infos, int count) {
  if (const char* why = check_infos(infos, count)) { fail("es_jpeg_decode_staging_bytes", why); return 0; }
  size_t total = 0;
  for (int i = 0; i < count; ++i) total += staging_bytes_one(infos[i]);
  return total;
}

extern "C" int es_jpeg_decode_u8(const uint8_t* const* bytes, const size_t* n, int count, const es_image_u8* out, void* staging_host,
                                 void* staging_dev, size_t staging_bytes, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "es_jpeg_decode_u8";
  if (!bytes || !n || !out || !staging_host || !staging_dev || !workspace) return fail(who, "null pointer");
  if (count < 1) return fail(who, "count < 1");
  if (count > kMaxDecode) return fail(who, "count > 64");
  if ((uintptr_t)staging_host % 16 || (uintptr_t)staging_dev % 16) return fail(who, "the staging buffers must be 16-byte aligned");
  if (es_plan_recording()) return fail(who, "a plan is recording on this thread; the JPEG calls are never part of a plan");
  es_jpeg_info infos[kMaxDecode];
  const int16_t* coeffs[kMaxDecode];
  const uint16_t* qtables[kMaxDecode];
  const char* why = nullptr;
  size_t used = 0;
  Header H;
  for (int i = 0; i < count; ++i) {               // headers first: sizes are known before anything is written
    if (!bytes[i]) return fail(who, "null pointer");
    if (!parse_header(bytes[i], n[i], H, &why)) return fail(who, why);
    infos[i] = H.info;
    used += staging_bytes_one(H.info);
  }
  if (staging_bytes < used) return fail(who, "staging too small (es_jpeg_decode_staging_bytes)");
  size_t at = 0;
  for (int i = 0; i < count; ++i) {
    if (!parse_header(bytes[i], n[i], H, &why)) return fail(who, why);
    int16_t* cf = (int16_t*)((uint8_t*)staging_host + at);
    uint16_t* qt = (uint16_t*)((uint8_t*)staging_host + at + coeff_count(H.info) * sizeof(int16_t));
    if (!entropy_decode(bytes[i], n[i], H, cf, &why)) return fail(who, why);
    memset(qt, 0, kQtableBytes);
    component_qtables(H, qt);
    coeffs[i] = (const int16_t*)((uint8_t*)staging_dev + at);
    qtables[i] = (const uint16_t*)((uint8_t*)staging_dev + at + coeff_count(H.info) * sizeof(int16_t));
    at += staging_bytes_one(H.info);
  }
  if (hipMemcpyAsync(staging_dev, staging_host, used, hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess) { fail(who, "upload failed"); return -2; }
  return es_jpeg_reconstruct(infos, count, coeffs, qtables, out, workspace, workspace_bytes, stream);
}
