// Byte images at the edge of the C ABI (gfx950): Pillow-exact bilinear resize + centre crop of uint8 HWC images of any size,
// uint8 HWC -> fp32 NCHW network input, fp32 NCHW network output -> uint8 HWC.
//
// The reference's callers prepare every condition image with torchvision's Resize(R, BILINEAR) -> CenterCrop(R) -> ToTensor
// (-> Normalize(.5, .5)) on a PIL image (test_text2image_pretrained_openpose.py:29-48).  On a PIL image that resize is Pillow's
// ImagingResample: separable (horizontal pass, then vertical pass, a uint8 image in between), antialiased (the triangle filter
// is stretched by the scale when shrinking), with double-precision weights normalised per output pixel and then quantised to
// 22 fractional bits; everything after the quantisation is integer arithmetic.  The kernels below redo exactly that, so their
// bytes EQUAL Pillow's.  The coefficient code is written once (resize_axis, __host__ __device__): es_image_resize_coeffs hands
// the host build of it to the CPU tests, the kernels run the device build.  Built with -ffp-contract=off (csrc/Makefile): a
// fused multiply-add in the weight arithmetic would round differently from Pillow's C.
// es_sam_preprocess_u8 (EfficientViTSam.transform: long side -> S, no crop, normalise, pad) lives here as well: it resamples with the same
// resize_axis, through kernels of its own (a rectangular result, every source row), so nothing the calls above compute changes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <algorithm>
#include <vector>

#include "../../include/edgestyle_hip.h"
#include "plan.h"

extern "C" void es_set_error(const char* msg);

namespace {

constexpr int kPrecisionBits = 32 - 8 - 2;      // Pillow's PRECISION_BITS for 8-bit channels

// Pillow's filters (Resample.c): the triangle of BILINEAR (support 1), the Keys cubic of BICUBIC (a = -0.5, support 2) and the
// truncated sinc of LANCZOS (sinc(x) * sinc(x / 3) on [-3, 3), support 3; sinc(x) = sin(pi x) / (pi x))
__host__ __device__ inline double filter_support(int filter) { return filter == ES_FILTER_LANCZOS ? 3.0 : (filter == ES_FILTER_BICUBIC ? 2.0 : 1.0); }
__host__ __device__ inline double sinc_pi(double x) {
  if (x == 0.0) return 1.0;
  x = x * 3.14159265358979323846;
  return sin(x) / x;
}
__host__ __device__ inline double filter_weight(int filter, double x) {
  if (filter == ES_FILTER_LANCZOS) return -3.0 <= x && x < 3.0 ? sinc_pi(x) * sinc_pi(x / 3) : 0.0;
  if (x < 0.0) x = -x;
  if (filter == ES_FILTER_BICUBIC) {
    const double a = -0.5;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
  }
  return x < 1.0 ? 1.0 - x : 0.0;
}

// One output pixel `xx` of an axis resampled from `in` to `out` pixels (Pillow precompute_coeffs + normalize_coeffs_8bpc with
// `filter`, box = the whole axis): calls sink(xmin, x, k) for every tap - source index xmin + x, 22-bit fixed-point weight k
// (negative for the outer lobes of the cubic) - in index order, returns the tap count and the first source index.
template <typename Sink>
__host__ __device__ inline int resize_axis(int filter, int in, int out, int xx, int* xmin_out, Sink&& sink) {
  const double scale = (double)in / (double)out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = filter_support(filter) * fs;
  const double ss = 1.0 / fs;
  const double center = (xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in) xmax = in;
  const int n = xmax - xmin;
  auto weight = [&](int x) { return filter_weight(filter, (x + xmin - center + 0.5) * ss); };
  double ww = 0.0;
  for (int x = 0; x < n; ++x) ww += weight(x);
  for (int x = 0; x < n; ++x) {
    double w = weight(x);
    if (ww != 0.0) w /= ww;
    sink(xmin, x, w < 0.0 ? (int)(-0.5 + w * (double)(1 << kPrecisionBits)) : (int)(0.5 + w * (double)(1 << kPrecisionBits)));
  }
  *xmin_out = xmin;
  return n;
}

__host__ __device__ inline uint8_t clip8(int v) {
  v >>= kPrecisionBits;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// ToTensor (-> Normalize(.5, .5)): both divisions correctly rounded, as numpy / torch compute them on the host
__device__ inline float u8_to_unit(uint8_t v, int normalize) {
  float y = __fdiv_rn((float)v, 255.0f);
  if (normalize) y = __fdiv_rn(y - 0.5f, 0.5f);
  return y;
}

// torchvision's Resize(R) = transformers' resize(shortest_edge = R) (shorter side -> R, longer side truncated), then the centre crop:
// torchvision's CenterCrop(R) (round-half-to-even offsets) or transformers' center_crop ((size - R) // 2: the half is dropped)
void fit(int height, int width, int R, int crop, int32_t out[4]) {
  int rh, rw;
  if (width <= height) { rw = R; rh = (int)((double)((long long)R * height) / (double)width); }
  else { rh = R; rw = (int)((double)((long long)R * width) / (double)height); }
  out[0] = rh; out[1] = rw;
  if (crop == ES_CROP_TRANSFORMERS) { out[2] = (rh - R) / 2; out[3] = (rw - R) / 2; }      // rh, rw >= R: no negative operand
  else { out[2] = (int)rint((rh - R) / 2.0); out[3] = (int)rint((rw - R) / 2.0); }
}

struct ImgDesc {
  const uint8_t* src;     // [in_h][stride bytes], ch bytes per pixel
  long long stride;
  uint8_t* tmp;           // horizontal pass result: source rows [y0, y0 + nrows) x the R kept columns x 3 (need_h only)
  uint8_t* out;           // [R, R, 3] or null
  float* fout;            // [3, R, R] or null
  int32_t in_h, in_w, ch;
  int32_t rh, rw, top, left;
  int32_t y0, nrows;
  int32_t need_h, need_v, normalize;
};
constexpr int kImgPerLaunch = 16;
struct Batch { ImgDesc d[kImgPerLaunch]; int32_t R, filter; };

// Horizontal pass.  grid.y = image; consecutive threads take consecutive (x * 3 + c) bytes of a row of the intermediate image,
// so the stores coalesce and the loads of a wave fall into a few neighbouring lines of one source row.  Only the columns the
// crop keeps and the source rows the kept output rows read are produced.
__global__ __launch_bounds__(256) void resize_h_kernel(const Batch b) {
  const ImgDesc& d = b.d[blockIdx.y];
  if (!d.need_h) return;
  const int row3 = 3 * b.R;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)d.nrows * row3) return;
  const int r = (int)(idx / row3), j = (int)(idx - (long long)r * row3);
  const int xx = d.left + j / 3, c = j % 3;
  const uint8_t* row = d.src + (size_t)(d.y0 + r) * (size_t)d.stride + c;
  int acc = 1 << (kPrecisionBits - 1), xmin;
  const int ch = d.ch;
  resize_axis(b.filter, d.in_w, d.rw, xx, &xmin, [&](int x0, int x, int k) { acc += k * (int)row[(size_t)(x0 + x) * ch]; });
  d.tmp[idx] = clip8(acc);
}

// Vertical pass + crop (+ ToTensor / Normalize).  grid.y = image; consecutive threads take consecutive (x * 3 + c) bytes of an
// output row: every tap is one coalesced row segment of the intermediate image (or of the source, when the horizontal pass was
// skipped).  An axis whose size does not change is skipped as Pillow skips it: the kept bytes are copied.
__global__ __launch_bounds__(256) void resize_v_kernel(const Batch b) {
  const ImgDesc& d = b.d[blockIdx.y];
  const int R = b.R, row3 = 3 * R;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)R * row3) return;
  const int yy = (int)(idx / row3), j = (int)(idx - (long long)yy * row3);
  const int x = j / 3, c = j - 3 * x;
  const uint8_t* base;
  size_t pitch;
  if (d.need_h) { base = d.tmp + j - (size_t)d.y0 * row3; pitch = (size_t)row3; }          // row y of the source is row y - y0 of tmp
  else { base = d.src + (size_t)(d.left + x) * d.ch + c; pitch = (size_t)d.stride; }
  uint8_t v;
  if (d.need_v) {
    int acc = 1 << (kPrecisionBits - 1), ymin;
    resize_axis(b.filter, d.in_h, d.rh, d.top + yy, &ymin, [&](int y0, int y, int k) { acc += k * (int)base[(size_t)(y0 + y) * pitch]; });
    v = clip8(acc);
  } else {
    v = base[(size_t)(d.top + yy) * pitch];
  }
  if (d.out) d.out[idx] = v;
  if (d.fout) d.fout[((size_t)c * R + yy) * R + x] = u8_to_unit(v, d.normalize);
}

__global__ __launch_bounds__(256) void u8_to_f32_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, long long count, long long HW, int normalize) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= count * 3 * HW) return;
  const long long p = i % HW, nc = i / HW;
  const long long n = nc / 3;
  const int c = (int)(nc - 3 * n);
  out[i] = u8_to_unit(in[(n * HW + p) * 3 + c], normalize);
}

__device__ inline unsigned unit_to_u8(float x) {
  float y = x * 255.0f;                       // the file is built with -ffp-contract=off: a plain product, then the rounding
  y = rintf(y);
  y = y < 0.0f ? 0.0f : (y > 255.0f ? 255.0f : y);
  return (unsigned)y;
}

// Four pixels per thread: one float4 per colour plane in, three dwords out.  The planes of an image are contiguous over H*W and
// so are its HWC bytes, so the pixels are taken in runs of four over H*W whatever W is; `vec` (uniform) says that every run of
// four is whole and aligned (H*W % 4 == 0, 16-byte aligned input, 4-byte aligned output); without it, and for nothing else,
// pixels are moved one by one.
__global__ __launch_bounds__(256) void f32_to_u8_kernel(const float* __restrict__ in, uint8_t* __restrict__ out, long long B, long long HW, int vec) {
  const long long groups = (HW + 3) / 4;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= B * groups) return;
  const long long n = i / groups, p0 = (i - n * groups) * 4;
  const float* src = in + n * 3 * HW + p0;
  uint8_t* dst = out + (n * HW + p0) * 3;
  if (vec) {
    const float4 r = *(const float4*)src, g = *(const float4*)(src + HW), bl = *(const float4*)(src + 2 * HW);
    const unsigned r0 = unit_to_u8(r.x), r1 = unit_to_u8(r.y), r2 = unit_to_u8(r.z), r3 = unit_to_u8(r.w);
    const unsigned g0 = unit_to_u8(g.x), g1 = unit_to_u8(g.y), g2 = unit_to_u8(g.z), g3 = unit_to_u8(g.w);
    const unsigned b0 = unit_to_u8(bl.x), b1 = unit_to_u8(bl.y), b2 = unit_to_u8(bl.z), b3 = unit_to_u8(bl.w);
    unsigned* d32 = (unsigned*)dst;
    d32[0] = r0 | (g0 << 8) | (b0 << 16) | (r1 << 24);
    d32[1] = g1 | (b1 << 8) | (r2 << 16) | (g2 << 24);
    d32[2] = b2 | (r3 << 8) | (g3 << 16) | (b3 << 24);
  } else {
    const int m = (int)(HW - p0 < 4 ? HW - p0 : 4);
    for (int q = 0; q < m; ++q)
      for (int c = 0; c < 3; ++c) dst[q * 3 + c] = (uint8_t)unit_to_u8(src[(long long)c * HW + q]);
  }
}

// ---- EfficientViTSam.transform --------------------------------------------------------------------------------------------------
// torchvision's resize(PIL, (rh, rw)) without a crop: Pillow's horizontal pass over every source row, then its vertical pass, then
// ToTensor / Normalize / SamPad.  `pix`: where the normalising kernel reads the resized bytes - the compact result of the passes, or the
// source itself (its own stride and channel count) when the long side already is S and Pillow is never called.
struct SamImg {
  const uint8_t* src;
  long long stride;
  uint8_t* tmp;           // [in_h][rw][3]  (need_h)
  uint8_t* res;           // [rh][rw][3]    (need_h or need_v)
  const uint8_t* pix;
  long long pix_pitch;
  int32_t pix_step;
  int32_t in_h, in_w, ch, rh, rw, need_h, need_v;
};
struct SamBatch { SamImg d[kImgPerLaunch]; float mean[3], std[3]; int32_t S, first; };

__global__ __launch_bounds__(256) void sam_resize_h_kernel(const SamBatch b) {
  const SamImg& d = b.d[blockIdx.y];
  if (!d.need_h) return;
  const int row3 = 3 * d.rw;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)d.in_h * row3) return;
  const int r = (int)(idx / row3), j = (int)(idx - (long long)r * row3);
  const int xx = j / 3, c = j - 3 * xx;
  const uint8_t* row = d.src + (size_t)r * (size_t)d.stride + c;
  int acc = 1 << (kPrecisionBits - 1), xmin;
  const int ch = d.ch;
  resize_axis(ES_FILTER_BILINEAR, d.in_w, d.rw, xx, &xmin, [&](int x0, int x, int k) { acc += k * (int)row[(size_t)(x0 + x) * ch]; });
  d.tmp[idx] = clip8(acc);
}

__global__ __launch_bounds__(256) void sam_resize_v_kernel(const SamBatch b) {
  const SamImg& d = b.d[blockIdx.y];
  if (!d.need_v) return;        // (a horizontal pass alone wrote `res` itself: sam_plan points tmp at it)
  const int row3 = 3 * d.rw;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)d.rh * row3) return;
  const int yy = (int)(idx / row3), j = (int)(idx - (long long)yy * row3);
  const int x = j / 3, c = j - 3 * x;
  const uint8_t* base;
  size_t pitch;
  if (d.need_h) { base = d.tmp + j; pitch = (size_t)row3; }
  else { base = d.src + (size_t)x * d.ch + c; pitch = (size_t)d.stride; }
  int acc = 1 << (kPrecisionBits - 1), ymin;
  resize_axis(ES_FILTER_BILINEAR, d.in_h, d.rh, yy, &ymin, [&](int y0, int y, int k) { acc += k * (int)base[(size_t)(y0 + y) * pitch]; });
  d.res[idx] = clip8(acc);
}

// one thread per canvas pixel: (v / 255 - mean) / std, both divisions correctly rounded and nothing fused (torch's ToTensor and Normalize);
// outside the resized image every output is exactly 0
template <typename T>
__global__ __launch_bounds__(256) void sam_normalize_kernel(const SamBatch b, T* out_nhwc, float* out_nchw, uint8_t* out_u8) {
  const SamImg& d = b.d[blockIdx.y];
  const int S = b.S;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)S * S) return;
  const int y = (int)(idx / S), x = (int)(idx - (long long)y * S);
  const size_t img = (size_t)(b.first + (int)blockIdx.y);
  float f[3] = {0.f, 0.f, 0.f};
  uint8_t v[3] = {0, 0, 0};
  if (y < d.rh && x < d.rw) {
    const uint8_t* px = d.pix + (size_t)y * (size_t)d.pix_pitch + (size_t)x * d.pix_step;
#pragma unroll
    for (int c = 0; c < 3; ++c) { v[c] = px[c]; f[c] = __fdiv_rn(__fdiv_rn((float)v[c], 255.0f) - b.mean[c], b.std[c]); }
  }
  if (out_nhwc) {
    T* o = out_nhwc + (img * S * S + (size_t)idx) * 8;
#pragma unroll
    for (int c = 0; c < 8; ++c) o[c] = (T)(c < 3 ? f[c] : 0.f);
  }
  if (out_nchw)
    for (int c = 0; c < 3; ++c) out_nchw[(img * 3 + c) * S * S + (size_t)idx] = f[c];
  if (out_u8)
    for (int c = 0; c < 3; ++c) out_u8[(img * S * S + (size_t)idx) * 3 + c] = v[c];
}

void sam_shape(int h, int w, int S, int32_t out[2]) {      // SamResize: get_preprocess_shape, and no resize when the long side is S
  const int lng = h > w ? h : w;
  if (lng == S) { out[0] = h; out[1] = w; return; }
  const double scale = (double)S * 1.0 / (double)lng;
  out[0] = (int)((double)h * scale + 0.5);
  out[1] = (int)((double)w * scale + 0.5);
}
size_t sam_plan(const es_image_u8& im, int S, SamImg& d) {  // bytes of workspace the image needs (tmp, then res, each 16-byte aligned)
  int32_t hw[2];
  sam_shape(im.height, im.width, S, hw);
  d.src = im.data; d.stride = im.row_stride; d.in_h = im.height; d.in_w = im.width; d.ch = im.channels;
  d.rh = hw[0]; d.rw = hw[1];
  d.need_h = d.rw != d.in_w; d.need_v = d.rh != d.in_h;
  d.tmp = nullptr; d.res = nullptr; d.pix = im.data; d.pix_pitch = im.row_stride; d.pix_step = im.channels;
  const size_t a = d.need_h && d.need_v ? (((size_t)d.in_h * d.rw * 3 + 15) & ~(size_t)15) : 0;
  const size_t r = d.need_h || d.need_v ? (((size_t)d.rh * d.rw * 3 + 15) & ~(size_t)15) : 0;
  return a + r;
}


// ---- create_processed_image: resize to any (new_h, new_w), keep a window that may hang outside ------------------------------------
// The two passes of the calls above with a rectangular window instead of the centre square: only the columns [x0, x0 + ncols) and the
// rows the window keeps are produced (the source rows the kept rows' taps reach, for the horizontal pass), and a pixel of the window
// that lies outside the resized image is 0, as PIL's crop pads it.
struct WinDesc {
  const uint8_t* src;
  long long stride;
  uint8_t* tmp;           // horizontal pass result: source rows [y0, y0 + nrows) x the ncols kept columns x 3 (need_h only)
  uint8_t* out;           // [out_h, out_w, 3]
  int32_t in_h, in_w, ch;
  int32_t rh, rw, top, left;
  int32_t y0, nrows, x0, ncols;
  int32_t need_h, need_v;
};
struct WinBatch { WinDesc d[kImgPerLaunch]; int32_t out_h, out_w, filter; };

__global__ __launch_bounds__(256) void window_h_kernel(const WinBatch b) {
  const WinDesc& d = b.d[blockIdx.y];
  if (!d.need_h) return;
  const int row3 = 3 * d.ncols;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)d.nrows * row3) return;
  const int r = (int)(idx / row3), j = (int)(idx - (long long)r * row3);
  const int xx = d.x0 + j / 3, c = j % 3;
  const uint8_t* row = d.src + (size_t)(d.y0 + r) * (size_t)d.stride + c;
  int acc = 1 << (kPrecisionBits - 1), xmin;
  const int ch = d.ch;
  resize_axis(b.filter, d.in_w, d.rw, xx, &xmin, [&](int x0, int x, int k) { acc += k * (int)row[(size_t)(x0 + x) * ch]; });
  d.tmp[idx] = clip8(acc);
}

__global__ __launch_bounds__(256) void window_v_kernel(const WinBatch b) {
  const WinDesc& d = b.d[blockIdx.y];
  const int row3 = 3 * b.out_w;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)b.out_h * row3) return;
  const int yy = (int)(idx / row3), j = (int)(idx - (long long)yy * row3);
  const int x = j / 3, c = j - 3 * x;
  const int ry = d.top + yy, rx = d.left + x;             // the pixel of the resized image this byte shows
  uint8_t v = 0;
  if (ry >= 0 && ry < d.rh && rx >= 0 && rx < d.rw) {     // (inside: rx is one of the kept columns, ry one of the kept rows)
    const uint8_t* base;                                  // row 0 of the column the taps run down
    long long pitch, first;                               // `first`: the source row that base points at
    if (d.need_h) { base = d.tmp + (size_t)(rx - d.x0) * 3 + c; pitch = 3ll * d.ncols; first = d.y0; }
    else { base = d.src + (size_t)rx * d.ch + c; pitch = d.stride; first = 0; }
    if (d.need_v) {
      int acc = 1 << (kPrecisionBits - 1), ymin;
      resize_axis(b.filter, d.in_h, d.rh, ry, &ymin, [&](int y0, int y, int k) { acc += k * (int)base[(size_t)((long long)(y0 + y) - first) * (size_t)pitch]; });
      v = clip8(acc);
    } else {
      v = base[(size_t)((long long)ry - first) * (size_t)pitch];
    }
  }
  d.out[idx] = v;
}

// create_processed_image's geometry (extract_dataset.py:118-164) in double, in its order of operations and with its int() truncations
// (Python's max(0, v) / min(n, v) keep v unless the bound is strictly better: the same values).  false: no positive scale comes out.
bool person_fit(int height, int width, const double box[4], int final_w, int final_h, double margin, int32_t out[4]) {
  double xmin = box[0], ymin = box[1], xmax = box[2], ymax = box[3];
  const double bbox_width = xmax - xmin, bbox_height = ymax - ymin;
  const double margin_width = bbox_width * margin, margin_height = bbox_height * margin;
  xmin = xmin - margin_width; if (0.0 > xmin) xmin = 0.0;
  xmax = xmax + margin_width; if ((double)width < xmax) xmax = (double)width;
  ymin = ymin - margin_height; if (0.0 > ymin) ymin = 0.0;
  ymax = ymax + margin_height; if ((double)height < ymax) ymax = (double)height;
  const double bbox_center_x = (xmin + xmax) / 2.0, bbox_center_y = (ymin + ymax) / 2.0;
  if (!(xmax - xmin > 0.0) || !(ymax - ymin > 0.0)) return false;
  const double scale_x = (double)final_w / (xmax - xmin), scale_y = (double)final_h / (ymax - ymin);
  const double scale = scale_y < scale_x ? scale_y : scale_x;
  const double nw = (double)width * scale, nh = (double)height * scale;
  if (!(nw >= 1.0 && nw <= 16777216.0 && nh >= 1.0 && nh <= 16777216.0)) return false;
  const int new_width = (int)nw, new_height = (int)nh;
  const int new_bbox_center_x = (int)(bbox_center_x * scale), new_bbox_center_y = (int)(bbox_center_y * scale);
  int left = new_bbox_center_x - final_w / 2, top = new_bbox_center_y - final_h / 2;
  if (left < 0) left = 0;
  if (top < 0) top = 0;
  if (left + final_w > new_width) left = new_width - final_w;
  if (top + final_h > new_height) top = new_height - final_h;
  out[0] = new_width; out[1] = new_height; out[2] = left; out[3] = top;
  return true;
}

thread_local char g_msg[224];
int fail(const char* who, const char* what) {
  snprintf(g_msg, sizeof(g_msg), "%s: %s", who, what);
  es_set_error(g_msg);
  return -1;
}
int fail_img(const char* who, int i, const char* what) {
  snprintf(g_msg, sizeof(g_msg), "%s: image %d: %s", who, i, what);
  es_set_error(g_msg);
  return -1;
}

// argument checks shared by the size query and the launcher: everything that can be judged without a GPU
int check_images(const char* who, const es_image_u8* imgs, int count, int R) {
  if (!imgs) return fail(who, "null pointer (imgs)");
  if (count < 1) return fail(who, "count < 1");
  if (R < 1) return fail(who, "R < 1");
  if (R > 16384) return fail(who, "R > 16384");
  for (int i = 0; i < count; ++i) {
    const es_image_u8& im = imgs[i];
    if (!im.data) return fail_img(who, i, "null pointer (data)");
    if (im.height < 1 || im.width < 1) return fail_img(who, i, "height or width < 1");
    if (im.channels != 3 && im.channels != 4) return fail_img(who, i, "channels must be 3 or 4");
    if (im.row_stride < (int64_t)im.width * im.channels) return fail_img(who, i, "row_stride < width*channels");
    const long long lng = im.height > im.width ? im.height : im.width, sht = im.height > im.width ? im.width : im.height;
    if ((long long)R * lng / sht > (1 << 24)) return fail_img(who, i, "the resized longer side would pass 2^24 pixels");
  }
  return 0;
}

// geometry of one image: resized size, crop, which passes run, and the source rows the kept output rows read (their range follows
// the filter's support: the cubic reaches twice as far as the triangle)
void plan_image(const es_image_u8& im, int R, int filter, int crop, ImgDesc& d) {
  int32_t f[4];
  fit(im.height, im.width, R, crop, f);
  d.src = im.data; d.stride = im.row_stride;
  d.in_h = im.height; d.in_w = im.width; d.ch = im.channels;
  d.rh = f[0]; d.rw = f[1]; d.top = f[2]; d.left = f[3];
  d.need_h = d.rw != d.in_w;
  d.need_v = d.rh != d.in_h;
  d.y0 = d.top; d.nrows = R;
  if (d.need_v) {
    int lo = d.in_h, hi = 0;
    for (int yy = d.top; yy < d.top + R; ++yy) {
      int ymin;
      const int n = resize_axis(filter, d.in_h, d.rh, yy, &ymin, [](int, int, int) {});
      lo = ymin < lo ? ymin : lo;
      hi = ymin + n > hi ? ymin + n : hi;
    }
    d.y0 = lo; d.nrows = hi - lo;
  }
  d.tmp = nullptr; d.out = nullptr; d.fout = nullptr; d.normalize = 0;
}
size_t tmp_bytes(const ImgDesc& d, int R) { return d.need_h ? (size_t)d.nrows * 3 * (size_t)R : 0; }

bool known_rules(const char* who, int filter, int crop) {
  if (filter != ES_FILTER_BILINEAR && filter != ES_FILTER_BICUBIC) { fail(who, "filter must be ES_FILTER_BILINEAR or ES_FILTER_BICUBIC"); return false; }
  if (crop != ES_CROP_TORCHVISION && crop != ES_CROP_TRANSFORMERS) { fail(who, "crop rule must be ES_CROP_TORCHVISION or ES_CROP_TRANSFORMERS"); return false; }
  return true;
}

// the windowed calls and es_image_resize_coeffs_ex also take ES_FILTER_LANCZOS (the centre-crop calls above keep their two filters)
bool known_filter(const char* who, int filter) {
  if (filter == ES_FILTER_BILINEAR || filter == ES_FILTER_BICUBIC || filter == ES_FILTER_LANCZOS) return true;
  fail(who, "filter must be ES_FILTER_BILINEAR, ES_FILTER_BICUBIC or ES_FILTER_LANCZOS");
  return false;
}

int resize_coeffs(const char* who, int filter, int in, int out, int32_t* xmin, int32_t* ntaps, int32_t* k, int cap) {
  if (in < 1 || out < 1) return fail(who, "in or out < 1");
  int most = 0;
  for (int xx = 0; xx < out; ++xx) {
    int x0;
    const int n = resize_axis(filter, in, out, xx, &x0, [&](int, int x, int kk) { if (k && x < cap) k[(size_t)xx * cap + x] = kk; });
    if (xmin) xmin[xx] = x0;
    if (ntaps) ntaps[xx] = n;
    most = n > most ? n : most;
  }
  if (k && cap < most) return fail(who, "cap is smaller than the longest run of taps (ask with k = NULL first)");
  return most;
}

size_t workspace_bytes(const char* who, const es_image_u8* imgs, int count, int R, int filter, int crop) {
  if (!imgs || count < 1 || R < 1) { fail(who, "null pointer (imgs), count < 1 or R < 1"); return 0; }
  size_t need = 0;
  for (int i = 0; i < count; ++i) {
    if (imgs[i].height < 1 || imgs[i].width < 1) { fail_img(who, i, "height or width < 1"); return 0; }
    ImgDesc d;
    plan_image(imgs[i], R, filter, crop, d);
    need += tmp_bytes(d, R);
  }
  return need;
}

}  // namespace

// library-internal (plan.hip: es_prepare_conds_u8; clip.hip: es_clip_pick): the resize with a uint8 [count,R,R,3] result (out_u8), an
// fp32 [3,R,R] result per image (out_f32[i], ToTensor (+ Normalize where normalize[i])), or both
int es_image_resize_impl_ex(const char* who, const es_image_u8* imgs, int count, uint8_t* out_u8, float* const* out_f32,
                            const int32_t* normalize, int R, int filter, int crop, void* workspace, size_t workspace_bytes, void* stream) {
  if (check_images(who, imgs, count, R)) return -1;
  if (!known_rules(who, filter, crop)) return -1;
  if (!out_u8 && !out_f32) return fail(who, "null pointer (out)");
  if (es_plan_recording()) return fail(who, "a plan is recording on this thread; the byte-image calls are never part of a plan");
  std::vector<ImgDesc> ds((size_t)count);
  size_t need = 0;
  for (int i = 0; i < count; ++i) {
    plan_image(imgs[i], R, filter, crop, ds[i]);
    ds[i].tmp = (uint8_t*)workspace + need;
    need += tmp_bytes(ds[i], R);
    if (out_u8) ds[i].out = out_u8 + (size_t)i * 3 * R * R;
    if (out_f32) {
      if (!out_f32[i]) return fail_img(who, i, "null pointer (fp32 output)");
      ds[i].fout = out_f32[i];
      ds[i].normalize = normalize ? normalize[i] != 0 : 0;
    }
  }
  if (need && !workspace) return fail(who, "null pointer (workspace)");
  if (workspace_bytes < need) {
    snprintf(g_msg, sizeof(g_msg), "%s: workspace too small: %zu bytes given, %zu needed (es_image_resize_workspace_bytes)", who, workspace_bytes, need);
    es_set_error(g_msg);
    return -1;
  }
  hipStream_t st = (hipStream_t)stream;
  const long long row3 = 3ll * R;
  for (int first = 0; first < count; first += kImgPerLaunch) {
    Batch b = {};
    b.R = R; b.filter = filter;
    const int n = count - first < kImgPerLaunch ? count - first : kImgPerLaunch;
    long long hmax = 0;
    for (int i = 0; i < n; ++i) {
      b.d[i] = ds[first + i];
      if (b.d[i].need_h && b.d[i].nrows * row3 > hmax) hmax = b.d[i].nrows * row3;
    }
    if (hmax) hipLaunchKernelGGL(resize_h_kernel, dim3((unsigned)((hmax + 255) / 256), n), dim3(256), 0, st, b);
    hipLaunchKernelGGL(resize_v_kernel, dim3((unsigned)((R * row3 + 255) / 256), n), dim3(256), 0, st, b);
  }
  if (hipGetLastError() != hipSuccess) { fail(who, "launch failed"); return -2; }
  return 0;
}

int es_image_resize_impl(const char* who, const es_image_u8* imgs, int count, uint8_t* out_u8, float* const* out_f32,
                         const int32_t* normalize, int R, void* workspace, size_t workspace_bytes, void* stream) {
  return es_image_resize_impl_ex(who, imgs, count, out_u8, out_f32, normalize, R, ES_FILTER_BILINEAR, ES_CROP_TORCHVISION, workspace, workspace_bytes, stream);
}

static int image_fit(const char* who, int height, int width, int R, int crop, int32_t out[4]) {
  if (!out) return fail(who, "null pointer (out)");
  if (height < 1 || width < 1) return fail(who, "height or width < 1");
  if (R < 1) return fail(who, "R < 1");
  if (!known_rules(who, ES_FILTER_BILINEAR, crop)) return -1;
  fit(height, width, R, crop, out);
  return 0;
}
extern "C" int es_image_fit(int height, int width, int R, int32_t out[4]) { return image_fit("es_image_fit", height, width, R, ES_CROP_TORCHVISION, out); }
extern "C" int es_image_fit_ex(int height, int width, int R, int crop, int32_t out[4]) { return image_fit("es_image_fit_ex", height, width, R, crop, out); }

extern "C" int es_image_resize_coeffs(int in, int out, int32_t* xmin, int32_t* ntaps, int32_t* k, int cap) {
  return resize_coeffs("es_image_resize_coeffs", ES_FILTER_BILINEAR, in, out, xmin, ntaps, k, cap);
}

extern "C" int es_image_resize_coeffs_ex(int filter, int in, int out, int32_t* xmin, int32_t* ntaps, int32_t* k, int cap) {
  if (!known_filter("es_image_resize_coeffs_ex", filter)) return -1;
  return resize_coeffs("es_image_resize_coeffs_ex", filter, in, out, xmin, ntaps, k, cap);
}

extern "C" size_t es_image_resize_workspace_bytes(const es_image_u8* imgs, int count, int R) {
  return workspace_bytes("es_image_resize_workspace_bytes", imgs, count, R, ES_FILTER_BILINEAR, ES_CROP_TORCHVISION);
}

extern "C" size_t es_image_resize_workspace_bytes_ex(const es_image_u8* imgs, int count, int R, int filter, int crop) {
  if (!known_rules("es_image_resize_workspace_bytes_ex", filter, crop)) return 0;
  return workspace_bytes("es_image_resize_workspace_bytes_ex", imgs, count, R, filter, crop);
}

extern "C" int es_image_resize_u8(const es_image_u8* imgs, int count, uint8_t* out, int R, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  if (!out) return fail("es_image_resize_u8", "null pointer (out)");
  return es_image_resize_impl("es_image_resize_u8", imgs, count, out, nullptr, nullptr, R, workspace, workspace_bytes, stream);
}

extern "C" int es_image_resize_u8_ex(const es_image_u8* imgs, int count, uint8_t* out, int R, int filter, int crop, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  if (!out) return fail("es_image_resize_u8_ex", "null pointer (out)");
  return es_image_resize_impl_ex("es_image_resize_u8_ex", imgs, count, out, nullptr, nullptr, R, filter, crop, workspace, workspace_bytes, stream);
}

extern "C" int es_image_u8_to_f32(const uint8_t* in, float* out_nchw, int count, int H, int W, int normalize, void* stream) {
  if (!in || !out_nchw) return fail("es_image_u8_to_f32", "null pointer");
  if (count < 1) return fail("es_image_u8_to_f32", "count < 1");
  if (H < 1 || W < 1) return fail("es_image_u8_to_f32", "height or width < 1");
  if (es_plan_recording()) return fail("es_image_u8_to_f32", "a plan is recording on this thread; the byte-image calls are never part of a plan");
  const long long HW = (long long)H * W, n = (long long)count * 3 * HW;
  if ((n + 255) / 256 > 0x7fffffffll) return fail("es_image_u8_to_f32", "too many elements for one launch");
  hipLaunchKernelGGL(u8_to_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, out_nchw, (long long)count, HW, normalize != 0);
  if (hipGetLastError() != hipSuccess) { fail("es_image_u8_to_f32", "launch failed"); return -2; }
  return 0;
}

extern "C" int es_image_f32_to_u8(const float* in_nchw, uint8_t* out_hwc, int B, int H, int W, void* stream) {
  if (!in_nchw || !out_hwc) return fail("es_image_f32_to_u8", "null pointer");
  if (B < 1) return fail("es_image_f32_to_u8", "count < 1 (B)");
  if (H < 1 || W < 1) return fail("es_image_f32_to_u8", "height or width < 1");
  if (es_plan_recording()) return fail("es_image_f32_to_u8", "a plan is recording on this thread; the byte-image calls are never part of a plan");
  const long long HW = (long long)H * W, n = (long long)B * ((HW + 3) / 4);
  if ((n + 255) / 256 > 0x7fffffffll) return fail("es_image_f32_to_u8", "too many elements for one launch");
  const int vec = HW % 4 == 0 && (uintptr_t)in_nchw % 16 == 0 && (uintptr_t)out_hwc % 4 == 0;
  hipLaunchKernelGGL(f32_to_u8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in_nchw, out_hwc, (long long)B, HW, vec);
  if (hipGetLastError() != hipSuccess) { fail("es_image_f32_to_u8", "launch failed"); return -2; }
  return 0;
}

extern "C" void es_sam_resize_shape(int height, int width, int S, int32_t out_hw[2]) {
  if (out_hw) { out_hw[0] = out_hw[1] = 0; if (height >= 1 && width >= 1 && S >= 1) sam_shape(height, width, S, out_hw); }
}

static int sam_check(const char* who, const es_image_u8* imgs, int count, int S) {
  if (check_images(who, imgs, count, S)) return -1;
  for (int i = 0; i < count; ++i) {
    int32_t hw[2];
    sam_shape(imgs[i].height, imgs[i].width, S, hw);
    if (hw[0] < 1 || hw[1] < 1) return fail_img(who, i, "the resized shorter side would be empty");
  }
  return 0;
}

extern "C" size_t es_sam_preprocess_u8_workspace_bytes(const es_image_u8* imgs, int count, int S) {
  if (sam_check("es_sam_preprocess_u8_workspace_bytes", imgs, count, S)) return 0;
  size_t need = 0;
  SamImg d;
  for (int i = 0; i < count; ++i) need += sam_plan(imgs[i], S, d);
  return need;
}

extern "C" int es_sam_preprocess_u8(const es_image_u8* imgs, int count, int S, const float mean[3], const float std[3], int dtype, void* out_nhwc,
                                    float* out_nchw, uint8_t* out_u8, int32_t* input_hw, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "es_sam_preprocess_u8";
  if (sam_check(who, imgs, count, S)) return -1;
  if (!mean || !std) return fail(who, "null pointer (mean / std)");
  if (!out_nhwc && !out_nchw && !out_u8) return fail(who, "null pointer (every output)");
  if (dtype != ES_F16 && dtype != ES_BF16) return fail(who, "dtype must be ES_F16 or ES_BF16");
  for (int c = 0; c < 3; ++c) if (!(std[c] > 0.f)) return fail(who, "std must be positive");
  if (es_plan_recording()) return fail(who, "a plan is recording on this thread; the byte-image calls are never part of a plan");
  std::vector<SamImg> ds((size_t)count);
  size_t need = 0;
  for (int i = 0; i < count; ++i) {
    SamImg& d = ds[i];
    const size_t bytes = sam_plan(imgs[i], S, d);
    uint8_t* at = (uint8_t*)workspace + need;
    if (d.need_h && d.need_v) { d.tmp = at; d.res = at + (((size_t)d.in_h * d.rw * 3 + 15) & ~(size_t)15); }
    else if (d.need_h) { d.tmp = at; d.res = at; }        // the horizontal pass alone: its result is the resized image
    else if (d.need_v) d.res = at;
    if (d.need_h || d.need_v) { d.pix = d.res; d.pix_pitch = 3ll * d.rw; d.pix_step = 3; }
    need += bytes;
    if (input_hw) { input_hw[2 * i] = d.rh; input_hw[2 * i + 1] = d.rw; }
  }
  if (need && !workspace) return fail(who, "null pointer (workspace)");
  if (workspace_bytes < need) {
    snprintf(g_msg, sizeof(g_msg), "%s: workspace too small: %zu bytes given, %zu needed (es_sam_preprocess_u8_workspace_bytes)", who, workspace_bytes, need);
    es_set_error(g_msg);
    return -1;
  }
  hipStream_t st = (hipStream_t)stream;
  for (int first = 0; first < count; first += kImgPerLaunch) {
    SamBatch b = {};
    b.S = S; b.first = first;
    for (int c = 0; c < 3; ++c) { b.mean[c] = mean[c]; b.std[c] = std[c]; }
    const int n = count - first < kImgPerLaunch ? count - first : kImgPerLaunch;
    long long hmax = 0, vmax = 0;
    for (int i = 0; i < n; ++i) {
      b.d[i] = ds[first + i];
      if (b.d[i].need_h) hmax = std::max(hmax, 3ll * b.d[i].in_h * b.d[i].rw);
      if (b.d[i].need_v) vmax = std::max(vmax, 3ll * b.d[i].rh * b.d[i].rw);
    }
    if (hmax) hipLaunchKernelGGL(sam_resize_h_kernel, dim3((unsigned)((hmax + 255) / 256), n), dim3(256), 0, st, b);
    if (vmax) hipLaunchKernelGGL(sam_resize_v_kernel, dim3((unsigned)((vmax + 255) / 256), n), dim3(256), 0, st, b);
    const dim3 grid((unsigned)(((long long)S * S + 255) / 256), n);
    if (dtype == ES_F16) hipLaunchKernelGGL(sam_normalize_kernel<_Float16>, grid, dim3(256), 0, st, b, (_Float16*)out_nhwc, out_nchw, out_u8);
    else hipLaunchKernelGGL(sam_normalize_kernel<__bf16>, grid, dim3(256), 0, st, b, (__bf16*)out_nhwc, out_nchw, out_u8);
  }
  if (hipGetLastError() != hipSuccess) { fail(who, "launch failed"); return -2; }
  return 0;
}

// ---- the windowed resize and create_processed_image ---------------------------------------------------------------------------------
namespace {

int window_check(const char* who, const es_image_u8* imgs, int count, const int32_t* geom, int out_h, int out_w, int filter) {
  if (!geom) return fail(who, "null pointer (geom)");
  if (out_h < 1 || out_w < 1) return fail(who, "out_h or out_w < 1");
  if (out_h > 16384 || out_w > 16384) return fail(who, "out_h or out_w > 16384");
  if (check_images(who, imgs, count, 1)) return -1;
  if (!known_filter(who, filter)) return -1;
  for (int i = 0; i < count; ++i) {
    const int32_t* g = geom + 4 * i;
    if (g[0] < 1 || g[1] < 1) return fail_img(who, i, "new_w or new_h < 1");
    if (g[0] > (1 << 24) || g[1] > (1 << 24)) return fail_img(who, i, "the resized image would pass 2^24 pixels on a side");
    if (g[2] < -(1 << 24) || g[2] > (1 << 24) || g[3] < -(1 << 24) || g[3] > (1 << 24)) return fail_img(who, i, "left or top beyond +-2^24");
  }
  return 0;
}

// geometry of one image: the kept columns and rows of the resized image, which passes run, the source rows the kept rows read
void window_plan(const es_image_u8& im, const int32_t g[4], int out_h, int out_w, int filter, WinDesc& d) {
  d.src = im.data; d.stride = im.row_stride;
  d.in_h = im.height; d.in_w = im.width; d.ch = im.channels;
  d.rw = g[0]; d.rh = g[1]; d.left = g[2]; d.top = g[3];
  d.need_h = d.rw != d.in_w;
  d.need_v = d.rh != d.in_h;
  const int x0 = d.left > 0 ? d.left : 0, x1 = std::min(d.left + out_w, d.rw);
  const int r0 = d.top > 0 ? d.top : 0, r1 = std::min(d.top + out_h, d.rh);
  d.x0 = x0; d.ncols = x1 > x0 ? x1 - x0 : 0;
  d.y0 = r0; d.nrows = r1 > r0 ? r1 - r0 : 0;
  if (d.ncols == 0 || d.nrows == 0) { d.ncols = d.nrows = 0; d.need_h = 0; }      // the window misses the image: all zeros
  else if (d.need_v) {
    int lo = d.in_h, hi = 0;
    for (int yy = r0; yy < r1; ++yy) {
      int ymin;
      const int n = resize_axis(filter, d.in_h, d.rh, yy, &ymin, [](int, int, int) {});
      lo = ymin < lo ? ymin : lo;
      hi = ymin + n > hi ? ymin + n : hi;
    }
    d.y0 = lo; d.nrows = hi - lo;
  }
  d.tmp = nullptr; d.out = nullptr;
}
size_t window_tmp_bytes(const WinDesc& d) { return d.need_h ? (size_t)d.nrows * 3 * (size_t)d.ncols : 0; }

int window_resize(const char* who, const es_image_u8* imgs, int count, const int32_t* geom, uint8_t* out, int out_h, int out_w, int filter,
                  void* workspace, size_t workspace_bytes, void* stream) {
  if (window_check(who, imgs, count, geom, out_h, out_w, filter)) return -1;
  if (!out) return fail(who, "null pointer (out)");
  if (es_plan_recording()) return fail(who, "a plan is recording on this thread; the byte-image calls are never part of a plan");
  std::vector<WinDesc> ds((size_t)count);
  size_t need = 0;
  for (int i = 0; i < count; ++i) {
    window_plan(imgs[i], geom + 4 * i, out_h, out_w, filter, ds[i]);
    ds[i].tmp = (uint8_t*)workspace + need;
    need += window_tmp_bytes(ds[i]);
    ds[i].out = out + (size_t)i * 3 * out_h * out_w;
  }
  if (need && !workspace) return fail(who, "null pointer (workspace)");
  if (workspace_bytes < need) {
    snprintf(g_msg, sizeof(g_msg), "%s: workspace too small: %zu bytes given, %zu needed", who, workspace_bytes, need);
    es_set_error(g_msg);
    return -1;
  }
  hipStream_t st = (hipStream_t)stream;
  const long long vtotal = 3ll * out_h * out_w;
  for (int first = 0; first < count; first += kImgPerLaunch) {
    WinBatch b = {};
    b.out_h = out_h; b.out_w = out_w; b.filter = filter;
    const int n = count - first < kImgPerLaunch ? count - first : kImgPerLaunch;
    long long hmax = 0;
    for (int i = 0; i < n; ++i) {
      b.d[i] = ds[first + i];
      if (b.d[i].need_h) hmax = std::max(hmax, 3ll * b.d[i].nrows * b.d[i].ncols);
    }
    if ((hmax + 255) / 256 > 0x7fffffffll) return fail(who, "too many elements for one launch");
    if (hmax) hipLaunchKernelGGL(window_h_kernel, dim3((unsigned)((hmax + 255) / 256), n), dim3(256), 0, st, b);
    hipLaunchKernelGGL(window_v_kernel, dim3((unsigned)((vtotal + 255) / 256), n), dim3(256), 0, st, b);
  }
  if (hipGetLastError() != hipSuccess) { fail(who, "launch failed"); return -2; }
  return 0;
}

size_t window_workspace(const char* who, const es_image_u8* imgs, int count, const int32_t* geom, int out_h, int out_w, int filter) {
  if (window_check(who, imgs, count, geom, out_h, out_w, filter)) return 0;
  size_t need = 0;
  WinDesc d;
  for (int i = 0; i < count; ++i) { window_plan(imgs[i], geom + 4 * i, out_h, out_w, filter, d); need += window_tmp_bytes(d); }
  return need;
}

constexpr int kPersonSize = 512;             // IMAGE_WIDTH = IMAGE_HEIGHT of extract_dataset.py
constexpr double kPersonMargin = 0.1;        // BOX_MARGIN

int person_geom(const char* who, const es_image_u8* imgs, int count, const double* boxes, std::vector<int32_t>& geom) {
  if (!boxes) return fail(who, "null pointer (boxes)");
  if (check_images(who, imgs, count, 1)) return -1;
  geom.resize((size_t)count * 4);
  for (int i = 0; i < count; ++i)
    if (!person_fit(imgs[i].height, imgs[i].width, boxes + 4 * i, kPersonSize, kPersonSize, kPersonMargin, &geom[(size_t)i * 4]))
      return fail_img(who, i, "the box (with its margin, inside the photo) is empty or gives a resized photo beyond 1 .. 2^24 pixels");
  return 0;
}

}  // namespace

extern "C" int es_person_crop_fit(int height, int width, const double box[4], int final_w, int final_h, double margin, int32_t out[4]) {
  const char* who = "es_person_crop_fit";
  if (!box || !out) return fail(who, "null pointer");
  if (height < 1 || width < 1) return fail(who, "height or width < 1");
  if (final_w < 1 || final_h < 1 || final_w > 16384 || final_h > 16384) return fail(who, "final_w or final_h outside 1 .. 16384");
  if (!(margin >= 0.0 && margin <= 16.0)) return fail(who, "margin outside 0 .. 16");
  for (int k = 0; k < 4; ++k) if (!(box[k] >= -1e9 && box[k] <= 1e9)) return fail(who, "a box coordinate is not a finite number of pixels");
  if (!person_fit(height, width, box, final_w, final_h, margin, out))
    return fail(who, "the box (with its margin, inside the photo) is empty or gives a resized photo beyond 1 .. 2^24 pixels");
  return 0;
}

extern "C" size_t es_image_resize_window_u8_workspace_bytes(const es_image_u8* imgs, int count, const int32_t* geom, int out_h, int out_w, int filter) {
  return window_workspace("es_image_resize_window_u8_workspace_bytes", imgs, count, geom, out_h, out_w, filter);
}

extern "C" int es_image_resize_window_u8(const es_image_u8* imgs, int count, const int32_t* geom, uint8_t* out, int out_h, int out_w, int filter,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  return window_resize("es_image_resize_window_u8", imgs, count, geom, out, out_h, out_w, filter, workspace, workspace_bytes, stream);
}

extern "C" size_t es_person_crop_u8_workspace_bytes(const es_image_u8* imgs, int count, const double* boxes) {
  std::vector<int32_t> geom;
  if (person_geom("es_person_crop_u8_workspace_bytes", imgs, count, boxes, geom)) return 0;
  return window_workspace("es_person_crop_u8_workspace_bytes", imgs, count, geom.data(), kPersonSize, kPersonSize, ES_FILTER_LANCZOS);
}

extern "C" int es_person_crop_u8(const es_image_u8* imgs, int count, const double* boxes, uint8_t* out, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  std::vector<int32_t> geom;
  if (person_geom("es_person_crop_u8", imgs, count, boxes, geom)) return -1;
  return window_resize("es_person_crop_u8", imgs, count, geom.data(), out, kPersonSize, kPersonSize, ES_FILTER_LANCZOS, workspace, workspace_bytes, stream);
}
