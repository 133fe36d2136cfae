// JPEG encoding (gfx950): RGB or gray bytes -> the bytes of Pillow's file, written by the device from SOI to EOI.  The per-sample and
// per-block integer rules, the tables, the header writer and the host twin are csrc/jpeg.h; include/edgestyle_hip.h states the format.
//
// 8 launches per 16 images (1 forward + 7 entropy), grid.y = image: images of different sizes and samplings share each launch and the
// workgroups past a smaller image's end leave at once.  Every workgroup has 256 threads.
//  1. jpeg_fdct_kernel       the mirror of jpeg_idct_kernel: 32 blocks of the coefficient buffer per workgroup, eight lanes per block.
//                            Lane j gathers row j of its block straight from the pixels (colour conversion and the downsampling taps
//                            are computed in the gather - FUSED, no component planes in the workspace: a plane would be written and read
//                            once each for nothing, the taps of neighbouring blocks do not overlap), runs the row pass in registers,
//                            writes it to an LDS tile (rows padded to 9 words), runs the column pass on column j, quantises, and stores
//                            row j of the coefficients as one 16-byte store.  A dummy block computes the real block whose DC it carries
//                            and zeroes the rest: no second pass.
//  2. jpeg_enc_length_kernel a thread per block IN SCAN ORDER (256 blocks = one chunk per workgroup): the bit length of its code (the DC
//                            predecessor comes from the scan geometry, esjpeg::scan_block), and the chunk's summary.
//  3. jpeg_enc_scan_kernel   one workgroup per image walks the chunk summaries in tiles of 256: where every chunk starts, and the total.
//  4. jpeg_enc_place_kernel  the bit position of every block (the scan inside the chunk, again, on the chunk's start), and the words of
//                            the bit stream and of the marker mask that will be used are zeroed.
//  5. jpeg_enc_emit_kernel   a thread per block codes it into the UNSTUFFED bit stream: 32-bit words, MSB first.  A word shared with a
//                            neighbour is combined by atomicOr into the zeroed word (order-independent), words a block owns alone are
//                            stored.  The first block of a restart interval also writes the 1-padding of the interval before it and
//                            the RSTn marker, and sets the marker's bit in the mask (a 0xFF that takes no stuffed zero).
//  6. jpeg_enc_count_kernel  0xFF data bytes per 1024 bytes of the stream.
//  7. jpeg_enc_scan2_kernel  one workgroup per image: prefix sum of those counts, the file's length, the header and EOI.
//  8. jpeg_enc_scatter_kernel every stream byte to its place in the file with the 0x00 after each 0xFF data byte; every store is bounded
//                            by the capacity.
// The prefix sum of step 2-4 is over functions, not numbers, so that it byte-aligns the intervals in the same pass: a run of blocks maps
// the bit position x it starts at to x + a (no marker inside) or to roundup8(x + a) + b (a: the bits before the first marker, b: all that
// follows its alignment, the 16 marker bits included).  Such functions compose to one of the same shape (compose() below), so they scan
// like sums, for any number of blocks.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "jpeg.h"
#include "plan.h"

extern "C" void es_set_error(const char* msg);

namespace {

using namespace esjpeg;

constexpr int kImgPerLaunch = 16;
constexpr int kMaxEncode = 64;
constexpr uint32_t kChunk = 256;                  // blocks per workgroup of the length / place / emit kernels
constexpr uint32_t kByteChunk = 1024;             // stream bytes per workgroup of the count / scatter kernels

__constant__ EncConst d_enc = make_enc_const();

struct Seg { uint32_t h, a, b; };                 // x -> h ? roundup8(x + a) + b : x + a
__host__ __device__ inline uint32_t r8(uint32_t x) { return (x + 7u) & ~7u; }
__device__ inline Seg compose(const Seg& f, const Seg& g) {       // f, then g
  if (!g.h) return f.h ? Seg{1u, f.a, f.b + g.a} : Seg{0u, f.a + g.a, 0u};
  return f.h ? Seg{1u, f.a, r8(f.b + g.a) + g.b} : Seg{1u, f.a + g.a, g.b};     // roundup8(x + f.a) is a multiple of 8: it leaves the inner roundup
}
__device__ inline uint32_t apply(const Seg& f, uint32_t x) { return f.h ? r8(x + f.a) + f.b : x + f.a; }
__device__ inline Seg block_seg(bool live, bool boundary, uint32_t len) {
  return !live ? Seg{0u, 0u, 0u} : boundary ? Seg{1u, 0u, 16u + len} : Seg{0u, len, 0u};
}

// Inclusive scan over the 256 threads of the workgroup (every thread calls it); on return lds[t] holds thread t's inclusive value.
template <class T, class Op>
__device__ inline T wg_scan(T v, T* lds, Op op) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    T u = v;
    if (t >= d) u = op(lds[t - d], v);
    __syncthreads();
    v = u;
    lds[t] = v;
    __syncthreads();
  }
  return v;
}
struct SegOp { __device__ inline Seg operator()(const Seg& f, const Seg& g) const { return compose(f, g); } };
struct SumOp { __device__ inline uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; } };

template <class T>
__device__ inline T pick3(const T a[3], int c) { return c == 0 ? a[0] : c == 1 ? a[1] : a[2]; }

// ---- forward ----------------------------------------------------------------------------------------------------------------------
struct FwdDesc {
  EncGeom g;
  const uint8_t* img;
  long long stride;
  int16_t* coef;
};
struct FwdBatch { FwdDesc d[kImgPerLaunch]; int32_t quality; };

__global__ __launch_bounds__(256) void jpeg_fdct_kernel(const FwdBatch b) {
  __shared__ int32_t tile[32][8][9];
  const FwdDesc& d = b.d[blockIdx.y];
  const EncGeom& G = d.g;
  const uint32_t n0 = G.nblk[0], n01 = n0 + G.nblk[1], total = n01 + G.nblk[2];
  if (blockIdx.x * 32u >= total) return;          // (the whole workgroup: no barrier is left behind)
  const int sub = threadIdx.x >> 3, j = threadIdx.x & 7;
  const uint32_t g = blockIdx.x * 32u + sub;
  const bool live = g < total;
  const int c = g < n0 ? 0 : g < n01 ? 1 : 2;
  bool dummy = false;
  int32_t in[8], o[8];
  if (live) {
    const uint32_t lb = g - (c == 0 ? 0u : c == 1 ? n0 : n01);
    const uint32_t bw = (uint32_t)pick3(G.blocks_w, c);
    const uint32_t by = lb / bw, bx = lb - by * bw;
    int sx, sy;
    dummy = dummy_source((int)bx, (int)by, pick3(G.rbw, c), pick3(G.rbh, c), c == 0 ? G.h : 1, &sx, &sy);
    gather_row(G, d.img, (size_t)d.stride, c, sx, sy, j, in);
    fdct_1d(in, o, false);
#pragma unroll
    for (int k = 0; k < 8; ++k) tile[sub][j][k] = o[k];
  }
  __syncthreads();
  if (live) {                                     // column j: read and written by this lane alone
#pragma unroll
    for (int k = 0; k < 8; ++k) in[k] = tile[sub][k][j];
    fdct_1d(in, o, true);
#pragma unroll
    for (int k = 0; k < 8; ++k)
      tile[sub][k][j] = dummy && (k || j) ? 0 : (int32_t)quantise(o[k], (uint16_t)quant_entry(d_enc.base_q[c ? 1 : 0][8 * k + j], b.quality));
  }
  __syncthreads();
  if (!live) return;
  uint32_t w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) w[k] = ((uint32_t)tile[sub][j][2 * k] & 0xffffu) | (uint32_t)tile[sub][j][2 * k + 1] << 16;
  *reinterpret_cast<uint4*>(d.coef + (size_t)g * 64 + j * 8) = make_uint4(w[0], w[1], w[2], w[3]);
}

// ---- entropy ----------------------------------------------------------------------------------------------------------------------
struct EntDesc {
  EncGeom g;
  const int16_t* coef;
  uint32_t* pos;          // [total]: the block's bit length, then its bit position
  Seg* csum;              // [nchunks]
  uint32_t* cstart;       // [nchunks]
  uint32_t* totals;       // [0]: bytes of the unstuffed stream
  uint32_t* stream;       // [stream_words]
  uint32_t* mask;         // [mask_words]: bit (i & 31) of word i >> 5: stream byte i is a marker's 0xFF
  uint32_t* ffc;          // [byte chunks]: 0xFF data bytes per chunk, then their exclusive prefix sum
  uint8_t* out;
  unsigned long long cap;
  uint32_t* length;
  uint32_t total, nchunks, stream_words, mask_words, hdr;
};
struct EntBatch { EntDesc d[kImgPerLaunch]; int32_t quality; };

__global__ __launch_bounds__(256) void jpeg_enc_length_kernel(const EntBatch b) {
  __shared__ Seg lds[256];
  const EntDesc& d = b.d[blockIdx.y];
  if (blockIdx.x >= d.nchunks) return;
  const uint32_t s = blockIdx.x * kChunk + threadIdx.x;
  const bool live = s < d.total;
  uint32_t len = 0;
  bool boundary = false;
  if (live) {
    const ScanBlock sb = scan_block(d.g, s);
    LengthSink sink;
    code_block(d_enc, sb.c ? 1 : 0, d.coef + (size_t)sb.block * 64, sb.pred == ~0u ? 0 : (int)d.coef[(size_t)sb.pred * 64], sink);
    len = sink.bits;
    boundary = sb.boundary;
    d.pos[s] = len;
  }
  wg_scan(block_seg(live, boundary, len), lds, SegOp());
  if (threadIdx.x == 255) d.csum[blockIdx.x] = lds[255];
}

__global__ __launch_bounds__(256) void jpeg_enc_scan_kernel(const EntBatch b) {
  __shared__ Seg lds[256];
  const EntDesc& d = b.d[blockIdx.y];
  uint32_t x = 0;                                 // where the tile starts; the same in every thread
  for (uint32_t base = 0; base < d.nchunks; base += 256) {
    const uint32_t i = base + threadIdx.x;
    wg_scan(i < d.nchunks ? d.csum[i] : Seg{0u, 0u, 0u}, lds, SegOp());
    if (i < d.nchunks) d.cstart[i] = threadIdx.x ? apply(lds[threadIdx.x - 1], x) : x;
    x = apply(lds[255], x);
    __syncthreads();                              // lds is written again by the next tile
  }
  if (threadIdx.x == 0) d.totals[0] = r8(x) / 8;  // the last interval is padded to a byte as well
}

__global__ __launch_bounds__(256) void jpeg_enc_place_kernel(const EntBatch b) {
  __shared__ Seg lds[256];
  const EntDesc& d = b.d[blockIdx.y];
  // zero what the stream and the mask will use (grid-stride: the grid is sized by the blocks, the stream by their codes)
  const uint32_t bytes = d.totals[0];
  uint32_t sw = bytes / 4 + 2, mw = bytes / 32 + 1;
  sw = sw < d.stream_words ? sw : d.stream_words;
  mw = mw < d.mask_words ? mw : d.mask_words;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < sw; i += gridDim.x * 256u) d.stream[i] = 0;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < mw; i += gridDim.x * 256u) d.mask[i] = 0;
  if (blockIdx.x >= d.nchunks) return;
  const uint32_t s = blockIdx.x * kChunk + threadIdx.x;
  const bool live = s < d.total;
  const uint32_t len = live ? d.pos[s] : 0u;
  const bool boundary = live && scan_block(d.g, s).boundary;
  wg_scan(block_seg(live, boundary, len), lds, SegOp());
  const uint32_t x0 = d.cstart[blockIdx.x];
  if (live) d.pos[s] = threadIdx.x ? apply(lds[threadIdx.x - 1], x0) : x0;
}

// bits into the zeroed word stream from bit position `at` on, MSB first
struct DevBits {
  uint32_t* w;
  uint32_t wi, words;     // words: the stream's size; no store goes past it whatever the positions are
  uint64_t acc = 0;       // the pending bits, from the top
  int fill;               // how many (below 32 between calls); at first the bits of word wi that belong to earlier blocks
  bool shared;            // word wi holds bits of another block: combine, do not store
  __device__ DevBits(uint32_t* w_, uint32_t words_, uint32_t at) : w(w_), wi(at >> 5), words(words_), fill((int)(at & 31u)), shared((at & 31u) != 0) {}
  __device__ inline void put(uint32_t bits, int n) {            // n <= 16, bits < 2^n
    if (n == 0) return;
    acc |= (uint64_t)bits << (64 - fill - n);
    fill += n;
    if (fill >= 32) {
      const uint32_t v = (uint32_t)(acc >> 32);
      if (wi >= words) {}
      else if (shared) atomicOr(w + wi, v);
      else w[wi] = v;
      shared = false;
      ++wi;
      acc <<= 32;
      fill -= 32;
    }
  }
  __device__ inline void bad() {}
  __device__ inline uint32_t at() const { return wi * 32u + (uint32_t)fill; }
  __device__ inline void finish() {               // the last word is shared with whatever follows
    if (fill > 0 && acc != 0 && wi < words) atomicOr(w + wi, (uint32_t)(acc >> 32));
  }
};

__global__ __launch_bounds__(256) void jpeg_enc_emit_kernel(const EntBatch b) {
  const EntDesc& d = b.d[blockIdx.y];
  if (blockIdx.x >= d.nchunks) return;
  const uint32_t s = blockIdx.x * kChunk + threadIdx.x;
  if (s >= d.total) return;
  const ScanBlock sb = scan_block(d.g, s);
  const uint32_t x = d.pos[s];
  DevBits w(d.stream, d.stream_words, x);
  if (sb.boundary) {
    const uint32_t start = r8(x);
    w.put((1u << (start - x)) - 1u, (int)(start - x));          // the interval before this one ends in 1-bits
    const uint32_t n = s / blocks_per_mcu(d.g) / (uint32_t)d.g.restart_interval - 1u;      // the marker's number
    w.put(0xFFD0u + (n & 7u), 16);
    if ((start >> 8) < d.mask_words) atomicOr(d.mask + (start >> 8), 1u << ((start >> 3) & 31u));
  }
  code_block(d_enc, sb.c ? 1 : 0, d.coef + (size_t)sb.block * 64, sb.pred == ~0u ? 0 : (int)d.coef[(size_t)sb.pred * 64], w);
  if (s == d.total - 1) {
    const uint32_t e = w.at();
    w.put((1u << (r8(e) - e)) - 1u, (int)(r8(e) - e));
  }
  w.finish();
}

// the four bytes of stream word i (the first in the top bits) and which of them are 0xFF data bytes
__device__ inline uint32_t ff_bits(const EntDesc& d, uint32_t i, uint32_t bytes, uint32_t* word) {
  uint32_t m = 0;
  *word = 0;
  if (i * 4u >= bytes || i >= d.stream_words) return 0;
  const uint32_t v = d.stream[i];
  const uint32_t marker = d.mask[i >> 3] >> ((i & 7u) * 4u);
  *word = v;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (i * 4u + k < bytes && ((v >> (24 - 8 * k)) & 255u) == 255u && !((marker >> k) & 1u)) m |= 1u << k;
  return m;
}

__global__ __launch_bounds__(256) void jpeg_enc_count_kernel(const EntBatch b) {
  __shared__ uint32_t lds[256];
  const EntDesc& d = b.d[blockIdx.y];
  const uint32_t bytes = d.totals[0];
  if (blockIdx.x * kByteChunk >= bytes) return;
  uint32_t word;
  const uint32_t m = ff_bits(d, blockIdx.x * 256u + threadIdx.x, bytes, &word);
  wg_scan((uint32_t)__popc(m), lds, SumOp());
  if (threadIdx.x == 255) d.ffc[blockIdx.x] = lds[255];
}

struct LdsBytes {
  uint8_t* p;
  uint32_t n;
  __device__ inline void byte(uint8_t v) { p[n++] = v; }
};

__global__ __launch_bounds__(256) void jpeg_enc_scan2_kernel(const EntBatch b) {
  __shared__ uint32_t lds[256];
  __shared__ uint8_t hdr[kMaxHeaderBytes + 3];
  const EntDesc& d = b.d[blockIdx.y];
  const uint32_t bytes = d.totals[0];
  const uint32_t nb = (bytes + kByteChunk - 1) / kByteChunk;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < nb; base += 256) {
    const uint32_t i = base + threadIdx.x;
    wg_scan(i < nb ? d.ffc[i] : 0u, lds, SumOp());
    if (i < nb) d.ffc[i] = carry + (threadIdx.x ? lds[threadIdx.x - 1] : 0u);
    carry += lds[255];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    LdsBytes o{hdr, 0};
    write_header(d_enc, d.g.width, d.g.height, d.g.components, d.g.h, d.g.v, b.quality, d.g.restart_interval, o);
  }
  __syncthreads();
  const unsigned long long eoi = (unsigned long long)d.hdr + bytes + carry;
  for (uint32_t i = threadIdx.x; i < d.hdr; i += 256)
    if (i < d.cap) d.out[i] = hdr[i];
  if (threadIdx.x == 0) {
    if (eoi < d.cap) d.out[eoi] = 0xFF;
    if (eoi + 1 < d.cap) d.out[eoi + 1] = 0xD9;
    *d.length = (uint32_t)(eoi + 2);
  }
}

__global__ __launch_bounds__(256) void jpeg_enc_scatter_kernel(const EntBatch b) {
  __shared__ uint32_t lds[256];
  const EntDesc& d = b.d[blockIdx.y];
  const uint32_t bytes = d.totals[0];
  if (blockIdx.x * kByteChunk >= bytes) return;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  uint32_t word;
  const uint32_t m = ff_bits(d, i, bytes, &word);
  wg_scan((uint32_t)__popc(m), lds, SumOp());
  unsigned long long o = (unsigned long long)d.hdr + (unsigned long long)i * 4u + d.ffc[blockIdx.x] + (threadIdx.x ? lds[threadIdx.x - 1] : 0u);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (i * 4u + k >= bytes) break;
    if (o < d.cap) d.out[o] = (uint8_t)(word >> (24 - 8 * k));
    ++o;
    if ((m >> k) & 1u) {
      if (o < d.cap) d.out[o] = 0;
      ++o;
    }
  }
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------
thread_local char g_msg[256];
int fail(const char* who, const char* what) {
  snprintf(g_msg, sizeof(g_msg), "%s: %s", who, what);
  es_set_error(g_msg);
  return -1;
}

inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }
struct Layout {
  size_t coef, pos, csum, cstart, totals, stream, mask, ffc, bytes;
  uint32_t total, nchunks, stream_words, mask_words, bchunks;
};
Layout layout(const es_jpeg_info& I) {
  Layout L;
  uint64_t blocks = 0;
  for (int c = 0; c < I.components; ++c) blocks += component_blocks(I, c);
  const uint64_t U = unstuffed_bound(I);          // below 2^29: checked by device_ok
  L.total = (uint32_t)blocks;
  L.nchunks = (uint32_t)((blocks + kChunk - 1) / kChunk);
  L.stream_words = (uint32_t)(U / 4 + 2);
  L.mask_words = L.stream_words / 8 + 1;
  L.bchunks = (uint32_t)((U + kByteChunk - 1) / kByteChunk);
  size_t at = 0;
  L.coef = at;   at += up16(coeff_count(I) * sizeof(int16_t));
  L.pos = at;    at += up16((size_t)L.total * 4);
  L.csum = at;   at += up16((size_t)L.nchunks * sizeof(Seg));
  L.cstart = at; at += up16((size_t)L.nchunks * 4);
  L.totals = at; at += 16;
  L.stream = at; at += up16((size_t)L.stream_words * 4);
  L.mask = at;   at += up16((size_t)L.mask_words * 4);
  L.ffc = at;    at += up16((size_t)L.bchunks * 4);
  L.bytes = at;
  return L;
}
// the device counts bits in 32
const char* size_ok(const es_jpeg_info& I) {
  return unstuffed_bound(I) >= (1ull << 29) ? "the image is too large: its size bound (es_jpeg_encode_capacity) must stay below 2^30 bytes" : nullptr;
}
const char* check_image(const es_image_u8& im, bool device) {
  if (!im.data) return "an image without memory";
  if (im.channels == 4) return "cannot write mode RGBA as JPEG";
  if (im.channels != 1 && im.channels != 3) return "1 or 3 channels expected";
  if (im.width < 1 || im.height < 1 || im.width > 65535 || im.height > 65535) return "height or width of 0 or above 65535";
  if (im.row_stride < (int64_t)im.width * im.channels) return "a row stride below width * channels";
  (void)device;
  return nullptr;
}
const char* check_infos(const es_jpeg_info* infos, int count, const es_jpeg_encode_params* P) {
  if (!infos || !P) return "null pointer";
  if (count < 1) return "count < 1";
  const char* why = nullptr;
  for (int i = 0; i < count; ++i) {
    if (!encode_info_ok(infos + i, P, &why)) return why;
    if ((why = size_ok(infos[i]))) return why;
  }
  return nullptr;
}
const char* images_to_infos(const es_image_u8* images, int count, const es_jpeg_encode_params* P, std::vector<es_jpeg_info>& infos) {
  if (!images || !P) return "null pointer";
  if (count < 1) return "count < 1";
  infos.resize((size_t)count);
  const char* why = nullptr;
  for (int i = 0; i < count; ++i) {
    if ((why = check_image(images[i], true))) return why;
    if (!encode_geometry(images[i].width, images[i].height, images[i].channels, P, infos[(size_t)i], &why)) return why;
    if ((why = size_ok(infos[(size_t)i]))) return why;
  }
  return nullptr;
}

int launch_forward(const char* who, const es_image_u8* images, const es_jpeg_info* infos, int count, int quality, int16_t* const* coeffs,
                   hipStream_t stream) {
  for (int first = 0; first < count; first += kImgPerLaunch) {
    const int n = count - first < kImgPerLaunch ? count - first : kImgPerLaunch;
    FwdBatch b;
    memset(&b, 0, sizeof(b));
    b.quality = quality;
    uint32_t groups = 0;
    for (int i = 0; i < n; ++i) {
      FwdDesc& d = b.d[i];
      d.g = enc_geom(infos[first + i], images[first + i].channels);
      d.img = images[first + i].data;
      d.stride = images[first + i].row_stride;
      d.coef = coeffs[first + i];
      const uint32_t g = (d.g.nblk[0] + d.g.nblk[1] + d.g.nblk[2] + 31) / 32;
      groups = g > groups ? g : groups;
    }
    hipLaunchKernelGGL(jpeg_fdct_kernel, dim3(groups, (unsigned)n), dim3(256), 0, stream, b);
    if (hipGetLastError() != hipSuccess) { fail(who, "launch failed"); return -2; }
  }
  return 0;
}

// ws: 16-byte aligned, the images' regions one after another (Layout::bytes each)
int launch_entropy(const char* who, const es_jpeg_info* infos, int count, int quality, const int16_t* const* coeffs, uint8_t* const* out,
                   const size_t* capacity, uint32_t* lengths, uint8_t* ws, hipStream_t stream) {
  for (int first = 0; first < count; first += kImgPerLaunch) {
    const int n = count - first < kImgPerLaunch ? count - first : kImgPerLaunch;
    EntBatch b;
    memset(&b, 0, sizeof(b));
    b.quality = quality;
    uint32_t chunks = 0, bchunks = 0;
    for (int i = 0; i < n; ++i) {
      const es_jpeg_info& I = infos[first + i];
      const Layout L = layout(I);
      EntDesc& d = b.d[i];
      d.g = enc_geom(I, I.components);
      d.coef = coeffs[first + i];
      d.pos = (uint32_t*)(ws + L.pos);
      d.csum = (Seg*)(ws + L.csum);
      d.cstart = (uint32_t*)(ws + L.cstart);
      d.totals = (uint32_t*)(ws + L.totals);
      d.stream = (uint32_t*)(ws + L.stream);
      d.mask = (uint32_t*)(ws + L.mask);
      d.ffc = (uint32_t*)(ws + L.ffc);
      d.out = out[first + i];
      d.cap = capacity[first + i];
      d.length = lengths + first + i;
      d.total = L.total; d.nchunks = L.nchunks; d.stream_words = L.stream_words; d.mask_words = L.mask_words;
      d.hdr = header_bytes(I.components, I.restart_interval);
      ws += L.bytes;
      chunks = L.nchunks > chunks ? L.nchunks : chunks;
      bchunks = L.bchunks > bchunks ? L.bchunks : bchunks;
    }
    const dim3 gc(chunks, (unsigned)n), gb(bchunks, (unsigned)n), one(1, (unsigned)n);
    hipLaunchKernelGGL(jpeg_enc_length_kernel, gc, dim3(256), 0, stream, b);
    hipLaunchKernelGGL(jpeg_enc_scan_kernel, one, dim3(256), 0, stream, b);
    hipLaunchKernelGGL(jpeg_enc_place_kernel, gc, dim3(256), 0, stream, b);
    hipLaunchKernelGGL(jpeg_enc_emit_kernel, gc, dim3(256), 0, stream, b);
    hipLaunchKernelGGL(jpeg_enc_count_kernel, gb, dim3(256), 0, stream, b);
    hipLaunchKernelGGL(jpeg_enc_scan2_kernel, one, dim3(256), 0, stream, b);
    hipLaunchKernelGGL(jpeg_enc_scatter_kernel, gb, dim3(256), 0, stream, b);
    if (hipGetLastError() != hipSuccess) { fail(who, "launch failed"); return -2; }
  }
  return 0;
}

size_t workspace_need(const es_jpeg_info* infos, int count) {
  size_t need = 16;                               // room to start on a 16-byte boundary
  for (int i = 0; i < count; ++i) need += layout(infos[i]).bytes;
  return need;
}

}  // namespace

extern "C" int es_jpeg_encode_info_host(int width, int height, int channels, const es_jpeg_encode_params* params, es_jpeg_info* info) {
  const char* who = "es_jpeg_encode_info_host";
  if (!params || !info) return fail(who, "null pointer");
  const char* why = nullptr;
  es_jpeg_info I;
  if (!encode_geometry(width, height, channels, params, I, &why)) return fail(who, why);
  *info = I;
  return 0;
}

extern "C" int es_jpeg_header_host(const es_jpeg_info* info, const es_jpeg_encode_params* params, uint8_t* out, size_t cap, size_t* n) {
  const char* who = "es_jpeg_header_host";
  if (!out || !n) return fail(who, "null pointer");
  const char* why = nullptr;
  if (!encode_info_ok(info, params, &why)) return fail(who, why);
  BoundedBytes o{out, cap, 0};
  write_header(kEnc, info->width, info->height, info->components, info->h[0], info->v[0], params->quality, info->restart_interval, o);
  *n = o.n;
  return o.n <= cap ? 0 : fail(who, "the header does not fit the capacity");
}

extern "C" size_t es_jpeg_encode_capacity(const es_jpeg_info* info, const es_jpeg_encode_params* params) {
  if (const char* why = check_infos(info, 1, params)) { fail("es_jpeg_encode_capacity", why); return 0; }
  return (size_t)capacity_bound(*info);
}

extern "C" size_t es_jpeg_encode_workspace_bytes(const es_jpeg_info* infos, int count, const es_jpeg_encode_params* params) {
  if (const char* why = check_infos(infos, count, params)) { fail("es_jpeg_encode_workspace_bytes", why); return 0; }
  return workspace_need(infos, count);
}

extern "C" int es_jpeg_forward(const es_image_u8* images, int count, const es_jpeg_encode_params* params, int16_t* const* coeffs_dev,
                               void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "es_jpeg_forward";
  (void)workspace; (void)workspace_bytes;
  if (!coeffs_dev) return fail(who, "null pointer");
  std::vector<es_jpeg_info> infos;
  if (const char* why = images_to_infos(images, count, params, infos)) return fail(who, why);
  if (es_plan_recording()) return fail(who, "a plan is recording on this thread; the JPEG calls are never part of a plan");
  for (int i = 0; i < count; ++i) {
    if (!coeffs_dev[i]) return fail(who, "null pointer");
    if ((uintptr_t)coeffs_dev[i] % 16) return fail(who, "coefficients must be 16-byte aligned");
  }
  return launch_forward(who, images, infos.data(), count, params->quality, coeffs_dev, (hipStream_t)stream);
}

extern "C" int es_jpeg_forward_host(const es_image_u8* images, int count, const es_jpeg_encode_params* params, int16_t* const* coeffs) {
  const char* who = "es_jpeg_forward_host";
  if (!coeffs) return fail(who, "null pointer");
  std::vector<es_jpeg_info> infos;
  if (const char* why = images_to_infos(images, count, params, infos)) return fail(who, why);
  for (int i = 0; i < count; ++i)
    if (!coeffs[i]) return fail(who, "null pointer");
  for (int i = 0; i < count; ++i) forward_host(infos[(size_t)i], params->quality, images[i].data, (size_t)images[i].row_stride, coeffs[i]);
  return 0;
}

extern "C" int es_jpeg_entropy_encode(const es_jpeg_info* infos, int count, const es_jpeg_encode_params* params, const int16_t* const* coeffs_dev,
                                      uint8_t* const* out_dev, const size_t* capacity, uint32_t* lengths_dev, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  const char* who = "es_jpeg_entropy_encode";
  if (!coeffs_dev || !out_dev || !capacity || !lengths_dev || !workspace) return fail(who, "null pointer");
  if (const char* why = check_infos(infos, count, params)) return fail(who, why);
  if (es_plan_recording()) return fail(who, "a plan is recording on this thread; the JPEG calls are never part of a plan");
  if ((uintptr_t)lengths_dev % 4) return fail(who, "lengths must be 4-byte aligned");
  for (int i = 0; i < count; ++i) {
    if (!coeffs_dev[i] || !out_dev[i]) return fail(who, "null pointer");
    if ((uintptr_t)coeffs_dev[i] % 16) return fail(who, "coefficients must be 16-byte aligned");
  }
  if (workspace_bytes < workspace_need(infos, count)) return fail(who, "workspace too small (es_jpeg_encode_workspace_bytes)");
  uint8_t* ws = (uint8_t*)(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  return launch_entropy(who, infos, count, params->quality, coeffs_dev, out_dev, capacity, lengths_dev, ws, (hipStream_t)stream);
}

extern "C" int es_jpeg_entropy_encode_host(const es_jpeg_info* infos, int count, const es_jpeg_encode_params* params, const int16_t* const* coeffs,
                                           uint8_t* const* out, const size_t* capacity, uint32_t* lengths) {
  const char* who = "es_jpeg_entropy_encode_host";
  if (!coeffs || !out || !capacity || !lengths) return fail(who, "null pointer");
  if (const char* why = check_infos(infos, count, params)) return fail(who, why);
  for (int i = 0; i < count; ++i)
    if (!coeffs[i] || !out[i]) return fail(who, "null pointer");
  bool any_bad = false;
  for (int i = 0; i < count; ++i) {
    bool bad = false;
    lengths[i] = (uint32_t)entropy_encode_host(infos[i], params->quality, coeffs[i], out[i], capacity[i], &bad);
    any_bad |= bad;
  }
  return any_bad ? fail(who, "a coefficient outside the baseline categories (|DC difference| >= 2048 or |AC| >= 1024)") : 0;
}

extern "C" int es_jpeg_encode_u8(const es_image_u8* images, int count, const es_jpeg_encode_params* params, uint8_t* const* out_dev,
                                 const size_t* capacity, uint32_t* lengths_dev, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "es_jpeg_encode_u8";
  if (!out_dev || !capacity || !lengths_dev || !workspace) return fail(who, "null pointer");
  if (count > kMaxEncode) return fail(who, "count > 64");
  std::vector<es_jpeg_info> infos;
  if (const char* why = images_to_infos(images, count, params, infos)) return fail(who, why);
  if (es_plan_recording()) return fail(who, "a plan is recording on this thread; the JPEG calls are never part of a plan");
  if ((uintptr_t)lengths_dev % 4) return fail(who, "lengths must be 4-byte aligned");
  for (int i = 0; i < count; ++i)
    if (!out_dev[i]) return fail(who, "null pointer");
  if (workspace_bytes < workspace_need(infos.data(), count)) return fail(who, "workspace too small (es_jpeg_encode_workspace_bytes)");
  uint8_t* ws = (uint8_t*)(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  int16_t* coeffs[kMaxEncode];
  uint8_t* at = ws;
  for (int i = 0; i < count; ++i) {
    const Layout L = layout(infos[(size_t)i]);
    coeffs[i] = (int16_t*)(at + L.coef);
    at += L.bytes;
  }
  if (int rc = launch_forward(who, images, infos.data(), count, params->quality, coeffs, (hipStream_t)stream)) return rc;
  return launch_entropy(who, infos.data(), count, params->quality, coeffs, out_dev, capacity, lengths_dev, ws, (hipStream_t)stream);
}

extern "C" int es_jpeg_encode_host(const es_image_u8* images, int count, const es_jpeg_encode_params* params, uint8_t* const* out,
                                   const size_t* capacity, uint32_t* lengths) {
  const char* who = "es_jpeg_encode_host";
  if (!out || !capacity || !lengths) return fail(who, "null pointer");
  std::vector<es_jpeg_info> infos;
  if (const char* why = images_to_infos(images, count, params, infos)) return fail(who, why);
  for (int i = 0; i < count; ++i)
    if (!out[i]) return fail(who, "null pointer");
  std::vector<int16_t> coeffs;
  for (int i = 0; i < count; ++i) {
    const es_jpeg_info& I = infos[(size_t)i];
    coeffs.resize(coeff_count(I));
    forward_host(I, params->quality, images[i].data, (size_t)images[i].row_stride, coeffs.data());
    bool bad = false;
    lengths[i] = (uint32_t)entropy_encode_host(I, params->quality, coeffs.data(), out[i], capacity[i], &bad);
  }
  return 0;
}
