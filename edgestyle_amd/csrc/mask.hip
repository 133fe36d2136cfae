// Mask post-processing (gfx950): binary morphology on bit-packed masks, 8-connected largest component by union-find, boolean
// algebra, draw_binary_mask and the reference's create_sam_images recipe as one call.  Integer arithmetic only.
//
// The reference runs this on the host between its segmenter and try_on (extract_dataset.py:316-351, :394-502; inference.py:322-447)
// with cv2.dilate / cv2.erode, skimage's closing(square(k)) and label / regionprops.  Restated here (include/edgestyle_hip.h has the
// semantics): dilate_r / erode_r are OR / AND over the (2r+1)^2 window clipped to the image.
//
// Packing.  A mask is H rows of WW = ceil(W / 64) 64-bit words, bit b of word w of a row = pixel 64 w + b; the bits past W in a
// row's last word are stored as zero, always.  One wave packs one word with one __ballot.  A morphology step is one launch, one
// thread per output word: OR / AND of the rows y-r..y+r (clipped) of the word and its two neighbours, then the horizontal window
// by shifts over that 192-bit strip (|r| <= 15 < 64: one neighbour word each side is enough).  OR and AND are separable and
// commute, so rows-first equals columns-first.  For an erosion what lies outside the image reads as ones (a clipped window):
// missing neighbour words and the bits past W are set on the way in, and the bits past W cleared again on the way out.  Every
// step reads one packed buffer and writes the other: the words stay in L2 at any size the API admits, and no step depends on LDS
// holding a whole mask.
//
// Components.  label is int32 [H, W] per mask.  Invariant: label[i] <= i for every true pixel, and label[i] is a pixel of the same
// component - every link points from a larger to a smaller linear index, so every pointer chase ends, at the component's first
// pixel in row-major order once all unions are done.  init links each pixel to the start of its horizontal run inside its word;
// merge unites each pixel with those of its W, NW, N, NE neighbours that the others do not already imply (the proof is by
// induction in raster order, next to the code); union is find both roots, atomicMin the larger root's link to the smaller, and,
// where the atomic shows that the larger was no root any more, go on from the link it had.  Reads that race with these atomics may
// be stale: a stale link is an older link of the same chain, still points down, and the atomic's return value is what decides.
// count then compresses every pixel to its root and adds the areas at the roots (one integer atomicAdd per distinct root per
// wave); argmax takes the largest (area, -root) pair with a 64-bit atomicMax per mask, which is the reference's tie rule; select
// keeps the winner's pixels.  Five launches, whatever the pixels are.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/edgestyle_hip.h"
#include "plan.h"

extern "C" void es_set_error(const char* msg);

namespace {

typedef unsigned long long u64;
constexpr int kMaxSide = 4096, kMaxCount = 4096, kMaxChain = 16, kMaxRadius = 15;
constexpr int kImgPerLaunch = 16;

// the masks a launch packs: mask m (grid.y) is image m / nslot of p[m % nslot], each [count, H, W] bytes
struct Src { const uint8_t* p[4]; int32_t nslot; };
// signed radius per slot (m % nslot): the reference closes the head mask with another square than the other three
struct Radii { int32_t r[4]; int32_t nslot; };
struct ImgBatch { const uint8_t* data[kImgPerLaunch]; long long stride[kImgPerLaunch]; int32_t ch[kImgPerLaunch]; };

// ---- pixel kernels: grid (ceil(H * WW / 4), masks), 256 threads; one WAVE per packed word, lane = bit.  Whole waves leave
// together (the word index is wave-uniform), so every __ballot below sees all 64 lanes.
#define ES_MASK_PIXEL_PROLOGUE                                          \
  const int word = blockIdx.x * 4 + (threadIdx.x >> 6);                 \
  const int lane = threadIdx.x & 63;                                    \
  if (word >= H * WW) return;                                           \
  const int m = blockIdx.y, y = word / WW, x = (word - y * WW) * 64 + lane; \
  const size_t HWW = (size_t)H * WW, HW = (size_t)H * W;                \
  (void)HW; (void)HWW; (void)m; (void)x

__global__ __launch_bounds__(256) void mask_pack_kernel(const Src s, u64* __restrict__ dst, int H, int W, int WW) {
  ES_MASK_PIXEL_PROLOGUE;
  const uint8_t* src = s.p[m % s.nslot] + (size_t)(m / s.nslot) * HW;
  const bool on = x < W && src[(size_t)y * W + x] != 0;
  const u64 bits = __ballot(on);
  if (lane == 0) dst[m * HWW + word] = bits;
}

__global__ __launch_bounds__(256) void mask_unpack_kernel(const u64* __restrict__ src, uint8_t* __restrict__ out, int H, int W, int WW) {
  ES_MASK_PIXEL_PROLOGUE;
  const u64 bits = src[m * HWW + word];
  if (x < W) out[m * HW + (size_t)y * W + x] = (uint8_t)((bits >> lane) & 1);
}

// ---- word kernels: grid (ceil(H * WW / 256), masks), one thread per packed word
__global__ __launch_bounds__(256) void mask_morph_kernel(const u64* __restrict__ src, u64* __restrict__ dst, int H, int W, int WW, const Radii rd) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= H * WW) return;
  const int m = blockIdx.y, y = idx / WW, wx = idx - y * WW;
  const int rs = rd.r[m % rd.nslot];
  const bool er = rs < 0;
  const int r = er ? -rs : rs;
  const u64* base = src + (size_t)m * H * WW;
  const u64 outside = er ? ~0ull : 0ull;                                 // what a clipped window reads beyond the image
  const u64 tail = (W & 63) ? ~0ull << (W & 63) : 0ull;                  // the bits past W in a row's last word
  const int y0 = y - r < 0 ? 0 : y - r, y1 = y + r > H - 1 ? H - 1 : y + r;
  u64 l = outside, c = outside, rr = outside;
  for (int yy = y0; yy <= y1; ++yy) {
    const u64* row = base + (size_t)yy * WW;
    u64 cl = wx > 0 ? row[wx - 1] : outside, cc = row[wx], cr = wx + 1 < WW ? row[wx + 1] : outside;
    if (er) {
      if (wx == WW - 1) cc |= tail;
      if (wx + 1 == WW - 1) cr |= tail;
      l &= cl; c &= cc; rr &= cr;
    } else {
      l |= cl; c |= cc; rr |= cr;
    }
  }
  u64 res = c;
  for (int s = 1; s <= r; ++s) {                                          // pixel x - s, then pixel x + s
    const u64 lo = (c << s) | (l >> (64 - s)), hi = (c >> s) | (rr << (64 - s));
    res = er ? (res & lo & hi) : (res | lo | hi);
  }
  if (wx == WW - 1) res &= ~tail;
  dst[(size_t)m * H * WW + idx] = res;
}

// create_sam_images' union: image m of dst = subject | clothes | head of the four packed masks of image m (slots 0, 2, 3)
__global__ __launch_bounds__(256) void mask_or3_kernel(const u64* __restrict__ src, u64* __restrict__ dst, int HWW) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= HWW) return;
  const u64* p = src + (size_t)blockIdx.y * 4 * HWW + idx;
  dst[(size_t)blockIdx.y * HWW + idx] = p[0] | p[2 * (size_t)HWW] | p[3 * (size_t)HWW];
}

// ---- union-find
__device__ inline int link_of(const int* L, int i) { return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline int find_root(const int* L, int x) {
  for (int p; (p = link_of(L, x)) != x;) x = p;                           // p < x: strictly down, ends at a pixel that links to itself
  return x;
}
__device__ inline void unite(int* L, int a, int b) {
  for (;;) {
    a = find_root(L, a);
    b = find_root(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(L + a, b);                                  // b < a: the link still points down
    if (old == a) return;                                                 // a was a root when the atomic ran: it hangs under b now
    a = old;                                                              // it was none any more: its former link and b are still to unite
  }
}
__device__ inline bool bit_at(const u64* mask, int H, int W, int WW, int y, int x) {
  if (x < 0 || x >= W || y < 0 || y >= H) return false;
  return (mask[(size_t)y * WW + (x >> 6)] >> (x & 63)) & 1;
}

__global__ __launch_bounds__(256) void mask_cc_init_kernel(const u64* __restrict__ src, int* __restrict__ label, int* __restrict__ area,
                                                           u64* __restrict__ best, int H, int W, int WW) {
  ES_MASK_PIXEL_PROLOGUE;
  if (word == 0 && lane == 0) best[m] = 0;
  if (x >= W) return;
  const u64 bits = src[m * HWW + word];
  const int i = y * W + x;
  int v = -1;
  if ((bits >> lane) & 1) {                                               // the start of this pixel's run inside the word
    const u64 zeros_below = ~bits & ((1ull << lane) - 1);
    const int start = zeros_below ? 64 - __clzll(zeros_below) : 0;
    v = i - (lane - start);
  }
  label[m * HW + i] = v;
  area[m * HW + i] = 0;
}

// P(i): pixel i is in one set with each of its true W, NW, N, NE neighbours.  By induction over raster order:
//   W   same word: both link to the same run start (init); across a word edge: united here.
//   N   united here, unless W and NW are true: then i ~ W, W ~ NW by P(W) (NW is W's N) and NW ~ N by P(N) (NW is N's W).
//   NW  N true: i ~ N and N ~ NW by P(N).  N false, W true: W ~ NW by P(W).  Otherwise united here.
//   NE  N true: i ~ N and N ~ NE by P(NE) (N is NE's W).  Otherwise united here.
__global__ __launch_bounds__(256) void mask_cc_merge_kernel(const u64* __restrict__ src, int* __restrict__ label, int H, int W, int WW) {
  ES_MASK_PIXEL_PROLOGUE;
  if (x >= W) return;
  const u64* mask = src + m * HWW;
  if (!((mask[word] >> lane) & 1)) return;
  int* L = label + m * HW;
  const int i = y * W + x;
  const bool w = bit_at(mask, H, W, WW, y, x - 1), nw = bit_at(mask, H, W, WW, y - 1, x - 1);
  const bool n = bit_at(mask, H, W, WW, y - 1, x), ne = bit_at(mask, H, W, WW, y - 1, x + 1);
  if (lane == 0 && w) unite(L, i, i - 1);
  if (n) {
    if (!(w && nw)) unite(L, i, i - W);
  } else {
    if (nw && !w) unite(L, i, i - W - 1);
    if (ne) unite(L, i, i - W + 1);
  }
}

// every true pixel: link -> root (final: all unions are done), area[root] += 1, one atomicAdd per distinct root per wave
__global__ __launch_bounds__(256) void mask_cc_count_kernel(const u64* __restrict__ src, int* __restrict__ label, int* __restrict__ area, int H, int W, int WW) {
  ES_MASK_PIXEL_PROLOGUE;
  int* L = label + m * HW;
  int root = -1;
  if (x < W && ((src[m * HWW + word] >> lane) & 1)) {
    const int i = y * W + x;
    root = find_root(L, i);
    __hip_atomic_store(L + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  u64 todo = __ballot(root >= 0);                                        // wave-uniform, so is the loop
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int lead_root = __shfl(root, leader);
    const u64 same = __ballot(root == lead_root);
    if (lane == leader) atomicAdd(area + m * HW + lead_root, __popcll(same));
    todo &= ~same;
  }
}

// best[m] = max over roots of (area << 32 | 0x7fffffff - root): the largest area, and of equal areas the smaller root
__global__ __launch_bounds__(256) void mask_cc_argmax_kernel(const u64* __restrict__ src, const int* __restrict__ label, const int* __restrict__ area,
                                                             u64* __restrict__ best, int H, int W, int WW) {
  ES_MASK_PIXEL_PROLOGUE;
  u64 key = 0;
  if (x < W && ((src[m * HWW + word] >> lane) & 1)) {
    const int i = y * W + x;
    if (label[m * HW + i] == i) key = ((u64)(unsigned)area[m * HW + i] << 32) | (u64)(0x7fffffff - i);
  }
  for (int d = 32; d >= 1; d >>= 1) {
    const u64 o = __shfl_xor(key, d);
    key = o > key ? o : key;
  }
  if (lane == 0 && key) atomicMax(best + m, key);
}

__global__ __launch_bounds__(256) void mask_cc_select_kernel(const u64* __restrict__ src, const int* __restrict__ label, const u64* __restrict__ best,
                                                             u64* __restrict__ dst, int32_t* __restrict__ area_out, int H, int W, int WW) {
  ES_MASK_PIXEL_PROLOGUE;
  const u64 b = best[m];
  bool on = false;
  if (x < W) {
    if (b == 0) on = true;                                                // no true pixel: the reference's labeled_array == 0 is true everywhere
    else on = ((src[m * HWW + word] >> lane) & 1) && label[m * HW + (size_t)y * W + x] == 0x7fffffff - (int)(unsigned)(b & 0xffffffffull);
  }
  const u64 bits = __ballot(on);
  if (lane == 0) dst[m * HWW + word] = bits;
  if (area_out && word == 0 && lane == 0) area_out[m] = (int32_t)(b >> 32);
}

// ---- images
__device__ inline void put3(uint8_t* o, bool keep, unsigned r, unsigned g, unsigned b, unsigned grey) {
  o[0] = (uint8_t)(keep ? r : grey); o[1] = (uint8_t)(keep ? g : grey); o[2] = (uint8_t)(keep ? b : grey);
}

// P: the four smoothed masks of every image (subject, body, clothes, head), Q: ALL.  grid.y = image of this batch.
__global__ __launch_bounds__(256) void mask_compose_kernel(const ImgBatch ib, int first, const u64* __restrict__ P, const u64* __restrict__ Q,
                                                           uint8_t* __restrict__ masks_out, uint8_t* __restrict__ images_out, int H, int W, int WW) {
  ES_MASK_PIXEL_PROLOGUE;
  const size_t img = (size_t)first + m;
  const u64* p = P + img * 4 * HWW + word;
  const u64 a = p[HWW], c = p[2 * HWW], hd = p[3 * HWW], all = Q[img * HWW + word];
  const u64 unknown = a & c;
  const bool k_all = (all >> lane) & 1, k_agn = ((a & ~unknown & all) >> lane) & 1, k_clo = ((c & ~unknown & all) >> lane) & 1,
             k_head = ((hd & all) >> lane) & 1;
  if (x >= W) return;
  const size_t pix = (size_t)y * W + x;
  if (masks_out) {
    uint8_t* mo = masks_out + img * 4 * HW + pix;
    mo[0] = k_all; mo[HW] = k_agn; mo[2 * HW] = k_clo; mo[3 * HW] = k_head;
  }
  if (images_out) {
    const uint8_t* px = ib.data[m] + (size_t)y * (size_t)ib.stride[m] + (size_t)x * ib.ch[m];
    const unsigned r = px[0], g = px[1], b = px[2];
    uint8_t* io = images_out + (img * 5 * HW + pix) * 3;
    put3(io, k_all, r, g, b, 127);
    put3(io + 3 * HW, k_agn, 0, 0, 0, 255);
    put3(io + 6 * HW, k_agn, r, g, b, 127);
    put3(io + 9 * HW, k_clo, r, g, b, 127);
    put3(io + 12 * HW, k_head, r, g, b, 127);
  }
}

// draw_binary_mask: grid (ceil(H * W / 256), images of this batch), one thread per pixel
__global__ __launch_bounds__(256) void mask_fill_kernel(const ImgBatch ib, int has_img, int first, const uint8_t* __restrict__ mask, uint8_t* __restrict__ out,
                                                        int H, int W, unsigned c0, unsigned c1, unsigned c2) {
  const size_t HW = (size_t)H * W, pix = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (pix >= HW) return;
  const int m = blockIdx.y;
  const size_t img = (size_t)first + m;
  const bool keep = mask[img * HW + pix] != 0;
  unsigned r = 0, g = 0, b = 0;
  if (has_img) {
    const int y = (int)(pix / W), x = (int)(pix - (size_t)y * W);
    const uint8_t* px = ib.data[m] + (size_t)y * (size_t)ib.stride[m] + (size_t)x * ib.ch[m];
    r = px[0]; g = px[1]; b = px[2];
  }
  uint8_t* o = out + (img * HW + pix) * 3;
  o[0] = (uint8_t)(keep ? r : c0); o[1] = (uint8_t)(keep ? g : c1); o[2] = (uint8_t)(keep ? b : c2);
}

__global__ __launch_bounds__(256) void mask_logic_kernel(const uint8_t* a, const uint8_t* b, uint8_t* out, long long n, int op) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const bool p = a[i] != 0, q = b[i] != 0;
    out[i] = (uint8_t)(op == ES_MASK_AND ? (p && q) : op == ES_MASK_OR ? (p || q) : (p && !q));
  }
}

// ---- host
thread_local char g_msg[224];
int fail(const char* who, const char* what) {
  snprintf(g_msg, sizeof(g_msg), "%s: %s", who, what);
  es_set_error(g_msg);
  return -1;
}

int check_geometry(const char* who, int count, int H, int W) {
  if (count < 1 || count > kMaxCount) return fail(who, "count must be in 1..4096");
  if (H < 1 || W < 1 || H > kMaxSide || W > kMaxSide) return fail(who, "H and W must be in 1..4096");
  return 0;
}

// the workspace of a call over `count` images: best u64 [count] | packed P0, P1 (nslot masks per image each) | packed Q0, Q1 (one mask
// per image each; `q`) | label, area int32 [count, H, W] (`cc`)
struct Layout { size_t best, p0, p1, q0, q1, label, area, total; };
Layout layout(int H, int W, int count, int nslot, bool q, bool cc) {
  const size_t hww = (size_t)H * ((W + 63) / 64) * sizeof(u64), n = (size_t)count;
  Layout l;
  size_t at = 0;
  l.best = at; at += cc ? n * sizeof(u64) : 0;
  l.p0 = at; at += n * nslot * hww;
  l.p1 = at; at += n * nslot * hww;
  l.q0 = at; at += q ? n * hww : 0;
  l.q1 = at; at += q ? n * hww : 0;
  l.label = at; at += cc ? n * H * W * sizeof(int32_t) : 0;
  l.area = at; at += cc ? n * H * W * sizeof(int32_t) : 0;
  l.total = at;
  return l;
}

int check_workspace(const char* who, const void* ws, size_t given, size_t need) {
  if (!ws) return fail(who, "null pointer (workspace)");
  if ((uintptr_t)ws % 8) return fail(who, "the workspace must be 8-byte aligned");
  if (given < need) {
    snprintf(g_msg, sizeof(g_msg), "%s: workspace too small: %zu bytes given, %zu needed (es_mask_workspace_bytes covers every call)", who, given, need);
    es_set_error(g_msg);
    return -1;
  }
  return 0;
}

int check_photos(const char* who, const es_image_u8* imgs, int count, int H, int W) {
  for (int i = 0; i < count; ++i) {
    const es_image_u8& im = imgs[i];
    const char* what = nullptr;
    if (!im.data) what = "null pointer (data)";
    else if (im.height != H || im.width != W) what = "height and width must equal H and W";
    else if (im.channels != 3 && im.channels != 4) what = "channels must be 3 or 4";
    else if (im.row_stride < (int64_t)im.width * im.channels) what = "row_stride < width*channels";
    if (what) {
      snprintf(g_msg, sizeof(g_msg), "%s: image %d: %s", who, i, what);
      es_set_error(g_msg);
      return -1;
    }
  }
  return 0;
}

ImgBatch batch_of(const es_image_u8* imgs, int first, int n) {
  ImgBatch b = {};
  for (int i = 0; imgs && i < n; ++i) {
    b.data[i] = imgs[first + i].data; b.stride[i] = imgs[first + i].row_stride; b.ch[i] = imgs[first + i].channels;
  }
  return b;
}

int check_radii(const char* who, const int32_t* radii, int n) {
  if (n < 0 || n > kMaxChain) return fail(who, "n must be in 0..16");
  if (n && !radii) return fail(who, "null pointer (radii)");
  for (int i = 0; i < n; ++i)
    if (radii[i] > kMaxRadius || radii[i] < -kMaxRadius) return fail(who, "a radius is beyond 15");
  return 0;
}

struct Geo {
  int H, W, WW;
  dim3 pixel_grid(int masks) const { return dim3((unsigned)((H * WW + 3) / 4), (unsigned)masks); }
  dim3 word_grid(int masks) const { return dim3((unsigned)((H * WW + 255) / 256), (unsigned)masks); }
};

// one step per nonzero radius over `masks` packed masks, from *cur to *other and swapped after each: *cur holds the result
void run_chain(hipStream_t st, const Geo& g, int masks, int nslot, const int32_t (*radii)[4], int n, u64** cur, u64** other) {
  for (int i = 0; i < n; ++i) {
    Radii rd = {};
    rd.nslot = nslot;
    bool any = false;
    for (int s = 0; s < nslot; ++s) { rd.r[s] = radii[i][s]; any |= radii[i][s] != 0; }
    if (!any) continue;
    hipLaunchKernelGGL(mask_morph_kernel, g.word_grid(masks), dim3(256), 0, st, *cur, *other, g.H, g.W, g.WW, rd);
    u64* t = *cur; *cur = *other; *other = t;
  }
}

// the largest component of `masks` packed masks: src -> dst (another buffer)
void run_largest(hipStream_t st, const Geo& g, int masks, const u64* src, u64* dst, int* label, int* area, u64* best, int32_t* area_out) {
  const dim3 grid = g.pixel_grid(masks), block(256);
  hipLaunchKernelGGL(mask_cc_init_kernel, grid, block, 0, st, src, label, area, best, g.H, g.W, g.WW);
  hipLaunchKernelGGL(mask_cc_merge_kernel, grid, block, 0, st, src, label, g.H, g.W, g.WW);
  hipLaunchKernelGGL(mask_cc_count_kernel, grid, block, 0, st, src, label, area, g.H, g.W, g.WW);
  hipLaunchKernelGGL(mask_cc_argmax_kernel, grid, block, 0, st, src, (const int*)label, (const int*)area, best, g.H, g.W, g.WW);
  hipLaunchKernelGGL(mask_cc_select_kernel, grid, block, 0, st, src, (const int*)label, (const u64*)best, dst, area_out, g.H, g.W, g.WW);
}

int launched(const char* who) {
  if (hipGetLastError() != hipSuccess) { fail(who, "launch failed"); return -2; }
  return 0;
}

const char* kNoPlan = "a plan is recording on this thread; the mask calls are never part of a plan";
constexpr int32_t kSmooth[4] = {3, -3, -3, 3};       // smooth_mask(kernel_size 3, iterations 3)

}  // namespace

extern "C" size_t es_mask_workspace_bytes(int H, int W, int count) {
  if (check_geometry("es_mask_workspace_bytes", count, H, W)) return 0;
  return layout(H, W, count, 4, true, true).total;
}

extern "C" int es_mask_morph(const uint8_t* in, uint8_t* out, int count, int H, int W, const int32_t* radii, int n, void* ws, size_t ws_bytes,
                             void* stream) {
  const char* who = "es_mask_morph";
  if (!in || !out) return fail(who, "null pointer");
  if (check_geometry(who, count, H, W) || check_radii(who, radii, n)) return -1;
  const Layout l = layout(H, W, count, 1, false, false);
  if (check_workspace(who, ws, ws_bytes, l.total)) return -1;
  if (es_plan_recording()) return fail(who, kNoPlan);
  hipStream_t st = (hipStream_t)stream;
  const Geo g = {H, W, (W + 63) / 64};
  u64 *cur = (u64*)((char*)ws + l.p0), *other = (u64*)((char*)ws + l.p1);
  Src s = {};
  s.p[0] = in; s.nslot = 1;
  hipLaunchKernelGGL(mask_pack_kernel, g.pixel_grid(count), dim3(256), 0, st, s, cur, H, W, g.WW);
  int32_t chain[kMaxChain][4] = {};
  for (int i = 0; i < n; ++i) chain[i][0] = radii[i];
  run_chain(st, g, count, 1, chain, n, &cur, &other);
  hipLaunchKernelGGL(mask_unpack_kernel, g.pixel_grid(count), dim3(256), 0, st, (const u64*)cur, out, H, W, g.WW);
  return launched(who);
}

extern "C" int es_mask_largest_component(const uint8_t* in, uint8_t* out, int32_t* area_out, int count, int H, int W, void* ws, size_t ws_bytes,
                                         void* stream) {
  const char* who = "es_mask_largest_component";
  if (!in || !out) return fail(who, "null pointer");
  if (check_geometry(who, count, H, W)) return -1;
  const Layout l = layout(H, W, count, 1, false, true);
  if (check_workspace(who, ws, ws_bytes, l.total)) return -1;
  if (es_plan_recording()) return fail(who, kNoPlan);
  hipStream_t st = (hipStream_t)stream;
  const Geo g = {H, W, (W + 63) / 64};
  char* base = (char*)ws;
  u64 *p0 = (u64*)(base + l.p0), *p1 = (u64*)(base + l.p1);
  Src s = {};
  s.p[0] = in; s.nslot = 1;
  hipLaunchKernelGGL(mask_pack_kernel, g.pixel_grid(count), dim3(256), 0, st, s, p0, H, W, g.WW);
  run_largest(st, g, count, p0, p1, (int*)(base + l.label), (int*)(base + l.area), (u64*)(base + l.best), area_out);
  hipLaunchKernelGGL(mask_unpack_kernel, g.pixel_grid(count), dim3(256), 0, st, (const u64*)p1, out, H, W, g.WW);
  return launched(who);
}

extern "C" int es_mask_logic(const uint8_t* a, const uint8_t* b, uint8_t* out, int64_t n, int op, void* stream) {
  const char* who = "es_mask_logic";
  if (!a || !b || !out) return fail(who, "null pointer");
  if (n < 1) return fail(who, "n < 1");
  if (op != ES_MASK_AND && op != ES_MASK_OR && op != ES_MASK_ANDNOT) return fail(who, "op must be ES_MASK_AND, ES_MASK_OR or ES_MASK_ANDNOT");
  if (es_plan_recording()) return fail(who, kNoPlan);
  const long long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(mask_logic_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, a, b, out, (long long)n, op);
  return launched(who);
}

extern "C" int es_image_mask_fill_u8(const es_image_u8* img_or_null, const uint8_t* mask, uint8_t* out_hwc3, int count, int H, int W,
                                     const uint8_t colour[3], void* stream) {
  const char* who = "es_image_mask_fill_u8";
  if (!mask || !out_hwc3 || !colour) return fail(who, "null pointer");
  if (check_geometry(who, count, H, W)) return -1;
  if (img_or_null && check_photos(who, img_or_null, count, H, W)) return -1;
  if (es_plan_recording()) return fail(who, kNoPlan);
  const unsigned blocks = (unsigned)(((size_t)H * W + 255) / 256);
  for (int first = 0; first < count; first += kImgPerLaunch) {
    const int n = count - first < kImgPerLaunch ? count - first : kImgPerLaunch;
    hipLaunchKernelGGL(mask_fill_kernel, dim3(blocks, (unsigned)n), dim3(256), 0, (hipStream_t)stream, batch_of(img_or_null, first, n),
                       img_or_null ? 1 : 0, first, mask, out_hwc3, H, W, (unsigned)colour[0], (unsigned)colour[1], (unsigned)colour[2]);
  }
  return launched(who);
}

extern "C" int es_sam_compose(const es_image_u8* imgs, const uint8_t* subject, const uint8_t* body, const uint8_t* clothes, const uint8_t* head,
                              int count, int H, int W, uint8_t* masks_out, uint8_t* images_out, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "es_sam_compose";
  if (!subject || !body || !clothes || !head) return fail(who, "null pointer (a mask)");
  if (!masks_out && !images_out) return fail(who, "null pointer (both outputs)");
  if (images_out && !imgs) return fail(who, "null pointer (imgs)");
  if (check_geometry(who, count, H, W)) return -1;
  if (images_out && check_photos(who, imgs, count, H, W)) return -1;
  const Layout l = layout(H, W, count, 4, true, true);
  if (check_workspace(who, ws, ws_bytes, l.total)) return -1;
  if (es_plan_recording()) return fail(who, kNoPlan);
  hipStream_t st = (hipStream_t)stream;
  const Geo g = {H, W, (W + 63) / 64};
  char* base = (char*)ws;
  u64 *p = (u64*)(base + l.p0), *p_other = (u64*)(base + l.p1), *q = (u64*)(base + l.q0), *q_other = (u64*)(base + l.q1);
  Src s = {};
  s.p[0] = subject; s.p[1] = body; s.p[2] = clothes; s.p[3] = head; s.nslot = 4;
  hipLaunchKernelGGL(mask_pack_kernel, g.pixel_grid(4 * count), dim3(256), 0, st, s, p, H, W, g.WW);
  // closing(square(3)) for subject, body and clothes, closing(square(7)) for the head, then smooth_mask for all four
  int32_t chain[6][4] = {{1, 1, 1, 3}, {-1, -1, -1, -3}};
  for (int i = 0; i < 4; ++i)
    for (int k = 0; k < 4; ++k) chain[2 + i][k] = kSmooth[i];
  run_chain(st, g, 4 * count, 4, chain, 6, &p, &p_other);
  hipLaunchKernelGGL(mask_or3_kernel, g.word_grid(count), dim3(256), 0, st, (const u64*)p, q, H * g.WW);
  run_largest(st, g, count, q, q_other, (int*)(base + l.label), (int*)(base + l.area), (u64*)(base + l.best), nullptr);
  { u64* t = q; q = q_other; q_other = t; }
  int32_t smooth[4][4] = {};
  for (int i = 0; i < 4; ++i) smooth[i][0] = kSmooth[i];
  run_chain(st, g, count, 1, smooth, 4, &q, &q_other);
  for (int first = 0; first < count; first += kImgPerLaunch) {
    const int n = count - first < kImgPerLaunch ? count - first : kImgPerLaunch;
    hipLaunchKernelGGL(mask_compose_kernel, g.pixel_grid(n), dim3(256), 0, st, batch_of(images_out ? imgs : nullptr, first, n), first,
                       (const u64*)p, (const u64*)q, masks_out, images_out, H, W, g.WW);
  }
  return launched(who);
}
