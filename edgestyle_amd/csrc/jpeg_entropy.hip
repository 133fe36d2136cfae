// Huffman decoding on the device (gfx950): the bytes of a baseline JPEG file -> the int16 coefficient buffer the serial host decoder
// (csrc/jpeg.h, entropy_decode) writes, bit for bit.  Opt-in; include/edgestyle_hip.h states the interface, csrc/jpeg.h the algorithm and
// the per-symbol code (bit reader over raw bytes, symbol decode, state step), which this kernel and the host twin both compile.
//
// Two launches per 16 images, grid.y = image (images of different sizes, samplings and segment counts share a launch; the workgroups
// past a smaller image's last segment leave at once), after one memset node per image that zeroes its coefficients:
//  1. jpeg_entropy_kernel: ONE workgroup of 1024 decoders owns ONE segment (the bytes between restart markers) from start to finish:
//     the image's six Huffman tables are copied into LDS (8.4 KB, random 2-byte lookups from there on); the segment's raw bytes are cut
//     into J <= 1024 subsequences; decoder j decodes subsequence j from its entry state and proposes its exit state to decoder j + 1
//     through LDS, round after round, until a workgroup vote (__syncthreads_or) finds no entry changed - a decoder whose entry did
//     not change skips the round, and the loop runs J + 1 times at most, a number that comes from the sizes alone.  Then the block
//     counts and the DC sums of the subsequences are scanned across the workgroup (Hillis-Steele in LDS, 10 steps), and every decoder
//     decodes once more from its true entry and stores: a block's address comes from its ordinal in the segment, which is checked
//     against the segment's share of the geometry.  Defects are folded by an LDS atomicMin of (block ordinal << 3 | status); the
//     segment's word goes to the workspace.  Workgroups never communicate: no flags, no spinning.
//  2. jpeg_status_kernel: one workgroup per image picks the status of the first segment that has one.
// The decoders of a wave diverge by nature (each walks its own symbols); the work per decoder is S raw bytes, S = max(subseq_bytes,
// ceil(len / 1024)).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include "jpeg.h"
#include "plan.h"

extern "C" void es_set_error(const char* msg);
extern "C" int es_jpeg_reconstruct(const es_jpeg_info* infos, int count, const int16_t* const* coeffs_dev, const uint16_t* const* qtables_dev,
                                   const es_image_u8* out, void* workspace, size_t workspace_bytes, void* stream);

namespace {

using namespace esjpeg;

constexpr int kImgPerLaunch = 16;
constexpr int kMaxDecode = 64;
constexpr int kT = 1024;                          // decoders per workgroup
constexpr size_t kQtableBytes = 3 * 64 * sizeof(uint16_t);

__constant__ uint8_t d_natural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct EntDesc {
  const uint8_t* bytes;
  const es_jpeg_segment* seg;
  const uint32_t* tables;                         // a ScanTables, read as words
  int16_t* coef;
  uint32_t* seg_status;                           // [nseg], in the workspace
  int32_t* status;
  uint32_t n;                                     // readable bytes (below 2^28)
  uint32_t nseg;
  ScanGeom G;
};
struct EntBatch {
  EntDesc d[kImgPerLaunch];
  uint32_t subseq;
};

__global__ __launch_bounds__(kT) void jpeg_entropy_kernel(const EntBatch B) {
  __shared__ ScanTables tab;
  __shared__ ScanState prop[kT + 1];
  __shared__ uint4 scan[kT];
  __shared__ uint8_t natural[64];
  __shared__ ScanGeom G;                          // (in LDS: the sinks hold a pointer to it, which must not force the argument into scratch)
  __shared__ uint32_t first, first_dead;
  const EntDesc& d = B.d[blockIdx.y];
  if (blockIdx.x >= d.nseg) return;               // (the whole workgroup: no barrier is left behind)
  const uint32_t j = threadIdx.x;
  if (j == 0) { G = d.G; first_dead = kT; }
  for (uint32_t w = j; w < sizeof(ScanTables) / 4; w += kT) reinterpret_cast<uint32_t*>(&tab)[w] = d.tables[w];
  if (j < 64) natural[j] = d_natural[j];
  if (j == 0) first = ~0u;
  // the segment, cut to the bytes that can be read
  const es_jpeg_segment sg = d.seg[blockIdx.x];
  const uint32_t end = sg.end < d.n ? sg.end : d.n, begin = sg.begin < end ? sg.begin : end;
  const uint8_t* p = d.bytes + begin;
  const uint32_t len = end - begin;
  const uint32_t S = subsequence_bytes(len, B.subseq, kT), J = len ? (len + S - 1) / S : 0;      // J <= kT
  const uint32_t expected = segment_blocks(d.G, blockIdx.x);       // (by value: G is not written yet)
  const bool live = j < J;
  const uint32_t bound = (j + 1) * S;             // (J * S < len + S: no overflow below 2^28 + 2^28)
  const ScanState guess = live ? guessed_entry(p, len, j * S) : dead_state();
  ScanState in = guess;
  prop[j] = in;
  if (j == 0) prop[kT] = dead_state();
  CountSink cnt;
  cnt.clear();
  bool dirty = live;
  __syncthreads();
  // ---- synchronise: at most J + 1 rounds ----
  for (uint32_t r = 0; r <= J; ++r) {
    if (dirty) {                                  // a dead entry (the neighbour met an impossible code): propose from the own guess again
      const bool dead = in.pos == kDeadPos;
      cnt.clear();
      prop[j + 1] = decode_subsequence(tab, G, p, len, dead ? guess : in, bound, cnt);
      if (dead) cnt.clear();                      // (what follows a dead entry is dropped by the write pass)
    }
    __syncthreads();
    dirty = false;
    if (live && j > 0) {
      const ScanState e = prop[j];
      dirty = !same_state(e, in);
      in = e;
    }
    if (!__syncthreads_or(dirty)) break;          // (also the barrier between this round's reads and the next round's writes)
  }
  // Behind the first dead entry nothing is a true state (the decoder after it proposed from a guess): all of it is dead from here on
  if (live && in.pos == kDeadPos) atomicMin(&first_dead, j);
  __syncthreads();
  if (j >= first_dead) { in = dead_state(); cnt.clear(); }
  // ---- count: exclusive scan of (blocks started, DC sums per component) ----
  scan[j] = live ? make_uint4(cnt.dcs, cnt.sum[0], cnt.sum[1], cnt.sum[2]) : make_uint4(0, 0, 0, 0);
  __syncthreads();
  for (uint32_t step = 1; step < (uint32_t)kT; step <<= 1) {
    uint4 v = scan[j];
    if (j >= step) {
      const uint4 u = scan[j - step];
      v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
    }
    __syncthreads();
    scan[j] = v;
    __syncthreads();
  }
  const uint4 before = j > 0 ? scan[j - 1] : make_uint4(0, 0, 0, 0);
  // ---- write ----
  if (live) {
    WriteSink w{&G, natural, d.coef, blockIdx.x, expected, before.x, ~0u, {before.y, before.z, before.w}, ~0u, nullptr};
    if ((in.bk & 255u) != 0u && in.pos != kDeadPos && before.x > 0) w.enter(before.x - 1);
    const ScanState exit = decode_subsequence(tab, G, p, len, in, bound, w);
    if (j + 1 == J) close_segment(w, exit);
    if (w.err != ~0u) atomicMin(&first, w.err);
  }
  if (J == 0 && j == 0) first = kStTruncated;     // an empty segment: block 0 is missing
  __syncthreads();
  if (j == 0) d.seg_status[blockIdx.x] = first == ~0u ? 0u : (first & 7u);
}

__global__ __launch_bounds__(256) void jpeg_status_kernel(const EntBatch B) {
  __shared__ uint32_t first;
  const EntDesc& d = B.d[blockIdx.y];
  if (threadIdx.x == 0) first = ~0u;
  __syncthreads();
  uint32_t mine = ~0u;
  for (uint32_t s = threadIdx.x; s < d.nseg; s += 256)
    if (d.seg_status[s] != 0u) { mine = s; break; }      // (the lowest index this thread sees)
  if (mine != ~0u) atomicMin(&first, mine);
  __syncthreads();
  if (threadIdx.x == 0) *d.status = first == ~0u ? 0 : (int32_t)d.seg_status[first];
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
const char* check_subseq(int subseq_bytes) {
  if (subseq_bytes != 0 && (subseq_bytes < (int)kMinSubseq || subseq_bytes > (1 << 24))) return "subseq_bytes must be 0 (the default) or 4 .. 2^24";
  return nullptr;
}
inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }
inline size_t segment_status_bytes(const es_jpeg_info& I) { return align16(restart_intervals(I) * sizeof(uint32_t)); }
size_t entropy_workspace_bytes(const es_jpeg_info* infos, int count) {
  size_t total = 16;                              // room to start on a 16-byte boundary
  for (int i = 0; i < count; ++i) total += segment_status_bytes(infos[i]);
  return total;
}
// the parts of one image in es_jpeg_decode_dev_u8's staging: uploaded (file, segments, tables, quantisation tables), then device-only
struct DevLayout { size_t file, seg, tab, qt, upload; };
inline DevLayout dev_layout(const es_jpeg_info& I, size_t n) {
  DevLayout L;
  L.file = 0;
  L.seg = align16(n);
  L.tab = L.seg + align16(restart_intervals(I) * sizeof(es_jpeg_segment));
  L.qt = L.tab + ES_JPEG_TABLES_BYTES;
  L.upload = L.qt + kQtableBytes;
  return L;
}

}  // namespace

extern "C" size_t es_jpeg_segment_count(const es_jpeg_info* info) {
  const char* why = nullptr;
  if (es_plan_recording()) { fail("es_jpeg_segment_count", "a plan is recording on this thread; the JPEG calls are never part of a plan"); return 0; }
  if (!info_ok(info, &why)) { fail("es_jpeg_segment_count", why); return 0; }
  return (size_t)restart_intervals(*info);
}

extern "C" const char* es_jpeg_status_text(int code) { return status_text(code); }

extern "C" int es_jpeg_scan_prepare_host(const uint8_t* bytes, size_t n, const es_jpeg_info* info, es_jpeg_segment* segments, void* tables,
                                         uint16_t* qtables) {
  const char* who = "es_jpeg_scan_prepare_host";
  if (!bytes || !info || !segments || !tables || !qtables) return fail(who, "null pointer");
  if (es_plan_recording()) return fail(who, "a plan is recording on this thread; the JPEG calls are never part of a plan");
  Header H;
  const char* why = nullptr;
  if (!parse_header(bytes, n, H, &why)) return fail(who, why);
  if (memcmp(&H.info, info, sizeof(H.info)) != 0) return fail(who, "the info is not what es_jpeg_info_host gives for these bytes");
  ScanTables T;
  if (!scan_prepare(bytes, n, H, segments, &T, &why)) return fail(who, why);
  memcpy(tables, &T, sizeof(T));
  component_qtables(H, qtables);
  return 0;
}

extern "C" size_t es_jpeg_entropy_decode_workspace_bytes(const es_jpeg_info* infos, int count) {
  if (const char* why = check_infos(infos, count)) { fail("es_jpeg_entropy_decode_workspace_bytes", why); return 0; }
  if (es_plan_recording()) { fail("es_jpeg_entropy_decode_workspace_bytes", "a plan is recording on this thread; the JPEG calls are never part of a plan"); return 0; }
  return entropy_workspace_bytes(infos, count);
}

extern "C" int es_jpeg_entropy_decode(const es_jpeg_info* infos, int count, const uint8_t* const* bytes_dev, const size_t* bytes_n,
                                      const es_jpeg_segment* const* segments_dev, const void* const* tables_dev, int subseq_bytes,
                                      int16_t* const* coeffs_dev, int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "es_jpeg_entropy_decode";
  if (!bytes_dev || !bytes_n || !segments_dev || !tables_dev || !coeffs_dev || !status_dev || !workspace) return fail(who, "null pointer");
  if (const char* why = check_infos(infos, count)) return fail(who, why);
  if (const char* why = check_subseq(subseq_bytes)) return fail(who, why);
  if (es_plan_recording()) return fail(who, "a plan is recording on this thread; the JPEG calls are never part of a plan");
  if ((uintptr_t)status_dev % 4) return fail(who, "the status words must be 4-byte aligned");
  for (int i = 0; i < count; ++i) {
    if (!bytes_dev[i] || !segments_dev[i] || !tables_dev[i] || !coeffs_dev[i]) return fail(who, "null pointer");
    if (bytes_n[i] >= kMaxParallelFile) return fail(who, "a file of 256 MiB or more is not decoded in parallel");
    if ((uintptr_t)segments_dev[i] % 4 || (uintptr_t)tables_dev[i] % 4) return fail(who, "segments and tables must be 4-byte aligned");
    if ((uintptr_t)coeffs_dev[i] % 16) return fail(who, "coefficients must be 16-byte aligned");
  }
  if (workspace_bytes < entropy_workspace_bytes(infos, count)) return fail(who, "workspace too small (es_jpeg_entropy_decode_workspace_bytes)");
  uint8_t* ws = (uint8_t*)(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  for (int i = 0; i < count; ++i)
    if (hipMemsetAsync(coeffs_dev[i], 0, coeff_count(infos[i]) * sizeof(int16_t), (hipStream_t)stream) != hipSuccess) { fail(who, "memset failed"); return -2; }
  for (int first = 0; first < count; first += kImgPerLaunch) {
    const int n = count - first < kImgPerLaunch ? count - first : kImgPerLaunch;
    EntBatch b;
    memset(&b, 0, sizeof(b));
    b.subseq = subseq_bytes ? (uint32_t)subseq_bytes : kDefaultSubseq;
    uint32_t max_seg = 0;
    for (int i = 0; i < n; ++i) {
      const es_jpeg_info& I = infos[first + i];
      EntDesc& d = b.d[i];
      d.bytes = bytes_dev[first + i];
      d.seg = segments_dev[first + i];
      d.tables = (const uint32_t*)tables_dev[first + i];
      d.coef = coeffs_dev[first + i];
      d.seg_status = (uint32_t*)ws;
      d.status = status_dev + first + i;
      d.n = (uint32_t)bytes_n[first + i];
      d.nseg = (uint32_t)restart_intervals(I);    // at most 8192 * 8192
      d.G = scan_geom(I);
      ws += segment_status_bytes(I);
      max_seg = d.nseg > max_seg ? d.nseg : max_seg;
    }
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(max_seg, (unsigned)n), dim3(kT), 0, (hipStream_t)stream, b);
    hipLaunchKernelGGL(jpeg_status_kernel, dim3(1, (unsigned)n), dim3(256), 0, (hipStream_t)stream, b);
    if (hipGetLastError() != hipSuccess) { fail(who, "launch failed"); return -2; }
  }
  return 0;
}

extern "C" int es_jpeg_entropy_decode_parallel_host(const es_jpeg_info* infos, int count, const uint8_t* const* bytes, const size_t* bytes_n,
                                                    const es_jpeg_segment* const* segments, const void* const* tables, int subseq_bytes,
                                                    int threads, int16_t* const* coeffs, int32_t* status, int32_t* rounds_out) {
  const char* who = "es_jpeg_entropy_decode_parallel_host";
  if (!bytes || !bytes_n || !segments || !tables || !coeffs || !status) return fail(who, "null pointer");
  if (const char* why = check_infos(infos, count)) return fail(who, why);
  if (const char* why = check_subseq(subseq_bytes)) return fail(who, why);
  if (threads < 1 || threads > kT) return fail(who, "threads must be 1 .. 1024");
  if (es_plan_recording()) return fail(who, "a plan is recording on this thread; the JPEG calls are never part of a plan");
  for (int i = 0; i < count; ++i) {
    if (!bytes[i] || !segments[i] || !tables[i] || !coeffs[i]) return fail(who, "null pointer");
    if (bytes_n[i] >= kMaxParallelFile) return fail(who, "a file of 256 MiB or more is not decoded in parallel");
  }
  uint32_t most = 0;
  for (int i = 0; i < count; ++i) {
    ScanTables T;
    memcpy(&T, tables[i], sizeof(T));
    uint32_t rounds = 0;
    status[i] = entropy_decode_parallel(bytes[i], bytes_n[i], infos[i], segments[i], T, (uint32_t)subseq_bytes, (uint32_t)threads, coeffs[i], &rounds);
    most = rounds > most ? rounds : most;
  }
  if (rounds_out) *rounds_out = (int32_t)most;
  return 0;
}

extern "C" size_t es_jpeg_decode_dev_staging_bytes(const es_jpeg_info* infos, const size_t* n, int count, size_t* upload_bytes) {
  const char* who = "es_jpeg_decode_dev_staging_bytes";
  if (!n || !upload_bytes) { fail(who, "null pointer"); return 0; }
  if (const char* why = check_infos(infos, count)) { fail(who, why); return 0; }
  if (es_plan_recording()) { fail(who, "a plan is recording on this thread; the JPEG calls are never part of a plan"); return 0; }
  size_t up = 0, dev = 0;
  for (int i = 0; i < count; ++i) {
    if (n[i] >= kMaxParallelFile) { fail(who, "a file of 256 MiB or more is not decoded in parallel"); return 0; }
    up += dev_layout(infos[i], n[i]).upload;
    dev += align16(coeff_count(infos[i]) * sizeof(int16_t));
  }
  *upload_bytes = up;
  return up + dev + entropy_workspace_bytes(infos, count);
}

extern "C" int es_jpeg_decode_dev_u8(const uint8_t* const* bytes, const size_t* n, int count, const es_image_u8* out, int subseq_bytes,
                                     int32_t* status_dev, void* staging_host, size_t staging_host_bytes, void* staging_dev,
                                     size_t staging_dev_bytes, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "es_jpeg_decode_dev_u8";
  if (!bytes || !n || !out || !status_dev || !staging_host || !staging_dev || !workspace) return fail(who, "null pointer");
  if (count < 1) return fail(who, "count < 1");
  if (count > kMaxDecode) return fail(who, "count > 64");
  if ((uintptr_t)staging_host % 16 || (uintptr_t)staging_dev % 16) return fail(who, "the staging buffers must be 16-byte aligned");
  if (es_plan_recording()) return fail(who, "a plan is recording on this thread; the JPEG calls are never part of a plan");
  es_jpeg_info infos[kMaxDecode];
  const uint8_t* bytes_dev[kMaxDecode];
  const es_jpeg_segment* seg_dev[kMaxDecode];
  const void* tab_dev[kMaxDecode];
  const uint16_t* qt_dev[kMaxDecode];
  int16_t* coef_dev[kMaxDecode];
  const char* why = nullptr;
  size_t up = 0, dev = 0;
  Header H;
  uint8_t *hs = (uint8_t*)staging_host, *ds = (uint8_t*)staging_dev;
  size_t coef_at[kMaxDecode];
  for (int i = 0; i < count; ++i) {               // one parse per file: the host staging is filled as the sizes become known, and nothing
    if (!bytes[i]) return fail(who, "null pointer");                     // reaches the device before every size has been checked
    if (!parse_header(bytes[i], n[i], H, &why)) return fail(who, why);
    if (n[i] >= kMaxParallelFile) return fail(who, "a file of 256 MiB or more is not decoded in parallel");
    infos[i] = H.info;
    const DevLayout L = dev_layout(H.info, n[i]);
    const size_t at = up;
    if (staging_host_bytes < at + L.upload) return fail(who, "staging_host too small (es_jpeg_decode_dev_staging_bytes)");
    memset(hs + at, 0, L.upload);
    memcpy(hs + at + L.file, bytes[i], n[i]);
    ScanTables* T = (ScanTables*)(hs + at + L.tab);
    if (!scan_prepare(bytes[i], n[i], H, (es_jpeg_segment*)(hs + at + L.seg), T, &why)) return fail(who, why);
    component_qtables(H, (uint16_t*)(hs + at + L.qt));
    bytes_dev[i] = ds + at + L.file;
    seg_dev[i] = (const es_jpeg_segment*)(ds + at + L.seg);
    tab_dev[i] = ds + at + L.tab;
    qt_dev[i] = (const uint16_t*)(ds + at + L.qt);
    coef_at[i] = dev;
    up += L.upload;
    dev += align16(coeff_count(H.info) * sizeof(int16_t));
  }
  const size_t ews = entropy_workspace_bytes(infos, count);
  if (staging_dev_bytes < up + dev + ews) return fail(who, "staging_dev too small (es_jpeg_decode_dev_staging_bytes)");
  for (int i = 0; i < count; ++i) coef_dev[i] = (int16_t*)(ds + up + coef_at[i]);
  const size_t cat = up + dev;
  if (hipMemcpyAsync(staging_dev, staging_host, up, hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess) { fail(who, "upload failed"); return -2; }
  const int rc = es_jpeg_entropy_decode(infos, count, bytes_dev, n, seg_dev, tab_dev, subseq_bytes, coef_dev, status_dev, ds + cat, ews, stream);
  if (rc != 0) return rc;
  return es_jpeg_reconstruct(infos, count, coef_dev, qt_dev, out, workspace, workspace_bytes, stream);
}
