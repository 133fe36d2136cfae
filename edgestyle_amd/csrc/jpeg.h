// Baseline JPEG, the host half and the shared integer rules (include/edgestyle_hip.h states format, limits and arithmetic in full):
// the marker parser and the Huffman decoder - serial by nature, plain C++ - and, behind ES_JPEG_HD, the per-sample rules that
// csrc/jpeg.hip's kernels and the host twin both run: the 1-D pass of the "islow" inverse DCT, its two descalings, libjpeg's triangle
// chroma upsampling and YCbCr -> RGB; and the per-symbol code of the opt-in parallel Huffman decoder (csrc/jpeg_entropy.hip and its host
// twin; the serial decoder stays the default).  Everything is integer arithmetic.  Any C++17 compiler can compile this header alone
// (examples/jpeg_host.cpp -DJPEG_HOST_DRY does, under a host sanitizer for instance): no HIP, no library.
//
// Safety on hostile bytes: every read of the file is bounds-checked against n (BitReader feeds zero bits once it has met a marker or the
// end, and the decoder refuses the file as soon as one of those bits was consumed); every coefficient index is checked against 63 before
// the store; block addresses come from the MCU counters alone, never from the file.  The inverse DCT is computed modulo 2^32.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/edgestyle_hip.h"

#if defined(__HIPCC__)
#define ES_JPEG_HD __host__ __device__
#else
#define ES_JPEG_HD
#endif

namespace esjpeg {

// ---- the shared integer rules ---------------------------------------------------------------------------------------------------
// One 8-point pass of jidctint.c's factorisation (CONST_BITS = 13) on dequantised values, before descaling; modulo 2^32.
ES_JPEG_HD inline void idct_1d(const uint32_t c[8], uint32_t o[8]) {
  uint32_t z1 = (c[2] + c[6]) * 4433u;
  const uint32_t e2 = z1 - c[6] * 15137u, e3 = z1 + c[2] * 6270u;
  const uint32_t e0 = (c[0] + c[4]) * 8192u, e1 = (c[0] - c[4]) * 8192u;
  const uint32_t t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  uint32_t t0 = c[7], t1 = c[5], t2 = c[3], t3 = c[1];
  z1 = t0 + t3;
  uint32_t z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const uint32_t z5 = (z3 + z4) * 9633u;
  t0 *= 2446u; t1 *= 16819u; t2 *= 25172u; t3 *= 12299u;
  z1 *= 0u - 7373u; z2 *= 0u - 20995u; z3 *= 0u - 16069u; z4 *= 0u - 3196u;
  z3 += z5; z4 += z5;
  t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
  o[0] = t10 + t3; o[7] = t10 - t3;
  o[1] = t11 + t2; o[6] = t11 - t2;
  o[2] = t12 + t1; o[5] = t12 - t1;
  o[3] = t13 + t0; o[4] = t13 - t0;
}
// after the column pass: (x + 1024) >> 11, an arithmetic shift of the two's-complement reading
ES_JPEG_HD inline uint32_t descale_column(uint32_t x) { return (uint32_t)((int32_t)(x + 1024u) >> 11); }
// after the row pass: (x + 2^17) >> 18, + 128, clamped
ES_JPEG_HD inline uint8_t descale_sample(uint32_t x) {
  const int32_t v = ((int32_t)(x + (1u << 17)) >> 18) + 128;
  return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}
ES_JPEG_HD inline uint32_t dequant(int16_t coef, uint16_t q) { return (uint32_t)(int32_t)coef * (uint32_t)q; }

enum { kUpNone = 0, kUpH2V1 = 1, kUpH2V2 = 2 };
// The value of a subsampled component at full-resolution pixel (x, y).  p: its plane, dw x dh real samples in rows of `stride` bytes.
ES_JPEG_HD inline int upsampled(const uint8_t* p, size_t stride, int dw, int dh, int mode, int x, int y) {
  if (mode == kUpNone) return p[(size_t)y * stride + x];
  const int i = x >> 1;
  if (mode == kUpH2V1) {
    const uint8_t* row = p + (size_t)y * stride;
    if (dw <= 2) return row[i];
    const int j = (x & 1) ? (i + 1 < dw ? i + 1 : dw - 1) : (i > 0 ? i - 1 : 0);
    return (3 * row[i] + row[j] + ((x & 1) ? 2 : 1)) >> 2;
  }
  const int cy = y >> 1;
  const uint8_t* near = p + (size_t)cy * stride;
  if (dw <= 2) return near[i];
  const int fy = (y & 1) ? (cy + 1 < dh ? cy + 1 : dh - 1) : (cy > 0 ? cy - 1 : 0);
  const uint8_t* far = p + (size_t)fy * stride;
  const int j = (x & 1) ? (i + 1 < dw ? i + 1 : dw - 1) : (i > 0 ? i - 1 : 0);
  const int si = 3 * near[i] + far[i], sj = 3 * near[j] + far[j];
  return (3 * si + sj + ((x & 1) ? 7 : 8)) >> 4;
}
ES_JPEG_HD inline int clamp8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
ES_JPEG_HD inline void ycc_to_rgb(int y, int cb, int cr, uint8_t rgb[3]) {
  cb -= 128; cr -= 128;
  rgb[0] = (uint8_t)clamp8(y + ((91881 * cr + 32768) >> 16));
  rgb[1] = (uint8_t)clamp8(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  rgb[2] = (uint8_t)clamp8(y + ((116130 * cb + 32768) >> 16));
}
ES_JPEG_HD inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
ES_JPEG_HD inline int up_mode(int h, int v) { return h == 1 ? kUpNone : v == 1 ? kUpH2V1 : kUpH2V2; }

// ---- geometry ----------------------------------------------------------------------------------------------------------------------
// fills the derived fields from width, height, components, h, v; false for what this decoder does not take
inline bool derive_geometry(es_jpeg_info& I, const char** why) {
  if (I.width < 1 || I.height < 1 || I.width > 65535 || I.height > 65535) { *why = "height or width of 0 or above 65535"; return false; }
  if (I.components == 1) {
    I.h[0] = I.v[0] = 1;                          // a scan of one component is not interleaved: its MCU is one block
    for (int c = 1; c < 3; ++c) I.h[c] = I.v[c] = I.tq[c] = I.td[c] = I.ta[c] = 0;
  } else if (I.components == 3) {
    const bool luma_ok = (I.h[0] == 1 && I.v[0] == 1) || (I.h[0] == 2 && I.v[0] == 1) || (I.h[0] == 2 && I.v[0] == 2);
    if (!luma_ok || I.h[1] != 1 || I.v[1] != 1 || I.h[2] != 1 || I.v[2] != 1) {
      *why = "sampling factors other than 4:4:4, 4:2:2 (2x1) and 4:2:0 (2x2) are not supported";
      return false;
    }
  } else { *why = "1 or 3 components expected"; return false; }
  I.hmax = I.h[0]; I.vmax = I.v[0];
  I.mcus_x = ceil_div(I.width, 8 * I.hmax);
  I.mcus_y = ceil_div(I.height, 8 * I.vmax);
  for (int c = 0; c < 3; ++c) {
    I.blocks_w[c] = c < I.components ? I.mcus_x * I.h[c] : 0;
    I.blocks_h[c] = c < I.components ? I.mcus_y * I.v[c] : 0;
  }
  return true;
}
// an es_jpeg_info a caller hands back: every field must be what derive_geometry gives (the kernels index by them)
inline bool info_ok(const es_jpeg_info* info, const char** why) {
  if (!info) { *why = "null info"; return false; }
  es_jpeg_info I = *info;
  if (!derive_geometry(I, why)) return false;
  for (int c = 0; c < 3; ++c)
    if ((unsigned)info->tq[c] > 3u || (unsigned)info->td[c] > 3u || (unsigned)info->ta[c] > 3u) { *why = "table selector above 3"; return false; }
  if (info->restart_interval < 0 || info->restart_interval > 65535) { *why = "restart interval out of range"; return false; }
  if (memcmp(&I, info, sizeof(I)) != 0) { *why = "the info's derived fields do not belong to its size and sampling"; return false; }
  return true;
}
inline size_t component_blocks(const es_jpeg_info& I, int c) { return (size_t)I.blocks_w[c] * (size_t)I.blocks_h[c]; }
inline size_t coeff_count(const es_jpeg_info& I) {
  size_t n = 0;
  for (int c = 0; c < I.components; ++c) n += component_blocks(I, c) * 64;
  return n;
}
// real samples of component c
ES_JPEG_HD inline int comp_w(const es_jpeg_info& I, int c) { return ceil_div(I.width * I.h[c], I.hmax); }
ES_JPEG_HD inline int comp_h(const es_jpeg_info& I, int c) { return ceil_div(I.height * I.v[c], I.vmax); }

// ---- headers -----------------------------------------------------------------------------------------------------------------------
static const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
  bool present;
  uint8_t vals[256];
  int32_t maxcode[18];                            // largest code of each length, -1: none
  int32_t valoff[17];                             // vals index of a code of length l = code + valoff[l]
  uint16_t look[512];                             // the next 9 bits -> length << 8 | symbol for codes of up to 9 bits, 0: longer
};
inline bool build_huff(Huff& t, const uint8_t counts[16], const uint8_t* vals, int total, bool dc, const char** why) {
  memset(&t, 0, sizeof(t));
  for (int i = 0; i < total; ++i) {
    if (dc && vals[i] > 15) { *why = "DHT: a DC category above 15"; return false; }
    t.vals[i] = vals[i];
  }
  int32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int cnt = counts[l - 1];
    if (code + cnt > (1 << l)) { *why = "DHT: more codes of one length than the code space holds"; return false; }
    t.valoff[l] = k - code;
    for (int i = 0; i < cnt; ++i, ++code, ++k)
      if (l <= 9)
        for (int f = 0; f < (1 << (9 - l)); ++f) t.look[(code << (9 - l)) | f] = (uint16_t)(l << 8 | t.vals[k]);
    t.maxcode[l] = cnt ? code - 1 : -1;
    code <<= 1;
  }
  t.maxcode[17] = 0x7fffffff;
  t.present = true;
  return true;
}

struct Header {
  es_jpeg_info info;
  uint16_t qt[4][64];                             // natural order
  bool qt_ok[4];
  Huff dc[4], ac[4];
  size_t scan_pos;                                // first byte of the entropy-coded data
};

inline bool parse_header(const uint8_t* p, size_t n, Header& H, const char** why) {
  memset(&H.info, 0, sizeof(H.info));
  for (int i = 0; i < 4; ++i) { H.qt_ok[i] = false; H.dc[i].present = H.ac[i].present = false; }
  H.scan_pos = 0;
  if (!p || n < 4 || p[0] != 0xFF || p[1] != 0xD8) { *why = "not a JPEG file (no SOI marker)"; return false; }
  size_t pos = 2;
  bool sof = false, jfif = false, adobe = false;
  int adobe_transform = -1;
  uint8_t ids[3] = {0, 0, 0};
  es_jpeg_info& I = H.info;
  for (;;) {
    if (pos >= n) { *why = "truncated: the file ends before the scan"; return false; }
    if (p[pos] != 0xFF) { *why = "malformed: no marker where one must stand"; return false; }
    while (pos < n && p[pos] == 0xFF) ++pos;      // fill bytes
    if (pos >= n) { *why = "truncated: the file ends inside a marker"; return false; }
    const int m = p[pos++];
    if (m == 0x01) continue;                      // TEM stands alone
    if (m == 0x00 || m == 0xD8 || (m >= 0xD0 && m <= 0xD7)) { *why = "malformed: a stuffed byte, SOI or RSTn between the headers"; return false; }
    if (m == 0xD9) { *why = "malformed: EOI before any scan"; return false; }
    if (pos + 2 > n) { *why = "truncated: the file ends inside a segment length"; return false; }
    const size_t len = (size_t)p[pos] << 8 | p[pos + 1];
    if (len < 2 || len > n - pos) { *why = "truncated or malformed: a segment reaches past the end of the file"; return false; }
    const uint8_t* s = p + pos + 2;
    size_t sl = len - 2;
    pos += len;
    switch (m) {
      case 0xC2: *why = "progressive JPEG (SOF2) is not supported"; return false;
      case 0xC3: case 0xC5: case 0xC6: case 0xC7: case 0xCB: case 0xCD: case 0xCE: case 0xCF:
        *why = "lossless and hierarchical JPEG are not supported"; return false;
      case 0xC9: case 0xCA: case 0xCC: *why = "arithmetic coding is not supported"; return false;
      case 0xDC: *why = "a DNL segment (height given after the scan) is not supported"; return false;
      case 0xC0: case 0xC1: {
        if (sof) { *why = "malformed: a second frame header"; return false; }
        if (sl < 6) { *why = "malformed: short frame header"; return false; }
        if (s[0] == 12) { *why = "12-bit samples are not supported"; return false; }
        if (s[0] != 8) { *why = "sample precision other than 8 bits"; return false; }
        I.height = s[1] << 8 | s[2];
        I.width = s[3] << 8 | s[4];
        I.components = s[5];
        if (I.components == 4) { *why = "4 components (CMYK / YCCK) are not supported"; return false; }
        if (I.components != 1 && I.components != 3) { *why = "1 or 3 components expected"; return false; }
        if (sl != (size_t)(6 + 3 * I.components)) { *why = "malformed: frame header length"; return false; }
        for (int c = 0; c < I.components; ++c) {
          ids[c] = s[6 + 3 * c];
          I.h[c] = s[7 + 3 * c] >> 4;
          I.v[c] = s[7 + 3 * c] & 15;
          I.tq[c] = s[8 + 3 * c];
          if (I.h[c] < 1 || I.h[c] > 4 || I.v[c] < 1 || I.v[c] > 4 || I.tq[c] > 3) { *why = "malformed: sampling factor or table selector out of range"; return false; }
        }
        if (I.width == 0 || I.height == 0) { *why = "height or width of 0"; return false; }
        sof = true;
        break;
      }
      case 0xDB:
        while (sl > 0) {
          const int pq = s[0] >> 4, tq = s[0] & 15;
          if (pq > 1 || tq > 3) { *why = "malformed: DQT precision or table number"; return false; }
          const size_t need = 1 + (size_t)64 * (pq + 1);
          if (sl < need) { *why = "malformed: short DQT segment"; return false; }
          for (int i = 0; i < 64; ++i)
            H.qt[tq][kNatural[i]] = pq ? (uint16_t)(s[1 + 2 * i] << 8 | s[2 + 2 * i]) : s[1 + i];
          H.qt_ok[tq] = true;
          s += need; sl -= need;
        }
        break;
      case 0xC4:
        while (sl > 0) {
          const int tc = s[0] >> 4, th = s[0] & 15;
          if (tc > 1 || th > 3) { *why = "malformed: DHT class or table number"; return false; }
          if (sl < 17) { *why = "malformed: short DHT segment"; return false; }
          int total = 0;
          for (int i = 0; i < 16; ++i) total += s[1 + i];
          if (total > 256 || sl < (size_t)(17 + total)) { *why = "malformed: DHT symbol count"; return false; }
          if (!build_huff(tc ? H.ac[th] : H.dc[th], s + 1, s + 17, total, tc == 0, why)) return false;
          s += 17 + total; sl -= 17 + total;
        }
        break;
      case 0xDD:
        if (sl != 2) { *why = "malformed: DRI length"; return false; }
        I.restart_interval = s[0] << 8 | s[1];
        break;
      case 0xE0:
        if (sl >= 5 && memcmp(s, "JFIF", 5) == 0) jfif = true;
        break;
      case 0xEE:
        if (sl >= 12 && memcmp(s, "Adobe", 5) == 0) { adobe = true; adobe_transform = s[11]; }
        break;
      case 0xDA: {
        if (!sof) { *why = "malformed: a scan before the frame header"; return false; }
        if (sl < 1) { *why = "malformed: short scan header"; return false; }
        if (s[0] != I.components) { *why = "multi-scan files are not supported (the scan does not hold every component)"; return false; }
        if (sl != (size_t)(4 + 2 * I.components)) { *why = "malformed: scan header length"; return false; }
        for (int c = 0; c < I.components; ++c) {
          if (s[1 + 2 * c] != ids[c]) { *why = "malformed: the scan's components are not the frame's, in order"; return false; }
          I.td[c] = s[2 + 2 * c] >> 4;
          I.ta[c] = s[2 + 2 * c] & 15;
          if (I.td[c] > 3 || I.ta[c] > 3) { *why = "malformed: Huffman table selector above 3"; return false; }
          if (!H.qt_ok[I.tq[c]]) { *why = "a quantisation table the frame names is missing"; return false; }
          if (!H.dc[I.td[c]].present || !H.ac[I.ta[c]].present) { *why = "a Huffman table the scan names is missing"; return false; }
        }
        const uint8_t* t = s + 1 + 2 * I.components;
        if (t[0] != 0 || t[1] != 63 || t[2] != 0) { *why = "spectral selection or successive approximation in a sequential scan"; return false; }
        if (I.components == 3 && !jfif) {         // libjpeg's order: JFIF decides, then Adobe, then the ids
          if (adobe && adobe_transform != 1) { *why = "Adobe transform other than 1 (the samples are not YCbCr)"; return false; }
          if (!adobe && ids[0] == 'R' && ids[1] == 'G' && ids[2] == 'B') { *why = "component ids R, G, B (the samples are not YCbCr)"; return false; }
        }
        if (!derive_geometry(I, why)) return false;
        H.scan_pos = pos;
        return true;
      }
      default: break;                             // APPn, COM and whatever else carries a length: skipped
    }
  }
}

// ---- entropy decoding ---------------------------------------------------------------------------------------------------------------
struct BitReader {
  const uint8_t* p;
  size_t n, pos;
  uint64_t acc = 0;                               // the next `cnt` bits, from the top
  int cnt = 0;
  long long fake = 0;                             // zero bits fed after a marker or the end was met (they are the last ones in acc)
  bool stop = false;
  BitReader(const uint8_t* p_, size_t n_, size_t pos_) : p(p_), n(n_), pos(pos_) {}
  inline void fill() {
    while (cnt <= 56) {
      uint64_t byte = 0;
      if (!stop && pos < n) {
        byte = p[pos];
        if (byte != 0xFF) ++pos;
        else {
          size_t q = pos + 1;
          while (q < n && p[q] == 0xFF) ++q;      // fill bytes
          if (q < n && p[q] == 0) pos = q + 1;    // FF 00: the data byte FF
          else { stop = true; byte = 0; }         // a marker (pos stays on it) or the end
        }
      } else stop = true;
      if (stop) fake += 8;
      acc |= byte << (56 - cnt);
      cnt += 8;
    }
  }
  inline uint32_t peek(int k) const { return (uint32_t)(acc >> (64 - k)); }        // 1 <= k <= 32
  inline void skip(int k) { acc <<= k; cnt -= k; }
  inline bool overran() const { return cnt < fake; }
};
// -1: no code of up to 16 bits matches
inline int decode_symbol(BitReader& b, const Huff& t) {
  const uint16_t e = t.look[b.peek(9)];
  if (e) { b.skip(e >> 8); return e & 255; }
  for (int l = 10; l <= 16; ++l) {
    const int32_t code = (int32_t)b.peek(l);
    if (code <= t.maxcode[l]) { b.skip(l); return t.vals[(code + t.valoff[l]) & 255]; }
  }
  return -1;
}
inline int receive_extend(BitReader& b, int s) {  // 1 <= s <= 15
  const int v = (int)b.peek(s);
  b.skip(s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}
// the marker that follows position pos (fill bytes and stray data skipped); -1 when the file ends first
inline int next_marker(const uint8_t* p, size_t n, size_t& pos) {
  for (;;) {
    if (pos >= n) return -1;
    if (p[pos] != 0xFF) { ++pos; continue; }
    size_t q = pos + 1;
    while (q < n && p[q] == 0xFF) ++q;
    if (q >= n) return -1;
    pos = q + 1;
    if (p[q] != 0) return p[q];
  }
}

// coeffs: [coeff_count(H.info)], every value written
inline bool entropy_decode(const uint8_t* p, size_t n, const Header& H, int16_t* coeffs, const char** why) {
  const es_jpeg_info& I = H.info;
  memset(coeffs, 0, coeff_count(I) * sizeof(int16_t));
  size_t off[3] = {0, 0, 0};
  for (int c = 1; c < I.components; ++c) off[c] = off[c - 1] + component_blocks(I, c - 1) * 64;
  const long long total = (long long)I.mcus_x * I.mcus_y;
  const long long ri = I.restart_interval ? I.restart_interval : total;
  BitReader b(p, n, H.scan_pos);
  int pred[3] = {0, 0, 0};
  int rst = 0;
  int mx = 0, my = 0;
  for (long long mcu = 0; mcu < total; ++mcu) {
    if (mcu && mcu % ri == 0) {
      size_t pos = b.pos;
      const int m = next_marker(p, n, pos);
      if (m != 0xD0 + (rst & 7)) { *why = m < 0 ? "truncated: the file ends where an RSTn marker must stand" : "a missing or misnumbered RSTn marker"; return false; }
      ++rst;
      b = BitReader(p, n, pos);
      pred[0] = pred[1] = pred[2] = 0;
    }
    for (int c = 0; c < I.components; ++c) {
      const Huff &dc = H.dc[I.td[c]], &ac = H.ac[I.ta[c]];
      for (int vy = 0; vy < I.v[c]; ++vy)
        for (int hx = 0; hx < I.h[c]; ++hx) {
          int16_t* blk = coeffs + off[c] + ((size_t)(my * I.v[c] + vy) * I.blocks_w[c] + (size_t)(mx * I.h[c] + hx)) * 64;
          b.fill();
          int s = decode_symbol(b, dc);
          if (s < 0) { *why = "a bit pattern that is no Huffman code (DC)"; return false; }
          if (s) pred[c] += receive_extend(b, s);
          if (pred[c] < -32768 || pred[c] > 32767) { *why = "a DC coefficient outside 16 bits"; return false; }
          blk[0] = (int16_t)pred[c];
          for (int k = 1; k < 64;) {
            b.fill();
            const int rs = decode_symbol(b, ac);
            if (rs < 0) { *why = "a bit pattern that is no Huffman code (AC)"; return false; }
            const int r = rs >> 4;
            s = rs & 15;
            if (s == 0) {
              if (r != 15) break;                 // EOB
              k += 16;
              if (k > 64) { *why = "a zero run past coefficient 63"; return false; }
              continue;
            }
            k += r;
            if (k > 63) { *why = "a zero run past coefficient 63"; return false; }
            blk[kNatural[k++]] = (int16_t)receive_extend(b, s);
          }
        }
    }
    if (b.overran()) { *why = "truncated: the entropy-coded data ends before the last MCU"; return false; }
    if (++mx == I.mcus_x) { mx = 0; ++my; }
  }
  size_t pos = b.pos;
  const int m = next_marker(p, n, pos);
  if (m < 0) { *why = "truncated: no EOI marker after the scan"; return false; }
  if (m != 0xD9) { *why = "multi-scan files are not supported (a segment follows the scan)"; return false; }
  return true;
}

// qtables: uint16 [components][64], per component, natural order
inline void component_qtables(const Header& H, uint16_t* qtables) {
  for (int c = 0; c < H.info.components; ++c) memcpy(qtables + 64 * c, H.qt[H.info.tq[c]], 64 * sizeof(uint16_t));
}

// ---- parallel entropy decoding (csrc/jpeg_entropy.hip and its host twin) ----------------------------------------------------------------
// A SEGMENT is the stretch of entropy-coded bytes between restart markers; it is cut into subsequences of S raw bytes, one decoder
// each.  Huffman streams re-synchronise, so a decoder started at a guessed state falls into step with the true symbol boundaries; the
// subsequences exchange their exit states until nothing changes (at most J + 1 rounds for J subsequences), then decode once more from
// the true states and write.  The per-symbol code below is what the kernel and the twin (entropy_decode_parallel) both compile.
//
// Bits are read from the RAW bytes, with no compaction pass.  Inside a segment a byte carries data unless it is a 00 that follows an FF
// (the stuffed byte) or an FF that is followed by an FF (a fill byte): FF 00 is the data byte FF and FF FF 00 is ONE data byte FF, as
// BitReader reads them.  A position is (raw byte, bit in it); it is kept canonical - on a data byte, or at the segment's end with bit
// 0 - so that two decoders that meet at a symbol boundary hold the same number.
//
// Safety: every loop is bounded by the segment's length; a symbol takes at least one bit; a table entry the host would never build
// (length 0 or above 16) counts as "no code"; table indices are masked; coefficient addresses come from block counters that are
// checked against the geometry, never from the stream.
inline uint64_t restart_intervals(const es_jpeg_info& I);       // (below, with the encoder's geometry)
struct HuffFlat {                                 // Huff without `present`, plain data
  uint16_t look[512];
  int32_t maxcode[18];
  int32_t valoff[17];
  uint8_t vals[256];
};
struct ScanTables {                               // what es_jpeg_scan_prepare_host writes: ES_JPEG_TABLES_BYTES
  HuffFlat t[6];                                  // [2 c]: the DC table of component c, [2 c + 1]: its AC table
  int32_t components;
  int32_t td[3], ta[3];                           // the selectors the scan named (for the record: t[] is already per component)
  int32_t pad[3];
};
static_assert(sizeof(ScanTables) == ES_JPEG_TABLES_BYTES, "ES_JPEG_TABLES_BYTES");
static_assert(sizeof(es_jpeg_segment) == 8, "es_jpeg_segment");

enum { kStOk = 0, kStBadDC = 1, kStBadAC = 2, kStRun = 3, kStDCRange = 4, kStTruncated = 5 };
inline const char* status_text(int code) {
  switch (code) {
    case kStOk: return "no defect";
    case kStBadDC: return "a bit pattern that is no Huffman code (DC)";
    case kStBadAC: return "a bit pattern that is no Huffman code (AC)";
    case kStRun: return "a zero run past coefficient 63";
    case kStDCRange: return "a DC coefficient outside 16 bits";
    case kStTruncated: return "truncated: the entropy-coded data ends before the last MCU";
    default: return "unknown JPEG status";
  }
}
constexpr uint32_t kDefaultSubseq = 128;          // raw bytes per subsequence when the caller passes 0: the reference's 512 x 512 photo
                                                  // settles in 4 rounds at 128 (11 at 32, 6 at 64, 3 at 256): rounds x bytes is lowest near here
constexpr uint32_t kMinSubseq = 4;
constexpr size_t kMaxParallelFile = (size_t)1 << 28;   // bit positions are 32-bit numbers

// The decoder's state at a symbol boundary.  pos: raw byte * 8 + bit inside the segment; bk: block within the MCU << 8 | next zigzag
// index (0: a DC symbol comes next).  kDead: where a speculative decode ends that met an impossible code - a pure function of the entry.
// A decoder handed a dead entry proposes from its own guess again (else one impossible code would silence every decoder after it
// until the true state arrives).  Once the rounds have settled, the entries up to the first dead one are the true ones; that one and
// every entry behind it (guesses, not true states) count as dead in the count and write passes: they decode and write nothing.  The
// true decode dies only on a defect, which the decoder before the dead entry reports if its block lies inside the segment's share -
// stray bytes behind the last block are the usual cause, and are no error.
struct ScanState { uint32_t pos, bk; };
constexpr uint32_t kDeadPos = 0xFFFFFFFFu;
ES_JPEG_HD inline ScanState dead_state() { return ScanState{kDeadPos, 0xFFFFu}; }
ES_JPEG_HD inline bool same_state(const ScanState& a, const ScanState& b) { return a.pos == b.pos && a.bk == b.bk; }

// the first data byte at or after j (len: none)
ES_JPEG_HD inline uint32_t next_data(const uint8_t* p, uint32_t len, uint32_t j) {
  while (j < len) {
    const uint8_t b = p[j];
    if (b == 0xFF) {
      if (j + 1 < len && p[j + 1] != 0xFF) return j;     // FF 00: the data byte FF
    } else if (!(b == 0 && j > 0 && p[j - 1] == 0xFF)) return j;
    ++j;
  }
  return len;
}
struct RawBits {
  const uint8_t* p;                               // the segment's raw bytes
  uint32_t len;
  uint32_t i, bit;                                // the next bit: bit `bit` (from the top) of data byte i; or i == len, bit == 0
  uint32_t w, n1, n2;                             // the window: data bytes i, n1, n2 in bits 23 .. 0 (zero past the end), and where they lie
  ES_JPEG_HD inline void window() {
    if (i + 2 < len) {
      const uint32_t b0 = p[i], b1 = p[i + 1], b2 = p[i + 2];
      if (b0 != 0xFF && b1 != 0xFF && b2 != 0xFF) { w = b0 << 16 | b1 << 8 | b2; n1 = i + 1; n2 = i + 2; return; }
    }
    w = 0; n1 = n2 = len;
    if (i >= len) return;
    w = (uint32_t)p[i] << 16;
    n1 = next_data(p, len, i + 1);
    if (n1 >= len) return;
    w |= (uint32_t)p[n1] << 8;
    n2 = next_data(p, len, n1 + 1);
    if (n2 < len) w |= p[n2];
  }
  ES_JPEG_HD inline uint32_t peek16() const { return (w >> (8 - bit)) & 0xFFFFu; }                    // after window()
  ES_JPEG_HD inline uint32_t peek(int n) const { return (w >> (24 - (int)bit - n)) & ((1u << n) - 1u); }   // 1 <= n <= 16
  // consumes n <= 16 bits of the window; false: they reach past the segment's real bits
  ES_JPEG_HD inline bool skip(int n) {
    const uint32_t have = 8u * ((i < len) + (n1 < len) + (n2 < len));
    const uint32_t total = bit + (uint32_t)n;
    if (total > have) { i = len; bit = 0; return false; }
    const uint32_t adv = total >> 3;
    i = adv == 0 ? i : adv == 1 ? n1 : n2;
    bit = total & 7u;
    return true;
  }
};
// >= 0: the symbol; -1: no code of up to 16 bits matches; -2: the code ends past the segment's real bits
ES_JPEG_HD inline int take_code(RawBits& r, const HuffFlat& t) {
  r.window();
  const uint32_t v = r.peek16();
  const uint32_t e = t.look[v >> 7];
  int l = (int)(e >> 8), sym = (int)(e & 255u);
  if (!e) {
    l = 0;
    for (int q = 10; q <= 16; ++q) {
      const int32_t code = (int32_t)(v >> (16 - q));
      if (code <= t.maxcode[q]) { l = q; sym = t.vals[(uint32_t)(code + t.valoff[q]) & 255u]; break; }
    }
    if (!l) return -1;
  } else if (l < 1 || l > 9) return -1;
  return r.skip(l) ? sym : -2;
}
// the s extra bits of a coefficient, 1 <= s <= 15, extended; false: they reach past the segment's real bits
ES_JPEG_HD inline bool take_value(RawBits& r, int s, int* out) {
  r.window();
  const int v = (int)r.peek(s);
  if (!r.skip(s)) return false;
  *out = v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
  return true;
}

// The geometry the passes need, by value (what a kernel gets as its argument)
struct ScanGeom {
  uint64_t off[3];                                // first coefficient of each component
  int32_t components, h, v, hv, bpm, mcus_x;      // luma blocks per MCU, blocks per MCU
  int32_t blocks_w[3];
  uint32_t mcus, ri;                              // MCUs of the image, MCUs per segment
};
inline ScanGeom scan_geom(const es_jpeg_info& I) {
  ScanGeom G;
  memset(&G, 0, sizeof(G));
  for (int c = 1; c < I.components; ++c) G.off[c] = G.off[c - 1] + component_blocks(I, c - 1) * 64;
  G.components = I.components; G.h = I.h[0]; G.v = I.v[0];
  G.hv = I.components == 1 ? 1 : I.h[0] * I.v[0];
  G.bpm = I.components == 1 ? 1 : G.hv + 2;
  G.mcus_x = I.mcus_x;
  for (int c = 0; c < 3; ++c) G.blocks_w[c] = I.blocks_w[c];
  G.mcus = (uint32_t)I.mcus_x * (uint32_t)I.mcus_y;
  G.ri = I.restart_interval > 0 ? (uint32_t)I.restart_interval : G.mcus;
  return G;
}
// blocks segment `seg` must hold (seg < ceil(mcus / ri))
ES_JPEG_HD inline uint32_t segment_blocks(const ScanGeom& G, uint32_t seg) {
  const uint32_t left = G.mcus - seg * G.ri;
  return (left < G.ri ? left : G.ri) * (uint32_t)G.bpm;
}
// where block `o` (o < segment_blocks) of segment `seg` lies in the coefficient buffer: entropy_decode's own formula
ES_JPEG_HD inline uint64_t segment_block_offset(const ScanGeom& G, uint32_t seg, uint32_t o) {
  const uint32_t mcu = seg * G.ri + o / (uint32_t)G.bpm, blk = o % (uint32_t)G.bpm;
  const uint32_t my = mcu / (uint32_t)G.mcus_x, mx = mcu - my * (uint32_t)G.mcus_x;
  if (blk < (uint32_t)G.hv) {
    const uint32_t vy = blk / (uint32_t)G.h, hx = blk - vy * (uint32_t)G.h;
    return ((uint64_t)(my * G.v + vy) * (uint32_t)G.blocks_w[0] + (mx * G.h + hx)) * 64u;
  }
  const int c = (int)(blk - (uint32_t)G.hv) + 1;
  return G.off[c] + ((uint64_t)my * (uint32_t)G.blocks_w[c] + mx) * 64u;
}

// Decodes the symbols whose first bit lies in raw bytes [.., bound) from state st; returns the state at the first symbol boundary at or
// past bound (or the segment's end), dead_state() after a defect.  The sink sees dc(component, difference), ac(zigzag index, value),
// and defect(status, whether a DC symbol was due).
template <class Sink>
ES_JPEG_HD inline ScanState decode_subsequence(const ScanTables& T, const ScanGeom& G, const uint8_t* p, uint32_t len, ScanState st, uint32_t bound,
                                               Sink& sink) {
  uint32_t b = st.bk >> 8, k = st.bk & 255u;
  if (st.pos == kDeadPos || (st.pos >> 3) > len || b >= (uint32_t)G.bpm || k > 63u) return dead_state();
  RawBits r{p, len, st.pos >> 3, st.pos & 7u, 0, 0, 0};
  if (bound > len) bound = len;
  const uint32_t most = bound > r.i ? (bound - r.i) * 8u : 0u;   // every symbol takes at least one bit
  for (uint32_t it = 0; it < most && r.i < bound; ++it) {
    const int c = b < (uint32_t)G.hv ? 0 : (int)(b - (uint32_t)G.hv) + 1;
    if (k == 0) {
      int s = take_code(r, T.t[2 * c]);
      if (s < 0) { sink.defect(s == -1 ? kStBadDC : kStTruncated, true); return dead_state(); }
      s &= 15;
      int diff = 0;
      if (s && !take_value(r, s, &diff)) { sink.defect(kStTruncated, true); return dead_state(); }
      sink.dc(c, diff);
      k = 1;
    } else {
      const int rs = take_code(r, T.t[2 * c + 1]);
      if (rs < 0) { sink.defect(rs == -1 ? kStBadAC : kStTruncated, false); return dead_state(); }
      const uint32_t run = (uint32_t)rs >> 4;
      const int s = rs & 15;
      if (s == 0) {
        if (run != 15u) k = 64;                   // EOB
        else {
          k += 16;
          if (k > 64u) { sink.defect(kStRun, false); return dead_state(); }
        }
      } else {
        k += run;
        if (k > 63u) { sink.defect(kStRun, false); return dead_state(); }
        int val = 0;
        if (!take_value(r, s, &val)) { sink.defect(kStTruncated, false); return dead_state(); }
        sink.ac(k, val);
        ++k;
      }
    }
    if (k >= 64u) { k = 0; b = b + 1 == (uint32_t)G.bpm ? 0 : b + 1; }
  }
  return ScanState{r.i * 8u + r.bit, b << 8 | k};
}
// the synchronise rounds: how many blocks start in the subsequence and what their DC differences sum to, modulo 2^32
struct CountSink {
  uint32_t dcs, sum[3];
  ES_JPEG_HD inline void clear() { dcs = sum[0] = sum[1] = sum[2] = 0; }
  ES_JPEG_HD inline void dc(int c, int diff) {      // (selects, not sum[c]: a dynamic index would put the array into scratch on the device)
    ++dcs;
    sum[0] += c == 0 ? (uint32_t)diff : 0u; sum[1] += c == 1 ? (uint32_t)diff : 0u; sum[2] += c == 2 ? (uint32_t)diff : 0u;
  }
  ES_JPEG_HD inline void ac(uint32_t, int) {}
  ES_JPEG_HD inline void defect(int, bool) {}
};
// The write pass.  next: the ordinal of the next block to start; cur: the ordinal of the block the decoder is inside (~0u: none, its
// values are dropped); blocks at or past `expected` are dropped and report nothing.  err: the first defect as ordinal << 3 | status.
struct WriteSink {
  const ScanGeom* G;
  const uint8_t* natural;
  int16_t* coeffs;
  uint32_t seg, expected, next, cur, pred[3], err;
  int16_t* blk;
  ES_JPEG_HD inline void enter(uint32_t o) {
    cur = o;
    blk = o < expected ? coeffs + segment_block_offset(*G, seg, o) : nullptr;
  }
  ES_JPEG_HD inline void note(uint32_t o, int status) {
    if (o >= expected) return;
    const uint32_t key = o << 3 | (uint32_t)status;
    if (key < err) err = key;
  }
  ES_JPEG_HD inline void dc(int c, int diff) {
    enter(next++);
    pred[0] += c == 0 ? (uint32_t)diff : 0u; pred[1] += c == 1 ? (uint32_t)diff : 0u; pred[2] += c == 2 ? (uint32_t)diff : 0u;
    const int32_t v = (int32_t)(c == 0 ? pred[0] : c == 1 ? pred[1] : pred[2]);
    if (v < -32768 || v > 32767) note(cur, kStDCRange);
    if (blk) blk[0] = (int16_t)v;
  }
  ES_JPEG_HD inline void ac(uint32_t k, int val) {
    if (blk) blk[natural[k & 63u] & 63u] = (int16_t)val;
  }
  ES_JPEG_HD inline void defect(int status, bool at_dc) { note(at_dc ? next : cur, status); }
};
// S and J of a segment of len raw bytes for a workgroup of T decoders: S = max(subseq, ceil(len / T)), J = ceil(len / S) <= T
ES_JPEG_HD inline uint32_t subsequence_bytes(uint32_t len, uint32_t subseq, uint32_t T) {
  const uint32_t per = (len + T - 1) / T;
  return subseq > per ? subseq : per;
}
// the guessed entry of subsequence j > 0 before the first round: a DC symbol of the MCU's first block at its first data byte
ES_JPEG_HD inline ScanState guessed_entry(const uint8_t* p, uint32_t len, uint32_t at) { return ScanState{next_data(p, len, at) * 8u, 0u}; }
// what the last decoder adds after the write pass: a block left unfinished at the segment's end, or fewer blocks than expected
ES_JPEG_HD inline void close_segment(WriteSink& w, const ScanState& exit) {
  if (exit.pos != kDeadPos && (exit.bk & 255u) != 0u && w.cur != ~0u) w.note(w.cur, kStTruncated);
  if (w.next < w.expected) w.note(w.next, kStTruncated);
}

// the marker that follows position pos, as next_marker; *ff: the first FF of the run that opens it (where the bit reader stops)
inline int next_marker_at(const uint8_t* p, size_t n, size_t& pos, size_t* ff) {
  for (;;) {
    if (pos >= n) { *ff = n; return -1; }
    if (p[pos] != 0xFF) { ++pos; continue; }
    size_t q = pos + 1;
    while (q < n && p[q] == 0xFF) ++q;
    if (q >= n) { *ff = pos; return -1; }
    if (p[q] != 0) { *ff = pos; pos = q + 1; return p[q]; }
    pos = q + 1;
  }
}
// The host preparation: one walk over the scan that finds the segments and checks what the serial decoder checks around them (RSTn
// present and numbered, EOI after the last segment); no Huffman decoding.  segments: [restart_intervals(H.info)], offsets from p.
inline bool scan_prepare(const uint8_t* p, size_t n, const Header& H, es_jpeg_segment* segments, ScanTables* tables, const char** why) {
  if (n >= kMaxParallelFile) { *why = "a file of 256 MiB or more is not decoded in parallel"; return false; }
  const es_jpeg_info& I = H.info;
  memset(tables, 0, sizeof(*tables));
  tables->components = I.components;
  for (int c = 0; c < I.components; ++c) {
    tables->td[c] = I.td[c]; tables->ta[c] = I.ta[c];
    const Huff* src[2] = {&H.dc[I.td[c]], &H.ac[I.ta[c]]};
    for (int a = 0; a < 2; ++a) {
      HuffFlat& t = tables->t[2 * c + a];
      memcpy(t.look, src[a]->look, sizeof(t.look));
      memcpy(t.maxcode, src[a]->maxcode, sizeof(t.maxcode));
      memcpy(t.valoff, src[a]->valoff, sizeof(t.valoff));
      memcpy(t.vals, src[a]->vals, sizeof(t.vals));
    }
  }
  const uint64_t count = restart_intervals(I);
  size_t pos = H.scan_pos;
  for (uint64_t k = 0; k < count; ++k) {
    const size_t begin = pos;
    size_t ff = n;
    const int m = next_marker_at(p, n, pos, &ff);
    segments[k].begin = (uint32_t)begin;
    segments[k].end = (uint32_t)ff;
    if (k + 1 < count) {
      if (m != 0xD0 + (int)(k & 7)) { *why = m < 0 ? "truncated: the file ends where an RSTn marker must stand" : "a missing or misnumbered RSTn marker"; return false; }
    } else {
      if (m < 0) { *why = "truncated: no EOI marker after the scan"; return false; }
      if (m != 0xD9) { *why = "multi-scan files are not supported (a segment follows the scan)"; return false; }
    }
  }
  return true;
}

// The twin of csrc/jpeg_entropy.hip: the same rounds over the same states, `threads` standing for the workgroup's size, run one
// decoder after the other.  coeffs: [coeff_count(I)], every value written.  Returns the status (kSt*); *rounds receives the largest
// number of synchronise rounds a segment took.  p / n: the bytes the segments' offsets refer to.
inline int entropy_decode_parallel(const uint8_t* p, size_t n, const es_jpeg_info& I, const es_jpeg_segment* segments, const ScanTables& T,
                                   uint32_t subseq, uint32_t threads, int16_t* coeffs, uint32_t* rounds) {
  memset(coeffs, 0, coeff_count(I) * sizeof(int16_t));
  const ScanGeom G = scan_geom(I);
  const uint32_t count = (uint32_t)restart_intervals(I);
  if (n >= kMaxParallelFile) n = kMaxParallelFile - 1;
  if (subseq == 0) subseq = kDefaultSubseq;
  *rounds = 0;
  int status = kStOk;
  std::vector<ScanState> in, prop;
  std::vector<CountSink> cnt;
  std::vector<uint8_t> dirty;
  for (uint32_t seg = 0; seg < count; ++seg) {
    uint32_t end = segments[seg].end < n ? segments[seg].end : (uint32_t)n;
    uint32_t begin = segments[seg].begin < end ? segments[seg].begin : end;
    const uint8_t* s = p + begin;
    const uint32_t len = end - begin;
    const uint32_t S = subsequence_bytes(len, subseq, threads), J = len ? (len + S - 1) / S : 0;
    const uint32_t expected = segment_blocks(G, seg);
    uint32_t err = ~0u;
    in.assign(J, dead_state()); prop.assign(J + 1, dead_state()); cnt.resize(J); dirty.assign(J, 1);
    for (uint32_t j = 0; j < J; ++j) prop[j] = in[j] = guessed_entry(s, len, j * S);
    uint32_t r = 0;
    for (bool changed = J > 0; changed && r <= J;) {
      for (uint32_t j = 0; j < J; ++j)
        if (dirty[j]) {                             // a dead entry (the neighbour met an impossible code): propose from the own guess again
          const bool dead = in[j].pos == kDeadPos;
          cnt[j].clear();
          prop[j + 1] = decode_subsequence(T, G, s, len, dead ? guessed_entry(s, len, j * S) : in[j], (j + 1) * S, cnt[j]);
          if (dead) cnt[j].clear();                 // (what follows a dead entry is dropped by the write pass)
        }
      changed = false;
      for (uint32_t j = 1; j < J; ++j) {
        dirty[j] = !same_state(prop[j], in[j]);
        in[j] = prop[j];
        changed = changed || dirty[j];
      }
      if (J) dirty[0] = 0;
      ++r;
    }
    if (r > *rounds) *rounds = r;
    // Behind the first dead entry nothing is a true state (the decoder after it proposed from a guess): all of it is dead in the write pass
    bool cut = false;
    for (uint32_t j = 0; j < J; ++j) {
      cut = cut || in[j].pos == kDeadPos;
      if (cut) { in[j] = dead_state(); cnt[j].clear(); }
    }
    uint32_t ord = 0, pred[3] = {0, 0, 0};
    WriteSink w;
    for (uint32_t j = 0; j < J; ++j) {
      w = WriteSink{&G, kNatural, coeffs, seg, expected, ord, ~0u, {pred[0], pred[1], pred[2]}, ~0u, nullptr};
      if ((in[j].bk & 255u) != 0u && in[j].pos != kDeadPos && ord > 0) w.enter(ord - 1);
      const ScanState exit = decode_subsequence(T, G, s, len, in[j], (j + 1) * S, w);
      if (j + 1 == J) close_segment(w, exit);
      if (w.err < err) err = w.err;
      ord += cnt[j].dcs;
      for (int c = 0; c < 3; ++c) pred[c] += cnt[j].sum[c];
    }
    if (J == 0) err = kStTruncated;               // an empty segment: block 0 is missing
    if (err != ~0u && status == kStOk) status = (int)(err & 7u);      // segments in order: the first defect by (segment, block)
  }
  return status;
}

// ---- the host twin of the two kernels -------------------------------------------------------------------------------------------------
inline void idct_block(const int16_t* coef, const uint16_t* q, uint8_t* out, size_t stride) {
  uint32_t ws[64], in[8], o[8];
  for (int x = 0; x < 8; ++x) {
    for (int k = 0; k < 8; ++k) in[k] = dequant(coef[8 * k + x], q[8 * k + x]);
    idct_1d(in, o);
    for (int k = 0; k < 8; ++k) ws[8 * k + x] = descale_column(o[k]);
  }
  for (int y = 0; y < 8; ++y) {
    idct_1d(ws + 8 * y, o);
    for (int k = 0; k < 8; ++k) out[y * stride + k] = descale_sample(o[k]);
  }
}
// out: height rows of row_stride bytes, width * 3 of each written
inline void reconstruct(const es_jpeg_info& I, const int16_t* coeffs, const uint16_t* qtables, uint8_t* out, size_t row_stride) {
  std::vector<uint8_t> plane[3];
  size_t stride[3] = {0, 0, 0};
  const int16_t* src = coeffs;
  for (int c = 0; c < I.components; ++c) {
    stride[c] = (size_t)I.blocks_w[c] * 8;
    plane[c].resize(stride[c] * I.blocks_h[c] * 8);
    for (int by = 0; by < I.blocks_h[c]; ++by)
      for (int bx = 0; bx < I.blocks_w[c]; ++bx, src += 64)
        idct_block(src, qtables + 64 * c, plane[c].data() + (size_t)by * 8 * stride[c] + (size_t)bx * 8, stride[c]);
  }
  const int mode = up_mode(I.hmax, I.vmax);
  const int dw = I.components == 3 ? comp_w(I, 1) : 0, dh = I.components == 3 ? comp_h(I, 1) : 0;
  for (int y = 0; y < I.height; ++y) {
    uint8_t* dst = out + (size_t)y * row_stride;
    const uint8_t* luma = plane[0].data() + (size_t)y * stride[0];
    for (int x = 0; x < I.width; ++x, dst += 3) {
      if (I.components == 1) { dst[0] = dst[1] = dst[2] = luma[x]; continue; }
      ycc_to_rgb(luma[x], upsampled(plane[1].data(), stride[1], dw, dh, mode, x, y), upsampled(plane[2].data(), stride[2], dw, dh, mode, x, y), dst);
    }
  }
}

// =====================================================================================================================================
// The encoder: RGB (or gray) bytes -> the file Pillow's Image.save(f, "JPEG", quality=, subsampling=[, restart_marker_blocks=]) writes,
// byte for byte (libjpeg's defaults: JFIF 1.01, the Annex K tables scaled by the quality, "islow" forward DCT, h2v1 / h2v2 box
// downsampling with the alternating bias, the standard Huffman tables, one interleaved scan).  As above, the per-sample and per-block
// rules are ES_JPEG_HD functions that csrc/jpeg_encode.hip's kernels and the host twin both call; the tables they read are one constexpr
// value (kEnc here, a __constant__ copy of it on the device) passed by reference.
// =====================================================================================================================================
struct HuffEnc { uint32_t e[256]; };              // symbol -> code length << 16 | code, 0: the table has no such symbol
struct EncConst {
  uint8_t base_q[2][64];                          // Annex K.1 / K.2, natural order
  uint8_t dc_bits[2][16], dc_vals[2][12];         // Annex K.3: codes per length, symbols in code order
  uint8_t ac_bits[2][16], ac_vals[2][162];
  uint8_t zigzag[64];                             // scan position -> natural index (kNatural)
  HuffEnc dc[2], ac[2];
};
constexpr uint8_t kBaseLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                   69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                                   81, 104, 113, 92, 49, 64, 78,  87,  103, 121, 120, 101, 72, 92,  95,  98,  112, 100, 103, 99};
constexpr uint8_t kBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                     99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// canonical codes (Annex C): the codes of one length are consecutive, the first of the next length is (last + 1) << 1
constexpr void fill_huff_enc(HuffEnc& t, const uint8_t bits[16], const uint8_t* vals) {
  uint32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code) t.e[vals[k]] = (uint32_t)l << 16 | code;
    code <<= 1;
  }
}
constexpr EncConst make_enc_const() {
  EncConst T{};
  for (int i = 0; i < 64; ++i) { T.base_q[0][i] = kBaseLuma[i]; T.base_q[1][i] = kBaseChroma[i]; T.zigzag[i] = kZigzag[i]; }
  for (int t = 0; t < 2; ++t) {
    for (int i = 0; i < 16; ++i) { T.dc_bits[t][i] = kDcBits[t][i]; T.ac_bits[t][i] = kAcBits[t][i]; }
    for (int i = 0; i < 12; ++i) T.dc_vals[t][i] = (uint8_t)i;
    for (int i = 0; i < 162; ++i) T.ac_vals[t][i] = kAcVals[t][i];
    fill_huff_enc(T.dc[t], T.dc_bits[t], T.dc_vals[t]);
    fill_huff_enc(T.ac[t], T.ac_bits[t], T.ac_vals[t]);
  }
  return T;
}
constexpr EncConst kEnc = make_enc_const();

// ---- the shared integer rules of the encoder -----------------------------------------------------------------------------------------
// jcparam.c: jpeg_quality_scaling and jpeg_add_quant_table with force_baseline
ES_JPEG_HD inline int quant_entry(int base, int quality) {
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  const int v = (base * scale + 50) / 100;
  return v < 1 ? 1 : v > 255 ? 255 : v;
}
// q: natural order; which: 0 luma, 1 chroma
ES_JPEG_HD inline void quality_table(const EncConst& T, int which, int quality, uint16_t q[64]) {
  for (int i = 0; i < 64; ++i) q[i] = (uint16_t)quant_entry(T.base_q[which][i], quality);
}
// jccolor.c, 16-bit fixed point; component c of one pixel
ES_JPEG_HD inline int rgb_to_ycc(int r, int g, int b, int c) {
  if (c == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  if (c == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}
ES_JPEG_HD inline int pixel_component(const uint8_t* img, size_t stride, int channels, int c, int x, int y) {
  const uint8_t* p = img + (size_t)y * stride + (size_t)x * channels;
  return channels == 1 ? p[0] : rgb_to_ycc(p[0], p[1], p[2], c);
}
// Sample (x, y) of component c's (downsampled) plane, for any x, y >= 0 inside the component's own blocks.  mode: kUpNone for luma and
// for 4:4:4 chroma.  Edges as libjpeg pads them: columns and rows are replicated at FULL resolution (rows only up to a multiple of the
// vertical factor), then the plane is downsampled, then ITS last row (dh - 1) is replicated down to whole blocks - so a row below the
// last real chroma row repeats that row's average of two source rows, not the last source row alone.
ES_JPEG_HD inline int enc_sample(const uint8_t* img, size_t stride, int channels, int W, int H, int c, int mode, int dh, int x, int y) {
  if (mode == kUpNone) return pixel_component(img, stride, channels, c, x < W ? x : W - 1, y < H ? y : H - 1);
  const int x0 = 2 * x < W ? 2 * x : W - 1, x1 = 2 * x + 1 < W ? 2 * x + 1 : W - 1;
  if (mode == kUpH2V1) {
    const int yy = y < H ? y : H - 1;
    return (pixel_component(img, stride, channels, c, x0, yy) + pixel_component(img, stride, channels, c, x1, yy) + (x & 1)) >> 1;
  }
  const int cy = y < dh ? y : dh - 1;
  const int y0 = 2 * cy < H ? 2 * cy : H - 1, y1 = 2 * cy + 1 < H ? 2 * cy + 1 : H - 1;
  return (pixel_component(img, stride, channels, c, x0, y0) + pixel_component(img, stride, channels, c, x1, y0) +
          pixel_component(img, stride, channels, c, x0, y1) + pixel_component(img, stride, channels, c, x1, y1) + 1 + (x & 1)) >> 2;
}
// One 8-point pass of jfdctint.c (CONST_BITS 13, PASS1_BITS 2).  first pass (rows): on sample - 128, outputs scaled by 4; second pass
// (columns): the outputs are 8 x the DCT.
ES_JPEG_HD inline int32_t fdescale(int32_t x, int n) { return (x + (1 << (n - 1))) >> n; }
ES_JPEG_HD inline void fdct_1d(const int32_t d[8], int32_t o[8], bool second) {
  const int32_t t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int32_t t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  const int n = second ? 15 : 11;
  o[0] = second ? fdescale(t10 + t11, 2) : (t10 + t11) * 4;
  o[4] = second ? fdescale(t10 - t11, 2) : (t10 - t11) * 4;
  int32_t z1 = (t12 + t13) * 4433;
  o[2] = fdescale(z1 + t13 * 6270, n);
  o[6] = fdescale(z1 - t12 * 15137, n);
  z1 = t4 + t7;
  int32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int32_t z5 = (z3 + z4) * 9633;
  const int32_t a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
  z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
  z3 += z5; z4 += z5;
  o[7] = fdescale(a4 + z1 + z3, n);
  o[5] = fdescale(a5 + z2 + z4, n);
  o[3] = fdescale(a6 + z2 + z3, n);
  o[1] = fdescale(a7 + z1 + z4, n);
}
// jcdctmgr.c: the DCT output carries a factor 8, so the divisor is 8 q; round half away from zero
ES_JPEG_HD inline int16_t quantise(int32_t c, uint16_t q) {
  const int32_t d = 8 * (int32_t)q, a = c < 0 ? -c : c, v = (a + d / 2) / d;
  return (int16_t)(c < 0 ? -v : v);
}
// jccoefct.c's dummy blocks.  (bx, by): a block of the MCU-padded grid of a component with rbw x rbh real blocks and h blocks per MCU
// row.  -> the REAL block whose DC it carries ((bx, by) itself for a real block); true for a dummy block, whose AC is all zero.
// Right of the last real block: the DC of the block to its left.  Below the last real block row: the DC of the previous block in MCU
// order, which is the last block of the row above within the MCU - itself possibly a dummy, hence the clamp.
ES_JPEG_HD inline bool dummy_source(int bx, int by, int rbw, int rbh, int h, int* sx, int* sy) {
  *sx = bx; *sy = by;
  if (bx < rbw && by < rbh) return false;
  if (by >= rbh) { *sy = rbh - 1; *sx = (bx / h) * h + h - 1; }
  else *sx = bx - 1;
  if (*sx > rbw - 1) *sx = rbw - 1;
  return true;
}
// real blocks of component c: its own ceil(samples / 8)
ES_JPEG_HD inline int real_blocks_w(const es_jpeg_info& I, int c) { return ceil_div(comp_w(I, c), 8); }
ES_JPEG_HD inline int real_blocks_h(const es_jpeg_info& I, int c) { return ceil_div(comp_h(I, c), 8); }

// All a block of the padded grid needs, by value (what a kernel gets as its argument)
struct EncGeom {
  int32_t width, height, channels, components, mode;   // mode: the chroma planes' downsampling (kUp*)
  int32_t h, v;                                         // luma blocks per MCU
  int32_t mcus_x, mcus_y;
  int32_t blocks_w[3], rbw[3], rbh[3], dh;              // padded and real block grids, real chroma rows
  uint32_t nblk[3];                                     // blocks per component (padded)
  int32_t restart_interval;
};
inline EncGeom enc_geom(const es_jpeg_info& I, int channels) {
  EncGeom G;
  memset(&G, 0, sizeof(G));
  G.width = I.width; G.height = I.height; G.channels = channels; G.components = I.components;
  G.mode = I.components == 3 ? up_mode(I.hmax, I.vmax) : kUpNone;
  G.h = I.h[0]; G.v = I.v[0];
  G.mcus_x = I.mcus_x; G.mcus_y = I.mcus_y;
  for (int c = 0; c < I.components; ++c) {
    G.blocks_w[c] = I.blocks_w[c];
    G.rbw[c] = real_blocks_w(I, c); G.rbh[c] = real_blocks_h(I, c);
    G.nblk[c] = (uint32_t)component_blocks(I, c);
  }
  G.dh = I.components == 3 ? comp_h(I, 1) : 0;
  G.restart_interval = I.restart_interval;
  return G;
}
// Row j of block (bx, by) of component c, before the DCT: sample - 128 of the block's source (dummy_source)
ES_JPEG_HD inline void gather_row(const EncGeom& G, const uint8_t* img, size_t stride, int c, int sx, int sy, int j, int32_t row[8]) {
  const int mode = c == 0 ? (int)kUpNone : G.mode;
  for (int k = 0; k < 8; ++k) row[k] = enc_sample(img, stride, G.channels, G.width, G.height, c, mode, G.dh, sx * 8 + k, sy * 8 + j) - 128;
}

// ---- the scan's geometry: block s of the scan (MCU after MCU, inside one luma row by row, then Cb, then Cr) -------------------------------
struct ScanBlock {
  int c;                                          // component
  uint32_t block;                                 // its number in the coefficient buffer (all components, 64 values each)
  uint32_t pred;                                  // the block whose DC is the predictor, ~0u: the predictor is 0
  bool boundary;                                  // the first block after a restart marker
};
ES_JPEG_HD inline uint32_t blocks_per_mcu(const EncGeom& G) { return G.components == 1 ? 1u : (uint32_t)(G.h * G.v + 2); }
ES_JPEG_HD inline ScanBlock scan_block(const EncGeom& G, uint32_t s) {
  const uint32_t bpm = blocks_per_mcu(G), luma = (uint32_t)(G.h * G.v);
  const uint32_t m = s / bpm, k = s - m * bpm;
  const uint32_t my = m / (uint32_t)G.mcus_x, mx = m - my * (uint32_t)G.mcus_x;
  const bool first = G.restart_interval > 0 ? m % (uint32_t)G.restart_interval == 0 : m == 0;     // no predecessor in this interval
  ScanBlock b;
  b.boundary = first && m > 0 && k == 0;
  if (k < luma) {
    const uint32_t vy = k / (uint32_t)G.h, hx = k - vy * (uint32_t)G.h;
    b.c = 0;
    b.block = (my * G.v + vy) * (uint32_t)G.blocks_w[0] + mx * G.h + hx;
    if (k > 0) {
      const uint32_t pv = (k - 1) / (uint32_t)G.h, ph = (k - 1) - pv * (uint32_t)G.h;
      b.pred = (my * G.v + pv) * (uint32_t)G.blocks_w[0] + mx * G.h + ph;
    } else if (first) b.pred = ~0u;
    else {
      const uint32_t pm = m - 1, py = pm / (uint32_t)G.mcus_x, px = pm - py * (uint32_t)G.mcus_x;
      b.pred = (py * G.v + G.v - 1) * (uint32_t)G.blocks_w[0] + px * G.h + G.h - 1;
    }
  } else {
    b.c = (int)(k - luma) + 1;
    const uint32_t base = G.nblk[0] + (b.c == 2 ? G.nblk[1] : 0u);
    b.block = base + my * (uint32_t)G.blocks_w[b.c] + mx;
    b.pred = first ? ~0u : b.block - 1;           // chroma has one block per MCU and rows of mcus_x blocks: the previous MCU's is the previous block
  }
  return b;
}

// ---- the block coder (jchuff.c with the standard tables) ------------------------------------------------------------------------------
ES_JPEG_HD inline int bit_length(uint32_t v) {
  int n = 0;
  while (v) { ++n; v >>= 1; }
  return n;
}
// Codes one block into a sink with put(bits, count) (count <= 16) and bad().  blk: natural order; t: 0 luma, 1 chroma tables.  A DC
// difference above category 11 or an AC value above category 10 has no code in a baseline file: the sink is told (bad) and the value
// is coded as if cut to the largest category, so that the bits written are bounded for ANY int16 input:
// kMaxBlockBits = 11 + 11 + 63 * (16 + 10).
constexpr uint32_t kMaxBlockBits = 11 + 11 + 63 * (16 + 10);
template <class Sink>
ES_JPEG_HD inline void code_block(const EncConst& T, int t, const int16_t* blk, int pred, Sink& s) {
  int diff = (int)blk[0] - pred;
  uint32_t mag = (uint32_t)(diff < 0 ? -diff : diff);
  int nb = bit_length(mag);
  if (nb > 11) { s.bad(); nb = 11; }
  uint32_t e = T.dc[t].e[nb];
  s.put(e & 0xffffu, (int)(e >> 16));
  if (nb) s.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1u), nb);
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = blk[T.zigzag[k]];
    if (v == 0) { ++run; continue; }
    for (; run > 15; run -= 16) { e = T.ac[t].e[0xf0]; s.put(e & 0xffffu, (int)(e >> 16)); }
    mag = (uint32_t)(v < 0 ? -v : v);
    nb = bit_length(mag);
    if (nb > 10) { s.bad(); nb = 10; }
    e = T.ac[t].e[run << 4 | nb];
    s.put(e & 0xffffu, (int)(e >> 16));
    s.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << nb) - 1u), nb);
    run = 0;
  }
  if (run > 0) { e = T.ac[t].e[0]; s.put(e & 0xffffu, (int)(e >> 16)); }
}
struct LengthSink {
  uint32_t bits = 0;
  bool is_bad = false;
  ES_JPEG_HD inline void put(uint32_t, int n) { bits += (uint32_t)n; }
  ES_JPEG_HD inline void bad() { is_bad = true; }
};

// ---- the header (SOI .. SOS) into a sink with byte(b) -----------------------------------------------------------------------------------
// at most 2 + 18 + 2 * 69 + 19 + 2 * 33 + 2 * 183 + 6 + 14 = 629 bytes
constexpr int kMaxHeaderBytes = 629;
template <class Bytes>
ES_JPEG_HD inline void write_header(const EncConst& T, int width, int height, int components, int h, int v, int quality, int restart_interval,
                                    Bytes& o) {
  const uint8_t app0[18] = {0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  o.byte(0xFF); o.byte(0xD8);
  for (int i = 0; i < 18; ++i) o.byte(app0[i]);
  const int tables = components == 1 ? 1 : 2;
  for (int t = 0; t < tables; ++t) {
    o.byte(0xFF); o.byte(0xDB); o.byte(0); o.byte(67); o.byte((uint8_t)t);
    for (int i = 0; i < 64; ++i) o.byte((uint8_t)quant_entry(T.base_q[t][T.zigzag[i]], quality));
  }
  o.byte(0xFF); o.byte(0xC0); o.byte(0); o.byte((uint8_t)(8 + 3 * components)); o.byte(8);
  o.byte((uint8_t)(height >> 8)); o.byte((uint8_t)height); o.byte((uint8_t)(width >> 8)); o.byte((uint8_t)width);
  o.byte((uint8_t)components);
  for (int c = 0; c < components; ++c) {
    o.byte((uint8_t)(c + 1));
    o.byte((uint8_t)(c == 0 ? (h << 4 | v) : 0x11));
    o.byte((uint8_t)(c == 0 ? 0 : 1));
  }
  for (int t = 0; t < tables; ++t)
    for (int ac = 0; ac < 2; ++ac) {
      const uint8_t* bits = ac ? T.ac_bits[t] : T.dc_bits[t];
      const uint8_t* vals = ac ? T.ac_vals[t] : T.dc_vals[t];
      const int n = ac ? 162 : 12;
      o.byte(0xFF); o.byte(0xC4); o.byte(0); o.byte((uint8_t)(2 + 1 + 16 + n)); o.byte((uint8_t)(ac << 4 | t));
      for (int i = 0; i < 16; ++i) o.byte(bits[i]);
      for (int i = 0; i < n; ++i) o.byte(vals[i]);
    }
  if (restart_interval > 0) {
    o.byte(0xFF); o.byte(0xDD); o.byte(0); o.byte(4); o.byte((uint8_t)(restart_interval >> 8)); o.byte((uint8_t)restart_interval);
  }
  o.byte(0xFF); o.byte(0xDA); o.byte(0); o.byte((uint8_t)(6 + 2 * components)); o.byte((uint8_t)components);
  for (int c = 0; c < components; ++c) { o.byte((uint8_t)(c + 1)); o.byte((uint8_t)(c == 0 ? 0x00 : 0x11)); }
  o.byte(0); o.byte(63); o.byte(0);
}
ES_JPEG_HD inline uint32_t header_bytes(int components, int restart_interval) {
  return (components == 1 ? 2u + 18 + 69 + 13 + 33 + 183 + 10 : 2u + 18 + 2 * 69 + 19 + 2 * 33 + 2 * 183 + 14) + (restart_interval > 0 ? 6u : 0u);
}
// counts every byte, stores those below cap
struct BoundedBytes {
  uint8_t* out;
  size_t cap, n;
  ES_JPEG_HD inline void byte(uint8_t b) {
    if (n < cap) out[n] = b;
    ++n;
  }
};

// ---- parameters, geometry and the size bound ------------------------------------------------------------------------------------------
inline bool encode_geometry(int width, int height, int channels, const es_jpeg_encode_params* P, es_jpeg_info& I, const char** why) {
  if (!P) { *why = "null params"; return false; }
  if (channels == 4) { *why = "cannot write mode RGBA as JPEG"; return false; }
  if (channels != 1 && channels != 3) { *why = "1 or 3 channels expected"; return false; }
  if (P->quality < 1 || P->quality > 100) { *why = "quality outside 1 .. 100"; return false; }
  if (P->restart_interval < 0 || P->restart_interval > 65535) { *why = "restart interval outside 0 .. 65535"; return false; }
  if (channels == 3 && P->subsampling != ES_JPEG_444 && P->subsampling != ES_JPEG_422 && P->subsampling != ES_JPEG_420) {
    *why = "unknown subsampling (ES_JPEG_444, ES_JPEG_422 or ES_JPEG_420)";
    return false;
  }
  memset(&I, 0, sizeof(I));
  I.width = width; I.height = height; I.components = channels;
  for (int c = 0; c < channels; ++c) { I.h[c] = I.v[c] = 1; I.tq[c] = I.td[c] = I.ta[c] = c ? 1 : 0; }
  if (channels == 3) {
    I.h[0] = P->subsampling == ES_JPEG_444 ? 1 : 2;
    I.v[0] = P->subsampling == ES_JPEG_420 ? 2 : 1;
  }
  I.restart_interval = P->restart_interval;
  return derive_geometry(I, why);
}
// what the encoder takes back as an info: one of encode_geometry's
inline bool encode_info_ok(const es_jpeg_info* info, const es_jpeg_encode_params* P, const char** why) {
  if (!info_ok(info, why)) return false;
  es_jpeg_info I;
  es_jpeg_encode_params Q;
  if (!P) { *why = "null params"; return false; }
  Q = *P;
  Q.subsampling = info->components == 3 ? (info->h[0] == 1 ? ES_JPEG_444 : info->v[0] == 1 ? ES_JPEG_422 : ES_JPEG_420) : ES_JPEG_444;
  if (!encode_geometry(info->width, info->height, info->components, &Q, I, why)) return false;
  if (info->components == 3 && P->subsampling != Q.subsampling) { *why = "the info's sampling is not the params' subsampling"; return false; }
  if (memcmp(&I, info, sizeof(I)) != 0) { *why = "the info is not what es_jpeg_encode_info_host gives for these params"; return false; }
  return true;
}
inline uint64_t restart_intervals(const es_jpeg_info& I) {
  const uint64_t mcus = (uint64_t)I.mcus_x * (uint64_t)I.mcus_y;
  return I.restart_interval > 0 ? (mcus + I.restart_interval - 1) / I.restart_interval : 1;
}
// The bit stream before byte stuffing, restart markers included, is at most this many bytes: a block codes into at most kMaxBlockBits
// (DC: the longest DC code, 11 bits in the chroma table, + 11 value bits; each of the 63 AC values: a 16-bit code + 10 value bits; the
// ZRL and EOB symbols only ever replace longer codes of non-zero values), every interval is padded to a byte (< 1 byte each) and every
// interval but the first is preceded by a 2-byte marker.
inline uint64_t unstuffed_bound(const es_jpeg_info& I) {
  uint64_t blocks = 0;
  for (int c = 0; c < I.components; ++c) blocks += component_blocks(I, c);
  const uint64_t n = restart_intervals(I);
  return (blocks * kMaxBlockBits + 7) / 8 + n + 2 * (n - 1);
}
// The file is at most: the header + twice the data bytes (every data byte may be 0xFF and then takes a stuffed 0x00; counting the
// marker bytes twice as well only loosens the bound) + EOI.
inline uint64_t capacity_bound(const es_jpeg_info& I) { return header_bytes(I.components, I.restart_interval) + 2 * unstuffed_bound(I) + 2; }

// ---- the host encoder ---------------------------------------------------------------------------------------------------------------
// coeffs: [coeff_count(I)], every value written (the decoder's layout, dummy blocks included)
inline void forward_host(const es_jpeg_info& I, int quality, const uint8_t* img, size_t stride, int16_t* coeffs) {
  const EncGeom G = enc_geom(I, I.components);
  uint16_t q[2][64];
  quality_table(kEnc, 0, quality, q[0]);
  quality_table(kEnc, 1, quality, q[1]);
  int16_t* dst = coeffs;
  for (int c = 0; c < I.components; ++c)
    for (int by = 0; by < I.blocks_h[c]; ++by)
      for (int bx = 0; bx < I.blocks_w[c]; ++bx, dst += 64) {
        int sx, sy;
        const bool dummy = dummy_source(bx, by, G.rbw[c], G.rbh[c], I.h[c], &sx, &sy);
        int32_t ws[8][8], col[8], o[8];
        for (int j = 0; j < 8; ++j) {
          int32_t row[8];
          gather_row(G, img, stride, c, sx, sy, j, row);
          fdct_1d(row, ws[j], false);
        }
        for (int x = 0; x < 8; ++x) {
          for (int k = 0; k < 8; ++k) col[k] = ws[k][x];
          fdct_1d(col, o, true);
          for (int k = 0; k < 8; ++k) dst[8 * k + x] = dummy && (k || x) ? (int16_t)0 : quantise(o[k], q[c ? 1 : 0][8 * k + x]);
        }
      }
}
// serial bit writer: MSB first, a 0x00 after every 0xFF
struct StuffedBits {
  BoundedBytes& o;
  uint64_t acc = 0;
  int cnt = 0;
  bool is_bad = false;
  explicit StuffedBits(BoundedBytes& o_) : o(o_) {}
  inline void put(uint32_t bits, int n) {
    acc = acc << n | bits;
    cnt += n;
    while (cnt >= 8) {
      const uint8_t b = (uint8_t)(acc >> (cnt - 8));
      o.byte(b);
      if (b == 0xFF) o.byte(0);
      cnt -= 8;
    }
  }
  inline void bad() { is_bad = true; }
  inline void flush() { if (cnt) put((1u << (8 - cnt)) - 1u, 8 - cnt); }
};
// The whole file into out (the bytes below cap are stored); returns its length.  *bad: a coefficient outside the baseline categories.
inline size_t entropy_encode_host(const es_jpeg_info& I, int quality, const int16_t* coeffs, uint8_t* out, size_t cap, bool* bad) {
  BoundedBytes o{out, cap, 0};
  write_header(kEnc, I.width, I.height, I.components, I.h[0], I.v[0], quality, I.restart_interval, o);
  const EncGeom G = enc_geom(I, I.components);
  const uint32_t total = G.nblk[0] + G.nblk[1] + G.nblk[2];
  StuffedBits w(o);
  uint32_t rst = 0;
  for (uint32_t s = 0; s < total; ++s) {
    const ScanBlock b = scan_block(G, s);
    if (b.boundary) {
      w.flush();
      o.byte(0xFF);
      o.byte((uint8_t)(0xD0 + (rst++ & 7)));
    }
    code_block(kEnc, b.c ? 1 : 0, coeffs + (size_t)b.block * 64, b.pred == ~0u ? 0 : coeffs[(size_t)b.pred * 64], w);
  }
  w.flush();
  o.byte(0xFF);
  o.byte(0xD9);
  *bad = w.is_bad;
  return o.n;
}

}  // namespace esjpeg
