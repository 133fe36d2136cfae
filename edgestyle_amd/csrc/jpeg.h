// Baseline JPEG, the host half and the shared integer rules (include/edgestyle_hip.h states format, limits and arithmetic in full):
// the marker parser and the Huffman decoder - serial by nature, plain C++ - and, behind ES_JPEG_HD, the per-sample rules that
// csrc/jpeg.hip's kernels and the host twin both run: the 1-D pass of the "islow" inverse DCT, its two descalings, libjpeg's triangle
// chroma upsampling and YCbCr -> RGB.  Everything is integer arithmetic.  Any C++17 compiler can compile this header alone
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

}  // namespace esjpeg
