// From RGB (or gray) bytes to a JPEG file, in plain C++ against the C ABI (include/edgestyle_hip.h) and the HIP runtime: no Python, no
// Pillow, no libjpeg.  What the reference does with Image.fromarray(a).save(path, "JPEG") on the host: es_jpeg_encode_u8 - colour
// conversion, downsampling, forward DCT, Huffman coding, byte stuffing, header and EOI all on the device - with Pillow's bytes as the
// result.  The pixels are uploaded here only because this host reads them from a file: es_vae_decode_u8 leaves them on the device.
//
//   hipcc -O2 -Iinclude examples/jpeg_encode_host.cpp -Ledgestyle_amd/lib -ledgestyle_hip -Wl,-rpath,$PWD/edgestyle_amd/lib -o jpeg_encode_host
//   ./jpeg_encode_host in.ppm out.jpg [-q quality] [-s 444|422|420] [-r restart_interval]
//
// in: a binary PPM (P6) or PGM (P5) with maxval 255.  Defaults are Pillow's: quality 75, 4:2:0, no restart markers.  What the encoder
// refuses ends the program with status 3 and the reason.
//
// Built with -DJPEG_HOST_DRY the program is the encoder's host twin alone, from edgestyle_amd/csrc/jpeg.h: no library, no HIP, no GPU (and
// so a program a host sanitizer can check):
//   c++ -std=c++17 -DJPEG_HOST_DRY -Iedgestyle_amd/csrc examples/jpeg_encode_host.cpp -o jpeg_encode_host_dry
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#ifdef JPEG_HOST_DRY
#include "jpeg.h"
#else
#include <hip/hip_runtime.h>
#include "edgestyle_hip.h"
#define HIP_OK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "HIP error at %s:%d\n", __FILE__, __LINE__); return 2; } } while (0)
#define ES_OK(x) do { if ((x) != 0) { fprintf(stderr, "%s: %s\n", #x, es_last_error()); return 3; } } while (0)
#endif

// one header token of a PNM file: comments ('#' to the end of the line) and white space skipped
static bool pnm_int(FILE* f, int* v) {
  int c = fgetc(f);
  while (c == '#' || c == ' ' || c == '\t' || c == '\r' || c == '\n') {
    if (c == '#')
      while (c != '\n' && c != EOF) c = fgetc(f);
    else c = fgetc(f);
  }
  if (c < '0' || c > '9') return false;
  long n = 0;
  for (; c >= '0' && c <= '9'; c = fgetc(f))
    if ((n = n * 10 + (c - '0')) > 65535) return false;
  *v = (int)n;                                    // (the character after the token is the single white space the format asks for)
  return true;
}
static bool read_pnm(const char* path, std::vector<uint8_t>& px, int* W, int* H, int* channels) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); return false; }
  bool ok = fgetc(f) == 'P';
  const int kind = fgetc(f);
  int maxval = 0;
  ok = ok && (kind == '5' || kind == '6') && pnm_int(f, W) && pnm_int(f, H) && pnm_int(f, &maxval) && maxval == 255 && *W > 0 && *H > 0;
  if (ok) {
    *channels = kind == '6' ? 3 : 1;
    px.resize((size_t)*W * *H * *channels);
    ok = fread(px.data(), 1, px.size(), f) == px.size();
  }
  fclose(f);
  if (!ok) fprintf(stderr, "%s: not a binary PPM / PGM with maxval 255 and sides of 1 .. 65535\n", path);
  return ok;
}
static bool write_file(const char* path, const uint8_t* p, size_t n) {
  FILE* f = fopen(path, "wb");
  if (!f) { perror(path); return false; }
  const bool ok = fwrite(p, 1, n, f) == n;
  if (fclose(f) != 0 || !ok) { perror(path); return false; }
  return true;
}

int main(int argc, char** argv) {
  es_jpeg_encode_params params = {75, ES_JPEG_420, 0};
  const char* paths[2] = {nullptr, nullptr};
  int npaths = 0;
  for (int i = 1; i < argc; ++i) {
    const bool opt = argv[i][0] == '-' && argv[i][1] && !argv[i][2] && i + 1 < argc;
    if (opt && argv[i][1] == 'q') params.quality = atoi(argv[++i]);
    else if (opt && argv[i][1] == 'r') params.restart_interval = atoi(argv[++i]);
    else if (opt && argv[i][1] == 's') {
      const char* s = argv[++i];
      params.subsampling = !strcmp(s, "444") ? ES_JPEG_444 : !strcmp(s, "422") ? ES_JPEG_422 : !strcmp(s, "420") ? ES_JPEG_420 : -1;
    } else if (npaths < 2 && argv[i][0] != '-') paths[npaths++] = argv[i];
    else npaths = 3;
  }
  if (npaths != 2) { fprintf(stderr, "usage: %s in.ppm|in.pgm out.jpg [-q quality] [-s 444|422|420] [-r restart_interval]\n", argv[0]); return 1; }
  std::vector<uint8_t> px, file;
  int W = 0, H = 0, channels = 0;
  if (!read_pnm(paths[0], px, &W, &H, &channels)) return 1;
  es_jpeg_info info;
  size_t length = 0;
#ifdef JPEG_HOST_DRY
  const char* why = nullptr;
  if (!esjpeg::encode_geometry(W, H, channels, &params, info, &why)) { fprintf(stderr, "%s: %s\n", paths[0], why); return 3; }
  std::vector<int16_t> coeffs(esjpeg::coeff_count(info));
  esjpeg::forward_host(info, params.quality, px.data(), (size_t)W * channels, coeffs.data());
  file.resize((size_t)esjpeg::capacity_bound(info));
  bool bad = false;
  length = esjpeg::entropy_encode_host(info, params.quality, coeffs.data(), file.data(), file.size(), &bad);
  if (bad || length > file.size()) { fprintf(stderr, "%s: the encoder broke its own bounds\n", paths[0]); return 3; }
#else
  ES_OK(es_jpeg_encode_info_host(W, H, channels, &params, &info));
  const size_t capacity = es_jpeg_encode_capacity(&info, &params), need = es_jpeg_encode_workspace_bytes(&info, 1, &params);
  if (!capacity || !need) { fprintf(stderr, "%s\n", es_last_error()); return 3; }
  uint8_t *d_px = nullptr, *d_out = nullptr;
  uint32_t* d_len = nullptr;
  void* d_ws = nullptr;
  HIP_OK(hipMalloc((void**)&d_px, px.size()));
  HIP_OK(hipMalloc((void**)&d_out, capacity));
  HIP_OK(hipMalloc((void**)&d_len, sizeof(uint32_t)));
  HIP_OK(hipMalloc(&d_ws, need));
  HIP_OK(hipMemcpy(d_px, px.data(), px.size(), hipMemcpyHostToDevice));
  const es_image_u8 image = {d_px, H, W, channels, (int64_t)W * channels};
  uint8_t* outs[1] = {d_out};
  ES_OK(es_jpeg_encode_u8(&image, 1, &params, outs, &capacity, d_len, d_ws, need, nullptr));
  uint32_t n32 = 0;
  HIP_OK(hipMemcpy(&n32, d_len, sizeof(n32), hipMemcpyDeviceToHost));       // (waits for the stream)
  length = n32;
  if (length > capacity) { fprintf(stderr, "the file needs %zu bytes, more than its bound %zu\n", length, capacity); return 3; }
  file.resize(length);
  HIP_OK(hipMemcpy(file.data(), d_out, length, hipMemcpyDeviceToHost));     // what crosses the bus: the finished file
  (void)hipFree(d_ws); (void)hipFree(d_len); (void)hipFree(d_out); (void)hipFree(d_px);
#endif
  if (!write_file(paths[1], file.data(), length)) return 1;
  printf("%s: %d x %d, %d component%s, sampling %dx%d, quality %d, restart interval %d -> %zu bytes\n", paths[1], info.width, info.height,
         info.components, info.components == 1 ? "" : "s", info.hmax, info.vmax, params.quality, info.restart_interval, length);
  return 0;
}
