// From a segmenter's four mask predictions to the images try_on takes, in plain C++ against the C ABI (include/edgestyle_hip.h)
// and the HIP runtime: no Python, no cv2, no skimage.  One photo and four masks in, five images out - what the reference's
// create_sam_images computes after its networks (extract_dataset.py:394-502): closings, smooth_mask, the largest component of
// the union, the boolean algebra and draw_binary_mask with grey 127, all in es_sam_compose on the device.
//
//   hipcc -O2 -Iinclude examples/mask_host.cpp -Ledgestyle_amd/lib -ledgestyle_hip -Wl,-rpath,$PWD/edgestyle_amd/lib -o mask_host
//   ./mask_host photo.ppm subject.pgm body.pgm clothes.pgm head.pgm out
//
// photo.ppm: binary PPM (P6, maxval 255).  *.pgm: binary PGM (P5, maxval 255) of the photo's size, nonzero = true: the predictions
// of the subject, body ("agnostic"), clothes and head segmenters.  Writes out_subject.ppm, out_mask.ppm, out_agnostic.ppm,
// out_clothes.ppm and out_head.ppm; their pixels are device memory that es_prepare_conds_u8 and es_clip_pick take as they are
// (examples/image_host.cpp, examples/prompt_host.cpp) - this host only downloads them to show them.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "edgestyle_hip.h"

#define HIP_OK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "HIP error at %s:%d\n", __FILE__, __LINE__); return 2; } } while (0)
#define ES_OK(x) do { if ((x) != 0) { fprintf(stderr, "%s: %s\n", #x, es_last_error()); return 3; } } while (0)

// one header token of a PNM file: digits after whitespace and # comments
static bool pnm_int(FILE* f, int* v) {
  int c = fgetc(f);
  while (c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '#') {
    if (c == '#') while (c != '\n' && c != EOF) c = fgetc(f);
    c = fgetc(f);
  }
  if (c < '0' || c > '9') return false;
  long n = 0;
  while (c >= '0' && c <= '9') { n = n * 10 + (c - '0'); if (n > (1 << 24)) return false; c = fgetc(f); }
  *v = (int)n;
  return c == ' ' || c == '\t' || c == '\n' || c == '\r';      // exactly one whitespace byte ends the header
}
// kind '6': PPM, 3 bytes per pixel; kind '5': PGM, 1 byte per pixel
static bool read_pnm(const char* path, char kind, std::vector<uint8_t>& px, int* H, int* W) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); return false; }
  int maxval = 0;
  bool ok = fgetc(f) == 'P' && fgetc(f) == kind && pnm_int(f, W) && pnm_int(f, H) && pnm_int(f, &maxval) && maxval == 255 && *H > 0 && *W > 0;
  if (ok) {
    px.resize((size_t)*H * *W * (kind == '6' ? 3 : 1));
    ok = fread(px.data(), 1, px.size(), f) == px.size();
  }
  fclose(f);
  if (!ok) fprintf(stderr, "%s: not a binary P%c file with maxval 255\n", path, kind);
  return ok;
}

int main(int argc, char** argv) {
  if (argc != 7) { fprintf(stderr, "usage: %s photo.ppm subject.pgm body.pgm clothes.pgm head.pgm out\n", argv[0]); return 1; }
  std::vector<uint8_t> photo, mask[4];
  int H = 0, W = 0;
  if (!read_pnm(argv[1], '6', photo, &H, &W)) return 1;
  for (int k = 0; k < 4; ++k) {
    int h = 0, w = 0;
    if (!read_pnm(argv[2 + k], '5', mask[k], &h, &w)) return 1;
    if (h != H || w != W) { fprintf(stderr, "%s: %d x %d, the photo is %d x %d\n", argv[2 + k], w, h, W, H); return 1; }
  }
  const size_t HW = (size_t)H * W, need = es_mask_workspace_bytes(H, W, 1);
  if (!need) { fprintf(stderr, "%s\n", es_last_error()); return 3; }
  uint8_t *d_photo = nullptr, *d_mask[4] = {}, *d_images = nullptr;
  void* d_ws = nullptr;
  HIP_OK(hipMalloc((void**)&d_photo, HW * 3));
  HIP_OK(hipMemcpy(d_photo, photo.data(), HW * 3, hipMemcpyHostToDevice));
  for (int k = 0; k < 4; ++k) {
    HIP_OK(hipMalloc((void**)&d_mask[k], HW));
    HIP_OK(hipMemcpy(d_mask[k], mask[k].data(), HW, hipMemcpyHostToDevice));
  }
  HIP_OK(hipMalloc((void**)&d_images, 5 * HW * 3));
  HIP_OK(hipMalloc(&d_ws, need));
  const es_image_u8 img = {d_photo, H, W, 3, (int64_t)W * 3};
  ES_OK(es_sam_compose(&img, d_mask[0], d_mask[1], d_mask[2], d_mask[3], 1, H, W, nullptr, d_images, d_ws, need, nullptr));
  HIP_OK(hipDeviceSynchronize());
  std::vector<uint8_t> images(5 * HW * 3);
  HIP_OK(hipMemcpy(images.data(), d_images, images.size(), hipMemcpyDeviceToHost));
  static const char* const names[5] = {"subject", "mask", "agnostic", "clothes", "head"};
  for (int k = 0; k < 5; ++k) {
    const std::string path = std::string(argv[6]) + "_" + names[k] + ".ppm";
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { perror(path.c_str()); return 1; }
    fprintf(f, "P6\n%d %d\n255\n", W, H);
    const bool ok = fwrite(images.data() + (size_t)k * HW * 3, 1, HW * 3, f) == HW * 3;
    if (fclose(f) != 0 || !ok) { perror(path.c_str()); return 1; }
  }
  (void)hipFree(d_ws); (void)hipFree(d_images); (void)hipFree(d_photo);
  for (int k = 0; k < 4; ++k) (void)hipFree(d_mask[k]);
  return 0;
}
