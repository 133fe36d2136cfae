// From a JPEG file to RGB bytes, in plain C++ against the C ABI (include/edgestyle_hip.h) and the HIP runtime: no Python, no Pillow, no
// libjpeg.  What the reference does with Image.open(path).convert("RGB") on the host: es_jpeg_decode_u8 - headers and Huffman decoding on
// this thread, inverse DCT, chroma upsampling and colour conversion on the device - with Pillow's bytes as the result.
//
//   hipcc -O2 -Iinclude examples/jpeg_host.cpp -Ledgestyle_amd/lib -ledgestyle_hip -Wl,-rpath,$PWD/edgestyle_amd/lib -o jpeg_host
//   ./jpeg_host photo.jpg out.ppm
//
// Writes a binary PPM (P6, maxval 255) and prints the file's geometry.  The decoded image is device memory that es_person_crop_u8,
// es_sam_encode_u8, es_clip_pick and es_prepare_conds_u8 take as it lies (examples/pose_host.cpp, examples/image_host.cpp) - this host only
// downloads it to show it.  A file the decoder refuses ends the program with status 3 and the reason.
//
//   ./jpeg_host --device-entropy photo.jpg out.ppm
// takes es_jpeg_decode_dev_u8 instead (opt-in; the default is the host decoder): the file is uploaded as it is and the Huffman decoding
// runs on the device as well; the status word is read back after the stream has drained.  The PPM is the same.
//
// Built with -DJPEG_HOST_DRY the program is the decoder's host twin alone, from edgestyle_amd/csrc/jpeg.h: no library, no HIP, no GPU (and
// so a program a host sanitizer can check):
//   c++ -std=c++17 -DJPEG_HOST_DRY -Iedgestyle_amd/csrc examples/jpeg_host.cpp -o jpeg_host_dry
//   ./jpeg_host_dry --parallel T S photo.jpg out.ppm
// runs the twin of the parallel Huffman decoder too (T decoders per segment, S bytes per subsequence, 0: the default) and compares its
// decision and its coefficients with the serial decoder's: status 4 where they differ.
#include <cstring>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#ifdef JPEG_HOST_DRY
#include "jpeg.h"
#else
#include <hip/hip_runtime.h>
#include "edgestyle_hip.h"
#define HIP_OK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "HIP error at %s:%d\n", __FILE__, __LINE__); return 2; } } while (0)
#define ES_OK(x) do { if ((x) != 0) { fprintf(stderr, "%s: %s\n", #x, es_last_error()); return 3; } } while (0)
#endif

static bool read_file(const char* path, std::vector<uint8_t>& bytes) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); return false; }
  uint8_t buf[65536];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) bytes.insert(bytes.end(), buf, buf + got);
  const bool ok = !ferror(f);
  fclose(f);
  if (!ok) perror(path);
  return ok;
}
static bool write_ppm(const char* path, const uint8_t* px, int H, int W) {
  FILE* f = fopen(path, "wb");
  if (!f) { perror(path); return false; }
  fprintf(f, "P6\n%d %d\n255\n", W, H);
  const size_t n = (size_t)H * W * 3;
  const bool ok = fwrite(px, 1, n, f) == n;
  if (fclose(f) != 0 || !ok) { perror(path); return false; }
  return true;
}

int main(int argc, char** argv) {
  const char* self = argv[0];
#ifdef JPEG_HOST_DRY
  int par_threads = 0, par_subseq = 0;
  if (argc == 6 && strcmp(argv[1], "--parallel") == 0) {
    par_threads = atoi(argv[2]); par_subseq = atoi(argv[3]);
    if (par_threads < 1 || par_threads > 1024 || par_subseq < 0 || (par_subseq > 0 && par_subseq < 4)) {
      fprintf(stderr, "--parallel T S: T in 1 .. 1024, S 0 or >= 4\n");
      return 1;
    }
    argv += 3; argc -= 3;
  }
  if (argc != 3) { fprintf(stderr, "usage: %s [--parallel T S] photo.jpg out.ppm\n", self); return 1; }
#else
  bool device_entropy = false;
  if (argc == 4 && strcmp(argv[1], "--device-entropy") == 0) { device_entropy = true; argv += 1; argc -= 1; }
  if (argc != 3) { fprintf(stderr, "usage: %s [--device-entropy] photo.jpg out.ppm\n", self); return 1; }
#endif
  std::vector<uint8_t> file;
  if (!read_file(argv[1], file)) return 1;
  es_jpeg_info info;
  std::vector<uint8_t> rgb;
#ifdef JPEG_HOST_DRY
  esjpeg::Header header;
  const char* why = nullptr;
  if (!esjpeg::parse_header(file.data(), file.size(), header, &why)) { fprintf(stderr, "%s: %s\n", argv[1], why); return 3; }
  info = header.info;
  std::vector<int16_t> coeffs(esjpeg::coeff_count(info));
  std::vector<uint16_t> qtables(3 * 64);
  const bool serial_ok = esjpeg::entropy_decode(file.data(), file.size(), header, coeffs.data(), &why);
  if (par_threads) {
    std::vector<es_jpeg_segment> segments((size_t)esjpeg::restart_intervals(info));
    std::vector<int16_t> twin(coeffs.size());
    esjpeg::ScanTables tables;
    const char* refused = nullptr;
    int status = -1;
    uint32_t rounds = 0;
    if (esjpeg::scan_prepare(file.data(), file.size(), header, segments.data(), &tables, &refused))
      status = esjpeg::entropy_decode_parallel(file.data(), file.size(), info, segments.data(), tables, (uint32_t)par_subseq, (uint32_t)par_threads,
                                               twin.data(), &rounds);
    const bool parallel_ok = status == 0;
    if (parallel_ok != serial_ok || (serial_ok && twin != coeffs)) {
      fprintf(stderr, "%s: the parallel decoder differs from the serial one (serial: %s, parallel: %s)\n", argv[1], serial_ok ? "accepts" : why,
              parallel_ok ? "accepts" : status < 0 ? refused : esjpeg::status_text(status));
      return 4;
    }
    if (!serial_ok) { fprintf(stderr, "%s: both refuse: %s | %s\n", argv[1], why, status < 0 ? refused : esjpeg::status_text(status)); return 3; }
    printf("%s: %d decoders, %zu segment%s, %u synchronise round%s: equal to the serial decoder\n", argv[1], par_threads, segments.size(),
           segments.size() == 1 ? "" : "s", rounds, rounds == 1 ? "" : "s");
  }
  if (!serial_ok) { fprintf(stderr, "%s: %s\n", argv[1], why); return 3; }
  esjpeg::component_qtables(header, qtables.data());
  rgb.resize((size_t)info.height * info.width * 3);
  esjpeg::reconstruct(info, coeffs.data(), qtables.data(), rgb.data(), (size_t)info.width * 3);
#else
  ES_OK(es_jpeg_info_host(file.data(), file.size(), &info));
  const size_t out_bytes = (size_t)info.height * info.width * 3;
  const uint8_t* files[1] = {file.data()};
  const size_t sizes[1] = {file.size()};
  size_t upload = 0;
  const size_t stage = device_entropy ? es_jpeg_decode_dev_staging_bytes(&info, sizes, 1, &upload) : es_jpeg_decode_staging_bytes(&info, 1);
  const size_t need = es_jpeg_reconstruct_workspace_bytes(&info, 1);
  if (!stage || !need) { fprintf(stderr, "%s\n", es_last_error()); return 3; }
  if (!device_entropy) upload = stage;
  uint8_t* d_out = nullptr;
  int32_t* d_status = nullptr;
  void *h_stage = nullptr, *d_stage = nullptr, *d_ws = nullptr;
  HIP_OK(hipMalloc((void**)&d_out, out_bytes));
  HIP_OK(hipMalloc((void**)&d_status, sizeof(int32_t)));
  HIP_OK(hipHostMalloc(&h_stage, upload));      // pinned: the upload is asynchronous
  HIP_OK(hipMalloc(&d_stage, stage));
  HIP_OK(hipMalloc(&d_ws, need));
  const es_image_u8 out = {d_out, info.height, info.width, 3, (int64_t)info.width * 3};
  if (device_entropy) {
    ES_OK(es_jpeg_decode_dev_u8(files, sizes, 1, &out, 0, d_status, h_stage, upload, d_stage, stage, d_ws, need, nullptr));
    HIP_OK(hipDeviceSynchronize());
    int32_t status = 0;
    HIP_OK(hipMemcpy(&status, d_status, sizeof(status), hipMemcpyDeviceToHost));
    if (status != 0) { fprintf(stderr, "%s: %s\n", argv[1], es_jpeg_status_text(status)); return 3; }
  } else {
    ES_OK(es_jpeg_decode_u8(files, sizes, 1, &out, h_stage, d_stage, stage, d_ws, need, nullptr));
    HIP_OK(hipDeviceSynchronize());
  }
  rgb.resize(out_bytes);
  HIP_OK(hipMemcpy(rgb.data(), d_out, out_bytes, hipMemcpyDeviceToHost));
  (void)hipFree(d_ws); (void)hipFree(d_stage); (void)hipHostFree(h_stage); (void)hipFree(d_status); (void)hipFree(d_out);
#endif
  if (!write_ppm(argv[2], rgb.data(), info.height, info.width)) return 1;
  printf("%s: %d x %d, %d component%s, sampling %dx%d, %d x %d MCUs, restart interval %d\n", argv[1], info.width, info.height, info.components,
         info.components == 1 ? "" : "s", info.hmax, info.vmax, info.mcus_x, info.mcus_y, info.restart_interval);
  return 0;
}
