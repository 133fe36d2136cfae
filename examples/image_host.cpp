// The try-on path from decoded photos to bytes, in plain C++ against the C ABI (include/edgestyle_hip.h) and the HIP runtime: no
// Python, no torch, no model code, and no float image ever crosses the bus.  It loads a context image (es_ctx_save /
// edgestyle_amd/native.py NativeEngine.save), uploads six binary PPM files of ANY size, has the library resize, crop and convert
// them on the device exactly as the reference's transforms would (test_text2image_pretrained_openpose.py:29-48), runs the
// 6-ControlNet denoising loop and the VAE decode, and writes the result as a PPM.
//
//   hipcc -O2 -Iinclude examples/image_host.cpp -Ledgestyle_amd/lib -ledgestyle_hip -Wl,-rpath,$PWD/edgestyle_amd/lib -o image_host
//   ./image_host ctx.esctx cond0.ppm cond1.ppm cond2.ppm cond3.ppm cond4.ppm cond5.ppm inputs.bin out.ppm [--seed S [--cond-seed S2]]
//
// cond<i>.ppm: binary PPM (P6, maxval 255) or a baseline JPEG file (told by its first two bytes, decoded by es_jpeg_decode_u8), the condition image of net i in the reference's order (agnostic, subject pose,
// clothes 1, pose 1, clothes 2, pose 2); a context of batch B > 1 takes the same six photos for every image of the batch.
// inputs.bin (little endian, written by tests/test_image_io_gpu.py):
//   int32 B, h, w, L, D, n_conds, n_steps, has_noise[n_conds], normalize[n_conds]; float guidance_scale; float timesteps[n_steps];
//   float latents[B*h*w*L] (NHWC); uint16 ehs[2B*77*D] (fp16 bits, negative prompt rows first);
//   per net with has_noise: float noise[2B*L*h*w]      (host noise, the default: the caller's own arrays, which the CPU oracle
//                                                       can reproduce)
// --seed S: the latents and noise records of inputs.bin are ignored and the library draws both from torch's device Philox stream
//   (csrc/rng.hip) - the latents as torch.Generator("cuda").manual_seed(S) would (TT:274, app.py:119), the VAE-sample noise as the
//   device's default generator would after torch.manual_seed(S2) (CL:39); --cond-seed S2 defaults to S.  Both schedulers the
//   library implements start from init_noise_sigma 1.
// out.ppm: image 0 of the batch, 8h x 8w
//
// What each call replaces in the reference: es_prepare_conds_u8 = the transforms of TT:29-48 + prepare_image + preprocess_image
// (PL:629-664, CL:289-290), es_denoise_loop = the loop of PL:435-543, es_vae_decode_u8 = PL:552-572 with output_type "pil".
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "edgestyle_hip.h"

#define HIP_OK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "HIP error at %s:%d\n", __FILE__, __LINE__); return 2; } } while (0)
#define ES_OK(x) do { if ((x) != 0) { fprintf(stderr, "%s: %s\n", #x, es_last_error()); return 3; } } while (0)

template <typename T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return fread(v.data(), sizeof(T), n, f) == n; }

// one header token of a PPM: digits (or the magic) after whitespace and # comments
static bool ppm_int(FILE* f, int* v) {
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
static bool read_ppm(const char* path, std::vector<uint8_t>& px, int* H, int* W) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); return false; }
  int maxval = 0;
  const bool ok = fgetc(f) == 'P' && fgetc(f) == '6' && ppm_int(f, W) && ppm_int(f, H) && ppm_int(f, &maxval) && maxval == 255 &&
                  *H > 0 && *W > 0 && rd(f, px, (size_t)*H * *W * 3);
  fclose(f);
  if (!ok) fprintf(stderr, "%s: not a binary PPM (P6, maxval 255)\n", path);
  return ok;
}

// A photo that starts FF D8 is a JPEG file: decoded on the device by es_jpeg_decode_u8 (headers and Huffman decoding on this thread) into
// [H, W, 3] device bytes, the bytes Pillow's Image.open(..).convert("RGB") gives.  0, or the exit status.
static bool is_jpeg(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  const bool yes = fgetc(f) == 0xFF && fgetc(f) == 0xD8;
  fclose(f);
  return yes;
}
static int load_jpeg(const char* path, uint8_t** d_px, int* H, int* W) {
  std::vector<uint8_t> file;
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); return 1; }
  uint8_t buf[65536];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) file.insert(file.end(), buf, buf + got);
  fclose(f);
  es_jpeg_info info;
  ES_OK(es_jpeg_info_host(file.data(), file.size(), &info));
  const size_t stage = es_jpeg_decode_staging_bytes(&info, 1), need = es_jpeg_reconstruct_workspace_bytes(&info, 1);
  void *h_stage = nullptr, *d_stage = nullptr, *d_ws = nullptr;
  HIP_OK(hipMalloc((void**)d_px, (size_t)info.height * info.width * 3));
  HIP_OK(hipHostMalloc(&h_stage, stage));
  HIP_OK(hipMalloc(&d_stage, stage));
  HIP_OK(hipMalloc(&d_ws, need));
  const es_image_u8 out = {*d_px, info.height, info.width, 3, (int64_t)info.width * 3};
  const uint8_t* files[1] = {file.data()};
  const size_t sizes[1] = {file.size()};
  ES_OK(es_jpeg_decode_u8(files, sizes, 1, &out, h_stage, d_stage, stage, d_ws, need, nullptr));
  HIP_OK(hipDeviceSynchronize());
  (void)hipFree(d_ws); (void)hipFree(d_stage); (void)hipHostFree(h_stage);
  *H = info.height; *W = info.width;
  return 0;
}

int main(int argc, char** argv) {
  bool seeded = false, usage = argc < 10 || (argc - 10) % 2 != 0;
  es_philox lat_gen = {0, 0}, cond_gen = {0, 0};
  bool cond_given = false;
  for (int a = 10; a + 1 < argc && !usage; a += 2) {
    char* end = nullptr;
    const unsigned long long v = strtoull(argv[a + 1], &end, 10);
    if (!*argv[a + 1] || *end) usage = true;
    else if (!strcmp(argv[a], "--seed")) { lat_gen.seed = v; seeded = true; }
    else if (!strcmp(argv[a], "--cond-seed")) { cond_gen.seed = v; cond_given = true; }
    else usage = true;
  }
  if (cond_given && !seeded) usage = true;
  if (usage) { fprintf(stderr, "usage: %s ctx.esctx cond0.ppm .. cond5.ppm inputs.bin out.ppm [--seed S [--cond-seed S2]]\n", argv[0]); return 1; }
  if (!cond_given) cond_gen.seed = lat_gen.seed;
  FILE* f = fopen(argv[8], "rb");
  if (!f) { perror(argv[8]); return 1; }
  int32_t hd[7];
  if (fread(hd, 4, 7, f) != 7) return 1;
  const int B = hd[0], h = hd[1], w = hd[2], L = hd[3], D = hd[4], nc = hd[5], T = hd[6];
  if (nc != 6 || B < 1) { fprintf(stderr, "this host feeds six condition images\n"); return 1; }
  std::vector<int32_t> has_noise, normalize;
  float gs;
  std::vector<float> ts, lat;
  std::vector<uint16_t> ehs;
  if (!rd(f, has_noise, nc) || !rd(f, normalize, nc) || fread(&gs, 4, 1, f) != 1 || !rd(f, ts, T) || !rd(f, lat, (size_t)B * h * w * L) ||
      !rd(f, ehs, (size_t)2 * B * 77 * D)) return 1;
  const size_t noise_n = (size_t)2 * B * L * h * w;

  es_ctx* ctx = nullptr;
  ES_OK(es_ctx_load(argv[1], 0, &ctx));

  std::vector<const float*> d_noise(nc, nullptr);
  std::vector<float> tmp;
  for (int i = 0; i < nc; ++i)
    if (has_noise[i]) {
      float* p = nullptr;
      if (!rd(f, tmp, noise_n)) return 1;
      if (seeded) continue;                     // drawn on the device instead (es_ctx_draw_cond_noise)
      HIP_OK(hipMalloc(&p, noise_n * 4));
      HIP_OK(hipMemcpy(p, tmp.data(), noise_n * 4, hipMemcpyHostToDevice));
      d_noise[i] = p;
    }
  fclose(f);

  // the photos: bytes up, as they are (any size, dense rows)
  std::vector<es_image_u8> imgs((size_t)nc * B);
  std::vector<uint8_t> px;
  for (int i = 0; i < nc; ++i) {
    int H = 0, W = 0;
    uint8_t* p = nullptr;
    if (is_jpeg(argv[2 + i])) {
      if (const int rc = load_jpeg(argv[2 + i], &p, &H, &W)) return rc;
    } else {
      if (!read_ppm(argv[2 + i], px, &H, &W)) return 1;
      HIP_OK(hipMalloc(&p, px.size()));
      HIP_OK(hipMemcpy(p, px.data(), px.size(), hipMemcpyHostToDevice));
    }
    for (int b = 0; b < B; ++b) imgs[(size_t)i * B + b] = es_image_u8{p, H, W, 3, (int64_t)W * 3};
  }
  const int R = 8 * h;
  const size_t ws_bytes = es_image_resize_workspace_bytes(imgs.data(), nc * B, R);
  void* d_ws = nullptr;
  HIP_OK(hipMalloc(&d_ws, ws_bytes ? ws_bytes : 1));

  float* d_lat = nullptr;
  void* d_ehs = nullptr;
  uint8_t* d_out = nullptr;
  const size_t out_n = (size_t)B * 8 * h * 8 * w * 3;
  HIP_OK(hipMalloc(&d_lat, lat.size() * 4));
  HIP_OK(hipMemcpy(d_lat, lat.data(), lat.size() * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMalloc(&d_ehs, ehs.size() * 2));
  HIP_OK(hipMemcpy(d_ehs, ehs.data(), ehs.size() * 2, hipMemcpyHostToDevice));
  HIP_OK(hipMalloc(&d_out, out_n));

  hipStream_t st;
  HIP_OK(hipStreamCreate(&st));
  if (seeded) {
    ES_OK(es_ctx_draw_cond_noise(ctx, &cond_gen, ES_F32, st));          // NULL noise pointers below keep what this drew
    ES_OK(es_ctx_draw_latents(ctx, &lat_gen, 1, 1.0f, ES_F32, d_lat, st));
  }
  ES_OK(es_prepare_conds_u8(ctx, imgs.data(), normalize.data(), d_noise.data(), d_ws, ws_bytes, st));
  ES_OK(es_denoise_loop(ctx, d_lat, d_ehs, gs, ts.data(), T, st));
  ES_OK(es_vae_decode_u8(ctx, d_lat, d_out, st));
  HIP_OK(hipStreamSynchronize(st));

  std::vector<uint8_t> out((size_t)8 * h * 8 * w * 3);
  HIP_OK(hipMemcpy(out.data(), d_out, out.size(), hipMemcpyDeviceToHost));
  FILE* o = fopen(argv[9], "wb");
  if (!o) { perror(argv[9]); return 1; }
  fprintf(o, "P6\n%d %d\n255\n", 8 * w, 8 * h);
  fwrite(out.data(), 1, out.size(), o);
  fclose(o);
  es_ctx_destroy(ctx);
  printf("ok\n");
  return 0;
}
