// From a person box and 18 body key points to the processed photo and the pose image, in plain C++ against the C ABI
// (include/edgestyle_hip.h) and the HIP runtime: no Python, no Pillow, no cv2.  What the reference's create_processed_image
// (extract_dataset.py:112-171: Pillow LANCZOS resize + crop around the box) and create_openpose after its detector (:270-295:
// controlnet_aux's draw_poses, body only) compute on the host: es_person_crop_u8 and es_pose_draw on the device, and the SAM point prompt
// of create_sam_images:361-365 from es_pose_points_host.
//
//   hipcc -O2 -Iinclude examples/pose_host.cpp -Ledgestyle_amd/lib -ledgestyle_hip -Wl,-rpath,$PWD/edgestyle_amd/lib -o pose_host
//   ./pose_host photo.ppm xmin ymin xmax ymax keypoints.txt out
//
// photo.ppm: binary PPM (P6, maxval 255) of any size, or a baseline JPEG file (told by its first two bytes, decoded by es_jpeg_decode_u8).  xmin .. ymax: the person detector's box in the photo's pixels.  keypoints.txt: 18
// lines "x y score" in OpenPose body order, x and y normalised to [0, 1] of the processed photo, score 0 for a point that was not found.
// Writes out_processed.ppm and out_pose.ppm (512 x 512 each) and prints the point prompt; both images are device memory that
// es_sam_encode_u8, es_sam_compose and es_prepare_conds_u8 take as they are (examples/mask_host.cpp, examples/image_host.cpp) - this host
// only downloads them to show them.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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
static bool read_ppm(const char* path, std::vector<uint8_t>& px, int* H, int* W) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); return false; }
  int maxval = 0;
  bool ok = fgetc(f) == 'P' && fgetc(f) == '6' && pnm_int(f, W) && pnm_int(f, H) && pnm_int(f, &maxval) && maxval == 255 && *H > 0 && *W > 0;
  if (ok) {
    px.resize((size_t)*H * *W * 3);
    ok = fread(px.data(), 1, px.size(), f) == px.size();
  }
  fclose(f);
  if (!ok) fprintf(stderr, "%s: not a binary P6 file with maxval 255\n", path);
  return ok;
}
static bool write_ppm(const std::string& path, const uint8_t* px, int H, int W) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) { perror(path.c_str()); return false; }
  fprintf(f, "P6\n%d %d\n255\n", W, H);
  const size_t n = (size_t)H * W * 3;
  const bool ok = fwrite(px, 1, n, f) == n;
  if (fclose(f) != 0 || !ok) { perror(path.c_str()); return false; }
  return true;
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
  if (argc != 8) { fprintf(stderr, "usage: %s photo.ppm xmin ymin xmax ymax keypoints.txt out\n", argv[0]); return 1; }
  std::vector<uint8_t> photo;
  int H = 0, W = 0;
  uint8_t* d_photo = nullptr;
  const bool jpeg = is_jpeg(argv[1]);
  if (jpeg) {
    if (const int rc = load_jpeg(argv[1], &d_photo, &H, &W)) return rc;
  } else if (!read_ppm(argv[1], photo, &H, &W)) return 1;
  const double box[4] = {atof(argv[2]), atof(argv[3]), atof(argv[4]), atof(argv[5])};
  float kp[18 * 3];
  {
    FILE* f = fopen(argv[6], "r");
    if (!f) { perror(argv[6]); return 1; }
    int got = 0;
    while (got < 54 && fscanf(f, "%f", &kp[got]) == 1) ++got;
    fclose(f);
    if (got != 54) { fprintf(stderr, "%s: 18 lines of \"x y score\" expected, %d numbers read\n", argv[6], got); return 1; }
  }
  const int S = 512;                            // the reference's IMAGE_WIDTH = IMAGE_HEIGHT: what es_person_crop_u8 writes
  const size_t out_bytes = (size_t)S * S * 3;
  uint8_t *d_processed = nullptr, *d_pose = nullptr;
  float* d_kp = nullptr;
  void* d_ws = nullptr;
  if (!jpeg) {
    HIP_OK(hipMalloc((void**)&d_photo, photo.size()));
    HIP_OK(hipMemcpy(d_photo, photo.data(), photo.size(), hipMemcpyHostToDevice));
  }
  HIP_OK(hipMalloc((void**)&d_kp, sizeof(kp)));
  HIP_OK(hipMemcpy(d_kp, kp, sizeof(kp), hipMemcpyHostToDevice));
  HIP_OK(hipMalloc((void**)&d_processed, out_bytes));
  HIP_OK(hipMalloc((void**)&d_pose, out_bytes));
  const es_image_u8 img = {d_photo, H, W, 3, (int64_t)W * 3};
  int32_t geom[4];
  ES_OK(es_person_crop_fit(H, W, box, S, S, 0.1, geom));
  const size_t need = es_person_crop_u8_workspace_bytes(&img, 1, box);
  HIP_OK(hipMalloc(&d_ws, need ? need : 1));
  ES_OK(es_person_crop_u8(&img, 1, box, d_processed, d_ws, need, nullptr));
  ES_OK(es_pose_draw(d_kp, d_pose, 1, S, S, nullptr));
  HIP_OK(hipDeviceSynchronize());
  std::vector<uint8_t> host(out_bytes);
  HIP_OK(hipMemcpy(host.data(), d_processed, out_bytes, hipMemcpyDeviceToHost));
  if (!write_ppm(std::string(argv[7]) + "_processed.ppm", host.data(), S, S)) return 1;
  HIP_OK(hipMemcpy(host.data(), d_pose, out_bytes, hipMemcpyDeviceToHost));
  if (!write_ppm(std::string(argv[7]) + "_pose.ppm", host.data(), S, S)) return 1;
  float points[18 * 2];
  const int P = es_pose_points_host(kp, S, S, points);
  if (P < 0) { fprintf(stderr, "es_pose_points_host: %s\n", es_last_error()); return 3; }
  printf("photo %d x %d -> resized %d x %d, window at (%d, %d); %d SAM points:", W, H, geom[0], geom[1], geom[2], geom[3], P);
  for (int i = 0; i < P; ++i) printf(" (%g, %g)", points[2 * i], points[2 * i + 1]);
  printf("\n");
  (void)hipFree(d_ws); (void)hipFree(d_pose); (void)hipFree(d_processed); (void)hipFree(d_kp); (void)hipFree(d_photo);
  return 0;
}
