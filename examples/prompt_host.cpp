// From a garment photo and two pieces of text to the text states of a try-on request in plain C++: no Python, no torch, no transformers.
// The host memory-maps a CLIPModel directory (transformers save_pretrained: config.json + model.safetensors), builds the library's
// tokenizer from a vocab.json and a merges.txt, scores the photo against the caller's words (es_clip_pick), assembles the prompt
// "edgestyle , c1 , c2 , i1 , i2 <suffix>" from the picks on the device (es_prompt_assemble) and encodes it, with the negative prompt,
// by the model's text tower (es_text_encode_dev).  The picks never visit the host.
//
//   hipcc -O2 -Iinclude examples/prompt_host.cpp -Ledgestyle_amd/lib -ledgestyle_hip -Wl,-rpath,$PWD/edgestyle_amd/lib -o prompt_host
//   ./prompt_host <clip_dir> vocab.json merges.txt words.txt garment.ppm "<suffix>" "<negative prompt>" ehs.bin [fp16|bf16]
// words.txt: one word per line; an empty line ends a vocabulary (the colours, then the garments: at most four lists).
// garment.ppm: binary PPM (P6, maxval 255) of any size.
// ehs.bin: uint16 [2, max_positions, hidden] - the bits of the compute dtype, the negative prompt's row first: exactly the `ehs` record
// of the inputs.bin that examples/image_host.cpp, tryon_host.cpp and checkpoint_host.cpp read at B = 1.
// The word lists, the suffix and the negative prompt are the caller's; the reference's own are its data and are not in this tree.
//
// Built with -DPROMPT_HOST_DRY the program is the tokenizer alone, from edgestyle_amd/csrc/bpe.h: no library, no HIP, no GPU (and so
// a fit subject for a host sanitizer):
//   c++ -std=c++17 -DPROMPT_HOST_DRY -Iedgestyle_amd/csrc examples/prompt_host.cpp -o prompt_host_dry
//   ./prompt_host_dry vocab.json merges.txt texts.bin [max_length]
// texts.bin: records of a little-endian uint32 length and that many bytes.  One line per record: the padded ids, or the refusal.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#ifdef PROMPT_HOST_DRY
#include "bpe.h"

static bool slurp(const char* path, std::string& out) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); return false; }
  char buf[4096]; size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) out.append(buf, n);
  fclose(f);
  return true;
}

int main(int argc, char** argv) {
  if (argc != 4 && argc != 5) { fprintf(stderr, "usage: %s vocab.json merges.txt texts.bin [max_length]\n", argv[0]); return 1; }
  std::string vocab, merges, texts, err;
  if (!slurp(argv[1], vocab) || !slurp(argv[2], merges) || !slurp(argv[3], texts)) return 1;
  es_bpe::Tokenizer tok;
  if (!es_bpe::load(&tok, vocab.data(), vocab.size(), merges.data(), merges.size(), argc == 5 ? atoi(argv[4]) : 77, &err)) { fprintf(stderr, "%s\n", err.c_str()); return 3; }
  std::vector<int32_t> row((size_t)tok.max_length), ids;
  size_t at = 0, refused = 0, count = 0;
  while (at + 4 <= texts.size()) {
    uint32_t len;
    memcpy(&len, texts.data() + at, 4);
    at += 4;
    if (len > texts.size() - at) { fprintf(stderr, "%s: a record runs past the end of the file\n", argv[3]); return 1; }
    const char* text = texts.data() + at;
    at += len;
    ++count;
    if (!es_bpe::check_text(text, len, &err)) { printf("refused: %s\n", err.c_str()); ++refused; continue; }
    ids.clear();
    es_bpe::encode(&tok, text, len, &ids);
    es_bpe::pad_row(tok, ids, row.data());
    for (int i = 0; i < tok.max_length; ++i) printf(i ? " %d" : "%d", row[i]);
    printf("\n");
  }
  if (at != texts.size()) { fprintf(stderr, "%s: trailing bytes\n", argv[3]); return 1; }
  fprintf(stderr, "%zu texts, %zu refused\n", count, refused);
  return 0;
}
#else
#include <hip/hip_runtime.h>

#include <cmath>

#include "safetensors.h"

#define HIP_OK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "HIP error at %s:%d\n", __FILE__, __LINE__); return 2; } } while (0)
#define ES_OK(x) do { if ((x) != 0) { fprintf(stderr, "%s: %s\n", #x, es_last_error()); return 3; } } while (0)

// one header token of a PPM: digits after whitespace and # comments (examples/image_host.cpp's reader)
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
  return c == ' ' || c == '\t' || c == '\n' || c == '\r';
}
static bool read_ppm(const char* path, std::vector<uint8_t>& px, int* H, int* W) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); return false; }
  int maxval = 0;
  bool ok = fgetc(f) == 'P' && fgetc(f) == '6' && ppm_int(f, W) && ppm_int(f, H) && ppm_int(f, &maxval) && maxval == 255 && *H > 0 && *W > 0;
  if (ok) { px.resize((size_t)*H * *W * 3); ok = fread(px.data(), 1, px.size(), f) == px.size(); }
  fclose(f);
  if (!ok) fprintf(stderr, "%s: not a binary PPM (P6, maxval 255)\n", path);
  return ok;
}

int main(int argc, char** argv) {
  if (argc != 9 && argc != 10) {
    fprintf(stderr, "usage: %s clip_dir vocab.json merges.txt words.txt garment.ppm suffix negative_prompt ehs.bin [fp16|bf16]\n", argv[0]);
    return 1;
  }
  const std::string dir = argv[1], dt = argc == 10 ? argv[9] : "fp16";
  if (dt != "fp16" && dt != "bf16") { fprintf(stderr, "dtype must be fp16 or bf16\n"); return 1; }
  const int dtype = dt == "fp16" ? ES_F16 : ES_BF16, device = 0;

  // ---- the model's description and weights ----
  std::string cs;
  if (!read_file(dir + "/config.json", cs)) return 1;
  const Json c = parse_json(cs.data(), cs.size());
  const Json *tj = c.get("text_config"), *vj = c.get("vision_config");
  if (!tj || !vj) { fprintf(stderr, "%s/config.json: text_config / vision_config missing (a CLIPModel directory is expected)\n", dir.c_str()); return 1; }
  auto act = [](const Json& j) { const Json* a = j.get("hidden_act"); return !a || a->str == "quick_gelu" ? 0 : -1; };      // else refused by the library
  es_text_config tc;
  memset(&tc, 0, sizeof(tc));
  tc.vocab_size = (int)num(*tj, "vocab_size", 49408); tc.hidden = (int)num(*tj, "hidden_size", 512); tc.heads = (int)num(*tj, "num_attention_heads", 8);
  tc.layers = (int)num(*tj, "num_hidden_layers", 12); tc.intermediate = (int)num(*tj, "intermediate_size", 2048);
  tc.max_positions = (int)num(*tj, "max_position_embeddings", 77); tc.ln_eps = (float)num(*tj, "layer_norm_eps", 1e-5); tc.act = act(*tj);
  es_clip_vision_config vc;
  memset(&vc, 0, sizeof(vc));
  vc.image_size = (int)num(*vj, "image_size", 224); vc.patch_size = (int)num(*vj, "patch_size", 32); vc.hidden = (int)num(*vj, "hidden_size", 768);
  vc.heads = (int)num(*vj, "num_attention_heads", 12); vc.layers = (int)num(*vj, "num_hidden_layers", 12);
  vc.intermediate = (int)num(*vj, "intermediate_size", 3072); vc.projection_dim = (int)num(c, "projection_dim", 512);
  vc.ln_eps = (float)num(*vj, "layer_norm_eps", 1e-5); vc.act = act(*vj);
  const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f}, stdv[3] = {0.26862954f, 0.26130258f, 0.27577711f};      // OpenAI CLIP's
  for (int i = 0; i < 3; ++i) { vc.image_mean[i] = mean[i]; vc.image_std[i] = stdv[i]; }
  SafeTensors st;
  if (!st.open(dir + "/model.safetensors", true)) return 1;
  const es_state_dict sd = st.dict();
  float logit_scale = 0.f;
  bool have_scale = false;
  for (const es_tensor& t : st.tensors)
    if (!strcmp(t.key, "logit_scale") && t.dtype == ES_F32) { memcpy(&logit_scale, t.data, 4); have_scale = true; }
  if (!have_scale) { fprintf(stderr, "%s/model.safetensors: no fp32 'logit_scale'\n", dir.c_str()); return 1; }

  // ---- the words ----
  std::string wtxt;
  if (!read_file(argv[4], wtxt)) return 1;
  std::vector<std::string> words;
  std::vector<int32_t> seg_ends;
  for (size_t a = 0; a <= wtxt.size();) {
    size_t e = wtxt.find('\n', a);
    if (e == std::string::npos) e = wtxt.size();
    std::string line = wtxt.substr(a, e - a);
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (!line.empty()) words.push_back(line);
    else if (!words.empty() && (seg_ends.empty() || seg_ends.back() != (int32_t)words.size())) seg_ends.push_back((int32_t)words.size());
    a = e + 1;
  }
  if (!words.empty() && (seg_ends.empty() || seg_ends.back() != (int32_t)words.size())) seg_ends.push_back((int32_t)words.size());
  if (words.empty() || seg_ends.size() > 4) { fprintf(stderr, "%s: one to four lists of words, separated by empty lines\n", argv[4]); return 1; }
  const int W = (int)words.size(), nseg = (int)seg_ends.size(), S = tc.max_positions, k = 2;

  es_tokenizer* tok = nullptr;
  ES_OK(es_tokenizer_create(argv[2], argv[3], S, &tok));
  std::vector<int32_t> word_ids((size_t)W * S), word_eos(W), neg_ids(S);
  for (int w = 0; w < W; ++w) ES_OK(es_tokenize_padded(tok, words[w].data(), words[w].size(), &word_ids[(size_t)w * S], &word_eos[w]));
  ES_OK(es_tokenize_padded(tok, argv[7], strlen(argv[7]), neg_ids.data(), nullptr));
  std::vector<const char*> wp(W);
  for (int w = 0; w < W; ++w) wp[w] = words[w].c_str();

  // ---- the towers, the bank (once per vocabulary) and the prompt table ----
  HIP_OK(hipSetDevice(device));
  hipStream_t s;
  HIP_OK(hipStreamCreate(&s));
  const int max_n = W < 32 ? (W < 2 ? 2 : W) : 32;
  es_text_encoder* enc = nullptr;
  es_clip_vision* vis = nullptr;
  es_clip_bank* bank = nullptr;
  es_prompt_table* table = nullptr;
  ES_OK(es_text_encoder_create(&sd, &tc, dtype, max_n, device, &enc));
  ES_OK(es_clip_vision_create(&sd, &vc, dtype, 1, device, &vis));
  ES_OK(es_clip_bank_create(&sd, tc.hidden, vc.projection_dim, W, max_n, dtype, device, &bank));
  ES_OK(es_prompt_table_create(tok, wp.data(), W, seg_ends.data(), nseg, "edgestyle", ",", argv[6], device, &table));
  void* d_ehs = nullptr;
  HIP_OK(hipMalloc(&d_ehs, (size_t)max_n * S * tc.hidden * 2));
  for (int a = 0; a < W; a += max_n) {
    const int n = W - a < max_n ? W - a : max_n;
    ES_OK(es_text_encode(enc, &word_ids[(size_t)a * S], n, d_ehs, s));
    ES_OK(es_clip_text_pool(bank, d_ehs, &word_eos[a], n, S, s));
  }

  // ---- the request: photo -> picks -> ids -> text states, all on the stream ----
  std::vector<uint8_t> px;
  int H = 0, Wd = 0;
  if (!read_ppm(argv[5], px, &H, &Wd)) return 1;
  void *d_px = nullptr, *d_ws = nullptr;
  int32_t *d_topk = nullptr, *d_ids = nullptr;
  HIP_OK(hipMalloc(&d_px, px.size()));
  HIP_OK(hipMemcpyAsync(d_px, px.data(), px.size(), hipMemcpyHostToDevice, s));
  es_image_u8 img;
  memset(&img, 0, sizeof(img));
  img.data = (const uint8_t*)d_px; img.height = H; img.width = Wd; img.channels = 3; img.row_stride = (int64_t)Wd * 3;
  const size_t need = es_clip_pick_workspace_bytes(vis, &img, 1);
  if (!need) { fprintf(stderr, "es_clip_pick_workspace_bytes: %s\n", es_last_error()); return 3; }
  HIP_OK(hipMalloc(&d_ws, need));
  HIP_OK(hipMalloc((void**)&d_topk, (size_t)nseg * k * 4));
  HIP_OK(hipMalloc((void**)&d_ids, (size_t)2 * S * 4));
  HIP_OK(hipMemcpyAsync(d_ids, neg_ids.data(), (size_t)S * 4, hipMemcpyHostToDevice, s));          // row 0: the negative prompt
  ES_OK(es_clip_pick(vis, bank, &img, 1, (float)exp((double)logit_scale), seg_ends.data(), nseg, k, nullptr, nullptr, d_topk, d_ws, need, s));
  ES_OK(es_prompt_assemble(table, d_topk, 1, k, d_ids + S, nullptr, s));                           // row 1: the prompt
  ES_OK(es_text_encode_dev(enc, d_ids, 2, d_ehs, s));
  HIP_OK(hipStreamSynchronize(s));

  const size_t out_n = (size_t)2 * S * tc.hidden;
  std::vector<uint16_t> out(out_n);
  std::vector<int32_t> topk((size_t)nseg * k);
  HIP_OK(hipMemcpy(out.data(), d_ehs, out_n * 2, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(topk.data(), d_topk, topk.size() * 4, hipMemcpyDeviceToHost));                  // for the log line only
  printf("prompt: edgestyle");
  for (int g = 0; g < nseg; ++g)
    for (int j = 0; j < k; ++j) {
      const int e = topk[(size_t)g * k + j], start = g ? seg_ends[g - 1] : 0;
      if (e >= 0 && e < seg_ends[g] - start) printf(", %s", words[start + e].c_str());
    }
  printf(" %s\n", argv[6]);
  FILE* o = fopen(argv[8], "wb");
  if (!o) { perror(argv[8]); return 1; }
  const bool wrote = fwrite(out.data(), 2, out_n, o) == out_n;
  if (fclose(o) != 0 || !wrote) { fprintf(stderr, "%s: write failed\n", argv[8]); return 1; }
  es_prompt_table_destroy(table);
  es_clip_bank_destroy(bank);
  es_clip_vision_destroy(vis);
  es_text_encoder_destroy(enc);
  es_tokenizer_destroy(tok);
  HIP_OK(hipFree(d_ehs)); HIP_OK(hipFree(d_px)); HIP_OK(hipFree(d_ws)); HIP_OK(hipFree(d_topk)); HIP_OK(hipFree(d_ids));
  HIP_OK(hipStreamDestroy(s));
  printf("ok: 2 x %d x %d\n", S, tc.hidden);
  return 0;
}
#endif
