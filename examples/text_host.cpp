// From a text_encoder/ directory and token ids to the text states of a try-on request in plain C++: no Python, no torch, no transformers.
// The host memory-maps the safetensors file of a CLIPTextModel checkpoint (transformers save_pretrained: config.json + model.safetensors,
// keys bare or with the `text_model.` prefix of the SD1.5 checkpoints), describes its tensors to es_text_encoder_create
// (include/edgestyle_hip.h) and encodes the ids with es_text_encode.  The ids come from es_tokenize_padded
// (examples/prompt_host.cpp goes from text and a photo to the same record) or from whatever CLIP BPE tokenizer the caller links, padded to
// max_position_embeddings like the reference pads them (padding="max_length").
//
//   hipcc -O2 -Iinclude examples/text_host.cpp -Ledgestyle_amd/lib -ledgestyle_hip -Wl,-rpath,$PWD/edgestyle_amd/lib -o text_host
//   ./text_host <text_encoder_dir> ids.bin ehs.bin [fp16|bf16]
// ids.bin: int32 [n, max_positions], the negative prompts' rows first, then the prompts' (the order of the `ehs` operand under CFG).
// ehs.bin: uint16 [n, max_positions, hidden] - the bits of the compute dtype: exactly the `ehs` record of the inputs.bin that
// examples/image_host.cpp, tryon_host.cpp and checkpoint_host.cpp read (n = 2B).
// Built with -DTEXT_HOST_DRY the program stops after a dry build (device -1): the loader alone, runnable on a machine without a GPU
// (under a host sanitizer, for instance).
#include <hip/hip_runtime.h>

#include "safetensors.h"

#define HIP_OK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "HIP error at %s:%d\n", __FILE__, __LINE__); return 2; } } while (0)
#define ES_OK(x) do { if ((x) != 0) { fprintf(stderr, "%s: %s\n", #x, es_last_error()); return 3; } } while (0)

// everything between the files and a built encoder: the part a host without a GPU can run too (device -1: dry build)
static int load_encoder(const std::string& dir, int dtype, int max_n, int device, es_text_config* cfg, es_text_encoder** enc) {
  SafeTensors st;
  if (!st.open(dir + "/model.safetensors", true)) return 1;
  std::string cs;
  if (!read_file(dir + "/config.json", cs)) return 1;
  const Json c = parse_json(cs.data(), cs.size());
  memset(cfg, 0, sizeof(*cfg));
  cfg->vocab_size = (int)num(c, "vocab_size", 49408); cfg->hidden = (int)num(c, "hidden_size", 768);
  cfg->heads = (int)num(c, "num_attention_heads", 12); cfg->layers = (int)num(c, "num_hidden_layers", 12);
  cfg->intermediate = (int)num(c, "intermediate_size", 3072); cfg->max_positions = (int)num(c, "max_position_embeddings", 77);
  cfg->ln_eps = (float)num(c, "layer_norm_eps", 1e-5);
  const Json* act = c.get("hidden_act");
  cfg->act = !act || act->str == "quick_gelu" ? 0 : -1;       // anything else is refused by the library, with its reason
  const es_state_dict sd = st.dict();
  ES_OK(es_text_encoder_create(&sd, cfg, dtype, max_n, device, enc));
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 4 && argc != 5) { fprintf(stderr, "usage: %s text_encoder_dir ids.bin ehs.bin [fp16|bf16]\n", argv[0]); return 1; }
  const std::string dt = argc == 5 ? argv[4] : "fp16";
  if (dt != "fp16" && dt != "bf16") { fprintf(stderr, "dtype must be fp16 or bf16\n"); return 1; }
  std::string raw;
  if (!read_file(argv[2], raw)) return 1;
#ifdef TEXT_HOST_DRY
  const int device = -1;           // loader check on a machine without a GPU: build dry, report the arena, stop
#else
  const int device = 0;
#endif
  // the config decides how many ids make a row; the ids decide max_n: read the config first with a one-row dry build
  es_text_config cfg;
  es_text_encoder* probe = nullptr;
  if (int rc = load_encoder(argv[1], dt == "fp16" ? ES_F16 : ES_BF16, 1, -1, &cfg, &probe)) return rc;
  printf("text encoder: hidden %d, %d layers, %d positions; arena for one prompt %zu bytes\n", cfg.hidden, cfg.layers, cfg.max_positions,
         es_text_encoder_arena_bytes(probe));
  es_text_encoder_destroy(probe);
  const size_t row = (size_t)cfg.max_positions * 4;
  if (raw.empty() || raw.size() % row) { fprintf(stderr, "%s: %zu bytes is no whole number of rows of %d int32 ids\n", argv[2], raw.size(), cfg.max_positions); return 1; }
  const int n = (int)(raw.size() / row);
  std::vector<int32_t> ids((size_t)n * cfg.max_positions);
  memcpy(ids.data(), raw.data(), raw.size());
  es_text_encoder* enc = nullptr;
  if (int rc = load_encoder(argv[1], dt == "fp16" ? ES_F16 : ES_BF16, n, device, &cfg, &enc)) return rc;
  if (device < 0) {
    printf("dry build for %d prompts: arena %zu bytes\n", n, es_text_encoder_arena_bytes(enc));
    es_text_encoder_destroy(enc);
    return 0;
  }
  const size_t out_n = (size_t)n * cfg.max_positions * cfg.hidden;
  void* d_out = nullptr;
  HIP_OK(hipMalloc(&d_out, out_n * 2));
  hipStream_t s;
  HIP_OK(hipStreamCreate(&s));
  ES_OK(es_text_encode(enc, ids.data(), n, d_out, s));
  HIP_OK(hipStreamSynchronize(s));
  std::vector<uint16_t> out(out_n);
  HIP_OK(hipMemcpy(out.data(), d_out, out_n * 2, hipMemcpyDeviceToHost));
  FILE* o = fopen(argv[3], "wb");
  if (!o) { perror(argv[3]); return 1; }
  fwrite(out.data(), 2, out_n, o);
  fclose(o);
  es_text_encoder_destroy(enc);
  HIP_OK(hipFree(d_out));
  printf("ok: %d x %d x %d\n", n, cfg.max_positions, cfg.hidden);
  return 0;
}
