// The prompt side of a try-on request at the C ABI (gfx950): text in, token ids out - and, on the device, the picker's best words in, the
// padded id row of their prompt out, with no host in between.
//
// Replaces what the reference does between BestEmbeddings and CLIPTextModel (app.py:161-176, model/utils.py:661): join the picked words
// into a string on the host, run transformers' CLIPTokenizer over it, upload the ids.  Three pieces live here:
//   es_tokenizer        the C ABI of bpe.h: CLIP's byte-level BPE from a vocab.json and a merges.txt, exact on its domain or refusing.
//   es_prompt_table     every word of the picker's vocabularies, and the prefix, separator and suffix, tokenised ONCE on the host and
//                       uploaded: tokens[W, Lw], len[W], the fixed ids.
//   es_prompt_assemble  one wave per prompt row: lane l finds the token of positions l, l + 64, ... by walking the at most 2 + 2 nseg k
//                       piece lengths (bpe.h prompt_token_at, the same code es_prompt_assemble_host runs).  Plain stores, no atomics, no
//                       allocation, nothing staged: capturable.  A topk entry outside its segment is skipped before it is used as an index.
// The assembled row equals tokenising the pieces joined by single spaces: a piece boundary is always a pre-token boundary.
// None of these calls is ever part of a plan: while a plan records on the calling thread they return -1.
#include "encoder.h"
#include "bpe.h"

using namespace es_enc;

struct es_tokenizer { es_bpe::Tokenizer t; };

struct es_prompt_table {
  es_bpe::PromptView host, dev;                // the same table through host and through device pointers (dev.tokens NULL: host only)
  std::vector<int32_t> store;                  // tokens | len | fixed
  int32_t* arena = nullptr;
  int device = -1, n_words = 0;
};

namespace {

const char* const kRecording = "a plan is recording on this thread; the prompt calls are never part of a plan";

__global__ __launch_bounds__(64) void prompt_assemble_kernel(const es_bpe::PromptView v, const int32_t* __restrict__ topk, const int k,
                                                            int32_t* __restrict__ ids, int32_t* __restrict__ eos_pos) {
  const int row = blockIdx.x, lane = threadIdx.x;
  const int32_t* tk = topk + (size_t)row * v.nseg * k;
  int32_t ep = 0;
  for (int pos = lane; pos < v.max_length; pos += 64) ids[(size_t)row * v.max_length + pos] = es_bpe::prompt_token_at(v, tk, k, pos, &ep);
  if (lane == 0 && eos_pos) eos_pos[row] = ep;         // max_length >= 2: lane 0 has walked the pieces
}

bool read_all(const char* path, std::string* out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  char buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) out->append(buf, n);
  const bool ok = !ferror(f);
  fclose(f);
  return ok;
}

int create_from(const char* who, const char* vj, size_t vn, const char* mt, size_t mn, int max_length, es_tokenizer** out) {
  std::unique_ptr<es_tokenizer> t(new es_tokenizer);
  std::string err;
  if (!es_bpe::load(&t->t, vj, vn, mt, mn, max_length, &err)) return fail(-1, who, err);
  *out = t.release();
  return 0;
}

int check_assemble(const char* who, const es_prompt_table* t, const void* topk, int n, int k, const void* ids_out) {
  if (!t || !topk || !ids_out) return fail(-1, who, "null pointer");
  if (n < 1 || n > 65535) return fail(-1, who, "n must be in 1..65535");
  if (k < 1 || k > es_bpe::MAX_K) return fail(-1, who, "k must be in 1..8 (es_clip_score's)");
  return 0;
}

}  // namespace

extern "C" int es_tokenizer_create_from_memory(const char* vocab_json, size_t vocab_bytes, const char* merges_txt, size_t merges_bytes,
                                               int max_length, es_tokenizer** out) {
  const char* who = "es_tokenizer_create_from_memory";
  if (out) *out = nullptr;
  if (!vocab_json || !out || (!merges_txt && merges_bytes)) return fail(-1, who, "null pointer");
  return create_from(who, vocab_json, vocab_bytes, merges_txt ? merges_txt : "", merges_bytes, max_length, out);
}

extern "C" int es_tokenizer_create(const char* vocab_json_path, const char* merges_txt_path, int max_length, es_tokenizer** out) {
  const char* who = "es_tokenizer_create";
  if (out) *out = nullptr;
  if (!vocab_json_path || !merges_txt_path || !out) return fail(-1, who, "null pointer");
  std::string v, m;
  if (!read_all(vocab_json_path, &v)) return fail(-1, who, std::string("cannot read ") + vocab_json_path);
  if (!read_all(merges_txt_path, &m)) return fail(-1, who, std::string("cannot read ") + merges_txt_path);
  return create_from(who, v.data(), v.size(), m.data(), m.size(), max_length, out);
}

extern "C" void es_tokenizer_destroy(es_tokenizer* t) { delete t; }
extern "C" int es_tokenizer_vocab_size(const es_tokenizer* t) { return t ? (int)t->t.vocab.size() : 0; }
extern "C" int es_tokenizer_max_length(const es_tokenizer* t) { return t ? t->t.max_length : 0; }
extern "C" int es_tokenizer_bos_id(const es_tokenizer* t) { return t ? t->t.bos : -1; }
extern "C" int es_tokenizer_eos_id(const es_tokenizer* t) { return t ? t->t.eos : -1; }
extern "C" int es_tokenizer_pad_id(const es_tokenizer* t) { return t ? t->t.eos : -1; }

extern "C" int es_tokenize(es_tokenizer* t, const char* text, size_t len, int32_t* ids_out, int capacity) {
  const char* who = "es_tokenize";
  if (!t || (!text && len) || (!ids_out && capacity > 0)) return fail(-1, who, "null pointer");
  if (capacity < 0) return fail(-1, who, "negative capacity");
  std::string err;
  if (!es_bpe::check_text(text, len, &err)) return fail(-1, who, err);
  std::vector<int32_t> ids;
  es_bpe::encode(&t->t, text, len, &ids);
  if (ids.size() > 0x7fffffffull) return fail(-1, who, "more than 2^31 - 1 tokens");
  for (size_t i = 0; i < ids.size() && i < (size_t)capacity; ++i) ids_out[i] = ids[i];
  return (int)ids.size();
}

extern "C" int es_tokenize_padded(es_tokenizer* t, const char* text, size_t len, int32_t* ids_out, int32_t* eos_pos_out) {
  const char* who = "es_tokenize_padded";
  if (!t || (!text && len) || !ids_out) return fail(-1, who, "null pointer");
  std::string err;
  if (!es_bpe::check_text(text, len, &err)) return fail(-1, who, err);
  std::vector<int32_t> ids;
  es_bpe::encode(&t->t, text, len, &ids);
  const int32_t ep = es_bpe::pad_row(t->t, ids, ids_out);
  if (eos_pos_out) *eos_pos_out = ep;
  return 0;
}

extern "C" void es_prompt_table_destroy(es_prompt_table* t) {
  if (!t) return;
  if (t->arena) (void)hipFree(t->arena);
  delete t;
}

extern "C" int es_prompt_table_create(es_tokenizer* tok, const char* const* words, int n_words, const int32_t* seg_ends, int nseg,
                                      const char* prefix, const char* separator, const char* suffix, int device, es_prompt_table** out) {
  const char* who = "es_prompt_table_create";
  if (out) *out = nullptr;
  if (!tok || !words || !seg_ends || !out) return fail(-1, who, "null pointer");
  if (es_plan_recording()) return fail(-1, who, kRecording);
  if (device < -1) return fail(-1, who, "device must be >= 0, or -1 for a table in host memory alone (es_prompt_assemble_host)");
  if (nseg < 1 || nseg > es_bpe::MAX_SEGMENTS) return fail(-1, who, "nseg must be in 1..4 (es_clip_score's)");
  if (n_words < 1 || n_words > (1 << 20)) return fail(-1, who, "n_words must be in 1..2^20");
  for (int s = 0; s < nseg; ++s)
    if (seg_ends[s] <= (s ? seg_ends[s - 1] : 0)) return fail(-1, who, "seg_ends must be increasing and positive");
  if (seg_ends[nseg - 1] != n_words) return fail(-1, who, "the last of seg_ends must be n_words");
  const int L = tok->t.max_length, cap = L - 2;

  // every piece, cut to the max_length - 2 ids that can ever show
  std::string err;
  auto piece = [&](const char* text, const std::string& what, std::vector<int32_t>* ids) {
    if (!text) return true;                    // an absent piece is an empty one
    const size_t n = strlen(text);
    if (!es_bpe::check_text(text, n, &err)) { err = what + ": " + err; return false; }
    es_bpe::encode(&tok->t, text, n, ids);
    if ((int)ids->size() > cap) ids->resize(cap);
    return true;
  };
  std::vector<int32_t> fixed[3];
  const char* const names[3] = {"prefix", "separator", "suffix"};
  const char* const texts[3] = {prefix, separator, suffix};
  for (int i = 0; i < 3; ++i)
    if (!piece(texts[i], names[i], &fixed[i])) return fail(-1, who, err);
  std::vector<std::vector<int32_t>> wt(n_words);
  int Lw = 1;
  for (int w = 0; w < n_words; ++w) {
    if (!words[w]) return fail(-1, who, "null pointer (word " + std::to_string(w) + ")");
    if (!piece(words[w], "word " + std::to_string(w), &wt[w])) return fail(-1, who, err);
    Lw = std::max(Lw, (int)wt[w].size());
  }

  std::unique_ptr<es_prompt_table, void (*)(es_prompt_table*)> t(new es_prompt_table, es_prompt_table_destroy);
  t->device = device; t->n_words = n_words;
  const size_t o_len = (size_t)n_words * Lw, o_fixed = o_len + n_words;
  t->store.assign(o_fixed + fixed[0].size() + fixed[1].size() + fixed[2].size() + 1, tok->t.eos);
  for (int w = 0; w < n_words; ++w) {
    std::copy(wt[w].begin(), wt[w].end(), t->store.begin() + (size_t)w * Lw);
    t->store[o_len + w] = (int32_t)wt[w].size();
  }
  size_t o = o_fixed;
  for (int i = 0; i < 3; ++i) { std::copy(fixed[i].begin(), fixed[i].end(), t->store.begin() + o); o += fixed[i].size(); }
  es_bpe::PromptView& v = t->host;
  memset(&v, 0, sizeof(v));
  v.tokens = t->store.data(); v.len = t->store.data() + o_len; v.fixed = t->store.data() + o_fixed;
  v.Lw = Lw; v.n_prefix = (int)fixed[0].size(); v.n_sep = (int)fixed[1].size(); v.n_suffix = (int)fixed[2].size();
  v.nseg = nseg;
  for (int s = 0; s < nseg; ++s) v.seg_ends[s] = seg_ends[s];
  v.bos = tok->t.bos; v.eos = tok->t.eos; v.max_length = L;
  t->dev = v;
  t->dev.tokens = t->dev.len = t->dev.fixed = nullptr;
  if (device < 0) { *out = t.release(); return 0; }

  int prev = 0;
  if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(device) != hipSuccess) return fail(-2, who, "cannot select the device");
  bool ok = hipMalloc((void**)&t->arena, t->store.size() * 4) == hipSuccess;
  ok = ok && hipMemcpy(t->arena, t->store.data(), t->store.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
  (void)hipSetDevice(prev);
  if (!ok) { (void)hipGetLastError(); return fail(-2, who, "device allocation or upload failed"); }
  t->dev.tokens = t->arena; t->dev.len = t->arena + o_len; t->dev.fixed = t->arena + o_fixed;
  *out = t.release();
  return 0;
}

extern "C" int es_prompt_assemble_host(const es_prompt_table* t, const int32_t* topk, int n, int k, int32_t* ids_out, int32_t* eos_pos) {
  const char* who = "es_prompt_assemble_host";
  if (int rc = check_assemble(who, t, topk, n, k, ids_out)) return rc;
  if (es_plan_recording()) return fail(-1, who, kRecording);
  const es_bpe::PromptView& v = t->host;
  for (int r = 0; r < n; ++r) {
    int32_t ep = 0;
    for (int pos = 0; pos < v.max_length; ++pos)
      ids_out[(size_t)r * v.max_length + pos] = es_bpe::prompt_token_at(v, topk + (size_t)r * v.nseg * k, k, pos, &ep);
    if (eos_pos) eos_pos[r] = ep;
  }
  return 0;
}

extern "C" int es_prompt_assemble(const es_prompt_table* t, const int32_t* topk_dev, int n, int k, int32_t* ids_out_dev, int32_t* eos_pos_dev,
                                  void* stream) {
  const char* who = "es_prompt_assemble";
  if (int rc = check_assemble(who, t, topk_dev, n, k, ids_out_dev)) return rc;
  if (es_plan_recording()) return fail(-1, who, kRecording);
  if (!t->arena) return fail(-1, who, "this table lives in host memory alone (es_prompt_table_create device -1): use es_prompt_assemble_host");
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev != t->device) return fail(-1, who, "the current device is not the one the table was built on");
  hipLaunchKernelGGL(prompt_assemble_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, t->dev, topk_dev, k, ids_out_dev, eos_pos_dev);
  if (ES_CHECK_LAUNCH()) return fail(-2, who, "launch failed");
  return 0;
}
