// The small readers the compiled hosts share (examples/checkpoint_host.cpp, examples/text_host.cpp): a JSON parser just large enough for
// safetensors headers and config.json, and a memory-mapped safetensors file described as es_tensor descriptors (include/edgestyle_hip.h).
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "edgestyle_hip.h"

// ---- a JSON reader just large enough for safetensors headers and config.json ---------------------------------------------
struct Json {
  enum Kind { Null, Bool, Num, Str, Arr, Obj } kind = Null;
  double num = 0; bool b = false; std::string str;
  std::vector<Json> arr;
  std::vector<std::pair<std::string, Json>> obj;
  const Json* get(const std::string& k) const { for (auto& kv : obj) if (kv.first == k) return &kv.second; return nullptr; }
};
struct JsonParser {
  const char* p; const char* e;
  [[noreturn]] void bad(const char* m) { fprintf(stderr, "json: %s\n", m); exit(4); }
  void ws() { while (p < e && (*p == ' ' || *p == '\n' || *p == '\t' || *p == '\r')) ++p; }
  std::string string() {
    std::string s;
    if (*p != '"') bad("string expected");
    for (++p; p < e && *p != '"'; ++p) {
      if (*p == '\\' && p + 1 < e) { ++p; s += (*p == 'n' ? '\n' : *p == 't' ? '\t' : *p); } else s += *p;
    }
    if (p >= e) bad("unterminated string");
    ++p;
    return s;
  }
  Json value() {
    ws();
    if (p >= e) bad("unexpected end");
    Json j;
    if (*p == '{') {
      j.kind = Json::Obj; ++p; ws();
      if (*p == '}') { ++p; return j; }
      for (;;) {
        ws(); std::string k = string(); ws();
        if (*p != ':') bad("':' expected");
        ++p;
        j.obj.emplace_back(k, value()); ws();
        if (*p == ',') { ++p; continue; }
        if (*p == '}') { ++p; return j; }
        bad("',' or '}' expected");
      }
    }
    if (*p == '[') {
      j.kind = Json::Arr; ++p; ws();
      if (*p == ']') { ++p; return j; }
      for (;;) {
        j.arr.push_back(value()); ws();
        if (*p == ',') { ++p; continue; }
        if (*p == ']') { ++p; return j; }
        bad("',' or ']' expected");
      }
    }
    if (*p == '"') { j.kind = Json::Str; j.str = string(); return j; }
    if (!strncmp(p, "true", 4)) { j.kind = Json::Bool; j.b = true; p += 4; return j; }
    if (!strncmp(p, "false", 5)) { j.kind = Json::Bool; p += 5; return j; }
    if (!strncmp(p, "null", 4)) { p += 4; return j; }
    char* end = nullptr;
    j.kind = Json::Num; j.num = strtod(p, &end);
    if (end == p) bad("value expected");
    p = end;
    return j;
  }
};
static Json parse_json(const char* data, size_t n) { JsonParser q{data, data + n}; return q.value(); }

// ---- safetensors: u64 header length, JSON header {key: {dtype, shape, data_offsets}}, raw little-endian data -------------------
struct SafeTensors {
  void* map = nullptr; size_t bytes = 0;
  std::vector<std::string> keys;            // owns the key strings the descriptors point at
  std::vector<es_tensor> tensors;
  // skip_other_dtypes: entries that are not F32 / F16 / BF16 (an int64 position_ids buffer) are left out instead of refused
  bool open(const std::string& path, bool skip_other_dtypes = false) {
    const int fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0) { perror(path.c_str()); return false; }
    struct stat st;
    if (fstat(fd, &st) != 0) { close(fd); return false; }
    bytes = (size_t)st.st_size;
    map = mmap(nullptr, bytes, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (map == MAP_FAILED || bytes < 8) { fprintf(stderr, "%s: cannot map\n", path.c_str()); return false; }
    uint64_t hl;
    memcpy(&hl, map, 8);
    if (hl > bytes - 8) { fprintf(stderr, "%s: bad header length\n", path.c_str()); return false; }
    const Json h = parse_json((const char*)map + 8, (size_t)hl);
    const char* data = (const char*)map + 8 + hl;
    keys.reserve(h.obj.size());
    for (const auto& kv : h.obj) {
      if (kv.first == "__metadata__") continue;
      const Json *dt = kv.second.get("dtype"), *sh = kv.second.get("shape"), *of = kv.second.get("data_offsets");
      if (!dt || !sh || !of || of->arr.size() != 2 || sh->arr.size() > 4) { fprintf(stderr, "%s: entry '%s' not understood\n", path.c_str(), kv.first.c_str()); return false; }
      es_tensor t;
      memset(&t, 0, sizeof(t));
      t.dtype = dt->str == "F32" ? ES_F32 : dt->str == "F16" ? ES_F16 : dt->str == "BF16" ? ES_BF16 : -1;
      if (t.dtype < 0 && skip_other_dtypes) continue;
      if (t.dtype < 0) { fprintf(stderr, "%s: '%s' has dtype %s (F32 / F16 / BF16 only)\n", path.c_str(), kv.first.c_str(), dt->str.c_str()); return false; }
      t.ndim = (int32_t)sh->arr.size();
      size_t n = t.dtype == ES_F32 ? 4 : 2;
      for (int i = 0; i < t.ndim; ++i) { t.shape[i] = (int64_t)sh->arr[i].num; n *= (size_t)t.shape[i]; }
      if (t.ndim == 0) { t.ndim = 1; t.shape[0] = 1; }          // a scalar (CLIPModel's logit_scale) is described as [1]
      const size_t a = (size_t)of->arr[0].num, b = (size_t)of->arr[1].num;
      if (b - a != n || 8 + hl + b > bytes) { fprintf(stderr, "%s: '%s' lies outside the file\n", path.c_str(), kv.first.c_str()); return false; }
      t.data = data + a;
      keys.push_back(kv.first);
      tensors.push_back(t);
    }
    for (size_t i = 0; i < tensors.size(); ++i) tensors[i].key = keys[i].c_str();
    return true;
  }
  es_state_dict dict() const { return es_state_dict{tensors.data(), (int32_t)tensors.size()}; }
};

static bool read_file(const std::string& path, std::string& out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) { perror(path.c_str()); return false; }
  char buf[4096]; size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) out.append(buf, n);
  fclose(f);
  return true;
}
static double num(const Json& j, const char* k, double dflt) { const Json* v = j.get(k); return v && v->kind == Json::Num ? v->num : dflt; }
