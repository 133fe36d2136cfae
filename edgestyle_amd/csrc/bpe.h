// CLIP's byte-level BPE tokenizer and the index rule of the assembled prompt row.  Pure C++17: no HIP include, so a host program can
// compile this header alone (examples/prompt_host.cpp -DPROMPT_HOST_DRY does, under a host sanitizer for instance).
//
// The rules are those of transformers' CLIPTokenizer on the `tokenizers` backend (models/clip/tokenization_clip.py):
//   normalise   NFC, every run of white space -> one space, lowercase
//   split       's|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+   (leftmost, alternatives in this order; the gaps are dropped)
//   alphabet    byte level: a printable ASCII byte is its own symbol
//   model       BPE with the end-of-word suffix </w> on the last symbol of a pre-token; a symbol that is not in the vocabulary becomes one
//               unk id (unk = pad = eos = <|endoftext|>, fuse_unk false); then the merges, lowest rank first, leftmost first - the queue of
//               tokenizers' Word::merge_all restated entry for entry, stale entries and their check included
//   row         BOS, at most max_length - 2 ids, EOS, EOS padding
// Domain: exact or refused.  Accepted bytes are 0x09-0x0D and 0x20-0x7E: NFC and lowercase are then ASCII's, \p{L} is a-z, \p{N} is 0-9
// and \s is the six bytes 0x09-0x0D, 0x20 - no Unicode tables.  A text that holds a special token's literal (in any letter case: lowercase
// makes them alike before the split, whose pattern leads with both literals) is refused too.
// A Tokenizer caches the ids of every pre-token it has seen: it is NOT thread-safe.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <queue>
#include <string>
#include <unordered_map>
#include <vector>

#if defined(__HIPCC__)
#define ES_BPE_HD __host__ __device__
#else
#define ES_BPE_HD
#endif

namespace es_bpe {

constexpr const char* BOS_TOKEN = "<|startoftext|>";
constexpr const char* EOS_TOKEN = "<|endoftext|>";
constexpr const char* END_OF_WORD = "</w>";
constexpr int MAX_SEGMENTS = 4, MAX_K = 8;

// ---- the assembled prompt row: written once, run by the kernel (one lane per position) and by es_prompt_assemble_host ------------------
// Pieces in order: prefix; for every segment s and every j < k in topk order, when topk[s * k + j] is inside [0, size of segment s):
// separator, word; suffix.  `fixed` holds the prefix, separator and suffix ids back to back.  A word's ids are tokens[w * Lw .. + len[w]).
struct PromptView {
  const int32_t* tokens;
  const int32_t* len;
  const int32_t* fixed;
  int32_t Lw, n_prefix, n_sep, n_suffix, nseg, seg_ends[MAX_SEGMENTS], bos, eos, max_length;
};

// the id at position `pos` (0 <= pos < max_length) of the row that `topk` (this row's [nseg, k] entries) selects; *eos_pos = 1 + min(total,
// max_length - 2).  An entry outside its segment is skipped and never used as an index.
ES_BPE_HD inline int32_t prompt_token_at(const PromptView& v, const int32_t* topk, int k, int pos, int32_t* eos_pos) {
  const int b = pos - 1;                       // index into the body (the pieces joined)
  int off = v.n_prefix;
  int32_t id = v.eos;
  if (b >= 0 && b < off) id = v.fixed[b];
  for (int s = 0; s < v.nseg; ++s) {
    const int start = s ? v.seg_ends[s - 1] : 0, size = v.seg_ends[s] - start;
    for (int j = 0; j < k; ++j) {
      const int32_t e = topk[s * k + j];
      if (e < 0 || e >= size) continue;
      if (b >= off && b < off + v.n_sep) id = v.fixed[v.n_prefix + (b - off)];
      off += v.n_sep;
      const int w = start + e, lw = v.len[w];
      if (b >= off && b < off + lw) id = v.tokens[(size_t)w * v.Lw + (b - off)];
      off += lw;
    }
  }
  if (b >= off && b < off + v.n_suffix) id = v.fixed[v.n_prefix + v.n_sep + (b - off)];
  off += v.n_suffix;
  const int body = off < v.max_length - 2 ? off : v.max_length - 2;
  *eos_pos = 1 + body;
  if (pos == 0) return v.bos;
  return b < body ? id : v.eos;
}

// ---- the tokenizer (host only) ------------------------------------------------------------------------------------------------------------
struct Tokenizer {
  std::unordered_map<std::string, int32_t> vocab;
  std::unordered_map<uint64_t, std::pair<uint32_t, int32_t>> merges;      // (left id << 32 | right id) -> (rank, merged id)
  int32_t sym[128], sym_end[128];              // the id of an ASCII byte as a symbol, bare and with </w>; -1: not in the vocabulary (unk)
  int32_t bos = -1, eos = -1, max_length = 0;
  std::unordered_map<std::string, std::vector<int32_t>> cache;
};

inline std::string fmt(const char* f, long long a = 0, long long b = 0) {
  char buf[160];
  snprintf(buf, sizeof(buf), f, a, b);
  return buf;
}

inline void put_utf8(std::string* s, uint32_t cp) {
  if (cp < 0x80) *s += (char)cp;
  else if (cp < 0x800) { *s += (char)(0xC0 | cp >> 6); *s += (char)(0x80 | (cp & 63)); }
  else if (cp < 0x10000) { *s += (char)(0xE0 | cp >> 12); *s += (char)(0x80 | (cp >> 6 & 63)); *s += (char)(0x80 | (cp & 63)); }
  else { *s += (char)(0xF0 | cp >> 18); *s += (char)(0x80 | (cp >> 12 & 63)); *s += (char)(0x80 | (cp >> 6 & 63)); *s += (char)(0x80 | (cp & 63)); }
}

// vocab.json: one flat object of string keys (raw UTF-8 or \uXXXX escapes, surrogate pairs included) and non-negative integers
inline bool parse_vocab(const char* p, size_t n, std::unordered_map<std::string, int32_t>* out, std::string* err) {
  size_t i = 0;
  auto ws = [&] { while (i < n && (p[i] == ' ' || p[i] == '\t' || p[i] == '\n' || p[i] == '\r')) ++i; };
  auto bad = [&](const char* what) { *err = std::string("vocab.json: ") + what + fmt(" at byte %lld", (long long)i); return false; };
  auto hex4 = [&](uint32_t* v) {
    if (i + 4 > n) return false;
    uint32_t x = 0;
    for (int k = 0; k < 4; ++k) {
      const char c = p[i + k];
      const int d = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
      if (d < 0) return false;
      x = x * 16 + (uint32_t)d;
    }
    i += 4;
    *v = x;
    return true;
  };
  if (n >= 3 && (unsigned char)p[0] == 0xEF && (unsigned char)p[1] == 0xBB && (unsigned char)p[2] == 0xBF) i = 3;      // a byte-order mark
  ws();
  if (i >= n || p[i] != '{') return bad("expected '{'");
  ++i;
  ws();
  if (i < n && p[i] == '}') { ++i; ws(); return i == n ? true : bad("text after the object"); }
  for (;;) {
    ws();
    if (i >= n || p[i] != '"') return bad("expected a string key");
    ++i;
    std::string key;
    for (;;) {
      if (i >= n) return bad("unterminated string");
      const unsigned char c = (unsigned char)p[i++];
      if (c == '"') break;
      if (c < 0x20) { --i; return bad("control character in a string"); }
      if (c != '\\') { key += (char)c; continue; }
      if (i >= n) return bad("unterminated escape");
      const char e = p[i++];
      switch (e) {
        case '"': key += '"'; break;
        case '\\': key += '\\'; break;
        case '/': key += '/'; break;
        case 'b': key += '\b'; break;
        case 'f': key += '\f'; break;
        case 'n': key += '\n'; break;
        case 'r': key += '\r'; break;
        case 't': key += '\t'; break;
        case 'u': {
          uint32_t cp = 0;
          if (!hex4(&cp)) return bad("bad \\u escape");
          if (cp >= 0xD800 && cp < 0xDC00) {          // a high surrogate: the low one must follow
            uint32_t lo = 0;
            if (i + 2 > n || p[i] != '\\' || p[i + 1] != 'u') return bad("lone surrogate in a \\u escape");
            i += 2;
            if (!hex4(&lo) || lo < 0xDC00 || lo >= 0xE000) return bad("lone surrogate in a \\u escape");
            cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00);
          } else if (cp >= 0xDC00 && cp < 0xE000) return bad("lone surrogate in a \\u escape");
          put_utf8(&key, cp);
          break;
        }
        default: --i; return bad("unknown escape");
      }
    }
    ws();
    if (i >= n || p[i] != ':') return bad("expected ':'");
    ++i;
    ws();
    long long v = 0;
    const size_t d0 = i;
    while (i < n && p[i] >= '0' && p[i] <= '9' && v < (1ll << 31)) v = v * 10 + (p[i++] - '0');
    if (i == d0 || v >= (1ll << 31)) return bad("expected an id in [0, 2^31)");
    (*out)[key] = (int32_t)v;                  // a repeated key: the last one holds
    ws();
    if (i < n && p[i] == ',') { ++i; continue; }
    if (i < n && p[i] == '}') { ++i; break; }
    return bad("expected ',' or '}'");
  }
  ws();
  return i == n ? true : bad("text after the object");
}

inline bool load(Tokenizer* t, const char* vocab_json, size_t vocab_bytes, const char* merges_txt, size_t merges_bytes, int max_length,
                 std::string* err) {
  if (max_length < 2) { *err = fmt("max_length = %lld is below 2 (BOS and EOS alone take two positions)", max_length); return false; }
  t->max_length = max_length;
  if (!parse_vocab(vocab_json, vocab_bytes, &t->vocab, err)) return false;
  auto find = [&](const std::string& s) { const auto it = t->vocab.find(s); return it == t->vocab.end() ? -1 : it->second; };
  if ((t->bos = find(BOS_TOKEN)) < 0) { *err = std::string("vocab.json: the special token '") + BOS_TOKEN + "' is missing"; return false; }
  if ((t->eos = find(EOS_TOKEN)) < 0) { *err = std::string("vocab.json: the special token '") + EOS_TOKEN + "' is missing"; return false; }
  for (int c = 0; c < 128; ++c) {
    t->sym[c] = t->sym_end[c] = -1;
    if (c < 0x21 || c > 0x7E) continue;
    t->sym[c] = find(std::string(1, (char)c));
    t->sym_end[c] = find(std::string(1, (char)c) + END_OF_WORD);
  }
  // merges.txt: one "left right" per line, lines that start with #version skipped; the rank is the order
  size_t i = 0;
  long long line_no = 0;
  uint32_t rank = 0;
  while (i < merges_bytes) {
    size_t e = i;
    while (e < merges_bytes && merges_txt[e] != '\n') ++e;
    size_t le = e;
    if (le > i && merges_txt[le - 1] == '\r') --le;
    const std::string line(merges_txt + i, le - i);
    i = e + 1;
    ++line_no;
    if (line.compare(0, 8, "#version") == 0) continue;
    const size_t sp = line.find(' ');
    if (sp == std::string::npos || sp == 0 || sp + 1 == line.size() || line.find(' ', sp + 1) != std::string::npos) {
      *err = fmt("merges.txt line %lld: expected two symbols separated by one space", line_no);
      return false;
    }
    const std::string a = line.substr(0, sp), b = line.substr(sp + 1);
    const int32_t ia = find(a), ib = find(b), iab = find(a + b);
    if (ia < 0 || ib < 0 || iab < 0) {
      *err = fmt("merges.txt line %lld: '", line_no) + (ia < 0 ? a : ib < 0 ? b : a + b) + "' is not in the vocabulary";
      return false;
    }
    t->merges[(uint64_t)(uint32_t)ia << 32 | (uint32_t)ib] = {rank++, iab};      // a repeated pair: the later line holds
  }
  return true;
}

// the first byte outside the domain, or the first special-token literal: false with the reason and the byte offset
inline bool check_text(const char* text, size_t len, std::string* err) {
  for (size_t i = 0; i < len; ++i) {
    const unsigned char c = (unsigned char)text[i];
    if (!((c >= 0x09 && c <= 0x0D) || (c >= 0x20 && c <= 0x7E))) {
      *err = fmt("byte 0x%02llX at offset %lld is outside the accepted set (0x09-0x0D, 0x20-0x7E)", c, (long long)i);
      return false;
    }
  }
  for (const char* lit : {BOS_TOKEN, EOS_TOKEN}) {
    const size_t m = strlen(lit);
    for (size_t i = 0; i + m <= len; ++i) {
      size_t k = 0;
      while (k < m && ((unsigned char)text[i + k] | (text[i + k] >= 'A' && text[i + k] <= 'Z' ? 0x20 : 0)) == (unsigned char)lit[k]) ++k;
      if (k == m) { *err = std::string("the text holds the special token literal '") + lit + fmt("' at offset %lld", (long long)i); return false; }
    }
  }
  return true;
}

// one pre-token (lowercase, bytes 0x21-0x7E) -> ids: tokenizers' BPE::merge_word and Word::merge_all
inline const std::vector<int32_t>& encode_word(Tokenizer* t, const std::string& w) {
  const auto hit = t->cache.find(w);
  if (hit != t->cache.end()) return hit->second;
  struct Sym { int32_t c; int prev, next; int len; };
  std::vector<Sym> s(w.size());
  for (size_t i = 0; i < w.size(); ++i) {
    const int c = (unsigned char)w[i];
    const int32_t id = i + 1 == w.size() ? t->sym_end[c] : t->sym[c];
    s[i] = Sym{id < 0 ? t->eos : id, (int)i - 1, i + 1 == w.size() ? -1 : (int)i + 1, 1};
  }
  struct Merge { uint32_t rank; int pos; int32_t new_id; };
  struct Later { bool operator()(const Merge& a, const Merge& b) const { return a.rank != b.rank ? a.rank > b.rank : a.pos > b.pos; } };
  std::priority_queue<Merge, std::vector<Merge>, Later> q;
  auto look = [&](int32_t a, int32_t b) -> const std::pair<uint32_t, int32_t>* {
    const auto it = t->merges.find((uint64_t)(uint32_t)a << 32 | (uint32_t)b);
    return it == t->merges.end() ? nullptr : &it->second;
  };
  for (size_t i = 0; i + 1 < s.size(); ++i)
    if (const auto* m = look(s[i].c, s[i + 1].c)) q.push(Merge{m->first, (int)i, m->second});
  while (!q.empty()) {
    const Merge top = q.top();
    q.pop();
    Sym& cur = s[top.pos];
    if (cur.len == 0 || cur.next == -1) continue;
    const Sym right = s[cur.next];
    const auto* m = look(cur.c, right.c);
    if (!m || m->second != top.new_id) continue;               // an expired entry
    s[cur.next].len = 0;
    cur.c = top.new_id; cur.len += right.len; cur.next = right.next;
    if (right.next > -1) s[right.next].prev = top.pos;
    if (cur.prev >= 0)
      if (const auto* pm = look(s[cur.prev].c, cur.c)) q.push(Merge{pm->first, cur.prev, pm->second});
    if (cur.next > -1)
      if (const auto* nm = look(cur.c, s[cur.next].c)) q.push(Merge{nm->first, top.pos, nm->second});
  }
  std::vector<int32_t> ids;
  for (const Sym& x : s)
    if (x.len) ids.push_back(x.c);
  return t->cache.emplace(w, std::move(ids)).first->second;
}

// a checked text -> ids without BOS / EOS, untruncated
inline void encode(Tokenizer* t, const char* text, size_t len, std::vector<int32_t>* out) {
  auto lower = [&](size_t i) { const char c = text[i]; return c >= 'A' && c <= 'Z' ? (char)(c + 32) : c; };
  auto space = [](char c) { return (c >= 0x09 && c <= 0x0D) || c == 0x20; };
  auto letter = [](char c) { return c >= 'a' && c <= 'z'; };
  auto digit = [](char c) { return c >= '0' && c <= '9'; };
  static const char* const contractions[] = {"'s", "'t", "'re", "'ve", "'m", "'ll", "'d"};
  std::string w;
  size_t i = 0;
  while (i < len) {
    const char c = lower(i);
    if (space(c)) { ++i; continue; }
    size_t e = i;
    if (c == '\'') {
      for (const char* ct : contractions) {
        const size_t m = strlen(ct);
        size_t k = 1;
        while (k < m && i + k < len && lower(i + k) == ct[k]) ++k;
        if (k == m) { e = i + m; break; }
      }
    }
    if (e == i) {
      if (letter(c)) { while (e < len && letter(lower(e))) ++e; }
      else if (digit(c)) e = i + 1;
      else { while (e < len && !space(lower(e)) && !letter(lower(e)) && !digit(lower(e))) ++e; }
    }
    w.clear();
    for (size_t k = i; k < e; ++k) w += lower(k);
    const std::vector<int32_t>& ids = encode_word(t, w);
    out->insert(out->end(), ids.begin(), ids.end());
    i = e;
  }
}

// the row of padding="max_length", truncation=True; returns the position of its first EOS
inline int32_t pad_row(const Tokenizer& t, const std::vector<int32_t>& ids, int32_t* row) {
  const int L = t.max_length, body = (int)ids.size() < L - 2 ? (int)ids.size() : L - 2;
  row[0] = t.bos;
  for (int i = 0; i < body; ++i) row[1 + i] = ids[i];
  for (int i = 1 + body; i < L; ++i) row[i] = t.eos;
  // an unk symbol is the EOS id too: the first EOS may come before the end of the text
  for (int i = 1; i < L; ++i)
    if (row[i] == t.eos) return i;
  return L - 1;
}

}  // namespace es_bpe
