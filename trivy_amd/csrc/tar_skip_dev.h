// LayerTar's skipDirs / skipFiles patterns in the forms the GPU stage of a resident layer's
// index takes (tarrequired.hip; tsg_analyzer_set_tar_required_skip mode 1).  Plain C++: the
// classifier runs on the host when the options are set, the matcher is shared with the
// kernels (TSG_HD), and both run without HIP.
//
// A cleaned pattern is device-decidable when it is one of
//
//   L        fp == L
//   **/L     fp == L, or fp ends with "/" + L
//   L/**     fp == L, or fp starts with L + "/"
//   **/*S    the base name of fp ends with S
//
// with L a non-empty ASCII literal of at most 255 bytes that holds none of * ? [ ] { } \ and
// whose '/'-separated elements are neither empty nor "." nor ".." (so it neither begins nor
// ends with '/'), and S such a literal without '/'.
//
// Why byte compares are doublestar.Match (skip_path.h: DoubleStarMatch) for these forms.  The
// matcher walks pattern and path rune by rune (RuneAt: an invalid byte is a rune of width 1).
// A multi-byte rune is a lead byte >= 0xC0 and continuation bytes 0x80..0xBF: an ASCII byte is
// never swallowed as a continuation byte, so every ASCII byte of the path begins a rune, and a
// rune of an ASCII literal equals a rune of the path only when that rune is the same single
// byte.  Matching L against a stretch of the path is therefore byte equality.  "**/" tries the
// rest of the pattern at every element start of the path: L must equal a whole suffix made of
// elements.  "/**" after L takes "" or "/" and anything.  In "**/*S" the '*' steps over runes
// that are no '/', and then S must match to the end of the path: the stretch is one element,
// the base name; the position where S begins holds an ASCII byte, so the rune walk stops
// there, and the base name ending with S is the whole condition.  As S has no '/', fp ending
// with S says the same.  Every accepted pattern is valid, so SkipPath's rule that a bad
// pattern ends the check cannot arise, and the patterns may be tried in any order.
//
// If a pattern of an option set is outside the forms, or the set outside the caps (32
// directory patterns, 32 file patterns, 2 KiB of literal bytes), the whole set is: the host
// half runs (tsg_tar_required_skip_stats.reason 3).
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <string_view>
#include <vector>

#if defined(__HIPCC__)
#define TSG_HD __host__ __device__
#else
#define TSG_HD
#endif

namespace tsg {

constexpr uint32_t kTarSkipMaxPatterns = 32;    // of either kind
constexpr uint32_t kTarSkipMaxLiteral = 255;
constexpr uint32_t kTarSkipMaxBytes = 2048;     // all literals together

enum : uint8_t { kSkipFormExact = 0, kSkipFormAnyDir = 1, kSkipFormBelow = 2, kSkipFormSuffix = 3 };

struct TarSkipPat {
  uint16_t off;  // of the literal in TarSkipTable::bytes
  uint8_t len;   // 1..255
  uint8_t form;
};
// What the kernels stage in LDS: the directory patterns, then the file patterns.
struct TarSkipTable {
  uint32_t n_dir = 0, n_file = 0;
  TarSkipPat pat[2 * kTarSkipMaxPatterns] = {};  // [0, n_dir) directories, [32, 32 + n_file) files
  uint8_t bytes[kTarSkipMaxBytes] = {};
};
static_assert(sizeof(TarSkipTable) == 8 + 256 + 2048 && sizeof(TarSkipTable) % 4 == 0, "staged as 4-B words");

// The literal of form L / S: see above.
inline bool TarSkipLiteralOk(std::string_view l, bool slashes) {
  if (l.empty() || l.size() > kTarSkipMaxLiteral) return false;
  size_t es = 0;
  for (size_t i = 0; i <= l.size(); i++) {
    if (i < l.size()) {
      const uint8_t c = uint8_t(l[i]);
      if (c >= 0x80 || c == '*' || c == '?' || c == '[' || c == ']' || c == '{' || c == '}' || c == '\\') return false;
      if (c != '/') continue;
      if (!slashes) return false;
    }
    const std::string_view e = l.substr(es, i - es);
    if (e.empty() || e == "." || e == "..") return false;
    es = i + 1;
  }
  return true;
}

// The form of one cleaned pattern and its literal; false: the device does not take it.
inline bool TarSkipForm(std::string_view p, uint8_t* form, std::string_view* lit) {
  if (p.substr(0, 4) == "**/*") {
    *form = kSkipFormSuffix;
    *lit = p.substr(4);
    return TarSkipLiteralOk(*lit, false);
  }
  if (p.substr(0, 3) == "**/") {
    *form = kSkipFormAnyDir;
    *lit = p.substr(3);
  } else if (p.size() > 3 && p.substr(p.size() - 3) == "/**") {
    *form = kSkipFormBelow;
    *lit = p.substr(0, p.size() - 3);
  } else {
    *form = kSkipFormExact;
    *lit = p;
  }
  return TarSkipLiteralOk(*lit, true);
}

// The table of an option set; false (the table is left empty): a pattern or the set is outside
// what the device takes.
inline bool TarSkipClassify(const std::vector<std::string>& dirs, const std::vector<std::string>& files,
                            TarSkipTable* t) {
  *t = TarSkipTable();
  if (dirs.size() > kTarSkipMaxPatterns || files.size() > kTarSkipMaxPatterns) return false;
  TarSkipTable w;
  size_t at = 0;
  for (int kind = 0; kind < 2; kind++) {
    const std::vector<std::string>& ps = kind ? files : dirs;
    for (size_t k = 0; k < ps.size(); k++) {
      uint8_t form;
      std::string_view lit;
      if (!TarSkipForm(ps[k], &form, &lit) || at + lit.size() > kTarSkipMaxBytes) return false;
      std::memcpy(w.bytes + at, lit.data(), lit.size());
      w.pat[kind * kTarSkipMaxPatterns + k] = TarSkipPat{uint16_t(at), uint8_t(lit.size()), form};
      at += lit.size();
    }
  }
  w.n_dir = uint32_t(dirs.size());
  w.n_file = uint32_t(files.size());
  *t = w;
  return true;
}

// One pattern of a table against a cleaned path (no leading '/', not empty).
TSG_HD inline bool TarSkipMatchOne(const TarSkipPat p, const uint8_t* bytes, const uint8_t* fp, uint32_t len) {
  const uint32_t l = p.len;
  if (len < l) return false;
  uint32_t at = 0;  // where the literal must stand in fp
  if (p.form == kSkipFormExact) {
    if (len != l) return false;
  } else if (p.form == kSkipFormAnyDir) {
    at = len - l;
    if (at && fp[at - 1] != '/') return false;
  } else if (p.form == kSkipFormBelow) {
    if (len > l && fp[l] != '/') return false;
  } else {
    at = len - l;
  }
  const uint8_t* lit = bytes + p.off;
  for (uint32_t k = 0; k < l; k++)
    if (fp[at + k] != lit[k]) return false;
  return true;
}

// SkipPath(fp, the set's directory patterns / file patterns).
TSG_HD inline bool TarSkipMatch(const TarSkipTable* t, bool files, const uint8_t* fp, uint32_t len) {
  const uint32_t n = files ? t->n_file : t->n_dir;
  const TarSkipPat* p = t->pat + (files ? kTarSkipMaxPatterns : 0);
  for (uint32_t k = 0; k < n && k < kTarSkipMaxPatterns; k++)
    if (TarSkipMatchOne(p[k], t->bytes, fp, len)) return true;
  return false;
}

}  // namespace tsg
