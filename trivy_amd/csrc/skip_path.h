// utils.SkipPath (pkg/fanal/utils/utils.go:112-126) and the doublestar matcher
// behind it, shared by the FS walk (fswalk.cpp) and the layer walks
// (tar_skip.h).  Plain C++: it runs without HIP.
#pragma once
#include <cstdint>
#include <string>
#include <string_view>
#include <vector>

namespace tsg {

// One UTF-8 rune of s at i (invalid byte: itself, width 1).
inline uint32_t RuneAt(std::string_view s, size_t i, size_t* w) {
  const uint8_t b = uint8_t(s[i]);
  auto cont = [&](size_t k) { return i + k < s.size() && (uint8_t(s[i + k]) & 0xC0) == 0x80; };
  if (b < 0x80) {
    *w = 1;
    return b;
  }
  if ((b & 0xE0) == 0xC0 && cont(1)) {
    *w = 2;
    return ((b & 0x1Fu) << 6) | (uint8_t(s[i + 1]) & 0x3Fu);
  }
  if ((b & 0xF0) == 0xE0 && cont(1) && cont(2)) {
    *w = 3;
    return ((b & 0x0Fu) << 12) | ((uint8_t(s[i + 1]) & 0x3Fu) << 6) | (uint8_t(s[i + 2]) & 0x3Fu);
  }
  if ((b & 0xF8) == 0xF0 && cont(1) && cont(2) && cont(3)) {
    *w = 4;
    return ((b & 0x07u) << 18) | ((uint8_t(s[i + 1]) & 0x3Fu) << 12) | ((uint8_t(s[i + 2]) & 0x3Fu) << 6) |
           (uint8_t(s[i + 3]) & 0x3Fu);
  }
  *w = 1;
  return b;
}

// doublestar.Match (github.com/bmatcuk/doublestar/v4, the matcher behind
// utils.SkipPath): '*' any run of non-'/' characters, '?' one non-'/'
// character, '[...]' a class ('!' or '^' negates, a-z ranges, '\' escapes),
// '{a,b}' alternatives, '\' escapes, and '**' as a whole path component zero
// or more directories ("a/**" also matches "a").  Returns -1 for a malformed
// pattern (ErrBadPattern: SkipPath then stops and reports false).
inline int DoubleStarMatch(std::string_view p, std::string_view s) {
  size_t i = 0;
  while (i < p.size()) {
    const char c = p[i];
    const bool comp_start = i == 0 || p[i - 1] == '/';
    if (c == '*' && comp_start && i + 1 < p.size() && p[i + 1] == '*' && (i + 2 == p.size() || p[i + 2] == '/')) {
      if (i + 2 == p.size()) return 1;  // trailing "**": everything below
      const std::string_view rest = p.substr(i + 3);
      for (size_t k = 0;;) {  // zero or more leading components of s
        const int r = DoubleStarMatch(rest, s.substr(k));
        if (r != 0) return r;
        const size_t sl = s.find('/', k);
        if (sl == std::string_view::npos) return 0;
        k = sl + 1;
      }
    }
    if (c == '/' && s.empty() && p.substr(i) == "/**") return 1;  // "a/**" matches "a"
    if (c == '*') {  // a run of '*' that is not a whole "**" component is one '*'
      size_t j = i;
      while (j < p.size() && p[j] == '*') j++;
      const std::string_view rest = p.substr(j);
      for (;;) {
        const int r = DoubleStarMatch(rest, s);
        if (r != 0) return r;
        if (s.empty() || s[0] == '/') return 0;
        size_t w;
        RuneAt(s, 0, &w);
        s.remove_prefix(w);
      }
    }
    if (c == '{') {  // alternatives up to the matching '}' (nesting allowed)
      size_t depth = 0, j = i, start = i + 1;
      std::vector<std::string_view> alts;
      for (; j < p.size(); j++) {
        if (p[j] == '\\') {
          j++;
          continue;
        }
        if (p[j] == '{') {
          depth++;
        } else if (p[j] == '}' && --depth == 0) {
          break;
        } else if (p[j] == ',' && depth == 1) {
          alts.push_back(p.substr(start, j - start));
          start = j + 1;
        }
      }
      if (j >= p.size()) return -1;
      alts.push_back(p.substr(start, j - start));
      const std::string_view rest = p.substr(j + 1);
      int bad = 0;
      for (auto a : alts) {
        std::string q(p.substr(0, 0));
        q.append(a.data(), a.size());
        q.append(rest.data(), rest.size());
        const int r = DoubleStarMatch(q, s);
        if (r == 1) return 1;
        if (r < 0) bad = -1;
      }
      return bad;
    }
    if (s.empty()) {
      if (c == '[' && p.find(']', i + 1) == std::string_view::npos) return -1;
      if (c == '\\' && i + 1 >= p.size()) return -1;
      return 0;
    }
    size_t w;
    const uint32_t r = RuneAt(s, 0, &w);
    if (c == '?') {
      if (r == '/') return 0;
      i++;
      s.remove_prefix(w);
      continue;
    }
    if (c == '[') {
      size_t j = i + 1;
      bool neg = false;
      if (j < p.size() && (p[j] == '!' || p[j] == '^')) {
        neg = true;
        j++;
      }
      bool hit = false, first = true;
      for (;;) {
        if (j >= p.size()) return -1;
        if (p[j] == ']' && !first) break;
        first = false;
        size_t cw;
        uint32_t lo;
        if (p[j] == '\\') {
          if (j + 1 >= p.size()) return -1;
          lo = RuneAt(p, j + 1, &cw);
          j += 1 + cw;
        } else {
          lo = RuneAt(p, j, &cw);
          j += cw;
        }
        uint32_t hi = lo;
        if (j + 1 < p.size() && p[j] == '-' && p[j + 1] != ']') {
          size_t hw;
          if (p[j + 1] == '\\') {
            if (j + 2 >= p.size()) return -1;
            hi = RuneAt(p, j + 2, &hw);
            j += 2 + hw;
          } else {
            hi = RuneAt(p, j + 1, &hw);
            j += 1 + hw;
          }
        }
        if (lo <= r && r <= hi) hit = true;
      }
      if (r == '/' || hit == neg) return 0;
      i = j + 1;
      s.remove_prefix(w);
      continue;
    }
    uint32_t want;
    size_t pw;
    if (c == '\\') {
      if (i + 1 >= p.size()) return -1;
      want = RuneAt(p, i + 1, &pw);
      pw += 1;
    } else {
      want = RuneAt(p, i, &pw);
    }
    if (want != r) return 0;
    i += pw;
    s.remove_prefix(w);
  }
  return s.empty() ? 1 : 0;
}

// doublestar.ValidatePattern: brackets and braces closed, no trailing '\'.
inline bool DoubleStarValid(std::string_view p) {
  int brace = 0;
  for (size_t i = 0; i < p.size(); i++) {
    if (p[i] == '\\') {
      if (++i >= p.size()) return false;
    } else if (p[i] == '[') {
      size_t j = i + 1;
      if (j < p.size() && (p[j] == '!' || p[j] == '^')) j++;
      if (j < p.size() && p[j] == ']') j++;  // a leading ']' is a member
      while (j < p.size() && p[j] != ']') j += p[j] == '\\' ? 2 : 1;
      if (j >= p.size()) return false;
      i = j;
    } else if (p[i] == '{') {
      brace++;
    } else if (p[i] == '}' && brace > 0) {
      brace--;
    }
  }
  return brace == 0;
}

// doublestar.Match: on a mismatch the pattern is validated (ErrBadPattern -> -1).
inline int DoubleStarMatchChecked(std::string_view p, std::string_view s) {
  const int r = DoubleStarMatch(p, s);
  return r == 0 && !DoubleStarValid(p) ? -1 : r;
}

// utils.SkipPath (utils.go:112-126).
inline bool SkipPath(std::string_view path, const std::vector<std::string>& pats) {
  while (!path.empty() && path[0] == '/') path.remove_prefix(1);
  for (const auto& p : pats) {
    const int m = DoubleStarMatchChecked(p, path);
    if (m < 0) return false;  // a bad pattern ends the check
    if (m == 1) return true;
  }
  return false;
}

}  // namespace tsg
