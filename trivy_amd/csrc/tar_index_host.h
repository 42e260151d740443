// The tar walk's reading of headers (Go 1.22 archive/tar/reader.go semantics;
// LayerTar.Walk's path logic, pkg/fanal/walker/tar.go:41-84), written over a
// block accessor so that the same code walks a layer held in host memory
// (analyzer.cpp: HostTarSrc, a pointer) and one resident in HBM, of which the
// host holds only the blocks that parse as headers (tarindex.hip's records:
// IndexedTarSrc) -- and the host half of the resident layer's index and of its
// batches (device_layer.cpp).  Plain C++: it runs without HIP.
//
// A source gives
//   const uint8_t* Block(uint64_t p)             the 512 bytes at p (p + 512 <= n); NULL: failed, error set
//   const uint8_t* Range(uint64_t off, uint64_t len)   the bytes [off, off + len) (inside the layer); NULL: failed
//   bool failed()                                a Block / Range failed (never a host layer)
//   const uint8_t* base()                        the layer buffer of a kView source, else NULL
//   kView          the pointers are into the one layer buffer, so an entry may
//                  keep its name as (offset, length) instead of a string
#pragma once
#include <immintrin.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <string_view>
#include <vector>

#include "tar_skip.h"
#include "tarchain.h"
#include "tsg_analyzer.h"

namespace tsg {
void SetError(const std::string& e);

// True when path.Clean(p) == p: no empty, "." or ".." element, no trailing
// slash (other than the root itself).  Most archive names already are clean.
inline bool GoPathIsClean(const char* p, size_t n) {
  if (n == 0) return false;
  if (n == 1) return p[0] != '.';
  if (p[n - 1] == '/') return false;
  size_t s = 0;  // element start
  for (size_t i = 0; i <= n; i++) {
    if (i < n && p[i] != '/') continue;
    const size_t len = i - s;
    if (len == 0 && i != 0) return false;                      // "//" (a leading '/' is the root)
    if (len == 1 && p[s] == '.') return false;                 // "."
    if (len == 2 && p[s] == '.' && p[s + 1] == '.') return false;  // ".."
    s = i + 1;
  }
  return true;
}

// path.Clean (Go, slash-separated).
inline std::string GoPathClean(const std::string& path) {
  if (path.empty()) return ".";
  if (GoPathIsClean(path.data(), path.size())) return path;
  const bool rooted = path[0] == '/';
  const size_t n = path.size();
  std::string out;
  out.reserve(n + 1);
  size_t r = 0, dotdot = 0;
  if (rooted) {
    out.push_back('/');
    r = dotdot = 1;
  }
  while (r < n) {
    if (path[r] == '/') {
      r++;
    } else if (path[r] == '.' && (r + 1 == n || path[r + 1] == '/')) {
      r++;
    } else if (path[r] == '.' && path[r + 1] == '.' && (r + 2 == n || path[r + 2] == '/')) {
      r += 2;
      if (out.size() > dotdot) {  // back to the last '/' at or after dotdot (Go: w--, then while out[w] != '/')
        size_t w = out.size() - 1;
        while (w > dotdot && out[w] != '/') w--;
        out.resize(w);
      } else if (!rooted) {
        if (!out.empty()) out.push_back('/');
        out += "..";
        dotdot = out.size();
      }
    } else {
      if ((rooted && out.size() != 1) || (!rooted && !out.empty())) out.push_back('/');
      for (; r < n && path[r] != '/'; r++) out.push_back(path[r]);
    }
  }
  if (out.empty()) return ".";
  return out;
}

// ---- archive/tar header reading (Go 1.22 archive/tar/reader.go semantics) ----
inline bool AllZero(const uint8_t* b) {
  uint64_t acc;
  std::memcpy(&acc, b, 8);  // a header starts with its name: almost always decided here
  if (acc) return false;
  for (int i = 0; i < 64; i++) {
    uint64_t w;
    std::memcpy(&w, b + 8 * i, 8);
    acc |= w;
  }
  return acc == 0;
}
inline std::string CStr(const uint8_t* b, size_t n) {  // parseString: up to the first NUL
  size_t k = 0;
  while (k < n && b[k]) k++;
  return std::string(reinterpret_cast<const char*>(b), k);
}
inline bool ParseNumeric(const uint8_t* b, size_t n, int64_t* out) {  // parseNumeric
  if (n > 0 && (b[0] & 0x80)) {  // base-256 (two's complement, big-endian)
    const bool neg = b[0] & 0x40;
    uint64_t v = 0;
    for (size_t i = 0; i < n; i++) {
      uint8_t c = i == 0 ? (b[0] & 0x7F) : b[i];
      if (neg) c ^= 0xFF;
      if (i == 0 && neg) c &= 0x7F;
      if (v >> 56) return false;
      v = (v << 8) | c;
    }
    if (v >> 63) return false;
    *out = neg ? -int64_t(v) - 1 : int64_t(v);
    return true;
  }
  // parseOctal: trim spaces and NULs at both ends
  size_t lo = 0, hi = n;
  while (lo < hi && (b[lo] == ' ' || b[lo] == 0)) lo++;
  while (hi > lo && (b[hi - 1] == ' ' || b[hi - 1] == 0)) hi--;
  int64_t v = 0;
  for (size_t i = lo; i < hi; i++) {
    if (b[i] < '0' || b[i] > '7') return false;
    if (v >> 60) return false;
    v = v * 8 + (b[i] - '0');
  }
  *out = v;
  return true;
}
inline bool ChecksumOK(const uint8_t* b) {
  int64_t want = 0;
  if (!ParseNumeric(b + 148, 8, &want)) return false;
  // the unsigned byte sum with the checksum field read as spaces, else the
  // signed one (old writers); plain loops, vectorised by the compiler
  __m256i acc = _mm256_setzero_si256();  // unsigned sum: psadbw against zero, 32 B a step
  for (int i = 0; i < 512; i += 32)
    acc = _mm256_add_epi64(acc, _mm256_sad_epu8(_mm256_loadu_si256(reinterpret_cast<const __m256i*>(b + i)),
                                                 _mm256_setzero_si256()));
  int32_t u = int32_t(_mm256_extract_epi64(acc, 0) + _mm256_extract_epi64(acc, 1) + _mm256_extract_epi64(acc, 2) +
                      _mm256_extract_epi64(acc, 3));
  for (int i = 148; i < 156; i++) u += ' ' - b[i];
  if (want == u) return true;
  int32_t s = 0;
  for (int i = 0; i < 512; i++) s += int8_t(b[i]);
  for (int i = 148; i < 156; i++) s += ' ' - int8_t(b[i]);
  return want == s;
}
// PAX records "%d %s=%s\n" (parsePAX): path, size and linkpath matter here.
inline bool ParsePax(const uint8_t* d, uint64_t n, std::string* path, int64_t* size, bool* has_path, bool* has_size) {
  uint64_t p = 0;
  while (p < n) {
    uint64_t sp = p;
    while (sp < n && d[sp] != ' ') sp++;
    if (sp >= n) return false;
    uint64_t len = 0;
    for (uint64_t i = p; i < sp; i++) {
      if (d[i] < '0' || d[i] > '9') return false;
      len = len * 10 + (d[i] - '0');
    }
    if (len < sp - p + 2 || p + len > n || d[p + len - 1] != '\n') return false;
    const std::string rec(reinterpret_cast<const char*>(d + sp + 1), size_t(len - (sp + 1 - p) - 1));
    const size_t eq = rec.find('=');
    if (eq == std::string::npos) return false;
    const std::string k = rec.substr(0, eq), v = rec.substr(eq + 1);
    if (k == "path") {
      *path = v;
      *has_path = true;
    } else if (k == "size") {
      char* e = nullptr;
      *size = std::strtoll(v.c_str(), &e, 10);
      if (v.empty() || *e) return false;
      *has_size = true;
    }
    p += len;
  }
  return true;
}
inline bool HeaderOnly(char t) { return t == '1' || t == '2' || t == '3' || t == '4' || t == '5' || t == '6'; }

// One archive entry as the walk sees it (header chain resolved).
struct TarEntry {
  uint64_t start, next;  // header chain start, next entry
  uint64_t hdr;          // the entry's own header
  uint64_t data, size;   // content
  uint64_t long_off, long_len;  // GNU 'L' long name data (long_len == ~0: none)
  uint8_t what;          // 0 other, 1 whiteout, 2 opaque dir, 3 regular file
  uint8_t has_pax_path;
  uint8_t bad;           // the entry header's checksum is wrong (checked on the threads)
  uint8_t dir = 0;       // TypeDir (typeflag '5', or TypeRegA with a resolved name ending in '/'), no marker
  uint8_t skip = 0;      // kTarSkip*: LayerTar's skipDirs / skipFiles (tar_skip.h)
  // The cleaned path (walker/tar.go:46-48): a view of the header's name field
  // in the archive itself when that is already the answer (a ustar name with
  // no prefix, clean; sources with kView only), else an owned string (PAX /
  // GNU long names, prefixes, names that Clean changes) -- no allocation per
  // entry on the common path.
  std::unique_ptr<std::string> fp_own;  // set: the path is *fp_own
  uint64_t fp_off = 0;
  uint32_t fp_len = 0;
  std::string_view path(const uint8_t* tar) const {
    return fp_own ? std::string_view(*fp_own) : std::string_view(reinterpret_cast<const char*>(tar + fp_off), fp_len);
  }
  void own(std::string v) { fp_own.reset(new std::string(std::move(v))); }
  // filled by the parallel pass
  uint8_t state;         // 0 not required, 1 binary skipped, 2 add
  uint8_t bin;
  uint64_t out_len, out_off;
};

// A layer in host memory.
struct HostTarSrc {
  static constexpr bool kView = true;
  const uint8_t* tar;
  const uint8_t* base() const { return tar; }
  bool failed() const { return false; }
  const uint8_t* Block(uint64_t p) const { return tar + p; }
  const uint8_t* Range(uint64_t off, uint64_t) const { return tar + off; }
};

// Sequential step of the walk: hop over the header chain starting at p using
// only what decides the next entry's position (zero block, typeflag, size,
// PAX size).  Extended headers are checked here (rare); the entry header's
// checksum and name are resolved later (ResolveT).
// 0 = entry read, 1 = end of archive, <0 = malformed.
template <class Src>
int ChainEntryT(const Src& src, uint64_t n, uint64_t p, TarEntry* e) {
  e->start = p;
  e->long_len = ~uint64_t(0);
  e->has_pax_path = 0;
  std::string pax_path;
  bool has_pax_path = false, has_pax_size = false;
  int64_t pax_size = 0, size = 0;
  const uint8_t* h = nullptr;
  char type = 0;
  for (;;) {
    if (p + 512 > n) {
      if (p >= n) return 1;  // io.EOF without the zero blocks
      SetError("tar: truncated header");
      return -1;
    }
    h = src.Block(p);
    if (!h) return -1;
    if (AllZero(h)) return 1;  // end-of-archive marker
    type = char(h[156]);
    if (!ParseNumeric(h + 124, 12, &size) || size < 0) {
      SetError("tar: invalid size field");
      return -1;
    }
    const uint64_t dsz = HeaderOnly(type) ? 0 : uint64_t(size);
    const uint64_t data = p + 512;
    if (data + dsz > n) {
      SetError("tar: truncated entry data");
      return -1;
    }
    if (type != 'x' && type != 'L' && type != 'K') break;
    if (!ChecksumOK(h)) {
      SetError("tar: invalid header checksum at offset " + std::to_string(p));
      return -1;
    }
    if (type == 'x') {
      const uint8_t* d = src.Range(data, dsz);
      if (!d) return -1;
      if (!ParsePax(d, dsz, &pax_path, &pax_size, &has_pax_path, &has_pax_size)) {
        SetError("tar: invalid PAX record");
        return -1;
      }
    }
    if (type == 'L') {
      e->long_off = data;
      e->long_len = dsz;
    }
    p = data + ((dsz + 511) & ~uint64_t(511));
  }
  e->hdr = p;
  if (has_pax_size) size = pax_size;
  if (type == '\0') {  // TypeRegA: a directory when the name ends in '/' (resolved name: ResolveT)
    type = '0';
  }
  const uint64_t dsz = HeaderOnly(type) ? 0 : uint64_t(size);
  e->data = p + 512;
  if (e->data + dsz > n) {
    SetError("tar: truncated entry data");
    return -1;
  }
  e->size = dsz;
  e->next = e->data + ((dsz + 511) & ~uint64_t(511));
  e->what = type == '0' ? 3 : 0;
  if (has_pax_path) {
    e->own(std::move(pax_path));
    e->has_pax_path = 1;
  }
  return 0;
}

// The entry's name (ustar prefix, GNU long name, PAX path) and header checksum.
// Returns the entry's header (NULL: the source failed; the entry is marked bad).
template <class Src>
const uint8_t* ResolveT(const Src& src, TarEntry* e) {
  const uint8_t* h = src.Block(e->hdr);
  if (!h) {
    e->bad = 1;
    e->own(std::string());
    return nullptr;
  }
  e->bad = ChecksumOK(h) ? 0 : 1;
  if (e->has_pax_path) return h;
  if (e->long_len != ~uint64_t(0)) {
    const uint8_t* d = src.Range(e->long_off, e->long_len);
    if (!d) {
      e->bad = 1;
      e->own(std::string());
      return nullptr;
    }
    e->own(CStr(d, size_t(e->long_len)));
  } else {
    auto clen = [](const uint8_t* b, size_t n) {
      const void* z = std::memchr(b, 0, n);
      return z ? size_t(static_cast<const uint8_t*>(z) - b) : n;
    };
    const size_t nl = clen(h, 100);
    size_t pl = 0;
    if (std::memcmp(h + 257, "ustar\0", 6) == 0 && std::memcmp(h + 263, "00", 2) == 0) pl = clen(h + 345, 155);
    if (pl) {
      std::string v;
      v.reserve(pl + 1 + nl);
      v.append(reinterpret_cast<const char*>(h + 345), pl);
      v.push_back('/');
      v.append(reinterpret_cast<const char*>(h), nl);
      e->own(std::move(v));
    } else if constexpr (Src::kView) {
      e->fp_own.reset();
      e->fp_off = e->hdr;
      e->fp_len = uint32_t(nl);
    } else {
      e->own(std::string(reinterpret_cast<const char*>(h), nl));
    }
  }
  return h;
}

// LayerTar.Walk's per-entry path logic (walker/tar.go:41-84): clean the name,
// classify whiteout / opaque markers.  `tar`: the layer buffer of a kView
// source (what TarEntry::path reads), else NULL.  ClassifyPath is the part after
// the name is resolved (typeflag: the header's).
inline void ClassifyPath(uint8_t typeflag, const uint8_t* tar, TarEntry* e) {
  std::string_view fp = e->path(tar);
  e->dir = typeflag == '5';
  e->skip = 0;
  if (typeflag == '\0' && !fp.empty() && fp.back() == '/') {  // TypeRegA dir
    e->what = 0;
    e->dir = 1;
  }
  if (!GoPathIsClean(fp.data(), fp.size())) {
    e->own(GoPathClean(std::string(fp)));
    fp = *e->fp_own;
  }
  size_t t = 0;
  while (t < fp.size() && fp[t] == '/') t++;
  if (t) {
    if (e->fp_own) {
      e->fp_own->erase(0, t);
    } else {
      e->fp_off += t;
      e->fp_len -= uint32_t(t);
    }
    fp = e->path(tar);
  }
  const size_t slash = fp.rfind('/');
  const std::string_view file_name = fp.substr(slash == std::string_view::npos ? 0 : slash + 1);
  if (file_name == ".wh..wh..opq") e->what = 2;
  else if (file_name.substr(0, 4) == ".wh.") e->what = 1;
  if (e->what == 1 || e->what == 2) e->dir = 0;  // markers come first (tar.go:51-62)
}
template <class Src>
void ClassifyT(const Src& src, const uint8_t* tar, TarEntry* e) {
  const uint8_t* h = ResolveT(src, e);
  if (!h) return;
  ClassifyPath(h[156], tar, e);
}

// ---- a layer resident in HBM ------------------------------------------------

// A header candidate as tar_headers_kernel writes it (tarindex.h).
struct TarRecord {
  uint64_t block;  // the block's index: its bytes are [512 block, 512 block + 512)
  uint64_t pad;
  uint8_t hdr[512];
};
static_assert(sizeof(TarRecord) == 528, "the kernel's record layout");

// The layer as the host sees it: the candidate records, sorted by block (any
// order is accepted and sorted here), and a way to copy a byte range of the
// layer from where it lives (the device; a host copy in tests).  A block on the
// chain that is no candidate -- the end-of-archive zero block, a corrupted
// header -- is fetched, and the walk's own code decides what it is.
struct IndexedTarSrc {
  static constexpr bool kView = false;
  using Fetch = std::function<bool(uint64_t off, uint64_t len, uint8_t* dst)>;

  IndexedTarSrc(const TarRecord* recs, size_t n_recs, Fetch fetch) : recs_(recs), fetch_(std::move(fetch)) {
    order_.resize(n_recs);
    for (size_t i = 0; i < n_recs; i++) order_[i] = uint32_t(i);
    std::sort(order_.begin(), order_.end(), [&](uint32_t a, uint32_t b) { return recs_[a].block < recs_[b].block; });
    seen_.assign(n_recs, 0);
  }
  const uint8_t* base() const { return nullptr; }  // (no entry of this source keeps a view)
  // A copy from where the layer lives failed (its error text is set): the walk
  // ends, and not as a malformed archive.
  bool failed() const { return failed_; }
  const uint8_t* Block(uint64_t p) const {
    const uint64_t b = p / 512;
    if (p % 512 == 0) {
      // binary search; the chain moves forward, so mostly among the few records after the last hit
      size_t lo = 0, hi = order_.size();
      if (cursor_ < hi && recs_[order_[cursor_]].block <= b) {
        lo = cursor_;
        const size_t near = std::min(hi, cursor_ + 64);
        if (recs_[order_[near - 1]].block >= b) hi = near;
      }
      auto it = std::lower_bound(order_.begin() + lo, order_.begin() + hi, b,
                                 [&](uint32_t i, uint64_t x) { return recs_[i].block < x; });
      if (it != order_.begin() + hi && recs_[*it].block == b) {
        cursor_ = size_t(it - order_.begin());
        seen_[*it] = 1;
        return recs_[*it].hdr;
      }
    }
    auto hit = fetched_.find(p);
    if (hit != fetched_.end()) return hit->second;
    held_.emplace_back(512);
    if (!fetch_(p, 512, held_.back().data())) {
      failed_ = true;
      return nullptr;
    }
    block_fetches++;
    fetched_[p] = held_.back().data();
    return held_.back().data();
  }
  const uint8_t* Range(uint64_t off, uint64_t len) const {
    held_.emplace_back(size_t(len) + 1);
    if (len && !fetch_(off, len, held_.back().data())) {
      failed_ = true;
      return nullptr;
    }
    ext_bytes += len;
    return held_.back().data();
  }
  uint64_t visited() const { return uint64_t(std::count(seen_.begin(), seen_.end(), uint8_t(1))); }

  mutable uint64_t block_fetches = 0;  // chain blocks that were no candidate
  mutable uint64_t ext_bytes = 0;      // bytes of x / L data copied

 private:
  const TarRecord* recs_;
  Fetch fetch_;
  std::vector<uint32_t> order_;
  mutable std::vector<uint8_t> seen_;
  mutable size_t cursor_ = 0;  // the last record handed out
  mutable bool failed_ = false;
  mutable std::deque<std::vector<uint8_t>> held_;  // what the walk was handed stays valid for the walk
  mutable std::map<uint64_t, const uint8_t*> fetched_;
};

// The Required-accepted regular files of a layer, in walk order.
struct TarIndexFile {
  uint64_t path_off, path_len;  // the cleaned path, in TarIndexData::pool (NUL after it)
  uint64_t start;               // the entry's header chain start (a 512-multiple)
  uint64_t data_off, size;
};
struct TarIndexData {
  std::string pool;
  std::vector<TarIndexFile> files;
  tsg_tar_stats tar{};  // entries, regular, required, whiteouts, opaque_dirs as the host walk counts them
  TarSkipCounts skip;   // what LayerTar's skip options dropped (all zero without them)
};

// The walk (tsg_collector_add_tar's rules, entry by entry): 0, or <0 with the
// host walk's error text set -- or, when src.failed(), the source's.  required(path, len, size) is the analyzer's
// Required.
// The chain itself is sequential; Required (the allow-path regexes) is the
// costly part and runs afterwards over the regular files through par(n, fn),
// which calls fn(i) for every i < n, on threads if it likes (SerialFor: here).
struct SerialFor {
  template <class Fn>
  void operator()(size_t n, Fn&& fn) const {
    for (size_t i = 0; i < n; i++) fn(i);
  }
};
// Required over the regular files through par, then the index of the accepted ones, in order.
template <class Req, class Par>
void FinishTarIndex(const std::string& pool, const std::vector<TarIndexFile>& regular, Req&& required,
                    TarIndexData* out, Par&& par) {
  std::vector<uint8_t> keep(regular.size(), 0);
  par(regular.size(), [&](size_t i) {
    const TarIndexFile& f = regular[i];
    keep[i] = required(pool.data() + f.path_off, f.path_len, int64_t(f.size)) ? 1 : 0;
  });
  for (size_t i = 0; i < regular.size(); i++) {
    if (!keep[i]) continue;
    TarIndexFile f = regular[i];
    const uint64_t at = out->pool.size();
    out->pool.append(pool, size_t(f.path_off), size_t(f.path_len) + 1);
    f.path_off = at;
    out->files.push_back(f);
    out->tar.required++;
  }
}
// skip (optional): LayerTar's skipDirs / skipFiles, applied entry by entry in
// chain order as tar.go:64-81 does; a dropped file is in `regular`, not in the index.
template <class Src, class Req, class Par = SerialFor>
int WalkTarIndex(const Src& src, uint64_t n, Req&& required, TarIndexData* out, Par&& par = Par(),
                 const TarSkipOpts* skip = nullptr) {
  std::string pool;
  std::vector<TarIndexFile> regular;
  TarSkipDirs skipped;
  const bool skips = skip && skip->any();
  uint64_t p = 0;
  for (;;) {
    TarEntry e;
    const int r = ChainEntryT(src, n, p, &e);
    if (r < 0) return -1;
    if (r == 1) break;
    ClassifyT(src, src.base(), &e);
    if (e.bad) {
      // (a source that failed has said why: that is no checksum error)
      if (!src.failed()) SetError("tar: invalid header checksum at offset " + std::to_string(e.hdr));
      return -1;
    }
    out->tar.entries++;
    out->tar.whiteouts += e.what == 1;
    out->tar.opaque_dirs += e.what == 2;
    out->tar.regular += e.what == 3;
    if (__builtin_expect(skips, 0) && (e.dir || e.what == 3))
      e.skip = TarSkipStep(*skip, e.dir, e.what == 3, e.path(src.base()), e.start, &skipped, &out->skip);
    if (e.what == 3 && !e.skip) {
      const std::string_view fp = e.path(src.base());
      regular.push_back({uint64_t(pool.size()), uint64_t(fp.size()), e.start, e.data, e.size});
      pool.append(fp.data(), fp.size());
      pool.push_back('\0');
    }
    p = e.next;
  }
  FinishTarIndex(pool, regular, required, out, par);
  return 0;
}

// The host half of the walk the GPU made (tarchain.h): n records in walk order and
// their raw names.  What is left of the walk per entry -- the TypeRegA directory
// test, path.Clean, the leading-slash strip, whiteouts and opaque dirs
// (ClassifyPath) -- runs through par in chunks of kTarEntryChunk entries, each
// with its own path pool and counts (a name that is clean stays a view of the
// name blob until it is copied there: no allocation per entry); the chunks are
// then joined in order, Required runs through par as in WalkTarIndex, and the
// index equals WalkTarIndex's.  ms (optional): classify, join, Required + index.
// -1: a record points outside the name blob (error set).
// skip (optional): LayerTar's skipDirs / skipFiles.  What an entry is by itself
// (TarSkipEval) is decided in its chunk; the skipped directories of all chunks
// are then recorded in walk order with the rank of their entry, and every
// surviving regular file is tested -- through par again -- against the
// directories recorded at a lower rank than its own, which is what the
// sequential walk's list held when it reached the file.
constexpr size_t kTarEntryChunk = 64;
template <class Req, class Par = SerialFor>
int IndexTarEntries(const tsg_tar_entry_rec* recs, uint64_t n, const uint8_t* names, uint64_t name_bytes,
                    Req&& required, TarIndexData* out, Par&& par = Par(), double* ms = nullptr,
                    const TarSkipOpts* skip = nullptr) {
  const bool skips = skip && skip->any();
  auto now = [] {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
  };
  const double t0 = now();
  struct Chunk {
    std::string pool;
    std::vector<TarIndexFile> regular;  // path_off relative to pool
    uint64_t whiteouts = 0, opaque_dirs = 0;
    bool bad = false;
    // with skip options: kTarSkip* per regular file, and the skipped directories (rank, path)
    std::vector<uint8_t> reg_skip;
    std::vector<std::pair<uint64_t, std::string>> skipped_dirs;
  };
  const size_t n_chunks = (size_t(n) + kTarEntryChunk - 1) / kTarEntryChunk;
  std::vector<Chunk> chunks(n_chunks);
  par(n_chunks, [&](size_t c) {
    Chunk& k = chunks[c];
    const size_t i1 = std::min(size_t(n), (c + 1) * kTarEntryChunk);
    for (size_t i = c * kTarEntryChunk; i < i1; i++) {
      const tsg_tar_entry_rec& r = recs[i];
      if (r.name_off > name_bytes || r.name_len > name_bytes - r.name_off) {
        k.bad = true;
        return;
      }
      TarEntry e;
      e.what = (r.typeflag == '0' || r.typeflag == '\0') ? 3 : 0;
      e.fp_off = r.name_off;  // a view of the name blob, which stands in for the layer buffer of a kView source
      e.fp_len = r.name_len;
      ClassifyPath(r.typeflag, names, &e);
      k.whiteouts += e.what == 1;
      k.opaque_dirs += e.what == 2;
      if (__builtin_expect(skips, 0) && (e.dir || e.what == 3)) {
        const std::string_view fp = e.path(names);
        e.skip = TarSkipEval(*skip, e.dir, e.what == 3, fp);
        if (e.skip == kTarSkipDir) k.skipped_dirs.emplace_back(r.start, std::string(fp));
        if (e.what == 3) k.reg_skip.push_back(e.skip);
      }
      if (e.what == 3) {
        const std::string_view fp = e.path(names);
        k.regular.push_back({uint64_t(k.pool.size()), uint64_t(fp.size()), r.start, r.data, r.size});
        k.pool.append(fp.data(), fp.size());
        k.pool.push_back('\0');
      }
    }
  });
  const double t1 = now();
  // where each chunk's paths and files go in the joined pool and list
  std::vector<size_t> pool_at(n_chunks + 1, 0), reg_at(n_chunks + 1, 0);
  for (size_t c = 0; c < n_chunks; c++) {
    const Chunk& k = chunks[c];
    if (k.bad) {
      SetError("tar entries: a record has its name outside the name blob");
      return -1;
    }
    pool_at[c + 1] = pool_at[c] + k.pool.size();
    reg_at[c + 1] = reg_at[c] + k.regular.size();
    out->tar.whiteouts += k.whiteouts;
    out->tar.opaque_dirs += k.opaque_dirs;
  }
  out->tar.entries += n;
  out->tar.regular += reg_at[n_chunks];
  std::string pool(pool_at[n_chunks], '\0');
  std::vector<TarIndexFile> regular(reg_at[n_chunks]);
  std::vector<uint8_t> reg_skip(skips ? reg_at[n_chunks] : 0);
  TarSkipDirs skipped;
  if (skips)
    for (const Chunk& k : chunks)  // in walk order: the ranks ascend
      for (const auto& d : k.skipped_dirs) skipped.Record(d.second, d.first);
  par(n_chunks, [&](size_t c) {
    Chunk& k = chunks[c];
    if (!k.pool.empty()) std::memcpy(&pool[pool_at[c]], k.pool.data(), k.pool.size());
    for (size_t j = 0; j < k.regular.size(); j++) {
      TarIndexFile f = k.regular[j];
      f.path_off += pool_at[c];
      regular[reg_at[c] + j] = f;
      if (skips) {
        uint8_t sk = k.reg_skip[j];
        if (!sk && skipped.Under(std::string_view(pool.data() + f.path_off, size_t(f.path_len)), f.start))
          sk = kTarSkipUnder;
        reg_skip[reg_at[c] + j] = sk;
      }
    }
    k = Chunk();
  });
  chunks.clear();
  if (skips) {  // the dropped files leave the list Required sees
    out->skip.skipped_dirs += skipped.size();
    size_t w = 0;
    for (size_t i = 0; i < regular.size(); i++) {
      out->skip.skipped_files += reg_skip[i] == kTarSkipFile;
      out->skip.under_skipped_dir += reg_skip[i] == kTarSkipUnder;
      if (!reg_skip[i]) regular[w++] = regular[i];
    }
    regular.resize(w);
  }
  const double t2 = now();
  FinishTarIndex(pool, regular, required, out, par);
  if (ms) {
    ms[0] = t1 - t0;
    ms[1] = t2 - t1;
    ms[2] = now() - t2;
  }
  return 0;
}

// Files [first, first + count) of an index as one batch whose arena is the
// layer itself from `base` on: 2 count + 1 pseudo-files, gap, file, gap, ...,
// file, gap.  A gap is what lies between two files -- headers, padding, every
// entry Required refused -- and has an empty path; the last gap is empty (the
// batch ends with the last file's data).  Scan paths carry the "/" prefix of an
// image file (secret.go:130-135).
struct TarBatchPlan {
  uint64_t base = 0;              // a 512-multiple: the chain start of file `first`
  std::vector<uint64_t> offs;     // 2 count + 2, from 0, relative to base
  std::string path_pool;          // NUL-terminated scan paths
  std::vector<const char*> path_ptrs;
  std::vector<uint64_t> path_lens;
  std::vector<uint8_t> flags, kinds, binary;
};
inline void PlanTarBatch(const TarIndexData& ix, uint32_t first, uint32_t count, TarBatchPlan* p) {
  const size_t n = 2 * size_t(count) + 1;
  p->base = count ? ix.files[first].start : 0;
  p->offs.assign(n + 1, 0);
  std::vector<uint64_t> at(n, 0);
  p->path_lens.assign(n, 0);
  p->path_pool.clear();
  for (uint32_t j = 0; j < count; j++) {
    const TarIndexFile& f = ix.files[first + j];
    p->offs[2 * j + 1] = f.data_off - p->base;
    p->offs[2 * j + 2] = f.data_off + f.size - p->base;
    p->path_lens[2 * j + 1] = f.path_len + 1;
  }
  p->offs[n] = p->offs[n - 1];
  for (size_t i = 0; i < n; i++) {
    at[i] = p->path_pool.size();
    if (i & 1) {
      const TarIndexFile& f = ix.files[first + i / 2];
      p->path_pool.push_back('/');
      p->path_pool.append(ix.pool, size_t(f.path_off), size_t(f.path_len));
    }
    p->path_pool.push_back('\0');
  }
  p->path_ptrs.resize(n);
  for (size_t i = 0; i < n; i++) p->path_ptrs[i] = p->path_pool.data() + at[i];
}

// filepath.Ext(path) == ".pyc" (the allowed binaries, secret.go:59-61)
inline bool TarPathIsPyc(const char* p, uint64_t n) {
  for (uint64_t i = n; i-- > 0 && p[i] != '/';)
    if (p[i] == '.') return n - i == 4 && std::memcmp(p + i, ".pyc", 4) == 0;
  return false;
}

// tsg_batch.transform / .binary per pseudo-file from the IsBinary flags over
// their heads (p->flags): a gap is dropped (kind 3); a file is kind 1, or when
// binary kind 2 for a .pyc and kind 3 otherwise -- DeviceKinds' rule for a file
// Required accepted.
inline void TarBatchKinds(TarBatchPlan* p) {
  const size_t n = p->path_ptrs.size();
  p->kinds.assign(n, 3);
  p->binary.assign(n, 0);
  for (size_t i = 1; i < n; i += 2) {
    if (!p->flags[i]) {
      p->kinds[i] = 1;
    } else if (TarPathIsPyc(p->path_ptrs[i], p->path_lens[i])) {
      p->kinds[i] = 2;
      p->binary[i] = 1;
    }
  }
}

}  // namespace tsg
