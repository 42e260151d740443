// What the single-layer pass (tarchain.hip) and the forest pass over all layers
// of an image (tarforest.hip) share: the device functions of the chain walk that
// read one entry of a layer, the inputs of the two rank scans, and the launchers'
// grid and alignment helpers.  Device code; the contract is tarchain.h.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>

#include "tarchain.h"

namespace tsg {
namespace {

constexpr int kCThreads = 256;
constexpr uint64_t kMaxGrid = 2048;
constexpr uint32_t kTerm = 0x80000000u;             // succ / exit: a terminal word
constexpr uint32_t kNonCand = kTerm | (0xFFu << 8);  // succ of a block that is no candidate
constexpr uint32_t kNoEntry = 0xFFFFFFFFu;          // seg_entry: the chain does not enter the segment

__device__ __forceinline__ bool bit_at(const uint8_t* __restrict__ bm, uint64_t b) { return (bm[b >> 3] >> (b & 7u)) & 1u; }

__device__ bool block_all_zero(const uint8_t* __restrict__ tar, uint64_t p) {  // p: a 512-multiple, p + 512 <= n
  const uint4* w = reinterpret_cast<const uint4*>(tar + p);
  uint32_t acc = 0;
  for (uint32_t i = 0; i < 32; i++) {
    const uint4 v = w[i];
    acc |= v.x | v.y | v.z | v.w;
  }
  return acc == 0;
}

// ParseNumeric (tar_index_host.h) over the 12-byte size field.
__device__ bool parse_size(const uint8_t* __restrict__ f, int64_t* out) {
  if (f[0] & 0x80u) {
    const bool neg = (f[0] & 0x40u) != 0;
    uint64_t v = 0;
    for (uint32_t i = 0; i < 12; i++) {
      uint32_t c = i == 0 ? (f[0] & 0x7Fu) : f[i];
      if (neg) c ^= 0xFFu;
      if (i == 0 && neg) c &= 0x7Fu;
      if (v >> 56) return false;
      v = (v << 8) | c;
    }
    if (v >> 63) return false;
    *out = neg ? -int64_t(v) - 1 : int64_t(v);
    return true;
  }
  uint32_t lo = 0, hi = 12;
  while (lo < hi && (f[lo] == ' ' || f[lo] == 0)) lo++;
  while (hi > lo && (f[hi - 1] == ' ' || f[hi - 1] == 0)) hi--;
  int64_t v = 0;
  for (uint32_t i = lo; i < hi; i++) {
    if (f[i] < '0' || f[i] > '7') return false;
    if (v >> 60) return false;
    v = v * 8 + (f[i] - '0');
  }
  *out = v;
  return true;
}

__device__ __forceinline__ bool header_only(uint8_t t) { return t >= '1' && t <= '6'; }

__device__ uint32_t clen(const uint8_t* __restrict__ b, uint32_t n) {  // up to the first NUL
  uint32_t k = 0;
  while (k < n && b[k]) k++;
  return k;
}

struct Entry {
  uint32_t reason;  // kTarOk, or why the entry is incomplete
  bool end;         // the extension headers run into the end of the archive (ChainEntryT's 1)
  uint32_t n_ext;
  uint64_t hdr, size, next;
  uint64_t name_src;           // the name's bytes in the layer (flags != 0), else it is built from hdr
  uint32_t name_len, pfx_len;  // pfx_len != 0: prefix + '/' + name
  uint8_t flags, typeflag;
};

// ParsePax over the data [at, at + n) of an x header, n <= kTarMaxPaxData.
__device__ uint32_t parse_pax(const uint8_t* __restrict__ tar, uint64_t at, uint64_t n, uint64_t* path_src,
                              uint32_t* path_len, bool* has_path, int64_t* size, bool* has_size) {
  const uint8_t* d = tar + at;
  uint64_t p = 0;
  while (p < n) {  // every record is at least 2 bytes: at most n / 2 rounds
    uint64_t sp = p;
    while (sp < n && d[sp] != ' ') sp++;
    if (sp >= n) return kTarBadPax;
    uint64_t len = 0;
    for (uint64_t i = p; i < sp; i++) {
      if (d[i] < '0' || d[i] > '9') return kTarBadPax;
      len = len * 10 + (d[i] - '0');
    }
    if (len < sp - p + 2 || len > n - p || d[p + len - 1] != '\n') return kTarBadPax;
    const uint64_t r0 = sp + 1, r1 = p + len - 1;  // the record "key=value" is [r0, r1)
    uint64_t eq = r0;
    while (eq < r1 && d[eq] != '=') eq++;
    if (eq >= r1) return kTarBadPax;
    if (eq - r0 == 4) {
      const uint8_t a = d[r0], b = d[r0 + 1], c = d[r0 + 2], e = d[r0 + 3];
      if (a == 'p' && b == 'a' && c == 't' && e == 'h') {
        *path_src = at + eq + 1;
        *path_len = uint32_t(r1 - eq - 1);  // (below kTarMaxPaxData)
        *has_path = true;
      } else if (a == 's' && b == 'i' && c == 'z' && e == 'e') {
        const uint64_t vl = r1 - eq - 1;
        if (vl < 1 || vl > kTarMaxPaxSizeDigits) return kTarPaxSizeForm;
        int64_t v = 0;
        for (uint64_t i = eq + 1; i < r1; i++) {
          if (d[i] < '0' || d[i] > '9') return kTarPaxSizeForm;
          v = v * 10 + (d[i] - '0');
        }
        *size = v;
        *has_size = true;
      }
    }
    p += len;
  }
  return kTarOk;
}

// ChainEntryT + the name part of ResolveT for the entry that starts at candidate
// block c (so 512 c + 512 <= n).  cand: the candidate bitmap.
__device__ Entry chain_entry(const uint8_t* __restrict__ tar, uint64_t n, uint64_t n_blocks,
                             const uint8_t* __restrict__ cand, uint64_t c) {
  Entry e{};
  uint64_t p = c * 512u;
  uint64_t path_src = 0, long_off = 0, long_len = 0;
  uint32_t path_len = 0;
  bool has_path = false, has_size = false, has_long = false;
  int64_t pax_size = 0, size = 0;
  uint8_t type = 0;
  for (;;) {  // at most kTarMaxExt + 1 rounds
    if (p + 512u > n) {
      if (p >= n) {
        e.end = true;
      } else {
        e.reason = kTarTruncated;
      }
      return e;
    }
    if (p != c * 512u && !bit_at(cand, p / 512u)) {  // (p + 512 <= n: a complete block, inside the bitmap)
      if (block_all_zero(tar, p)) {
        e.end = true;
      } else {
        e.reason = kTarNotCandidate;
      }
      return e;
    }
    const uint8_t* h = tar + p;
    type = h[156];
    if (!parse_size(h + 124, &size) || size < 0) {
      e.reason = kTarBadSize;
      return e;
    }
    const uint64_t dsz = header_only(type) ? 0 : uint64_t(size);
    const uint64_t data = p + 512u;
    if (dsz > n || data + dsz > n) {
      e.reason = kTarTruncated;
      return e;
    }
    if (type != 'x' && type != 'L' && type != 'K') break;
    if (e.n_ext == kTarMaxExt) {
      e.reason = kTarCap;
      return e;
    }
    e.n_ext++;
    if (type == 'x') {
      if (dsz > kTarMaxPaxData) {
        e.reason = kTarCap;
        return e;
      }
      const uint32_t r = parse_pax(tar, data, dsz, &path_src, &path_len, &has_path, &pax_size, &has_size);
      if (r != kTarOk) {
        e.reason = r;
        return e;
      }
    }
    if (type == 'L') {
      if (dsz > kTarMaxNameSrc) {
        e.reason = kTarCap;
        return e;
      }
      has_long = true;
      long_off = data;
      long_len = dsz;
    }
    p = data + ((dsz + 511u) & ~uint64_t(511));
  }
  e.hdr = p;
  e.typeflag = type;
  if (has_size) size = pax_size;
  const uint64_t dsz = header_only(type) ? 0 : uint64_t(size);  // (TypeRegA is no header-only type either)
  const uint64_t data = p + 512u;
  if (dsz > n || data + dsz > n) {
    e.reason = kTarTruncated;
    return e;
  }
  e.size = dsz;
  e.next = data + ((dsz + 511u) & ~uint64_t(511));
  const uint8_t* h = tar + p;
  if (has_path) {
    e.flags = kTarNamePax;
    e.name_src = path_src;
    e.name_len = path_len;
  } else if (has_long) {
    e.flags = kTarNameLong;
    e.name_src = long_off;
    e.name_len = clen(tar + long_off, uint32_t(long_len));  // (long_len <= kTarMaxNameSrc, inside the layer)
  } else {
    const uint32_t nl = clen(h, 100);
    uint32_t pl = 0;
    if (h[257] == 'u' && h[258] == 's' && h[259] == 't' && h[260] == 'a' && h[261] == 'r' && h[262] == 0 &&
        h[263] == '0' && h[264] == '0')
      pl = clen(h + 345, 155);
    e.pfx_len = pl;
    e.name_len = pl ? pl + 1u + nl : nl;
  }
  return e;
}

// One entry's 64-B record and its raw name (ResolveT's precedence): `start` is the entry's first block
// offset in the layer, `off` the name's offset as the record states it, dst where the name goes.
__device__ __forceinline__ void write_entry(const uint8_t* __restrict__ tar, const Entry& e, uint64_t start, uint64_t off,
                                            uint8_t* __restrict__ rec, uint8_t* __restrict__ dst) {
  uint4* o = reinterpret_cast<uint4*>(rec);
  const uint64_t data = e.hdr + 512u;
  o[0] = make_uint4(uint32_t(start), uint32_t(start >> 32), uint32_t(e.hdr), uint32_t(e.hdr >> 32));
  o[1] = make_uint4(uint32_t(data), uint32_t(data >> 32), uint32_t(e.size), uint32_t(e.size >> 32));
  o[2] = make_uint4(uint32_t(off), uint32_t(off >> 32), e.name_len,
                    uint32_t(e.typeflag) | (uint32_t(e.flags) << 8) | (e.n_ext << 16));
  o[3] = make_uint4(0u, 0u, 0u, 0u);
  if (e.flags) {
    const uint8_t* src = tar + e.name_src;
    for (uint32_t i = 0; i < e.name_len; i++) dst[i] = src[i];
  } else {
    const uint8_t* h = tar + e.hdr;
    uint32_t k = 0;
    if (e.pfx_len) {
      for (uint32_t i = 0; i < e.pfx_len; i++) dst[k++] = h[345 + i];
      dst[k++] = '/';
    }
    for (uint32_t i = 0; k < e.name_len; i++) dst[k++] = h[i];
  }
}

// The inputs of the two rank scans: block b's on-chain bit, and its name length where the bit is set.
struct ChainFlag {
  const uint8_t* chain;
  __host__ __device__ uint32_t operator()(uint32_t b) const { return (chain[b >> 3] >> (b & 7u)) & 1u; }
};
struct ChainNameLen {
  const uint8_t* chain;
  const uint32_t* nlen;
  __host__ __device__ uint64_t operator()(uint32_t b) const { return ((chain[b >> 3] >> (b & 7u)) & 1u) ? nlen[b] : 0; }
};
using FlagIter = hipcub::TransformInputIterator<uint32_t, ChainFlag, hipcub::CountingInputIterator<uint32_t>>;
using NameIter = hipcub::TransformInputIterator<uint64_t, ChainNameLen, hipcub::CountingInputIterator<uint32_t>>;

inline uint64_t Up256(uint64_t x) { return (x + 255) & ~uint64_t(255); }
inline uint32_t GridFor(uint64_t items, uint32_t grid_cap) {
  uint64_t g = std::min<uint64_t>(std::max<uint64_t>(items, 1), kMaxGrid);
  if (grid_cap) g = std::min<uint64_t>(g, grid_cap);
  return uint32_t(g);
}

}  // namespace
}  // namespace tsg
