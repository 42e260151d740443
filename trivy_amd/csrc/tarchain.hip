// The header chain of a tar layer resident in HBM, walked on the GPU (tarchain.h,
// tarindex.h).  After tar_bitmap_kernel (tarindex.hip) has marked the blocks that
// parse as headers:
//
//  tar_entries : a lane per block.  A candidate c is read as an entry start, as
//                tar_index_host.h's ChainEntryT reads it: hop over x / L / K
//                headers, parse sizes and PAX records, apply every bound check.
//                succ[c] is the next entry start (a block index, always > c), or
//                a terminal word: END, or INCOMPLETE with a reason.  A block that
//                is no candidate gets the terminal word kNonCand.  Most
//                candidates of a layer are on the chain; the ones that are not (a
//                tar inside a file) are attacker-controlled, so every loop of the
//                parse ends at a cap of tarchain.h.  Only the name's length is
//                kept per entry; the fields are computed again for the entries on
//                the chain (tar_compact), which costs less than 40 B a block.
//  tar_exits   : a workgroup per segment of S blocks, its succ slice in LDS.
//                Pointer jumping inside the segment gives every block its exit:
//                the first successor at or past the segment's end, or the
//                terminal block the chain from it runs into.  Successors point
//                forward, so ceil(log2 S) rounds do.
//  tar_stitch  : one wave follows the chain from block 0 through the exits: one
//                dependent load per segment entered (a large file skips the
//                segments it spans), notes where the chain enters each segment,
//                and decides the stop (the all-zero test of a non-candidate block
//                is made here, on the one block it matters for).
//  tar_mark    : a workgroup per segment, one lane walks the slice in LDS from
//                the segment's entry and sets the on-chain bits.
//  ranks       : hipcub inclusive sums over the blocks give each on-chain entry
//                its record index and its name's offset.
//  tar_compact : a lane per on-chain entry writes its 64-B record and its raw name
//                (ResolveT's precedence), in walk order.
// Vector stores only; no atomics; no lane waits on another workgroup.
#include "tarindex.h"

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

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

__global__ __launch_bounds__(kCThreads) void tar_entries_kernel(const uint8_t* __restrict__ tar, uint64_t n,
                                                                uint64_t n_blocks, const uint8_t* __restrict__ cand,
                                                                uint32_t* __restrict__ succ,
                                                                uint32_t* __restrict__ nlen) {
  for (uint64_t b = uint64_t(blockIdx.x) * kCThreads + threadIdx.x; b < n_blocks; b += uint64_t(gridDim.x) * kCThreads) {
    if (!bit_at(cand, b)) {
      succ[b] = kNonCand;
      continue;
    }
    const Entry e = chain_entry(tar, n, n_blocks, cand, b);
    if (e.end || e.reason != kTarOk) {
      succ[b] = kTerm | (e.reason << 8) | e.n_ext;  // (reason 0: END)
    } else {
      succ[b] = uint32_t(e.next / 512u);  // > b, <= n_blocks + 1 < 2^31
      nlen[b] = e.name_len;
    }
  }
}

__global__ __launch_bounds__(kCThreads) void tar_exits_kernel(const uint32_t* __restrict__ succ, uint64_t n_blocks,
                                                              uint32_t seg, uint64_t n_segments,
                                                              uint32_t* __restrict__ exits) {
  extern __shared__ uint32_t v[];  // seg words
  for (uint64_t sg = blockIdx.x; sg < n_segments; sg += gridDim.x) {
    const uint64_t s0 = sg * seg;
    const uint64_t s1 = min(s0 + seg, n_blocks);
    const uint32_t m = uint32_t(s1 - s0);
    for (uint32_t i = threadIdx.x; i < m; i += kCThreads) {
      const uint32_t w = succ[s0 + i];
      v[i] = (w & kTerm) ? (kTerm | uint32_t(s0 + i)) : w;
    }
    __syncthreads();
    // v[i] only ever moves forward along block i's chain, so the rounds may read and write in place:
    // a word read is the one of the round before or a later one.  After round k it is 2^k hops on, or final.
    for (uint32_t round = 0; round < 32; round++) {
      int moved = 0;
      for (uint32_t i = threadIdx.x; i < m; i += kCThreads) {
        const uint32_t x = v[i];
        if (!(x & kTerm) && x < s1) {  // (x > s0 + i >= s0)
          v[i] = v[x - uint32_t(s0)];
          moved = 1;
        }
      }
      if (!__syncthreads_or(moved)) break;
    }
    for (uint32_t i = threadIdx.x; i < m; i += kCThreads) exits[s0 + i] = v[i];
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void tar_stitch_kernel(const uint8_t* __restrict__ tar, uint64_t n, uint64_t n_blocks,
                                                        uint32_t seg_shift, uint64_t n_segments,
                                                        const uint32_t* __restrict__ succ,
                                                        const uint32_t* __restrict__ exits,
                                                        uint32_t* __restrict__ seg_entry, TarChainHead* __restrict__ head) {
  const uint32_t lane = threadIdx.x;
  uint64_t e = 0, steps = 0, ext = 0;
  uint32_t kind = kTarStopEnd, reason = kTarOk;
  uint64_t at = 0;
  for (uint64_t it = 0; it <= n_segments; it++) {  // every step enters a later segment
    if (e >= n_blocks) {
      at = e * 512u;
      if (at < n) {
        kind = kTarStopIncomplete;
        reason = kTarTruncated;
      }
      break;
    }
    if (lane == 0) seg_entry[e >> seg_shift] = uint32_t(e);
    const uint32_t x = exits[e];
    steps++;
    if (!(x & kTerm)) {
      e = x;
      continue;
    }
    const uint64_t b = x & ~kTerm;
    at = b * 512u;
    const uint32_t w = succ[b];
    if (w == kNonCand) {
      const uint2 q = *reinterpret_cast<const uint2*>(tar + at + lane * 8u);  // (b < n_blocks: a complete block)
      if (__ballot((q.x | q.y) != 0u) != 0ull) {
        kind = kTarStopIncomplete;
        reason = kTarNotCandidate;
      }
    } else {
      reason = (w >> 8) & 0xFFu;
      ext = w & 0xFFu;
      kind = reason ? kTarStopIncomplete : kTarStopEnd;
    }
    break;
  }
  if (lane == 0) {
    uint4* o = reinterpret_cast<uint4*>(&head->stop);
    o[0] = make_uint4(kind, reason, uint32_t(at), uint32_t(at >> 32));
    o[1] = make_uint4(uint32_t(ext), 0u, uint32_t(steps), uint32_t(steps >> 32));
  }
}

__global__ __launch_bounds__(kCThreads) void tar_mark_kernel(const uint32_t* __restrict__ succ, uint64_t n_blocks,
                                                             uint32_t seg, uint64_t n_segments,
                                                             const uint32_t* __restrict__ seg_entry,
                                                             uint8_t* __restrict__ chain) {
  extern __shared__ uint32_t v[];  // seg words, then seg / 8 bytes of bits
  uint8_t* bits = reinterpret_cast<uint8_t*>(v + seg);
  for (uint64_t sg = blockIdx.x; sg < n_segments; sg += gridDim.x) {
    const uint64_t s0 = sg * seg;
    const uint64_t s1 = min(s0 + seg, n_blocks);
    const uint32_t m = uint32_t(s1 - s0);
    const uint32_t entry = seg_entry[sg];
    if (entry != kNoEntry)  // (workgroup-uniform)
      for (uint32_t i = threadIdx.x; i < m; i += kCThreads) v[i] = succ[s0 + i];
    for (uint32_t i = threadIdx.x; i < seg / 8u; i += kCThreads) bits[i] = 0;
    __syncthreads();
    if (entry != kNoEntry && threadIdx.x == 0) {
      uint64_t cur = entry;  // s0 <= entry < s1
      while (cur < s1) {     // successors point forward: at most m steps
        const uint32_t w = v[cur - s0];
        if (w & kTerm) break;
        bits[(cur - s0) >> 3] |= uint8_t(1u << ((cur - s0) & 7u));
        cur = w;
      }
    }
    __syncthreads();
    // (the chain bitmap has seg / 8 bytes for every segment, the last one included)
    for (uint32_t i = threadIdx.x; i < seg / 8u; i += kCThreads) chain[s0 / 8u + i] = bits[i];
    __syncthreads();
  }
}

struct ChainFlag {
  const uint8_t* chain;
  __host__ __device__ uint32_t operator()(uint32_t b) const { return (chain[b >> 3] >> (b & 7u)) & 1u; }
};
struct ChainNameLen {
  const uint8_t* chain;
  const uint32_t* nlen;
  __host__ __device__ uint64_t operator()(uint32_t b) const { return ((chain[b >> 3] >> (b & 7u)) & 1u) ? nlen[b] : 0; }
};
struct WordPop {
  __host__ __device__ uint64_t operator()(uint64_t w) const {
#if defined(__HIP_DEVICE_COMPILE__)
    return uint64_t(__popcll(w));
#else
    return uint64_t(__builtin_popcountll(w));
#endif
  }
};
using FlagIter = hipcub::TransformInputIterator<uint32_t, ChainFlag, hipcub::CountingInputIterator<uint32_t>>;
using NameIter = hipcub::TransformInputIterator<uint64_t, ChainNameLen, hipcub::CountingInputIterator<uint32_t>>;
using PopIter = hipcub::TransformInputIterator<uint64_t, WordPop, const uint64_t*>;

__global__ void tar_totals_kernel(const uint32_t* __restrict__ rank, const uint64_t* __restrict__ noff,
                                  uint64_t n_blocks, TarChainHead* __restrict__ head) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    head->entries = rank[n_blocks - 1];
    head->name_bytes = noff[n_blocks - 1];
  }
}

__global__ __launch_bounds__(kCThreads) void tar_compact_kernel(const uint8_t* __restrict__ tar, uint64_t n,
                                                                uint64_t n_blocks, const uint8_t* __restrict__ cand,
                                                                const uint8_t* __restrict__ chain,
                                                                const uint32_t* __restrict__ rank,
                                                                const uint64_t* __restrict__ noff,
                                                                uint64_t n_entries, uint64_t name_bytes,
                                                                uint8_t* __restrict__ records,
                                                                uint8_t* __restrict__ names) {
  for (uint64_t b = uint64_t(blockIdx.x) * kCThreads + threadIdx.x; b < n_blocks; b += uint64_t(gridDim.x) * kCThreads) {
    if (!bit_at(chain, b)) continue;
    const Entry e = chain_entry(tar, n, n_blocks, cand, b);  // (complete: tar_mark set no bit otherwise)
    const uint64_t r = uint64_t(rank[b]) - 1u;
    const uint64_t off = noff[b] - e.name_len;
    if (e.end || e.reason != kTarOk || r >= n_entries || off + e.name_len > name_bytes) continue;  // (the layer changed)
    uint4* o = reinterpret_cast<uint4*>(records + r * 64u);
    const uint64_t start = b * 512u, data = e.hdr + 512u;
    o[0] = make_uint4(uint32_t(start), uint32_t(start >> 32), uint32_t(e.hdr), uint32_t(e.hdr >> 32));
    o[1] = make_uint4(uint32_t(data), uint32_t(data >> 32), uint32_t(e.size), uint32_t(e.size >> 32));
    o[2] = make_uint4(uint32_t(off), uint32_t(off >> 32), e.name_len,
                      uint32_t(e.typeflag) | (uint32_t(e.flags) << 8) | (e.n_ext << 16));
    o[3] = make_uint4(0u, 0u, 0u, 0u);
    uint8_t* dst = names + off;
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
}

uint64_t Up256(uint64_t x) { return (x + 255) & ~uint64_t(255); }
uint32_t GridFor(uint64_t items, uint32_t grid_cap) {
  uint64_t g = std::min<uint64_t>(std::max<uint64_t>(items, 1), kMaxGrid);
  if (grid_cap) g = std::min<uint64_t>(g, grid_cap);
  return uint32_t(g);
}

}  // namespace

bool TarChainPlan(uint64_t n_bytes, uint32_t segment_blocks, TarChainLayout* L) {
  const uint32_t seg = segment_blocks ? segment_blocks : kTarDefaultSegment;
  // the marking workgroup holds a word per block and a bit per block: inside the 64 KiB a workgroup may take
  if (seg < kTarMinSegment || (seg & (seg - 1)) || uint64_t(seg) * 4 + seg / 8 > (64u << 10)) return false;
  const uint64_t nb = n_bytes / 512;
  if (nb + 2 >= kTarMaxBlocks) return false;
  *L = TarChainLayout();
  L->n_blocks = nb;
  L->segment = seg;
  L->n_segments = (nb + seg - 1) / seg;
  size_t t1 = 0, t2 = 0, t3 = 0;
  const int items = int(std::max<uint64_t>(nb, 1));
  (void)hipcub::DeviceScan::InclusiveSum(nullptr, t1, FlagIter(hipcub::CountingInputIterator<uint32_t>(0), ChainFlag{nullptr}),
                                         static_cast<uint32_t*>(nullptr), items);
  (void)hipcub::DeviceScan::InclusiveSum(nullptr, t2,
                                         NameIter(hipcub::CountingInputIterator<uint32_t>(0), ChainNameLen{nullptr, nullptr}),
                                         static_cast<uint64_t*>(nullptr), items);
  (void)hipcub::DeviceReduce::Sum(nullptr, t3, PopIter(nullptr, WordPop()), static_cast<uint64_t*>(nullptr),
                                  int((nb + 63) / 64 + 1));
  L->temp_bytes = std::max({t1, t2, t3, size_t(256)});
  // both bitmaps: whole 64-bit words of the candidates, whole segments of the chain
  const uint64_t bm = Up256(std::max((nb + 63) / 64 * 8, L->n_segments * (seg / 8)));
  uint64_t at = 0;
  auto take = [&](uint64_t bytes) {
    const uint64_t o = at;
    at += Up256(bytes);
    return o;
  };
  L->head = take(sizeof(TarChainHead));
  L->cand = take(bm);
  L->chain = take(bm);
  L->seg_entry = take(L->n_segments * 4);
  L->succ = take(nb * 4);
  L->nlen = take(nb * 4);
  L->rank = take(nb * 4);
  L->noff = take(nb * 8);
  L->temp = take(L->temp_bytes);
  L->bytes = at;
  return true;
}

hipError_t TarChainWalk(const uint8_t* dev_tar, uint64_t n_bytes, const TarChainLayout& L, uint8_t* d_work,
                        uint32_t grid_cap, hipStream_t s, hipEvent_t* ev) {
  const uint64_t nb = L.n_blocks;
  if (nb == 0) return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  auto rec = [&](int i) { return ev ? hipEventRecord(ev[i], s) : hipSuccess; };
  TarChainHead* head = reinterpret_cast<TarChainHead*>(d_work + L.head);
  uint64_t* cand64 = reinterpret_cast<uint64_t*>(d_work + L.cand);
  const uint8_t* cand = d_work + L.cand;
  uint8_t* chain = d_work + L.chain;
  uint32_t* seg_entry = reinterpret_cast<uint32_t*>(d_work + L.seg_entry);
  uint32_t* succ = reinterpret_cast<uint32_t*>(d_work + L.succ);
  uint32_t* nlen = reinterpret_cast<uint32_t*>(d_work + L.nlen);
  uint32_t* rank = reinterpret_cast<uint32_t*>(d_work + L.rank);  // the exits first, then the ranks
  uint64_t* noff = reinterpret_cast<uint64_t*>(d_work + L.noff);
  void* temp = d_work + L.temp;
  uint32_t shift = 0;
  while ((1u << shift) < L.segment) shift++;
  const size_t lds_exits = size_t(L.segment) * 4, lds_mark = lds_exits + L.segment / 8;
  const uint32_t seg_grid = GridFor(L.n_segments, grid_cap);
  if ((e = rec(0)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(head, 0, sizeof(TarChainHead), s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(seg_entry, 0xFF, L.n_segments * 4, s)) != hipSuccess) return e;
  if ((e = TarBitmap(dev_tar, n_bytes, cand64, grid_cap, s)) != hipSuccess) return e;
  if ((e = rec(1)) != hipSuccess) return e;
  tar_entries_kernel<<<GridFor((nb + kCThreads - 1) / kCThreads, grid_cap), kCThreads, 0, s>>>(dev_tar, n_bytes, nb, cand,
                                                                                               succ, nlen);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = rec(2)) != hipSuccess) return e;
  tar_exits_kernel<<<seg_grid, kCThreads, lds_exits, s>>>(succ, nb, L.segment, L.n_segments, rank);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  tar_stitch_kernel<<<1, 64, 0, s>>>(dev_tar, n_bytes, nb, shift, L.n_segments, succ, rank, seg_entry, head);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  tar_mark_kernel<<<seg_grid, kCThreads, lds_mark, s>>>(succ, nb, L.segment, L.n_segments, seg_entry, chain);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  size_t tb = L.temp_bytes;
  if ((e = hipcub::DeviceScan::InclusiveSum(temp, tb, FlagIter(hipcub::CountingInputIterator<uint32_t>(0), ChainFlag{chain}),
                                            rank, int(nb), s)) != hipSuccess)
    return e;
  tb = L.temp_bytes;
  if ((e = hipcub::DeviceScan::InclusiveSum(temp, tb,
                                            NameIter(hipcub::CountingInputIterator<uint32_t>(0), ChainNameLen{chain, nlen}),
                                            noff, int(nb), s)) != hipSuccess)
    return e;
  tb = L.temp_bytes;
  if ((e = hipcub::DeviceReduce::Sum(temp, tb, PopIter(cand64, WordPop()), &head->candidates, int((nb + 63) / 64), s)) !=
      hipSuccess)
    return e;
  tar_totals_kernel<<<1, 64, 0, s>>>(rank, noff, nb, head);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return rec(3);
}

hipError_t TarChainCompact(const uint8_t* dev_tar, uint64_t n_bytes, const TarChainLayout& L, const uint8_t* d_work,
                           uint64_t n_entries, uint64_t name_bytes, uint8_t* d_records, uint8_t* d_names,
                           uint32_t grid_cap, hipStream_t s) {
  const uint64_t nb = L.n_blocks;
  if (nb == 0 || n_entries == 0) return hipSuccess;
  tar_compact_kernel<<<GridFor((nb + kCThreads - 1) / kCThreads, grid_cap), kCThreads, 0, s>>>(
      dev_tar, n_bytes, nb, d_work + L.cand, d_work + L.chain, reinterpret_cast<const uint32_t*>(d_work + L.rank),
      reinterpret_cast<const uint64_t*>(d_work + L.noff), n_entries, name_bytes, d_records, d_names);
  return hipGetLastError();
}

}  // namespace tsg
