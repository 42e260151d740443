// Path classify and Required of a resident tar layer's entries on the GPU (the contract:
// tarrequired.h).  All on the pass's stream after the compaction; vector stores and plain
// C++ stores only, no atomics, nothing waits on another workgroup.
//
//  decide  : a lane per entry reads its record and its raw name once and stores a 16-B
//            decision: the verdict, where fp begins in the name, its length, the entry's
//            extension headers, and the allow rules whose literal fp holds.  The two
//            shift-ands are pathfilter.h's steps over the same tables path_filter_kernel
//            reads, staged in LDS.  Every loop is bounded by the name's length, which
//            tarchain.h's caps keep at 64 KiB; a name outside its layer's blob is never read.
//  ranks   : two hipcub inclusive sums over the decisions give each emitted entry its
//            record index and the end of its path in the blob.
//  totals  : a workgroup per layer counts its verdicts and takes its record and path
//            bases from the sums at its two ends.
//  emit    : a lane per emitted entry writes the 48-B record and copies fp (or the raw
//            name) and a NUL.
//
// With skip options three kernels go between decide and ranks (tarrequired.h says what they
// decide); these use ordinary vector atomics on HBM -- a counter, a compare-and-swap per
// claimed slot, a 64-bit minimum per key:
//
//  match   : a lane per entry, the patterns staged in LDS; bounded byte compares.
//  build   : a lane per recorded directory inserts its path and its direct parent.
//  under   : a lane per regular survivor reads fp once with a running hash, and looks up
//            every ancestor at its '/', then fp itself in both roles.
// A probe sequence ends at an empty slot or after as many steps as the table has slots.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <hipcub/hipcub.hpp>

#include "pathfilter.h"
#include "tar_skip_dev.h"
#include "tarindex.h"

namespace tsg {
namespace {

constexpr int kRThreads = 256;
constexpr uint32_t kRMaxGrid = 4096;

inline uint64_t Up256(uint64_t x) { return (x + 255) & ~uint64_t(255); }
inline uint32_t GridFor(uint64_t items, uint32_t grid_cap) {
  uint64_t g = std::min<uint64_t>(std::max<uint64_t>(items, 1), kRMaxGrid);
  if (grid_cap) g = std::min<uint64_t>(g, grid_cap);
  return uint32_t(g);
}

// The decision of an entry: x, y the rules mask; z the bytes the entry puts into the blob
// before its NUL; w = verdict | skip << 8 | n_ext << 16 | all_rules << 24, skip being where
// those bytes begin in the raw name.
__device__ __forceinline__ uint32_t dec_verdict(const uint4& d) { return d.w & 0xFFu; }
__device__ __host__ __forceinline__ bool emits(uint32_t v) { return (v >= kReqKeep && v <= kReqAskName) || v == kReqSkipDir; }

// The layer of entry i: the last row whose rec_base is at or below i (rows[n_layers].rec_base = n > i).
__device__ __forceinline__ uint32_t layer_of(const TarRequiredRow* __restrict__ rows, uint32_t n_layers, uint64_t i) {
  uint32_t lo = 0, hi = n_layers;  // the answer is in [lo, hi)
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (rows[mid].rec_base <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ bool bytes_eq(const uint8_t* __restrict__ p, const char* lit, uint32_t n) {
  for (uint32_t i = 0; i < n; i++)
    if (p[i] != uint8_t(lit[i])) return false;
  return true;
}
#define TSG_IS(p, n, lit) ((n) == sizeof(lit) - 1 && bytes_eq((p), (lit), sizeof(lit) - 1))

__device__ __forceinline__ uint32_t git_byte(uint32_t k) { return (0x7469672Eu >> (8u * k)) & 0xFFu; }  // ".git"
__device__ __forceinline__ uint32_t node_byte(uint32_t k) {  // "node_modules"
  return k < 8 ? uint32_t(0x646F6D5F65646F6Eull >> (8u * k)) & 0xFFu : (0x73656C75u >> (8u * (k - 8u))) & 0xFFu;
}

// secret.go's skipFiles and skipExts over a base name / an extension (from the dot).
__device__ __forceinline__ bool skip_file(const uint8_t* __restrict__ b, uint32_t n) {
  return TSG_IS(b, n, "go.mod") || TSG_IS(b, n, "go.sum") || TSG_IS(b, n, "package-lock.json") ||
         TSG_IS(b, n, "yarn.lock") || TSG_IS(b, n, "pnpm-lock.yaml") || TSG_IS(b, n, "Pipfile.lock") ||
         TSG_IS(b, n, "Gemfile.lock");
}
__device__ __forceinline__ bool skip_ext(const uint8_t* __restrict__ x, uint32_t n) {
  return TSG_IS(x, n, ".jpg") || TSG_IS(x, n, ".png") || TSG_IS(x, n, ".gif") || TSG_IS(x, n, ".doc") ||
         TSG_IS(x, n, ".pdf") || TSG_IS(x, n, ".bin") || TSG_IS(x, n, ".svg") || TSG_IS(x, n, ".socket") ||
         TSG_IS(x, n, ".deb") || TSG_IS(x, n, ".rpm") || TSG_IS(x, n, ".zip") || TSG_IS(x, n, ".gz") ||
         TSG_IS(x, n, ".gzip") || TSG_IS(x, n, ".tar");
}

template <bool kPath, bool kSure>
__global__ __launch_bounds__(kRThreads) void req_decide_kernel(const uint4* __restrict__ recs,
                                                               const uint8_t* __restrict__ names, uint64_t n,
                                                               const TarRequiredRow* __restrict__ rows,
                                                               uint32_t n_layers, uint64_t name_bytes,
                                                               const uint8_t* __restrict__ cfg, uint32_t cfg_len,
                                                               const PathTable* __restrict__ T,
                                                               const SureTable* __restrict__ X,
                                                               uint4* __restrict__ dec) {
  __shared__ uint64_t sB[kPath ? 256 : 1][4];
  __shared__ uint64_t sX[kSure ? 256 : 1][4];
  __shared__ uint8_t s_rule[kPath ? 256 : 4];
  uint64_t S[4] = {}, E[4] = {}, XS[4] = {}, XS0[4] = {}, XE[4] = {}, XEZ[4] = {};
  if (kPath) {
    for (uint32_t i = threadIdx.x; i < 256 * 4; i += kRThreads) (&sB[0][0])[i] = (&T->B[0][0])[i];
    for (uint32_t i = threadIdx.x; i < 256; i += kRThreads) s_rule[i] = T->rule_of[i];
#pragma unroll
    for (int w = 0; w < 4; w++) {
      S[w] = T->S[w];
      E[w] = T->E[w];
    }
  }
  if (kSure) {
    for (uint32_t i = threadIdx.x; i < 256 * 4; i += kRThreads) (&sX[0][0])[i] = (&X->B[0][0])[i];
#pragma unroll
    for (int w = 0; w < 4; w++) {
      XS[w] = X->S[w];
      XS0[w] = X->S0[w];
      XE[w] = X->E[w];
      XEZ[w] = X->EZ[w];
    }
  }
  __syncthreads();
  for (uint64_t i = uint64_t(blockIdx.x) * kRThreads + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kRThreads) {
    const uint4 w1 = recs[i * 4 + 1], w2 = recs[i * 4 + 2];
    const uint64_t size = uint64_t(w1.z) | (uint64_t(w1.w) << 32);
    const uint64_t name_off = uint64_t(w2.x) | (uint64_t(w2.y) << 32);
    const uint32_t len = w2.z, typeflag = w2.w & 0xFFu, n_ext = (w2.w >> 16) & 0xFFu;
    const uint32_t l = layer_of(rows, n_layers, i);
    const uint64_t lb = rows[l].name_base, le = rows[l + 1].name_base;
    uint32_t verdict = kReqAskName, skip = 0, out_len = len, all = 0;
    uint64_t rules = 0;
    if (le < lb || le > name_bytes || name_off > le - lb || len > le - lb - name_off) {
      verdict = kReqBad;  // (never read)
      out_len = 0;
    } else {
      const uint8_t* __restrict__ N = names + lb + name_off;
      uint32_t p0 = 0;
      if (len >= 2 && N[0] == '.' && N[1] == '/') p0 = 2;
      else if (len >= 1 && N[0] == '/') p0 = 1;
      uint32_t p1 = len;
      while (p1 > p0 && N[p1 - 1] == '/') p1--;
      bool clean = p1 > p0 && N[p0] != '/';
      if (clean) {
        uint32_t es = p0, last_dot = ~0u, high = 0;
        bool eg = true, en = true, dots = true, skipdir = false;
        uint64_t D[4] = {0, 0, 0, 0}, H[4] = {0, 0, 0, 0}, XD[4] = {0, 0, 0, 0}, XH = 0;
        for (uint32_t j = p0; j < p1; j++) {
          const uint32_t c = N[j];
          high |= c;
          if (kPath) {
            const uint32_t lc = c + ((c - 'A') < 26u ? 32u : 0u);
#pragma unroll
            for (int w = 0; w < 4; w++) {
              D[w] = TSG_PATH_STEP(D[w], w, lc, sB, S);
              H[w] |= D[w] & E[w];
            }
          }
          if (kSure) {
#pragma unroll
            for (int w = 0; w < 4; w++) {
              XD[w] = TSG_SURE_STEP(XD[w], w, c, j == p0, sX, XS, XS0, XE, XEZ);
              XH |= XD[w] & (XE[w] | (j + 1 == p1 ? XEZ[w] : 0));
            }
          }
          const uint32_t k = j - es;
          if (c == '/') {
            if (k == 0 || (dots && k <= 2)) {  // an empty, "." or ".." element
              clean = false;
              break;
            }
            if ((eg && k == 4) || (en && k == 12)) skipdir = true;
            es = j + 1;
            last_dot = ~0u;
            eg = en = dots = true;
          } else {
            eg = eg && k < 4 && c == git_byte(k & 3u);
            en = en && k < 12 && c == node_byte(k < 12 ? k : 0);
            dots = dots && c == '.';
            if (c == '.') last_dot = j;
          }
        }
        const uint32_t blen = p1 - es;  // the base name: never empty (N[p1 - 1] != '/')
        if (clean && dots && blen <= 2) clean = false;
        if (clean) {
          const uint8_t* __restrict__ base = N + es;
          const bool regular = typeflag == '0' || (typeflag == 0 && p1 == len);
          skip = p0;
          out_len = p1 - p0;
          if (TSG_IS(base, blen, ".wh..wh..opq")) {
            verdict = kReqOpaque;
          } else if (blen >= 4 && bytes_eq(base, ".wh.", 4)) {
            verdict = kReqWhiteout;
          } else if (!regular) {
            verdict = kReqOther;
          } else if (int64_t(size) < 10 || skipdir || skip_file(base, blen) ||
                     (out_len == cfg_len && bytes_eq(N + p0, reinterpret_cast<const char*>(cfg), cfg_len)) ||
                     (last_dot != ~0u && p1 - last_dot <= 7 && skip_ext(N + last_dot, p1 - last_dot))) {
            verdict = kReqDrop;
          } else if (!kPath || (high & 0x80u)) {
            verdict = kReqAskAllow;
            all = 1;
          } else if (kSure && XH != 0 && out_len <= kSureMaxPath) {
            verdict = kReqDrop;
          } else {
#pragma unroll
            for (int w = 0; w < 4; w++)
              for (uint64_t h = H[w]; h; h &= h - 1) rules |= uint64_t(1) << s_rule[w * 64 + __builtin_ctzll(h)];
            verdict = rules ? kReqAskAllow : kReqKeep;
          }
        }
      }
      if (!clean) {
        verdict = kReqAskName;
        skip = 0;
        out_len = len;
      }
    }
    dec[i] = make_uint4(uint32_t(rules), uint32_t(rules >> 32), out_len, verdict | (skip << 8) | (n_ext << 16) | (all << 24));
  }
}

// ---- the skip stage ------------------------------------------------------------------
// fp of entry i as the decide kernel found it (its verdict is not kReqBad): a view of the raw name.
struct ReqName {
  const uint8_t* fp;
  uint32_t len, layer;
};
__device__ __forceinline__ ReqName name_of(const uint4* __restrict__ recs, const uint8_t* __restrict__ names,
                                           const TarRequiredRow* __restrict__ rows, uint32_t n_layers,
                                           const uint4* __restrict__ dec, uint64_t i) {
  const uint4 w2 = recs[i * 4 + 2], d = dec[i];
  ReqName r;
  r.layer = layer_of(rows, n_layers, i);
  r.fp = names + rows[r.layer].name_base + (uint64_t(w2.x) | (uint64_t(w2.y) << 32)) + ((d.w >> 8) & 0xFFu);
  r.len = d.z;
  return r;
}
__device__ __forceinline__ bool regular_verdict(uint32_t v) { return v == kReqDrop || v == kReqKeep || v == kReqAskAllow; }

__global__ __launch_bounds__(kRThreads) void skip_match_kernel(const uint4* __restrict__ recs,
                                                               const uint8_t* __restrict__ names, uint64_t n,
                                                               const TarRequiredRow* __restrict__ rows, uint32_t n_layers,
                                                               const TarSkipTable* __restrict__ pats,
                                                               uint4* __restrict__ dec, uint32_t* __restrict__ n_dirs) {
  __shared__ uint32_t s_words[sizeof(TarSkipTable) / 4];
  for (uint32_t k = threadIdx.x; k < sizeof(TarSkipTable) / 4; k += kRThreads)
    s_words[k] = reinterpret_cast<const uint32_t*>(pats)[k];
  __syncthreads();
  const TarSkipTable* s_pat = reinterpret_cast<const TarSkipTable*>(s_words);
  for (uint64_t i = uint64_t(blockIdx.x) * kRThreads + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kRThreads) {
    const uint32_t w = dec[i].w, v = w & 0xFFu;
    if (v != kReqOther && !regular_verdict(v)) continue;
    const ReqName nm = name_of(recs, names, rows, n_layers, dec, i);
    uint32_t to = v;
    if (v == kReqOther) {
      // a directory: typeflag '5', or '\0' (then the decide kernel saw trailing slashes: it is not regular)
      const uint32_t typeflag = recs[i * 4 + 2].w & 0xFFu;
      if ((typeflag == '5' || typeflag == 0) && TarSkipMatch(s_pat, false, nm.fp, nm.len)) {
        to = kReqSkipDir;
        atomicAdd(n_dirs, 1u);
      }
    } else if (TarSkipMatch(s_pat, true, nm.fp, nm.len)) {
      to = kReqSkipFile;
    }
    if (to != v) dec[i].w = (w & ~0xFFu) | to;
  }
}

constexpr uint32_t kSlotEmpty = 0xFFFFFFFFu;
constexpr uint32_t kHash0 = 2166136261u, kHashMul = 16777619u;  // FNV-1a over fp's bytes, from the left
__device__ __forceinline__ uint32_t slot_of(uint32_t h, uint32_t layer, uint32_t parent, uint32_t mask) {
  uint32_t x = h ^ (layer * 0x9E3779B1u) ^ (parent ? 0x7F4A7C15u : 0u);
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x & mask;
}
// Is the key of a slot's owner (its fp, or the direct parent of its fp) the klen bytes at key, in `layer`?
__device__ __forceinline__ bool owner_is(uint32_t owner, uint32_t parent, uint32_t layer, const uint8_t* __restrict__ key,
                                         uint32_t klen, const uint4* __restrict__ recs,
                                         const uint8_t* __restrict__ names, const TarRequiredRow* __restrict__ rows,
                                         uint32_t n_layers, const uint4* __restrict__ dec) {
  if ((owner >> 31) != parent) return false;
  const ReqName o = name_of(recs, names, rows, n_layers, dec, owner & 0x7FFFFFFFu);
  if (o.layer != layer || o.len < klen) return false;
  if (parent ? (o.len == klen || o.fp[klen] != '/') : o.len != klen) return false;
  for (uint32_t k = 0; k < klen; k++)
    if (o.fp[k] != key[k]) return false;
  if (parent)  // the direct parent: no further '/' below it
    for (uint32_t k = klen + 1; k < o.len; k++)
      if (o.fp[k] == '/') return false;
  return true;
}

__global__ __launch_bounds__(kRThreads) void skip_build_kernel(const uint4* __restrict__ recs,
                                                               const uint8_t* __restrict__ names, uint64_t n,
                                                               const TarRequiredRow* __restrict__ rows, uint32_t n_layers,
                                                               const uint4* __restrict__ dec,
                                                               TarSkipSlot* __restrict__ tab, uint32_t mask) {
  for (uint64_t i = uint64_t(blockIdx.x) * kRThreads + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kRThreads) {
    if ((dec[i].w & 0xFFu) != kReqSkipDir) continue;
    const ReqName nm = name_of(recs, names, rows, n_layers, dec, i);
    const uint4 w0 = recs[i * 4];
    const unsigned long long rank = uint64_t(w0.x) | (uint64_t(w0.y) << 32);
    uint32_t h = kHash0, h_parent = 0, parent_len = 0;
    for (uint32_t j = 0; j < nm.len; j++) {
      const uint32_t c = nm.fp[j];
      if (c == '/') {
        parent_len = j;
        h_parent = h;
      }
      h = (h ^ c) * kHashMul;
    }
    for (uint32_t parent = 0; parent < 2; parent++) {
      if (parent && parent_len == 0) break;  // (a clean fp has no '/' at 0)
      const uint32_t klen = parent ? parent_len : nm.len, me = uint32_t(i) | (parent << 31);
      uint32_t slot = slot_of(parent ? h_parent : h, nm.layer, parent, mask);
      for (uint32_t step = 0; step <= mask; step++, slot = (slot + 1) & mask) {
        const uint32_t was = atomicCAS(&tab[slot].owner, kSlotEmpty, me);
        if (was == kSlotEmpty || was == me ||
            owner_is(was, parent, nm.layer, nm.fp, klen, recs, names, rows, n_layers, dec)) {
          atomicMin(reinterpret_cast<unsigned long long*>(&tab[slot].rank), rank);
          break;
        }
      }
    }
  }
}

// The lowest rank recorded for a key; all ones: none.
__device__ __forceinline__ uint64_t skip_find(const TarSkipSlot* __restrict__ tab, uint32_t mask, uint32_t h, uint32_t parent,
                                              uint32_t layer, const uint8_t* __restrict__ key, uint32_t klen,
                                              const uint4* __restrict__ recs, const uint8_t* __restrict__ names,
                                              const TarRequiredRow* __restrict__ rows, uint32_t n_layers,
                                              const uint4* __restrict__ dec) {
  uint32_t slot = slot_of(h, layer, parent, mask);
  for (uint32_t step = 0; step <= mask; step++, slot = (slot + 1) & mask) {
    const uint32_t owner = tab[slot].owner;
    if (owner == kSlotEmpty) break;
    if (owner_is(owner, parent, layer, key, klen, recs, names, rows, n_layers, dec)) return tab[slot].rank;
  }
  return ~uint64_t(0);
}

__global__ __launch_bounds__(kRThreads) void skip_under_kernel(const uint4* __restrict__ recs,
                                                               const uint8_t* __restrict__ names, uint64_t n,
                                                               const TarRequiredRow* __restrict__ rows, uint32_t n_layers,
                                                               uint4* __restrict__ dec,
                                                               const TarSkipSlot* __restrict__ tab, uint32_t mask) {
  for (uint64_t i = uint64_t(blockIdx.x) * kRThreads + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kRThreads) {
    const uint32_t w = dec[i].w;
    if (!regular_verdict(w & 0xFFu)) continue;
    const ReqName nm = name_of(recs, names, rows, n_layers, dec, i);
    const uint4 w0 = recs[i * 4];
    const uint64_t rank = uint64_t(w0.x) | (uint64_t(w0.y) << 32);
    uint32_t h = kHash0;
    bool under = false;
    for (uint32_t j = 0; j < nm.len && !under; j++) {
      const uint32_t c = nm.fp[j];
      if (c == '/')  // an ancestor of fp
        under = skip_find(tab, mask, h, 0, nm.layer, nm.fp, j, recs, names, rows, n_layers, dec) < rank;
      h = (h ^ c) * kHashMul;
    }
    under = under || skip_find(tab, mask, h, 0, nm.layer, nm.fp, nm.len, recs, names, rows, n_layers, dec) < rank ||
            skip_find(tab, mask, h, 1, nm.layer, nm.fp, nm.len, recs, names, rows, n_layers, dec) < rank;
    if (under) dec[i].w = (w & ~0xFFu) | kReqSkipUnder;
  }
}

// The inputs of the two rank scans: whether entry i has a record, and its bytes in the blob.
struct ReqFlag {
  const uint4* dec;
  __host__ __device__ uint64_t operator()(uint32_t i) const { return emits(dec[i].w & 0xFFu) ? 1u : 0u; }
};
struct ReqBytes {
  const uint4* dec;
  __host__ __device__ uint64_t operator()(uint32_t i) const {
    const uint4 d = dec[i];
    return emits(d.w & 0xFFu) ? uint64_t(d.z) + 1u : 0u;
  }
};
using ReqFlagIter = hipcub::TransformInputIterator<uint64_t, ReqFlag, hipcub::CountingInputIterator<uint32_t>>;
using ReqBytesIter = hipcub::TransformInputIterator<uint64_t, ReqBytes, hipcub::CountingInputIterator<uint32_t>>;

constexpr int kVerdicts = 11;
constexpr int kCountSlots = kVerdicts + 1;  // the verdicts and the extension headers

__global__ __launch_bounds__(kRThreads) void req_totals_kernel(const uint4* __restrict__ dec,
                                                               const uint64_t* __restrict__ rrank,
                                                               const uint64_t* __restrict__ brank,
                                                               const TarRequiredRow* __restrict__ rows,
                                                               uint32_t n_layers, TarRequiredCounts* __restrict__ counts) {
  __shared__ uint64_t s_cnt[kRThreads / 64][kCountSlots];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t l = blockIdx.x; l < n_layers; l += gridDim.x) {
    const uint64_t i0 = rows[l].rec_base, i1 = rows[l + 1].rec_base;
    uint64_t cnt[kCountSlots] = {};
    for (uint64_t i = i0 + threadIdx.x; i < i1; i += kRThreads) {
      const uint32_t w = dec[i].w;
#pragma unroll
      for (int v = 0; v < kVerdicts; v++) cnt[v] += (w & 0xFFu) == uint32_t(v);
      cnt[kVerdicts] += (w >> 16) & 0xFFu;
    }
#pragma unroll
    for (int v = 0; v < kCountSlots; v++) {
      uint64_t x = cnt[v];
      for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o);
      if (lane == 0) s_cnt[wave][v] = x;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint64_t t[kCountSlots];
      for (int v = 0; v < kCountSlots; v++) {
        t[v] = 0;
        for (int k = 0; k < kRThreads / 64; k++) t[v] += s_cnt[k][v];
      }
      const uint64_t r0 = i0 ? rrank[i0 - 1] : 0, r1 = i1 ? rrank[i1 - 1] : 0;
      const uint64_t b0 = i0 ? brank[i0 - 1] : 0, b1 = i1 ? brank[i1 - 1] : 0;
      TarRequiredCounts c;
      c.entries = i1 - i0;
      c.regular = t[kReqDrop] + t[kReqKeep] + t[kReqAskAllow] + t[kReqSkipFile] + t[kReqSkipUnder];
      c.whiteouts = t[kReqWhiteout];
      c.opaque_dirs = t[kReqOpaque];
      c.records = r1 - r0;
      c.path_bytes = b1 - b0;
      c.kept = t[kReqKeep];
      c.dropped = t[kReqDrop];
      c.ask_allow = t[kReqAskAllow];
      c.ask_name = t[kReqAskName];
      c.bad = t[kReqBad];
      c.ext_headers = t[kVerdicts];
      c.rec_first = r0;
      c.path_first = b0;
      c.pad[0] = t[kReqSkipDir];
      c.pad[1] = t[kReqSkipFile] | (t[kReqSkipUnder] << 32);
      counts[l] = c;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kRThreads) void req_emit_kernel(const uint4* __restrict__ recs,
                                                             const uint8_t* __restrict__ names, uint64_t n,
                                                             const TarRequiredRow* __restrict__ rows, uint32_t n_layers,
                                                             const uint4* __restrict__ dec,
                                                             const uint64_t* __restrict__ rrank,
                                                             const uint64_t* __restrict__ brank, uint64_t blob_cap,
                                                             uint4* __restrict__ out, uint8_t* __restrict__ blob) {
  for (uint64_t i = uint64_t(blockIdx.x) * kRThreads + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kRThreads) {
    const uint4 d = dec[i];
    const uint32_t verdict = dec_verdict(d);
    if (!emits(verdict)) continue;
    const uint32_t out_len = d.z, skip = (d.w >> 8) & 0xFFu;
    const uint64_t r = rrank[i] - 1u, end = brank[i];
    if (r >= n || end > blob_cap || end < uint64_t(out_len) + 1u) continue;  // (cannot happen: the sums are over these decisions)
    const uint64_t at = end - out_len - 1u;
    const uint32_t l = layer_of(rows, n_layers, i);
    const uint64_t i0 = rows[l].rec_base;
    const uint64_t path_first = i0 ? brank[i0 - 1] : 0;
    const uint4 w0 = recs[i * 4], w1 = recs[i * 4 + 1], w2 = recs[i * 4 + 2];
    const uint64_t off = at - path_first;
    uint4* o = out + r * 3;
    o[0] = make_uint4(w0.x, w0.y, w1.x, w1.y);                               // start, data
    o[1] = make_uint4(w1.z, w1.w, uint32_t(off), uint32_t(off >> 32));       // size, path_off
    o[2] = make_uint4(out_len, (w2.w & 0xFFu) | (verdict << 8) | ((d.w >> 24) << 16), d.x, d.y);
    // (the decide kernel found the name inside its layer's blob: verdict is not kReqBad)
    const uint8_t* __restrict__ src =
        names + rows[l].name_base + (uint64_t(w2.x) | (uint64_t(w2.y) << 32)) + skip;
    uint8_t* __restrict__ dst = blob + at;
    for (uint32_t k = 0; k < out_len; k++) dst[k] = src[k];
    dst[out_len] = 0;
  }
}

}  // namespace

bool TarRequiredPlan(uint64_t n, uint32_t n_layers, uint64_t name_bytes, uint32_t cfg_len, TarRequiredLayout* L,
                     bool skip) {
  if (n_layers == 0 || n >= (uint64_t(1) << 31)) return false;
  *L = TarRequiredLayout();
  L->n = n;
  L->n_layers = n_layers;
  L->name_bytes = name_bytes;
  L->cfg_len = cfg_len;
  L->skip = skip;
  size_t t1 = 0, t2 = 0;
  const int items = int(std::max<uint64_t>(n, 1));
  (void)hipcub::DeviceScan::InclusiveSum(nullptr, t1, ReqFlagIter(hipcub::CountingInputIterator<uint32_t>(0), ReqFlag{nullptr}),
                                         static_cast<uint64_t*>(nullptr), items);
  (void)hipcub::DeviceScan::InclusiveSum(nullptr, t2,
                                         ReqBytesIter(hipcub::CountingInputIterator<uint32_t>(0), ReqBytes{nullptr}),
                                         static_cast<uint64_t*>(nullptr), items);
  L->temp_bytes = std::max({t1, t2, size_t(256)});
  const uint64_t row_bytes = (uint64_t(n_layers) + 1) * sizeof(TarRequiredRow);
  L->tables_bytes = Up256(row_bytes) + Up256(cfg_len) + (skip ? Up256(sizeof(TarSkipTable)) : 0);
  L->blob_cap = name_bytes + n;  // every name and its NUL
  uint64_t at = 0;
  auto take = [&](uint64_t bytes) {
    const uint64_t o = at;
    at += Up256(bytes);
    return o;
  };
  L->tables = take(L->tables_bytes);
  L->cfg = L->tables + Up256(row_bytes);
  L->skip_tab = L->cfg + Up256(cfg_len);
  L->counts = take(uint64_t(n_layers) * sizeof(TarRequiredCounts));
  L->dec = take(n * 16);
  L->rrank = take(n * 8);
  L->brank = take(n * 8);
  L->temp = take(L->temp_bytes);
  L->recs = take(n * sizeof(tsg_tar_file_rec));
  L->blob = take(L->blob_cap);
  L->bytes = at;
  return true;
}

void TarRequiredTables(const TarRequiredLayout& L, const uint64_t* rec_base, const uint64_t* name_base, const char* cfg,
                       uint8_t* h_tables, const TarSkipTable* skip) {
  std::memset(h_tables, 0, size_t(L.tables_bytes));
  TarRequiredRow* rows = reinterpret_cast<TarRequiredRow*>(h_tables);
  for (uint32_t k = 0; k <= L.n_layers; k++) rows[k] = TarRequiredRow{rec_base[k], name_base[k]};
  if (L.cfg_len) std::memcpy(h_tables + (L.cfg - L.tables), cfg, L.cfg_len);
  if (L.skip && skip) std::memcpy(h_tables + (L.skip_tab - L.tables), skip, sizeof(TarSkipTable));
}

hipError_t TarRequiredRun(const TarRequiredLayout& L, const uint8_t* h_tables, const uint8_t* d_records,
                          const uint8_t* d_names, const PathTable* d_path, const SureTable* d_sure, uint8_t* d_req,
                          uint32_t grid_cap, hipStream_t s) {
  const hipError_t e = TarRequiredDecide(L, h_tables, d_records, d_names, d_path, d_sure, d_req, grid_cap, s);
  return e != hipSuccess ? e : TarRequiredFinish(L, d_records, d_names, d_req, grid_cap, s);
}

hipError_t TarRequiredDecide(const TarRequiredLayout& L, const uint8_t* h_tables, const uint8_t* d_records,
                             const uint8_t* d_names, const PathTable* d_path, const SureTable* d_sure, uint8_t* d_req,
                             uint32_t grid_cap, hipStream_t s) {
  hipError_t e = hipMemcpyAsync(d_req + L.tables, h_tables, L.tables_bytes, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return e;
  const TarRequiredRow* rows = reinterpret_cast<const TarRequiredRow*>(d_req + L.tables);
  uint4* dec = reinterpret_cast<uint4*>(d_req + L.dec);
  const uint4* recs = reinterpret_cast<const uint4*>(d_records);
  const uint64_t n = L.n;
  if (n) {
    const uint32_t grid = GridFor((n + kRThreads - 1) / kRThreads, grid_cap);
    if (d_path && d_sure)
      req_decide_kernel<true, true><<<grid, kRThreads, 0, s>>>(recs, d_names, n, rows, L.n_layers, L.name_bytes,
                                                               d_req + L.cfg, L.cfg_len, d_path, d_sure, dec);
    else if (d_path)
      req_decide_kernel<true, false><<<grid, kRThreads, 0, s>>>(recs, d_names, n, rows, L.n_layers, L.name_bytes,
                                                                d_req + L.cfg, L.cfg_len, d_path, nullptr, dec);
    else
      req_decide_kernel<false, false><<<grid, kRThreads, 0, s>>>(recs, d_names, n, rows, L.n_layers, L.name_bytes,
                                                                 d_req + L.cfg, L.cfg_len, nullptr, nullptr, dec);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t TarSkipMatchRun(const TarRequiredLayout& L, const uint8_t* d_records, const uint8_t* d_names, uint8_t* d_req,
                           uint32_t* d_n_dirs, uint32_t grid_cap, hipStream_t s) {
  hipError_t e = hipMemsetAsync(d_n_dirs, 0, 4, s);
  if (e != hipSuccess || L.n == 0) return e;
  if (!L.skip) return hipErrorInvalidValue;
  skip_match_kernel<<<GridFor((L.n + kRThreads - 1) / kRThreads, grid_cap), kRThreads, 0, s>>>(
      reinterpret_cast<const uint4*>(d_records), d_names, L.n, reinterpret_cast<const TarRequiredRow*>(d_req + L.tables),
      L.n_layers, reinterpret_cast<const TarSkipTable*>(d_req + L.skip_tab), reinterpret_cast<uint4*>(d_req + L.dec),
      d_n_dirs);
  return hipGetLastError();
}

hipError_t TarSkipUnderRun(const TarRequiredLayout& L, const uint8_t* d_records, const uint8_t* d_names, uint8_t* d_req,
                           TarSkipSlot* d_table, uint64_t slots, uint32_t grid_cap, hipStream_t s) {
  if (L.n == 0 || slots < 2 || (slots & (slots - 1)) || slots > (uint64_t(1) << 31)) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(d_table, 0xFF, slots * sizeof(TarSkipSlot), s);
  if (e != hipSuccess) return e;
  const uint32_t grid = GridFor((L.n + kRThreads - 1) / kRThreads, grid_cap);
  const uint4* recs = reinterpret_cast<const uint4*>(d_records);
  const TarRequiredRow* rows = reinterpret_cast<const TarRequiredRow*>(d_req + L.tables);
  uint4* dec = reinterpret_cast<uint4*>(d_req + L.dec);
  skip_build_kernel<<<grid, kRThreads, 0, s>>>(recs, d_names, L.n, rows, L.n_layers, dec, d_table, uint32_t(slots - 1));
  if ((e = hipGetLastError()) != hipSuccess) return e;
  skip_under_kernel<<<grid, kRThreads, 0, s>>>(recs, d_names, L.n, rows, L.n_layers, dec, d_table, uint32_t(slots - 1));
  return hipGetLastError();
}

hipError_t TarRequiredFinish(const TarRequiredLayout& L, const uint8_t* d_records, const uint8_t* d_names,
                             uint8_t* d_req, uint32_t grid_cap, hipStream_t s) {
  hipError_t e = hipSuccess;
  const TarRequiredRow* rows = reinterpret_cast<const TarRequiredRow*>(d_req + L.tables);
  TarRequiredCounts* counts = reinterpret_cast<TarRequiredCounts*>(d_req + L.counts);
  uint4* dec = reinterpret_cast<uint4*>(d_req + L.dec);
  uint64_t* rrank = reinterpret_cast<uint64_t*>(d_req + L.rrank);
  uint64_t* brank = reinterpret_cast<uint64_t*>(d_req + L.brank);
  const uint4* recs = reinterpret_cast<const uint4*>(d_records);
  const uint64_t n = L.n;
  if (n) {
    size_t tb = L.temp_bytes;
    if ((e = hipcub::DeviceScan::InclusiveSum(d_req + L.temp, tb,
                                              ReqFlagIter(hipcub::CountingInputIterator<uint32_t>(0), ReqFlag{dec}), rrank,
                                              int(n), s)) != hipSuccess)
      return e;
    tb = L.temp_bytes;
    if ((e = hipcub::DeviceScan::InclusiveSum(d_req + L.temp, tb,
                                              ReqBytesIter(hipcub::CountingInputIterator<uint32_t>(0), ReqBytes{dec}),
                                              brank, int(n), s)) != hipSuccess)
      return e;
  }
  req_totals_kernel<<<GridFor(L.n_layers, grid_cap), kRThreads, 0, s>>>(dec, rrank, brank, rows, L.n_layers, counts);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (n) {
    req_emit_kernel<<<GridFor((n + kRThreads - 1) / kRThreads, grid_cap), kRThreads, 0, s>>>(
        recs, d_names, n, rows, L.n_layers, dec, rrank, brank, L.blob_cap, reinterpret_cast<uint4*>(d_req + L.recs),
        d_req + L.blob);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace tsg
