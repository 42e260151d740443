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

#include "tarchain_dev.h"  // the entry parse and the rank scans' inputs, shared with tarforest.hip

namespace tsg {
namespace {

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

struct WordPop {
  __host__ __device__ uint64_t operator()(uint64_t w) const {
#if defined(__HIP_DEVICE_COMPILE__)
    return uint64_t(__popcll(w));
#else
    return uint64_t(__builtin_popcountll(w));
#endif
  }
};
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
    write_entry(tar, e, b * 512u, off, records + r * 64u, names + off);
  }
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
