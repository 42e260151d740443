// The header chains of all layers of an image resident in HBM in one pass
// (tarforest.h, tarindex.h): the stages of tarchain.hip over the virtual block
// space of the layers, every lane finding its layer through the u32 of its
// segment.
//
//  forest_bitmap  : a wave per 64 virtual blocks, tarindex.hip's group_mask over
//                   the blocks of the layer that owns them; padding is not read
//                   and its bits are 0.
//  forest_entries : a lane per virtual block; tarchain.hip's entry parse with the
//                   layer's pointer, its bound n_bytes_k and its slice of the
//                   bitmap.  succ is a block of the layer, or a terminal word.
//  forest_exits   : a workgroup per segment, as tar_exits.
//  forest_stitch  : a wave per layer follows that layer's chain from its block 0
//                   through the exits -- one dependent load per segment entered;
//                   the waves of the layers run side by side -- and writes the
//                   layer's stop.  A layer without a complete block stops
//                   without a read.
//  forest_mark    : a workgroup per segment, as tar_mark; the segments of a layer
//                   whose stop is INCOMPLETE get no mark, so it takes no record.
//  ranks          : one inclusive sum of the on-chain bit and one of the name
//                   lengths over the whole virtual space.
//  forest_totals  : a workgroup per layer: entries and name bytes from the sums
//                   at the layer's two ends, the candidates from its bitmap.
//  forest_compact : a lane per on-chain entry: its record at its global rank,
//                   its name at its global offset; name_off relative to the
//                   layer's first name.
// Vector stores only; no atomics; no lane waits on another workgroup.  Every
// loop ends at a cap of tarchain.h, at the layer's bound or at its segments.
#include "tarindex.h"

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>

#include "tarchain_dev.h"
#include "tarindex_dev.h"

namespace tsg {
namespace {

__device__ __forceinline__ TarForestLayer layer_at(const TarForestLayer* __restrict__ layers, uint32_t k) {
  const uint4* w = reinterpret_cast<const uint4*>(layers + k);
  const uint4 a = w[0], b = w[1];
  TarForestLayer y;
  y.ptr = reinterpret_cast<const uint8_t*>(uint64_t(a.x) | (uint64_t(a.y) << 32));
  y.n_bytes = uint64_t(a.z) | (uint64_t(a.w) << 32);
  y.n_blocks = uint64_t(b.x) | (uint64_t(b.y) << 32);
  y.v0 = uint64_t(b.z) | (uint64_t(b.w) << 32);
  return y;
}

__global__ __launch_bounds__(kCThreads) void forest_bitmap_kernel(const TarForestLayer* __restrict__ layers,
                                                                  const uint32_t* __restrict__ seg_layer,
                                                                  uint32_t seg_shift, uint64_t n_segments,
                                                                  uint64_t n_groups, uint64_t* __restrict__ bitmap) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t l = lane & 31u, half = lane >> 5;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t sub = min(1u << seg_shift, kGroupBlocks);  // blocks of a group that surely share a layer
  for (uint64_t g = uint64_t(blockIdx.x) * 4u + wave; g < n_groups; g += uint64_t(gridDim.x) * 4u) {
    uint64_t mask = 0;
    for (uint32_t j = 0; j < kGroupBlocks; j += sub) {  // (everything here is wave-uniform)
      const uint64_t v = g * kGroupBlocks + j;
      if ((v >> seg_shift) >= n_segments) break;
      const uint32_t k = __builtin_amdgcn_readfirstlane(seg_layer[v >> seg_shift]);
      const TarForestLayer y = layer_at(layers, k);
      const uint64_t g0 = v - y.v0;
      if (g0 >= y.n_blocks) continue;  // padding: not read
      // the bound keeps the verdict inside this layer's `sub` blocks: blocks at or past it are not read
      mask |= group_mask(y.ptr, min(y.n_blocks, g0 + sub), g0, l, half) << j;
    }
    if (lane == 0) bitmap[g] = mask;
  }
}

__global__ __launch_bounds__(kCThreads) void forest_entries_kernel(const TarForestLayer* __restrict__ layers,
                                                                   const uint32_t* __restrict__ seg_layer,
                                                                   uint32_t seg_shift, uint64_t v_blocks,
                                                                   const uint8_t* __restrict__ cand,
                                                                   uint32_t* __restrict__ succ,
                                                                   uint32_t* __restrict__ nlen) {
  for (uint64_t v = uint64_t(blockIdx.x) * kCThreads + threadIdx.x; v < v_blocks; v += uint64_t(gridDim.x) * kCThreads) {
    if (!bit_at(cand, v)) {  // (padding too: its bits are 0)
      succ[v] = kNonCand;
      continue;
    }
    const TarForestLayer y = layer_at(layers, seg_layer[v >> seg_shift]);
    const uint64_t b = v - y.v0;
    if (b >= y.n_blocks) {
      succ[v] = kNonCand;
      continue;
    }
    const Entry e = chain_entry(y.ptr, y.n_bytes, y.n_blocks, cand + y.v0 / 8u, b);  // (v0: a multiple of 8)
    if (e.end || e.reason != kTarOk) {
      succ[v] = kTerm | (e.reason << 8) | e.n_ext;  // (reason 0: END)
    } else {
      succ[v] = uint32_t(e.next / 512u);  // in the layer: > b, <= n_blocks + 1 < 2^31
      nlen[v] = e.name_len;
    }
  }
}

// The blocks of the layer in segment sg of the virtual space: [*s0, *s0 + m) of the layer; m may be 0 (padding).
// forest_exits_kernel and forest_mark_kernel below are tarchain.hip's tar_exits_kernel and tar_mark_kernel with s0
// and m taken from here (and, in the marking, the head check): a change to one pair belongs in the other.
__device__ __forceinline__ uint32_t segment_of(const TarForestLayer& y, uint64_t sg, uint32_t seg, uint64_t* s0) {
  *s0 = sg * seg - y.v0;
  return *s0 >= y.n_blocks ? 0u : uint32_t(min(uint64_t(seg), y.n_blocks - *s0));
}

__global__ __launch_bounds__(kCThreads) void forest_exits_kernel(const TarForestLayer* __restrict__ layers,
                                                                 const uint32_t* __restrict__ seg_layer,
                                                                 const uint32_t* __restrict__ succ, uint32_t seg,
                                                                 uint64_t n_segments, uint32_t* __restrict__ exits) {
  extern __shared__ uint32_t v[];  // seg words
  for (uint64_t sg = blockIdx.x; sg < n_segments; sg += gridDim.x) {
    const TarForestLayer y = layer_at(layers, seg_layer[sg]);
    uint64_t s0;
    const uint32_t m = segment_of(y, sg, seg, &s0);  // (workgroup-uniform)
    const uint64_t s1 = s0 + m, at = sg * seg;       // at: the segment's first virtual block
    for (uint32_t i = threadIdx.x; i < m; i += kCThreads) {
      const uint32_t w = succ[at + i];
      v[i] = (w & kTerm) ? (kTerm | uint32_t(s0 + i)) : w;
    }
    __syncthreads();
    // as tar_exits_kernel: a word only moves forward along its block's chain, so the rounds work in place
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
    for (uint32_t i = threadIdx.x; i < m; i += kCThreads) exits[at + i] = v[i];
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void forest_stitch_kernel(const TarForestLayer* __restrict__ layers, uint32_t n_layers,
                                                           uint32_t seg_shift, const uint32_t* __restrict__ succ,
                                                           const uint32_t* __restrict__ exits,
                                                           uint32_t* __restrict__ seg_entry,
                                                           TarChainHead* __restrict__ heads) {
  const uint32_t lane = threadIdx.x;
  for (uint32_t k = blockIdx.x; k < n_layers; k += gridDim.x) {
    const TarForestLayer y = layer_at(layers, k);
    const uint64_t n = y.n_bytes, n_blocks = y.n_blocks;
    const uint64_t n_segments = (n_blocks + (uint64_t(1) << seg_shift) - 1) >> seg_shift;
    uint64_t e = 0, steps = 0, ext = 0;
    uint32_t kind = kTarStopEnd, reason = kTarOk;
    uint64_t at = 0;
    for (uint64_t it = 0; it <= n_segments; it++) {  // every step enters a later segment of the layer
      if (e >= n_blocks) {                           // (at once for a layer without a complete block)
        at = e * 512u;
        if (at < n) {
          kind = kTarStopIncomplete;
          reason = kTarTruncated;
        }
        break;
      }
      if (lane == 0) seg_entry[(y.v0 + e) >> seg_shift] = uint32_t(e);
      const uint32_t x = exits[y.v0 + e];
      steps++;
      if (!(x & kTerm)) {
        e = x;
        continue;
      }
      const uint64_t b = x & ~kTerm;
      at = b * 512u;
      const uint32_t w = succ[y.v0 + b];
      if (w == kNonCand) {
        const uint2 q = *reinterpret_cast<const uint2*>(y.ptr + at + lane * 8u);  // (b < n_blocks: a complete block)
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
      uint4* o = reinterpret_cast<uint4*>(&heads[k].stop);
      o[0] = make_uint4(kind, reason, uint32_t(at), uint32_t(at >> 32));
      o[1] = make_uint4(uint32_t(ext), 0u, uint32_t(steps), uint32_t(steps >> 32));
    }
  }
}

__global__ __launch_bounds__(kCThreads) void forest_mark_kernel(const TarForestLayer* __restrict__ layers,
                                                                const uint32_t* __restrict__ seg_layer,
                                                                const TarChainHead* __restrict__ heads,
                                                                const uint32_t* __restrict__ succ, uint32_t seg,
                                                                uint64_t n_segments,
                                                                const uint32_t* __restrict__ seg_entry,
                                                                uint8_t* __restrict__ chain) {
  extern __shared__ uint32_t v[];  // seg words, then seg / 8 bytes of bits
  uint8_t* bits = reinterpret_cast<uint8_t*>(v + seg);
  for (uint64_t sg = blockIdx.x; sg < n_segments; sg += gridDim.x) {
    const uint32_t k = seg_layer[sg];
    const TarForestLayer y = layer_at(layers, k);
    uint64_t s0;
    const uint32_t m = segment_of(y, sg, seg, &s0);
    const uint64_t s1 = s0 + m, at = sg * seg;
    // an INCOMPLETE layer hands nothing over: no mark, so no rank and no record
    const uint32_t entry = (m == 0 || heads[k].stop.kind != kTarStopEnd) ? kNoEntry : seg_entry[sg];
    if (entry != kNoEntry)  // (workgroup-uniform)
      for (uint32_t i = threadIdx.x; i < m; i += kCThreads) v[i] = succ[at + i];
    for (uint32_t i = threadIdx.x; i < seg / 8u; i += kCThreads) bits[i] = 0;
    __syncthreads();
    if (entry != kNoEntry && threadIdx.x == 0) {
      uint64_t cur = entry;  // s0 <= entry < s1
      while (cur >= s0 && cur < s1) {  // successors point forward: at most m steps
        const uint32_t w = v[cur - s0];
        if (w & kTerm) break;
        bits[(cur - s0) >> 3] |= uint8_t(1u << ((cur - s0) & 7u));
        cur = w;
      }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < seg / 8u; i += kCThreads) chain[at / 8u + i] = bits[i];
    __syncthreads();
  }
}

__global__ __launch_bounds__(kCThreads) void forest_totals_kernel(const TarForestLayer* __restrict__ layers,
                                                                  uint32_t n_layers, uint32_t seg_shift,
                                                                  const uint8_t* __restrict__ cand,
                                                                  const uint32_t* __restrict__ rank,
                                                                  const uint64_t* __restrict__ noff,
                                                                  TarChainHead* __restrict__ heads) {
  __shared__ uint64_t part[kCThreads / 64];
  for (uint32_t k = blockIdx.x; k < n_layers; k += gridDim.x) {
    const TarForestLayer y = layer_at(layers, k);
    // the candidates: the bits of the layer's slice of the bitmap (the bits past its blocks are 0)
    uint64_t c = 0;
    if (seg_shift >= 6) {  // the slice is whole 64-bit words
      const uint64_t* w = reinterpret_cast<const uint64_t*>(cand) + y.v0 / 64u;
      for (uint64_t i = threadIdx.x; i < (y.n_blocks + 63u) / 64u; i += kCThreads) c += uint64_t(__popcll(w[i]));
    } else {
      const uint8_t* w = cand + y.v0 / 8u;
      for (uint64_t i = threadIdx.x; i < (y.n_blocks + 7u) / 8u; i += kCThreads) c += uint64_t(__popc(uint32_t(w[i])));
    }
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint64_t cands = 0;
      for (uint32_t i = 0; i < kCThreads / 64; i++) cands += part[i];
      const uint64_t blocks = y.n_blocks ? y.n_blocks : 1u;
      const uint64_t span = ((blocks + (uint64_t(1) << seg_shift) - 1) >> seg_shift) << seg_shift;
      const uint64_t last = y.v0 + span - 1u;
      const uint64_t entries = uint64_t(rank[last]) - (y.v0 ? uint64_t(rank[y.v0 - 1u]) : 0u);
      const uint64_t names = noff[last] - (y.v0 ? noff[y.v0 - 1u] : 0u);
      uint4* o = reinterpret_cast<uint4*>(&heads[k].entries);
      o[0] = make_uint4(uint32_t(entries), uint32_t(entries >> 32), uint32_t(names), uint32_t(names >> 32));
      o[1] = make_uint4(uint32_t(cands), uint32_t(cands >> 32), 0u, 0u);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kCThreads) void forest_compact_kernel(const TarForestLayer* __restrict__ layers,
                                                                   const uint32_t* __restrict__ seg_layer,
                                                                   uint32_t seg_shift, uint64_t v_blocks,
                                                                   const uint8_t* __restrict__ cand,
                                                                   const uint8_t* __restrict__ chain,
                                                                   const uint32_t* __restrict__ rank,
                                                                   const uint64_t* __restrict__ noff,
                                                                   uint64_t n_entries, uint64_t name_bytes,
                                                                   uint8_t* __restrict__ records,
                                                                   uint8_t* __restrict__ names) {
  for (uint64_t v = uint64_t(blockIdx.x) * kCThreads + threadIdx.x; v < v_blocks; v += uint64_t(gridDim.x) * kCThreads) {
    if (!bit_at(chain, v)) continue;
    const TarForestLayer y = layer_at(layers, seg_layer[v >> seg_shift]);
    const uint64_t b = v - y.v0;
    if (b >= y.n_blocks) continue;
    const Entry e = chain_entry(y.ptr, y.n_bytes, y.n_blocks, cand + y.v0 / 8u, b);  // (complete: it was marked)
    const uint64_t r = uint64_t(rank[v]) - 1u;
    const uint64_t base = y.v0 ? noff[y.v0 - 1u] : 0u;  // the layer's first name
    const uint64_t end = noff[v];
    // (a layer that changed under the pass: nothing is written outside the counted records and names)
    if (e.end || e.reason != kTarOk || r >= n_entries || end > name_bytes || end < base + e.name_len) continue;
    const uint64_t off = end - e.name_len;
    write_entry(y.ptr, e, b * 512u, off - base, records + r * 64u, names + off);
  }
}

}  // namespace

bool TarForestPlan(const uint64_t* n_bytes, uint32_t n_layers, uint32_t segment_blocks, TarForestLayout* L) {
  const uint32_t seg = segment_blocks ? segment_blocks : kTarDefaultSegment;
  if (seg < kTarMinSegment || (seg & (seg - 1)) || uint64_t(seg) * 4 + seg / 8 > (64u << 10)) return false;
  if (n_layers == 0 || n_layers > kTarForestMaxLayers) return false;
  if (TarForestCut(n_bytes, n_layers, 0, seg) != n_layers) return false;
  uint64_t vb = 0;
  for (uint32_t k = 0; k < n_layers; k++) vb += TarForestSpan(n_bytes[k], seg);
  *L = TarForestLayout();
  L->n_layers = n_layers;
  L->v_blocks = vb;
  L->segment = seg;
  L->n_segments = vb / seg;
  size_t t1 = 0, t2 = 0;
  (void)hipcub::DeviceScan::InclusiveSum(nullptr, t1, FlagIter(hipcub::CountingInputIterator<uint32_t>(0), ChainFlag{nullptr}),
                                         static_cast<uint32_t*>(nullptr), int(vb));
  (void)hipcub::DeviceScan::InclusiveSum(nullptr, t2,
                                         NameIter(hipcub::CountingInputIterator<uint32_t>(0), ChainNameLen{nullptr, nullptr}),
                                         static_cast<uint64_t*>(nullptr), int(vb));
  L->temp_bytes = std::max({t1, t2, size_t(256)});
  const uint64_t bm = Up256((vb + 63) / 64 * 8);  // whole 64-bit words of candidates; whole segments of the chain
  uint64_t at = 0;
  auto take = [&](uint64_t bytes) {
    const uint64_t o = at;
    at += Up256(bytes);
    return o;
  };
  L->heads = take(uint64_t(n_layers) * sizeof(TarChainHead));
  L->layers = take(uint64_t(n_layers) * sizeof(TarForestLayer));
  L->seg_layer = take(L->n_segments * 4);
  L->tables_bytes = at - L->layers;
  L->cand = take(bm);
  L->chain = take(bm);
  L->seg_entry = take(L->n_segments * 4);
  L->succ = take(vb * 4);
  L->nlen = take(vb * 4);
  L->rank = take(vb * 4);
  L->noff = take(vb * 8);
  L->temp = take(L->temp_bytes);
  L->bytes = at;
  return true;
}

void TarForestTables(const TarForestLayout& L, const void* const* ptrs, const uint64_t* n_bytes, uint8_t* h_tables) {
  std::memset(h_tables, 0, size_t(L.tables_bytes));
  TarForestLayer* ly = reinterpret_cast<TarForestLayer*>(h_tables);
  uint32_t* seg_layer = reinterpret_cast<uint32_t*>(h_tables + (L.seg_layer - L.layers));
  uint64_t v = 0;
  for (uint32_t k = 0; k < L.n_layers; k++) {
    ly[k].ptr = static_cast<const uint8_t*>(ptrs[k]);
    ly[k].n_bytes = n_bytes[k];
    ly[k].n_blocks = n_bytes[k] / 512;
    ly[k].v0 = v;
    const uint64_t span = TarForestSpan(n_bytes[k], L.segment);
    for (uint64_t sg = v / L.segment; sg < (v + span) / L.segment; sg++) seg_layer[sg] = k;
    v += span;
  }
}

hipError_t TarForestWalk(const TarForestLayout& L, const uint8_t* h_tables, uint8_t* d_work, uint32_t grid_cap,
                         hipStream_t s, hipEvent_t* ev) {
  const uint64_t vb = L.v_blocks;
  if (vb == 0 || L.n_layers == 0) return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  auto rec = [&](int i) { return ev ? hipEventRecord(ev[i], s) : hipSuccess; };
  TarChainHead* heads = reinterpret_cast<TarChainHead*>(d_work + L.heads);
  const TarForestLayer* layers = reinterpret_cast<const TarForestLayer*>(d_work + L.layers);
  const uint32_t* seg_layer = reinterpret_cast<const uint32_t*>(d_work + L.seg_layer);
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
  const uint32_t blk_grid = GridFor((vb + kCThreads - 1) / kCThreads, grid_cap);
  const uint32_t layer_grid = GridFor(L.n_layers, grid_cap);
  const uint64_t n_groups = (vb + kGroupBlocks - 1) / kGroupBlocks;
  if ((e = hipMemcpyAsync(d_work + L.layers, h_tables, L.tables_bytes, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(heads, 0, uint64_t(L.n_layers) * sizeof(TarChainHead), s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(seg_entry, 0xFF, L.n_segments * 4, s)) != hipSuccess) return e;
  if ((e = rec(0)) != hipSuccess) return e;  // (after the upload and the memsets: the stage times are the kernels')
  forest_bitmap_kernel<<<GridFor((n_groups + 3) / 4, grid_cap), kCThreads, 0, s>>>(layers, seg_layer, shift, L.n_segments,
                                                                                  n_groups, cand64);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = rec(1)) != hipSuccess) return e;
  forest_entries_kernel<<<blk_grid, kCThreads, 0, s>>>(layers, seg_layer, shift, vb, cand, succ, nlen);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = rec(2)) != hipSuccess) return e;
  forest_exits_kernel<<<seg_grid, kCThreads, lds_exits, s>>>(layers, seg_layer, succ, L.segment, L.n_segments, rank);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  forest_stitch_kernel<<<layer_grid, 64, 0, s>>>(layers, L.n_layers, shift, succ, rank, seg_entry, heads);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  forest_mark_kernel<<<seg_grid, kCThreads, lds_mark, s>>>(layers, seg_layer, heads, succ, L.segment, L.n_segments,
                                                           seg_entry, chain);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  size_t tb = L.temp_bytes;
  if ((e = hipcub::DeviceScan::InclusiveSum(temp, tb, FlagIter(hipcub::CountingInputIterator<uint32_t>(0), ChainFlag{chain}),
                                            rank, int(vb), s)) != hipSuccess)
    return e;
  tb = L.temp_bytes;
  if ((e = hipcub::DeviceScan::InclusiveSum(
           temp, tb, NameIter(hipcub::CountingInputIterator<uint32_t>(0), ChainNameLen{chain, nlen}), noff, int(vb), s)) !=
      hipSuccess)
    return e;
  forest_totals_kernel<<<layer_grid, kCThreads, 0, s>>>(layers, L.n_layers, shift, cand, rank, noff, heads);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return rec(3);
}

hipError_t TarForestCompact(const TarForestLayout& L, const uint8_t* d_work, uint64_t n_entries, uint64_t name_bytes,
                            uint8_t* d_records, uint8_t* d_names, uint32_t grid_cap, hipStream_t s) {
  if (L.v_blocks == 0 || n_entries == 0) return hipSuccess;
  uint32_t shift = 0;
  while ((1u << shift) < L.segment) shift++;
  forest_compact_kernel<<<GridFor((L.v_blocks + kCThreads - 1) / kCThreads, grid_cap), kCThreads, 0, s>>>(
      reinterpret_cast<const TarForestLayer*>(d_work + L.layers), reinterpret_cast<const uint32_t*>(d_work + L.seg_layer),
      shift, L.v_blocks, d_work + L.cand, d_work + L.chain, reinterpret_cast<const uint32_t*>(d_work + L.rank),
      reinterpret_cast<const uint64_t*>(d_work + L.noff), n_entries, name_bytes, d_records, d_names);
  return hipGetLastError();
}

}  // namespace tsg
