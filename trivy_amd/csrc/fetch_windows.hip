// Device-only batches, windows mode: mark the candidates' granules, rank them,
// pack them into the staging buffer (fetch_windows.h, fetch_layout.h).
//
//  mark_granules  : a wave per candidate record (a fixed grid strides over the
//                   records; their count is read on the device).  The lanes
//                   stride the bitmap words of the candidate's granules: an
//                   interior word is a plain store of all ones, the two edge
//                   words are atomic ORs.  Only idempotent ORs: no order, no
//                   spin.  A whole-file mark of a multi-MiB file is 64 lanes'
//                   work, not one thread's loop.
//  count_granules : per bitmap word, its popcount; the starts of runs (a set
//                   bit after a clear one), summed by atomics.
//  one exclusive sum (hipcub): each word's rank in the packed layout.
//  pack_granules  : 16 lanes per granule, four granules per wave and pass: the
//                   word by binary search of the ranks, the bit by its rank in
//                   the word, then one aligned 16-B load and one aligned 16-B
//                   store per lane.  No byte loads.
#include "fetch_windows.h"

#include <algorithm>

#include <hipcub/hipcub.hpp>

namespace tsg {
namespace {

constexpr int kWThreads = 256;

struct WinLayout {  // offsets into the scratch
  size_t bitmap, cnt, rank, whole, scan, scan_bytes, total;
  uint32_t n_words;
};

WinLayout LayoutOf(uint64_t n_bytes, uint32_t n_files) {
  const uint64_t gran = FetchGranules(n_bytes);
  WinLayout L;
  L.n_words = uint32_t((gran + 31) / 32);
  const size_t n1 = size_t(L.n_words) + 1;
  size_t t32 = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t32, static_cast<const uint32_t*>(nullptr),
                                         static_cast<uint32_t*>(nullptr), int(n1));
  auto up = [](size_t x) { return (x + 255) & ~size_t(255); };
  L.bitmap = 0;
  L.cnt = up(L.bitmap + n1 * 4);
  L.rank = up(L.cnt + n1 * 4);
  L.whole = up(L.rank + n1 * 4);
  L.scan = up(L.whole + (size_t(n_files) + 1) * 4);
  L.scan_bytes = t32;
  L.total = up(L.scan + L.scan_bytes);
  return L;
}

__global__ __launch_bounds__(kWThreads) void mark_granules_kernel(
    const Candidate* __restrict__ cands, const uint32_t* __restrict__ cand_count, uint32_t cand_cap,
    const uint64_t* __restrict__ off, uint32_t n_files, uint64_t n_gran, const uint32_t* __restrict__ rule_max_len,
    uint32_t n_rules, FetchWinParams prm, uint32_t* __restrict__ bitmap, uint32_t* __restrict__ whole,
    FetchWinCounters* ctr) {
  // (an overflowed list counts past its capacity: only the records written)
  const uint32_t n = min(*cand_count, cand_cap);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t waves = gridDim.x * (kWThreads / 64);
  for (uint32_t i = blockIdx.x * (kWThreads / 64) + (threadIdx.x >> 6); i < n; i += waves) {
    const Candidate c = cands[i];  // (wave-uniform)
    if (c.file >= n_files || (c.flags & kCandDrop)) continue;
    uint64_t g0, g1;
    bool all;
    const uint32_t ml = c.rule < n_rules ? rule_max_len[c.rule] : kFetchNoMaxLen;
    if (!CandidateGranules(c.wlo, c.whi, ml, off[c.file], off[c.file + 1], prm, &g0, &g1, &all)) continue;
    if (g1 > n_gran) g1 = n_gran;  // (offsets past the arena: the bitmap has no such bits)
    if (g0 >= g1) continue;
    if (all && lane == 0 && atomicExch(&whole[c.file], 1u) == 0u)
      atomicAdd(reinterpret_cast<unsigned long long*>(&ctr->whole_files), 1ull);
    const uint64_t w0 = g0 >> 5, w1 = (g1 - 1) >> 5;
    for (uint64_t w = w0 + lane; w <= w1; w += 64) {
      uint32_t m = ~0u;
      if (w == w0) m &= ~0u << uint32_t(g0 & 31);
      if (w == w1) m &= ~0u >> (31u - uint32_t((g1 - 1) & 31));
      if (w == w0 || w == w1) atomicOr(&bitmap[w], m);
      else bitmap[w] = ~0u;  // (racing stores and ORs all end in all ones)
    }
  }
}

__global__ __launch_bounds__(kWThreads) void count_granules_kernel(const uint32_t* __restrict__ bitmap,
                                                                   uint32_t n_words, uint32_t* __restrict__ cnt,
                                                                   FetchWinCounters* ctr) {
  for (uint32_t w = blockIdx.x * kWThreads + threadIdx.x; w <= n_words; w += gridDim.x * kWThreads) {
    uint32_t c = 0;
    if (w < n_words) {
      const uint32_t m = bitmap[w];
      if (m) {
        c = uint32_t(__popc(m));
        const uint32_t prev = w > 0 ? bitmap[w - 1] >> 31 : 0u;
        const uint32_t starts = uint32_t(__popc(m & ~((m << 1) | prev)));
        if (starts) atomicAdd(reinterpret_cast<unsigned long long*>(&ctr->runs), static_cast<unsigned long long>(starts));
      }
    }
    cnt[w] = c;  // (entry n_words: 0, so the exclusive sum ends with the total)
  }
}

__global__ void finish_granules_kernel(const uint32_t* __restrict__ rank, uint32_t n_words, FetchWinCounters* ctr) {
  ctr->granules = rank[n_words];
}

__global__ __launch_bounds__(kWThreads) void pack_granules_kernel(const uint8_t* __restrict__ arena, uint64_t n_bytes,
                                                                  const uint32_t* __restrict__ bitmap,
                                                                  const uint32_t* __restrict__ rank, uint32_t n_words,
                                                                  const FetchWinCounters* __restrict__ ctr, uint64_t p0,
                                                                  uint64_t p1, uint8_t* __restrict__ stage) {
  const uint32_t lane = threadIdx.x & 63u, sub = lane >> 4, l = lane & 15u;
  const uint64_t end = min(p1, min(ctr->granules, uint64_t(rank[n_words])));
  const uint64_t waves = uint64_t(gridDim.x) * (kWThreads / 64);
  const uint64_t wave = uint64_t(blockIdx.x) * (kWThreads / 64) + (threadIdx.x >> 6);
  for (uint64_t q = p0 + 4 * wave + sub; q < end; q += 4 * waves) {
    // the word that holds packed granule q: rank[x] <= q < rank[y]  (rank[0] = 0, rank[n_words] = the total > q)
    uint32_t x = 0, y = n_words;
    while (y - x > 1) {
      const uint32_t mid = x + ((y - x) >> 1);
      if (rank[mid] <= q) x = mid;
      else y = mid;
    }
    uint32_t m = bitmap[x];
    for (uint32_t k = uint32_t(q) - rank[x]; k > 0 && m; k--) m &= m - 1;  // drop the set bits before it
    if (!m) continue;
    const uint64_t g = uint64_t(x) * 32 + uint32_t(__ffs(int(m)) - 1);
    const uint64_t b = g * kFetchGranule + l * 16;
    // the arena is readable to n_bytes + 64: a 16-B block that begins below n_bytes ends within it
    if (b < n_bytes)
      *reinterpret_cast<uint4*>(stage + (q - p0) * kFetchGranule + l * 16) =
          *reinterpret_cast<const uint4*>(arena + b);
  }
}

uint32_t GridFor(uint64_t items) {
  const uint64_t g = (items + kWThreads - 1) / kWThreads;
  return uint32_t(g < 1 ? 1 : (g > 1024 ? 1024 : g));
}

}  // namespace

size_t FetchWinScratchBytes(uint64_t n_bytes, uint32_t n_files) { return LayoutOf(n_bytes, n_files).total; }

hipError_t FetchWinPlan(const Candidate* cands, const uint32_t* cand_count, uint32_t cand_cap, const uint64_t* off,
                        uint32_t n_files, uint64_t n_bytes, const uint32_t* rule_max_len, uint32_t n_rules,
                        const FetchWinParams& prm, void* scratch, FetchWinCounters* ctr, hipStream_t s) {
  const WinLayout L = LayoutOf(n_bytes, n_files);
  uint8_t* sc = static_cast<uint8_t*>(scratch);
  uint32_t* bitmap = reinterpret_cast<uint32_t*>(sc + L.bitmap);
  uint32_t* cnt = reinterpret_cast<uint32_t*>(sc + L.cnt);
  uint32_t* rank = reinterpret_cast<uint32_t*>(sc + L.rank);
  uint32_t* whole = reinterpret_cast<uint32_t*>(sc + L.whole);
  const int n1 = int(L.n_words) + 1;
  hipError_t e;
  if ((e = hipMemsetAsync(ctr, 0, sizeof(FetchWinCounters), s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(bitmap, 0, size_t(n1) * 4, s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(whole, 0, (size_t(n_files) + 1) * 4, s)) != hipSuccess) return e;
  // a fixed grid: the record count is known on the device only
  mark_granules_kernel<<<256, kWThreads, 0, s>>>(cands, cand_count, cand_cap, off, n_files, FetchGranules(n_bytes),
                                                 rule_max_len, n_rules, prm, bitmap, whole, ctr);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  count_granules_kernel<<<GridFor(uint64_t(n1)), kWThreads, 0, s>>>(bitmap, L.n_words, cnt, ctr);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  size_t tb = L.scan_bytes;
  if ((e = hipcub::DeviceScan::ExclusiveSum(sc + L.scan, tb, cnt, rank, n1, s)) != hipSuccess) return e;
  finish_granules_kernel<<<1, 1, 0, s>>>(rank, L.n_words, ctr);
  return hipGetLastError();
}

hipError_t FetchWinPack(const uint8_t* arena, uint64_t n_bytes, const void* scratch, uint32_t n_files,
                        const FetchWinCounters* ctr, uint64_t w0, uint64_t w1, uint8_t* stage, hipStream_t s) {
  if (w1 <= w0) return hipSuccess;
  if (w0 % kFetchGranule != 0 || w1 % kFetchGranule != 0) return hipErrorInvalidValue;
  const WinLayout L = LayoutOf(n_bytes, n_files);
  if (L.n_words == 0) return hipSuccess;
  const uint8_t* sc = static_cast<const uint8_t*>(scratch);
  const uint64_t gran = (w1 - w0) / kFetchGranule;  // four per wave and pass, sixteen per workgroup
  const uint32_t grid = uint32_t(std::min<uint64_t>(std::max<uint64_t>((gran + 15) / 16, 1), 1024));
  pack_granules_kernel<<<grid, kWThreads, 0, s>>>(arena, n_bytes, reinterpret_cast<const uint32_t*>(sc + L.bitmap),
                                                  reinterpret_cast<const uint32_t*>(sc + L.rank), L.n_words, ctr,
                                                  w0 / kFetchGranule, w1 / kFetchGranule, stage);
  return hipGetLastError();
}

}  // namespace tsg
