// Device-only batches: mark the candidates' files, lay them out, pack them
// into the staging buffer (fetch.h).
//
//  mark_files     : a thread per candidate record sets flag[file]; the record
//                   count is read on the device (a fixed grid strides over it).
//  fetch_len      : per file, its packed length (0: not marked, or direct) and
//                   a 0/1 selector; the totals by atomics.
//  two exclusive scans (hipcub): packed offsets of every file, list positions.
//  fetch_compact  : the marked files' ids and packed offsets, compacted.
//  fetch_files    : a wave per (16-KiB block of the packed layout) x (file in
//                   it): 16-B stores to the staging buffer, whose blocks are
//                   16-B aligned by construction; the source by one aligned
//                   16-B load per block where file and layout agree mod 16, by
//                   two aligned loads and a byte shift where they do not, by
//                   byte loads for the blocks whose aligned source would leave
//                   the file (its first and last two) and for the ragged tail.
#include "fetch.h"

#include <hipcub/hipcub.hpp>

namespace tsg {
namespace {

constexpr int kFThreads = 256;

struct FetchLayout {  // offsets into the scratch
  size_t flag, len16, poff, sel, pos, list, lpoff, scan, scan_bytes, total;
};

FetchLayout LayoutOf(uint32_t n_files) {
  const size_t n1 = size_t(n_files) + 1;
  size_t t64 = 0, t32 = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t64, static_cast<const uint64_t*>(nullptr),
                                         static_cast<uint64_t*>(nullptr), int(n1));
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t32, static_cast<const uint32_t*>(nullptr),
                                         static_cast<uint32_t*>(nullptr), int(n1));
  auto up = [](size_t x) { return (x + 255) & ~size_t(255); };
  FetchLayout L;
  L.flag = 0;
  L.len16 = up(L.flag + n1 * 4);
  L.poff = up(L.len16 + n1 * 8);
  L.sel = up(L.poff + n1 * 8);
  L.pos = up(L.sel + n1 * 4);
  L.list = up(L.pos + n1 * 4);
  L.lpoff = up(L.list + n1 * 4);
  L.scan = up(L.lpoff + n1 * 8);
  L.scan_bytes = std::max(t64, t32);
  L.total = up(L.scan + L.scan_bytes);
  return L;
}

__global__ __launch_bounds__(kFThreads) void mark_files_kernel(const Candidate* __restrict__ cands,
                                                               const uint32_t* __restrict__ cand_count,
                                                               uint32_t cand_cap, uint32_t n_files,
                                                               uint32_t* __restrict__ flag) {
  // (an overflowed list counts past its capacity: only the records written)
  const uint32_t n = min(*cand_count, cand_cap);
  for (uint32_t i = blockIdx.x * kFThreads + threadIdx.x; i < n; i += gridDim.x * kFThreads) {
    const uint32_t f = cands[i].file;
    if (f < n_files && !(cands[i].flags & kCandDrop)) flag[f] = 1;  // (racing stores of the same value)
  }
}

__global__ __launch_bounds__(kFThreads) void fetch_len_kernel(const uint64_t* __restrict__ off,
                                                              const uint32_t* __restrict__ flag, uint32_t n_files,
                                                              uint64_t direct_bytes, uint64_t* __restrict__ len16,
                                                              uint32_t* __restrict__ sel, FetchCounters* ctr) {
  for (uint32_t f = blockIdx.x * kFThreads + threadIdx.x; f <= n_files; f += gridDim.x * kFThreads) {
    uint64_t l16 = 0;
    uint32_t s = 0;
    if (f < n_files && flag[f]) {
      const uint64_t len = off[f + 1] - off[f];
      atomicAdd(reinterpret_cast<unsigned long long*>(&ctr->n_files), 1ull);
      atomicAdd(reinterpret_cast<unsigned long long*>(&ctr->file_bytes), static_cast<unsigned long long>(len));
      if (len >= direct_bytes) {
        atomicAdd(reinterpret_cast<unsigned long long*>(&ctr->n_direct), 1ull);
      } else {
        l16 = (len + 15) & ~uint64_t(15);
        s = 1;
      }
    }
    len16[f] = l16;  // (entry n_files: 0, so the exclusive sums end with the totals)
    sel[f] = s;
  }
}

__global__ __launch_bounds__(kFThreads) void fetch_compact_kernel(const uint64_t* __restrict__ poff,
                                                                  const uint32_t* __restrict__ sel,
                                                                  const uint32_t* __restrict__ pos, uint32_t n_files,
                                                                  uint32_t* __restrict__ list,
                                                                  uint64_t* __restrict__ lpoff, FetchCounters* ctr) {
  for (uint32_t f = blockIdx.x * kFThreads + threadIdx.x; f <= n_files; f += gridDim.x * kFThreads) {
    if (f == n_files) {  // the end of the list: pos <= n_files, so lpoff has the room
      lpoff[pos[f]] = poff[f];
      ctr->packed_bytes = poff[f];
      ctr->n_packed = pos[f];
    } else if (sel[f]) {
      list[pos[f]] = f;
      lpoff[pos[f]] = poff[f];
    }
  }
}

__device__ __forceinline__ uint4 fload16(const uint8_t* p) { return *reinterpret_cast<const uint4*>(p); }

// dst [d, d + n) = src [s, s + n) for one wave; d is a multiple of 16 (and dst
// 16-B aligned); [fs, fe) is the file the bytes belong to: nothing outside it
// is read.
__device__ void fetch_copy(const uint8_t* __restrict__ src, uint64_t s, uint64_t fs, uint64_t fe,
                           uint8_t* __restrict__ dst, uint64_t d, uint64_t n, uint32_t lane) {
  const uint32_t k = uint32_t(s & 15);  // the source's byte shift against the 16-B blocks (wave-uniform)
  const uint32_t q = k >> 2, r = k & 3;
  for (uint64_t j = uint64_t(lane) * 16; j < n; j += 1024) {
    const uint64_t sp = s + j;
    if (j + 16 <= n) {
      uint4 o;
      const uint64_t sa = sp & ~uint64_t(15);
      if (k == 0) {
        o = fload16(src + sp);
      } else if (sa >= fs && sa + 32 <= fe) {
        const uint4 A = fload16(src + sa), B = fload16(src + sa + 16);
        const uint32_t w[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
        uint32_t v[4];
        switch (q) {  // wave-uniform
          case 0:
#pragma unroll
            for (int i = 0; i < 4; i++) v[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], r);
            break;
          case 1:
#pragma unroll
            for (int i = 0; i < 4; i++) v[i] = __builtin_amdgcn_alignbyte(w[i + 2], w[i + 1], r);
            break;
          case 2:
#pragma unroll
            for (int i = 0; i < 4; i++) v[i] = __builtin_amdgcn_alignbyte(w[i + 3], w[i + 2], r);
            break;
          default:
#pragma unroll
            for (int i = 0; i < 4; i++) v[i] = __builtin_amdgcn_alignbyte(w[i + 4], w[i + 3], r);
            break;
        }
        o = make_uint4(v[0], v[1], v[2], v[3]);
      } else {  // the aligned pair would leave the file: its own 16 bytes singly
        uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
        for (int b = 0; b < 16; b++) v[b >> 2] |= uint32_t(src[sp + b]) << (8 * (b & 3));
        o = make_uint4(v[0], v[1], v[2], v[3]);
      }
      *reinterpret_cast<uint4*>(dst + d + j) = o;
    } else {  // the ragged tail
      for (uint64_t b = j; b < n; b++) dst[d + b] = src[s + b];
    }
  }
}

__global__ __launch_bounds__(kFThreads) void fetch_files_kernel(const uint8_t* __restrict__ arena,
                                                                const uint64_t* __restrict__ off, uint32_t n_files,
                                                                const uint32_t* __restrict__ list,
                                                                const uint64_t* __restrict__ lpoff,
                                                                const FetchCounters* __restrict__ ctr, uint64_t w0,
                                                                uint64_t w1, uint8_t* __restrict__ stage) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t n_list = min(ctr->n_packed, uint64_t(n_files));
  const uint64_t end = min(w1, ctr->packed_bytes);
  if (n_list == 0 || end <= w0) return;
  const uint64_t waves = uint64_t(gridDim.x) * (kFThreads / 64);
  const uint64_t b0 = w0 / kFetchSeg, b1 = (end + kFetchSeg - 1) / kFetchSeg;
  for (uint64_t b = b0 + uint64_t(blockIdx.x) * (kFThreads / 64) + (threadIdx.x >> 6); b < b1; b += waves) {
    const uint64_t lo = b * kFetchSeg, hi = min(lo + kFetchSeg, end);  // (lo >= w0: w0 is a block edge)
    // the last list entry that starts at or before lo: lpoff[x] <= lo < lpoff[y]  (lpoff[0] = 0)
    uint64_t x = 0, y = n_list;
    while (y - x > 1) {
      const uint64_t mid = (x + y) >> 1;
      if (lpoff[mid] <= lo) x = mid;
      else y = mid;
    }
    for (uint64_t i = x; i < n_list; i++) {
      const uint64_t p0 = lpoff[i];
      if (p0 >= hi) break;
      const uint32_t f = list[i];
      if (f >= n_files) continue;
      const uint64_t fs = off[f], fe = off[f + 1];
      const uint64_t a = max(lo, p0), z = min(hi, p0 + (fe - fs));  // the file's bytes inside the block
      if (a < z) fetch_copy(arena, fs + (a - p0), fs, fe, stage, a - w0, z - a, lane);
    }
  }
}

uint32_t GridFor(uint64_t items) {
  const uint64_t g = (items + kFThreads - 1) / kFThreads;
  return uint32_t(g < 1 ? 1 : (g > 1024 ? 1024 : g));
}

}  // namespace

size_t FetchScratchBytes(uint32_t n_files) { return LayoutOf(n_files).total; }

uint32_t* FetchFlags(void* scratch, uint32_t n_files) {
  return reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(scratch) + LayoutOf(n_files).flag);
}

const uint32_t* FetchList(const void* scratch, uint32_t n_files) {
  return reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(scratch) + LayoutOf(n_files).list);
}

const uint64_t* FetchListOffsets(const void* scratch, uint32_t n_files) {
  return reinterpret_cast<const uint64_t*>(static_cast<const uint8_t*>(scratch) + LayoutOf(n_files).lpoff);
}

hipError_t FetchPlan(const Candidate* cands, const uint32_t* cand_count, uint32_t cand_cap, const uint64_t* off,
                     uint32_t n_files, uint64_t direct_bytes, void* scratch, FetchCounters* ctr, hipStream_t s) {
  const FetchLayout L = LayoutOf(n_files);
  uint8_t* sc = static_cast<uint8_t*>(scratch);
  uint32_t* flag = reinterpret_cast<uint32_t*>(sc + L.flag);
  uint64_t* len16 = reinterpret_cast<uint64_t*>(sc + L.len16);
  uint64_t* poff = reinterpret_cast<uint64_t*>(sc + L.poff);
  uint32_t* sel = reinterpret_cast<uint32_t*>(sc + L.sel);
  uint32_t* pos = reinterpret_cast<uint32_t*>(sc + L.pos);
  uint32_t* list = reinterpret_cast<uint32_t*>(sc + L.list);
  uint64_t* lpoff = reinterpret_cast<uint64_t*>(sc + L.lpoff);
  const int n1 = int(n_files) + 1;
  hipError_t e;
  if ((e = hipMemsetAsync(ctr, 0, sizeof(FetchCounters), s)) != hipSuccess) return e;
  if (cands) {
    if ((e = hipMemsetAsync(flag, 0, size_t(n1) * 4, s)) != hipSuccess) return e;
    // a fixed grid: the record count is known on the device only
    mark_files_kernel<<<256, kFThreads, 0, s>>>(cands, cand_count, cand_cap, n_files, flag);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  fetch_len_kernel<<<GridFor(uint64_t(n1)), kFThreads, 0, s>>>(off, flag, n_files, direct_bytes, len16, sel, ctr);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  size_t tb = L.scan_bytes;
  if ((e = hipcub::DeviceScan::ExclusiveSum(sc + L.scan, tb, len16, poff, n1, s)) != hipSuccess) return e;
  tb = L.scan_bytes;
  if ((e = hipcub::DeviceScan::ExclusiveSum(sc + L.scan, tb, sel, pos, n1, s)) != hipSuccess) return e;
  fetch_compact_kernel<<<GridFor(uint64_t(n1)), kFThreads, 0, s>>>(poff, sel, pos, n_files, list, lpoff, ctr);
  return hipGetLastError();
}

hipError_t FetchPack(const uint8_t* arena, const uint64_t* off, uint32_t n_files, const void* scratch,
                     const FetchCounters* ctr, uint64_t w0, uint64_t w1, uint8_t* stage, hipStream_t s) {
  if (w1 <= w0) return hipSuccess;
  if (w0 % kFetchSeg != 0 || w1 % 16 != 0) return hipErrorInvalidValue;
  const FetchLayout L = LayoutOf(n_files);
  const uint8_t* sc = static_cast<const uint8_t*>(scratch);
  const uint64_t blocks = (w1 - w0 + kFetchSeg - 1) / kFetchSeg;  // a wave per block, four per workgroup
  const uint32_t grid = uint32_t(std::min<uint64_t>(std::max<uint64_t>((blocks + 3) / 4, 1), 1024));
  fetch_files_kernel<<<grid, kFThreads, 0, s>>>(arena, off, n_files, reinterpret_cast<const uint32_t*>(sc + L.list),
                                                reinterpret_cast<const uint64_t*>(sc + L.lpoff), ctr, w0, w1, stage);
  return hipGetLastError();
}

}  // namespace tsg
