// The tar index of a layer resident in HBM (tarindex.h).
//
//  tar_headers : a wave per group of eight 4-KiB tiles (eight 512-B blocks each), grid-stride.  A
//                block is half a wave: 32 lanes x one aligned 16-B load, so a
//                wave-wide load reads 1 KiB contiguously; the four loads of a
//                tile are issued before the first is used.  Per block the
//                kernel decides what analyzer.cpp's ChecksumOK decides:
//                  - every lane sums its 16 bytes (v_sad_u8 against zero) and
//                    counts the bytes >= 0x80; lane 9 of the half holds bytes
//                    144..159, leaves the checksum field's eight bytes
//                    (148..155) out of both and adds 8 x 0x20 for the spaces
//                    they count as, and parses the field (base-256 or octal,
//                    trimmed of spaces and NULs, as ParseNumeric does);
//                  - sum and count travel packed in one word (the sum stays
//                    below 2^20) through four row-rotate DPP adds, and the two
//                    16-lane rows of a half are added from v_readlane values,
//                    so the verdict is wave-uniform: the field equals the
//                    unsigned sum, or the signed one = unsigned - 256 x count.
//                An all-zero block needs no test of its own: its field parses
//                as 0 and its sum, with the spaces, is 256.
//                The wave keeps one bit per block of its group.  One atomicAdd
//                per group that has a candidate reserves its slots (per tile
//                it was 1.3 M adds to one address on a 5-GB layer of small
//                files, and the kernel ran at the atomic's rate); the
//                candidates are then read again, two a step, and the 32
//                lanes of a half store their 16 B each into the record, lane
//                0 the block index before them, only below the capacity.
//                No LDS, no waiting on other waves or workgroups.
#include "tarindex.h"

#include <hip/hip_runtime.h>

#include <algorithm>

#include "tarindex_dev.h"  // group_mask, shared with tarforest.hip

namespace tsg {
namespace {

constexpr int kTThreads = 256;
// Memory-bound streaming kernel: at most 256 CUs x 8 workgroups, the rest by the grid stride.
constexpr uint64_t kMaxGrid = 2048;

__global__ __launch_bounds__(kTThreads) void tar_headers_kernel(const uint8_t* __restrict__ tar, uint64_t n_blocks,
                                                                uint8_t* __restrict__ records, uint32_t capacity,
                                                                uint32_t* __restrict__ count) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t l = lane & 31u, half = lane >> 5;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t n_groups = (n_blocks + kGroupBlocks - 1) / kGroupBlocks;
  for (uint64_t g = uint64_t(blockIdx.x) * 4u + wave; g < n_groups; g += uint64_t(gridDim.x) * 4u) {
    const uint64_t g0 = g * kGroupBlocks;
    uint64_t mask = group_mask(tar, n_blocks, g0, l, half);
    if (mask == 0) continue;  // (wave-uniform)
    // One reservation for the group's candidates: every wave adds to the one counter, and a layer of
    // small files has a candidate in most tiles.  The candidates' bytes are then read again (they
    // were just read: cache hits), two blocks a step, one per half.
    uint32_t slot = 0;
    if (lane == 0) slot = atomicAdd(count, uint32_t(__builtin_popcountll(mask)));
    slot = __builtin_amdgcn_readfirstlane(slot);
    while (mask) {
      const uint32_t i0 = uint32_t(__builtin_ctzll(mask));
      mask &= mask - 1;
      const bool two = mask != 0;
      const uint32_t i1 = two ? uint32_t(__builtin_ctzll(mask)) : i0;
      if (two) mask &= mask - 1;
      const uint32_t my_slot = slot + half;
      if ((half == 0 || two) && my_slot < capacity) {
        const uint64_t blk = g0 + (half ? i1 : i0);  // (a candidate: below n_blocks)
        const uint4 d = *reinterpret_cast<const uint4*>(tar + blk * 512u + l * 16u);
        uint8_t* rec = records + uint64_t(my_slot) * kTarRecordBytes;
        if (l == 0) *reinterpret_cast<uint4*>(rec) = make_uint4(uint32_t(blk), uint32_t(blk >> 32), 0u, 0u);
        *reinterpret_cast<uint4*>(rec + 16u + l * 16u) = d;
      }
      slot += two ? 2u : 1u;
    }
  }
}

// tar_bitmap : the same pass with the verdict stored as it is, one 64-bit word per group of 64 blocks
//              (bit i of word g: block 64 g + i), lane 0's vector store: no atomics, no capacity, no
//              second run.  Every word of the groups below n_blocks is written; the bits of blocks at or
//              past n_blocks are 0.
__global__ __launch_bounds__(kTThreads) void tar_bitmap_kernel(const uint8_t* __restrict__ tar, uint64_t n_blocks,
                                                               uint64_t* __restrict__ bitmap) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t l = lane & 31u, half = lane >> 5;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t n_groups = (n_blocks + kGroupBlocks - 1) / kGroupBlocks;
  for (uint64_t g = uint64_t(blockIdx.x) * 4u + wave; g < n_groups; g += uint64_t(gridDim.x) * 4u) {
    const uint64_t mask = group_mask(tar, n_blocks, g * kGroupBlocks, l, half);
    if (lane == 0) bitmap[g] = mask;
  }
}

}  // namespace

hipError_t TarHeaders(const uint8_t* dev_tar, uint64_t n_bytes, uint8_t* d_records, uint32_t capacity,
                      uint32_t* d_count, uint32_t grid_cap, hipStream_t s) {
  const uint64_t n_blocks = n_bytes / 512;
  if (n_blocks == 0) return hipSuccess;
  // the grid depends on n_bytes alone: a wave per group of tiles, four per workgroup
  const uint64_t n_groups = (n_blocks + kGroupBlocks - 1) / kGroupBlocks;
  uint64_t grid = std::min((n_groups + 3) / 4, kMaxGrid);
  if (grid_cap) grid = std::min<uint64_t>(grid, grid_cap);
  tar_headers_kernel<<<uint32_t(grid), kTThreads, 0, s>>>(dev_tar, n_blocks, d_records, capacity, d_count);
  return hipGetLastError();
}

hipError_t TarBitmap(const uint8_t* dev_tar, uint64_t n_bytes, uint64_t* d_bitmap, uint32_t grid_cap, hipStream_t s) {
  const uint64_t n_blocks = n_bytes / 512;
  if (n_blocks == 0) return hipSuccess;
  const uint64_t n_groups = (n_blocks + kGroupBlocks - 1) / kGroupBlocks;
  uint64_t grid = std::min((n_groups + 3) / 4, kMaxGrid);
  if (grid_cap) grid = std::min<uint64_t>(grid, grid_cap);
  tar_bitmap_kernel<<<uint32_t(grid), kTThreads, 0, s>>>(dev_tar, n_blocks, d_bitmap);
  return hipGetLastError();
}

}  // namespace tsg
