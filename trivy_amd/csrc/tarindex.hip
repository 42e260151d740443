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

namespace tsg {
namespace {

constexpr int kTThreads = 256;
constexpr uint32_t kTileBlocks = 8;  // 4 loads x 2 blocks
constexpr uint32_t kGroupTiles = 8;  // tiles a wave tests before it reserves their candidates' slots
constexpr uint32_t kGroupBlocks = kGroupTiles * kTileBlocks;  // 64: one bit each
// Memory-bound streaming kernel: at most 256 CUs x 8 workgroups, the rest by the grid stride.
constexpr uint64_t kMaxGrid = 2048;
constexpr int32_t kNoWant = INT32_MIN;  // the field does not parse, or no sum can equal it

__device__ __forceinline__ uint32_t field_byte(uint64_t f, uint32_t i) { return uint32_t(f >> (8u * i)) & 0xFFu; }

// ParseNumeric over the 8-byte checksum field (bytes 148..155 = f's bytes 0..7).
__device__ int32_t parse_field(uint64_t f) {
  if (f & 0x80u) {  // base-256, two's complement, big-endian; 8 bytes never overflow
    const bool neg = (f & 0x40u) != 0;
    uint64_t v = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; i++) {
      uint32_t c = field_byte(f, i);
      if (i == 0) c &= 0x7Fu;
      if (neg) c ^= 0xFFu;
      if (i == 0 && neg) c &= 0x7Fu;
      v = (v << 8) | c;
    }
    const int64_t w = neg ? -int64_t(v) - 1 : int64_t(v);
    return (w > -(int64_t(1) << 24) && w < (int64_t(1) << 24)) ? int32_t(w) : kNoWant;  // (the sums are far inside)
  }
  uint32_t lo = 0, hi = 8;
  while (lo < hi && (field_byte(f, lo) == ' ' || field_byte(f, lo) == 0)) lo++;
  while (hi > lo && (field_byte(f, hi - 1) == ' ' || field_byte(f, hi - 1) == 0)) hi--;
  int32_t v = 0;
  for (uint32_t i = lo; i < hi; i++) {
    const uint32_t c = field_byte(f, i);
    if (c < '0' || c > '7') return kNoWant;
    v = v * 8 + int32_t(c - '0');  // (at most 8 digits: below 2^24)
  }
  return v;
}

__device__ __forceinline__ uint32_t high_bytes(uint32_t w) { return uint32_t(__builtin_popcount(w & 0x80808080u)); }

template <int kCtrl>
__device__ __forceinline__ uint32_t row_ror_add(uint32_t p) {  // p + (p rotated within its row of 16 lanes)
  return p + uint32_t(__builtin_amdgcn_update_dpp(0, int(p), kCtrl, 0xF, 0xF, false));
}

// The verdict on the 64 blocks from g0 on, one bit each (bit i: block g0 + i is a candidate), wave-uniform:
// what tar_headers_kernel turns into records and tar_bitmap_kernel stores as it is.
__device__ __forceinline__ uint64_t group_mask(const uint8_t* __restrict__ tar, uint64_t n_blocks, uint64_t g0,
                                               uint32_t l, uint32_t half) {
  uint64_t mask = 0;  // bit i: block g0 + i is a candidate (wave-uniform)
  for (uint32_t k = 0; k < kGroupTiles; k++) {
    const uint64_t b0 = g0 + k * kTileBlocks;
    if (b0 >= n_blocks) break;  // (wave-uniform)
    uint4 v[4];
#pragma unroll
    for (uint32_t u = 0; u < 4; u++) {
      // no branch around a load (it would wait for each before the next is issued): a block past the
      // end reads the last block instead (n_blocks >= 1 here) and is no candidate, whatever it holds
      const uint64_t blk = min(b0 + 2u * u + half, n_blocks - 1);
      v[u] = *reinterpret_cast<const uint4*>(tar + blk * 512u + l * 16u);  // (ends at or before 512 n_blocks)
    }
#pragma unroll
    for (uint32_t u = 0; u < 4; u++) {
      uint32_t su = __builtin_amdgcn_sad_u8(v[u].x, 0u, __builtin_amdgcn_sad_u8(v[u].w, 0u, 0u));
      uint32_t hb = high_bytes(v[u].x) + high_bytes(v[u].w);
      int32_t want = kNoWant;
      if (l == 9) {  // bytes 148..155 are this lane's y and z: eight spaces in the sums
        su += 8u * 0x20u;
        want = parse_field(uint64_t(v[u].y) | (uint64_t(v[u].z) << 32));
      } else {
        su = __builtin_amdgcn_sad_u8(v[u].y, 0u, __builtin_amdgcn_sad_u8(v[u].z, 0u, su));
        hb += high_bytes(v[u].y) + high_bytes(v[u].z);
      }
      uint32_t p = su | (hb << 20);  // su <= 512 x 255 < 2^17, hb <= 512: no carry between them
      p = row_ror_add<0x128>(p);
      p = row_ror_add<0x124>(p);
      p = row_ror_add<0x122>(p);
      p = row_ror_add<0x121>(p);
#pragma unroll
      for (uint32_t h = 0; h < 2; h++) {
        const uint32_t s = uint32_t(__builtin_amdgcn_readlane(int(p), int(32 * h))) +
                           uint32_t(__builtin_amdgcn_readlane(int(p), int(32 * h + 16)));
        const int32_t w = __builtin_amdgcn_readlane(want, int(32 * h + 9));
        const int32_t uns = int32_t(s & 0xFFFFFu), sgn = uns - 256 * int32_t(s >> 20);
        const bool cand = w != kNoWant && (w == uns || w == sgn) && b0 + 2u * u + h < n_blocks;
        if (cand) mask |= uint64_t(1) << (k * kTileBlocks + 2u * u + h);
      }
    }
  }
  return mask;
}

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
