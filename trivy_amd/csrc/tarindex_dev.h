// The header-candidate verdict on a group of 64 blocks of a tar layer, one wave
// per group: shared by tarindex.hip's kernels and the forest pass over all layers
// of an image (tarforest.hip).  Device code; how the verdict is reached is told
// at the top of tarindex.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace tsg {
namespace {

constexpr uint32_t kTileBlocks = 8;  // 4 loads x 2 blocks
constexpr uint32_t kGroupTiles = 8;  // tiles a wave tests before it reserves their candidates' slots
constexpr uint32_t kGroupBlocks = kGroupTiles * kTileBlocks;  // 64: one bit each
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

}  // namespace
}  // namespace tsg
