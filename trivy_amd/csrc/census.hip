// Resident batches with a transform: the census of the files the transform
// changes, and the gather of chosen files from the resident arena (census.h).
//
//  census_kinds     : a thread per file: mark[f] = kind 2 or 3.  It writes every
//                     mark, so the buffer needs no memset.
//  transform_census : a wave per 4-KiB tile of the arena, grid-stride; each lane
//                     holds four aligned 16-B loads (1 KiB apart, so every wave
//                     instruction reads 1 KiB contiguously) and turns them into
//                     four 16-bit masks of the positions that hold 0x0D, exact per
//                     byte, the bytes at or past n_bytes masked out.  A tile
//                     without a hit ends there (one ballot).  Otherwise the wave
//                     finds the file of the tile's first hit by one binary search
//                     of the offsets and walks forward to the file of its last
//                     hit; the walk is wave-uniform.  A kind-1 file not yet
//                     marked tests the masks against its byte range and stores
//                     a 1 (plain byte stores; racing stores of the same value).
//                     A CRLF file is marked by the first of its tiles to get
//                     there; its other tiles read the mark and move on.
//  gather_device    : a wave per (file, piece) item; see census.h.
#include "census.h"

#include <algorithm>

namespace tsg {
namespace {

constexpr int kCThreads = 256;
constexpr uint32_t kCensusTile = 4096;
// Memory-bound streaming kernels: at most 256 CUs x 8 workgroups, the rest by the grid stride.
constexpr uint64_t kMaxGrid = 2048;

__global__ __launch_bounds__(kCThreads) void census_kinds_kernel(const uint8_t* __restrict__ kind, uint32_t n_files,
                                                                 uint8_t* __restrict__ mark) {
  for (uint32_t f = blockIdx.x * kCThreads + threadIdx.x; f < n_files; f += gridDim.x * kCThreads) {
    const uint8_t k = kind[f];
    mark[f] = (k == kXformPrintable || k == kXformDrop) ? 1 : 0;
  }
}

// Bit i = byte i of w is 0x0D.  The zero-byte test keeps every byte to itself
// (no borrow crosses a byte, unlike (x - 0x01010101) & ~x & 0x80808080).
__device__ __forceinline__ uint32_t cr_bits(uint32_t w) {
  const uint32_t x = w ^ 0x0D0D0D0Du;
  const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
  return (((z >> 7) * 0x00204081u) >> 21) & 0xFu;  // bits 0, 8, 16, 24 -> 0 .. 3
}

__global__ __launch_bounds__(kCThreads) void transform_census_kernel(const uint8_t* __restrict__ arena,
                                                                     uint64_t n_bytes,
                                                                     const uint64_t* __restrict__ off,
                                                                     const uint8_t* __restrict__ kind,
                                                                     uint32_t n_files, uint8_t* mark) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t n_tiles = (n_bytes + kCensusTile - 1) / kCensusTile;
  for (uint64_t t = uint64_t(blockIdx.x) * 4u + wave; t < n_tiles; t += uint64_t(gridDim.x) * 4u) {
    const uint64_t base = t * kCensusTile;
    uint4 v[4];
#pragma unroll
    for (uint32_t u = 0; u < 4; u++) {
      const uint64_t p = base + u * 1024u + lane * 16u;
      v[u] = make_uint4(0, 0, 0, 0);
      if (p < n_bytes) v[u] = *reinterpret_cast<const uint4*>(arena + p);  // (ends before n_bytes + 16)
    }
    uint32_t m[4];
#pragma unroll
    for (uint32_t u = 0; u < 4; u++) {
      const uint64_t p = base + u * 1024u + lane * 16u;
      uint32_t b = cr_bits(v[u].x) | (cr_bits(v[u].y) << 4) | (cr_bits(v[u].z) << 8) | (cr_bits(v[u].w) << 12);
      if (p < n_bytes && n_bytes - p < 16) b &= (1u << uint32_t(n_bytes - p)) - 1u;  // the bytes past n_bytes
      m[u] = b;
    }
    if (__ballot((m[0] | m[1] | m[2] | m[3]) != 0) == 0) continue;
    // the tile's first and last hit (tile-relative positions; wave-uniform)
    uint32_t first = 0, last = 0;
#pragma unroll
    for (int u = 3; u >= 0; u--) {
      const unsigned long long b = __ballot(m[u] != 0);
      if (b) {
        const uint32_t l = uint32_t(__builtin_ctzll(b));
        first = uint32_t(u) * 1024u + l * 16u + uint32_t(__builtin_ctz(__builtin_amdgcn_readlane(m[u], l)));
      }
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const unsigned long long b = __ballot(m[u] != 0);
      if (b) {
        const uint32_t l = 63u - uint32_t(__builtin_clzll(b));
        last = uint32_t(u) * 1024u + l * 16u + 31u - uint32_t(__builtin_clz(__builtin_amdgcn_readlane(m[u], l)));
      }
    }
    const uint64_t p_first = base + first, p_last = base + last;  // (both below n_bytes)
    // the file of the first hit: the last f with off[f] <= p_first (off[0] = 0;
    // of files that start at one offset the last one owns the byte there)
    uint32_t lo = 0, hi = n_files;
    while (hi - lo > 1) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (off[mid] <= p_first) lo = mid;
      else hi = mid;
    }
    for (uint32_t f = lo; f < n_files; f++) {
      const uint64_t fs = off[f];
      if (fs > p_last) break;
      const uint64_t fe = off[f + 1];
      if (fe <= fs || kind[f] != kXformStripCR || mark[f]) continue;
      uint32_t hit = 0;
#pragma unroll
      for (uint32_t u = 0; u < 4; u++) {
        const uint64_t blk = base + u * 1024u + lane * 16u;
        const uint64_t a = max(fs, blk), z = min(fe, blk + 16);
        if (a < z) {  // bits [a - blk, z - blk) of the block's mask
          const uint32_t below_z = (1u << uint32_t(z - blk)) - 1u, below_a = (1u << uint32_t(a - blk)) - 1u;
          hit |= m[u] & below_z & ~below_a;
        }
      }
      if (__ballot(hit != 0) != 0 && lane == 0) mark[f] = 1;
    }
  }
}

__device__ __forceinline__ uint4 shift_bytes(const uint4& A, const uint4& B, uint32_t q, uint32_t r) {
  // bytes [4q + r, 4q + r + 16) of A:B  (q, r wave-uniform)
  const uint32_t w[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
  uint32_t v[4];
  switch (q) {
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
  return make_uint4(v[0], v[1], v[2], v[3]);
}

__global__ __launch_bounds__(kCThreads) void gather_device_kernel(const uint8_t* __restrict__ src,
                                                                  const uint64_t* __restrict__ src_off,
                                                                  const uint64_t* __restrict__ dst_off,
                                                                  const GatherItem* __restrict__ items,
                                                                  uint32_t n_items, uint8_t* __restrict__ dst) {
  // The source is HBM: a lane loads both aligned blocks its destination block
  // takes bytes from (the second is the next lane's first, a hit in the L1), so
  // no lane waits for another's load; kU blocks a lane, 2 kU loads in flight.
  constexpr uint32_t kU = 4;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (uint32_t it = blockIdx.x * 4u + wave; it < n_items; it += gridDim.x * 4u) {
    const GatherItem g = items[it];
    const uint64_t f0 = dst_off[g.file], f1 = dst_off[g.file + 1];
    const uint64_t d0 = f0 + uint64_t(g.piece) * kGatherPiece;
    const uint64_t d1 = min(f1, d0 + kGatherPiece);
    if (d0 >= d1) continue;
    // the item's source bytes [s0, s1); destination byte x comes from x + delta.
    // A destination block below d0 has its source below s0, below 0 for a file at
    // the arena's start: signed, and only blocks that meet [s0, s1) are loaded.
    const int64_t s0 = int64_t(src_off[g.file] + (d0 - f0)), s1 = s0 + int64_t(d1 - d0);
    const int64_t delta = s0 - int64_t(d0);
    const uint64_t b_lo = d0 & ~uint64_t(15);
    const uint32_t r = uint32_t((int64_t(b_lo) + delta) & 15);  // byte shift, the same for every block
    for (uint64_t k = 0; b_lo + 16 * k < d1; k += 64 * kU) {
      uint4 A[kU], B[kU];
#pragma unroll
      for (uint32_t u = 0; u < kU; u++) {
        const uint64_t blk = b_lo + 16 * (k + 64 * u + lane);
        const int64_t sa = (int64_t(blk) + delta) & ~int64_t(15);
        A[u] = make_uint4(0, 0, 0, 0);
        B[u] = make_uint4(0, 0, 0, 0);
        if (blk < d1) {
          if (sa + 16 > s0 && sa < s1) A[u] = *reinterpret_cast<const uint4*>(src + sa);
          if (r && sa + 32 > s0 && sa + 16 < s1) B[u] = *reinterpret_cast<const uint4*>(src + sa + 16);
        }
      }
#pragma unroll
      for (uint32_t u = 0; u < kU; u++) {
        const uint64_t blk = b_lo + 16 * (k + 64 * u + lane);
        if (blk >= d1) continue;
        const uint4 o = r ? shift_bytes(A[u], B[u], r >> 2, r & 3u) : A[u];
        if (blk >= d0 && blk + 16 <= d1) {
          *reinterpret_cast<uint4*>(dst + blk) = o;
        } else {  // a ragged end: only the item's bytes (the neighbours belong to other files / items)
          const uint32_t ow[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
          for (uint32_t jb = 0; jb < 16; jb++) {
            const uint64_t x = blk + jb;
            if (x >= d0 && x < d1) dst[x] = uint8_t(ow[jb >> 2] >> (8 * (jb & 3)));
          }
        }
      }
    }
  }
}

}  // namespace

hipError_t TransformCensus(const uint8_t* arena, uint64_t n_bytes, const uint64_t* d_off, const uint8_t* d_kind,
                           uint32_t n_files, uint8_t* d_mark, hipStream_t s) {
  if (n_files == 0) return hipSuccess;
  const uint64_t gk = (uint64_t(n_files) + kCThreads - 1) / kCThreads;
  census_kinds_kernel<<<uint32_t(std::min(gk, kMaxGrid)), kCThreads, 0, s>>>(d_kind, n_files, d_mark);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || n_bytes == 0) return e;
  // the grid depends on n_bytes alone: a wave per tile, four per workgroup
  const uint64_t n_tiles = (n_bytes + kCensusTile - 1) / kCensusTile;
  const uint64_t grid = std::min((n_tiles + 3) / 4, kMaxGrid);
  transform_census_kernel<<<uint32_t(grid), kCThreads, 0, s>>>(arena, n_bytes, d_off, d_kind, n_files, d_mark);
  return hipGetLastError();
}

hipError_t GatherDeviceFiles(const uint8_t* arena, const uint64_t* src_off, const uint64_t* dst_off,
                             const GatherItem* items, uint32_t n_items, uint8_t* dst, hipStream_t s) {
  if (!n_items) return hipSuccess;
  // HBM to HBM, memory-bound: a wave per item, four per workgroup, up to 256 CUs
  // x 8 workgroups (each lane keeps 8 16-B loads in flight, 8 KiB a wave); more
  // items than that go round the grid stride.  gather_host_kernel's 32
  // workgroups are sized for the host link and would leave most CUs idle here.
  const uint64_t grid = std::min((uint64_t(n_items) + 3) / 4, kMaxGrid);
  gather_device_kernel<<<uint32_t(grid), kCThreads, 0, s>>>(arena, src_off, dst_off, items, n_items, dst);
  return hipGetLastError();
}

}  // namespace tsg
