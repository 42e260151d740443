// utils.IsBinary (pkg/fanal/utils/utils.go:85-103) over the heads of the files
// of an HBM-resident arena: the analyzer's binary gate (secret.go:108-117) for
// bytes the host holds no copy of.
//
// A file belongs to half a wave: the head is at most 300 bytes, so the aligned
// 16-B blocks that intersect it are at most 20 (a head starting at byte 15 of
// its first block ends in block 19), and lane j of the 32 reads block j.  The
// arena is 16-B aligned with 64 readable bytes past its end, so each of those
// blocks is readable whole; a lane whose block lies past the head reads the
// file's first block instead and is masked out.  The bytes of the first and
// the last block outside [start, start + head) are masked too: a neighbour's
// bytes and the pad never reach a flag.  One ballot reduces the two files of a
// wave.  Traffic: at most 320 B per file, plus its two offsets.
#include "classify.h"

#include <algorithm>

namespace tsg {
namespace {

constexpr int kCThreads = 256;
constexpr uint32_t kCFilesPerBlock = kCThreads / 32;

// Bit i (i < 4): byte i of w is one IsBinary rejects -- 0x7F, or below 0x20
// and set in the table (every control byte but BEL, BS, TAB, LF, FF, CR, ESC).
__device__ __forceinline__ uint32_t bad_bytes(uint32_t w) {
  uint32_t m = 0;
#pragma unroll
  for (uint32_t i = 0; i < 4; i++) {
    const uint32_t b = (w >> (8 * i)) & 0xFFu;
    const uint32_t ctl = (0xF7FFC87Fu >> (b & 31u)) & uint32_t(b < 0x20u);
    m |= (ctl | uint32_t(b == 0x7Fu)) << i;
  }
  return m;
}

__global__ __launch_bounds__(kCThreads) void classify_heads_kernel(const uint8_t* __restrict__ arena,
                                                                   const uint64_t* __restrict__ off,
                                                                   uint32_t n_files, uint8_t* __restrict__ flags) {
  const uint32_t lane = threadIdx.x & 63u, sub = lane & 31u, half = lane >> 5;
  const uint32_t group = threadIdx.x >> 5;  // the file of the workgroup's 8 this lane works on
  // every lane of a wave runs the same number of rounds (the ballot below needs them all)
  for (uint64_t base = uint64_t(blockIdx.x) * kCFilesPerBlock; base < n_files;
       base += uint64_t(gridDim.x) * kCFilesPerBlock) {
    const uint64_t fi = base + group;
    const bool live = fi < n_files;
    const uint32_t f = live ? uint32_t(fi) : n_files - 1;  // (a spare half wave rereads the last file)
    const uint64_t s = off[f], len = off[f + 1] - s;
    const uint64_t e = s + (len < kBinaryHead ? len : uint64_t(kBinaryHead));  // the head is [s, e)
    const uint64_t b0 = s & ~uint64_t(15);
    const uint64_t blk = b0 + 16u * sub;
    const bool in = blk < e;  // the block holds a byte of the head (never for an empty file)
    const uint4 v = *reinterpret_cast<const uint4*>(arena + (in ? blk : b0));
    const uint32_t bad = bad_bytes(v.x) | (bad_bytes(v.y) << 4) | (bad_bytes(v.z) << 8) | (bad_bytes(v.w) << 12);
    // the block's bytes inside the head: bits [lo, hi)
    const uint32_t lo = s > blk ? uint32_t(s - blk) : 0u;
    const uint32_t hi = (in && e < blk + 16) ? uint32_t(e - blk) : 16u;
    const uint32_t keep = in ? (((1u << hi) - 1u) & ~((1u << lo) - 1u)) : 0u;
    const uint64_t any = __ballot((bad & keep) != 0u);
    if (sub == 0 && live) flags[f] = uint8_t(uint32_t(any >> (32u * half)) != 0u);
  }
}

}  // namespace

hipError_t ClassifyHeads(const uint8_t* arena, const uint64_t* off, uint32_t n_files, uint8_t* flags, hipStream_t s) {
  if (n_files == 0) return hipSuccess;
  const uint32_t grid = std::min<uint32_t>((n_files + kCFilesPerBlock - 1) / kCFilesPerBlock, 4096);
  classify_heads_kernel<<<grid, kCThreads, 0, s>>>(arena, off, n_files, flags);
  return hipGetLastError();
}

}  // namespace tsg
