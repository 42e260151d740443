// The analyzer's binary gate on HBM-resident files (classify.hip):
// utils.IsBinary (pkg/fanal/utils/utils.go:85-103) over each file's head, on
// the bytes as read, for callers that hold no host copy of them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace tsg {

constexpr uint32_t kBinaryHead = 300;  // IsBinary reads min(size, 300) bytes

// flags[f] = 1 when IsBinary is true on file f's head [off[f], off[f] +
// min(len, kBinaryHead)), else 0 (an empty file: 0).  arena follows the
// tsg_batch.dev_arena contract (16-B aligned, 64 readable bytes past
// off[n_files]); off (n_files + 1, ascending) and flags (n_files) are device
// memory.  Reads the aligned 16-B blocks that intersect a head, nothing else.
hipError_t ClassifyHeads(const uint8_t* arena, const uint64_t* off, uint32_t n_files, uint8_t* flags, hipStream_t s);

}  // namespace tsg
