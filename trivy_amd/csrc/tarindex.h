// The tar index of a layer resident in HBM (tarindex.hip): one streaming pass
// over the layer's complete 512-B blocks that appends every block which parses
// as a tar header -- analyzer.cpp's ChecksumOK(block) && !AllZero(block) -- to a
// record buffer.  The chain walk over those records stays on the host
// (tar_index_host.h).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace tsg {

// A header candidate as the kernel writes it (tar_index_host.h's TarRecord).
constexpr uint64_t kTarRecordBytes = 528;  // u64 block index, 8 B of zero padding, the 512 header bytes

// Blocks b < n_bytes / 512 of dev_tar (16-B aligned) are read, nothing else.
// *d_count (zeroed by the caller, on the stream) receives the number of
// candidates, which may exceed `capacity`; records [0, min(count, capacity)) of
// d_records (16-B aligned) are written, in no particular order, and nothing
// past the capacity.  grid_cap != 0 caps the grid (tests: one workgroup strides
// over everything); otherwise the grid is a function of n_bytes alone.
hipError_t TarHeaders(const uint8_t* dev_tar, uint64_t n_bytes, uint8_t* d_records, uint32_t capacity,
                      uint32_t* d_count, uint32_t grid_cap, hipStream_t s);

}  // namespace tsg
