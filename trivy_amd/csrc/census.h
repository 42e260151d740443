// Resident batches with a transform (census.hip): which files the transform
// really changes, found on the GPU before the scan, and the gather of chosen
// files from the resident arena into a packed buffer.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "xform.h"

namespace tsg {

// mark[f] = 1 when the transform of kind[f] does not leave file f as it is read:
// kind 2 (printable extraction) and kind 3 (dropped) always, kind 1 (CR strip)
// when the file holds a byte 0x0D; 0 otherwise (kind 0, a CR-free kind 1).  The
// marks are exact: a 0x0D of a neighbouring file or of the bytes past n_bytes
// marks nothing.  Every mark[0 .. n_files) is written by the call (no memset
// needed before it).  arena: 16-B aligned with 64 readable bytes past n_bytes;
// no read leaves [arena, arena + n_bytes + 64).  d_off: n_files + 1 ascending
// offsets from 0 to n_bytes.  One streaming pass over the arena.
hipError_t TransformCensus(const uint8_t* arena, uint64_t n_bytes, const uint64_t* d_off, const uint8_t* d_kind,
                           uint32_t n_files, uint8_t* d_mark, hipStream_t s);

// Gather of files that lie scattered in a resident arena into a packed buffer:
// dst[dst_off[f] .. dst_off[f + 1]) = arena[src_off[f] ..) for the files of the
// items (the item scheme of GatherHostFiles: (file, piece), a wave per item of
// up to kGatherPiece bytes).  dst is 16-B aligned; 16-B stores where a block
// lies inside the item, byte stores at its ragged ends, so no byte outside
// [dst_off[f], dst_off[f + 1]) is written.  The source by aligned 16-B loads and
// a byte shift; only aligned blocks that hold a byte of the file are loaded, so
// no read leaves [arena, arena + n_bytes + 64) wherever the file lies (a file
// at source offset < 16 with an unaligned destination included), given
// src_off[f] + its length <= n_bytes.
hipError_t GatherDeviceFiles(const uint8_t* arena, const uint64_t* src_off, const uint64_t* dst_off,
                             const GatherItem* items, uint32_t n_items, uint8_t* dst, hipStream_t s);

}  // namespace tsg
