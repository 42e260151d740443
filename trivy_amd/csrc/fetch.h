// Fetch of a device-only batch's candidate files (fetch.hip): the files that
// got candidates are marked on the GPU, laid out back to back (each rounded up
// to 16 B) and packed from the arena into a bounded staging buffer, window by
// window, for the copy to pinned host memory.  Everything is stream-ordered
// behind the scan's finalize kernel: the host learns the candidate count only
// when it collects the scan, so no launch parameter depends on it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "engine.h"

namespace tsg {

// Packed bytes per work item of fetch_files_kernel (a wave copies one item, the
// part of one file inside one kFetchSeg block of the packed layout): the piece
// size of the host-memory gather (xform.h kGatherPiece), which split files for
// the same reason -- a multi-MiB file must not be one wave's work.
constexpr uint32_t kFetchSeg = 16384;
static_assert(kFetchSeg % 16 == 0, "a window edge is a 16-B block edge");

// What the plan found (device; copy it back with the stream's other results).
struct FetchCounters {
  uint64_t packed_bytes;  // the packed layout's size: sum of the packed files' lengths, each rounded up to 16
  uint64_t n_packed;      // files in the packed layout
  uint64_t n_direct;      // marked files of direct_bytes or more (not packed: copied where they lie)
  uint64_t n_files;       // marked files
  uint64_t file_bytes;    // their lengths, summed
  uint64_t pad_[3];
};
static_assert(sizeof(FetchCounters) == 64, "copied back as one 64-B record");

// Device scratch of a plan over n_files files (flags, lengths, offsets, list, scan temp).
size_t FetchScratchBytes(uint32_t n_files);
// The per-file flags of the scratch (n_files u32): FetchPlan's input when no
// candidate list is given -- the caller fills them (nonzero: fetch the file).
uint32_t* FetchFlags(void* scratch, uint32_t n_files);
// What FetchPlan left in the scratch for FetchPack (device addresses; tests read
// them back): the packed files' ids in file order (ctr->n_packed entries) and
// their packed offsets (n_packed + 1: the last is packed_bytes).
const uint32_t* FetchList(const void* scratch, uint32_t n_files);
const uint64_t* FetchListOffsets(const void* scratch, uint32_t n_files);

// Marks the files of the candidates cands[0 .. min(*cand_count, cand_cap)) that
// the host will see (not kCandDrop) -- or, with cands == nullptr, takes the
// flags as the caller wrote them -- then lays the marked files below
// direct_bytes out in file order, each rounded up to 16 B, and writes *ctr.
hipError_t FetchPlan(const Candidate* cands, const uint32_t* cand_count, uint32_t cand_cap, const uint64_t* off,
                     uint32_t n_files, uint64_t direct_bytes, void* scratch, FetchCounters* ctr, hipStream_t s);

// stage[0 .. w1 - w0) = bytes [w0, w1) of the packed layout (w0 a multiple of
// kFetchSeg, w1 of 16); the padding after a file is left as it was.  Nothing is
// written past min(w1, packed_bytes) - w0.  Arena reads stay inside the files
// copied: [off[f], off[f + 1]).
hipError_t FetchPack(const uint8_t* arena, const uint64_t* off, uint32_t n_files, const void* scratch,
                     const FetchCounters* ctr, uint64_t w0, uint64_t w1, uint8_t* stage, hipStream_t s);

}  // namespace tsg
