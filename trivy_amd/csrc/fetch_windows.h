// The windows fetch of a device-only batch, device side (fetch_windows.hip;
// the layout: fetch_layout.h): the candidates mark 256-B granules of the arena
// in a bitmap, the bitmap's words are ranked by an exclusive sum of their
// popcounts, and the marked granules are packed, in arena order, into a
// bounded staging buffer, window by window.  Everything is stream-ordered
// behind the scan's finalize kernel and no launch parameter depends on the
// candidate count (the host learns it only when it collects the scan).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "engine.h"
#include "fetch_layout.h"

namespace tsg {

// What the marking found (device; copied back with the scan's other counters).
struct FetchWinCounters {
  uint64_t granules;     // marked granules: the packed layout is granules * 256 bytes
  uint64_t runs;         // maximal runs of consecutive marked granules
  uint64_t whole_files;  // files a candidate marked whole
  uint64_t pad_[5];
};
static_assert(sizeof(FetchWinCounters) == 64, "copied back as one 64-B record");

// Device scratch of a plan over an arena of n_bytes with n_files files (the
// bitmap, the word popcounts and ranks, the per-file whole flags, scan temp).
size_t FetchWinScratchBytes(uint64_t n_bytes, uint32_t n_files);

// Marks the granules of cands[0 .. min(*cand_count, cand_cap)) that the host
// will see (not kCandDrop), ranks them and writes *ctr.  rule_max_len: one
// u32 per rule (RuleGpu::max_len, kNoMaxLen: unbounded), n_rules of them.  The
// bitmap is cleared here by a hipMemsetAsync of n_bytes / 2048 bytes, not by
// the pack that consumed it: a pack covers only the windows the host asked
// for, and a scan that is rerun or abandoned between rounds would leave bits
// behind for the next one; the memset is 2 MiB for a 4-GiB arena.
hipError_t FetchWinPlan(const Candidate* cands, const uint32_t* cand_count, uint32_t cand_cap, const uint64_t* off,
                        uint32_t n_files, uint64_t n_bytes, const uint32_t* rule_max_len, uint32_t n_rules,
                        const FetchWinParams& prm, void* scratch, FetchWinCounters* ctr, hipStream_t s);

// stage[0 .. w1 - w0) = bytes [w0, w1) of the packed layout (both multiples of
// 256).  Nothing is written past min(w1, granules * 256) - w0.  Arena reads
// are aligned 16-B blocks that begin below n_bytes: none leaves the arena's
// readable extent [arena, arena + n_bytes + 64); the blocks of the last
// granule at or past n_bytes are not read and their staging bytes stay as
// they were.
hipError_t FetchWinPack(const uint8_t* arena, uint64_t n_bytes, const void* scratch, uint32_t n_files,
                        const FetchWinCounters* ctr, uint64_t w0, uint64_t w1, uint8_t* stage, hipStream_t s);

}  // namespace tsg
