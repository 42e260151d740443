// The tar index of a layer resident in HBM (tarindex.hip): one streaming pass
// over the layer's complete 512-B blocks that appends every block which parses
// as a tar header -- analyzer.cpp's ChecksumOK(block) && !AllZero(block) -- to a
// record buffer.  The chain walk over those records stays on the host
// (tar_index_host.h) -- or, in the analyzer's walk mode 1, the same verdict is
// kept as one bit per block and the chain is walked on the GPU too
// (tarchain.hip; declared below).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "tarchain.h"
#include "tarforest.h"
#include "tarrequired.h"

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

// The same verdict as one bit per block: word g of d_bitmap (8-B aligned,
// (n_bytes / 512 + 63) / 64 words, all written) holds blocks 64 g .. 64 g + 63,
// bit i block 64 g + i.  No counter, no capacity.
hipError_t TarBitmap(const uint8_t* dev_tar, uint64_t n_bytes, uint64_t* d_bitmap, uint32_t grid_cap, hipStream_t s);

// ---- the chain walk on the GPU (tarchain.hip; the contract: tarchain.h) ----
// What the pass leaves at the start of its work buffer for the host to copy.
struct TarChainHead {
  tsg_tar_stop stop;
  uint64_t entries, name_bytes;  // on the chain, up to the stop
  uint64_t candidates;
  uint64_t pad;
};
static_assert(sizeof(TarChainHead) == 64, "");

// The one device buffer of a pass over n_blocks blocks in segments of `segment`
// blocks: byte offsets of its parts (256-B aligned) and its size.
struct TarChainLayout {
  uint64_t n_blocks = 0, n_segments = 0;
  uint32_t segment = 0;
  uint64_t head = 0, cand = 0, chain = 0, seg_entry = 0, succ = 0, nlen = 0, rank = 0, noff = 0, temp = 0;
  uint64_t temp_bytes = 0, bytes = 0;
};
// segment_blocks: 0 = kTarDefaultSegment, else a power of two >= kTarMinSegment whose
// words fit a workgroup's LDS; false: it is neither.  n_bytes / 512 < kTarMaxBlocks - 2.
bool TarChainPlan(uint64_t n_bytes, uint32_t segment_blocks, TarChainLayout* L);

// Stage times are taken between these events, recorded on s when ev != NULL:
// ev[0] start, [1] after the bitmap, [2] after the entries, [3] after the marking
// (exits, stitch, marks, ranks, totals).
// After it the head (d_work + L.head) is complete.  n_bytes >= 512.
hipError_t TarChainWalk(const uint8_t* dev_tar, uint64_t n_bytes, const TarChainLayout& L, uint8_t* d_work,
                        uint32_t grid_cap, hipStream_t s, hipEvent_t* ev);
// The records (64 B each, 16-B aligned, n_entries = head.entries of them) and the
// name blob (name_bytes = head.name_bytes) of the entries TarChainWalk marked, in
// walk order; nothing is written past either.
hipError_t TarChainCompact(const uint8_t* dev_tar, uint64_t n_bytes, const TarChainLayout& L, const uint8_t* d_work,
                           uint64_t n_entries, uint64_t name_bytes, uint8_t* d_records, uint8_t* d_names,
                           uint32_t grid_cap, hipStream_t s);

// ---- all layers of an image in one pass (tarforest.hip; the contract: tarforest.h) ----
// The one device buffer of a pass over n_layers layers whose virtual space has
// v_blocks blocks: byte offsets of its parts (256-B aligned) and its size.  The
// head array (a TarChainHead per layer) comes first; the layer table and the
// u32 per segment that names its layer follow it as one range of tables_bytes,
// which the host fills (TarForestTables) and the pass uploads.
struct TarForestLayout {
  uint32_t n_layers = 0, segment = 0;
  uint64_t v_blocks = 0, n_segments = 0;
  uint64_t heads = 0, layers = 0, seg_layer = 0, cand = 0, chain = 0, seg_entry = 0, succ = 0, nlen = 0, rank = 0,
           noff = 0, temp = 0;
  uint64_t tables_bytes = 0, temp_bytes = 0, bytes = 0;
};
// segment_blocks as for TarChainPlan.  false: it is no segment size, n_layers is 0 or above
// kTarForestMaxLayers, or the layers do not fit one pass (TarForestCut says how many do).
bool TarForestPlan(const uint64_t* n_bytes, uint32_t n_layers, uint32_t segment_blocks, TarForestLayout* L);
// The tables of a planned pass into h_tables (L.tables_bytes bytes, host memory): ptrs[k] is 16-B aligned.
void TarForestTables(const TarForestLayout& L, const void* const* ptrs, const uint64_t* n_bytes, uint8_t* h_tables);
// Events as for TarChainWalk, ev[0] recorded after the upload of the tables.  After it the head array (d_work + L.heads) is complete.  h_tables stays
// valid until the stream has passed the upload.
hipError_t TarForestWalk(const TarForestLayout& L, const uint8_t* h_tables, uint8_t* d_work, uint32_t grid_cap,
                         hipStream_t s, hipEvent_t* ev);
// The records (64 B each; n_entries: the sum of the heads' entries) and the names (name_bytes: the sum
// of the heads' name_bytes) of all layers, layer after layer; nothing is written past either.
hipError_t TarForestCompact(const TarForestLayout& L, const uint8_t* d_work, uint64_t n_entries, uint64_t name_bytes,
                            uint8_t* d_records, uint8_t* d_names, uint32_t grid_cap, hipStream_t s);

// ---- path classify and Required on the GPU (tarrequired.hip; the contract: tarrequired.h) ----
struct PathTable;  // pathfilter.h
struct SureTable;
struct TarSkipTable;  // tar_skip_dev.h
// The stage's one device buffer for n entries (below 2^31) of n_layers layers (at least one) whose
// names take name_bytes, with a config base of cfg_len bytes; false: a count out of range.
// skip: the stage will run with LayerTar's skip options (room for their table in the upload).
bool TarRequiredPlan(uint64_t n, uint32_t n_layers, uint64_t name_bytes, uint32_t cfg_len, TarRequiredLayout* L,
                     bool skip = false);
// The tables of a planned stage into h_tables (L.tables_bytes bytes, host memory): n_layers + 1 record
// and name bases, the last pair (n, name_bytes), the config base, and (L.skip) the skip patterns.
void TarRequiredTables(const TarRequiredLayout& L, const uint64_t* rec_base, const uint64_t* name_base, const char* cfg,
                       uint8_t* h_tables, const TarSkipTable* skip = nullptr);
// The stage over d_records (64 B each, 16-B aligned) and d_names, as the compaction on the same stream
// wrote them: afterwards d_req (L.bytes, 256-B aligned) holds a TarRequiredCounts per layer at L.counts,
// the file records at L.recs and the path blob at L.blob.  d_path / d_sure: the scanner's tables in HBM
// (SecretScanner::allow_tables), either may be NULL.  h_tables stays valid until the stream has passed the upload.
// It is TarRequiredDecide followed by TarRequiredFinish; with skip options the two steps of the skip
// stage go between them: TarSkipMatchRun, which leaves the number of recorded directories in
// *d_n_dirs (4 B, zeroed on the stream here), and -- when the caller has read that count and it is
// not zero -- TarSkipUnderRun with a table of `slots` TarSkipSlot (a power of two, at least four
// times the recorded directories), which it clears on the stream first.
hipError_t TarRequiredRun(const TarRequiredLayout& L, const uint8_t* h_tables, const uint8_t* d_records,
                          const uint8_t* d_names, const PathTable* d_path, const SureTable* d_sure, uint8_t* d_req,
                          uint32_t grid_cap, hipStream_t s);
hipError_t TarRequiredDecide(const TarRequiredLayout& L, const uint8_t* h_tables, const uint8_t* d_records,
                             const uint8_t* d_names, const PathTable* d_path, const SureTable* d_sure, uint8_t* d_req,
                             uint32_t grid_cap, hipStream_t s);
hipError_t TarRequiredFinish(const TarRequiredLayout& L, const uint8_t* d_records, const uint8_t* d_names,
                             uint8_t* d_req, uint32_t grid_cap, hipStream_t s);
hipError_t TarSkipMatchRun(const TarRequiredLayout& L, const uint8_t* d_records, const uint8_t* d_names, uint8_t* d_req,
                           uint32_t* d_n_dirs, uint32_t grid_cap, hipStream_t s);
hipError_t TarSkipUnderRun(const TarRequiredLayout& L, const uint8_t* d_records, const uint8_t* d_names, uint8_t* d_req,
                           TarSkipSlot* d_table, uint64_t slots, uint32_t grid_cap, hipStream_t s);

}  // namespace tsg
