// The layout of the small arrays one scan of the candidate engine talks through
// (DESIGN.md §4.10 / §4.11): the scan counters, the full-scan list counters, the
// skip-list counters and the phase events -- and what the host does with the
// counters when a list overflowed.  Plain C++: kernels, host code and the debug
// C API share it.  The slot numbers are a debug ABI (tsg_debug_stage_dump hands
// the scan counters to the tests as they are): a slot is never renumbered.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace tsg {

// Words in each of the three counter arrays; K0 clears them all (chunk_map_kernel).
constexpr uint32_t kScanCtrWords = 16;
constexpr size_t kScanCtrBytes = kScanCtrWords * sizeof(uint32_t);

// Scan counters (WorkSet::counters, StageDump::counters).
constexpr uint32_t kCtHits = 0,         // anchor hits past the follow requirements + fold hits (may exceed hit_cap)
                   kCtCands = 1,        // candidates, kCandDrop ones included (may exceed cand_cap)
                   kCtSpecial = 2,      // files with fold runes
                   kCtHitOvf = 3,       // flag: the hit list overflowed
                   kCtCandOvf = 4,      // flag: the candidate list overflowed
                   kCtUnused5 = 5,
                   kCtFsOvf = 6,        // flag: a full-scan pair / task list overflowed
                   kCtRecs = 7,         // flagged-block records (may exceed rec_cap)
                   kCtRecOvf = 8,       // flag: the record list overflowed
                   kCtFolds = 9,        // fold-rune sites (may exceed fold_cap)
                   kCtFoldOvf = 10,     // flag: the fold-site list overflowed
                   kCtAnchorHits = 11,  // exact anchor-item matches in the confirm kernel (stats)
                   kCtUnused12 = 12,
                   kCtOpenPairs = 13,   // open (file, full-scan rule) pairs (stats)
                   kCtUnused14 = 14, kCtUnused15 = 15;

// Full-scan list counters (WorkSet::fs_ctr, FsLists::ctr).
constexpr uint32_t kFsPairs = 0,      // pairs
                   kFsTasks = 1,      // lane tasks, one counter per NFA width: kFsTasks + w, w < kFsWidths
                   kFsWidths = 4,
                   kFsWavePairs = 5,  // pairs run wave-wide
                   kNFsCtr = 6;

// Skip-list counters (WorkSet::skip_info; scans with a skip list).
constexpr uint32_t kSkRuns = 0,      // runs of kept tiles
                   kSkKept = 1,      // kept tiles
                   kSkTailKept = 2,  // the last tile is kept
                   kSkFiles = 3,     // files marked
                   kSkBytes = 4,     // their bytes (u64: 4, 5)
                   kSkWaveRuns = 6,  // most runs one K1 wave walked
                   kSkTiles = 7;     // the arena's tiles

// Phase events of one scan on the engine stream (PhaseEvents::ev).
enum : int {
  kEvStart = 0,     // start of the GPU phase (K0 when it runs on the engine stream, else what K1 still waits for)
  kEvK1 = 1,        // K1 start
  kEvK2 = 2,        // K1 end = K2 start
  kEvFold = 3,      // K2 end = fold start
  kEvVerify = 4,    // fold end = verify start
  kEvFinalize = 5,  // verify + full-scan end = finalize start
  kEvEnd = 6,       // finalize end
  kNScanEv = 7
};

// The capacities of the lists a scan fills; an overflow grows one and the scan runs again.
struct ScanCaps {
  uint32_t hit = 0, cand = 0, rec = 0, fold = 0;
  uint32_t fs_pair = 0, fs_task = 0;  // FsPair list / each of the kFsWidths FsTask lists
  uint32_t fs_task_bytes = 4096;      // TSG_FS_TASK_BYTES: full-scan lane task size (min; >= 8 x max_len)
};

constexpr uint32_t kFsTaskRecBytes = 8;  // sizeof(FsTask)
constexpr uint64_t kMaxFsTasks = 0x7FFFFFFFu / kFsTaskRecBytes / kFsWidths;

enum ScanList { kListNone = 0, kListRecs, kListFullScan, kListFolds, kListHits, kListCands };

// The list to grow after a scan with these counters: the first that overflowed, in the order
// the kernels fill them (a later list's count is not final while an earlier one was cut short).
inline ScanList OverflowedList(const uint32_t* cnt) {
  if (cnt[kCtRecOvf]) return kListRecs;
  if (cnt[kCtFsOvf]) return kListFullScan;
  if (cnt[kCtFoldOvf]) return kListFolds;
  if (cnt[kCtHitOvf]) return kListHits;
  if (cnt[kCtCandOvf]) return kListCands;
  return kListNone;
}

// Grows OverflowedList(cnt) to the count seen plus a quarter, and says which it was.
// fc: the full-scan list counters, read only for kListFullScan.
inline ScanList GrowOverflowed(const uint32_t* cnt, const uint32_t* fc, ScanCaps* c) {
  auto grown = [](uint32_t n, uint32_t slack, uint32_t rec_bytes) {
    return uint32_t(std::min<uint64_t>(uint64_t(n) + n / 4 + slack, 0xFFFFFFF0u / rec_bytes));
  };
  const ScanList which = OverflowedList(cnt);
  switch (which) {
    case kListNone: break;
    case kListRecs: c->rec = grown(cnt[kCtRecs], 4096, 4); break;
    case kListFullScan: {  // to the counts seen
      c->fs_pair = std::max<uint32_t>(c->fs_pair, fc[kFsPairs] + fc[kFsPairs] / 4 + 1024);
      uint32_t mt = 0;  // the longest of the task lists: they share one capacity
      for (uint32_t w = 0; w < kFsWidths; w++) mt = std::max(mt, fc[kFsTasks + w]);
      const uint64_t want = uint64_t(mt) + mt / 4 + 1024;
      if (want > kMaxFsTasks) {
        // the lists cannot grow that far: coarser lane tasks instead (any task
        // size is exact -- each lane starts max_len bytes before its range), so
        // the scan degrades instead of failing with an overflow on every attempt
        uint64_t tb = c->fs_task_bytes;
        while (tb < (uint64_t(1) << 26) && want * c->fs_task_bytes / tb > kMaxFsTasks) tb *= 2;
        c->fs_task_bytes = uint32_t(tb);
      }
      c->fs_task = uint32_t(std::min<uint64_t>(std::max<uint64_t>(c->fs_task, want), kMaxFsTasks));
      break;
    }
    case kListFolds: c->fold = grown(cnt[kCtFolds], 1024, 16); break;
    case kListHits: c->hit = grown(cnt[kCtHits], 1024, 12); break;
    case kListCands: c->cand = grown(cnt[kCtCands], 1024, 1); break;
  }
  return which;
}

}  // namespace tsg
