// GPU candidate engine: one instance per HIP device.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <memory>
#include <string>
#include <mutex>
#include <thread>
#include <vector>

#include "fetch_layout.h"
#include "rules.h"
#include "scan_layout.h"

namespace tsg {

constexpr uint32_t kChunk = 1024;  // bytes per chunk of the per-chunk '\n' counts and chunk -> file map

constexpr uint32_t kCandGateOpen = 1;   // a keyword of the rule occurs in the file (ASCII, GPU bits)
constexpr uint32_t kCandFoldFile = 2;   // keyword bits may miss occurrences through U+0130 / U+212A in this file
constexpr uint32_t kCandGateValid = 4;  // the two bits above were computed (GPU candidates)
constexpr uint32_t kCandDrop = 8;       // MatchKeywords is false for the rule in this file (never reaches the host)

struct Candidate {      // produced by the verify / full-scan kernels
  uint32_t file;
  uint32_t rule;
  int64_t wlo, whi;     // allowed match-start window, file-relative, inclusive
  int64_t nl_before;    // '\n' count in [file start, wlo)
  uint32_t flags;       // kCand*
  // wlo minus the positions of the last three '\n' before wlo, nearest first
  // (finalize kernel): the host's code-context walk reads these instead of
  // scanning back over long lines.  kNlNone: fewer newlines precede wlo;
  // kNlUnknown: not computed (host candidates, or farther than kNlReach).
  uint32_t nl_back[3];
  // The first three '\n' at or after wlo, as distances from wlo, nearest
  // first (finalize kernel): the line ends of the match line and the code
  // lines after it, which the host otherwise finds by memchr over long lines.
  // kNlNone: fewer newlines follow before the file end; kNlUnknown: not
  // computed (host candidates, or farther than kNlReach).
  uint32_t nl_fwd[3];
  uint32_t pad_;
};
static_assert(sizeof(Candidate) == 64, "Candidate is a 64-B record (tsg_oracle.h, tests/test_host_tail.py)");
constexpr uint32_t kNlNone = 0xFFFFFFFEu, kNlUnknown = 0xFFFFFFFFu;
// A candidate made on the host (no newline hints).
inline Candidate HostCandidate(uint32_t file, uint32_t rule, int64_t wlo, int64_t whi, int64_t nl_before,
                               uint32_t flags) {
  return Candidate{file, rule, wlo, whi, nl_before, flags, {kNlUnknown, kNlUnknown, kNlUnknown},
                   {kNlUnknown, kNlUnknown, kNlUnknown}, 0};
}
constexpr uint64_t kNlReach = uint64_t(1) << 20;

// The transformed bytes of chosen files of a host batch whose transform ran
// on the GPU (RunHost with kinds): buf holds them in file order, off is a
// full n_files+1 offset table into buf (files not chosen are empty).
// Files whose transform is the identity (kind 0, or kind 1 without a '\r')
// are not gathered: raw[f] = 1 and the exact pass reads them in the host
// batch as given.
struct TailOut {
  std::vector<uint8_t> buf;
  std::vector<uint64_t> off;
  std::vector<uint8_t> raw;
  uint64_t xform_bytes = 0;  // transformed arena bytes of the whole batch
};

// The candidate files of a device-only batch (no host copy of the bytes),
// brought back from HBM for the exact pass (fetch.h).  The caller sets
// h_offsets (the batch's n_files + 1 host offsets) and passes the struct to
// Run / Enqueue + Collect / FetchFiles; on return buf holds the fetched files:
// file f's bytes start at buf + off[f] where fetched[f] is set (its length is
// the batch's), off[n_files] is the bytes of buf in use.  Files below the
// direct threshold come packed in file order, each rounded up to 16 B; the
// others follow, copied straight from the arena.  buf is pinned memory on
// loan from the engine: it goes back when the struct is released or destroyed
// (before the engine is).
class GpuEngine;
class FetchPool;
struct FetchOut {
  const uint64_t* h_offsets = nullptr;
  const uint8_t* buf = nullptr;
  std::vector<uint64_t> off;
  std::vector<uint8_t> fetched;
  uint64_t files = 0, bytes = 0, direct_files = 0;
  uint32_t rounds = 0;   // staging rounds that carried packed bytes
  double ms_fetch = 0;   // plan + pack + copies (HIP events; direct copies by the host clock)
  // Windows mode (fetch_layout.h): the caller sets want_windows and prm; on return `windows`
  // says the fetch went that way, and buf then holds the packed granules instead of files:
  // run k's bytes start at buf + runs[k].packed (off / fetched are unused; fetch_host.h
  // FileViewOf gives a file's pieces).  whole_marked: files a candidate marked whole.
  bool want_windows = false, windows = false;
  FetchWinParams prm;
  std::vector<GranuleRun> runs;
  uint64_t granules = 0, whole_marked = 0;
  FetchOut() = default;
  FetchOut(const FetchOut&) = delete;
  FetchOut& operator=(const FetchOut&) = delete;
  ~FetchOut() { Release(); }
  void Release();
  // the loan (GpuEngine::TakeFetchBuf / GiveFetchBuf)
  GpuEngine* owner = nullptr;
  void* lease = nullptr;
  size_t lease_cap = 0;
};

struct BatchStats {
  uint64_t bytes = 0, files = 0, hits = 0, candidates = 0, special_files = 0, fullscan_tasks = 0, fold_sites = 0;
  uint64_t flagged_blocks = 0;
  uint64_t follow_hits = 0;     // anchor hits past the follow requirements + fold-kernel hits (the NFA runs on these)
  float ms_scan = 0, ms_confirm = 0, ms_careful = 0, ms_verify = 0, ms_fullscan = 0, ms_total = 0;
  float ms_finalize = 0, ms_chunkmap = 0;
  float ms_h2d_span = 0;  // RunHost: first copy issued -> last chunk done (the ingest-inclusive GPU time)
  float ms_xform = 0;     // RunHost with kinds: pre-transform kernels (part of ms_total)
  float ms_k0 = 0;        // the K0 phase's own span on the stream it ran on (ms_chunkmap: what K1 still waited for)
  uint64_t h2d_chunks = 0;
  bool hit_overflow = false, cand_overflow = false;
  // a scan with a skip list (SkipIn): the files marked and their bytes, the 4-KiB tiles K1 left out,
  // the runs of kept tiles, the most runs one K1 wave walked, the arena's tiles
  uint64_t skip_files = 0, skip_bytes = 0, skip_tiles = 0, skip_runs = 0, skip_wave_runs = 0, tiles = 0;
};

// The intermediate buffers of one synchronous scan (Run's optional `dump`;
// tsg_debug_engine_stages): copied out after the last kernel
// of the attempt that did not overflow, before the dropped candidates are
// erased.  Tests compare each stage with a CPU model; no product path asks
// for it.
struct StageHit {
  uint32_t file, aid;  // anchor id
  uint64_t end;        // the literal's end, file-relative
};
struct StageDump {
  uint32_t counters[kScanCtrWords] = {};  // scan_layout.h kCt*
  uint32_t kw_words = 0, hit_cap = 0, rec_cap = 0, cand_cap = 0;
  std::vector<StageHit> hits;        // min(counters[kCtHits], hit_cap)
  std::vector<uint32_t> kw;          // n_files x kw_words
  std::vector<uint32_t> flags;       // n_files
  std::vector<uint16_t> nl;          // '\n' per 1-KiB chunk, ceil(n_bytes / kChunk)
  std::vector<uint32_t> recs;        // min(counters[kCtRecs], rec_cap) flagged 16-B block indices
  std::vector<uint32_t> chunk_file;  // ceil(n_bytes / kChunk)
  std::vector<Candidate> cands;      // all counters[kCtCands], kCandDrop ones included
};

// The timing events of one scan's GPU phase (EnqueuePhase records them).
struct PhaseEvents {
  hipEvent_t ev[kNScanEv] = {};  // on the engine stream (scan_layout.h kEv*)
  hipEvent_t ev_fs = nullptr;    // before the full scan (scans with full-scan rules)
  hipEvent_t ev_k0[2] = {};      // the K0 phase's span on the stream it ran on
  bool Create();
  void Destroy();
};

// Files whose bytes the result does not need: d_skip[f] != 0
// for a file whose path is surely allow-listed (pathfilter.h).  The stream K0
// runs on waits for `ready`; the bytes stay readable until the scan's GPU phase
// is over.  K1 then streams only the 4-KiB tiles that hold a byte of
// some other file, and the full scan makes no pair for a marked file.
struct SkipIn {
  const uint8_t* d_skip = nullptr;
  hipEvent_t ready = nullptr;
  // The marked files belong to another scan (the split of a resident batch with a
  // transform): a candidate in one -- its ragged-end tile was
  // streamed with a neighbour's -- is dropped by the finalize kernel (kCandDrop),
  // so it reaches neither the fetch nor the host.  Off for the allow-path marks.
  bool drop_marked = false;
};

class GpuEngine {
 public:
  GpuEngine(const CompiledRules& cr, int device);
  ~GpuEngine();
  bool ok() const { return err_.empty(); }
  const std::string& error() const { return err_; }
  int device() const { return device_; }
  hipStream_t stream() const { return stream_; }

  // Run the kernels over a device-resident arena.  Offsets: n_files+1 u64
  // (device); the arena must have 64 readable bytes past n_bytes.  The
  // candidates are copied back into `cands`.
  // With fetch (a device-only batch): the candidate files' bytes are brought
  // back too, sized exactly (the candidates are known before the fetch is issued).
  // With dump (tests): the scan's intermediate buffers are copied out as well.
  bool Run(const uint8_t* d_arena, uint64_t n_bytes, const uint64_t* d_offsets, uint32_t n_files,
           std::vector<Candidate>* cands, BatchStats* st, FetchOut* fetch = nullptr, const SkipIn* skip = nullptr,
           StageDump* dump = nullptr);
  // The files want[f] != 0 of a device-resident arena into *out (synchronous;
  // the caller holds the engine's lock).  For the files a GPU pre-transform of
  // resident bytes left as they were read.
  bool FetchFiles(const uint8_t* d_arena, const uint64_t* d_offsets, uint32_t n_files,
                  const std::vector<uint8_t>& want, FetchOut* out);

  // Host-resident batch (PCIe-inclusive path): streamed in chunks through the
  // engine's staging ring (below), copies overlapping the kernels of earlier
  // chunks -- of this call and of the calls before it.  With kinds (per file,
  // xform.h), h_arena holds the bytes as read: each chunk is transformed on the
  // GPU before the scan, and the transformed bytes of the files that got
  // candidates come back in *tail.  Concurrent calls are allowed; the caller
  // must NOT hold the engine's device lock: RunHost takes `dev_mu` (the lock
  // the caller's other scans on this engine use) around each chunk's GPU work;
  // a null dev_mu means the engine's own device lock (dev_mu_), which then
  // must be the only lock guarding this engine's Run / Enqueue calls.  A
  // failure's text comes back in *err (err_ is shared with the other users of
  // the engine, so it is not the channel for a call that runs beside them).
  // d_src (optional, with kinds): the bytes as read are resident in HBM at d_src
  // (h_arena may be NULL): each chunk is copied device to device into its
  // staging buffer instead of from the host.
  // gather_base / gather_src (optional, with kinds): the files are not in
  // h_arena (NULL then) but at gather_base + gather_src[f] in page-locked,
  // device-mapped host memory (a registered tar layer); each chunk is gathered
  // from there into its staging buffer by a kernel (xform.h GatherHostFiles)
  // instead of one DMA copy -- no host copy of the file bytes.
  // d_src with gather_src (no gather_base): the files lie scattered in the resident
  // arena d_src, file f at d_src + gather_src[f]; each chunk is gathered from there
  // by census.h GatherDeviceFiles (no read leaves the arena and its 64-B tail).
  bool RunHost(const uint8_t* h_arena, uint64_t n_bytes, const uint64_t* h_offsets, uint32_t n_files,
               std::vector<Candidate>* cands, BatchStats* st, const uint8_t* kinds, TailOut* tail,
               std::mutex* dev_mu, std::string* err, const uint8_t* gather_base = nullptr,
               const uint64_t* gather_src = nullptr, const uint8_t* d_src = nullptr);

  // Split form of Run for pipelined callers: Enqueue (with the engine's lock
  // held) puts the whole GPU phase and the copies of the counters and of the
  // full candidate buffer into pinned host memory on the engine's streams and
  // returns; Collect (no lock) waits for that ticket.  The next scan's kernels
  // queue right behind the finalize kernel, so the GPU does not idle while a
  // caller wakes up, reads back and releases the lock; its K0 phase runs on a
  // stream of its own beside this scan's last kernels, and the copies on
  // another beside the next scan's (TSG_OVERLAP_K0=0 /
  // TSG_READBACK_STREAM=0 put either back on the engine stream).  Enqueue returns false when no
  // ticket is free or a diagnostic mode is on (then call Run); Collect sets
  // *rerun when a buffer overflowed (then call Run under the lock: it grows
  // the buffers and rescans).
  // The candidate read-back copies min(cand_cap, 2 x the largest count of
  // the last collected scans + 64 Ki) records: a one-off spike that grew the
  // device buffer does not make every later scan copy all of it; a count
  // above the copied part reruns the scan (as an overflow does).  Errors of
  // Enqueue / Collect are returned in *err (Collect runs without the engine's
  // lock, so it must not write err_).
  // With fetch (a device-only batch; the same struct to Enqueue and Collect):
  // the fetch of the candidate files is enqueued right behind the finalize
  // kernel -- marked, laid out and packed on the GPU, copied to pinned memory
  // on the fetch stream beside the next scan's kernels -- for a pre-sized
  // amount that follows the recent scans'; Collect sets *rerun when the marked
  // bytes exceed it (Run then fetches the exact amount and the next Enqueue
  // sizes for it).  Files of the direct threshold or more are copied by
  // Collect, one hipMemcpyAsync each on the fetch stream.
  struct Ticket {
    int slot = -1;
    uint32_t cand_copy = 0;  // candidates copied back
  };
  bool Enqueue(const uint8_t* d_arena, uint64_t n_bytes, const uint64_t* d_offsets, uint32_t n_files, Ticket* t,
               std::string* err, FetchOut* fetch = nullptr, const SkipIn* skip = nullptr);
  bool Collect(Ticket* t, std::vector<Candidate>* cands, BatchStats* st, bool* rerun, std::string* err,
               FetchOut* fetch = nullptr);

  // Device-only batches: the staging buffer's size (a round packs at most this
  // much; TSG_FETCH_STAGE_MB, default 256 MiB) and the length from which a file
  // is copied straight from the arena (TSG_FETCH_DIRECT_MB, default 8 MiB).
  // Rounded to the packing granule; takes effect with the next scan.
  void SetFetchSizes(uint64_t stage_bytes, uint64_t direct_bytes);
  // pinned fetch buffers on loan to a FetchOut
  void* TakeFetchBuf(size_t need, size_t* cap);
  void GiveFetchBuf(void* p, size_t cap);

 private:
  bool Ensure(void** p, size_t* cap, size_t need);
  // The buffers a scan's K0 phase writes before its K1 may start, or the
  // read-back and the fetch read after its finalize kernel.
  // Two sets, taken in turn by Enqueue: K0 of scan i + 1 fills the other set
  // on aux_stream_ while scan i's kernels run, and scan i's candidates leave
  // on rb_stream_ while scan i + 1's kernels run.  Everything produced and
  // consumed between K1 and finalize (d_nl_, d_recs_, d_hits_, d_folds_,
  // the full-scan lists) stays single: only stream_ touches it.
  struct WorkSet {
    void* chunk_file = nullptr; size_t cap_chunk_file = 0;
    // scans with a skip list: the kept-tile bitmap, the runs of kept tiles (begin tile, kept tiles before),
    // and the skip-list counters (scan_layout.h kSk*)
    void* keep_bits = nullptr; size_t cap_keep_bits = 0;
    void* runs = nullptr; size_t cap_runs = 0;
    uint32_t* skip_info = nullptr;
    void* kw = nullptr; size_t cap_kw = 0;
    void* flags = nullptr; size_t cap_flags = 0;
    void* cands = nullptr; size_t cap_cands = 0;
    uint32_t* counters = nullptr;  // the scan counters (scan_layout.h kCt*)
    uint32_t* fs_ctr = nullptr;    // the full-scan list counters (scan_layout.h kFs*)
    // free_ev: the last read of the set by the scan that used it (recorded beside Slot::done);
    // k0_done: the last K0 phase that filled it on aux_stream_.  *_rec: recorded at least once.
    hipEvent_t free_ev = nullptr, k0_done = nullptr;
    bool free_rec = false, k0_rec = false;
  };
  static constexpr int kSets = 2;
  WorkSet sets_[kSets];
  uint32_t set_turn_ = 0;                // the set the next Enqueue takes; Run and its fetches use sets_[0]
  hipStream_t aux_stream_ = nullptr;     // K0 phases of Enqueue'd scans (highest priority; TSG_OVERLAP_K0=0: unused)
  hipStream_t rb_stream_ = nullptr;      // counter / candidate read-back of Enqueue'd scans (TSG_READBACK_STREAM=0: unused)
  bool overlap_k0_ = true, readback_stream_ = true;
  // The end of the last K2 enqueued on stream_: a K0 phase on aux_stream_ starts behind it, beside the
  // latency-bound fold / verify / finalize kernels, never beside K1 or K2 (§4.10: launched together with
  // a K1, K0's workgroups take wave slots first and leave K1's two workgroups per CU unevenly placed for
  // the whole kernel; beside K2 it costs K2 what it saves).
  hipEvent_t k2_done_ = nullptr;
  bool k2_rec_ = false;
  struct KernelArgs;  // fills the kernels' parameter structs for EnqueuePhase (engine.hip, with their types)
  bool EnsureSets(uint64_t n_chunks, uint32_t n_files, uint64_t f_tiles, bool skip);
  bool EnqueuePhase(const uint8_t* d_arena, uint64_t n_bytes, const uint64_t* d_offsets, uint32_t n_files,
                    uint64_t n_chunks, WorkSet& W, bool k0_aux, PhaseEvents& E, const SkipIn* skip = nullptr);
  void InitCaps(uint64_t n_bytes);
  struct Slot {  // one in-flight Enqueue: its phase events and pinned read-back buffers
    PhaseEvents ev;
    hipEvent_t done = nullptr;
    hipEvent_t fin = nullptr, rb_done = nullptr;  // finalize done (stream_) / read-back done (rb_stream_)
    uint32_t* h_cnt = nullptr;
    uint32_t* h_skip = nullptr;  // pinned copy of the skip counters (WorkSet::skip_info), scans with a skip list
    bool has_skip = false;
    Candidate* h_cands = nullptr;
    size_t h_cap = 0;
    bool busy = false, has_fs = false;
    uint64_t n_bytes = 0;
    uint32_t n_files = 0;
    // device-only batches: the fetch enqueued with the scan
    bool has_fetch = false;
    hipEvent_t ev_f[2] = {};          // before the plan (scan stream) / after the last copy (fetch stream)
    void* h_fctr = nullptr;           // pinned FetchCounters
    void* lease = nullptr;            // pinned fetch buffer (TakeFetchBuf)
    size_t lease_cap = 0;
    uint64_t fetch_copy = 0;          // packed bytes copied back
    uint64_t stage = 0, direct = 0;   // the sizes the fetch was enqueued with
    bool win = false;                 // a windows fetch (h_fctr then holds FetchWinCounters)
    FetchWinParams prm;
    const uint8_t* d_arena = nullptr; // (direct copies are issued by Collect)
  };
  static constexpr int kSlots = 4;
  std::atomic<uint32_t> cand_recent_{0};  // largest candidate count of the recently collected scans
  Slot slots_[kSlots];
  std::mutex slot_mu_;
  std::mutex dev_mu_;  // RunHost's device lock when the caller passes none
  // Outgrown pinned read-back buffers.  hipHostFree waits for the whole
  // device, so they are not freed by the thread that regrows a slot (it holds
  // the GPU lock); a reaper thread frees them outside every engine lock, so
  // only that thread waits for the device.  Nothing references a retired
  // buffer: a slot is regrown only after Collect released its last ticket.
  void RetireHost(void* p);
  void ReaperLoop();
  std::mutex reap_mu_;
  std::condition_variable reap_cv_;
  std::vector<void*> retired_host_;  // (reap_mu_)
  bool reap_stop_ = false;           // (reap_mu_)
  std::thread reaper_;               // started with the first retirement
  std::atomic<uint64_t> retired_pending_{0}, retired_freed_{0};
  // Device-only batches (fetch.h).  The plan's scratch, the staging buffer and
  // the counters are shared by the scans in flight, in stream order: a pack
  // waits (ev_drained_) for the copy of the round before it, of this scan or of
  // the one before, and the copy (fetch_stream_) for its pack (ev_packed_).
  bool IssueFetch(const WorkSet& W, const uint8_t* d_arena, const uint64_t* d_offsets, uint32_t n_files,
                  const uint32_t* h_flags, uint64_t direct, uint64_t stage, uint64_t copy_bytes, uint8_t* h_dst,
                  void* h_ctr, hipEvent_t ev0);
  bool FetchNow(const uint8_t* d_arena, const uint64_t* d_offsets, uint32_t n_files, std::vector<uint8_t> want,
                bool upload_flags, FetchOut* out);
  void NoteFetch(uint64_t packed, uint64_t total);
  // windows mode (fetch_windows.h): the same rounds, events, staging buffer and fetch stream
  bool IssueFetchWin(const WorkSet& W, const uint8_t* d_arena, uint64_t n_bytes, const uint64_t* d_offsets,
                     uint32_t n_files, const FetchWinParams& prm, uint64_t stage, uint64_t copy_bytes, uint8_t* h_dst,
                     void* h_ctr, hipEvent_t ev0);
  bool FetchNowWin(const uint8_t* d_arena, uint64_t n_bytes, const uint64_t* d_offsets, uint32_t n_files,
                   const std::vector<Candidate>& cands, FetchOut* out);
  std::atomic<uint64_t> fetchw_stage_bytes_{uint64_t(256) << 20};  // SetFetchSizes' stage, rounded to granules
  std::atomic<uint64_t> fetchw_recent_packed_{0};  // the recent windows fetches' packed bytes (as fetch_recent_packed_)
  void* d_wscratch_ = nullptr; size_t cap_wscratch_ = 0;
  uint32_t* d_rule_max_len_ = nullptr;   // RuleGpu::max_len per rule, compact (the marking kernel's fwd reach)
  std::vector<uint32_t> h_rule_max_len_;
  bool EnsureFetchStream();
  std::atomic<uint64_t> fetch_stage_bytes_{uint64_t(256) << 20}, fetch_direct_bytes_{uint64_t(8) << 20};
  std::atomic<uint64_t> fetch_recent_packed_{0}, fetch_recent_total_{0};
  hipStream_t fetch_stream_ = nullptr;
  hipEvent_t ev_packed_ = nullptr, ev_drained_ = nullptr, ev_run_f_[2] = {};
  void* d_fscratch_ = nullptr; size_t cap_fscratch_ = 0;
  void* d_fstage_ = nullptr; size_t cap_fstage_ = 0;
  void* d_fctr_ = nullptr;
  void* h_run_fctr_ = nullptr;  // pinned FetchCounters of Run / FetchFiles
  void* h_fflags_ = nullptr; size_t cap_h_fflags_ = 0;  // pinned flags upload (FetchFiles)
  std::unique_ptr<FetchPool> fetch_pool_;  // pinned buffers not on loan (fetch_host.h)

 public:
  // Host memory bookkeeping (tests, tsg_debug_scanner_engine): retired
  // buffers not yet freed, retired buffers freed, the candidate capacity and
  // the pinned read-back bytes the ticket slots hold.
  struct HostMemInfo {
    uint64_t retired_pending, retired_freed, cand_cap, slot_bytes;
  };
  HostMemInfo host_mem_info();

 private:
  bool Transform(int b, uint32_t nf, const uint8_t** arena, const uint64_t** offsets, uint64_t* n_bytes,
                 std::vector<uint64_t>* xoff, float* ms);
  bool GatherTail(const std::vector<Candidate>& part, uint32_t f0, uint32_t nf, const std::vector<uint64_t>& xoff,
                  const uint64_t* raw_off, const uint8_t* kinds, std::vector<uint64_t>* tail_len, TailOut* tail);
  void DumpItemDiag();
  bool DumpStages(const WorkSet& W, const uint32_t* cnt, uint64_t n_bytes, uint32_t n_files, StageDump* d);
  std::vector<uint8_t> h_items_kind_;
  std::vector<uint32_t> h_items_id_;
  std::string err_;
  int device_ = 0;
  hipStream_t stream_ = nullptr;
  PhaseEvents run_ev_;  // Run's (Slot::ev for Enqueue'd scans)
  // tables
  uint32_t diag_mode_ = 0, diag_confirm_ = 0;
  AnchorInfo* d_anchors_ = nullptr;
  RuleGpu* d_rules_ = nullptr;
  uint32_t* d_rule_kw_ = nullptr;
  uint64_t* d_nfa_ = nullptr;
  uint32_t* d_fullscan_rules_ = nullptr;
  uint32_t kw_words_ = 0, n_rules_ = 0, n_fullscan_rules_ = 0;
  std::vector<uint32_t> fullscan_rules_;
  // streaming prefilter (filter.h)
  uint32_t* d_reach_ = nullptr;
  uint64_t* d_core_ = nullptr;
  uint32_t* d_group_items_ = nullptr;
  uint32_t* d_bucket_groups_ = nullptr;
  void* d_ftabs_ = nullptr;
  void* d_fold_pairs_ = nullptr;  // fold kernel work list
  void* d_fold_first_ = nullptr;  // per item: bytes that can start it (fold kernel prefilter)
  uint32_t n_fold_pairs_k_ = 0, n_fold_pairs_s_ = 0, n_fold_cap_k_ = 0, n_fold_cap_s_ = 0;
  void* d_fold_idx_off_ = nullptr;   // fold kernel: capable tasks by (rune kind, q, key byte)
  void* d_fold_idx_items_ = nullptr;
  uint32_t n_fold_cap_k_idx_ = 0, n_fold_cap_s_idx_ = 0;
  void* d_kwfold_pairs_ = nullptr;  // kwfold kernel work list (keyword items through U+0130 / U+212A)
  uint32_t n_kwf_ri_ = 0, n_kwf_rk_ = 0, n_kwf_ci_ = 0, n_kwf_ck_ = 0;
  bool kw_fold_ = false;
  uint32_t ftabs_bytes_ = 0, ft_bucket_off_ = 0, ft_bucket_items_ = 0, ft_items_ = 0;
  uint32_t ft_item_ids_ = 0, ft_item_cls_ = 0, ft_classes_ = 0, ft_luts_ = 0;
  // confirm-only part of the table blob (after the fold kernel's prefix): the
  // core tables over byte classes (filter.h core, columns deduplicated)
  uint32_t ftabs_fold_bytes_ = 0, ft_cmap_ = 0, ft_ccore_ = 0, ft_gitems_ = 0, ft_bgroups_ = 0, n_core_cls_ = 0;
  uint32_t ft_hkeys_ = 0, ft_hitems_ = 0, hash_bits_ = 0, hash_buckets_ = 0;  // literal-window hash
  size_t c_lds_bytes_ = 0;
  bool lds_tabs_ = true;  // confirm/fold kernels stage the item tables in LDS
  bool fold_stage_ = false;        // global-table fold kernel: items + classes staged in LDS, 16-wave workgroups
  uint32_t fold_grid_ = 2048;      // workgroups of the LDS-table fold kernel (TSG_FOLD_GRID)
  bool c_stage_classes_ = false;   // global-table confirm kernel: classes staged in LDS
  size_t fold_stage_bytes_ = 0;
  uint32_t n_fclasses_ = 0;
  void* d_recs_ = nullptr; size_t cap_recs_ = 0;
  uint32_t n_fitems_ = 0;
  // per-batch buffers
  void* d_nl_ = nullptr; size_t cap_nl_ = 0;
  uint32_t* h_run_skip_ = nullptr;  // pinned skip counters (Run)
  uint32_t k1_grid_cap_ = 0;        // TSG_DIAG_K1_GRID: at most this many K1 workgroups (tests; 0: no cap)
  void NoteSkip(const uint32_t* info, BatchStats* st) const;
  void* d_hits_ = nullptr; size_t cap_hits_ = 0;
  void* d_folds_ = nullptr; size_t cap_folds_ = 0;
  // host-batch streaming (RunHost): a ring of staging buffers, a copy stream
  hipStream_t copy_stream_ = nullptr;
  static constexpr int kNStage = 4;  // staging buffers: the copier runs up to three chunks ahead
  // The staging ring.  RunHost reserves one slot per chunk, numbered in call
  // arrival order across calls; slot s uses staging buffer s % kNStage.  One
  // copier thread (CopierLoop) copies the slots in order, slot s as soon as
  // slot s - kNStage has been scanned; chunks are scanned in slot order
  // (ring_turn_).  So the copy engine moves the next call's first chunks while
  // this call's last chunk is transformed, scanned and read back, and several
  // small host batches in flight (the analyzer's collectors) overlap their
  // copies with each other's kernels.
  struct HostCall;
  struct StageJob {
    uint64_t slot;
    HostCall* call;
    uint32_t f0, f1;  // the chunk's files
  };
  bool CopyChunk(const StageJob& j, std::string* err);
  void CopierLoop();
  std::mutex ring_mu_;
  std::condition_variable ring_cv_;
  std::deque<StageJob> ring_jobs_;                     // reserved, not yet copied (slot order)
  uint64_t ring_next_ = 0, ring_turn_ = 0, ring_copied_ = 0;  // next slot to reserve / to scan / copied below
  bool stage_ok_[kNStage] = {};                        // the copy of the buffer's current slot was issued
  std::string stage_err_[kNStage];
  bool ring_stop_ = false;
  std::thread copier_;
  hipEvent_t ev_copied_[kNStage] = {}, ev_h2d_[2] = {};
  void* d_stage_[kNStage] = {}; size_t cap_stage_[kNStage] = {};
  void* d_stage_off_[kNStage] = {}; size_t cap_stage_off_[kNStage] = {};
  uint64_t* h_off_[kNStage] = {}; size_t cap_h_off_[kNStage] = {};  // pinned, rebased chunk offsets
  uint64_t* h_xoff_ = nullptr; size_t cap_h_xoff_ = 0;  // pinned: transformed offsets + the error word
  // Pinned staging of Run's counter / candidate read-back and GatherTail's
  // uploads and read-back: a pageable hipMemcpy goes through the runtime's own
  // staging and held up the copier's H2D of later chunks (blocking 20-80 ms
  // copies at fixed chunks of the C2 ingest leg, TSG_RING_DEBUG).
  uint32_t* h_run_cnt_ = nullptr;
  void* h_run_cands_ = nullptr; size_t cap_h_run_cands_ = 0;
  void* h_gup_ = nullptr; size_t cap_h_gup_ = 0;
  void* h_gbuf_ = nullptr; size_t cap_h_gbuf_ = 0;
  bool EnsureHost(void** p, size_t* cap, size_t need);
  // GPU pre-transform (xform.h): per-chunk kinds, lengths, transformed offsets and bytes, the gather
  void* d_kind_[kNStage] = {}; size_t cap_kind_[kNStage] = {};
  // host-memory gather (RunHost gather_base): per staging buffer the chunk's source
  // offsets + work items (device) and their pinned staging
  void* d_gsrc_[kNStage] = {}; size_t cap_gsrc_[kNStage] = {};
  void* h_gsrc_[kNStage] = {}; size_t cap_h_gsrc_[kNStage] = {};
  void* d_xlen_ = nullptr; size_t cap_xlen_ = 0;
  void* d_xoff_ = nullptr; size_t cap_xoff_ = 0;
  void* d_xscan_ = nullptr; size_t cap_xscan_ = 0;
  void* d_xf_ = nullptr; size_t cap_xf_ = 0;
  void* d_gfiles_ = nullptr; size_t cap_gfiles_ = 0;
  void* d_gdst_ = nullptr; size_t cap_gdst_ = 0;
  void* d_gbuf_ = nullptr; size_t cap_gbuf_ = 0;
  hipEvent_t ev_x_[2] = {};
  uint64_t chunk_bytes_ = uint64_t(1) << 30;             // TSG_INGEST_CHUNK_MB
  ScanCaps caps_;                     // the list capacities (InitCaps; Run grows them after an overflow)
  uint32_t fs_chunk_ = 65536;         // TSG_FULLSCAN_CHUNK: full-scan bytes per lane (min, wave-wide pairs)
  void* d_fs_pairs_ = nullptr; size_t cap_fs_pairs_ = 0;  // FsPair list
  void* d_fs_tasks_ = nullptr; size_t cap_fs_tasks_ = 0;  // 4 x FsTask lists (by NFA width)
  void* d_fs_wave_ = nullptr; size_t cap_fs_wave_ = 0;    // pairs run wave-wide
  hipEvent_t ev_sync_ = nullptr;  // blocking-sync: the host waits asleep, not spinning
  bool blocking_sync_ = true;
  uint32_t verify_blocks_ = 4096;  // a lane per deferred hit (0.59 -> 0.51 ms vs 2048 on C2)
  uint32_t finalize_blocks_ = 16384;  // a wave per candidate, latency-bound: ~1 candidate per wave (0.42 -> 0.25 ms vs 1024)
  hipError_t WaitStream();
  hipError_t WaitEvent(hipEvent_t ev);
  uint32_t* d_item_diag_ = nullptr;   // TSG_DIAG_ITEMS=<file>: per-item counters dumped after each run
  std::string item_diag_path_;
};

}  // namespace tsg
