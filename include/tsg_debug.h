/* Host-logic inspection entry points of libtsg.so (no GPU needed).
 *
 * These expose the exact host pass's Go-regexp engine so the CPU test-suite can
 * check it against the oracle.  They replace nothing in the reference: they are
 * the C-ABI view of Go's regexp calls made by pkg/fanal/secret/scanner.go:112
 * (FindAllIndex), :130 (FindAllSubmatchIndex) and :171/:207/:216 (MatchString).
 * Status codes: 0 = OK, <0 = error (text via tsg_last_error()).
 */
#ifndef TSG_DEBUG_H
#define TSG_DEBUG_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* FindAll[Submatch]Index(text, -1).  windows: optional (lo,hi) inclusive pairs
 * restricting match starts (sorted); pass NULL/0 for an unrestricted search.
 * Writes up to out_cap int64 offsets; *out_len receives the full count and
 * *num_cap the number of capture groups. */
int tsg_regex_find_all(const char* pattern, const uint8_t* text, uint64_t n, int submatch,
                       const int64_t* windows, uint32_t n_windows, int64_t* out, uint64_t out_cap,
                       uint64_t* out_len, int32_t* num_cap);

/* Engine selection for the exact pass's FindAll (tests only; process-wide):
 * 0 auto (bit-state backtracker, Pike VM past its row budget), 1 Pike VM only,
 * 2 backtracker with an 8-position budget (exercises the fallback). */
void tsg_debug_regex_engine(int mode);
/* The GPU pre-transform (trivy_amd/csrc/xform.hip) on a host batch, on HIP
 * device `device`: out receives the transformed arena (up to out_cap bytes),
 * xoff the n_files + 1 transformed offsets.  kinds per file: 0 as is, 1 CR
 * strip (secret.go:121), 2 ExtractPrintableBytes (utils.go:128-160), 3 dropped
 * (no bytes).  Tests compare it with the oracle's transforms byte for byte. */
int tsg_debug_xform(int device, const uint8_t* raw, uint64_t n_bytes, const uint64_t* offsets, uint32_t n_files,
                    const uint8_t* kinds, uint8_t* out, uint64_t out_cap, uint64_t* xoff);
/* The analyzer's binary gate on the GPU (trivy_amd/csrc/classify.hip) on a host
 * batch, on HIP device `device`: the n_bytes of raw are uploaded followed by 64
 * bytes of 0x00 (the arena's readable tail; NUL is a byte IsBinary rejects, so
 * a kernel that let the tail reach a flag shows up), the kernel runs, and flags
 * receives one byte per file: utils.IsBinary (utils.go:85-103) over the file's
 * first min(size, 300) bytes. */
int tsg_debug_classify(int device, const uint8_t* raw, uint64_t n_bytes, const uint64_t* offsets, uint32_t n_files,
                       uint8_t* flags);
/* The census of the files a transform changes (trivy_amd/csrc/census.hip) on a
 * host batch, on HIP device `device`.  raw holds n_bytes + 64 bytes: the arena
 * and its readable tail, uploaded as given into an allocation of exactly that
 * size (the caller chooses the tail: bytes no file owns, which must not reach a
 * mark).  kinds per file as tsg_debug_xform's.  mark_out receives one byte per
 * file: 1 for kind 2 and kind 3, 1 for a kind-1 file that holds a 0x0D, else 0. */
int tsg_debug_transform_census(int device, const uint8_t* raw, uint64_t n_bytes, const uint64_t* offsets,
                               uint32_t n_files, const uint8_t* kinds, uint8_t* mark_out);
/* The gather of files from a resident arena into a packed buffer
 * (trivy_amd/csrc/census.hip GatherDeviceFiles) on HIP device `device`.  raw
 * holds n_bytes + 64 bytes as above.  File i is raw[src_off[i] .. src_off[i] +
 * dst_off[i + 1] - dst_off[i]) and lands at out + dst_off[i]: src_off has
 * n_files entries in any order, dst_off n_files + 1 ascending ones (dst_off[0]
 * need not be 0).  out holds dst_off[n_files] + 64 bytes; it is uploaded before
 * the kernel and read back after it, so every byte no file owns returns as given. */
int tsg_debug_gather_device(int device, const uint8_t* raw, uint64_t n_bytes, const uint64_t* src_off,
                            const uint64_t* dst_off, uint32_t n_files, uint8_t* out);
/* ---- the kernels that only move file bytes ----
 * Each is one synchronous call on HIP device `device`; the device allocations
 * have exactly the sizes stated; the argument checks come before any HIP call
 * (-2, text via tsg_last_error()); a HIP error is -1.
 *
 * The gather of transformed files (trivy_amd/csrc/xform.hip GatherFiles).  src
 * holds n_bytes + 64 bytes, uploaded as given (the caller chooses the tail);
 * xoff has n_files + 1 ascending entries ending at or before n_bytes; `files`
 * lists n file ids in any order and dst_off their n destinations: file files[i]
 * lands at out + dst_off[i].  out holds dst_bytes + 64 bytes; it is uploaded
 * before the kernel and read back after it, so every byte no file owns returns
 * as given.  Destinations that leave dst_bytes or overlap are refused. */
int tsg_debug_gather_files(int device, const uint8_t* src, uint64_t n_bytes, const uint64_t* xoff, uint32_t n_files,
                           const uint32_t* files, const uint64_t* dst_off, uint32_t n, uint8_t* out,
                           uint64_t dst_bytes);
/* The gather from mapped host memory (xform.hip GatherHostFiles).  The n_bytes
 * of src are copied into page-locked host memory mapped into the device's
 * address space, which the kernel reads through its device pointer, as in
 * production.  File i is src[src_off[i] .. src_off[i] + len[i]) and lands at
 * out + dst_off[i]; the (file, piece) items are built as the engine builds
 * them, one per 16 KiB.  out and dst_bytes as above.  A file with src_off < 32
 * or src_off + len + 32 > n_bytes is refused: the kernel's aligned loads touch
 * up to 30 bytes before a file and 31 after it. */
int tsg_debug_gather_host(int device, const uint8_t* src, uint64_t n_bytes, const uint64_t* src_off,
                          const uint64_t* len, const uint64_t* dst_off, uint32_t n_files, uint8_t* out,
                          uint64_t dst_bytes);
/* The files fetch of device-only batches (trivy_amd/csrc/fetch.hip): FetchPlan,
 * then the FetchPack rounds as GpuEngine::IssueFetch drives them.  The arena is
 * uploaded into an allocation of exactly n_bytes + 64 (the tail 0xEE); offsets
 * run from 0 to n_bytes.  The marked files come either from 64-B Candidate
 * records (flags NULL: the device buffer holds min(n_cands, cand_cap) records
 * while the device count says n_cands) or from `flags`, one u32 per file (cands
 * NULL, n_cands 0: the route FetchPlan takes without a candidate list).
 * stage_bytes is rounded down to 16 KiB, at least one; copy_bytes 0 means the
 * plan's packed_bytes, else a multiple of 16 below or above it.  The staging
 * allocation of stage_bytes + 64 is filled with 0xA5 before each round; a
 * round's bytes [0, w1 - w0) go to packed_out + w0, and a byte from there to the
 * allocation's end that is no longer 0xA5 is -4 (the text names round and
 * offset).  -3: packed_cap is below the bytes to copy.  list_out (n_files
 * entries) and lpoff_out (n_files + 1) receive the n_packed ids and n_packed + 1
 * packed offsets of the compacted list.  counters: packed_bytes, n_packed,
 * n_direct, n_files, file_bytes (fetch.h FetchCounters), rounds.  Files of
 * direct_bytes or more are counted, not copied. */
int tsg_debug_fetch_files_device(int device, const uint8_t* arena, uint64_t n_bytes, const uint64_t* offsets,
                                 uint32_t n_files, const void* cands, uint64_t n_cands, uint32_t cand_cap,
                                 const uint32_t* flags, uint64_t direct_bytes, uint64_t stage_bytes,
                                 uint64_t copy_bytes, uint8_t* packed_out, uint64_t packed_cap, uint32_t* list_out,
                                 uint64_t* lpoff_out, uint64_t counters[6]);
/* regexp.MatchString: 1 = match, 0 = no match, <0 = compile error. */
int tsg_regex_match(const char* pattern, const uint8_t* text, uint64_t n);

/* bytes.ToLower (Go semantics).  Writes up to out_cap bytes, returns the full length. */
int64_t tsg_go_bytes_to_lower(const uint8_t* s, uint64_t n, uint8_t* out, uint64_t out_cap);

/* ---- rule compiler inspection (tables the GPU kernels consume) ---- */
struct tsg_global;
typedef struct tsg_compiled tsg_compiled;
struct tsg_table_info;
typedef struct tsg_debug_rule_info {
  uint32_t nfa_words;     /* 0: relaxed NFA empty */
  uint32_t gate;          /* 0 always, 1 keyword bitset, 2 host-verified */
  uint32_t anchored;      /* 1 anchor-driven, 0 full-scan */
  uint32_t has_regex;
  const uint64_t* nfa;    /* O[W] L[W] F[W] B[256][W] */
  const uint32_t* kw_ids;
  uint32_t n_kw;
} tsg_debug_rule_info;
int tsg_debug_compile(const struct tsg_global* g, tsg_compiled** out);
/* The same with compiler options (tsg_scanner.h tsg_compile_options); out_calibrated (optional):
 * the anchors the calibration sample moved to a class run. */
struct tsg_compile_options;
int tsg_debug_compile_ex(const struct tsg_global* g, const struct tsg_compile_options* opt, tsg_compiled** out,
                         uint32_t* out_calibrated);
void tsg_debug_compiled_free(tsg_compiled* c);
int tsg_debug_compiled_info(const tsg_compiled* c, struct tsg_table_info* out);
int tsg_debug_rule(const tsg_compiled* c, uint32_t i, tsg_debug_rule_info* out);
/* 1 when every match of rule i holds one of its keywords (rules.h RuleGpu::kw_match_implied: the
 * kernels then neither test nor report its keyword gate), 0 otherwise, -1 for no such rule. */
int tsg_debug_rule_gate_implied(const tsg_compiled* c, uint32_t i);
int tsg_debug_anchor(const tsg_compiled* c, uint32_t j, uint32_t* rule, uint32_t* lit_len,
                     int32_t* off_lo, int32_t* off_hi);
const char* tsg_debug_keyword(const tsg_compiled* c, uint32_t k);
/* Anchor j's follow requirements (trivy_amd/csrc/rules.h FollowLut, 32 B), or NULL. */
const void* tsg_debug_anchor_req(const tsg_compiled* c, uint32_t j);
/* The streaming prefilter's tables (trivy_amd/csrc/filter.h): shape = {buckets, window, words},
 * reach[256 * words] (u32; bucket j in word j/4, slot s at bit 4s + j%4; the last bucket counts
 * newlines), bucket_off[buckets+1] -> bucket_items, items (16-B records), item_cls, classes
 * (8 u32 each). */
int tsg_debug_filter(const tsg_compiled* c, uint32_t* shape, const uint32_t** reach, const uint32_t** bucket_off,
                     const uint32_t** bucket_items, const void** items, uint32_t* n_items, const uint8_t** item_cls,
                     const uint32_t** classes, double* est_fp);
/* The anchor / fold ids of the prefilter items (items[k] owns ids[ids_off .. ids_off + n_ids)). */
int tsg_debug_filter_ids(const tsg_compiled* c, const uint32_t** ids, uint32_t* n);
/* The confirm step's core tables (trivy_amd/csrc/filter.h): out = {core groups (8 items each), distinct
 * byte columns over all groups (the byte classes the confirm kernel's LDS copy is compressed to: groups x
 * classes x 8 B), the most groups one bucket holds (lookups per fire), slots of the literal-window hash}. */
int tsg_debug_filter_core(const tsg_compiled* c, uint32_t out[4]);
/* Rule i's anchor summary: "[off_lo,off_hi] lit[*][+la] ..." or "-" (no anchor). */
const char* tsg_debug_rule_anchor(const tsg_compiled* c, uint32_t i);

/* The CPU-only test hooks (host tail with whole-file windows, host-only
 * scanners) and the CPU reference scan are NOT in libtsg.so: they live in the
 * oracle's library (oracle/native/tsg_oracle.h, oracle/build/libtsg_host.so). */

/* Host workers the process-wide pool would start now (TSG_POOL_THREADS unset):
 * the affinity mask, capped by the cgroup quota, shared by LOCAL_WORLD_SIZE
 * ranks (or TSG_POOL_SHARE processes), minus the per-process reserve. */
int tsg_debug_pool_budget(void);

/* A scanner's GPU engines' host-memory bookkeeping, summed over its engines:
 * out[0] retired pinned read-back buffers not yet freed, out[1] retired buffers
 * freed (by the engine's reaper thread), out[2] the largest candidate capacity,
 * out[3] pinned read-back bytes held by the ticket slots.  Returns -1 for a
 * scanner without a GPU engine.  (Bookkeeping for tests; call it between scans.) */
struct tsg_scanner;
int tsg_debug_scanner_engine(struct tsg_scanner* s, uint64_t out[4]);
/* K1's OR-form table (trivy_amd/csrc/k1_orform.h) of compiled rules: out receives
 * 256 rows of 4 u32, row b = (W_0, W_1, W_2, W_3)[b] with W_k = m_{2k+1} << 16 |
 * m_{2k}, m_s the 16-bit not-allowed mask of window slot s over the 16 buckets
 * (bit j = bit 4s + j%4 of reach word j/4), and W_3 = 1 for '\n' only.  It is
 * the row every replica of the filter kernel's LDS image holds.  -1: no filter,
 * or one that is not 16 buckets with a window of at most 6. */
int tsg_debug_filter_orform(const tsg_compiled* c, uint32_t out[1024]);

/* Where a scanner makes the findings of HBM-resident batches (tsg_batch.dev_arena):
 * mode 0 the host (the default; TSG_GPU_FINDINGS at scanner creation sets
 * another), 1 the GPU (trivy_amd/csrc/materialize.h), 2 the GPU while the exact
 * host pass is the bound (the last scan's outlasted 1.5x its GPU phase).  A
 * windows-mode device-only batch takes the GPU whatever the mode.  Returns the
 * previous mode, -1 for a scanner without a GPU engine.  (A/B and parity tests.) */
int tsg_debug_scanner_gpu_findings(struct tsg_scanner* s, int mode);

/* Device-only batches (tsg_batch.host_arena NULL): the size of the device staging
 * buffer the candidate files are packed into (a round carries at most this much)
 * and the length from which a file is copied straight from the arena instead
 * (defaults: TSG_FETCH_STAGE_MB, 256, and TSG_FETCH_DIRECT_MB, 8, read at scanner
 * creation).  stage_bytes is rounded down to the packing granule (16 KiB, at
 * least one; in windows mode 256 B, at least one); both take effect with the next scan.  Returns -1 for a scanner
 * without a GPU engine.  (Tests reach several rounds and the direct route on
 * kilobyte inputs with it.) */
int tsg_debug_scanner_fetch(struct tsg_scanner* s, uint64_t stage_bytes, uint64_t direct_bytes);

/* ---- the windows fetch of device-only batches (trivy_amd/csrc/fetch_layout.h) ----
 * FindAll over a piece of a text: the engine is handed bytes [lo, hi) of text
 * alone (a copy in a block of exactly that size) with the text's true length;
 * windows and results are relative to the text.  *hit_limit: 1 when the answer
 * could depend on a byte outside the piece (Regex::FindAllBounded, goregex.h),
 * the matches written are then not to be used.  Otherwise as tsg_regex_find_all. */
int tsg_regex_find_all_bounded(const char* pattern, const uint8_t* text, uint64_t true_len, uint64_t lo, uint64_t hi,
                               int submatch, const int64_t* windows, uint32_t n_windows, int64_t* out,
                               uint64_t out_cap, uint64_t* out_len, int32_t* num_cap, int32_t* hit_limit);
/* The host's plan of a windows fetch (fetch_host.h PlanWindowsOnHost) for the
 * given offsets and candidates (64-B Candidate records, engine.h).  rule_max_len:
 * one u32 per rule, 0xFFFFFFFF unbounded.  opts: {back, fwd_bytes, fwd_cap,
 * max_span}, 0 (or opts NULL) the default; back below 4 is refused.  runs:
 * (first granule, end granule, packed byte offset) triples; views: (file,
 * lo, hi, packed byte offset) quads, the file-relative pieces of every file in
 * file order; totals: granules, runs, whole files, packed bytes.  Up to the caps
 * are written, *n_runs / *n_views receive the full counts. */
int tsg_debug_fetch_windows_plan(const uint64_t* offsets, uint32_t n_files, const void* cands, uint64_t n_cands,
                                 const uint32_t* rule_max_len, uint32_t n_rules, const uint32_t* opts, uint64_t* runs,
                                 uint64_t runs_cap, uint64_t* n_runs, uint64_t* views, uint64_t views_cap,
                                 uint64_t* n_views, uint64_t totals[4]);
/* The same marking, ranking and packing on HIP device `device`
 * (fetch_windows.hip): the batch is uploaded into an allocation of exactly
 * n_bytes + 64 (the tail 0xEE), the candidate buffer holds min(n_cands,
 * cand_cap) records while the device count says n_cands (an overflowed list),
 * and the packed layout comes back through a staging buffer of stage_bytes
 * (rounded down to 256, at least 256) zeroed before each round.  counters:
 * granules, runs, whole files, rounds. */
int tsg_debug_fetch_windows_device(int device, const uint8_t* arena, uint64_t n_bytes, const uint64_t* offsets,
                                   uint32_t n_files, const void* cands, uint64_t n_cands, uint32_t cand_cap,
                                   const uint32_t* rule_max_len, uint32_t n_rules, const uint32_t* opts,
                                   uint64_t stage_bytes, uint8_t* packed, uint64_t packed_cap, uint64_t counters[4]);

/* The windows fetch's host side on a host batch, without a GPU (SecretScanner::SparseTail):
 * the windows of the given candidates (64-B Candidate records) are planned, each run of marked
 * granules is copied into a heap block of exactly its size, the sparse exact pass runs on those
 * blocks alone, the files it cannot answer are rescanned whole from the host arena, and the
 * findings are made by the host from the whole bytes (the stand-in for the GPU findings pass).
 * opts as tsg_debug_fetch_windows_plan's.  The result compares with tsg_debug_host_tail_cands
 * (oracle/native/tsg_oracle.h) on the same candidates. */
struct tsg_batch;
struct tsg_result;
struct tsg_fetch_window_stats;
int tsg_debug_sparse_tail(const struct tsg_global* g, const struct tsg_batch* batch, const void* cands,
                          uint64_t n_cands, const uint32_t* opts, struct tsg_result** out,
                          struct tsg_fetch_window_stats* window_stats);

/* ---- scans that skip allow-listed files (trivy_amd/csrc/pathfilter.h) ----
 * The GPU's "surely allowed" decision on the host: the table is built from the
 * exact literal forms of the given path regexes (the same builder the scanner
 * uses for its global allow rules) and run over the n_paths paths packed in
 * `paths` (path i is bytes off[i] .. off[i + 1]).  sure[i]: 1 when path i is
 * surely allowed.  has_form[r] (optional): 1 when pattern r has an exact
 * literal form.  <0: a pattern does not compile. */
int tsg_debug_sure_allow(const char* const* patterns, uint32_t n_patterns, const uint8_t* paths, const uint64_t* off,
                         uint32_t n_paths, uint8_t* sure, uint8_t* has_form);
/* What a scan's skip list did: out = {files marked, bytes in them, 4-KiB tiles
 * the streaming filter left out, runs of kept tiles, the most runs one of its
 * waves walked, the arena's tiles}.  All zero for a scan without one (no packed
 * paths, no rule with an exact form, TSG_GPU_SKIP_ALLOWED=0, a host arena or a
 * transform).  TSG_DIAG_K1_GRID=<n> at scanner creation caps the filter's grid
 * at n workgroups, so a small arena still gives a wave many tiles. */
int tsg_debug_result_skip(const struct tsg_result* r, uint64_t out[6]);
/* The span of a resident scan's K0 phase (chunk map with the clears, kept tiles,
 * their runs) on the stream it ran on, in ms.  In a pipeline that phase runs on
 * a stream of its own beside the kernels of the scan before, so it is no part
 * of tsg_stats.ms_chunkmap_kernel, which is the time the streaming filter
 * still waited for it (TSG_OVERLAP_K0=0 at scanner creation: the phase runs on
 * the engine stream and the two agree).  Summed over the chunks of a host batch. */
int tsg_debug_result_k0(const struct tsg_result* r, double* ms_k0);

/* ---- the candidate engine's stages (trivy_amd/csrc/engine.h StageDump) ----
 * One synchronous scan (GpuEngine::Run) of a host batch on HIP device `device`,
 * by an engine built from the compiled rules with the scanner's own constructor
 * (the TSG_* variant switches read there apply).  The arena is uploaded into an
 * allocation of exactly n_bytes + 64 whose last 64 bytes are `tail`: bytes no
 * file owns, which no stage may attribute to one.  What the kernels left behind
 * comes back before the dropped candidates are erased.  The caller sets the
 * buffers and their capacities (in records); up to the capacity is written and
 * the n_* fields receive the full counts:
 *   hits        (file, file-relative literal end, anchor id) as three u64 each
 *   kw          n_files x kw_words keyword bit words; flags: one u32 per file
 *   nl, chunk_file   one entry per 1-KiB chunk of the arena
 *   recs        flagged 16-B block indices (arena byte / 16)
 *   cands       64-B Candidate records, kCandDrop ones included
 * caps: {hit, record, candidate} capacity of the device lists in this scan.
 * counters: the engine's 16 scan counters (trivy_amd/csrc/scan_layout.h; a slot
 * keeps its number).  A count may exceed its list's capacity; a flag is 0 or 1:
 *   kCtHits 0        anchor hits past the follow requirements + fold-kernel hits
 *   kCtCands 1       candidates            kCtSpecial 2     files with fold runes
 *   kCtHitOvf 3      flag: hit list overflowed
 *   kCtCandOvf 4     flag: candidate list overflowed
 *   kCtFsOvf 6       flag: a full-scan list overflowed
 *   kCtRecs 7        flagged-block records  kCtRecOvf 8     flag: record list overflowed
 *   kCtFolds 9       fold-rune sites        kCtFoldOvf 10   flag: fold-site list overflowed
 *   kCtAnchorHits 11 exact anchor-item matches
 *   kCtOpenPairs 13  open (file, full-scan rule) pairs
 *   5, 12, 14, 15    unused */
typedef struct tsg_debug_stage_dump {
  uint32_t struct_size;  /* sizeof(tsg_debug_stage_dump) */
  uint32_t kw_words;
  uint32_t counters[16];
  uint32_t caps[3];
  uint32_t reserved_;
  uint64_t* hits;        uint64_t hits_cap, n_hits;
  uint32_t* kw;          uint64_t kw_cap, n_kw;
  uint32_t* flags;       uint64_t flags_cap, n_flags;
  uint16_t* nl;          uint64_t nl_cap, n_nl;
  uint32_t* chunk_file;  uint64_t chunk_file_cap, n_chunk_file;
  uint32_t* recs;        uint64_t recs_cap, n_recs;
  void* cands;           uint64_t cands_cap, n_cands;
} tsg_debug_stage_dump;
int tsg_debug_engine_stages(const tsg_compiled* c, int device, const uint8_t* arena, uint64_t n_bytes,
                            const uint64_t* offsets, uint32_t n_files, const uint8_t tail[64],
                            tsg_debug_stage_dump* out);
/* The same scan with a skip list: skip holds one byte per file, non-zero for a file whose
 * bytes the result does not need (NULL: no list, as above).  K1 then streams only the 4-KiB tiles that hold
 * a byte of another file (filter_kernel<true>: runs of kept tiles), so recs holds the flagged blocks of the
 * kept tiles only, and the nl entries of a dropped tile's four chunks are not written by this scan (their
 * content is unspecified); the later stages see the kept tiles' records. */
int tsg_debug_engine_stages_skip(const tsg_compiled* c, int device, const uint8_t* arena, uint64_t n_bytes,
                                 const uint64_t* offsets, uint32_t n_files, const uint8_t tail[64],
                                 const uint8_t* skip, tsg_debug_stage_dump* out);
/* What the engine grows after a scan that overflowed a list (scan_layout.h
 * GrowOverflowed), without a GPU.  counters: the 16 scan counters above;
 * fs_counters: the 6 full-scan list counters {pairs, tasks per NFA width x 4,
 * wave pairs}, read only when kCtFsOvf is set; caps, in and out: {hit, candidate,
 * record, fold site, full-scan pair, full-scan task capacity, full-scan lane
 * task bytes}.  Exactly one list grows per call.  Returns which: 0 none (no
 * flag set), 1 records, 2 full-scan lists, 3 fold sites, 4 hits, 5 candidates. */
int tsg_debug_scan_grow(const uint32_t counters[16], const uint32_t fs_counters[6], uint32_t caps[7]);

/* ---- layers resident in HBM (trivy_amd/csrc/tarindex.hip, tar_index_host.h) ----
 * tar_headers_kernel alone on HIP device `device`: dev_tar and records_out are
 * DEVICE pointers, both 16-B aligned (the caller's buffers: records_out holds
 * `capacity` 528-B records -- u64 block index, 8 B of padding, the 512 header
 * bytes -- and whatever guard the caller puts after them).  Blocks b < n_bytes /
 * 512 are read.  *count_out: the candidates found, which may exceed capacity;
 * records [0, min(count, capacity)) are written, in no particular order.
 * grid_cap != 0 caps the grid at that many workgroups.  ms_out (optional): the
 * kernel's time from HIP events. */
int tsg_debug_tar_headers(int device, const void* dev_tar, uint64_t n_bytes, uint64_t capacity, uint32_t grid_cap,
                          void* records_out, uint64_t* count_out, double* ms_out);
/* The record capacity tsg_analyzer_index_device_tar starts with (process-wide;
 * 0 = the default, n_bytes / 4096 + 1024): a small one forces the second run. */
void tsg_debug_set_tar_capacity(uint64_t records);
struct tsg_analyzer;
struct tsg_tar_index;
struct tsg_device_tar_stats;
/* The host half of tsg_analyzer_index_device_tar without a GPU: the candidate
 * records are given (n_records 528-B records, any order) instead of computed,
 * and `host_tar` (n_bytes) stands in for the device where the walk copies a
 * block or a range of the layer.  The index (not submittable: it has no device
 * layer) and the stats come back as from the real call; kernel_runs is 0. */
int tsg_debug_index_tar_records(struct tsg_analyzer* a, const uint8_t* host_tar, uint64_t n_bytes,
                                const void* records, uint64_t n_records, struct tsg_tar_index** out,
                                struct tsg_device_tar_stats* st);
/* What tsg_analyzer_submit_device_tar builds for files [first, first + count) of
 * an index, from given IsBinary flags (one per pseudo-file, 2 count + 1): *base,
 * the layer offset of the batch's arena; offs, 2 count + 2 offsets from 0; kinds
 * and binary, 2 count + 1 each.  -1: the range is outside the index. */
/* The GPU half of the chain walk alone (tsg_analyzer_set_tar_walk mode 1;
 * trivy_amd/csrc/tarchain.h) on HIP device `device`: dev_tar is a DEVICE pointer,
 * 16-B aligned; segment_blocks 0 = the default, else a power of two >= 8;
 * grid_cap != 0 caps every grid.  The outputs are HOST buffers: up to rec_cap
 * 64-B records into records_out and up to name_cap bytes into names_out (-3 when
 * either is too small; *n_records and *name_bytes then say what is needed);
 * stop_out: 4 words -- kind (0 END, 1 INCOMPLETE), reason, offset, extension
 * headers hopped before an END inside an entry; *candidates_out: the candidate
 * blocks.  Nothing is handed over for an INCOMPLETE stop (*n_records = 0). */
int tsg_debug_tar_chain(int device, const void* dev_tar, uint64_t n_bytes, uint32_t segment_blocks, uint32_t grid_cap,
                        void* records_out, uint64_t rec_cap, uint64_t* n_records, uint8_t* names_out,
                        uint64_t name_cap, uint64_t* name_bytes, uint64_t* stop_out, uint64_t* candidates_out);
/* The virtual block space of a forest pass without a GPU (trivy_amd/csrc/tarforest.h:
 * TarForestSpan, TarForestCut): v0_out[k], layer k's first virtual block with segments
 * of segment_blocks (0 = the default), as if all layers shared one pass; *v_blocks_out,
 * their total; *first_pass_out, how many layers from layer 0 on fit the first pass (0:
 * layer 0 alone is too large).  -1: an argument error. */
int tsg_debug_tar_forest_layout(const uint64_t* n_bytes, uint32_t n_layers, uint32_t segment_blocks, uint64_t* v0_out,
                                uint64_t* v_blocks_out, uint32_t* first_pass_out);
/* The GPU half of tsg_analyzer_index_device_tars alone (trivy_amd/csrc/tarforest.h):
 * one forest pass over n_layers layers on HIP device `device`.  dev_tars: n_layers
 * DEVICE pointers, each 16-B aligned; n_bytes: their sizes; segment_blocks and
 * grid_cap as above.  The outputs are HOST buffers: heads_out, 8 words per layer --
 * the 64 bytes of the layer's head: kind and reason (u32 each), offset, extension
 * headers hopped, stitch steps, entries, name bytes, candidates, 0; rec_base_out and
 * name_base_out, n_layers words each: where the layer's records (in records) and
 * names (in bytes) begin; the records and names of all layers (-3 when either
 * buffer is too small; *n_records and *name_bytes are the totals in any case).
 * Nothing is written past the outputs.  -2: an argument or HIP error. */
int tsg_debug_tar_forest(int device, const void* const* dev_tars, const uint64_t* n_bytes, uint32_t n_layers,
                         uint32_t segment_blocks, uint32_t grid_cap, uint64_t* heads_out, uint64_t* rec_base_out,
                         uint64_t* name_base_out, void* records_out, uint64_t rec_cap, uint64_t* n_records,
                         uint8_t* names_out, uint64_t name_cap, uint64_t* name_bytes);
/* The fallback reason (tsg_tar_walk_stats.fallback) of the analyzer's last index
 * call in mode 1, also of one that failed and so left no index to ask; -1: NULL. */
int tsg_debug_tar_walk_last_fallback(const struct tsg_analyzer* a);
/* The host half of mode 1 without a GPU: n_records 64-B records in walk order,
 * their name blob and the stop (4 words as above; it must be END) are given
 * instead of computed.  The index (not submittable) and the stats come back as
 * from the real call with candidates_given candidates; kernel_runs is 0. */
int tsg_debug_index_tar_entries(struct tsg_analyzer* a, const void* records, uint64_t n_records, const uint8_t* names,
                                uint64_t name_bytes, const uint64_t* stop, uint64_t n_bytes,
                                uint64_t candidates_given, struct tsg_tar_index** out,
                                struct tsg_device_tar_stats* st);
int tsg_debug_tar_batch_plan(const struct tsg_tar_index* ix, uint32_t first, uint32_t count, const uint8_t* flags,
                             uint64_t* base, uint64_t* offs, uint8_t* kinds, uint8_t* binary);
/* The allow-path tables the Required stage of a resident layer reads (tsg_analyzer_set_tar_required
 * mode 1; trivy_amd/csrc/pathfilter.h), as the scanner keeps them on the host: the raw PathTable
 * into path_table_out and the raw SureTable into sure_table_out.  *have_out: bit 0 a path table,
 * bit 1 a sure table.  -1: an argument error or a buffer too small. */
int tsg_debug_tar_required_tables(const struct tsg_analyzer* a, void* path_table_out, uint64_t path_cap,
                                  void* sure_table_out, uint64_t sure_cap, uint32_t* have_out);
/* The device stage alone (trivy_amd/csrc/tarrequired.h) on the analyzer's GPU, over HOST buffers:
 * n_records 64-B entry records in walk order, the name blob, and the layer table as n_layers + 1
 * record bases and name bases (from 0 to n_records / name_bytes).  grid_cap != 0 caps every grid.
 * Back come: a verdict byte per entry (0 other, 1 whiteout, 2 opaque dir, 3 dropped, 4 kept,
 * 5 ask-allow, 6 ask-name, 7 a name outside its layer's blob), up to rec_cap 48-B file records, up to
 * blob_cap bytes of paths (-3 when either is too small; the two totals are set in any case), and 16
 * words of counts per layer.  -4: a record has its name outside its layer's blob -- it was not read,
 * its verdict is 7, and the other outputs are those of the remaining entries.  -2: an argument or
 * HIP error. */
int tsg_debug_tar_required(struct tsg_analyzer* a, const void* records, uint64_t n_records, const uint8_t* names,
                           uint64_t name_bytes, const uint64_t* rec_base, const uint64_t* name_base, uint32_t n_layers,
                           uint32_t grid_cap, uint8_t* verdicts_out, void* file_recs_out, uint64_t rec_cap,
                           uint64_t* n_file_recs, uint8_t* blob_out, uint64_t blob_cap, uint64_t* blob_bytes,
                           uint64_t* counts_out);
/* The same stage with its skip stage (tsg_analyzer_set_tar_required_skip mode 1; tarrequired.h),
 * whatever the analyzer's switches and options say: the cleaned patterns are given.  table_slots
 * != 0 forces the size of the recorded directories' table: a power of two of at least four times
 * the recorded directories (twice their keys: a path and its direct parent each), else -1 -- the
 * smallest such table has the longest probe sequences.  Verdicts 8 (a skipped directory: it has a
 * record), 9 (a skipped file) and 10 (under a skipped directory) can come back; words 14 and 15 of
 * a layer's counts are then the number of verdicts 8, and of 9 | 10 << 32.  *table_slots_out
 * (optional): the slots used, 0 when no directory was recorded.  -1 also: no pattern, or one the
 * device does not take. */
int tsg_debug_tar_required_skip(struct tsg_analyzer* a, const void* records, uint64_t n_records, const uint8_t* names,
                                uint64_t name_bytes, const uint64_t* rec_base, const uint64_t* name_base,
                                uint32_t n_layers, uint32_t grid_cap, const char* const* skip_dirs, uint32_t n_dirs,
                                const char* const* skip_files, uint32_t n_files, uint64_t table_slots,
                                uint8_t* verdicts_out, void* file_recs_out, uint64_t rec_cap, uint64_t* n_file_recs,
                                uint8_t* blob_out, uint64_t blob_cap, uint64_t* blob_bytes, uint64_t* counts_out,
                                uint64_t* table_slots_out);
/* The pattern classifier behind that switch (trivy_amd/csrc/tar_skip_dev.h), without a GPU.
 * classify: 1 when the device takes the whole option set -- forms_out (optional, n_dirs + n_files
 * bytes) then holds each pattern's form: 0 L, 1 "**" "/L", 2 "L/" "**", 3 "**" "/" "*S" --, 0 when
 * it does not, -1 an argument error.  match: the device's matcher for one pattern against a
 * cleaned path: 1 / 0, -1 when the device does not take the pattern. */
int tsg_debug_tar_skip_classify(const char* const* skip_dirs, uint32_t n_dirs, const char* const* skip_files,
                                uint32_t n_files, uint8_t* forms_out);
int tsg_debug_tar_skip_match(const char* pattern, const uint8_t* fp, uint32_t len);
/* The host half behind that stage without a GPU: one layer's file records, its path blob and its 16
 * words of counts are given instead of computed, with the stop (it must be END) as for
 * tsg_debug_index_tar_entries.  The index (not submittable) and the stats come back as from the
 * real call; kernel_runs is 0.  -1: an argument error, or records that contradict the blob or the
 * counts.  With tsg_analyzer_set_tar_required_skip mode 1 and options the device takes, the input
 * is that of a stage with its skip stage; then 1 (no index): an asked name is a skipped directory,
 * and the real call indexes such a layer from the walk's records. */
int tsg_debug_index_tar_files(struct tsg_analyzer* a, const void* file_recs, uint64_t n_recs, const uint8_t* blob,
                              uint64_t blob_bytes, const uint64_t* counts, const uint64_t* stop, uint64_t n_bytes,
                              uint64_t candidates_given, struct tsg_tar_index** out, struct tsg_device_tar_stats* st);

/* ---- the findings kernels and the path filter ----
 * Each is one synchronous call on HIP device `device`; the argument checks come
 * before any HIP call (-2, text via tsg_last_error()); a HIP error is -1.
 *
 * mat_locate_kernel and mat_write_kernel (trivy_amd/csrc/materialize.hip) through
 * the real FindingMaterializer (Begin, fill, Run, End).  arena holds n_bytes + 64
 * bytes, uploaded as given into an allocation of exactly that size (the caller
 * chooses the tail); offsets has n_files + 1 entries from 0 to n_bytes.
 * mat_files, matches and spans are MatFile (24 B), MatMatch (40 B) and MatSpan
 * (24 B) records as materialize.h lays them out; text_bound is the scanner's own
 * (the sum of MatTextBound over the locations).  Refused (-2): a location outside
 * its file, with e < s, with a_wlo > s, or (when not empty) covered by no span;
 * spans of a file that are unsorted, touch, overlap, leave the file or lack the
 * sentinel (s = e = INT64_MAX) as their last; m0 / s0 that are not the sums of
 * the nm / ns of the file records before, a location whose fidx is not the record
 * that holds it, records that leave locations or spans over.  MatFile.file may
 * come in any order and repeat.
 * Out: findings_out, n_match FindingOut records (40 B); pref_out, n_match + 1
 * words (text offset << 32 | line index, exclusive, global to the call); up to
 * lines_cap LineOut records (24 B) and up to text_cap text bytes; totals =
 * {lines, text bytes}, set whenever the locate pass came back.  -3: a cap is
 * below its total (findings and pref are written).  -5: Run's "line search and
 * line count disagree" (the kernel's error word).  -6: the totals are past
 * text_bound or 4 lines per location.  guard != 0 turns on the materializer's
 * guard bytes (FindingMaterializer::set_guard): the three device output buffers
 * are 0xA5 over their whole capacity before the first kernel, and a byte past
 * the n_match findings, the lines or the text that is not 0xA5 after the write
 * kernel is -4 (the text names the buffer and the offset). */
int tsg_debug_materialize(int device, const uint8_t* arena, uint64_t n_bytes, const uint64_t* offsets, uint32_t n_files,
                          const void* mat_files, uint32_t n_mat_files, const void* matches, uint32_t n_match,
                          const void* spans, uint32_t n_span, int guard, void* findings_out, uint64_t* pref_out,
                          void* lines_out, uint64_t lines_cap, uint8_t* text_out, uint64_t text_cap,
                          uint64_t totals[2]);
/* BuildPathTable / BuildSureTable (trivy_amd/csrc/pathfilter.h) on given literals, without a GPU.
 * The prefilter's: literal i is lit_bytes[lit_off[i] .. lit_off[i + 1]) with rule id lit_rule[i].
 * The exact ones: literal i has positions sure_off[i] .. sure_off[i + 1], position p accepting the
 * two bytes sure_pairs[2 p], sure_pairs[2 p + 1] (equal for a case-sensitive one); sure_flags[i]:
 * bit 0 begin (^), bit 1 end ($).  The raw PathTable and SureTable are written (sizes as for
 * tsg_debug_tar_required_tables; zeroed when not built).  Returns bit 0: the path table was built,
 * bit 1: the sure table; -1: an argument error or a buffer too small. */
int tsg_debug_path_tables(const uint8_t* lit_bytes, const uint64_t* lit_off, const uint32_t* lit_rule, uint32_t n_lits,
                          const uint8_t* sure_pairs, const uint64_t* sure_off, const uint8_t* sure_flags,
                          uint32_t n_sure, void* path_table_out, uint64_t path_cap, void* sure_table_out,
                          uint64_t sure_cap);
/* path_filter_kernel (trivy_amd/csrc/pathfilter.hip) through one PathFilter built from the raw
 * path_table and (unless NULL) sure_table: the batches run one after another through Submit /
 * Finish / Release, so the slot, its counter parity and the last record count carry over from
 * batch to batch.  Batch b holds paths batch_first[b] .. batch_first[b + 1]; path i is
 * paths[off[i] .. off[i + 1]).  flags: bit 0 the paths go through Submit's host-packed route
 * (else into a device allocation of exactly the batch's path bytes, offsets from 0), bit 1
 * want_skip.  Out: batch b's PathHit records (16 B) at hits_out + batch_first[b] and their count
 * in n_hits_out[b]; have_skip_out[b] = 1 when the batch had skip bytes (want_skip and a sure
 * table), then copied after the `ready` event from Pending::d_skip to skip_out +
 * batch_first[b]; the slot's skip bytes are 0xEE when allocated (PathFilter::set_skip_fill), so
 * a byte the kernel leaves unwritten shows.  hits_out and skip_out hold one entry per path. */
int tsg_debug_path_filter(int device, const void* path_table, const void* sure_table, const uint8_t* paths,
                          const uint64_t* off, const uint32_t* batch_first, uint32_t n_batches, uint32_t flags,
                          void* hits_out, uint32_t* n_hits_out, uint8_t* skip_out, uint8_t* have_skip_out);

/* Thread-local text of the last error. */
const char* tsg_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
