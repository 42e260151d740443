/* libtsg.so -- MI355X secret-scanning engine, C ABI (cgo / ctypes bindable).
 *
 * Drop-in boundary for pkg/fanal/secret (undistro/trivy @ 2024-12-20).  The
 * host language keeps ParseConfig / NewScanner's rule-set assembly
 * (pkg/fanal/secret/scanner.go:277-364) and hands the resulting *Global* to
 * tsg_scanner_new; Scan(ScanArgs) (scanner.go:377-463) becomes a batched
 * tsg_scan over a contiguous arena of CR-stripped file contents
 * (pkg/fanal/analyzer/secret/secret.go:117-141 does the stripping).
 *
 * Entry point                 replaces (reference)
 *   tsg_scanner_new           secret.NewScanner(config)            scanner.go:320-364
 *   tsg_scanner_allow_path    (Global).AllowPath(path)             scanner.go:57-59
 *   tsg_scan                  (*Scanner).Scan(ScanArgs), per file  scanner.go:377-463
 *   tsg_result_*              types.Secret / SecretFinding / Code  pkg/fanal/types/secret.go:5-20,
 *                                                                 misconf.go:48-61
 * Conventions: all pointers are borrowed for the duration of the call;
 * results are owned by the library until tsg_result_free.  Status: 0 = OK,
 * <0 = error, text via tsg_last_error() (tsg_debug.h).  Thread-safety: scans on
 * one scanner may overlap (tsg_scan_submit); their GPU phases are serialized
 * on the scanner's HIP stream, the exact host passes run concurrently.
 */
#ifndef TSG_SCANNER_H
#define TSG_SCANNER_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct tsg_allow_rule {  /* AllowRule, scanner.go:196-201 */
  const char* id;
  const char* regex;             /* NULL = none; "" = matches everything (Go compiles "") */
  const char* path;              /* NULL = none; "" = matches everything */
} tsg_allow_rule;

typedef struct tsg_rule {        /* Rule, scanner.go:89-100 */
  const char* id;
  const char* category;
  const char* title;
  const char* severity;          /* already normalised by ParseConfig */
  const char* regex;             /* NULL = rule without regex (never matches); "" = empty regex */
  const char* path;              /* NULL = any path; "" = empty regex (matches every path) */
  const char* secret_group_name; /* "" = whole match */
  const char* const* keywords;
  uint32_t n_keywords;
  const tsg_allow_rule* allow_rules;
  uint32_t n_allow_rules;
  const char* const* exclude_regexes; /* ExcludeBlock.Regexes */
  uint32_t n_exclude_regexes;
} tsg_rule;

typedef struct tsg_global {      /* Global, scanner.go:45-49 (the assembled rule set) */
  const tsg_rule* rules;
  uint32_t n_rules;
  const tsg_allow_rule* allow_rules;
  uint32_t n_allow_rules;
  const char* const* exclude_regexes;
  uint32_t n_exclude_regexes;
} tsg_global;

typedef struct tsg_scanner tsg_scanner;
typedef struct tsg_result tsg_result;

/* Compile the rule set (keyword/anchor automaton + relaxed NFAs) and bind a HIP device. */
int tsg_scanner_new(const tsg_global* g, int device, tsg_scanner** out);

/* Compiler options (versioned like tsg_batch_ext: struct_size first, unknown
 * sizes refused).  v1: calib / calib_bytes, an optional sample of the bytes
 * the scanner will see (e.g. the first batch of a scan job): a rule with both
 * a literal and a class-run anchor then takes the one that fires less on it
 * (trivy_amd/csrc/rules.h CompileOptions).  Findings never depend on it --
 * only which prefilter item finds the candidates. */
typedef struct tsg_compile_options {
  uint32_t struct_size;
  uint32_t reserved;
  const uint8_t* calib;
  uint64_t calib_bytes;
} tsg_compile_options;
#define TSG_COMPILE_OPTIONS_SIZE_V1 ((uint32_t)(offsetof(tsg_compile_options, calib_bytes) + sizeof(uint64_t)))
int tsg_scanner_new_ex(const tsg_global* g, int device, const tsg_compile_options* opt, tsg_scanner** out);
void tsg_scanner_free(tsg_scanner* s);
/* 1 if path is globally allowed (Global.AllowPath), else 0. */
int tsg_scanner_allow_path(const tsg_scanner* s, const char* path, uint64_t len);

/* A batch of files, back to back in one arena.  Where the bytes are:
 *   host_arena only             a host-resident batch, streamed to the GPU;
 *   host_arena + dev_arena      a mirrored batch: the GPU scans dev_arena, the exact
 *                               host pass reads host_arena (the same bytes);
 *   dev_arena only              a device-only batch (host_arena NULL): no host copy
 *                               of the bytes exists.  The GPU scans dev_arena and the
 *                               files that got candidates -- only those, whole -- are
 *                               copied back to pinned host memory for the exact pass
 *                               (tsg_result_fetch_stats says how much); in windows mode
 *                               (tsg_scanner_set_fetch_options) only the bytes around
 *                               the candidates are;
 *   gather_base (tsg_batch_ext) host_arena NULL, the files in mapped host memory.
 * host_arena NULL with neither dev_arena nor gather_base is an argument error
 * (status <0 before any GPU work), as is gather_base together with dev_arena.
 * host_offsets is always required: it is small, and the host needs the sizes.
 * dev_arena, in every mode: 16-B aligned, with 64 readable bytes past its end
 * (host_offsets[n_files]); the library never pads it by copying. */
typedef struct tsg_batch {
  uint32_t n_files;
  const uint8_t* host_arena;     /* concatenated contents; NULL: a device-only batch (dev_arena set)
                                    or a gathered one */
  const uint64_t* host_offsets;  /* n_files + 1, required */
  const void* dev_arena;         /* optional: the batch's bytes in HBM -- the same bytes as host_arena
                                    where that is given, the only copy where it is NULL (16-B aligned,
                                    64 readable bytes past the end) */
  const void* dev_offsets;       /* optional: device copy of host_offsets (without it the library
                                    uploads one for the scan) */
  const char* const* paths;      /* ScanArgs.FilePath per file */
  const uint64_t* path_lens;     /* optional */
  const uint8_t* binary;         /* optional ScanArgs.Binary per file */
  /* optional, per file: the analyzer's pre-scan transform, run on the GPU:
   * 0 as is, 1 every '\r' removed (secret.go:121), 2
   * utils.ExtractPrintableBytes (.pyc, secret.go:112-117, utils.go:128-160),
   * 3 dropped: a file the analyzer skips (Required false, or binary and not
   * .pyc, secret.go:108-117) that still lies in the arena -- it contributes no
   * bytes to the scan, gets no candidates, is never fetched, and its result
   * is kind 0 (valid for host, gathered and resident batches alike).
   * host_arena / host_offsets then hold the bytes as read.  With dev_arena
   * the bytes as read are resident: dev_arena holds them, host_offsets lays
   * them out as read, and host_arena is NULL or holds the same bytes; how such
   * a batch is scanned -- in rewritten chunks, or the unchanged files where they
   * lie -- is the scanner's tsg_scanner_set_resident_transform mode. */
  const uint8_t* transform;
  /* optional: the FilePath bytes packed in HBM (dev_path_offsets: n_files + 1
   * u64, device) -- the global allow-path rules (scanner.go:381-386) are then
   * prefiltered on the GPU and the host runs them only on the paths that hold
   * one of their literals (trivy_amd/csrc/pathfilter.h).  `paths` is still
   * required (the exact rule and the results use it). */
  const void* dev_paths;
  const void* dev_path_offsets;
} tsg_batch;  /* frozen: the layout of round 4; later fields go to tsg_batch_ext */

/* Versioned batch.  struct_size is sizeof(tsg_batch_ext) as the caller was
 * built: the library reads only the fields that size covers, and refuses a
 * size it does not know (status <0, tsg_last_error names the sizes it knows),
 * so a caller built against an older or newer header never has fields read
 * past the end of its struct.  Known sizes: TSG_BATCH_EXT_SIZE_V1 (112 on
 * the 64-bit ABI), TSG_BATCH_EXT_SIZE_V2 (128).  The plain tsg_batch entry points read the frozen fields
 * only (a caller built against the round-4 header passes exactly those). */
typedef struct tsg_batch_ext {
  uint32_t struct_size;
  tsg_batch base;
  /* v1: the FilePath bytes packed in host memory (host_path_offsets: n_files
   * + 1 u64 into host_paths), as the analyzer's collectors hold them; without
   * base.dev_paths the engine copies them to HBM for the same GPU allow-path
   * prefilter (NULL: the host runs the rules over every path). */
  const uint8_t* host_paths;
  const uint64_t* host_path_offsets;
  /* v2 (round 6): gather_base / gather_src, with base.transform set and
   * base.host_arena NULL -- file f's bytes as read are gather_base +
   * gather_src[f] .. + (host_offsets[f + 1] - host_offsets[f]) in page-locked,
   * device-mapped host memory (tsg_host_register_mapped; a tar layer as the
   * analyzer's collectors hold it): the GPU gathers them itself, no host copy.
   * host_offsets still lay out the batch (the files back to back).  The GPU
   * reads aligned 16-B blocks: the 32 bytes before each file's data and the 32
   * after its end must lie in the mapped region too (the loads touch up to 30
   * before and 31 after; a tar's 512-B headers and padding provide them). */
  const uint8_t* gather_base;
  const uint64_t* gather_src;
} tsg_batch_ext;
#define TSG_BATCH_EXT_SIZE_V1 ((uint32_t)(offsetof(tsg_batch_ext, host_path_offsets) + sizeof(const uint64_t*)))
#define TSG_BATCH_EXT_SIZE_V2 ((uint32_t)(offsetof(tsg_batch_ext, gather_src) + sizeof(const uint64_t*)))
#define TSG_BATCH_EXT_SIZE TSG_BATCH_EXT_SIZE_V2  /* what this header's callers set */

int tsg_scan(tsg_scanner* s, const tsg_batch* batch, tsg_result** out);
int tsg_scan_ext(tsg_scanner* s, const tsg_batch_ext* batch, tsg_result** out);
/* Pipelined scanning: tsg_scan on a background thread.  The GPU phases of
 * the scans in flight on one scanner run one after another (one HIP stream);
 * a batch's exact host pass overlaps the next batch's kernels.  The batch's
 * buffers stay borrowed until tsg_scan_wait returns. */
typedef struct tsg_pending tsg_pending;
int tsg_scan_submit(tsg_scanner* s, const tsg_batch* batch, tsg_pending** out);
int tsg_scan_submit_ext(tsg_scanner* s, const tsg_batch_ext* batch, tsg_pending** out);
int tsg_scan_wait(tsg_pending* p, tsg_result** out); /* frees p */
void tsg_result_free(tsg_result* r);

/* kind: 0 = types.Secret{} (no findings), 1 = Secret{FilePath} (allowed path), 2 = findings */
int tsg_result_file(const tsg_result* r, uint32_t file, uint32_t* kind, uint32_t* n_findings);

typedef struct tsg_finding {
  uint32_t rule_index;           /* into tsg_global.rules */
  int64_t start_line, end_line;
  const char* match;
  uint64_t match_len;
  uint32_t n_lines;
} tsg_finding;
int tsg_result_finding(const tsg_result* r, uint32_t file, uint32_t k, tsg_finding* out);

typedef struct tsg_line {
  int64_t number;
  const char* content;
  uint64_t content_len;
  uint8_t is_cause, first_cause, last_cause;
} tsg_line;
int tsg_result_line(const tsg_result* r, uint32_t file, uint32_t k, uint32_t line, tsg_line* out);

/* Compact record of every finding, in file then finding order: the unit a
 * multi-process (one rank per GPU) job gathers to its merging rank, where
 * the findings are put in AnalysisResult.Sort order (pkg/fanal/analyzer/
 * analyzer.go:225-234) by the file paths the caller holds.  digest is a
 * 64-bit FNV-1a over the finding's Match and its Code lines (number, flags,
 * content), so the merged set can be compared without the text.  Returns the
 * record count; writes up to cap of them. */
typedef struct tsg_record {
  uint32_t file, rule_index;
  int64_t start_line, end_line;
  uint64_t digest;
} tsg_record;
uint64_t tsg_result_records(const tsg_result* r, tsg_record* out, uint64_t cap);

/* Whole batch as JSON ([{"kind":..,"findings":[..]}...], Go field names). */
int tsg_result_json(const tsg_result* r, const char** json, uint64_t* len);
/* Files [lo, hi) only (same format; the text stays valid until the next range call on r; the
   whole-result text of tsg_result_json is kept apart). */
int tsg_result_json_range(const tsg_result* r, uint32_t lo, uint32_t hi, const char** json, uint64_t* len);

/* Timings / counters of the batch (GPU ms from HIP events on the engine stream). */
typedef struct tsg_stats {
  uint64_t bytes, files, anchor_hits, candidates, special_files, findings;
  double ms_scan_kernel, ms_verify_kernel, ms_fullscan_kernel, ms_gpu_total;
  double ms_host_gpu_phase, ms_host_allow_path, ms_host_exact, ms_host_total;
  uint64_t flagged_blocks;   /* 16-B blocks the streaming filter sent to its exact confirm step */
  double ms_careful_kernel;  /* fold-rune files' careful pass (part of ms_gpu_total) */
  /* per-kernel split of ms_gpu_total (HIP events on the engine stream) */
  uint64_t follow_hits;      /* anchor_hits (exact anchor-item matches) past the follow requirements */
  double ms_chunkmap_kernel, ms_confirm_kernel, ms_nfa_kernel, ms_finalize_kernel;
  /* host-resident batches: copies + kernels from the first H2D to the last chunk (chunks streamed) */
  double ms_h2d_span;
  uint64_t h2d_chunks;
  uint64_t fullscan_pairs;   /* (file, unanchored rule) pairs with an open keyword gate, NFA-scanned */
  uint64_t fold_sites;       /* U+212A / U+017F / U+0130 occurrences the fold kernel examined */
  double ms_xform_kernel;    /* GPU pre-transform (batch.transform; part of ms_gpu_total) */
} tsg_stats;
int tsg_result_stats(const tsg_result* r, tsg_stats* out);

/* What a device-only batch's scan brought back from HBM for the exact pass
 * (versioned like tsg_batch_ext: the caller sets struct_size, an unknown size
 * is refused; tsg_stats is unversioned and does not grow).  files / bytes: the
 * files that got candidates and their lengths, summed; direct_files: those of
 * them copied straight from the arena, one copy each (files of
 * TSG_FETCH_DIRECT_MB or more, default 8 MiB), the others being packed on the
 * GPU into a staging buffer (TSG_FETCH_STAGE_MB, default 256 MiB) and copied
 * in `rounds` rounds; ms_fetch: the fetch's GPU work and copies.  All zero for
 * a batch with a host arena. */
typedef struct tsg_fetch_stats {
  uint32_t struct_size;
  uint32_t rounds;
  uint64_t files, bytes, direct_files;
  double ms_fetch;
} tsg_fetch_stats;
#define TSG_FETCH_STATS_SIZE_V1 ((uint32_t)(offsetof(tsg_fetch_stats, ms_fetch) + sizeof(double)))
int tsg_result_fetch_stats(const tsg_result* r, tsg_fetch_stats* out);

/* How a device-only batch's bytes come back for the exact pass (versioned: the
 * caller sets struct_size, an unknown size is refused).
 *   TSG_FETCH_FILES (the default)  the files that got candidates, whole;
 *   TSG_FETCH_WINDOWS              the 256-B granules of the arena around each
 *     candidate: back_bytes before its window (default 16, at least 4: the regex
 *     engine looks back one rune), and after it the rule's longest match + 4
 *     where that is bounded and at most fwd_cap (default 4096), else fwd_bytes
 *     (default 1024); a window wider than max_span (default 65536), or a span
 *     that covers its file anyway, brings the whole file.  The exact pass runs
 *     on those bytes and notices when an answer could depend on a byte it was
 *     not given; such a file is then fetched whole (the fallback), so results
 *     never depend on these numbers -- only how much is fetched does.  The
 *     findings' lines are read from the resident arena by the GPU findings pass.
 * A field given as 0 means its default.  Windows apply to untransformed
 * device-only batches (host_arena NULL, dev_arena set, no transform); a batch
 * with a transform scanned in chunks (TSG_RESIDENT_CHUNKED, the default) keeps
 * the files fetch whatever the mode (its transformed bytes are not resident as
 * a whole) and reports mode_used 0; scanned in TSG_RESIDENT_SPLIT mode, the
 * files its transform leaves as read are an untransformed device-only batch
 * and take the windows fetch like one (mode_used 1).  The options take
 * effect with the next submitted scan.  TSG_FETCH_MODE=windows at scanner
 * creation sets the initial mode.  Unknown struct_size, mode > 1 and
 * back_bytes in 1..3 are argument errors (<0, with a text). */
#define TSG_FETCH_FILES 0u
#define TSG_FETCH_WINDOWS 1u
typedef struct tsg_fetch_options {
  uint32_t struct_size;
  uint32_t mode;
  uint32_t back_bytes;
  uint32_t fwd_bytes;
  uint32_t fwd_cap;
  uint32_t max_span;
} tsg_fetch_options;
#define TSG_FETCH_OPTIONS_SIZE_V1 ((uint32_t)(offsetof(tsg_fetch_options, max_span) + sizeof(uint32_t)))
int tsg_scanner_set_fetch_options(tsg_scanner* s, const tsg_fetch_options* opt);
/* The effective values (defaults filled in). */
int tsg_scanner_get_fetch_options(const tsg_scanner* s, tsg_fetch_options* out);

/* What the windows fetch of a scan did.  mode_used: 1 when the batch went the
 * windows route, 0 otherwise (a host arena, a transform scanned in chunks, or the mode off) --
 * the other fields are then zero.  granules / runs: the 256-B granules fetched
 * and the contiguous pieces they form; window_bytes = granules * 256;
 * sparse_files: files answered from their pieces; whole_files: files with
 * candidates whose every byte came back with the windows; fallback_files / fallback_bytes / ms_fallback: files
 * fetched whole afterwards because the pieces did not answer them.
 * tsg_result_fetch_stats then counts, in files, the files of which any byte came
 * back, in bytes everything copied (window_bytes + fallback_bytes), in rounds the
 * staging rounds, in direct_files the fallback files that took the direct route. */
typedef struct tsg_fetch_window_stats {
  uint32_t struct_size;
  uint32_t mode_used;
  uint64_t granules, runs, window_bytes, sparse_files, whole_files, fallback_files, fallback_bytes;
  double ms_fallback;
} tsg_fetch_window_stats;
#define TSG_FETCH_WINDOW_STATS_SIZE_V1 ((uint32_t)(offsetof(tsg_fetch_window_stats, ms_fallback) + sizeof(double)))
int tsg_result_fetch_window_stats(const tsg_result* r, tsg_fetch_window_stats* out);

/* How a resident batch with a transform (dev_arena and transform both set) is scanned.
 *   TSG_RESIDENT_CHUNKED (the default)  every chunk of the arena is copied into the
 *     staging ring, rewritten by the pre-transform and scanned, one chunk after the
 *     other; the candidate files the transform left as read are fetched whole.
 *   TSG_RESIDENT_SPLIT  a census kernel first marks the files the transform really
 *     changes (kind 2, kind 3, and kind 1 with a '\r' in it).  The unmarked files are
 *     scanned where they lie, as an untransformed resident batch that skips the
 *     marked ones: pipelined, and for a device-only batch with the scanner's fetch
 *     mode (files or windows).  The marked files of kind 1 and 2 alone are gathered,
 *     rewritten and scanned as a small second batch.  Results are the same; what
 *     differs is how many bytes are copied, rewritten and fetched
 *     (tsg_result_split_stats).
 * The mode takes effect with the next submitted scan.  TSG_RESIDENT_TRANSFORM=split
 * at scanner creation sets the initial mode.  Another mode is an argument error (<0,
 * with a text). */
#define TSG_RESIDENT_CHUNKED 0u
#define TSG_RESIDENT_SPLIT 1u
int tsg_scanner_set_resident_transform(tsg_scanner* s, uint32_t mode);
int tsg_scanner_get_resident_transform(const tsg_scanner* s, uint32_t* mode);

/* What the split scan did (versioned: the caller sets struct_size, an unknown size
 * is refused before anything else is read or written).  mode_used: 1 when the batch
 * took the split, else 0 and every other field 0 (no transform, no dev_arena, an
 * empty batch, or the mode off).  files / bytes_in_place: the files scanned where
 * they lie; _changed: the files of the second batch; _dropped: the kind-3 files.
 * ms_census: the census kernels (HIP events); ms_sub: the second batch's scan, wall
 * time, beside the in-place scan's kernels (0 when no file changed). */
typedef struct tsg_split_stats {
  uint32_t struct_size;
  uint32_t mode_used;
  uint64_t files_in_place, bytes_in_place, files_changed, bytes_changed, files_dropped, bytes_dropped;
  double ms_census, ms_sub;
} tsg_split_stats;
#define TSG_SPLIT_STATS_SIZE_V1 ((uint32_t)(offsetof(tsg_split_stats, ms_sub) + sizeof(double)))
int tsg_result_split_stats(const tsg_result* r, tsg_split_stats* out);

/* Page-lock a caller's host buffer (hipHostRegister) so batches in it stream
 * to the GPU asynchronously (the engine's staging ring: copies of this and of
 * the next submitted batches overlap the kernels): the Go caller's pinned arena
 * pool.  Unregister before freeing it. */
int tsg_host_register(void* p, uint64_t bytes);
/* The same, also mapped into the device's address space, so kernels read it
 * directly (tsg_batch_ext.gather_base: a tar layer the GPU gathers from). */
int tsg_host_register_mapped(void* p, uint64_t bytes);
int tsg_host_unregister(void* p);

/* Compiled-table facts (for reports/tests). */
typedef struct tsg_table_info {
  uint32_t n_rules, n_keywords, n_anchors, n_filter_items, n_filter_buckets, filter_window;
  uint32_t n_fullscan_rules, nfa_words_total;
  uint64_t filter_table_bytes;  /* reach + item + class + core tables */
  double filter_est_fp;         /* estimated bucket fires per input byte (static byte prior) */
} tsg_table_info;
int tsg_scanner_table_info(const tsg_scanner* s, tsg_table_info* out);
/* Anchor description of rule i ("[lo,hi] lit lit..." or "-"). */
const char* tsg_scanner_rule_anchor(const tsg_scanner* s, uint32_t i);

#ifdef __cplusplus
}
#endif
#endif
