/* libtsg.so -- the secret analyzer's ingest side, C ABI (cgo / ctypes bindable).
 *
 * Replaces the per-file half of pkg/fanal/analyzer/secret (undistro/trivy @
 * 2024-12-20) that runs before Scanner.Scan, and the analyzer group's
 * goroutine-per-file fan-out for this analyzer, with a batch collector that
 * packs transformed contents straight into one (pinned) arena for tsg_scan:
 *
 * Entry point                  replaces (reference)
 *   tsg_is_binary              utils.IsBinary                      pkg/fanal/utils/utils.go:85-103
 *   tsg_extract_printable      utils.ExtractPrintableBytes         pkg/fanal/utils/utils.go:128-160
 *   tsg_strip_cr               bytes.ReplaceAll(content, "\r", "") pkg/fanal/analyzer/secret/secret.go:121
 *   tsg_analyzer_new           NewSecretAnalyzer + Init            secret.go:79-101
 *   tsg_analyzer_required      (*SecretAnalyzer).Required          secret.go:152-190
 *   tsg_collector_add          (*SecretAnalyzer).Analyze up to the secret.go:103-136
 *                              Scan call (binary gate, transform,
 *                              "/" prefix for image files)
 *   tsg_collector_submit       the Scan calls of a batch           secret.go:137-141 -> scanner.go:377
 *   tsg_collector_add_tar      LayerTar.Walk + AnalyzeFile's       pkg/fanal/walker/tar.go:35-103,
 *                              Required gate for this analyzer     pkg/fanal/analyzer/analyzer.go:403-455
 *   tsg_analyzer_set_tar_skip  NewLayerTar's skipFiles / skipDirs  pkg/fanal/walker/tar.go:23-33, 64-81, 105-116
 *
 * Results: tsg_scan_wait gives a tsg_result whose file i is the collector's
 * i-th added file; Analyze returns nil unless that file's kind is 2 (findings),
 * secret.go:143-149.  Conventions as in tsg_scanner.h (0 = OK, <0 = error,
 * text via tsg_last_error()).
 */
#ifndef TSG_ANALYZER_H
#define TSG_ANALYZER_H
#include <stdint.h>

#include "tsg_scanner.h"
#ifdef __cplusplus
extern "C" {
#endif

/* utils.IsBinary over the first min(size, 300) bytes of content: 1 = binary. */
int tsg_is_binary(const uint8_t* content, uint64_t size);
/* utils.ExtractPrintableBytes: runs of unicode.IsPrint bytes longer than 4, each
 * followed by '\n'.  out must hold n + n / 5 + 1 bytes; returns the length. */
uint64_t tsg_extract_printable(const uint8_t* in, uint64_t n, uint8_t* out);
/* every '\r' removed; out must hold n bytes (may equal in); returns the length. */
uint64_t tsg_strip_cr(const uint8_t* in, uint64_t n, uint8_t* out);

typedef struct tsg_analyzer tsg_analyzer;
/* The scanner is borrowed for the analyzer's lifetime; config_path is the
 * SecretScannerOption.ConfigPath given to Init ("" = builtin rules). */
int tsg_analyzer_new(const tsg_scanner* s, const char* config_path, tsg_analyzer** out);
void tsg_analyzer_free(tsg_analyzer* a);
/* Required(filePath, fi) with fi.Size() = size: 1 = analyze, 0 = skip. */
int tsg_analyzer_required(const tsg_analyzer* a, const char* path, uint64_t path_len, int64_t size);

typedef struct tsg_collector tsg_collector;
/* A batch of at most arena_bytes transformed bytes (a single larger file is
 * accepted alone); the arena is pinned host memory when the scanner has a GPU. */
int tsg_collector_new(tsg_analyzer* a, uint64_t arena_bytes, tsg_collector** out);
void tsg_collector_free(tsg_collector* c);

#define TSG_SKIPPED (-1) /* binary and not .pyc: Analyze returns nil without scanning */
#define TSG_FULL (-2)    /* the batch is full: submit (or reset) and add again */
/* Analyze's pre-scan half for one file (dir = AnalysisInput.Dir; "" means a
 * file extracted from an image, whose path gets the "/" prefix).  Returns the
 * file's index in the batch (>= 0), TSG_SKIPPED or TSG_FULL; -3 (error set)
 * when the arena cannot grow or the collector gathers (tsg_collector_set_gather). */
int64_t tsg_collector_add(tsg_collector* c, const char* path, uint64_t path_len, const char* dir,
                          const uint8_t* content, uint64_t size);

typedef struct tsg_tar_stats {
  uint64_t entries, regular, required, added, skipped_binary, whiteouts, opaque_dirs, input_bytes;
} tsg_tar_stats;
/* Walk an uncompressed tar layer held in memory from *cursor (a header
 * offset; 0 to start): every regular file that Required accepts is added as
 * an image file (Dir "").  Returns 0 at the end of the archive, 1 when the
 * batch filled up (*cursor = the entry to resume from), <0 on a malformed
 * archive.  Whiteout (.wh.) and opaque-dir entries are counted, not added. */
int tsg_collector_add_tar(tsg_collector* c, const uint8_t* tar, uint64_t n, uint64_t* cursor, tsg_tar_stats* st);
/* Walk-ahead (opt-in, off by default): with tsg_analyzer_set_walk_ahead(a, 1)
 * the analyzer indexes the next window of entries on a background thread after
 * tsg_collector_add_tar returns 1.  Buffer lifetime in that mode: `tar` must
 * stay valid and unchanged until the walk ends -- add_tar returned 0 (end of
 * the archive) or < 0 -- or until tsg_analyzer_walk_end / tsg_analyzer_free /
 * tsg_analyzer_set_walk_ahead(a, 0) returns (call one before freeing the
 * buffer of a walk abandoned midway).  With walk-ahead off, nothing reads
 * `tar` after add_tar returns.  tsg_analyzer_walk_end also drops the walk's
 * cached window, so a later buffer at the same address starts afresh. */
int tsg_analyzer_set_walk_ahead(tsg_analyzer* a, int on);
int tsg_analyzer_walk_end(tsg_analyzer* a);

/* LayerTar's options (walker/tar.go:23-33): skip_dirs / skip_files as utils.SkipPath
 * doublestar patterns, already cleaned (the caller applies utils.CleanSkipPaths as
 * NewLayerTar does; the division of labour of tsg_fs_walk_new).  They hold for every
 * layer walk of this analyzer made afterwards: tsg_collector_add_tar in copy and in
 * gather mode, tsg_analyzer_index_device_tar in both walk modes.  Per entry, in
 * chain order and on the cleaned path without leading '/' (tar.go:46-81): whiteout
 * and opaque markers are counted first, as without options; a directory (typeflag
 * '5', or '\0' with a resolved name that ends in '/') that skip_dirs matches is
 * recorded and dropped; a regular file that skip_files matches is dropped; a file
 * that survives is dropped when underSkippedDir holds against the directories
 * recorded so far (filepath.Rel: below one, equal to one, or the direct parent of
 * one; a Rel failure ends the test with false).  The test depends on the order of
 * the archive: a file before its directory's entry is kept.  A skipped subtree of a
 * resident layer lies in the gaps between the index's files and is dropped where it
 * lies.  tsg_tar_stats.regular still counts every regular entry; .required only
 * those not skipped that Required accepts.
 * The call ends the tar walk in progress (as tsg_analyzer_walk_end) and drops its
 * cached window, and resets the analyzer's skip counts; zero patterns restore the
 * walk without options.  A walk resumed by cursor continues its list of recorded
 * directories when the cursor continues the walk in progress on the same buffer
 * (it is where the last call stopped, or lies inside what that walk has read);
 * cursor 0 starts a fresh list, and any other cursor -- another buffer, a position
 * past what was read, a walk ended by tsg_analyzer_walk_end -- starts with an
 * empty one.  Index calls running on other threads keep the options they began with.
 * -1 (before any work): NULL analyzer, a NULL array with a non-zero count, a NULL
 * pattern.  A malformed pattern is no error: SkipPath stops at it with false. */
int tsg_analyzer_set_tar_skip(tsg_analyzer* a, const char* const* skip_dirs, uint32_t n_dirs,
                              const char* const* skip_files, uint32_t n_files);
/* How many patterns are set. */
int tsg_analyzer_get_tar_skip(const tsg_analyzer* a, uint32_t* n_dirs, uint32_t* n_files);

/* What the options dropped (versioned, struct_size first): skipped_dirs, directory
 * entries recorded; skipped_files, regular files skip_files matched;
 * under_skipped_dir, regular files (only) dropped by underSkippedDir. */
typedef struct tsg_tar_skip_stats {
  uint32_t struct_size, reserved;
  uint64_t skipped_dirs, skipped_files, under_skipped_dir;
} tsg_tar_skip_stats;
#define TSG_TAR_SKIP_STATS_SIZE_V1 ((uint32_t)(offsetof(tsg_tar_skip_stats, under_skipped_dir) + sizeof(uint64_t)))
/* The host walks (tsg_collector_add_tar) of this analyzer, cumulative since the last
 * tsg_analyzer_set_tar_skip; an entry counts when a batch takes it or passes it.
 * -1: NULL argument or an unknown struct_size. */
int tsg_analyzer_tar_skip_stats(tsg_analyzer* a, tsg_tar_skip_stats* out);

/* GPU pre-transform mode (empty collector only): files go into the arena as
 * read, and the CR strip / printable extraction runs on the GPU at scan time
 * (tsg_batch.transform).  The batch limit then counts each file's largest
 * transformed size. */
int tsg_collector_set_gpu_transform(tsg_collector* c, int on);
/* Gather mode (round 6; GPU-transform collectors, tar walks only): the walk no
 * longer copies a file's bytes into the arena -- the batch records where the
 * layer holds them, and the GPU gathers them from the layer buffer itself
 * (tsg_batch_ext v2 gather_base / gather_src).  The layer buffer must be
 * page-locked and device-mapped (tsg_host_register_mapped) for the whole walk
 * and until the batch's tsg_scan_wait.  A batch holds one layer's files: a
 * tsg_collector_add_tar on another buffer returns 1 (full) while the batch is
 * not empty.  tsg_collector_add / _add_fs fail in this mode. */
int tsg_collector_set_gather(tsg_collector* c, int on);

/* FS.Walk (pkg/fanal/walker/fs.go:25-78) feeding a collector: the tree under
 * root in filepath.WalkDir order, skip_dirs / skip_files as utils.SkipPath
 * doublestar patterns relative to root (the caller applies BuildSkipPaths,
 * fs.go:102-155; defaultSkipDirs are added here), regular files only,
 * permission errors ignored; per file AnalyzeFile's Required and Analyze up
 * to Scan (binary gate, contents read into the batch arena; FilePath = the
 * path relative to root, Dir = root).  tsg_collector_add_fs returns 1 when the
 * collector is full (submit, reset, call again), 0 when the walk is done,
 * <0 on error (tsg_last_error). */
typedef struct tsg_fs_walk tsg_fs_walk;
typedef struct tsg_fs_stats {
  uint64_t files, dirs, skipped_dirs, skipped_files, nonregular, perm_errors;
} tsg_fs_stats;
typedef struct tsg_fs_add_stats {
  uint64_t walked, required, skipped_binary, added, input_bytes;
} tsg_fs_add_stats;
int tsg_fs_walk_new(const char* root, const char* const* skip_dirs, uint32_t n_skip_dirs,
                    const char* const* skip_files, uint32_t n_skip_files, tsg_fs_walk** out);
int tsg_collector_add_fs(tsg_collector* c, tsg_fs_walk* w, tsg_fs_add_stats* st);
int tsg_fs_walk_stats(const tsg_fs_walk* w, tsg_fs_stats* st);
void tsg_fs_walk_free(tsg_fs_walk* w);
/* utils.SkipPath's doublestar.Match: 1 match, 0 no match, -1 malformed pattern. */
int tsg_doublestar_match(const char* pattern, const char* path);
uint32_t tsg_collector_files(const tsg_collector* c);
uint64_t tsg_collector_bytes(const tsg_collector* c);       /* arena bytes (transformed; as read in GPU mode) */
uint64_t tsg_collector_input_bytes(const tsg_collector* c); /* bytes as read, added files only */
/* The ScanArgs of file i as they will be scanned (tests / host-language mirror). */
int tsg_collector_file(const tsg_collector* c, uint32_t i, const char** path, uint64_t* path_len,
                       const uint8_t** content, uint64_t* len, int* binary);
/* Scan the batch (tsg_scan_submit); the arena stays borrowed until tsg_scan_wait.
 * Reset the collector after the wait to reuse it. */
int tsg_collector_submit(tsg_collector* c, tsg_pending** out);
void tsg_collector_reset(tsg_collector* c);

/* Analyze for files whose bytes exist only in HBM (secret.go:103-150): the
 * caller holds the bytes as read in a resident arena, and the paths and sizes
 * on the host.  Required (path, size) runs on the host; the binary gate --
 * utils.IsBinary over each file's first min(size, 300) bytes -- runs on the GPU
 * over the arena (trivy_amd/csrc/classify.hip), and only the n_files flags
 * come back.  Versioned like tsg_batch_ext: struct_size first, an unknown size
 * is refused.  `paths` are AnalysisInput.FilePath (no "/" prefix); the library
 * adds the prefix for the scan when dir is "" or NULL (a file extracted from an
 * image, secret.go:130-135).  dev_arena follows the tsg_batch.dev_arena
 * contract: 16-B aligned, 64 readable bytes past host_offsets[n_files]. */
typedef struct tsg_device_files {
  uint32_t struct_size, n_files;
  const void* dev_arena;         /* the bytes as read, resident */
  const uint64_t* host_offsets;  /* n_files + 1, ascending from 0 */
  const void* dev_offsets;       /* optional: device copy of host_offsets */
  const char* const* paths;      /* AnalysisInput.FilePath per file */
  const uint64_t* path_lens;     /* optional */
  const char* dir;               /* AnalysisInput.Dir; "" / NULL = image file */
} tsg_device_files;
#define TSG_DEVICE_FILES_SIZE_V1 ((uint32_t)(offsetof(tsg_device_files, dir) + sizeof(const char*)))

/* ms_kernel: classify_heads_kernel alone (HIP events); ms_total: the whole
 * classify call -- offsets upload, kernel, flags read-back, the host's
 * Required pass and the gate.  required: files Required accepted;
 * skipped_binary: of those, binary and not .pyc (dropped); pyc: binary .pyc. */
typedef struct tsg_device_classify_stats {
  uint32_t struct_size, reserved;
  uint64_t files, required, skipped_binary, pyc;
  double ms_kernel, ms_total;
} tsg_device_classify_stats;
#define TSG_DEVICE_CLASSIFY_STATS_SIZE_V1 \
  ((uint32_t)(offsetof(tsg_device_classify_stats, ms_total) + sizeof(double)))

/* Per file: kind_out = the tsg_batch.transform value -- 3 (dropped) when
 * Required refuses the file or it is binary and not .pyc, 2 for a binary .pyc
 * (binary_out 1, ScanArgs.Binary), else 1 (binary_out 0).  st is optional.
 * Argument errors (unknown struct_size; NULL dev_arena, host_offsets or paths;
 * dev_arena not 16-B aligned; offsets not ascending from 0) return <0 before
 * any GPU work.  The classify pass runs on a stream of its own and does not
 * take the scanner's GPU lock. */
int tsg_analyzer_classify_device(tsg_analyzer* a, const tsg_device_files* f, uint8_t* kind_out, uint8_t* binary_out,
                                 tsg_device_classify_stats* st);
/* Classify, then tsg_scan_submit of the device-only batch (host_arena NULL)
 * with the computed transform and binary flags and the scan paths.  The same
 * argument errors, returned here; everything after them runs on the pending's
 * thread, so several submits may be in flight.  The library owns what it built
 * (kinds, flags, path strings) until tsg_scan_wait returns; the caller's
 * buffers -- the struct's arrays, not the struct -- stay borrowed until then.
 * Result file i is the caller's file i; Analyze's nil is a file whose result
 * kind is not 2. */
int tsg_analyzer_submit_device(tsg_analyzer* a, const tsg_device_files* f, tsg_pending** out);

/* An uncompressed tar layer whose bytes exist only in HBM.  Where
 * the files are is written in the 512-B headers inside the bytes: one streaming
 * GPU pass (trivy_amd/csrc/tarindex.hip) collects every block that parses as a
 * header -- the checksum test of the host walk -- and only those come to the
 * host, which follows the header chain over them by the rules of
 * tsg_collector_add_tar (PAX path / size, GNU long names, ustar prefix,
 * path.Clean, whiteouts, opaque dirs, Required).  File data that looks like a
 * header (a tar inside the layer) is never on the chain and never visited.
 * Contract: dev_tar is 16-B aligned; 64 readable bytes follow dev_tar + n_bytes
 * (the dev_arena contract: only the scan kernels use it, the index pass reads
 * complete 512-B blocks below n_bytes alone); the layer stays valid and
 * unchanged until the index is freed and every pending made from it is waited
 * for.  Versioned like tsg_device_files. */
typedef struct tsg_device_tar {
  uint32_t struct_size, reserved;
  const void* dev_tar;
  uint64_t n_bytes;
} tsg_device_tar;
#define TSG_DEVICE_TAR_SIZE_V1 ((uint32_t)(offsetof(tsg_device_tar, n_bytes) + sizeof(uint64_t)))

/* tar: entries, regular, required, whiteouts, opaque_dirs as the host walk counts
 * them (added, skipped_binary and input_bytes are 0: the index does not read file
 * contents).  blocks: complete 512-B blocks read; candidates: blocks that parse
 * as a header; off_chain: candidates the chain never visited; block_fetches:
 * chain blocks that were no candidate (the end-of-archive block, a corrupted
 * header), each copied from the device on its own; ext_bytes: bytes of PAX
 * records and GNU long names copied from the device; kernel_runs: 2 when the
 * record buffer (n_bytes / 4096 + 1024 records at first) was too small and the
 * pass ran again with room for the count.  ms_kernel: the kernel run(s), HIP
 * events; ms_total: the whole call. */
typedef struct tsg_device_tar_stats {
  uint32_t struct_size, reserved;
  tsg_tar_stats tar;
  uint64_t blocks, candidates, off_chain, block_fetches, ext_bytes, kernel_runs;
  double ms_kernel, ms_total;
} tsg_device_tar_stats;
#define TSG_DEVICE_TAR_STATS_SIZE_V1 ((uint32_t)(offsetof(tsg_device_tar_stats, ms_total) + sizeof(double)))

typedef struct tsg_tar_index tsg_tar_index;
/* The index of a resident layer: its Required-accepted regular files in walk
 * order.  st is optional.  Argument errors -- unknown struct_size (of t or st),
 * NULL analyzer, t, out or dev_tar, dev_tar not 16-B aligned, n_bytes / 512 >=
 * 2^32 -- return -1 before any GPU work; -2: no GPU engine, or a HIP error (also
 * one in a copy the walk asked for); a malformed archive returns -3 with the host
 * walk's message.  The record buffers of the pass (about 13 % of the layer's size
 * in HBM and as much page-locked host memory, while the call runs) are freed before
 * it returns when they exceed 16 MiB.  The pass runs on
 * a stream of its own and does not take the scanner's GPU lock. */
int tsg_analyzer_index_device_tar(tsg_analyzer* a, const tsg_device_tar* t, tsg_tar_index** out,
                                  tsg_device_tar_stats* st);
uint32_t tsg_tar_index_files(const tsg_tar_index* ix);
/* File i: its cleaned path (no "/" prefix; NUL-terminated, owned by the index),
 * where its content lies in the layer, and its size.  -1: i out of range. */
int tsg_tar_index_file(const tsg_tar_index* ix, uint32_t i, const char** path, uint64_t* path_len,
                       uint64_t* data_off, uint64_t* size);
/* Every file's layout at once (tsg_tar_index_files values each; any may be NULL):
 * start, the 512-B boundary where the entry's header chain begins (its PAX / GNU
 * long-name headers lie there, before its own header) -- where a batch that begins
 * with this file has its arena; data_off and size as tsg_tar_index_file gives them. */
int tsg_tar_index_spans(const tsg_tar_index* ix, uint64_t* start, uint64_t* data_off, uint64_t* size);
/* Files [first, first + count) as one device-only batch with no copy: the layer
 * itself is the arena, from the 512-B boundary where file `first`'s header chain
 * starts.  The batch has 2 count + 1 pseudo-files, gap, file, gap, ..., file,
 * gap: a gap is what lies between two files (headers, padding, every entry
 * Required refused), has an empty path and is dropped where it lies (transform
 * kind 3).  IsBinary runs on the GPU over the files' heads, then the batch is
 * scanned as tsg_analyzer_submit_device scans its own: a binary .pyc is kind 2,
 * any other binary is dropped.  The scanner's fetch mode and resident-transform
 * mode apply unchanged.
 * Result indexing: result file 2 j + 1 is index file first + j; the even results
 * are the gaps, kind 0.  first + count beyond tsg_tar_index_files is refused (-1)
 * before any GPU work.  The library owns what it built until tsg_scan_wait;
 * several submits may be in flight. */
int tsg_analyzer_submit_device_tar(tsg_analyzer* a, const tsg_tar_index* ix, uint32_t first, uint32_t count,
                                   tsg_pending** out);
void tsg_tar_index_free(tsg_tar_index* ix);

/* Where the header chain of tsg_analyzer_index_device_tar is walked.  Mode 0,
 * host (the default): the GPU collects the candidate records and the host walks
 * the chain over them, as described above.  Mode 1, gpu (opt-in): the candidates
 * stay in HBM as one bit per block, the GPU reads every candidate as an entry
 * start, marks the entries the chain from block 0 visits and writes one 64-B
 * record and the raw name per entry, in walk order (trivy_amd/csrc/tarchain.hip);
 * the host copies those two buffers, cleans and classifies the names and runs
 * Required on its threads.  The index, the tar stats, the return code and the
 * error text are those of mode 0 for any bytes: a layer the GPU walk does not
 * complete -- a malformed archive, a PAX size that is not plain digits, PAX or
 * long-name data above 64 KiB, more than 16 extension headers before one entry
 * -- is indexed again from scratch by mode 0 (tsg_tar_walk_stats.fallback says
 * why).  In mode 1 the stats of tsg_device_tar_stats mean: candidates, the
 * candidate blocks; off_chain, those not on the chain; block_fetches and
 * ext_bytes, what the host copied block by block (0 on a layer the GPU
 * completes); kernel_runs 1; ms_kernel the sum of the pass's kernels.  The pass
 * allocates about 20 B per 512-B block in HBM (4 % of the layer) while it runs,
 * plus the records and names; no page-locked memory beyond those two.
 * Takes effect with the next index call.  TSG_TAR_WALK=gpu (or host) in the
 * environment sets the initial mode of analyzers made afterwards.  -1: NULL
 * analyzer or a mode above 1. */
int tsg_analyzer_set_tar_walk(tsg_analyzer* a, int mode);
int tsg_analyzer_get_tar_walk(const tsg_analyzer* a, int* mode);

/* How an index was made (versioned, struct_size first).  walk: the mode in force
 * for the call; fallback: 0, or why the GPU walk's result was discarded and mode
 * 0 ran (1 a size field, 2 a PAX record, 3 the form of a PAX size, 4 a cap, 5 a
 * chain block that is no header candidate, 6 truncation, 7 a layer of 2^31 or
 * more blocks); chain_entries, name_bytes: what the GPU walk handed over;
 * segments: of the marking pass; device_bytes: the most HBM the pass held at one
 * time.  ms_candidates, ms_entries, ms_mark, ms_compact: the kernels by stage
 * (HIP events); ms_copy: the records and names to the host; ms_host: clean,
 * classify, Required and the index.  All zero but walk for a mode-0 index. */
typedef struct tsg_tar_walk_stats {
  uint32_t struct_size, reserved;
  uint32_t walk, fallback;
  uint64_t chain_entries, name_bytes, segments, device_bytes;
  double ms_candidates, ms_entries, ms_mark, ms_compact, ms_copy, ms_host;
} tsg_tar_walk_stats;
#define TSG_TAR_WALK_STATS_SIZE_V1 ((uint32_t)(offsetof(tsg_tar_walk_stats, ms_host) + sizeof(double)))
/* -1: NULL argument or an unknown struct_size. */
int tsg_tar_index_walk_stats(const tsg_tar_index* ix, tsg_tar_walk_stats* out);
/* What tsg_analyzer_set_tar_skip's options dropped from this index (all zero without
 * options).  -1: NULL argument or an unknown struct_size. */
int tsg_tar_index_skip_stats(const tsg_tar_index* ix, tsg_tar_skip_stats* out);

/* Where the path work and Required of a resident layer's index run.
 * Mode 0, host (the default): as described above.  Mode 1, gpu (opt-in): behind the
 * GPU walk's compaction a device stage (trivy_amd/csrc/tarrequired.hip) decides per
 * entry what the host's clean-and-classify followed by Required decide, and hands
 * over only the files Required keeps -- 48-B records and their cleaned paths, laid
 * out as the index stores them -- plus the entries it leaves to the host: files
 * whose path holds a literal of an allow-path rule (the exact rules run on those),
 * and names that need more of path.Clean than a "./" or "/" prefix and trailing
 * slashes.  The index, the stats and the results are those of mode 0 for any bytes.
 * Applies to tsg_analyzer_index_device_tar and tsg_analyzer_index_device_tars, and is
 * in force only when the walk mode is 1, no tsg_analyzer_set_tar_skip options are set
 * and the GPU walk completed the layer; otherwise the host half of the walk mode in
 * force runs, and tsg_tar_required_stats.reason says why -- that is no error.
 * Takes effect with the next index call.  TSG_TAR_REQUIRED=gpu (or host) in the
 * environment sets the initial mode of analyzers made afterwards.  -1: NULL analyzer
 * or another mode (the text names it). */
int tsg_analyzer_set_tar_required(tsg_analyzer* a, int mode);
int tsg_analyzer_get_tar_required(const tsg_analyzer* a, int* mode);

/* How an index's Required ran (versioned, struct_size first).  mode: the one in force
 * for this index (1: the device stage ran); reason, when it is 0: 1 the setter is off,
 * 2 walk mode 0, 3 skip options are set, 4 the GPU walk did not complete the layer,
 * 5 (only with tsg_analyzer_set_tar_required_skip mode 1) a name the device does not
 * clean was a skipped directory (reason 0: the stage ran).  Of the layer's `entries` the device kept `kept` files,
 * dropped `dropped` by Required, and asked the host about `ask_allow` (the exact allow
 * rules) and `ask_name` (clean, classify, Required); ask_dropped: asked entries the
 * host then dropped; path_bytes: the path blob handed over.  ms_kernel: the stage (HIP
 * events; shared by the layers of one tsg_analyzer_index_device_tars pass, as ms_copy
 * is); ms_copy: the file records and paths to the host; ms_host: the host half. */
typedef struct tsg_tar_required_stats {
  uint32_t struct_size, reserved;
  uint32_t mode, reason;
  uint64_t entries, kept, dropped, ask_allow, ask_name, ask_dropped, path_bytes;
  double ms_kernel, ms_copy, ms_host;
} tsg_tar_required_stats;
#define TSG_TAR_REQUIRED_STATS_SIZE_V1 ((uint32_t)(offsetof(tsg_tar_required_stats, ms_host) + sizeof(double)))
/* -1: NULL argument or an unknown struct_size. */
int tsg_tar_index_required_stats(const tsg_tar_index* ix, tsg_tar_required_stats* out);

/* LayerTar's skip options in that device stage.  Mode 0, host (the
 * default): with tsg_analyzer_set_tar_skip options set the stage gives way to the host
 * half (tsg_tar_required_stats.reason 3), as described above.  Mode 1, gpu (opt-in):
 * the stage honours the options itself when every pattern, as tsg_analyzer_set_tar_skip
 * received it, has one of four forms -- "L" (the path equals L), "**" "/L" (the path
 * is L or ends with "/" + L), "L/" "**" (the path is L or begins with L + "/"),
 * "**" "/" "*S" (the base name ends with S) -- with L a non-empty ASCII literal of at most
 * 255 bytes without * ? [ ] { } \ and without an empty, "." or ".." element, S such a
 * literal without '/'; at most 32 directory patterns, 32 file patterns and 2 KiB of
 * literals.  Three more kernels then mark the directories a pattern matches, the
 * regular files a pattern matches, and the regular files that lie under a directory
 * recorded earlier in the same layer (tar.go's underSkippedDir); the index holds only
 * what survives skip-files, under-skipped-dir and Required, and the index, the stats
 * and the results are those of the host half with the same options.  In force when
 * tsg_analyzer_set_tar_required is 1, the walk mode is 1, the GPU walk completed the
 * layer, options are set and every pattern is taken; with any other pattern the whole
 * option set goes to the host half (reason 3 stays).  A layer in which a name the
 * device does not clean is a skipped directory is indexed by the host half alone
 * (tsg_tar_required_stats.reason 5).  Without options the switch has no effect.
 * TSG_TAR_REQUIRED_SKIP=gpu (or host) in the environment sets the initial mode of
 * analyzers made afterwards.  -1: NULL analyzer or another mode (the text names it). */
int tsg_analyzer_set_tar_required_skip(tsg_analyzer* a, int mode);
int tsg_analyzer_get_tar_required_skip(const tsg_analyzer* a, int* mode);

/* How an index's skip options were honoured (versioned, struct_size first).  mode: the
 * switch when the index was made; reason: 0 the device stage honoured them, 1 the
 * switch is off, 2 no options are set, 3 a pattern (or the set) is outside what the
 * device takes, 4 the Required stage did not run (tsg_tar_required_stats.reason says
 * why), 5 a name the device does not clean was a skipped directory: the host half
 * indexed the layer.  dir_patterns, file_patterns: the options; skipped_dirs,
 * skipped_files, under_skipped_dir: tsg_tar_index_skip_stats' counts, whichever half
 * produced them; table_slots: the 16-B slots of the recorded directories' table (0:
 * no directory was recorded, two kernels did not run); ms_kernel: the stage's three
 * kernels (HIP events; shared by the layers of one tsg_analyzer_index_device_tars
 * pass, as table_slots is). */
typedef struct tsg_tar_required_skip_stats {
  uint32_t struct_size, reserved;
  uint32_t mode, reason;
  uint32_t dir_patterns, file_patterns;
  uint64_t skipped_dirs, skipped_files, under_skipped_dir, table_slots;
  double ms_kernel;
} tsg_tar_required_skip_stats;
#define TSG_TAR_REQUIRED_SKIP_STATS_SIZE_V1 \
  ((uint32_t)(offsetof(tsg_tar_required_skip_stats, ms_kernel) + sizeof(double)))
/* -1: NULL argument or an unknown struct_size. */
int tsg_tar_index_required_skip_stats(const tsg_tar_index* ix, tsg_tar_required_skip_stats* out);

/* All layers of an image resident in HBM, indexed by one call.  The
 * layers may be separate allocations or 512-B-aligned ranges of one buffer (as inside
 * a `docker save` archive); each obeys tsg_device_tar's contract on its own: only the
 * complete blocks below its n_bytes are read by the index, and the 64 readable bytes
 * past a range's end are whatever follows it in the buffer.  Versioned like
 * tsg_device_files. */
typedef struct tsg_device_tars {
  uint32_t struct_size, n_layers;
  const tsg_device_tar* layers; /* n_layers of them, each v1 */
} tsg_device_tars;
#define TSG_DEVICE_TARS_SIZE_V1 ((uint32_t)(offsetof(tsg_device_tars, layers) + sizeof(const tsg_device_tar*)))
#define TSG_DEVICE_TARS_MAX_LAYERS 65536u

/* layers: of the call; batched: layers whose index came from a forest pass; fallbacks:
 * layers a pass left INCOMPLETE (or too large for one) and mode 0 indexed again;
 * passes: forest passes run (more than one when the layers' virtual block space --
 * each layer's blocks rounded up to whole segments -- exceeds 2^31 blocks);
 * virtual_blocks, segments: summed over the passes; device_bytes: the most HBM the
 * call held at one time.  ms_candidates .. ms_compact: the kernels by stage and ms_copy
 * the records and names to the host (HIP events); ms_host: clean, classify, Required
 * and the indexes of all layers (wall); ms_total: the whole call.  All zero but layers
 * and ms_total in walk mode 0. */
typedef struct tsg_tar_forest_stats {
  uint32_t struct_size, reserved;
  uint64_t layers, batched, fallbacks, passes, virtual_blocks, segments, device_bytes;
  double ms_candidates, ms_entries, ms_mark, ms_compact, ms_copy, ms_host, ms_total;
} tsg_tar_forest_stats;
#define TSG_TAR_FOREST_STATS_SIZE_V1 ((uint32_t)(offsetof(tsg_tar_forest_stats, ms_total) + sizeof(double)))

/* out[k] (n_layers pointers) becomes what tsg_analyzer_index_device_tar gives for
 * layer k alone in the analyzer's walk mode and with its tar-skip options: the files,
 * the spans, st[k].tar and the skip stats; each index is independent, is freed with
 * tsg_tar_index_free and is submitted with tsg_analyzer_submit_device_tar.  st
 * (optional): n_layers stats, each with its struct_size set; for a layer indexed by a
 * forest pass kernel_runs is 1, ms_kernel 0 (the kernels are shared: fs) and ms_total
 * that layer's host half.  fs, bad_layer: optional.
 * Walk mode 1: the header chains of all layers are walked by one GPU pass
 * (trivy_amd/csrc/tarforest.hip) on one stream with one work buffer, one copy of the
 * heads, one of all records and one of all names; the host half then runs per layer,
 * the layers in parallel.  A layer the pass does not complete is indexed again by mode
 * 0, alone (its tsg_tar_walk_stats.fallback says why); the others keep their batched
 * result.  For a batched index tsg_tar_index_walk_stats carries walk, fallback,
 * chain_entries, name_bytes and segments of that layer; the stage times are shared and
 * live in fs.  Walk mode 0: the layers are indexed one after another by the
 * single-layer path.
 * Argument errors return -1 before any GPU work, a layer's with "layer k: " before the
 * single-layer call's text: a NULL argument, an unknown struct_size (of t, of a layer,
 * of a st[k], of fs), n_layers 0 or above TSG_DEVICE_TARS_MAX_LAYERS, a NULL or
 * misaligned dev_tar, a layer of 2^32 or more blocks.  -3: a malformed layer -- the
 * first one, lowest index -- with the host walk's message after "layer k: ", *bad_layer
 * set; -2: no GPU engine, or a HIP error (one met in a layer's own single-layer pass has
 * "layer k: " before its text; *bad_layer is written for -3 alone).  On any error every index made is freed and
 * out[] is all NULL.  Work buffers above 16 MiB are freed before the call returns:
 * once per image. */
int tsg_analyzer_index_device_tars(tsg_analyzer* a, const tsg_device_tars* t, tsg_tar_index** out,
                                   tsg_device_tar_stats* st, tsg_tar_forest_stats* fs, uint32_t* bad_layer);

#ifdef __cplusplus
}
#endif
#endif
