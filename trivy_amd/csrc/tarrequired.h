// Path classify and Required of a resident tar layer's entries on the GPU
// (tarrequired.hip; opt-in tsg_analyzer_set_tar_required mode 1, beside walk mode 1).
// This header is plain C++: what the device stage reads, what it decides, and what it
// hands to the host half (tar_required_host.h: IndexTarFiles).  The launcher is declared
// in tarindex.h.
//
// Input: what TarChainCompact / TarForestCompact wrote -- n tsg_tar_entry_rec in walk
// order, the name blob, and a table of (record base, name base) per layer, n_layers + 1
// rows, the last one (n, name_bytes).  A record's name_off is relative to its layer's name
// base; an entry finds its layer by binary search in the table.
//
// Per entry (record r, raw name N) the stage decides exactly what tar_index_host.h's
// ClassifyPath followed by analyzer.cpp's Required decide, or asks the host:
//
//   type     regular when typeflag is '0' or '\0'; a '\0' entry whose non-empty name ends
//            in '/' is a directory.
//   name     N = P + M + T with P the longest of "./", "/", "" that prefixes N, T zero or
//            more trailing '/', M non-empty, M[0] != '/', GoPathIsClean(M).  Then the
//            cleaned, slash-stripped path is fp = M, a view of the raw name.  Every other
//            name ("", ".", "./", "/", "//a", ".//a", "a//b", "a/./b", "a/../b", "../a",
//            "/../a", ...) is kReqAskName, whatever the typeflag: the host cleans it.
//   markers  the base name of fp: ".wh..wh..opq" is an opaque dir, else a ".wh." prefix a
//            whiteout, for any typeflag; a marker is counted and is never a regular file.
//   Required for a regular non-marker, in the host's order: int64(size) < 10; a ".git" or
//            "node_modules" element in the directory part; the seven skip files; fp equal
//            to the analyzer's config base; the fourteen skip extensions (the last '.' of
//            the base name, at most 7 bytes from the dot); then the global allow paths:
//            without a PathTable kReqAskAllow for all rules; a non-ASCII fp kReqAskAllow
//            for all rules; an ASCII fp of at most kSureMaxPath bytes completing a literal
//            of the SureTable is dropped; an fp holding no literal of the PathTable is
//            kReqKeep; anything else kReqAskAllow with the mask of the rules whose literal
//            it holds (SecretScanner::AllowPathMasked).
//
// Output, in walk order, layer after layer: one tsg_tar_file_rec per kReqKeep /
// kReqAskAllow / kReqAskName entry, and a path blob that holds fp + NUL for the first two
// and the raw name + NUL for the third -- so when nothing asked is later dropped or
// renamed the blob is already TarIndexData::pool.  path_off is relative to the layer's
// first path byte.  One TarRequiredCounts per layer.  Offsets come from two inclusive sums
// on the stream; there is no capacity and no second run: the outputs are sized for the
// worst case (a record per entry, every name plus its NUL) and nothing is written past the
// counted sizes.  A record whose name lies outside its layer's name blob is kReqBad: it is
// counted, never read, and the pass's result is refused.
//
// With LayerTar's skip options (tsg_analyzer_set_tar_required_skip mode 1, every pattern one of
// tar_skip_dev.h's forms) three more kernels run between the decisions and the sums, and
// rewrite the verdict byte of the entries the options drop (tar_skip.h is the host's side):
//
//   match   a non-marker directory (kReqOther with typeflag '5', or '\0' with a name that ends
//           in '/') whose fp a directory pattern matches becomes kReqSkipDir: it is recorded.
//           A regular non-marker (kReqDrop, kReqKeep, kReqAskAllow) whose fp a file pattern
//           matches becomes kReqSkipFile.  Markers and kReqAskName entries are not tested.
//   build   an open-addressing table in HBM of the recorded directories: (layer, fp) and
//           (layer, direct parent of fp) -> the lowest rank (header chain start) recorded, as
//           TarSkipDirs::first_ and parent_first_.  A slot is owned by an entry index, claimed
//           by compare-and-swap; a key is compared byte by byte with the owner's name.
//   under   a regular survivor whose fp, or an ancestor of fp, is a recorded directory of its
//           layer, or whose fp is the direct parent of one, with a rank below its own, becomes
//           kReqSkipUnder.  On the names the device decides (clean, not empty, no ".."
//           element) that is tar.go's underSkippedDir: filepath.Rel never fails there, and
//           its result avoids the "../" prefix in exactly those three cases.
//
// kReqSkipFile and kReqSkipUnder entries stay in `regular`, are counted and have no record;
// a kReqSkipDir entry has a record (fp + NUL, its rank in `start`), so the host knows the
// recorded list for the names it was asked about.
#pragma once
#include <cstdint>

namespace tsg {

enum : uint8_t {
  kReqOther = 0,     // decided: neither a regular file nor a marker (directories, links, ...)
  kReqWhiteout = 1,  // decided: a ".wh." marker
  kReqOpaque = 2,    // decided: ".wh..wh..opq"
  kReqDrop = 3,      // decided: a regular file Required refuses
  kReqKeep = 4,      // decided: a regular file Required accepts
  kReqAskAllow = 5,  // a regular file up to the allow paths: the host runs the exact rules
  kReqAskName = 6,   // a name the device does not clean: the host runs ClassifyPath and Required
  kReqBad = 7,       // the record's name lies outside its layer's name blob
  // only when the skip stage ran:
  kReqSkipDir = 8,    // decided: a directory that skipDirs matches (recorded; it has a record)
  kReqSkipFile = 9,   // decided: a regular file that skipFiles matches
  kReqSkipUnder = 10, // decided: a regular file under a directory recorded before it
};

struct tsg_tar_file_rec {
  uint64_t start;     // the entry's header chain start
  uint64_t data;      // its content
  uint64_t size;
  uint64_t path_off;  // in the layer's part of the path blob; a NUL follows the path
  uint32_t path_len;
  uint8_t typeflag;   // as written (what kReqAskName's host half needs)
  uint8_t verdict;    // kReqKeep, kReqAskAllow, kReqAskName; kReqSkipDir with skip options
  uint8_t all_rules;  // kReqAskAllow: run every allow rule (non-ASCII, or no PathTable)
  uint8_t pad;
  uint64_t rules;     // kReqAskAllow without all_rules: bit i = allow rule i has a literal in fp
};
static_assert(sizeof(tsg_tar_file_rec) == 48, "the kernel writes three 16-B words per record");

struct TarRequiredRow {
  uint64_t rec_base, name_base;
};

struct TarRequiredCounts {       // per layer
  uint64_t entries;              // all of the layer's entries
  uint64_t regular, whiteouts, opaque_dirs;  // among the decided entries (kReqAskName ones are the host's)
  uint64_t records, path_bytes;  // what the layer has in the two outputs (kReqSkipDir records included)
  uint64_t kept, dropped, ask_allow, ask_name, bad;  // verdict totals (after the skip stage, where it ran)
  uint64_t ext_headers;          // the sum of the entries' n_ext (tsg_device_tar_stats.off_chain)
  uint64_t rec_first, path_first;  // where the layer's records / paths begin in the outputs
  // the skip stage's verdict totals (zero where it did not run): pad[0] = kReqSkipDir,
  // pad[1] = kReqSkipFile | kReqSkipUnder << 32 (a stage has fewer than 2^31 entries)
  uint64_t pad[2];
  uint64_t skipped_dirs() const { return pad[0]; }
  uint64_t skipped_files() const { return pad[1] & 0xFFFFFFFFu; }
  uint64_t under_skipped_dir() const { return pad[1] >> 32; }
};
static_assert(sizeof(TarRequiredCounts) == 128, "sixteen 8-B words per layer");

// The one device buffer of a stage over n entries of n_layers layers: byte offsets of its
// parts (256-B aligned) and its size.  `tables` (rows, then the config base) is filled by
// the host (TarRequiredTables) and uploaded.  skip_tab: the TarSkipTable behind the config base,
// part of `tables` and of the upload only when the stage was planned with skip options.
struct TarRequiredLayout {
  uint64_t n = 0, name_bytes = 0;
  uint32_t n_layers = 0, cfg_len = 0;
  bool skip = false;
  uint64_t tables = 0, cfg = 0, skip_tab = 0, counts = 0, dec = 0, rrank = 0, brank = 0, temp = 0, recs = 0, blob = 0;
  uint64_t tables_bytes = 0, temp_bytes = 0, blob_cap = 0, bytes = 0;
};

// A slot of the skip stage's table: the entry (bit 31: the key is its direct parent) that claimed
// it, and the lowest rank recorded for the key.  Empty: all ones.
struct TarSkipSlot {
  uint32_t owner, pad;
  uint64_t rank;
};
static_assert(sizeof(TarSkipSlot) == 16, "one 16-B slot");
// Slots for n_dirs recorded directories: every one may bring two keys, and the table is four
// times the keys, rounded up to a power of two.
inline uint64_t TarSkipSlots(uint64_t n_dirs) {
  uint64_t s = 8;
  while (s < 8 * n_dirs) s <<= 1;
  return s;
}

}  // namespace tsg
