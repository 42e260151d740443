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
};

struct tsg_tar_file_rec {
  uint64_t start;     // the entry's header chain start
  uint64_t data;      // its content
  uint64_t size;
  uint64_t path_off;  // in the layer's part of the path blob; a NUL follows the path
  uint32_t path_len;
  uint8_t typeflag;   // as written (what kReqAskName's host half needs)
  uint8_t verdict;    // kReqKeep, kReqAskAllow, kReqAskName
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
  uint64_t records, path_bytes;  // what the layer has in the two outputs
  uint64_t kept, dropped, ask_allow, ask_name, bad;  // verdict totals
  uint64_t ext_headers;          // the sum of the entries' n_ext (tsg_device_tar_stats.off_chain)
  uint64_t rec_first, path_first;  // where the layer's records / paths begin in the outputs
  uint64_t pad[2];
};
static_assert(sizeof(TarRequiredCounts) == 128, "sixteen 8-B words per layer");

// The one device buffer of a stage over n entries of n_layers layers: byte offsets of its
// parts (256-B aligned) and its size.  `tables` (rows, then the config base) is filled by
// the host (TarRequiredTables) and uploaded.
struct TarRequiredLayout {
  uint64_t n = 0, name_bytes = 0;
  uint32_t n_layers = 0, cfg_len = 0;
  uint64_t tables = 0, cfg = 0, counts = 0, dec = 0, rrank = 0, brank = 0, temp = 0, recs = 0, blob = 0;
  uint64_t tables_bytes = 0, temp_bytes = 0, blob_cap = 0, bytes = 0;
};

}  // namespace tsg
