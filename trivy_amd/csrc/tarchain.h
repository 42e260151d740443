// The header chain of a tar layer resident in HBM, walked on the GPU
// (tarchain.hip; tsg_analyzer_set_tar_walk mode 1).  This header is plain C++:
// what the GPU half hands to the host half (tar_index_host.h: IndexTarEntries)
// -- one record and the raw name per archive entry, in walk order, and where
// and why the chain stopped -- and the caps of the GPU half.  The launchers are
// declared in tarindex.h.
//
// The GPU half decides, exactly as tar_index_host.h's ChainEntryT / ResolveT
// decide, every entry from block 0 up to the stop, the first entry start that is
// not completed.  The stop is END (the offset is at or past the layer's end, the
// block there is all zero, or the entry's extension headers run into either), or
// INCOMPLETE with a reason: something the device does not decide, or that is
// malformed.  An INCOMPLETE layer is walked again by the host walk, which alone
// words the errors of malformed archives.
#pragma once
#include <cstdint>

namespace tsg {

// One entry on the chain.  `name_off` / `name_len`: its raw name in the name
// blob, by ResolveT's precedence (PAX path, GNU 'L' data up to its first NUL,
// ustar prefix + '/' + name, name), before path.Clean.
struct tsg_tar_entry_rec {
  uint64_t start;     // the entry's first header (an x / L / K header, or hdr itself)
  uint64_t hdr;       // the entry's own header
  uint64_t data;      // hdr + 512
  uint64_t size;      // content bytes (0 for the header-only types; the PAX size where given)
  uint64_t name_off;
  uint32_t name_len;
  uint8_t typeflag;   // the own header's byte 156, as written
  uint8_t flags;      // kTarNamePax, kTarNameLong
  uint8_t n_ext;      // extension headers (x, L, K) before hdr
  uint8_t pad0;
  uint64_t pad1[2];
};
static_assert(sizeof(tsg_tar_entry_rec) == 64, "the kernel writes four 16-B words per record");
constexpr uint8_t kTarNamePax = 1;   // the name is a PAX path record's value
constexpr uint8_t kTarNameLong = 2;  // the name is GNU 'L' data

// Where the chain stopped.
enum : uint32_t { kTarStopEnd = 0, kTarStopIncomplete = 1 };
// Why an entry is incomplete: tsg_tar_walk_stats.fallback.
enum : uint32_t {
  kTarOk = 0,
  kTarBadSize = 1,       // a size field that does not parse, or is negative
  kTarBadPax = 2,        // a PAX record that does not parse
  kTarPaxSizeForm = 3,   // a PAX size value that is not 1..18 ASCII digits (the host reads it with strtoll)
  kTarCap = 4,           // over one of the caps below
  kTarNotCandidate = 5,  // a chain block that is neither a header candidate nor all zero
  kTarTruncated = 6,     // a header or an entry's data runs past the layer
  kTarTooLarge = 7,      // 2^31 or more blocks: the pass is not run (block indices keep bit 31 free)
};
struct tsg_tar_stop {
  uint32_t kind;    // kTarStopEnd / kTarStopIncomplete
  uint32_t reason;  // kTarOk for END
  uint64_t offset;  // the entry start where the chain stopped
  uint64_t ext_visited;  // END inside an entry: the extension headers hopped before it
  uint64_t steps;        // dependent loads of the stitch (at most one per segment entered)
};
static_assert(sizeof(tsg_tar_stop) == 32, "two 16-B words");

// The caps of a lane: every loop of the entry parse ends at one of these.
constexpr uint32_t kTarMaxExt = 16;               // extension headers in one entry
constexpr uint64_t kTarMaxPaxData = 64u << 10;    // bytes of one x header's data
constexpr uint64_t kTarMaxNameSrc = 64u << 10;    // bytes of an 'L' header's data
constexpr uint32_t kTarMaxPaxSizeDigits = 18;
constexpr uint64_t kTarMaxBlocks = uint64_t(1) << 31;

// The marking pass works on segments of a power-of-two number of blocks, one
// workgroup each with a 4-B word per block in LDS.
constexpr uint32_t kTarMinSegment = 8;
constexpr uint32_t kTarDefaultSegment = 8192;  // 32 KiB of LDS: two workgroups fit a CU's 160 KiB with room to spare

}  // namespace tsg
