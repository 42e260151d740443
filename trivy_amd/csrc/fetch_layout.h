// The windows fetch of a device-only batch: what is fetched, shared by the
// device (fetch_windows.hip) and the host (fetch_host.h), so that both derive
// the same layout from the same candidates.
//
// Granule: kFetchGranule = 256 bytes of the arena at a multiple of 256 from
// its start -- 16 lanes x one aligned 16-B access; the bitmap of marked
// granules is 1/2048 of the arena; a bounded rule's span fits in two or three.
// Granules ignore file boundaries: one may carry a neighbour's bytes, which
// the host's file views never expose.
//
// Span: a candidate (wlo, whi) of a file of len bytes wants the file-relative
// bytes [max(0, wlo - back), min(len, whi + 1 + fwd)): a match starts in
// [wlo, whi]; the regex engine looks back at most one rune (<= 4 B) for \b, ^
// and (?m)^, so back >= 4 (16, one aligned block, by default); fwd is the
// rule's max_len + 4 (one look-ahead rune of \b / $) where max_len is bounded
// and at most fwd_cap, else fwd_bytes.  A window wider than max_span, and a
// span that covers every granule of its file anyway, mark the whole file.
// Correctness never rests on these numbers: the exact pass reports a read
// beyond the bytes it was given (goregex.h FindAllBounded) and the file is
// then fetched whole.
//
// Packed layout: the marked granules in arena order, 256 B each, no gaps.  A
// maximal run of consecutive marked granules is one contiguous piece.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define TSG_HD __host__ __device__
#else
#define TSG_HD
#endif

namespace tsg {

constexpr uint32_t kFetchGranule = 256;
constexpr uint32_t kFetchGranuleShift = 8;
constexpr uint32_t kFetchNoMaxLen = 0xFFFFFFFFu;  // (rules.h kNoMaxLen)

constexpr uint32_t kFetchBackDefault = 16, kFetchBackMin = 4;
constexpr uint32_t kFetchFwdDefault = 1024, kFetchFwdCapDefault = 4096, kFetchMaxSpanDefault = 65536;

struct FetchWinParams {
  uint32_t back = kFetchBackDefault, fwd_bytes = kFetchFwdDefault, fwd_cap = kFetchFwdCapDefault,
           max_span = kFetchMaxSpanDefault;
};

// A maximal run of consecutive marked granules and its place in the packed layout.
struct GranuleRun {
  uint64_t g0, g1;  // arena granules [g0, g1)
  uint64_t packed;  // byte offset of granule g0 in the packed layout
};

TSG_HD inline uint64_t FetchGranules(uint64_t n_bytes) { return (n_bytes + kFetchGranule - 1) >> kFetchGranuleShift; }

// The arena granules [*g0, *g1) a candidate marks; *whole: the whole file.
// [fs, fe): the file's bytes in the arena.  false: nothing (an empty file).
TSG_HD inline bool CandidateGranules(int64_t wlo, int64_t whi, uint32_t rule_max_len, uint64_t fs, uint64_t fe,
                                     const FetchWinParams& p, uint64_t* g0, uint64_t* g1, bool* whole) {
  if (fe <= fs) return false;
  const int64_t len = int64_t(fe - fs);
  if (wlo < 0) wlo = 0;
  if (wlo > len) wlo = len;
  if (whi < wlo) whi = wlo;
  if (whi > len) whi = len;
  const uint64_t f0 = fs >> kFetchGranuleShift, f1 = (fe + kFetchGranule - 1) >> kFetchGranuleShift;
  bool all = uint64_t(whi - wlo) + 1 > uint64_t(p.max_span);
  if (!all) {
    const int64_t fwd = rule_max_len != kFetchNoMaxLen && rule_max_len <= p.fwd_cap ? int64_t(rule_max_len) + 4
                                                                                      : int64_t(p.fwd_bytes);
    int64_t a = wlo - int64_t(p.back), b = whi + 1 + fwd;
    if (a < 0) a = 0;
    if (b > len) b = len;
    if (a >= b) a = b - 1;  // (wlo == len: the file's last byte; len >= 1)
    *g0 = (fs + uint64_t(a)) >> kFetchGranuleShift;
    *g1 = (fs + uint64_t(b) + kFetchGranule - 1) >> kFetchGranuleShift;
    all = *g0 == f0 && *g1 == f1;
  }
  if (all) {
    *g0 = f0;
    *g1 = f1;
  }
  *whole = all;
  return true;
}

}  // namespace tsg
