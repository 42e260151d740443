// Global allow-path prefilter on the GPU (scanner.go:57-59, 381-386).
//
// Scan returns Secret{FilePath} for every file whose path an allow rule
// matches, so the allow-path rules run over every path of a batch -- on the
// host that was ~31 ns per path, a sixth of the host CPU of a C2 scan.  Here
// one lane per path runs a shift-and over the allow rules' required literals
// (Matcher::lits: an ASCII path holding none of a rule's lowercased literals
// cannot match it) and reports the paths that hold one, with the rules whose
// literal they hold, plus every non-ASCII path.  The host runs the exact rule
// only on those (about 10 % of C2's paths); every other path is not allowed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <string>
#include <vector>

namespace tsg {

struct PathHit {        // one reported path
  uint32_t file;        // | kPathNonAscii: the host runs every rule on it
  uint32_t pad;
  uint64_t rules;       // allow rules (bit i = rule i) with a literal in the lowered path
};
constexpr uint32_t kPathNonAscii = 0x80000000u;

// Literals packed into up to four 64-bit shift-and words (a literal never
// crosses a word); the byte table is indexed by the ASCII-lowered byte.
struct PathTable {
  uint64_t B[256][4];   // positions that accept the byte
  uint64_t S[4], E[4];  // first / last position of each literal
  uint8_t rule_of[256]; // word * 64 + bit of a literal's last position -> its rule
  uint32_t words;
};

// Builds the table; false when the literals do not fit (more than 64 rules,
// a literal shorter than 2 or longer than 64 bytes, over 256 positions).
bool BuildPathTable(const std::vector<std::pair<std::string, uint32_t>>& lits, PathTable* t);

// The "surely allowed" decision: a second shift-and beside the
// prefilter's, over the exact literal forms of the allow-path regexes that
// have one (rules.h ExactPathLiterals).  Indexed by the raw byte: a
// case-sensitive position accepts one byte, a (?i) position both cases.  A
// path that is ASCII-only, at most kSureMaxPath bytes long and completes a
// literal is matched by that literal's regex, so its file is allow-listed
// whatever its bytes hold: the scan may skip them.  The decision never says
// yes for a path the host's exact AllowPath would refuse; it says no for every
// non-ASCII or over-long path and when no rule has an exact form.
struct SureTable {
  uint64_t B[256][4];     // positions that accept the byte
  uint64_t S[4], S0[4];   // first positions: injected at every byte / at offset 0 only (^ literals)
  uint64_t E[4], EZ[4];   // last positions: honoured anywhere / at the path's last byte only ($ literals)
  uint32_t words;         // 0: no exact form (or the literals do not fit): nothing is surely allowed
};
constexpr uint64_t kSureMaxPath = 4096;

// One step of either shift-and for word w and byte c, shared by path_filter_kernel, its host
// model and the resident layers' Required stage (tarrequired.hip).  The prefilter's table is
// indexed by the ASCII-lowered byte.  The exact one leaves a literal at its last position (a
// carry into the next literal's first position would be a start the regex does not have -- a
// ^ literal starts at offset 0 only).
#define TSG_PATH_STEP(D, w, c, T_B, T_S) ((((D) << 1) | (T_S)[w]) & (T_B)[c][w])
#define TSG_SURE_STEP(D, w, c, first, T_B, T_S, T_S0, T_E, T_EZ) \
  ((((D) & ~((T_E)[w] | (T_EZ)[w])) << 1 | (T_S)[w] | ((first) ? (T_S0)[w] : 0)) & (T_B)[c][w])
struct SureLit {          // one exact literal: per position the byte(s) it accepts
  std::vector<std::pair<uint8_t, uint8_t>> pos;
  bool begin = false, end = false;
};
// False (words = 0) when there is no literal or they do not fit 4 x 64 positions.
bool BuildSureTable(const std::vector<SureLit>& lits, SureTable* t);
// The kernel's decision on the host (the model the tests check against the oracle).
bool SureAllowHost(const SureTable& t, const uint8_t* p, uint64_t n);

class PathFilter {
 public:
  PathFilter(int device, const PathTable& t);
  ~PathFilter();
  bool ok() const { return err_.empty(); }
  const std::string& error() const { return err_; }
  // Paths [off[i], off[i+1]) of d_paths (device), i < n: the reported ones
  // (any order).  Thread-safe: up to kSlots calls run at once, each on a
  // high-priority stream and buffers of its own (a few microseconds of GPU time
  // that should not queue behind a scan's kernels, nor behind another scan's
  // filter: one shared stream and lock serialised the first scans of a
  // pipeline, each waiting out a filter kernel queued behind a K1).
  bool Run(const uint8_t* d_paths, const uint64_t* d_off, uint32_t n, std::vector<PathHit>* out, std::string* err) {
    return RunImpl(d_paths, d_off, nullptr, nullptr, n, out, err);
  }
  // The same over paths packed in host memory (the analyzer's collectors:
  // h_off[i] .. h_off[i+1] into h_paths): staged through the slot's pinned
  // buffer and copied to HBM on the slot's stream first.
  bool RunHost(const uint8_t* h_paths, const uint64_t* h_off, uint32_t n, std::vector<PathHit>* out,
               std::string* err) {
    return RunImpl(nullptr, nullptr, h_paths, h_off, n, out, err);
  }

  // The split form, for a scan that skips the surely allowed files: Submit
  // launches the kernel (and the read-back copies) on a slot's stream and
  // returns at once; with want_skip the kernel also fills the slot's per-file
  // skip bytes (1 = surely allowed) and `ready` is recorded behind it, for the
  // scan's stream to wait on.  Finish waits for the read-back and returns the
  // reported paths, as Run does.  The slot -- the skip bytes -- stays the
  // caller's until Release, which the caller calls once the scan's GPU phase
  // is over.  Give either host or device paths, as to Run / RunHost.
  struct Pending {
    int slot = -1;
    const uint8_t* d_skip = nullptr;  // null without want_skip (or without a sure table)
    hipEvent_t ready = nullptr;
    uint32_t n = 0, guess = 0;
  };
  void SetSureTable(const SureTable& t);  // before the first Submit; a table with words = 0 is ignored
  bool has_sure() const { return d_sure_ != nullptr; }
  // Test-only, off by default: a slot's skip bytes are filled with 0xEE when they are
  // allocated, so a byte the kernel leaves unwritten shows (tsg_debug_path_filter).
  void set_skip_fill(bool on) { skip_fill_ = on; }
  // The two tables in HBM, for kernels outside this class (tarrequired.hip); d_sure() is NULL without one.
  const PathTable* d_table() const { return d_table_; }
  const SureTable* d_sure() const { return d_sure_; }
  bool Submit(const uint8_t* d_paths, const uint64_t* d_off, const uint8_t* h_paths, const uint64_t* h_off,
              uint32_t n, bool want_skip, Pending* p, std::string* err);
  bool Finish(Pending* p, std::vector<PathHit>* out, std::string* err);
  void Release(Pending* p);

 private:
  bool RunImpl(const uint8_t* d_paths, const uint64_t* d_off, const uint8_t* h_paths, const uint64_t* h_off,
               uint32_t n, std::vector<PathHit>* out, std::string* err) {
    Pending p;
    const bool ok = Submit(d_paths, d_off, h_paths, h_off, n, false, &p, err) && Finish(&p, out, err);
    Release(&p);
    return ok;
  }
  struct Slot {
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    hipEvent_t ready = nullptr;  // behind the kernel: the skip bytes are written
    uint8_t* d_skip = nullptr;   // one byte per file (Submit with want_skip)
    size_t skip_cap = 0;
    uint32_t* d_cnt = nullptr;  // two counters used in turn: each launch zeroes the next one's
    uint32_t parity = 0;
    uint32_t* h_cnt = nullptr;
    PathHit* d_out = nullptr;
    PathHit* h_out = nullptr;  // pinned: a pageable read-back stalled the engine's stream (5 ms per C2 scan)
    size_t cap = 0;
    // RunHost: the packed paths and their offsets in HBM, and their pinned staging
    uint8_t* d_paths = nullptr;
    size_t paths_cap = 0;
    uint8_t* h_stage = nullptr;
    size_t stage_cap = 0;
    bool busy = false;
  };
  // (a scan that skips holds its slot through its GPU phase: as many as scans in flight)
  static constexpr int kSlots = 8;
  std::mutex mu_;
  std::condition_variable cv_;
  Slot slots_[kSlots];
  std::atomic<uint32_t> last_k_{0};  // records of the last call: one read-back when the count repeats
  int device_ = 0;
  bool skip_fill_ = false;
  std::string err_;
  PathTable* d_table_ = nullptr;
  SureTable* d_sure_ = nullptr;
};

}  // namespace tsg
