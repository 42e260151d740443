// LayerTar's skipFiles / skipDirs (pkg/fanal/walker/tar.go:23-33, :64-81,
// underSkippedDir :105-116) for every layer walk: the host walk
// (analyzer.cpp) and both host halves of a resident layer's index
// (tar_index_host.h).  Plain C++: it runs without HIP.
//
// What an entry is by itself -- a directory that a skipDirs pattern matches, a
// regular file that a skipFiles pattern matches -- is a pure function of the
// entry (TarSkipEval) and is computed wherever the entry is evaluated, on any
// thread.  What depends on the order of the archive -- whether a survivor lies
// under a directory that was skipped *before* it -- is answered by TarSkipDirs,
// which keeps the recorded directories with the rank (the offset of the entry's
// header chain) at which each was recorded.
#pragma once
#include <cstdint>
#include <deque>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "skip_path.h"
#include "tar_skip_dev.h"

namespace tsg {

// The patterns, already cleaned (utils.CleanSkipPaths: the caller's part, as in tsg_fs_walk_new).
struct TarSkipOpts {
  std::vector<std::string> dirs, files;
  bool any() const { return !dirs.empty() || !files.empty(); }
  // the same patterns as the GPU stage reads them (tar_skip_dev.h), where it takes them all:
  // filled by whoever sets the options (Classify)
  bool dev_ok = false;
  TarSkipTable dev;
  void Classify() { dev_ok = TarSkipClassify(dirs, files, &dev); }
};

struct TarSkipCounts {
  uint64_t skipped_dirs = 0, skipped_files = 0, under_skipped_dir = 0;
};

// TarEntry::skip
enum : uint8_t {
  kTarSkipNone = 0,
  kTarSkipDir = 1,    // a directory that skipDirs matches: recorded, dropped
  kTarSkipFile = 2,   // a regular file that skipFiles matches: dropped
  kTarSkipUnder = 3,  // a regular file under a directory recorded before it: dropped
};

// tar.go:64-77 for an entry that is no whiteout and no opaque marker: is_dir is
// TypeDir (typeflag '5', or '\0' with a resolved name that ends in '/'),
// is_reg TypeReg.  Out of line, as TarSkipStep below: the walks' per-entry loops,
// which call these only with options set, keep the code they have without them.
__attribute__((noinline)) inline uint8_t TarSkipEval(const TarSkipOpts& o, bool is_dir, bool is_reg, std::string_view file_path) {
  if (is_dir) return !o.dirs.empty() && SkipPath(file_path, o.dirs) ? kTarSkipDir : kTarSkipNone;
  if (is_reg) return !o.files.empty() && SkipPath(file_path, o.files) ? kTarSkipFile : kTarSkipNone;
  return kTarSkipNone;
}

// filepath.Rel(base, targ) on Unix (Go 1.22 path/filepath/path.go), both
// inputs path.Clean-ed already but for "", which cleans to ".".  false: Rel fails.
inline bool GoRel(std::string_view base, std::string_view targ, std::string* rel) {
  if (base.empty()) base = ".";
  if (targ.empty()) targ = ".";
  if (base == targ) {
    *rel = ".";
    return true;
  }
  if (base == ".") base = std::string_view();
  const bool base_slashed = !base.empty() && base[0] == '/';
  const bool targ_slashed = !targ.empty() && targ[0] == '/';
  if (base_slashed != targ_slashed) return false;
  const size_t bl = base.size(), tl = targ.size();
  size_t b0 = 0, bi = 0, t0 = 0, ti = 0;
  while (bi < bl && ti < tl) {  // base[b0:bi] and targ[t0:ti] at the first differing elements
    while (bi < bl && base[bi] != '/') bi++;
    while (ti < tl && targ[ti] != '/') ti++;
    if (targ.substr(t0, ti - t0) != base.substr(b0, bi - b0)) break;
    if (bi < bl) bi++;
    if (ti < tl) ti++;
    b0 = bi;
    t0 = ti;
  }
  if (base.substr(b0, bi - b0) == "..") return false;
  if (b0 != bl) {  // base elements left: up before down
    rel->assign("..");
    for (size_t i = b0; i < bl; i++)
      if (base[i] == '/') rel->append("/..");
    if (t0 != tl) {
      rel->push_back('/');
      rel->append(targ.substr(t0));
    }
    return true;
  }
  rel->assign(targ.substr(t0));
  return true;
}

// The directories a walk has skipped, in recording order, each with its rank
// (ranks ascend), and underSkippedDir over those recorded before a given rank.
//
// underSkippedDir loops over the list (first Rel failure: false; first result
// that does not start with "../": true).  On the common domain -- neither the
// path nor a recorded directory starts with "..", and no "." is recorded -- Rel
// never fails and its result avoids the "../" prefix in exactly three cases:
// the path is a recorded directory ("."), lies below one (the rest of the
// path), or is the direct parent of one ("..", which has no trailing slash).
// Those are hashed lookups of the path and of its ancestors; the list is
// looped over only outside that domain.
class TarSkipDirs {
 public:
  bool empty() const { return dirs_.empty(); }
  size_t size() const { return dirs_.size(); }
  void Clear() {
    dirs_.clear();
    at_.clear();
    first_.clear();
    parent_first_.clear();
    slow_from_ = ~uint64_t(0);
  }
  // Forgets what was recorded at `rank` or later (a walk resumed before its end).
  void Truncate(uint64_t rank) {
    if (at_.empty() || at_.back() < rank) return;
    std::deque<std::string> dirs;
    std::vector<uint64_t> at;
    for (size_t i = 0; i < at_.size() && at_[i] < rank; i++) {
      dirs.push_back(std::move(dirs_[i]));
      at.push_back(at_[i]);
    }
    Clear();
    for (size_t i = 0; i < at.size(); i++) Record(dirs[i], at[i]);
  }
  void Record(std::string_view file_path, uint64_t rank) {
    dirs_.emplace_back(file_path);
    at_.push_back(rank);
    const std::string_view d = dirs_.back();
    if (d.empty() || d == "." || d.substr(0, 2) == "..") {
      if (rank < slow_from_) slow_from_ = rank;
      return;
    }
    first_.emplace(d, rank);  // (the lowest rank stays)
    const size_t sl = d.rfind('/');
    if (sl != std::string_view::npos && sl > 0) parent_first_.emplace(d.substr(0, sl), rank);
  }
  // underSkippedDir(file_path, the directories recorded at a rank below `rank`).
  bool Under(std::string_view file_path, uint64_t rank) const {
    if (dirs_.empty() || at_.front() >= rank) return false;
    if (rank > slow_from_ || file_path.substr(0, 2) == "..") return UnderLoop(file_path, rank);
    auto before = [rank](const Map& m, std::string_view k) {
      auto it = m.find(k);
      return it != m.end() && it->second < rank;
    };
    if (before(first_, file_path) || before(parent_first_, file_path)) return true;
    for (size_t sl = file_path.find('/'); sl != std::string_view::npos; sl = file_path.find('/', sl + 1))
      if (sl > 0 && before(first_, file_path.substr(0, sl))) return true;
    return false;
  }
  // tar.go:105-116 as written.
  bool UnderLoop(std::string_view file_path, uint64_t rank) const {
    std::string rel;
    for (size_t i = 0; i < dirs_.size() && at_[i] < rank; i++) {
      if (!GoRel(dirs_[i], file_path, &rel)) return false;
      if (rel.compare(0, 3, "../") != 0) return true;
    }
    return false;
  }

 private:
  using Map = std::unordered_map<std::string_view, uint64_t>;
  std::deque<std::string> dirs_;  // (a deque: the maps' keys are views of its strings)
  std::vector<uint64_t> at_;
  Map first_;         // a recorded directory -> the lowest rank it was recorded at
  Map parent_first_;  // the direct parent of a recorded directory -> that rank
  uint64_t slow_from_ = ~uint64_t(0);  // the lowest rank of a directory outside the common domain
};

// tar.go:64-81 for one entry of a walk that goes through the archive in order
// (the entry is no marker): records a skipped directory at `rank`, counts, and
// returns the entry's kTarSkip* -- not kTarSkipNone: the entry is dropped.
__attribute__((noinline)) inline uint8_t TarSkipStep(const TarSkipOpts& o, bool is_dir, bool is_reg,
                                                     std::string_view file_path, uint64_t rank, TarSkipDirs* skipped,
                                                     TarSkipCounts* counts) {
  const uint8_t sk = TarSkipEval(o, is_dir, is_reg, file_path);
  if (sk == kTarSkipDir) {
    skipped->Record(file_path, rank);
    counts->skipped_dirs++;
  } else if (sk == kTarSkipFile) {
    counts->skipped_files++;
  } else if (is_reg && skipped->Under(file_path, rank)) {
    counts->under_skipped_dir++;
    return kTarSkipUnder;
  }
  return sk;
}

}  // namespace tsg
