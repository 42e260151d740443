// The host half of the split scan of a resident batch with a transform
// (SecretScanner::Scan): the sub-batch of the files the
// transform changes, planned from the census marks; its candidates and
// transformed bytes mapped back to the batch's files; where the exact pass
// reads each file.  No HIP here: tools/san_resident_split.cpp runs it under
// ASan + UBSan.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace tsg {

// What the census marks say about a batch.  A file is in place (mark 0: the
// transform leaves its bytes as they lie in the arena), changed (mark 1, kind
// 1 or 2: it goes through the pre-transform in the sub-batch) or dropped (kind
// 3: it takes no part).  The sub-batch holds the changed files in file order,
// back to back: ids[i] is sub-file i's batch id, off its compact offsets, src
// where its bytes as read start in the arena.
struct SplitPlan {
  std::vector<uint32_t> ids;
  std::vector<uint64_t> off;  // ids.size() + 1
  std::vector<uint8_t> kinds;
  std::vector<uint64_t> src;
  uint64_t files_in_place = 0, bytes_in_place = 0, files_changed = 0, bytes_changed = 0, files_dropped = 0,
           bytes_dropped = 0;
};

// False (with *err) for marks that contradict the kinds: a kind-0 file marked,
// a kind-2 or kind-3 file not, a kind above 3.
inline bool PlanSplit(const uint8_t* mark, const uint8_t* kind, const uint64_t* off, uint32_t n_files, SplitPlan* p,
                      std::string* err) {
  *p = SplitPlan();
  p->off.push_back(0);
  for (uint32_t f = 0; f < n_files; f++) {
    const uint64_t len = off[f + 1] - off[f];
    const uint8_t k = kind[f];
    const bool m = mark[f] != 0;
    if (k > 3 || (k == 0 && m) || (k >= 2 && !m) || mark[f] > 1) {
      *err = "split scan: census mark " + std::to_string(mark[f]) + " for file " + std::to_string(f) + " of kind " +
             std::to_string(k);
      return false;
    }
    if (!m) {
      p->files_in_place++;
      p->bytes_in_place += len;
    } else if (k == 3) {
      p->files_dropped++;
      p->bytes_dropped += len;
    } else {
      p->files_changed++;
      p->bytes_changed += len;
      p->ids.push_back(f);
      p->kinds.push_back(k);
      p->src.push_back(off[f]);
      p->off.push_back(p->off.back() + len);
    }
  }
  return true;
}

// The sub-batch's candidates get their batch file ids.  Every sub-batch file is
// changed by its transform, so the engine gathered the transformed bytes of each
// one that got candidates (sub_raw[i] == 0); anything else is an error.
template <class Cand>
bool RemapSubCandidates(const SplitPlan& p, const std::vector<uint8_t>& sub_raw, std::vector<Cand>* sub,
                        std::string* err) {
  if (sub_raw.size() != p.ids.size()) {
    *err = "split scan: the sub-batch's tail does not match its plan";
    return false;
  }
  for (Cand& c : *sub) {
    if (c.file >= p.ids.size()) {
      *err = "split scan: a sub-batch candidate names file " + std::to_string(c.file) + " of " +
             std::to_string(p.ids.size());
      return false;
    }
    if (sub_raw[c.file]) {
      *err = "split scan: changed file " + std::to_string(p.ids[c.file]) + " came back as read";
      return false;
    }
    c.file = p.ids[c.file];
  }
  return true;
}

// In-place candidates in a marked file (the finalize kernel drops them; none is
// expected) are removed: the file belongs to the sub-batch's scan.
template <class Cand>
size_t DropMarkedCandidates(const uint8_t* mark, uint32_t n_files, std::vector<Cand>* cands) {
  size_t w = 0;
  for (size_t i = 0; i < cands->size(); i++)
    if ((*cands)[i].file < n_files && !mark[(*cands)[i].file]) (*cands)[w++] = (*cands)[i];
  const size_t dropped = cands->size() - w;
  cands->resize(w);
  return dropped;
}

// Where the exact pass reads the changed files: their transformed bytes in the
// sub-batch's tail (tail_off: ids.size() + 1 offsets into tail_buf; a file
// without candidates is empty there).  fdata / flen / host_only have one entry
// per batch file; host_only[f] = 1: the bytes are not the resident arena's, the
// host makes the file's findings.  sparse (optional): the windows fetch's
// per-file flag, cleared for the changed files.
inline void MergeChanged(const SplitPlan& p, const uint8_t* tail_buf, const std::vector<uint64_t>& tail_off,
                         std::vector<const uint8_t*>* fdata, std::vector<uint64_t>* flen,
                         std::vector<uint8_t>* host_only, std::vector<uint8_t>* sparse) {
  for (size_t i = 0; i < p.ids.size(); i++) {
    const uint32_t f = p.ids[i];
    (*fdata)[f] = tail_buf + tail_off[i];
    (*flen)[f] = tail_off[i + 1] - tail_off[i];
    (*host_only)[f] = 1;
    if (sparse) (*sparse)[f] = 0;
  }
}

}  // namespace tsg
