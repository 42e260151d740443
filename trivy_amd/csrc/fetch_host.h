// Host side of a device-only batch's fetch (engine.h FetchOut, fetch.h): the
// layout the device makes, restated from the files the host knows are marked,
// and the pool of pinned buffers the fetched bytes come back in.  No HIP calls
// here: the engine supplies the allocator and the retirement, so this logic
// runs (and is sanitized) without a GPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <functional>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "engine.h"
#include "fetch_layout.h"

namespace tsg {

// The layout FetchPlan makes on the device, restated on the host from the
// files marked: the packed files in file order, each rounded up to 16 B, then
// the direct ones (of direct bytes or more), each at a 16-B boundary too.
struct HostFetchPlan {
  uint64_t packed = 0, total = 0, bytes = 0, files = 0;
  std::vector<uint32_t> direct;
};

inline void PlanFetchOnHost(std::vector<uint8_t> want, const uint64_t* h_off, uint32_t n_files, uint64_t direct,
                            FetchOut* out, HostFetchPlan* P) {
  out->Release();
  out->fetched = std::move(want);
  out->fetched.resize(n_files, 0);
  out->off.assign(size_t(n_files) + 1, 0);
  *P = HostFetchPlan();
  uint64_t p = 0;
  for (uint32_t f = 0; f < n_files; f++) {
    out->off[f] = p;
    if (!out->fetched[f]) continue;
    const uint64_t len = h_off[f + 1] - h_off[f];
    P->files++;
    P->bytes += len;
    if (len >= direct) P->direct.push_back(f);
    else p += (len + 15) & ~uint64_t(15);
  }
  P->packed = p;
  for (uint32_t f : P->direct) {
    out->off[f] = p;
    p += (h_off[f + 1] - h_off[f] + 15) & ~uint64_t(15);
  }
  P->total = p;
  out->off[n_files] = p;
}

// The counters the device's plan wrote (fetch.h FetchCounters, passed field by field) against the host's.
inline bool SameFetchPlan(uint64_t dev_packed, uint64_t dev_direct, uint64_t dev_files, uint64_t dev_bytes,
                          const HostFetchPlan& P, std::string* err) {
  if (dev_packed == P.packed && dev_direct == P.direct.size() && dev_files == P.files && dev_bytes == P.bytes)
    return true;
  *err = "fetch: the device laid out " + std::to_string(dev_files) + " files / " + std::to_string(dev_packed) +
         " packed bytes / " + std::to_string(dev_direct) + " direct, the host " + std::to_string(P.files) + " / " +
         std::to_string(P.packed) + " / " + std::to_string(P.direct.size());
  return false;
}

inline void FinishFetch(const HostFetchPlan& P, uint64_t stage, double ms, FetchOut* out) {
  out->files = P.files;
  out->bytes = P.bytes;
  out->direct_files = P.direct.size();
  out->rounds = uint32_t((P.packed + stage - 1) / stage);
  out->ms_fetch = ms;
}

// ---- the windows fetch (fetch_layout.h), restated on the host ----
//
// From the candidates the host holds: the maximal runs of marked granules in
// arena order (sorted, merged spans -- no bitmap), each with its place in the
// packed layout, and the totals the device counted (fetch_windows.h
// FetchWinCounters).  A file's view is the runs that meet its bytes, clipped
// to the file.
struct FilePiece {  // file-relative bytes [lo, hi), where they lie in the packed layout, and the run they are of
  uint64_t lo, hi, packed;
  size_t run;
};
struct HostWindowPlan {
  std::vector<GranuleRun> runs;
  std::vector<uint8_t> whole;  // per file: marked whole
  uint64_t granules = 0, whole_files = 0;
  uint64_t packed_bytes() const { return granules * kFetchGranule; }
};

inline void PlanWindowsOnHost(const Candidate* c, size_t nc, const uint64_t* h_off, uint32_t n_files,
                              const uint32_t* rule_max_len, uint32_t n_rules, const FetchWinParams& prm,
                              HostWindowPlan* P) {
  *P = HostWindowPlan();
  P->whole.assign(n_files, 0);
  std::vector<std::pair<uint64_t, uint64_t>> spans;
  spans.reserve(nc);
  for (size_t i = 0; i < nc; i++) {
    const uint32_t f = c[i].file;
    if (f >= n_files || (c[i].flags & kCandDrop)) continue;  // as mark_files_kernel
    uint64_t g0, g1;
    bool whole;
    const uint32_t ml = c[i].rule < n_rules ? rule_max_len[c[i].rule] : kFetchNoMaxLen;
    if (!CandidateGranules(c[i].wlo, c[i].whi, ml, h_off[f], h_off[f + 1], prm, &g0, &g1, &whole)) continue;
    if (whole && !P->whole[f]) {
      P->whole[f] = 1;
      P->whole_files++;
    }
    spans.push_back({g0, g1});
  }
  std::sort(spans.begin(), spans.end());
  for (const auto& s : spans) {
    if (!P->runs.empty() && s.first <= P->runs.back().g1) P->runs.back().g1 = std::max(P->runs.back().g1, s.second);
    else P->runs.push_back(GranuleRun{s.first, s.second, 0});
  }
  for (GranuleRun& r : P->runs) {
    r.packed = P->granules * kFetchGranule;
    P->granules += r.g1 - r.g0;
  }
}

// File [fs, fe)'s view: appended to *out in file order; `from`: a run index at
// or before the file's first (views taken in file order pass the last result).
inline size_t FileViewOf(const HostWindowPlan& P, uint64_t fs, uint64_t fe, size_t from, std::vector<FilePiece>* out) {
  size_t k = from;
  while (k < P.runs.size() && P.runs[k].g1 * kFetchGranule <= fs) k++;
  const size_t first = k;
  for (; k < P.runs.size() && P.runs[k].g0 * kFetchGranule < fe; k++) {
    const uint64_t a = std::max(fs, P.runs[k].g0 * kFetchGranule), b = std::min(fe, P.runs[k].g1 * kFetchGranule);
    if (a < b) out->push_back(FilePiece{a - fs, b - fs, P.runs[k].packed + (a - P.runs[k].g0 * kFetchGranule), k});
  }
  return first;
}

inline bool SameWindowPlan(uint64_t dev_granules, uint64_t dev_runs, uint64_t dev_whole, const HostWindowPlan& P,
                           std::string* err) {
  if (dev_granules == P.granules && dev_runs == P.runs.size() && dev_whole == P.whole_files) return true;
  *err = "fetch windows: the device marked " + std::to_string(dev_granules) + " granules / " +
         std::to_string(dev_runs) + " runs / " + std::to_string(dev_whole) + " whole files, the host " +
         std::to_string(P.granules) + " / " + std::to_string(P.runs.size()) + " / " + std::to_string(P.whole_files);
  return false;
}

// Pinned fetch buffers: on loan to the scans' FetchOut, back to a small free
// list afterwards.  Take hands out the smallest free buffer that holds `need`,
// or allocates one a quarter larger; a buffer the list has no room for -- the
// smallest -- is retired (the engine's RetireHost: freed by the reaper thread,
// outside every engine lock), never freed by the caller's thread.
class FetchPool {
 public:
  using Alloc = std::function<void*(size_t)>;
  using Retire = std::function<void(void*)>;
  FetchPool(size_t keep, Alloc alloc, Retire retire)
      : keep_(keep), alloc_(std::move(alloc)), retire_(std::move(retire)) {}
  void* Take(size_t need, size_t* cap) {
    {
      std::lock_guard<std::mutex> g(mu_);
      size_t best = free_.size();
      for (size_t i = 0; i < free_.size(); i++)
        if (free_[i].cap >= need && (best == free_.size() || free_[i].cap < free_[best].cap)) best = i;
      if (best < free_.size()) {
        const Buf b = free_[best];
        free_.erase(free_.begin() + long(best));
        *cap = b.cap;
        return b.p;
      }
    }
    const size_t n = std::max<size_t>(need + need / 4, size_t(64) << 10);
    void* p = alloc_(n);
    if (!p) return nullptr;
    *cap = n;
    Trim(keep_ > 0 ? keep_ - 1 : 0);  // every free buffer was too small: the smallest makes room for the new one
    return p;
  }
  void Give(void* p, size_t cap) {
    if (!p) return;
    {
      std::lock_guard<std::mutex> g(mu_);
      free_.push_back(Buf{p, cap});
    }
    Trim(keep_);
  }
  // the free buffers, for the owner's destructor (nothing is on loan then)
  std::vector<void*> Drain() {
    std::lock_guard<std::mutex> g(mu_);
    std::vector<void*> v;
    for (const Buf& b : free_) v.push_back(b.p);
    free_.clear();
    return v;
  }
  size_t free_count() {
    std::lock_guard<std::mutex> g(mu_);
    return free_.size();
  }

 private:
  struct Buf {
    void* p;
    size_t cap;
  };
  void Trim(size_t keep) {
    for (;;) {
      void* old = nullptr;
      {
        std::lock_guard<std::mutex> g(mu_);
        if (free_.size() <= keep) return;
        size_t s = 0;
        for (size_t i = 1; i < free_.size(); i++)
          if (free_[i].cap < free_[s].cap) s = i;
        old = free_[s].p;
        free_.erase(free_.begin() + long(s));
      }
      retire_(old);
    }
  }
  size_t keep_;
  Alloc alloc_;
  Retire retire_;
  std::mutex mu_;
  std::vector<Buf> free_;
};

}  // namespace tsg
