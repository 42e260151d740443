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
