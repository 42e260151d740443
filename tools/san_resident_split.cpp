// The host half of the split scan (trivy_amd/csrc/split_host.h) as a stand-alone
// program for ASan + UBSan (tools/san_resident_split.sh): the sub-batch plan from
// census marks, the remapping of the sub-batch's candidates, the merge of the
// exact pass's per-file views.  Every array is a heap block of exactly its size,
// so a read or write past an end is outside an allocation.  No GPU, no HIP.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "split_host.h"

namespace {

struct Cand {  // (the engine's Candidate has more fields; the host half touches `file` only)
  uint32_t file, rule;
};

int g_fail = 0;
#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);     \
      g_fail++;                                                    \
    }                                                              \
  } while (0)

template <class T>
std::unique_ptr<T[]> Exact(const std::vector<T>& v) {  // a heap block of exactly v's size
  std::unique_ptr<T[]> p(new T[v.size()]);
  if (!v.empty()) std::memcpy(p.get(), v.data(), v.size() * sizeof(T));
  return p;
}

void OneBatch(std::mt19937& rng, uint32_t n_files) {
  std::vector<uint64_t> off(n_files + 1, 0);
  std::vector<uint8_t> kind(n_files), mark(n_files);
  const uint32_t lens[] = {0, 0, 1, 5, 16, 17, 100, 1000, 4096, 5000};
  for (uint32_t f = 0; f < n_files; f++) {
    off[f + 1] = off[f] + lens[rng() % 10];
    kind[f] = uint8_t(rng() % 4);
    mark[f] = kind[f] >= 2 ? 1 : kind[f] == 1 ? uint8_t(rng() % 2) : 0;
  }
  auto h_off = Exact(off);
  auto h_kind = Exact(kind);
  auto h_mark = Exact(mark);
  tsg::SplitPlan p;
  std::string err;
  CHECK(tsg::PlanSplit(h_mark.get(), h_kind.get(), h_off.get(), n_files, &p, &err));
  CHECK(p.files_in_place + p.files_changed + p.files_dropped == n_files);
  CHECK(p.bytes_in_place + p.bytes_changed + p.bytes_dropped == off[n_files]);
  CHECK(p.ids.size() == p.files_changed && p.off.size() == p.ids.size() + 1 && p.off.back() == p.bytes_changed);
  for (size_t i = 0; i < p.ids.size(); i++) {
    const uint32_t f = p.ids[i];
    CHECK(f < n_files && mark[f] && kind[f] != 3 && p.kinds[i] == kind[f] && p.src[i] == off[f]);
    CHECK(p.off[i + 1] - p.off[i] == off[f + 1] - off[f]);
    CHECK(i == 0 || p.ids[i - 1] < f);
  }
  // the sub-batch's tail: every second file got candidates and its (shorter) transformed bytes
  std::vector<uint64_t> tail_off(p.ids.size() + 1, 0);
  std::vector<uint8_t> tail_raw(p.ids.size(), 1);
  std::vector<Cand> sub;
  for (size_t i = 0; i < p.ids.size(); i++) {
    uint64_t len = 0;
    if (i % 2 == 0) {
      tail_raw[i] = 0;
      len = (p.off[i + 1] - p.off[i]) / 2;
      sub.push_back(Cand{uint32_t(i), 7});
      sub.push_back(Cand{uint32_t(i), 9});
    }
    tail_off[i + 1] = tail_off[i] + len;
  }
  std::vector<uint8_t> tail_buf(tail_off.back(), 0x5A);
  auto h_tail = Exact(tail_buf);
  std::vector<Cand> sub2 = sub;
  CHECK(tsg::RemapSubCandidates(p, tail_raw, &sub2, &err));
  for (size_t i = 0; i < sub.size(); i++) CHECK(sub2[i].file == p.ids[sub[i].file] && sub2[i].rule == sub[i].rule);
  // in-place candidates: none in a marked file; a stray one is counted and removed
  std::vector<Cand> in_place;
  for (uint32_t f = 0; f < n_files; f++)
    if (!mark[f] && f % 3 == 0) in_place.push_back(Cand{f, 1});
  const size_t n_in_place = in_place.size();
  CHECK(tsg::DropMarkedCandidates(h_mark.get(), n_files, &in_place) == 0 && in_place.size() == n_in_place);
  if (!p.ids.empty()) {
    in_place.insert(in_place.begin(), Cand{p.ids[0], 2});
    in_place.push_back(Cand{n_files, 2});  // (and a file id past the batch)
    CHECK(tsg::DropMarkedCandidates(h_mark.get(), n_files, &in_place) == 2 && in_place.size() == n_in_place);
  }
  // the merge of the views
  std::vector<const uint8_t*> fdata(n_files, nullptr);
  std::vector<uint64_t> flen(n_files, 0);
  std::vector<uint8_t> host_only, sparse(n_files, 1);
  host_only.assign(n_files, 0);
  tsg::MergeChanged(p, h_tail.get(), tail_off, &fdata, &flen, &host_only, &sparse);
  uint64_t sum = 0;
  for (size_t i = 0; i < p.ids.size(); i++) {
    const uint32_t f = p.ids[i];
    CHECK(host_only[f] == 1 && sparse[f] == 0 && fdata[f] == h_tail.get() + tail_off[i]);
    for (uint64_t b = 0; b < flen[f]; b++) sum += fdata[f][b];  // (reads every byte the exact pass may)
    CHECK(flen[f] == tail_off[i + 1] - tail_off[i]);
  }
  CHECK(sum == tail_off.back() * 0x5A);
  for (uint32_t f = 0; f < n_files; f++)
    if (!mark[f] || kind[f] == 3) CHECK(host_only[f] == 0 && sparse[f] == 1 && fdata[f] == nullptr);
  tsg::MergeChanged(p, h_tail.get(), tail_off, &fdata, &flen, &host_only, nullptr);  // (no sparse views)
}

void Refusals() {
  std::string err;
  tsg::SplitPlan p;
  const uint64_t off[3] = {0, 10, 20};
  const struct {
    uint8_t kind[2], mark[2];
  } bad[] = {{{0, 1}, {1, 0}}, {{2, 1}, {0, 0}}, {{3, 0}, {0, 0}}, {{4, 0}, {0, 0}}, {{1, 1}, {2, 0}}};
  for (const auto& b : bad) {
    err.clear();
    CHECK(!tsg::PlanSplit(b.mark, b.kind, off, 2, &p, &err) && !err.empty());
  }
  const uint8_t kind[2] = {1, 2}, mark[2] = {1, 1};
  CHECK(tsg::PlanSplit(mark, kind, off, 2, &p, &err) && p.ids.size() == 2);
  std::vector<Cand> c{Cand{0, 1}, Cand{2, 1}};  // a file id past the sub-batch
  CHECK(!tsg::RemapSubCandidates(p, std::vector<uint8_t>{0, 0}, &c, &err));
  c = {Cand{1, 1}};  // a changed file that came back as read
  CHECK(!tsg::RemapSubCandidates(p, std::vector<uint8_t>{0, 1}, &c, &err));
  CHECK(!tsg::RemapSubCandidates(p, std::vector<uint8_t>{0}, &c, &err));  // a tail of another batch
  CHECK(tsg::PlanSplit(nullptr, nullptr, off, 0, &p, &err) && p.ids.empty() && p.off.size() == 1);
}

}  // namespace

int main() {
  std::mt19937 rng(20261020);
  for (uint32_t n : {0u, 1u, 2u, 3u, 17u, 100u, 1000u, 20000u})
    for (int rep = 0; rep < (n < 1000 ? 50 : 3); rep++) OneBatch(rng, n);
  Refusals();
  std::printf("san_resident_split: %s (%d failed checks)\n", g_fail ? "FAILED" : "ok", g_fail);
  return g_fail ? 1 : 0;
}
