// Stand-alone sanitizer program for the host half of the forest pass over all
// layers of an image (trivy_amd/csrc/tarforest.h: the virtual block space, the
// cut into passes, the record and name bases; trivy_amd/csrc/tar_index_host.h:
// IndexTarEntries per layer; no GPU, no interpreter, no HIP): built with
// -fsanitize=address,undefined (tools/san_tar_forest.sh) and run on the layer
// files given on the command line, which together are one image.
//
//  1. Per layer the entry records and raw names -- what the GPU half hands over
//     -- are made with the host walk's own ChainEntryT / ResolveT and appended to
//     ONE record buffer and ONE name blob, as the pass lays them out: name_off
//     relative to the layer's first name.  A layer whose name starts with "bad_"
//     must fail the host walk; like an INCOMPLETE layer it hands nothing over.
//     Both buffers are heap blocks of exactly their size.
//  2. From the heads' counts TarForestBases gives every layer's slice; the host
//     half (IndexTarEntries) runs per layer over its slice, the layers one after
//     another and then four layers at a time, each on four threads, and must give
//     what WalkTarIndex gives over that layer alone.
//  3. The virtual block space: every layer's span is whole segments, and
//     TarForestCut cuts a set of layers whose spans exceed 2^31 blocks into
//     passes that each stay below it, without skipping or reordering a layer.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "tar_index_host.h"
#include "tarforest.h"

namespace tsg {
static thread_local std::string g_err;
void SetError(const std::string& e) { g_err = e; }
}  // namespace tsg

#define CHECK(x)                                                                                          \
  do {                                                                                                    \
    if (!(x)) {                                                                                           \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s (last error: %s)\n", __FILE__, __LINE__, #x,          \
                   tsg::g_err.c_str());                                                                   \
      std::exit(1);                                                                                       \
    }                                                                                                     \
  } while (0)

static bool Required(const char* p, uint64_t len, int64_t size) {
  const std::string s(p, size_t(len));
  if (size < 10) return false;
  if (s.size() >= 4 && s.compare(s.size() - 4, 4, ".tar") == 0) return false;
  return s.find("node_modules/") == std::string::npos;
}

static void Same(const tsg::TarIndexData& a, const tsg::TarIndexData& b) {
  CHECK(a.files.size() == b.files.size());
  for (size_t i = 0; i < a.files.size(); i++) {
    const tsg::TarIndexFile &x = a.files[i], &y = b.files[i];
    CHECK(x.start == y.start && x.data_off == y.data_off && x.size == y.size && x.path_len == y.path_len);
    CHECK(std::memcmp(a.pool.data() + x.path_off, b.pool.data() + y.path_off, size_t(x.path_len) + 1) == 0);
  }
  CHECK(std::memcmp(&a.tar, &b.tar, sizeof(a.tar)) == 0);
}

struct FourThreads {
  template <class Fn>
  void operator()(size_t n, Fn&& fn) const {
    std::vector<std::thread> th;
    for (size_t t = 0; t < 4; t++)
      th.emplace_back([&, t] {
        for (size_t i = t; i < n; i += 4) fn(i);
      });
    for (auto& x : th) x.join();
  }
};

struct Head {  // the words of a TarChainHead the host half reads
  uint64_t kind, entries, name_bytes;
};

static void CheckCuts() {
  using namespace tsg;
  for (uint32_t seg : {kTarMinSegment, 64u, kTarDefaultSegment}) {
    CHECK(TarForestSpan(0, seg) == seg && TarForestSpan(100, seg) == seg && TarForestSpan(512, seg) == seg);
    CHECK(TarForestSpan(512ull * seg, seg) == seg && TarForestSpan(512ull * seg + 512, seg) == 2ull * seg);
    // 40 layers of 2^27 blocks: 16 fit a pass less the margin, so every pass takes 15
    std::vector<uint64_t> nb(40, 512ull << 27);
    nb[7] = 0;
    nb[20] = (512ull << 31);  // too large for any pass
    uint32_t first = 0, passes = 0, alone = 0;
    while (first < nb.size()) {
      const uint32_t cnt = TarForestCut(nb.data(), uint32_t(nb.size()), first, seg);
      if (cnt == 0) {
        CHECK(first == 20);
        alone++;
        first++;
        continue;
      }
      uint64_t v = 0;
      for (uint32_t k = first; k < first + cnt; k++) v += TarForestSpan(nb[k], seg);
      CHECK(v + 2 < kTarMaxBlocks);
      if (first + cnt < nb.size() && first + cnt != 20)
        CHECK(v + TarForestSpan(nb[first + cnt], seg) + 2 >= kTarMaxBlocks);  // greedy: the next one did not fit
      passes++;
      first += cnt;
    }
    CHECK(alone == 1 && passes >= 3);
  }
}

int main(int argc, char** argv) {
  CHECK(argc > 1);
  CheckCuts();
  const size_t n_layers = size_t(argc - 1);
  std::vector<std::unique_ptr<uint8_t[]>> layers(n_layers);
  std::vector<uint64_t> sizes(n_layers);
  std::vector<tsg::TarIndexData> want(n_layers);
  std::vector<Head> heads(n_layers);
  std::vector<tsg::tsg_tar_entry_rec> all_recs;
  std::string all_names;
  size_t n_bad = 0;
  for (size_t k = 0; k < n_layers; k++) {
    std::ifstream in(argv[k + 1], std::ios::binary);
    CHECK(in.good());
    const std::string bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const uint64_t n = sizes[k] = bytes.size();
    layers[k].reset(new uint8_t[n ? n : 1]);
    std::memcpy(layers[k].get(), bytes.data(), n);
    const tsg::HostTarSrc src{layers[k].get()};
    const char* name = std::strrchr(argv[k + 1], '/');
    name = name ? name + 1 : argv[k + 1];
    const bool bad = std::strncmp(name, "bad_", 4) == 0;
    tsg::g_err.clear();
    CHECK((tsg::WalkTarIndex(src, n, Required, &want[k]) < 0) == bad);
    heads[k] = Head{bad ? 1u : 0u, 0, 0};
    if (bad) {  // INCOMPLETE: nothing handed over
      n_bad++;
      continue;
    }
    const size_t name_base = all_names.size();
    for (uint64_t p = 0;;) {
      tsg::TarEntry e;
      const int r = tsg::ChainEntryT(src, n, p, &e);
      CHECK(r >= 0);
      if (r == 1) break;
      const uint8_t* h = tsg::ResolveT(src, &e);
      CHECK(h && !e.bad);
      const std::string_view raw = e.path(layers[k].get());
      tsg::tsg_tar_entry_rec rec{};
      rec.start = e.start;
      rec.hdr = e.hdr;
      rec.data = e.data;
      rec.size = e.size;
      rec.name_off = all_names.size() - name_base;  // relative to the layer's first name
      rec.name_len = uint32_t(raw.size());
      rec.typeflag = h[156];
      rec.flags = e.has_pax_path ? tsg::kTarNamePax : e.long_len != ~uint64_t(0) ? tsg::kTarNameLong : 0;
      all_names.append(raw.data(), raw.size());
      all_recs.push_back(rec);
      heads[k].entries++;
      p = e.next;
    }
    heads[k].name_bytes = all_names.size() - name_base;
  }
  // the two shared buffers, in heap blocks of exactly their size
  std::unique_ptr<tsg::tsg_tar_entry_rec[]> recs(new tsg::tsg_tar_entry_rec[all_recs.size() ? all_recs.size() : 1]);
  std::copy(all_recs.begin(), all_recs.end(), recs.get());
  std::unique_ptr<uint8_t[]> names(new uint8_t[all_names.size() ? all_names.size() : 1]);
  std::memcpy(names.get(), all_names.data(), all_names.size());
  std::vector<uint64_t> rec_base, name_base;
  constexpr size_t kStride = sizeof(Head) / 8;
  tsg::TarForestBases(&heads[0].entries, kStride, uint32_t(n_layers), &rec_base);
  tsg::TarForestBases(&heads[0].name_bytes, kStride, uint32_t(n_layers), &name_base);
  CHECK(rec_base[n_layers] == all_recs.size() && name_base[n_layers] == all_names.size());

  auto index_layer = [&](size_t k, bool threaded, tsg::TarIndexData* d) {
    if (heads[k].kind != 0) return;  // left to the host walk
    const tsg::tsg_tar_entry_rec* r = recs.get() + rec_base[k];
    const uint8_t* nm = names.get() + name_base[k];
    double ms[3];
    if (threaded)
      CHECK(tsg::IndexTarEntries(r, heads[k].entries, nm, heads[k].name_bytes, Required, d, FourThreads(), ms) == 0);
    else
      CHECK(tsg::IndexTarEntries(r, heads[k].entries, nm, heads[k].name_bytes, Required, d) == 0);
  };
  std::vector<tsg::TarIndexData> serial(n_layers), threaded(n_layers);
  for (size_t k = 0; k < n_layers; k++) index_layer(k, false, &serial[k]);
  FourThreads()(n_layers, [&](size_t k) { index_layer(k, true, &threaded[k]); });  // four layers side by side
  size_t files = 0;
  for (size_t k = 0; k < n_layers; k++) {
    if (heads[k].kind != 0) continue;
    Same(serial[k], want[k]);
    Same(threaded[k], want[k]);
    files += want[k].files.size();
  }
  // a layer's slice one name byte short is refused, with nothing read past the blob
  for (size_t k = n_layers; k-- > 0;) {
    if (heads[k].kind != 0 || heads[k].name_bytes == 0 || recs[rec_base[k + 1] - 1].name_len == 0) continue;
    std::unique_ptr<uint8_t[]> shorter(new uint8_t[heads[k].name_bytes - 1 ? heads[k].name_bytes - 1 : 1]);
    std::memcpy(shorter.get(), names.get() + name_base[k], heads[k].name_bytes - 1);
    tsg::TarIndexData none;
    tsg::g_err.clear();
    CHECK(tsg::IndexTarEntries(recs.get() + rec_base[k], heads[k].entries, shorter.get(), heads[k].name_bytes - 1,
                               Required, &none, FourThreads()) < 0);
    CHECK(tsg::g_err.find("outside the name blob") != std::string::npos);
    break;
  }
  std::printf("san_tar_forest: %zu layers in one image (%zu left to the host walk), %zu records, %zu name bytes, %zu files; "
              "the per-layer host half over the shared buffers equals the host walk, serially and four layers at a time "
              "on four threads each; the cuts into passes stay below 2^31 virtual blocks\n",
              n_layers, n_bad, all_recs.size(), all_names.size(), files);
  return 0;
}
