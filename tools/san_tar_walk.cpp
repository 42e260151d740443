// Stand-alone sanitizer program for the host half of the GPU chain walk of a
// resident tar layer (trivy_amd/csrc/tar_index_host.h: IndexTarEntries; the
// records: trivy_amd/csrc/tarchain.h; no GPU, no interpreter, no HIP): built with
// -fsanitize=address,undefined (tools/san_tar_walk.sh) and run on layer files
// given on the command line.
//
// For every layer:
//  1. the entry records and the raw names -- what the GPU half hands over -- are
//     made here with the host walk's own ChainEntryT / ResolveT over the layer in
//     host memory, and handed over in heap blocks of exactly their size;
//  2. IndexTarEntries over them, serially and on four threads, must give what
//     WalkTarIndex gives over the whole layer: the same files, paths, spans and
//     tar stats;
//  3. a name blob that is one byte short is refused, with nothing read past it.
// A layer whose name starts with "bad_" must fail the host walk; it has no
// records to hand over (the GPU walk stops INCOMPLETE and the host walk runs).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "tar_index_host.h"

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

int main(int argc, char** argv) {
  int n_bad = 0;
  for (int a = 1; a < argc; a++) {
    std::ifstream in(argv[a], std::ios::binary);
    CHECK(in.good());
    const std::string bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const uint64_t n = bytes.size();
    std::unique_ptr<uint8_t[]> layer(new uint8_t[n ? n : 1]);
    std::memcpy(layer.get(), bytes.data(), n);
    const tsg::HostTarSrc src{layer.get()};
    const char* name = std::strrchr(argv[a], '/');
    name = name ? name + 1 : argv[a];
    const bool bad = std::strncmp(name, "bad_", 4) == 0;
    tsg::TarIndexData want;
    tsg::g_err.clear();
    const int rc_want = tsg::WalkTarIndex(src, n, Required, &want);
    CHECK((rc_want < 0) == bad);
    if (bad) {
      CHECK(!tsg::g_err.empty());
      std::printf("%-28s %9llu bytes  malformed: %s\n", name, static_cast<unsigned long long>(n), tsg::g_err.c_str());
      n_bad++;
      continue;
    }
    // the GPU half's output, from the host walk's own reading of the chain
    std::vector<tsg::tsg_tar_entry_rec> found;
    std::string blob;
    for (uint64_t p = 0;;) {
      tsg::TarEntry e;
      const int r = tsg::ChainEntryT(src, n, p, &e);
      CHECK(r >= 0);
      if (r == 1) break;
      const uint8_t* h = tsg::ResolveT(src, &e);
      CHECK(h && !e.bad);
      const std::string_view raw = e.path(layer.get());
      tsg::tsg_tar_entry_rec rec{};
      rec.start = e.start;
      rec.hdr = e.hdr;
      rec.data = e.data;
      rec.size = e.size;
      rec.name_off = blob.size();
      rec.name_len = uint32_t(raw.size());
      rec.typeflag = h[156];
      rec.flags = e.has_pax_path ? tsg::kTarNamePax : e.long_len != ~uint64_t(0) ? tsg::kTarNameLong : 0;
      blob.append(raw.data(), raw.size());
      found.push_back(rec);
      p = e.next;
    }
    std::unique_ptr<tsg::tsg_tar_entry_rec[]> recs(new tsg::tsg_tar_entry_rec[found.size() ? found.size() : 1]);
    std::copy(found.begin(), found.end(), recs.get());
    std::unique_ptr<uint8_t[]> names(new uint8_t[blob.size() ? blob.size() : 1]);
    std::memcpy(names.get(), blob.data(), blob.size());
    tsg::TarIndexData serial, threaded;
    double ms[3];
    CHECK(tsg::IndexTarEntries(recs.get(), found.size(), names.get(), blob.size(), Required, &serial) == 0);
    CHECK(tsg::IndexTarEntries(recs.get(), found.size(), names.get(), blob.size(), Required, &threaded, FourThreads(), ms) == 0);
    Same(serial, want);
    Same(threaded, want);
    if (!blob.empty() && found.back().name_len) {
      std::unique_ptr<uint8_t[]> shorter(new uint8_t[blob.size() - 1 ? blob.size() - 1 : 1]);
      std::memcpy(shorter.get(), blob.data(), blob.size() - 1);
      tsg::TarIndexData none;
      tsg::g_err.clear();
      CHECK(tsg::IndexTarEntries(recs.get(), found.size(), shorter.get(), blob.size() - 1, Required, &none, FourThreads()) < 0);
      CHECK(tsg::g_err.find("outside the name blob") != std::string::npos);
    }
    std::printf("%-28s %9llu bytes  %5zu entries  %7zu name bytes  %4zu files  ok\n", name,
                static_cast<unsigned long long>(n), found.size(), blob.size(), want.files.size());
  }
  CHECK(argc > 1);
  std::printf("san_tar_walk: %d layers, %d malformed (left to the host walk); the host half over entry records equals "
              "the host walk, serially and on four threads\n", argc - 1, n_bad);
  return 0;
}
