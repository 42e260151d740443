// Stand-alone sanitizer program for the host half behind the GPU's path classify and
// Required of a resident tar layer (trivy_amd/csrc/tar_required_host.h: IndexTarFiles; the
// records: trivy_amd/csrc/tarrequired.h; no GPU, no interpreter, no HIP): built with
// -fsanitize=address,undefined (tools/san_tar_required.sh) and run on layer files given
// on the command line.
//
// Beside every <name>.tar the script has written what the device stage hands over for it,
// made by the tests' model (tests/tar_required_model.py) without allow-path tables, so that
// every file that reaches the allow paths is asked about: <name>.frecs (48-B file records),
// <name>.blob (the paths) and <name>.counts (16 words).  For every layer:
//  1. the entry records and raw names are made with the host walk's own ChainEntryT /
//     ResolveT, and IndexTarEntries over them gives the index mode 1 builds;
//  2. IndexTarFiles over the model's output, handed over in heap blocks of exactly their
//     size, serially and on four threads, must give the same index: files, spans, paths,
//     the pool byte for byte, the tar stats;
//  3. a blob that is one byte short, and counts that contradict the records, are refused
//     with nothing read past the blocks.
// Required here is analyzer.cpp's up to the allow paths, which are a stand-in without a
// regex engine: the host half only ever calls them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "tar_required_host.h"

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

static bool Allow(const char* p, uint64_t len) {
  const std::string_view s(p, size_t(len));
  return s.find("example") != std::string_view::npos || s.find("/vendor/") != std::string_view::npos ||
         (s.size() >= 3 && s.substr(s.size() - 3) == ".md");
}

static bool Required(const char* path, uint64_t len, int64_t size) {  // analyzer.cpp, with Allow for the scanner's
  if (size < 10) return false;
  const std::string_view fp(path, size_t(len));
  const size_t slash = fp.rfind('/');
  const std::string dir = "/" + std::string(slash == std::string_view::npos ? std::string_view() : fp.substr(0, slash + 1));
  const std::string_view name = slash == std::string_view::npos ? fp : fp.substr(slash + 1);
  if (dir.find("/.git/") != std::string::npos || dir.find("/node_modules/") != std::string::npos) return false;
  for (const char* f : {"go.mod", "go.sum", "package-lock.json", "yarn.lock", "pnpm-lock.yaml", "Pipfile.lock",
                        "Gemfile.lock"})
    if (name == f) return false;
  if (fp == ".") return false;  // the config base of an analyzer without a config
  const size_t dot = name.rfind('.');
  if (dot != std::string_view::npos && name.size() - dot <= 7)
    for (const char* x : {".jpg", ".png", ".gif", ".doc", ".pdf", ".bin", ".svg", ".socket", ".deb", ".rpm", ".zip",
                          ".gz", ".gzip", ".tar"})
      if (name.substr(dot) == x) return false;
  return !Allow(path, len);
}

static void Same(const tsg::TarIndexData& a, const tsg::TarIndexData& b) {
  CHECK(a.files.size() == b.files.size());
  for (size_t i = 0; i < a.files.size(); i++) {
    const tsg::TarIndexFile &x = a.files[i], &y = b.files[i];
    CHECK(x.start == y.start && x.data_off == y.data_off && x.size == y.size && x.path_len == y.path_len);
    CHECK(x.path_off == y.path_off);
  }
  CHECK(a.pool == b.pool);
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

static std::string ReadFile(const std::string& path) {
  std::ifstream in(path, std::ios::binary);
  CHECK(in.good());
  return std::string((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

// A heap block of exactly n bytes (one when n is 0), so that a read past it is seen.
static std::unique_ptr<uint8_t[]> Exact(const void* p, size_t n) {
  std::unique_ptr<uint8_t[]> b(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(b.get(), p, n);
  return b;
}

template <class Par>
static int Files(const uint8_t* recs, size_t n_recs, const uint8_t* blob, size_t blob_bytes, const tsg::TarRequiredCounts& cnt,
                 tsg::TarIndexData* out, Par&& par, tsg::TarRequiredHostStats* hs) {
  return tsg::IndexTarFiles(
      reinterpret_cast<const tsg::tsg_tar_file_rec*>(recs), n_recs, blob, blob_bytes, cnt,
      [](const char* p, uint64_t len, uint64_t) { return Allow(p, len); }, Allow, Required, out, par, hs);
}

int main(int argc, char** argv) {
  size_t adopted = 0;
  for (int a = 1; a < argc; a++) {
    const std::string tar_path = argv[a], stem = tar_path.substr(0, tar_path.size() - 4);
    const std::string bytes = ReadFile(tar_path);
    const uint64_t n = bytes.size();
    const std::unique_ptr<uint8_t[]> layer = Exact(bytes.data(), n);
    const tsg::HostTarSrc src{layer.get()};
    const char* name = std::strrchr(argv[a], '/');
    name = name ? name + 1 : argv[a];
    // mode 1's index, from the host walk's own reading of the chain
    std::vector<tsg::tsg_tar_entry_rec> found;
    std::string names;
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
      rec.name_off = names.size();
      rec.name_len = uint32_t(raw.size());
      rec.typeflag = h[156];
      names.append(raw.data(), raw.size());
      found.push_back(rec);
      p = e.next;
    }
    tsg::TarIndexData want;
    CHECK(tsg::IndexTarEntries(found.data(), found.size(), reinterpret_cast<const uint8_t*>(names.data()), names.size(),
                               Required, &want) == 0);
    // what the device stage handed over
    const std::string frecs = ReadFile(stem + ".frecs"), blob = ReadFile(stem + ".blob"), counts = ReadFile(stem + ".counts");
    CHECK(frecs.size() % sizeof(tsg::tsg_tar_file_rec) == 0 && counts.size() == sizeof(tsg::TarRequiredCounts));
    tsg::TarRequiredCounts cnt;
    std::memcpy(&cnt, counts.data(), sizeof(cnt));
    CHECK(cnt.entries == found.size());
    const size_t n_recs = frecs.size() / sizeof(tsg::tsg_tar_file_rec);
    const std::unique_ptr<uint8_t[]> r_block = Exact(frecs.data(), frecs.size()), b_block = Exact(blob.data(), blob.size());
    tsg::TarIndexData serial, threaded;
    tsg::TarRequiredHostStats hs, ht;
    CHECK(Files(r_block.get(), n_recs, b_block.get(), blob.size(), cnt, &serial, tsg::SerialFor(), &hs) == 0);
    CHECK(Files(r_block.get(), n_recs, b_block.get(), blob.size(), cnt, &threaded, FourThreads(), &ht) == 0);
    Same(serial, want);
    Same(threaded, want);
    CHECK(hs.ask_dropped == ht.ask_dropped && hs.adopted == ht.adopted);
    adopted += hs.adopted;
    if (!blob.empty()) {
      const std::unique_ptr<uint8_t[]> shorter = Exact(blob.data(), blob.size() - 1);
      tsg::TarIndexData none;
      tsg::g_err.clear();
      CHECK(Files(r_block.get(), n_recs, shorter.get(), blob.size() - 1, cnt, &none, FourThreads(), nullptr) < 0);
      CHECK(tsg::g_err.find("counts contradict") != std::string::npos);
      tsg::TarRequiredCounts less = cnt;
      less.path_bytes--;
      tsg::g_err.clear();
      CHECK(Files(r_block.get(), n_recs, shorter.get(), blob.size() - 1, less, &none, FourThreads(), nullptr) < 0);
      CHECK(tsg::g_err.find("outside the path blob") != std::string::npos);
    }
    std::printf("%-28s %9llu bytes  %5zu entries  %5zu file records  %7zu path bytes  %4zu asked and dropped  %4zu files  %s  ok\n",
                name, static_cast<unsigned long long>(n), found.size(), n_recs, blob.size(), size_t(hs.ask_dropped),
                want.files.size(), hs.adopted ? "adopted  " : "compacted");
  }
  CHECK(argc > 1);
  std::printf("san_tar_required: %d layers (%zu adopted the blob as the pool); the host half over file records equals the "
              "host half over entry records, serially and on four threads\n", argc - 1, adopted);
  return 0;
}
