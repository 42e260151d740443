// Stand-alone sanitizer program for the host side of LayerTar's skip options in the GPU's
// Required stage of a resident tar layer (tsg_analyzer_set_tar_required_skip; no GPU, no
// interpreter, no HIP): the pattern classifier and the matcher the kernels share
// (trivy_amd/csrc/tar_skip_dev.h) and the extended host half (trivy_amd/csrc/tar_required_host.h:
// IndexTarFiles with skip options).  Built with -fsanitize=address,undefined
// (tools/san_tar_required_skip.sh) and run on layer files given on the command line.
//
// Beside every <name>.tar the script has written the layer's options (<name>.dirs, <name>.files:
// a cleaned pattern per line) and what the device stage hands over for it with them, made by
// the tests' model (tests/tar_required_skip_model.py) without allow-path tables: <name>.frecs,
// <name>.blob, <name>.counts; <name>.fallback exists when an asked name is a skipped
// directory.  patterns.txt beside them holds a pattern per line, preceded by '+' when the device
// takes it and '-' when it does not.  For every layer:
//  1. the entry records and raw names are made with the host walk's own ChainEntryT / ResolveT,
//     and IndexTarEntries over them with the options gives the index and the skip counts of
//     mode 1's host half;
//  2. the matcher, given every cleaned name in a heap block of exactly its size, must say what
//     SkipPath says for the directory and the file patterns;
//  3. IndexTarFiles over the model's output with the options, handed over in heap blocks of
//     exactly their size, serially and on four threads, must give the same index and counts --
//     or 1 with nothing added for a <name>.fallback layer;
//  4. without the options the same records are refused.
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
  return s.find("example") != std::string_view::npos || (s.size() >= 3 && s.substr(s.size() - 3) == ".md");
}
static bool Required(const char* path, uint64_t len, int64_t size) {  // the part of analyzer.cpp's these layers reach
  if (size < 10 || std::string_view(path, size_t(len)) == ".") return false;
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
  CHECK(a.skip.skipped_dirs == b.skip.skipped_dirs && a.skip.skipped_files == b.skip.skipped_files &&
        a.skip.under_skipped_dir == b.skip.under_skipped_dir);
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
static std::vector<std::string> Lines(const std::string& text) {
  std::vector<std::string> out;
  for (size_t at = 0; at < text.size();) {
    const size_t nl = text.find('\n', at);
    out.push_back(text.substr(at, nl - at));
    at = nl == std::string::npos ? text.size() : nl + 1;
  }
  return out;
}

// A heap block of exactly n bytes (one when n is 0), so that a read past it is seen.
static std::unique_ptr<uint8_t[]> Exact(const void* p, size_t n) {
  std::unique_ptr<uint8_t[]> b(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(b.get(), p, n);
  return b;
}

template <class Par>
static int Files(const uint8_t* recs, size_t n_recs, const uint8_t* blob, size_t blob_bytes, const tsg::TarRequiredCounts& cnt,
                 tsg::TarIndexData* out, Par&& par, tsg::TarRequiredHostStats* hs, const tsg::TarSkipOpts* skip) {
  return tsg::IndexTarFiles(
      reinterpret_cast<const tsg::tsg_tar_file_rec*>(recs), n_recs, blob, blob_bytes, cnt,
      [](const char* p, uint64_t len, uint64_t) { return Allow(p, len); }, Allow, Required, out, par, hs, skip);
}

static void Classifier(const std::string& path) {
  size_t taken = 0, refused = 0;
  for (const std::string& line : Lines(ReadFile(path))) {
    CHECK(!line.empty() && (line[0] == '+' || line[0] == '-'));
    // the pattern in a block of exactly its size: the classifier reads no byte past it
    const std::unique_ptr<uint8_t[]> block = Exact(line.data() + 1, line.size() - 1);
    uint8_t form = 0;
    std::string_view lit;
    const bool ok = tsg::TarSkipForm(std::string_view(reinterpret_cast<const char*>(block.get()), line.size() - 1), &form, &lit);
    CHECK(ok == (line[0] == '+'));
    tsg::TarSkipTable t;
    CHECK(tsg::TarSkipClassify({line.substr(1)}, {}, &t) == ok && tsg::TarSkipClassify({}, {line.substr(1)}, &t) == ok);
    (ok ? taken : refused)++;
  }
  CHECK(taken && refused);
  // the caps: 32 of a kind, 2 KiB of literals
  std::vector<std::string> many(33, "d"), big(9, std::string(255, 'a'));
  tsg::TarSkipTable t;
  CHECK(!tsg::TarSkipClassify(many, {}, &t) && !tsg::TarSkipClassify({}, many, &t) && !tsg::TarSkipClassify(big, {}, &t));
  many.pop_back();
  big.pop_back();
  CHECK(tsg::TarSkipClassify(many, many, &t) && t.n_dir == 32 && t.n_file == 32);
  CHECK(tsg::TarSkipClassify(big, std::vector<std::string>(8, "x"), &t) && !tsg::TarSkipClassify(big, std::vector<std::string>(9, "x"), &t));
  std::printf("%-28s %zu patterns taken, %zu refused, the caps  ok\n", "patterns.txt", taken, refused);
}

int main(int argc, char** argv) {
  CHECK(argc > 2);
  Classifier(argv[1]);
  size_t fell_back = 0;
  for (int a = 2; a < argc; a++) {
    const std::string tar_path = argv[a], stem = tar_path.substr(0, tar_path.size() - 4);
    const std::string bytes = ReadFile(tar_path);
    const uint64_t n = bytes.size();
    const std::unique_ptr<uint8_t[]> layer = Exact(bytes.data(), n);
    const tsg::HostTarSrc src{layer.get()};
    const char* name = std::strrchr(argv[a], '/');
    name = name ? name + 1 : argv[a];
    tsg::TarSkipOpts opts;
    opts.dirs = Lines(ReadFile(stem + ".dirs"));
    opts.files = Lines(ReadFile(stem + ".files"));
    opts.Classify();
    CHECK(opts.any() && opts.dev_ok);
    const bool fallback = std::ifstream(stem + ".fallback").good();
    std::vector<tsg::tsg_tar_entry_rec> found;
    std::string names;
    size_t matched = 0;
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
      // the matcher against SkipPath on the cleaned name, in a block of exactly its size
      tsg::ClassifyPath(h[156], layer.get(), &e);
      const std::string_view fp = e.path(layer.get());
      if (fp.empty() || fp == "." || fp.substr(0, 2) == "..") continue;  // (names the device does not decide)
      const std::unique_ptr<uint8_t[]> block = Exact(fp.data(), fp.size());
      for (int files = 0; files < 2; files++) {
        const bool got = tsg::TarSkipMatch(&opts.dev, files != 0, block.get(), uint32_t(fp.size()));
        CHECK(got == tsg::SkipPath(fp, files ? opts.files : opts.dirs));
        matched += got;
      }
    }
    tsg::TarIndexData want;
    CHECK(tsg::IndexTarEntries(found.data(), found.size(), reinterpret_cast<const uint8_t*>(names.data()), names.size(),
                               Required, &want, tsg::SerialFor(), nullptr, &opts) == 0);
    const std::string frecs = ReadFile(stem + ".frecs"), blob = ReadFile(stem + ".blob"), counts = ReadFile(stem + ".counts");
    CHECK(frecs.size() % sizeof(tsg::tsg_tar_file_rec) == 0 && counts.size() == sizeof(tsg::TarRequiredCounts));
    tsg::TarRequiredCounts cnt;
    std::memcpy(&cnt, counts.data(), sizeof(cnt));
    CHECK(cnt.entries == found.size());
    const size_t n_recs = frecs.size() / sizeof(tsg::tsg_tar_file_rec);
    const std::unique_ptr<uint8_t[]> r_block = Exact(frecs.data(), frecs.size()), b_block = Exact(blob.data(), blob.size());
    tsg::TarIndexData serial, threaded;
    tsg::TarRequiredHostStats hs, ht;
    const int rc = Files(r_block.get(), n_recs, b_block.get(), blob.size(), cnt, &serial, tsg::SerialFor(), &hs, &opts);
    CHECK(rc == Files(r_block.get(), n_recs, b_block.get(), blob.size(), cnt, &threaded, FourThreads(), &ht, &opts));
    CHECK(rc == (fallback ? 1 : 0));
    if (fallback) {
      CHECK(serial.files.empty() && serial.pool.empty() && serial.tar.entries == 0 && serial.skip.skipped_dirs == 0);
      fell_back++;
    } else {
      Same(serial, want);
      Same(threaded, want);
      CHECK(hs.ask_dropped == ht.ask_dropped && hs.adopted == ht.adopted);
      CHECK(hs.skip.skipped_dirs == want.skip.skipped_dirs && hs.skip.under_skipped_dir == want.skip.under_skipped_dir);
    }
    if (cnt.pad[0] | cnt.pad[1]) {  // without the options the records of a skip stage are refused
      tsg::TarIndexData none;
      tsg::g_err.clear();
      CHECK(Files(r_block.get(), n_recs, b_block.get(), blob.size(), cnt, &none, FourThreads(), nullptr, nullptr) < 0);
      CHECK(tsg::g_err.find("counts contradict") != std::string::npos);
    }
    std::printf("%-28s %7llu bytes  %4zu entries  %4zu file records  %3zu pattern hits  dirs %llu files %llu under %llu  "
                "%4zu files  %s  ok\n",
                name, static_cast<unsigned long long>(n), found.size(), n_recs, matched,
                static_cast<unsigned long long>(want.skip.skipped_dirs), static_cast<unsigned long long>(want.skip.skipped_files),
                static_cast<unsigned long long>(want.skip.under_skipped_dir), want.files.size(),
                fallback ? "falls back" : hs.adopted ? "adopted   " : "compacted ");
  }
  std::printf("san_tar_required_skip: %d layers (%zu fall back on an asked name); the classifier, the matcher against SkipPath, "
              "and the host half over a skip stage's records against the host half over entry records, serially and on "
              "four threads\n", argc - 2, fell_back);
  return 0;
}
