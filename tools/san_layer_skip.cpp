// Stand-alone sanitizer program for LayerTar's skipDirs / skipFiles in the layer
// walks (tsg_analyzer_set_tar_skip; trivy_amd/csrc/tar_skip.h, analyzer.cpp,
// tar_index_host.h; no GPU, no interpreter): built with
// -fsanitize=address,undefined together with the host sources it calls
// (tools/san_layer_skip.sh) and run on layer files given on the command line.
// Next to every <name>.tar lies <name>.opts: lines "d <pattern>" (skipDirs),
// "f <pattern>" (skipFiles), and what tests/tar_skip_model.py expects --
// "k <files kept and Required>", "s <skipped_dirs> <skipped_files> <under_skipped_dir>".
//
// For every layer, with the options set on an analyzer over a host-only scanner:
//  1. WalkTarIndex (walk mode 0's host half) over the layer in host memory, serially and with its
//     Required pass on four threads, gives the model's counts;
//  2. IndexTarEntries (walk mode 1's host half) over entry records made with the walk's own
//     ChainEntryT / ResolveT, serially and on four threads, gives the same index;
//  3. the host walk, tsg_collector_add_tar -- one large batch; one file a batch; two collectors of
//     different kinds filling in turn (every call indexes again from inside what was read); with
//     walk-ahead on and off -- gives the same files and counts;
//  4. clearing the options gives the unfiltered walk, and the setter's argument errors come first.
// Then four threads, each with an analyzer of its own, run step 3 over all layers at once.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "tar_index_host.h"
#include "tsg_analyzer.h"
#include "tsg_debug.h"
#include "tsg_oracle.h"
#include "tsg_scanner.h"

#define CHECK(x)                                                                                                    \
  do {                                                                                                              \
    if (!(x)) {                                                                                                     \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s (last error: %s)\n", __FILE__, __LINE__, #x, tsg_last_error()); \
      std::exit(1);                                                                                                 \
    }                                                                                                               \
  } while (0)

static tsg_scanner* HostScanner() {
  static const char* kw[] = {"ghp_"};
  static tsg_rule rule{};
  rule.id = "github-pat";
  rule.category = "GitHub";
  rule.title = "GitHub Personal Access Token";
  rule.severity = "CRITICAL";
  rule.regex = "ghp_[0-9a-zA-Z]{36}";
  rule.secret_group_name = "";
  rule.keywords = kw;
  rule.n_keywords = 1;
  tsg_global g{};
  g.rules = &rule;
  g.n_rules = 1;
  tsg_scanner* s = nullptr;
  CHECK(tsg_debug_scanner_host_only(&g, &s) == 0 && s);
  return s;
}

struct Layer {
  std::string name;
  std::unique_ptr<uint8_t[]> bytes;  // a heap block of exactly the layer's size
  uint64_t n = 0;
  tsg::TarSkipOpts opts;
  std::vector<const char*> dirs, files;
  uint64_t kept = 0, counts[3] = {0, 0, 0};
  std::vector<std::string> want;  // the scan paths of the index, from step 1
};

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

static std::vector<std::string> Paths(const tsg::TarIndexData& d) {
  std::vector<std::string> out;
  for (const auto& f : d.files) out.push_back("/" + std::string(d.pool.data() + f.path_off, size_t(f.path_len)));
  return out;
}

static void SameCounts(const tsg::TarSkipCounts& c, const Layer& L) {
  CHECK(c.skipped_dirs == L.counts[0] && c.skipped_files == L.counts[1] && c.under_skipped_dir == L.counts[2]);
}

static void SetOpts(tsg_analyzer* a, const Layer& L) {
  CHECK(tsg_analyzer_set_tar_skip(a, L.dirs.data(), uint32_t(L.dirs.size()), L.files.data(),
                                  uint32_t(L.files.size())) == 0);
}

// The whole layer through the collectors given, filling in turn; the scan paths and this walk's skip counts.
static std::vector<std::string> HostWalk(tsg_analyzer* a, const std::vector<tsg_collector*>& colls, const Layer& L,
                                         tsg_tar_stats* st, tsg::TarSkipCounts* sk) {
  tsg_tar_skip_stats s0{}, s1{};
  s0.struct_size = s1.struct_size = TSG_TAR_SKIP_STATS_SIZE_V1;
  CHECK(tsg_analyzer_tar_skip_stats(a, &s0) == 0);
  std::vector<std::string> out;
  uint64_t cur = 0;
  for (size_t call = 0;; call++) {
    tsg_collector* c = colls[call % colls.size()];
    const int rc = tsg_collector_add_tar(c, L.bytes.get(), L.n, &cur, st);
    CHECK(rc == 0 || rc == 1);
    for (uint32_t i = 0; i < tsg_collector_files(c); i++) {
      const char* p;
      const uint8_t* data;
      uint64_t pl, dl;
      int bin;
      CHECK(tsg_collector_file(c, i, &p, &pl, &data, &dl, &bin) == 0);
      out.emplace_back(p, size_t(pl));
    }
    tsg_collector_reset(c);
    if (rc == 0) break;
  }
  CHECK(tsg_analyzer_walk_end(a) == 0);
  CHECK(tsg_analyzer_tar_skip_stats(a, &s1) == 0);
  sk->skipped_dirs = s1.skipped_dirs - s0.skipped_dirs;
  sk->skipped_files = s1.skipped_files - s0.skipped_files;
  sk->under_skipped_dir = s1.under_skipped_dir - s0.under_skipped_dir;
  return out;
}

static void HostWalks(tsg_analyzer* a, const Layer& L) {
  SetOpts(a, L);
  tsg_collector *big = nullptr, *tiny = nullptr, *as_read = nullptr, *packed = nullptr;
  CHECK(tsg_collector_new(a, 1 << 20, &big) == 0 && tsg_collector_new(a, 64, &tiny) == 0);
  CHECK(tsg_collector_new(a, 2048, &as_read) == 0 && tsg_collector_new(a, 2048, &packed) == 0);
  CHECK(tsg_collector_set_gpu_transform(big, 1) == 0 && tsg_collector_set_gpu_transform(as_read, 1) == 0);
  for (int ahead = 0; ahead < 2; ahead++) {
    CHECK(tsg_analyzer_set_walk_ahead(a, ahead) == 0);
    const std::vector<std::vector<tsg_collector*>> runs = {{big}, {tiny}, {as_read, packed}};
    for (const auto& colls : runs) {
      tsg_tar_stats st{};
      tsg::TarSkipCounts sk;
      CHECK(HostWalk(a, colls, L, &st, &sk) == L.want);
      SameCounts(sk, L);
      CHECK(st.required == L.kept && st.added == L.kept);
    }
  }
  tsg_collector_free(big);
  tsg_collector_free(tiny);
  tsg_collector_free(as_read);
  tsg_collector_free(packed);
}

int main(int argc, char** argv) {
  CHECK(argc > 1);
  tsg_scanner* s = HostScanner();
  tsg_analyzer* a = nullptr;
  CHECK(tsg_analyzer_new(s, "", &a) == 0 && a);
  const char* one[] = {"a"};
  const char* null_pat[] = {nullptr};
  CHECK(tsg_analyzer_set_tar_skip(nullptr, one, 1, one, 1) == -1);
  CHECK(tsg_analyzer_set_tar_skip(a, nullptr, 1, one, 1) == -1 && tsg_analyzer_set_tar_skip(a, one, 1, nullptr, 1) == -1);
  CHECK(tsg_analyzer_set_tar_skip(a, null_pat, 1, nullptr, 0) == -1);
  tsg_tar_skip_stats bad{};
  bad.struct_size = 24;
  CHECK(tsg_analyzer_tar_skip_stats(a, &bad) == -1);

  auto required = [a](const char* p, uint64_t len, int64_t size) { return tsg_analyzer_required(a, p, len, size) == 1; };
  std::vector<Layer> layers(size_t(argc - 1));
  for (int k = 1; k < argc; k++) {
    Layer& L = layers[size_t(k - 1)];
    const std::string path = argv[k];
    const size_t sl = path.rfind('/');
    L.name = path.substr(sl == std::string::npos ? 0 : sl + 1);
    std::ifstream in(path, std::ios::binary);
    CHECK(in.good());
    const std::string bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    L.n = bytes.size();
    L.bytes.reset(new uint8_t[L.n ? L.n : 1]);
    std::memcpy(L.bytes.get(), bytes.data(), L.n);
    std::ifstream oin(path.substr(0, path.size() - 4) + ".opts");
    CHECK(oin.good());
    for (std::string line; std::getline(oin, line);) {
      if (line.size() < 2) continue;
      const std::string v = line.substr(2);
      if (line[0] == 'd') L.opts.dirs.push_back(v);
      if (line[0] == 'f') L.opts.files.push_back(v);
      std::istringstream num(v);
      if (line[0] == 'k') num >> L.kept;
      if (line[0] == 's') num >> L.counts[0] >> L.counts[1] >> L.counts[2];
    }
    for (const auto& p : L.opts.dirs) L.dirs.push_back(p.c_str());
    for (const auto& p : L.opts.files) L.files.push_back(p.c_str());

    // 1. walk mode 0's host half
    const tsg::HostTarSrc src{L.bytes.get()};
    tsg::TarIndexData serial, threaded, plain;
    CHECK(tsg::WalkTarIndex(src, L.n, required, &serial, tsg::SerialFor(), &L.opts) == 0);
    CHECK(tsg::WalkTarIndex(src, L.n, required, &threaded, FourThreads(), &L.opts) == 0);
    CHECK(tsg::WalkTarIndex(src, L.n, required, &plain) == 0);
    L.want = Paths(serial);
    CHECK(L.want.size() == L.kept && Paths(threaded) == L.want);
    SameCounts(serial.skip, L);
    SameCounts(threaded.skip, L);
    CHECK(serial.tar.required == L.kept && serial.tar.regular == plain.tar.regular &&
          serial.tar.whiteouts == plain.tar.whiteouts && serial.tar.opaque_dirs == plain.tar.opaque_dirs);
    CHECK(plain.files.size() == L.kept + L.counts[1] + L.counts[2]);  // (every regular file of these layers is Required)

    // 2. walk mode 1's host half, over records in heap blocks of exactly their size
    std::vector<tsg::tsg_tar_entry_rec> found;
    std::string blob;
    for (uint64_t p = 0;;) {
      tsg::TarEntry e;
      const int r = tsg::ChainEntryT(src, L.n, p, &e);
      CHECK(r >= 0);
      if (r == 1) break;
      const uint8_t* h = tsg::ResolveT(src, &e);
      CHECK(h && !e.bad);
      const std::string_view raw = e.path(L.bytes.get());
      tsg::tsg_tar_entry_rec rec{};
      rec.start = e.start;
      rec.hdr = e.hdr;
      rec.data = e.data;
      rec.size = e.size;
      rec.name_off = blob.size();
      rec.name_len = uint32_t(raw.size());
      rec.typeflag = h[156];
      blob.append(raw.data(), raw.size());
      found.push_back(rec);
      p = e.next;
    }
    std::unique_ptr<tsg::tsg_tar_entry_rec[]> recs(new tsg::tsg_tar_entry_rec[found.size() ? found.size() : 1]);
    std::copy(found.begin(), found.end(), recs.get());
    std::unique_ptr<uint8_t[]> names(new uint8_t[blob.size() ? blob.size() : 1]);
    std::memcpy(names.get(), blob.data(), blob.size());
    tsg::TarIndexData e_serial, e_threaded, e_plain;
    CHECK(tsg::IndexTarEntries(recs.get(), found.size(), names.get(), blob.size(), required, &e_serial, tsg::SerialFor(),
                               nullptr, &L.opts) == 0);
    CHECK(tsg::IndexTarEntries(recs.get(), found.size(), names.get(), blob.size(), required, &e_threaded, FourThreads(),
                               nullptr, &L.opts) == 0);
    CHECK(tsg::IndexTarEntries(recs.get(), found.size(), names.get(), blob.size(), required, &e_plain, FourThreads()) == 0);
    CHECK(Paths(e_serial) == L.want && Paths(e_threaded) == L.want && Paths(e_plain) == Paths(plain));
    SameCounts(e_serial.skip, L);
    SameCounts(e_threaded.skip, L);
    CHECK(e_serial.tar.required == L.kept && e_serial.tar.regular == plain.tar.regular);
    for (size_t i = 0; i < serial.files.size(); i++)
      CHECK(serial.files[i].start == e_threaded.files[i].start && serial.files[i].data_off == e_threaded.files[i].data_off &&
            serial.files[i].size == e_threaded.files[i].size);

    // 3. the host walk; 4. and without the options again
    HostWalks(a, L);
    CHECK(tsg_analyzer_set_tar_skip(a, nullptr, 0, nullptr, 0) == 0);
    tsg_collector* c = nullptr;
    CHECK(tsg_collector_new(a, 1 << 20, &c) == 0);
    tsg_tar_stats st{};
    tsg::TarSkipCounts sk;
    Layer none;
    CHECK(HostWalk(a, {c}, L, &st, &sk) == Paths(plain));
    SameCounts(sk, none);
    tsg_collector_free(c);
    std::printf("%-24s %8llu bytes  %4zu entries  kept %3llu  skipped dirs %2llu files %2llu under %3llu  ok\n",
                L.name.c_str(), static_cast<unsigned long long>(L.n), found.size(),
                static_cast<unsigned long long>(L.kept), static_cast<unsigned long long>(L.counts[0]),
                static_cast<unsigned long long>(L.counts[1]), static_cast<unsigned long long>(L.counts[2]));
  }
  // four analyzers on four threads, all layers each
  std::vector<std::thread> th;
  for (int t = 0; t < 4; t++)
    th.emplace_back([&, t] {
      tsg_analyzer* mine = nullptr;
      CHECK(tsg_analyzer_new(s, "", &mine) == 0 && mine);
      for (size_t k = 0; k < layers.size(); k++) HostWalks(mine, layers[(k + size_t(t)) % layers.size()]);
      tsg_analyzer_free(mine);
    });
  for (auto& x : th) x.join();
  tsg_analyzer_free(a);
  tsg_scanner_free(s);
  std::printf("san_layer_skip: %d layers; both host halves, serially and on four threads, and the host walk (one batch, one "
              "file a batch, re-indexed inside a window; walk-ahead on and off), alone and on four threads, agree with "
              "the model's counts\n", argc - 1);
  return 0;
}
