// Stand-alone sanitizer program for the host half of a tar layer resident in HBM
// (trivy_amd/csrc/tar_index_host.h; no GPU, no interpreter, no HIP: the header
// is plain C++): built with -fsanitize=address,undefined
// (tools/san_device_layer.sh) and run on layer files given on the command line.
//
// For every layer:
//  1. the candidate records come from a model of tar_headers_kernel written out
//     here byte by byte (field parse, unsigned and signed sums with the field as
//     spaces), handed over in a shuffled order, in a heap block of exactly their
//     size;
//  2. the walk over them (IndexedTarSrc; the layer stands in for the device, in a
//     heap block of exactly its size, every copy bounds-checked) must give what
//     the walk over the whole layer in host memory (HostTarSrc) gives: the same
//     files, stats and return value, and for a malformed layer the same error;
//  3. a copy that fails (of a block, of an x / L range) ends the walk with
//     failed() set and the copy's error text kept;
//  4. every sub-range plan (PlanTarBatch, TarBatchKinds) has ascending offsets
//     inside the layer, gaps of kind 3, paths inside the pool.
// A layer whose name starts with "bad_" must fail the walk; the others must not.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "tar_index_host.h"

namespace tsg {
static std::string g_err;
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

// tar_headers_kernel's verdict on one block, the slow way.
static bool ModelCandidate(const uint8_t* b) {
  const uint8_t* f = b + 148;
  long long want = 0;
  if (f[0] & 0x80) {
    const bool neg = f[0] & 0x40;
    unsigned long long v = 0;
    for (int i = 0; i < 8; i++) {
      unsigned c = f[i];
      if (i == 0) c &= 0x7F;
      if (neg) c ^= 0xFF;
      if (i == 0 && neg) c &= 0x7F;
      v = (v << 8) | c;
    }
    want = neg ? -static_cast<long long>(v) - 1 : static_cast<long long>(v);
  } else {
    int lo = 0, hi = 8;
    while (lo < hi && (f[lo] == ' ' || f[lo] == 0)) lo++;
    while (hi > lo && (f[hi - 1] == ' ' || f[hi - 1] == 0)) hi--;
    for (int i = lo; i < hi; i++) {
      if (f[i] < '0' || f[i] > '7') return false;
      want = want * 8 + (f[i] - '0');
    }
  }
  long long uns = 0, sgn = 0;
  bool any = false;
  for (int i = 0; i < 512; i++) {
    const uint8_t c = (i >= 148 && i < 156) ? uint8_t(' ') : b[i];
    uns += c;
    sgn += static_cast<int8_t>(c);
    any = any || b[i];
  }
  return any && (want == uns || want == sgn);
}

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

static void Plans(const tsg::TarIndexData& ix, uint64_t n_bytes, std::mt19937& rng) {
  const uint32_t n = uint32_t(ix.files.size());
  std::vector<std::pair<uint32_t, uint32_t>> ranges = {{0, n}, {0, 0}, {n, 0}};
  for (uint32_t i = 0; i < n; i++) ranges.push_back({i, 1});
  for (int k = 0; k < 20 && n; k++) {
    const uint32_t first = rng() % n;
    ranges.push_back({first, uint32_t(rng() % (n - first + 1))});
  }
  for (auto [first, count] : ranges) {
    tsg::TarBatchPlan p;
    tsg::PlanTarBatch(ix, first, count, &p);
    const size_t m = 2 * size_t(count) + 1;
    CHECK(p.offs.size() == m + 1 && p.path_ptrs.size() == m && p.path_lens.size() == m && p.offs[0] == 0);
    CHECK(p.base % 512 == 0 && p.base + p.offs[m] <= n_bytes);
    for (size_t i = 0; i < m; i++) {
      CHECK(p.offs[i] <= p.offs[i + 1]);
      CHECK(p.path_ptrs[i] >= p.path_pool.data() &&
            p.path_ptrs[i] + p.path_lens[i] < p.path_pool.data() + p.path_pool.size());
      CHECK(p.path_ptrs[i][p.path_lens[i]] == '\0');
      if (i & 1) {
        const tsg::TarIndexFile& f = ix.files[first + i / 2];
        CHECK(p.base + p.offs[i] == f.data_off && p.offs[i + 1] - p.offs[i] == f.size);
        CHECK(p.path_ptrs[i][0] == '/' && p.path_lens[i] == f.path_len + 1);
      } else {
        CHECK(p.path_lens[i] == 0);
      }
    }
    p.flags.resize(m);
    for (auto& f : p.flags) f = uint8_t(rng() & 1);
    tsg::TarBatchKinds(&p);
    for (size_t i = 0; i < m; i++) {
      CHECK((i & 1) || p.kinds[i] == 3);
      CHECK(p.binary[i] == (p.kinds[i] == 2));
      if ((i & 1) && !p.flags[i]) CHECK(p.kinds[i] == 1);
      if ((i & 1) && p.flags[i]) CHECK(p.kinds[i] == 2 || p.kinds[i] == 3);
    }
  }
}

int main(int argc, char** argv) {
  std::mt19937 rng(7);
  int n_bad = 0, n_broken = 0;
  for (int a = 1; a < argc; a++) {
    std::ifstream in(argv[a], std::ios::binary);
    CHECK(in.good());
    const std::string bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const uint64_t n = bytes.size();
    std::unique_ptr<uint8_t[]> layer(new uint8_t[n ? n : 1]);  // exactly n: a read past the layer is a finding
    std::memcpy(layer.get(), bytes.data(), n);
    std::vector<tsg::TarRecord> found;
    for (uint64_t b = 0; b < n / 512; b++)
      if (ModelCandidate(layer.get() + 512 * b)) {
        tsg::TarRecord r{};
        r.block = b;
        std::memcpy(r.hdr, layer.get() + 512 * b, 512);
        found.push_back(r);
      }
    std::shuffle(found.begin(), found.end(), rng);
    std::unique_ptr<tsg::TarRecord[]> recs(new tsg::TarRecord[found.size() ? found.size() : 1]);
    std::copy(found.begin(), found.end(), recs.get());
    uint64_t copies = 0;
    tsg::IndexedTarSrc src(recs.get(), found.size(), [&](uint64_t off, uint64_t len, uint8_t* dst) {
      CHECK(off <= n && len <= n - off);
      std::memcpy(dst, layer.get() + off, size_t(len));
      copies++;
      return true;
    });
    tsg::TarIndexData got, want;
    tsg::g_err.clear();
    const int rc_want = tsg::WalkTarIndex(tsg::HostTarSrc{layer.get()}, n, Required, &want);
    const std::string err_want = tsg::g_err;
    tsg::g_err.clear();
    const int rc_got = tsg::WalkTarIndex(src, n, Required, &got);
    const char* name = std::strrchr(argv[a], '/');
    name = name ? name + 1 : argv[a];
    const bool bad = std::strncmp(name, "bad_", 4) == 0;
    CHECK(rc_got == rc_want && tsg::g_err == err_want);
    CHECK((rc_got < 0) == bad);
    if (bad) {
      CHECK(!tsg::g_err.empty());
      n_bad++;
    } else {
      Same(got, want);
      CHECK(src.visited() <= found.size() && src.block_fetches <= 2);
      Plans(got, n, rng);
      // a copy that fails ends the walk as a source failure, with the source's text, not as a malformed archive
      for (const bool fail_blocks : {false, true}) {
        if (fail_blocks ? src.block_fetches == 0 : src.ext_bytes == 0) continue;
        tsg::IndexedTarSrc broken(recs.get(), found.size(), [&](uint64_t off, uint64_t len, uint8_t* dst) {
          CHECK(off <= n && len <= n - off);
          if ((len == 512) == fail_blocks) {
            tsg::SetError("device copy failed");
            return false;
          }
          std::memcpy(dst, layer.get() + off, size_t(len));
          return true;
        });
        tsg::TarIndexData none;
        tsg::g_err.clear();
        CHECK(tsg::WalkTarIndex(broken, n, Required, &none) < 0);
        CHECK(broken.failed() && tsg::g_err == "device copy failed");
        n_broken++;
      }
      CHECK(!src.failed());
    }
    std::printf("%-28s %9llu bytes  %5zu candidates  %5llu off the chain  %4zu files  %llu block fetches  %llu ext bytes  %s\n",
                name, static_cast<unsigned long long>(n), found.size(),
                static_cast<unsigned long long>(found.size() - src.visited()), got.files.size(),
                static_cast<unsigned long long>(src.block_fetches), static_cast<unsigned long long>(src.ext_bytes),
                bad ? tsg::g_err.c_str() : "ok");
  }
  CHECK(argc > 1);
  CHECK(n_broken >= 4);
  std::printf("san_device_layer: %d layers, %d malformed, all as the host walk; %d walks with a failing copy ended as source failures\n",
              argc - 1, n_bad, n_broken);
  return 0;
}
