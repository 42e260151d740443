// Stand-alone sanitizer program for the host code of device-only batches (no
// GPU, no interpreter): built with -fsanitize=address,undefined together with
// the host sources it calls (tools/san_device_only.sh) and run as it is.
//
//  1. argument validation: tsg_scan / tsg_scan_ext / the submit forms on a
//     scanner without a GPU engine -- the batch errors come back first, valid
//     batches (mirrored, device-only, device-only with a transform) stop at
//     "no GPU engine"; tsg_result_fetch_stats refuses unknown sizes;
//  2. offset tables: PlanFetchOnHost over random batches -- every fetched file
//     inside the buffer, 16-B aligned, no two overlapping, packed before direct;
//  3. buffer growth and retirement: FetchPool over malloc / free, every buffer
//     written to its capacity while on loan, nothing freed twice or leaked.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "fetch_host.h"
#include "tsg_debug.h"
#include "tsg_oracle.h"
#include "tsg_scanner.h"

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                                    \
    }                                                                  \
  } while (0)

static bool Has(const char* text, const char* what) { return std::strstr(text, what) != nullptr; }

static void ArgumentValidation() {
  const char* kw[] = {"akia"};
  tsg_rule rule{};
  rule.id = "aws-access-key-id";
  rule.category = "AWS";
  rule.title = "AWS Access Key ID";
  rule.severity = "CRITICAL";
  rule.regex = "AKIA[A-Z0-9]{16}";
  rule.secret_group_name = "";
  rule.keywords = kw;
  rule.n_keywords = 1;
  tsg_global g{};
  g.rules = &rule;
  g.n_rules = 1;
  tsg_scanner* s = nullptr;
  CHECK(tsg_debug_scanner_host_only(&g, &s) == 0 && s);

  std::vector<uint8_t> arena(64, ' ');
  const uint64_t offs[3] = {0, 8, 16};
  const char* paths[2] = {"a.txt", "b.txt"};
  const uint8_t kinds[2] = {1, 0};
  const uint64_t gsrc[2] = {0, 8};
  const void* fake_dev = reinterpret_cast<const void*>(uintptr_t(0x700000000000ull));  // never dereferenced
  auto batch = [&](const uint8_t* host, const void* dev) {
    tsg_batch b{};
    b.n_files = 2;
    b.host_arena = host;
    b.host_offsets = offs;
    b.dev_arena = dev;
    b.paths = paths;
    return b;
  };
  tsg_result* r = nullptr;
  tsg_pending* p = nullptr;

  tsg_batch b = batch(nullptr, nullptr);  // no bytes anywhere
  CHECK(tsg_scan(s, &b, &r) < 0 && !r && Has(tsg_last_error(), "host_arena is NULL"));
  CHECK(tsg_scan_submit(s, &b, &p) < 0 && !p && Has(tsg_last_error(), "host_arena is NULL"));
  tsg_batch_ext e{};
  e.struct_size = TSG_BATCH_EXT_SIZE;
  e.base = b;
  CHECK(tsg_scan_ext(s, &e, &r) < 0 && !r && Has(tsg_last_error(), "host_arena is NULL"));
  CHECK(tsg_scan_submit_ext(s, &e, &p) < 0 && !p && Has(tsg_last_error(), "host_arena is NULL"));

  e.base = batch(nullptr, fake_dev);  // gathered and resident at once
  e.base.transform = kinds;
  e.gather_base = arena.data();
  e.gather_src = gsrc;
  CHECK(tsg_scan_ext(s, &e, &r) < 0 && !r && Has(tsg_last_error(), "no dev_arena"));

  b = batch(arena.data(), nullptr);
  b.host_offsets = nullptr;
  CHECK(tsg_scan(s, &b, &r) < 0 && !r && Has(tsg_last_error(), "host_offsets is required"));

  e = tsg_batch_ext{};
  e.struct_size = TSG_BATCH_EXT_SIZE + 8;
  CHECK(tsg_scan_ext(s, &e, &r) < 0 && !r && Has(tsg_last_error(), "struct_size"));

  // valid batches reach the scanner, which has no engine
  for (int k = 0; k < 4; k++) {
    b = batch(k < 2 ? arena.data() : nullptr, k >= 1 ? fake_dev : nullptr);
    if (k == 3) b.transform = kinds;
    CHECK(tsg_scan(s, &b, &r) < 0 && !r && Has(tsg_last_error(), "no GPU engine"));
    CHECK(tsg_scan_submit(s, &b, &p) == 0 && p);
    CHECK(tsg_scan_wait(p, &r) < 0 && !r && Has(tsg_last_error(), "no GPU engine"));
    p = nullptr;
  }

  tsg_fetch_stats fs{};
  for (uint32_t bogus : {0u, 8u, TSG_FETCH_STATS_SIZE_V1 - 8, TSG_FETCH_STATS_SIZE_V1 + 8, 0xFFFFFFFFu}) {
    fs.struct_size = bogus;
    fs.files = 7;
    CHECK(tsg_result_fetch_stats(reinterpret_cast<const tsg_result*>(arena.data()), &fs) < 0 && fs.files == 7);
  }
  fs.struct_size = TSG_FETCH_STATS_SIZE_V1;
  CHECK(tsg_result_fetch_stats(nullptr, &fs) < 0);
  CHECK(tsg_debug_scanner_fetch(s, 1 << 20, 1 << 20) == -1);  // no engine to set it on
  CHECK(tsg_debug_scanner_fetch(nullptr, 1 << 20, 1 << 20) == -1);
  tsg_scanner_free(s);
}

static void OffsetTables() {
  std::mt19937_64 rng(7);
  for (int round = 0; round < 400; round++) {
    const uint32_t n = uint32_t(rng() % 70);
    const uint64_t direct = round % 5 == 0 ? 1 : (round % 3 == 0 ? 40 : 4096);
    std::vector<uint64_t> off(size_t(n) + 1, 0);
    for (uint32_t f = 0; f < n; f++) {
      const uint64_t r = rng();
      off[f + 1] = off[f] + (r % 7 == 0 ? 0 : (r % 11 == 0 ? 5000 + r % 4000 : r % 100));
    }
    std::vector<uint8_t> want(n);
    for (auto& w : want) w = round % 7 == 0 ? 0 : (round % 9 == 0 ? 1 : uint8_t(rng() % 3 == 0));
    if (round % 13 == 0) want.resize(n / 2);  // a short table is padded with "not fetched"
    tsg::FetchOut out;
    tsg::HostFetchPlan P;
    tsg::PlanFetchOnHost(want, off.data(), n, direct, &out, &P);
    CHECK(out.off.size() == size_t(n) + 1 && out.fetched.size() == n);
    CHECK(P.packed <= P.total && out.off[n] == P.total && P.packed % 16 == 0 && P.total % 16 == 0);
    uint64_t files = 0, bytes = 0, packed_end = 0, direct_lo = UINT64_MAX;
    std::vector<std::pair<uint64_t, uint64_t>> spans;
    std::set<uint32_t> dset(P.direct.begin(), P.direct.end());
    for (uint32_t f = 0; f < n; f++) {
      if (!out.fetched[f]) continue;
      const uint64_t len = off[f + 1] - off[f];
      files++;
      bytes += len;
      CHECK(out.off[f] % 16 == 0 && out.off[f] + len <= P.total);
      CHECK((len >= direct) == (dset.count(f) == 1));
      if (dset.count(f)) direct_lo = std::min(direct_lo, out.off[f]);
      else packed_end = std::max(packed_end, out.off[f] + len);
      if (len) spans.push_back({out.off[f], out.off[f] + len});
    }
    CHECK(files == P.files && bytes == P.bytes && packed_end <= P.packed);
    CHECK(direct_lo == UINT64_MAX || direct_lo >= P.packed);
    std::sort(spans.begin(), spans.end());
    for (size_t i = 1; i < spans.size(); i++) CHECK(spans[i - 1].second <= spans[i].first);
    // the device's counters, as they would come back
    std::string err;
    CHECK(tsg::SameFetchPlan(P.packed, P.direct.size(), P.files, P.bytes, P, &err));
    CHECK(!tsg::SameFetchPlan(P.packed + 16, P.direct.size(), P.files, P.bytes, P, &err) && !err.empty());
    // the bytes of a fetch: every fetched file written where the table says, in a buffer of the planned size
    std::vector<uint8_t> buf(size_t(P.total) + 64, 0);
    for (uint32_t f = 0; f < n; f++)
      if (out.fetched[f]) std::memset(buf.data() + out.off[f], int(f % 251) + 1, size_t(off[f + 1] - off[f]));
    for (uint64_t stage : {uint64_t(16384), uint64_t(65536)}) {
      tsg::FinishFetch(P, stage, 1.5, &out);
      CHECK(out.files == P.files && out.bytes == P.bytes && out.direct_files == P.direct.size());
      CHECK(uint64_t(out.rounds) * stage >= P.packed && (out.rounds == 0 || uint64_t(out.rounds - 1) * stage < P.packed));
    }
  }
}

static void BufferGrowthAndRetirement() {
  std::set<void*> live, retired;
  size_t n_alloc = 0;
  {
    tsg::FetchPool pool(
        3,
        [&](size_t n) -> void* {
          void* p = std::malloc(n);
          CHECK(p && live.insert(p).second);
          n_alloc++;
          return p;
        },
        [&](void* p) {
          CHECK(live.erase(p) == 1 && retired.insert(p).second);
          std::free(p);  // (the engine hands it to its reaper thread)
        });
    std::mt19937_64 rng(11);
    std::vector<std::pair<void*, size_t>> loans;
    size_t need = 100;
    for (int step = 0; step < 600; step++) {
      if (step % 50 == 49) need *= 3;  // the batches grow: the free buffers are outgrown
      if (step % 150 == 149) need = 100;
      if (loans.size() < 5 && (loans.empty() || rng() % 2)) {
        size_t cap = 0;
        const size_t want = need + rng() % need;
        void* p = pool.Take(want, &cap);
        CHECK(p && cap >= want && live.count(p) == 1);
        for (auto& l : loans) CHECK(l.first != p);  // never on loan twice
        std::memset(p, 0xA5, cap);                  // the whole capacity is the borrower's
        loans.push_back({p, cap});
      } else {
        const size_t i = size_t(rng() % loans.size());
        pool.Give(loans[i].first, loans[i].second);
        loans.erase(loans.begin() + long(i));
        CHECK(pool.free_count() <= 3);
      }
    }
    for (auto& l : loans) pool.Give(l.first, l.second);
    pool.Give(nullptr, 0);
    CHECK(pool.free_count() <= 3 && !retired.empty() && n_alloc > 6);
    // a FetchOut's own release without an owner is a no-op; moved tables are freed with it
    {
      tsg::FetchOut out;
      out.off.assign(10, 0);
      out.Release();
      out.Release();
    }
    const std::vector<void*> rest = pool.Drain();
    CHECK(rest.size() == live.size());
    for (void* p : rest) {
      CHECK(live.erase(p) == 1);
      std::free(p);
    }
    CHECK(pool.free_count() == 0);
  }
  CHECK(live.empty());
}

int main() {
  ArgumentValidation();
  OffsetTables();
  BufferGrowthAndRetirement();
  std::printf("san_device_only: ok\n");
  return 0;
}
