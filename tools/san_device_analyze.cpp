// Stand-alone sanitizer program for the host half of Analyze on HBM-resident
// files (trivy_amd/csrc/analyze_device.cpp; no GPU, no interpreter): built with
// -fsanitize=address,undefined together with the host sources it calls
// (tools/san_device_analyze.sh) and run as it is.
//
//  1. argument validation of tsg_analyzer_classify_device / _submit_device on an
//     analyzer whose scanner has no GPU engine: every argument error comes back
//     first, valid arguments stop at "no GPU engine";
//  2. the Required / gate / kind table (DeviceKinds) from given flags, against
//     tsg_analyzer_required and the rule written out here, with and without
//     path_lens, over paths that are not NUL-terminated where lengths are given;
//  3. path prefixing (BuildScanPaths): "/" + path for image files, the path as
//     it is under a dir, every pointer inside the pool, lengths exact;
//  4. lifetime of what a pending submit owns: submits with the flags given
//     (the GPU half skipped), the caller's struct destroyed right after the
//     call, two pendings waited in reverse order, each failing at the scanner's
//     missing engine only after the kinds, flags and paths were built and used.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "analyze_device.h"
#include "tsg_analyzer.h"
#include "tsg_debug.h"
#include "tsg_oracle.h"
#include "tsg_scanner.h"

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s (last error: %s)\n", __FILE__, __LINE__, #x, tsg_last_error()); \
      std::exit(1);                                                    \
    }                                                                  \
  } while (0)

static bool Has(const char* text, const char* what) { return std::strstr(text, what) != nullptr; }

static tsg_scanner* HostScanner() {
  static const char* kw[] = {"akia"};
  static tsg_rule rule{};
  rule.id = "aws-access-key-id";
  rule.category = "AWS";
  rule.title = "AWS Access Key ID";
  rule.severity = "CRITICAL";
  rule.regex = "AKIA[A-Z0-9]{16}";
  rule.secret_group_name = "";
  rule.keywords = kw;
  rule.n_keywords = 1;
  static tsg_allow_rule allow{};
  allow.id = "vendor";
  allow.path = "(^|/)vendor/";
  tsg_global g{};
  g.rules = &rule;
  g.n_rules = 1;
  g.allow_rules = &allow;
  g.n_allow_rules = 1;
  tsg_scanner* s = nullptr;
  CHECK(tsg_debug_scanner_host_only(&g, &s) == 0 && s);
  return s;
}

static const void* kFakeDev = reinterpret_cast<const void*>(uintptr_t(0x700000000000ull));  // never dereferenced

struct Files {  // a tsg_device_files with its arrays
  std::vector<std::string> names;
  std::vector<uint64_t> offs{0};
  std::vector<const char*> ptrs;
  std::vector<uint64_t> lens;
  std::string packed;  // the paths back to back, no NULs between them (path_lens form)
  tsg_device_files f{};
  void Add(const std::string& p, uint64_t size) {
    names.push_back(p);
    offs.push_back(offs.back() + size);
  }
  const tsg_device_files* Build(const char* dir, bool with_lens) {
    ptrs.clear();
    lens.clear();
    packed.clear();
    if (with_lens) {
      for (auto& n : names) packed += n;
      size_t at = 0;
      for (auto& n : names) {
        ptrs.push_back(packed.data() + at);
        lens.push_back(n.size());
        at += n.size();
      }
    } else {
      for (auto& n : names) ptrs.push_back(n.c_str());
    }
    f = tsg_device_files{};
    f.struct_size = TSG_DEVICE_FILES_SIZE_V1;
    f.n_files = uint32_t(names.size());
    f.dev_arena = kFakeDev;
    f.host_offsets = offs.data();
    f.paths = ptrs.data();
    f.path_lens = with_lens ? lens.data() : nullptr;
    f.dir = dir;
    return &f;
  }
};

static void ArgumentValidation(tsg_analyzer* a) {
  Files F;
  F.Add("a.txt", 20);
  F.Add("b.txt", 20);
  uint8_t kind[2] = {0xAA, 0xAA}, bin[2] = {0xAA, 0xAA};
  tsg_pending* p = nullptr;
  auto refused = [&](const tsg_device_files* f, const char* what) {
    CHECK(tsg_analyzer_classify_device(a, f, kind, bin, nullptr) < 0 && Has(tsg_last_error(), what));
    CHECK(tsg_analyzer_submit_device(a, f, &p) < 0 && !p && Has(tsg_last_error(), what));
    CHECK(kind[0] == 0xAA && kind[1] == 0xAA && bin[0] == 0xAA && bin[1] == 0xAA);
  };
  tsg_device_files f = *F.Build("", false);
  for (uint32_t bogus : {0u, 8u, TSG_DEVICE_FILES_SIZE_V1 - 8, TSG_DEVICE_FILES_SIZE_V1 + 8, 0xFFFFFFFFu}) {
    f.struct_size = bogus;
    refused(&f, "struct_size");
  }
  f = *F.Build("", false);
  f.dev_arena = nullptr;
  refused(&f, "dev_arena is NULL");
  f = *F.Build("", false);
  f.host_offsets = nullptr;
  refused(&f, "host_offsets is required");
  f = *F.Build("", false);
  f.paths = nullptr;
  refused(&f, "paths is NULL");
  f = *F.Build("", false);
  f.dev_arena = static_cast<const uint8_t*>(kFakeDev) + 8;
  refused(&f, "16-B aligned");
  const uint64_t bad1[3] = {1, 20, 40}, bad2[3] = {0, 30, 20};
  f.dev_arena = kFakeDev;
  f.host_offsets = bad1;
  refused(&f, "ascend from 0");
  f.host_offsets = bad2;
  refused(&f, "ascend from 0");
  CHECK(tsg_analyzer_classify_device(nullptr, &f, kind, bin, nullptr) < 0);
  CHECK(tsg_analyzer_submit_device(a, nullptr, &p) < 0 && !p);
  tsg_device_classify_stats st{};
  st.struct_size = TSG_DEVICE_CLASSIFY_STATS_SIZE_V1 + 8;
  CHECK(tsg_analyzer_classify_device(a, F.Build("", false), kind, bin, &st) < 0 && Has(tsg_last_error(), "struct_size"));
  refused(F.Build("", false), "no GPU engine");  // valid arguments: the scanner has no engine
  refused(F.Build("/src", true), "no GPU engine");
  f = *F.Build("", false);  // an empty batch reads nothing
  f.n_files = 0;
  CHECK(tsg_analyzer_classify_device(a, &f, nullptr, nullptr, nullptr) == 0);
}

static bool IsPyc(const std::string& p) {
  const size_t slash = p.rfind('/'), dot = p.rfind('.');
  return dot != std::string::npos && (slash == std::string::npos || dot > slash) && p.substr(dot) == ".pyc";
}

static void KindTable(tsg_analyzer* a) {
  std::mt19937_64 rng(3);
  const char* dirs[] = {"", "src/", "node_modules/", "a/.git/", "vendor/", "x/vendor/y/", "lib.pyc/", "deep/er/"};
  const char* names[] = {"a.go", "m.pyc", "go.sum", "img.png", "noext", ".pyc", "x.pyc.txt", "y.PYC", "t.tar", "k.env"};
  for (int round = 0; round < 60; round++) {
    Files F;
    const uint32_t n = uint32_t(rng() % 300);
    std::vector<uint8_t> flags(n);
    for (uint32_t i = 0; i < n; i++) {
      F.Add(std::string(dirs[rng() % 8]) + names[rng() % 10], rng() % 4 == 0 ? rng() % 10 : 10 + rng() % 5000);
      flags[i] = uint8_t(rng() % 2);
    }
    const bool with_lens = round % 2 == 1;
    const tsg_device_files* f = F.Build(round % 3 ? "" : "/root", with_lens);
    std::vector<uint8_t> kind(n, 0xAA), bin(n, 0xAA);
    tsg_device_classify_stats st{};
    st.struct_size = TSG_DEVICE_CLASSIFY_STATS_SIZE_V1;
    tsg::DeviceKinds(a, *f, flags.data(), kind.data(), bin.data(), &st);
    uint64_t req = 0, skipped = 0, pyc = 0;
    for (uint32_t i = 0; i < n; i++) {
      const std::string& p = F.names[i];
      const bool r = tsg_analyzer_required(a, p.data(), p.size(), int64_t(F.offs[i + 1] - F.offs[i])) == 1;
      uint8_t wk = 1, wb = 0;
      if (!r) wk = 3;
      else if (flags[i] && IsPyc(p)) wk = 2, wb = 1, pyc++;
      else if (flags[i]) wk = 3, skipped++;
      req += r;
      CHECK(kind[i] == wk && bin[i] == wb);
    }
    CHECK(st.files == n && st.required == req && st.skipped_binary == skipped && st.pyc == pyc);
  }
}

static void PathPrefixing() {
  Files F;
  for (const char* p : {"etc/passwd", "a", "", "dir/with space/x.txt", "/rooted"}) F.Add(p, 10);
  for (int form = 0; form < 6; form++) {
    const char* dir = form % 3 == 0 ? "" : (form % 3 == 1 ? nullptr : "/src");
    const bool image = form % 3 != 2;
    const tsg_device_files* f = F.Build(dir, form >= 3);
    tsg::DevicePlan plan;
    tsg::BuildScanPaths(*f, &plan);
    CHECK(plan.path_ptrs.size() == F.names.size() && plan.path_lens.size() == F.names.size());
    for (size_t i = 0; i < F.names.size(); i++) {
      const std::string want = (image ? "/" : "") + F.names[i];
      CHECK(plan.path_lens[i] == want.size());
      CHECK(plan.path_ptrs[i] >= plan.path_pool.data() &&
            plan.path_ptrs[i] + want.size() < plan.path_pool.data() + plan.path_pool.size());
      CHECK(std::memcmp(plan.path_ptrs[i], want.data(), want.size()) == 0 && plan.path_ptrs[i][want.size()] == '\0');
    }
  }
  tsg_device_files e = *F.Build("", false);
  e.n_files = 0;
  tsg::DevicePlan plan;
  tsg::BuildScanPaths(e, &plan);
  CHECK(plan.path_ptrs.empty() && plan.path_off.size() == 1);
}

static void PendingLifetime(tsg_analyzer* a) {
  std::mt19937_64 rng(5);
  auto make = [&](uint32_t n, bool with_lens, const char* dir, std::vector<uint8_t>* flags) {
    std::unique_ptr<Files> F(new Files());
    for (uint32_t i = 0; i < n; i++) F->Add("d" + std::to_string(i % 7) + "/f" + std::to_string(i) + (i % 5 ? ".txt" : ".pyc"), 10 + rng() % 900);
    flags->resize(n);
    for (auto& x : *flags) x = uint8_t(rng() % 2);
    F->Build(dir, with_lens);
    return F;
  };
  for (int round = 0; round < 8; round++) {
    std::vector<uint8_t> fa, fb;
    std::unique_ptr<Files> A = make(1 + uint32_t(rng() % 2000), round % 2 == 0, "", &fa);
    std::unique_ptr<Files> B = make(1 + uint32_t(rng() % 50), round % 2 == 1, "/srv", &fb);
    tsg_pending *pa = nullptr, *pb = nullptr;
    {
      // the struct is the caller's for the call only: a copy that is destroyed (and scribbled on) after it
      std::unique_ptr<tsg_device_files> ca(new tsg_device_files(A->f)), cb(new tsg_device_files(B->f));
      CHECK(tsg::SubmitDeviceWithFlags(a, ca.get(), fa.data(), &pa) == 0 && pa);
      CHECK(tsg::SubmitDeviceWithFlags(a, cb.get(), fb.data(), &pb) == 0 && pb);
      std::memset(ca.get(), 0xEE, sizeof(tsg_device_files));
      std::memset(cb.get(), 0xEE, sizeof(tsg_device_files));
      std::fill(fa.begin(), fa.end(), uint8_t(0xEE));  // the flags were copied too
    }
    tsg_result* r = nullptr;
    CHECK(tsg_scan_wait(pb, &r) < 0 && !r && Has(tsg_last_error(), "no GPU engine"));  // reverse order
    CHECK(tsg_scan_wait(pa, &r) < 0 && !r && Has(tsg_last_error(), "no GPU engine"));
  }
  // a submit refused for its arguments leaves nothing behind
  Files F;
  F.Add("a.txt", 20);
  tsg_device_files f = *F.Build("", false);
  f.paths = nullptr;
  const uint8_t flag = 0;
  tsg_pending* p = nullptr;
  CHECK(tsg::SubmitDeviceWithFlags(a, &f, &flag, &p) < 0 && !p);
  CHECK(tsg::SubmitDeviceWithFlags(a, F.Build("", false), nullptr, &p) < 0 && !p);
}

int main() {
  tsg_scanner* s = HostScanner();
  tsg_analyzer* a = nullptr;
  CHECK(tsg_analyzer_new(s, "conf/trivy-secret.yaml", &a) == 0 && a);
  ArgumentValidation(a);
  KindTable(a);
  PathPrefixing();
  PendingLifetime(a);
  tsg_analyzer_free(a);
  tsg_scanner_free(s);
  std::printf("san_device_analyze: ok\n");
  return 0;
}
