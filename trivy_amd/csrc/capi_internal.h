// Definitions shared by the C-ABI translation units (not part of the ABI).
#pragma once
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "scanner.h"
#include "tsg_scanner.h"

struct tsg_scanner {
  std::unique_ptr<tsg::SecretScanner> s;
};

struct tsg_compiled {  // tsg_debug_compile (tsg_debug.h)
  tsg::CompiledRules cr;
};

struct tsg_result {
  tsg::BatchResult files;
  tsg_stats stats;
  tsg::FetchStats fetch;  // tsg_result_fetch_stats (device-only batches; zero otherwise)
  tsg::FetchWindowStats win;  // tsg_result_fetch_window_stats (the windows fetch; zero otherwise)
  tsg::SplitStats split;      // tsg_result_split_stats (the split scan of a resident batch with a transform)
  // tsg_debug_result_skip: files marked, their bytes, tiles dropped, runs, most runs per K1 wave, tiles
  uint64_t skip[6] = {0, 0, 0, 0, 0, 0};
  float ms_k0 = 0;  // tsg_debug_result_k0: the K0 phase's own span (BatchStats::ms_k0)
  std::string json;        // tsg_result_json: every file (built once)
  std::string json_range;  // tsg_result_json_range: the last range asked for
  const tsg::SecretScanner* owner;
  std::unique_ptr<tsg::SecretScanner> owned;  // results of scanners made for one call (oracle hooks)
};

// A scan on its background thread (tsg_scan_submit; tsg_scan_wait joins and frees it).
struct tsg_pending {
  std::thread th;
  tsg_result* r = nullptr;
  int rc = 0;
  std::string err;
  std::shared_ptr<void> owned;  // what the library built for the batch (tsg_analyzer_submit_device): freed with p
};

namespace tsg {
void SetError(const std::string& e);
// tsg_global -> the host scanner's rule specs (capi_scanner.cpp)
bool MakeRules(const tsg_global* g, std::vector<RuleSpec>* rules, std::string* err);
bool MakeAllow(const tsg_allow_rule* a, uint32_t n, std::vector<AllowRuleSpec>* out, std::string* err);
bool MakeExclude(const char* const* rx, uint32_t n, std::vector<std::unique_ptr<Regex>>* out, std::string* err);
}  // namespace tsg
