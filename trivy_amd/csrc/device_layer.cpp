// Analyze for a tar layer whose bytes exist only in HBM (include/tsg_analyzer.h:
// tsg_analyzer_index_device_tar, tsg_analyzer_submit_device_tar).  The GPU finds
// the blocks that parse as headers (tarindex.hip); the chain walk over them,
// the plan of a batch whose arena is the layer itself, and the kinds are the
// host half (tar_index_host.h, plain C++); this file is the glue: argument
// checks, the pooled stream and buffers of an index pass, the copies of single
// blocks and ranges the walk asks for, and the pending of a submit.  In walk
// mode 1 (tsg_analyzer_set_tar_walk) the GPU walks the chain as well
// (tarchain.hip) and the host half starts from its entry records
// (IndexTarEntries); a layer that walk does not complete takes the path above.
// tsg_analyzer_index_device_tars takes all layers of an image: in walk mode 1
// one forest pass (tarforest.hip) walks the chains of all of them, the host half
// runs per layer, and a layer the pass does not complete takes the single-layer
// path alone.  With tsg_analyzer_set_tar_required mode 1 a device stage behind
// either pass's compaction (tarrequired.hip) runs the path work and Required, and
// the host half starts from its file records instead (IndexTarFiles).
#include <hip/hip_runtime_api.h>
#include <pthread.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>

#include "analyze_device.h"
#include "capi_internal.h"
#include "collector.h"
#include "parallel.h"
#include "tar_index_host.h"
#include "tar_required_host.h"
#include "tarindex.h"
#include "tsg_debug.h"
#include "xform.h"

struct tsg_tar_index {
  const uint8_t* dev_tar = nullptr;  // NULL: made from given records (tsg_debug_index_tar_records)
  uint64_t n_bytes = 0;
  tsg::TarIndexData d;
  tsg_tar_walk_stats ws{};  // tsg_tar_index_walk_stats
  tsg_tar_required_stats rs{};  // tsg_tar_index_required_stats
  tsg_tar_required_skip_stats ss{};  // tsg_tar_index_required_skip_stats
};

namespace tsg {
bool RequiredPath(const tsg_analyzer* a, const char* path, uint64_t len, int64_t size);  // analyzer.cpp

// One index pass's stream, events and buffers, pooled like ClassifyCtx: passes
// of several layers run side by side and none takes the scanner's GPU lock.
struct TarIndexCtx {
  hipStream_t s = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  void* d_rec = nullptr;
  uint32_t* d_count = nullptr;
  uint8_t* h_rec = nullptr;      // pinned
  uint32_t* h_count = nullptr;   // pinned
  uint64_t cap_rec = 0, cap_h = 0;  // records
  // the GPU walk (tsg_analyzer_set_tar_walk mode 1): its stage events, its work buffer, the entry
  // records and names on the device and page-locked on the host, the head the host reads
  hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // ([5], [6]: the forest pass)
  uint8_t* d_work = nullptr;
  uint8_t* d_out = nullptr;
  uint8_t* h_out = nullptr;        // pinned
  TarChainHead* h_head = nullptr;  // pinned
  uint64_t cap_work = 0, cap_out = 0, cap_hout = 0;  // bytes
  // the forest pass (tsg_analyzer_index_device_tars): the head array and the uploaded tables, pinned
  uint8_t* h_heads = nullptr;
  uint8_t* h_tables = nullptr;
  uint64_t cap_heads = 0, cap_tables = 0;  // bytes
  // Required on the GPU (tsg_analyzer_set_tar_required mode 1): the stage's device buffer, its
  // uploaded tables and the per-layer counts (pinned), its two events
  uint8_t* d_req = nullptr;
  uint8_t* h_req = nullptr;
  uint64_t cap_req = 0, cap_hreq = 0;  // bytes
  hipEvent_t ev_req[2] = {nullptr, nullptr};
  // its skip stage (tsg_analyzer_set_tar_required_skip mode 1): the table of the recorded directories,
  // and the events around the match kernel and around the build and under kernels
  uint8_t* d_skip = nullptr;
  uint64_t cap_skip = 0;  // bytes
  hipEvent_t ev_skip[4] = {nullptr, nullptr, nullptr, nullptr};
  ~TarIndexCtx() {
    if (d_skip) (void)hipFree(d_skip);
    for (hipEvent_t e : ev_skip)
      if (e) (void)hipEventDestroy(e);
    if (d_req) (void)hipFree(d_req);
    if (h_req) (void)hipHostFree(h_req);
    for (hipEvent_t e : ev_req)
      if (e) (void)hipEventDestroy(e);
    if (h_heads) (void)hipHostFree(h_heads);
    if (h_tables) (void)hipHostFree(h_tables);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    if (d_work) (void)hipFree(d_work);
    if (d_out) (void)hipFree(d_out);
    if (h_out) (void)hipHostFree(h_out);
    if (h_head) (void)hipHostFree(h_head);
    if (d_rec) (void)hipFree(d_rec);
    if (d_count) (void)hipFree(d_count);
    if (h_rec) (void)hipHostFree(h_rec);
    if (h_count) (void)hipHostFree(h_count);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (s) (void)hipStreamDestroy(s);
  }
};
struct TarIndexPool {
  std::mutex mu;
  std::vector<std::unique_ptr<TarIndexCtx>> free;
};
void FreeTarIndexPool(TarIndexPool* p) { delete p; }

namespace {

std::atomic<uint64_t> g_tar_capacity{0};  // tsg_debug_set_tar_capacity

double NowMs() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

std::unique_ptr<TarIndexCtx> TakeCtx(tsg_analyzer* a) {
  {
    std::lock_guard<std::mutex> g(a->tar_index_mu);
    if (!a->tar_index) a->tar_index = new TarIndexPool();
    std::lock_guard<std::mutex> g2(a->tar_index->mu);
    if (!a->tar_index->free.empty()) {
      std::unique_ptr<TarIndexCtx> c = std::move(a->tar_index->free.back());
      a->tar_index->free.pop_back();
      return c;
    }
  }
  std::unique_ptr<TarIndexCtx> c(new TarIndexCtx());
  if (hipStreamCreateWithFlags(&c->s, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&c->e0) != hipSuccess ||
      hipEventCreate(&c->e1) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&c->d_count), 16) != hipSuccess ||
      hipHostMalloc(reinterpret_cast<void**>(&c->h_count), 16, hipHostMallocDefault) != hipSuccess)
    return nullptr;
  return c;
}

// A context goes back to the pool with its stream, events and counter, and with
// record buffers of up to 16 MiB; larger ones are freed here.  The buffers of a
// multi-GB layer are about 13 % of the layer in HBM and as much pinned: nothing
// of that size stays allocated between index calls.
constexpr uint64_t kKeepRecords = (uint64_t(16) << 20) / kTarRecordBytes;
void GiveCtx(tsg_analyzer* a, std::unique_ptr<TarIndexCtx> c) {
  if (c->cap_rec > kKeepRecords) {
    (void)hipFree(c->d_rec);
    c->d_rec = nullptr;
    c->cap_rec = 0;
  }
  if (c->cap_h > kKeepRecords) {
    (void)hipHostFree(c->h_rec);
    c->h_rec = nullptr;
    c->cap_h = 0;
  }
  constexpr uint64_t kKeepBytes = uint64_t(16) << 20;
  if (c->cap_work > kKeepBytes) {
    (void)hipFree(c->d_work);
    c->d_work = nullptr;
    c->cap_work = 0;
  }
  if (c->cap_out > kKeepBytes) {
    (void)hipFree(c->d_out);
    c->d_out = nullptr;
    c->cap_out = 0;
  }
  if (c->cap_hout > kKeepBytes) {
    (void)hipHostFree(c->h_out);
    c->h_out = nullptr;
    c->cap_hout = 0;
  }
  if (c->cap_heads > kKeepBytes) {
    (void)hipHostFree(c->h_heads);
    c->h_heads = nullptr;
    c->cap_heads = 0;
  }
  if (c->cap_tables > kKeepBytes) {
    (void)hipHostFree(c->h_tables);
    c->h_tables = nullptr;
    c->cap_tables = 0;
  }
  if (c->cap_req > kKeepBytes) {
    (void)hipFree(c->d_req);
    c->d_req = nullptr;
    c->cap_req = 0;
  }
  if (c->cap_skip > kKeepBytes) {
    (void)hipFree(c->d_skip);
    c->d_skip = nullptr;
    c->cap_skip = 0;
  }
  if (c->cap_hreq > kKeepBytes) {
    (void)hipHostFree(c->h_req);
    c->h_req = nullptr;
    c->cap_hreq = 0;
  }
  std::lock_guard<std::mutex> g(a->tar_index->mu);
  if (a->tar_index->free.size() < 2) a->tar_index->free.push_back(std::move(c));  // (else freed here)
}

void FillStats(tsg_device_tar_stats* st, const TarIndexData& d, const IndexedTarSrc& src, uint64_t n_bytes,
               uint64_t candidates, uint64_t kernel_runs, double ms_kernel, double ms_total) {
  if (!st) return;
  st->tar = d.tar;
  st->blocks = n_bytes / 512;
  st->candidates = candidates;
  st->off_chain = candidates - src.visited();
  st->block_fetches = src.block_fetches;
  st->ext_bytes = src.ext_bytes;
  st->kernel_runs = kernel_runs;
  st->ms_kernel = ms_kernel;
  st->ms_total = ms_total;
}

bool StatsSizeOk(const tsg_device_tar_stats* st, const char* who) {
  if (!st || st->struct_size == TSG_DEVICE_TAR_STATS_SIZE_V1) return true;
  SetError(std::string(who) + ": tsg_device_tar_stats.struct_size " + std::to_string(st->struct_size) +
           " is not a size this library knows (v1 = " + std::to_string(TSG_DEVICE_TAR_STATS_SIZE_V1) + ")");
  return false;
}

// Required and the per-entry path work of an index, 1,024 entries a task on the host pool.
auto ChunkedPar() {
  return [](size_t n, const std::function<void(size_t)>& fn) {
    const size_t blocks = (n + 1023) / 1024;
    ParallelFor(blocks, 16, [&](size_t b) {
      for (size_t i = b * 1024; i < std::min(n, (b + 1) * 1024); i++) fn(i);
    });
  };
}
// The same for the host half of the GPU walk, whose first pass has one item per 64 entries: at most
// 1,024 items a task, and at least 128 tasks where there are that many items.
auto EntriesPar() {
  return [](size_t n, const std::function<void(size_t)>& fn) {
    const size_t per = std::max<size_t>(1, std::min<size_t>(1024, n / 128));
    const size_t blocks = (n + per - 1) / per;
    ParallelFor(blocks, 16, [&](size_t b) {
      for (size_t i = b * per; i < std::min(n, (b + 1) * per); i++) fn(i);
    });
  };
}

// (the analyzer's skip options, tsg_analyzer_set_tar_skip, as they are when the walk begins)
int WalkRecords(tsg_analyzer* a, const IndexedTarSrc& src, uint64_t n_bytes, TarIndexData* d) {
  const std::shared_ptr<const TarSkipOpts> skip = a->TarSkip();
  return WalkTarIndex(
      src, n_bytes, [a](const char* p, uint64_t len, int64_t size) { return RequiredPath(a, p, len, size); }, d,
      ChunkedPar(), skip.get());
}

// ---- the chain walk on the GPU (tarchain.h) ----------------------------------
// The host half over given records: the index, and the V1 stats of mode 1.
int EntriesToIndex(tsg_analyzer* a, const tsg_tar_entry_rec* recs, uint64_t n, const uint8_t* names, uint64_t name_bytes,
                   const tsg_tar_stop& stop, uint64_t n_bytes, uint64_t candidates, TarIndexData* d,
                   tsg_device_tar_stats* st, double* ms = nullptr) {
  const std::shared_ptr<const TarSkipOpts> skip = a->TarSkip();
  if (IndexTarEntries(
          recs, n, names, name_bytes,
          [a](const char* p, uint64_t len, int64_t size) { return RequiredPath(a, p, len, size); }, d, EntriesPar(),
          ms, skip.get()) < 0)
    return -1;
  if (st) {
    uint64_t on_chain = stop.ext_visited;  // every header of every entry, as the host walk's records visited
    for (uint64_t i = 0; i < n; i++) on_chain += uint64_t(recs[i].n_ext) + 1;
    st->tar = d->tar;
    st->blocks = n_bytes / 512;
    st->candidates = candidates;
    st->off_chain = candidates > on_chain ? candidates - on_chain : 0;
    st->block_fetches = 0;
    st->ext_bytes = 0;
  }
  return 0;
}

bool Grow(uint8_t** p, uint64_t* cap, uint64_t want, bool pinned, hipError_t* e) {
  if (*cap >= want) return true;
  if (*p) (void)(pinned ? hipHostFree(*p) : hipFree(*p));
  *p = nullptr;
  *cap = 0;
  *e = pinned ? hipHostMalloc(reinterpret_cast<void**>(p), want, hipHostMallocDefault)
              : hipMalloc(reinterpret_cast<void**>(p), want);
  if (*e != hipSuccess) return false;
  *cap = want;
  return true;
}

// ---- path classify and Required on the GPU (tarrequired.h) ---------------------
// Why an index call ran Required on the host (tsg_tar_required_stats.reason); 0: the GPU stage ran.
enum : uint32_t {
  kReqUsedGpu = 0,
  kReqSetterOff = 1,
  kReqWalkHost = 2,
  kReqSkipOptions = 3,
  kReqLayerFellBack = 4,
  kReqAskedSkipDir = 5,  // (only with tsg_analyzer_set_tar_required_skip mode 1)
};
// Whether the stage honoured the skip options (tsg_tar_required_skip_stats.reason); 0: it did.
enum : uint32_t {
  kSkipRan = 0,
  kSkipSetterOff = 1,
  kSkipNoOptions = 2,
  kSkipPatterns = 3,
  kSkipNoStage = 4,
  kSkipAskedDir = 5,
};
// *skip_reason (optional) as far as it is known before the walk; *with_skip (optional): the options
// the stage is to honour (set only with reason 0 and options the device takes).
uint32_t RequiredReason(const tsg_analyzer* a, int walk_mode, uint32_t* skip_reason = nullptr,
                        std::shared_ptr<const TarSkipOpts>* with_skip = nullptr) {
  const std::shared_ptr<const TarSkipOpts> skip = a->TarSkip();
  const bool has = skip && skip->any();
  uint32_t sr = a->tar_required_skip.load() != 1 ? kSkipSetterOff : !has ? kSkipNoOptions
                : !skip->dev_ok ? kSkipPatterns : kSkipRan;
  uint32_t r = kReqUsedGpu;
  if (a->tar_required.load() != 1) r = kReqSetterOff;
  else if (walk_mode != 1) r = kReqWalkHost;
  else if (has && sr != kSkipRan) r = kReqSkipOptions;
  if (sr == kSkipRan && r != kReqUsedGpu) sr = kSkipNoStage;
  if (skip_reason) *skip_reason = sr;
  if (with_skip && r == kReqUsedGpu && has) *with_skip = skip;
  return r;
}
void SkipStatsInit(const tsg_analyzer* a, uint32_t reason, tsg_tar_required_skip_stats* ss) {
  *ss = tsg_tar_required_skip_stats{};
  ss->mode = uint32_t(a->tar_required_skip.load());
  ss->reason = reason;
  const std::shared_ptr<const TarSkipOpts> skip = a->TarSkip();
  if (skip) {
    ss->dir_patterns = uint32_t(skip->dirs.size());
    ss->file_patterns = uint32_t(skip->files.size());
  }
}

// One run of the stage behind a compaction on the context's stream, and what it handed over.
struct ReqPass {
  const PathTable* d_path = nullptr;  // the scanner's tables in HBM (either may be NULL)
  const SureTable* d_sure = nullptr;
  std::string cfg;                    // the analyzer's config base
  TarRequiredLayout L;
  const TarRequiredCounts* counts = nullptr;  // per layer (in c->h_req)
  const tsg_tar_file_rec* recs = nullptr;     // all layers' (in c->h_out)
  const uint8_t* blob = nullptr;
  uint64_t n_recs = 0, blob_bytes = 0, bad = 0;
  double ms_kernel = 0, ms_copy = 0;
  // the skip stage: the options it honours (NULL: it does not run), a table size forced by the debug
  // hook (0: TarSkipSlots), and what it did
  std::shared_ptr<const TarSkipOpts> skip;
  uint64_t forced_slots = 0;
  bool bad_slots = false;  // the forced size is no power of two of at least four times the directories
  uint64_t n_dirs = 0, slots = 0;
  double ms_skip = 0;
};
void ReqPassInit(const tsg_analyzer* a, ReqPass* R) {
  const SecretScanner::AllowTables t = a->s->s->allow_tables();
  R->d_path = t.dev_path;
  R->d_sure = t.dev_path ? t.dev_sure : nullptr;
  R->cfg = a->config_base;
}
// The stage over the n records at d_recs and the names at d_names, which the compaction queued on
// c->s before this call is writing: the counts, then one copy of the file records and one of the
// paths, into c->h_out.  Synchronises the stream twice.  keep_dec: the decisions are copied out too.
hipError_t RequiredOnGpu(TarIndexCtx* c, ReqPass* R, const uint8_t* d_recs, const uint8_t* d_names, uint64_t n,
                         uint64_t name_bytes, const uint64_t* rec_base, const uint64_t* name_base, uint32_t n_layers,
                         uint32_t grid_cap, std::vector<uint8_t>* keep_dec = nullptr) {
  hipError_t e = hipSuccess;
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  const TarSkipOpts* skip = R->skip.get();
  if (!TarRequiredPlan(n, n_layers, name_bytes, uint32_t(R->cfg.size()), &R->L, skip != nullptr))
    return hipErrorInvalidValue;
  const TarRequiredLayout& L = R->L;
  for (hipEvent_t& v : c->ev_req)
    if (!v) ok(hipEventCreate(&v));
  if (skip) {
    for (hipEvent_t& v : c->ev_skip)
      if (!v) ok(hipEventCreate(&v));
    if (!c->d_count) ok(hipMalloc(reinterpret_cast<void**>(&c->d_count), 16));
    if (!c->h_count) ok(hipHostMalloc(reinterpret_cast<void**>(&c->h_count), 16, hipHostMallocDefault));
  }
  const uint64_t cnt_bytes = uint64_t(n_layers) * sizeof(TarRequiredCounts);
  if (!ok(e) || !Grow(&c->d_req, &c->cap_req, L.bytes, false, &e) ||
      !Grow(&c->h_req, &c->cap_hreq, L.tables_bytes + cnt_bytes, true, &e))
    return e;
  TarRequiredTables(L, rec_base, name_base, R->cfg.data(), c->h_req, skip ? &skip->dev : nullptr);
  R->n_dirs = R->slots = 0;
  R->ms_skip = 0;
  if (skip) {
    // the decisions, the match kernel, and one small copy: the number of directories it recorded
    // sizes the table, and with none the other two kernels do not run
    if (!(ok(hipEventRecord(c->ev_req[0], c->s)) &&
          ok(TarRequiredDecide(L, c->h_req, d_recs, d_names, R->d_path, R->d_sure, c->d_req, grid_cap, c->s)) &&
          ok(hipEventRecord(c->ev_skip[0], c->s)) &&
          ok(TarSkipMatchRun(L, d_recs, d_names, c->d_req, c->d_count, grid_cap, c->s)) &&
          ok(hipEventRecord(c->ev_skip[1], c->s)) &&
          ok(hipMemcpyAsync(c->h_count, c->d_count, 4, hipMemcpyDeviceToHost, c->s)) && ok(hipStreamSynchronize(c->s))))
      return e;
    R->n_dirs = *c->h_count;
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ev_skip[0], c->ev_skip[1]) == hipSuccess) R->ms_skip = ms;
    if (R->n_dirs) {
      R->slots = R->forced_slots ? R->forced_slots : TarSkipSlots(R->n_dirs);
      if ((R->slots & (R->slots - 1)) || R->slots < 4 * R->n_dirs || R->slots > (uint64_t(1) << 31)) {
        R->bad_slots = true;
        return hipErrorInvalidValue;
      }
      if (!Grow(&c->d_skip, &c->cap_skip, R->slots * sizeof(TarSkipSlot), false, &e) ||
          !(ok(hipEventRecord(c->ev_skip[2], c->s)) &&
            ok(TarSkipUnderRun(L, d_recs, d_names, c->d_req, reinterpret_cast<TarSkipSlot*>(c->d_skip), R->slots, grid_cap,
                               c->s)) &&
            ok(hipEventRecord(c->ev_skip[3], c->s))))
        return e;
    }
  }
  if (!((skip ? ok(TarRequiredFinish(L, d_recs, d_names, c->d_req, grid_cap, c->s))
              : ok(hipEventRecord(c->ev_req[0], c->s)) &&
                    ok(TarRequiredRun(L, c->h_req, d_recs, d_names, R->d_path, R->d_sure, c->d_req, grid_cap, c->s))) &&
        ok(hipEventRecord(c->ev_req[1], c->s)) &&
        ok(hipMemcpyAsync(c->h_req + L.tables_bytes, c->d_req + L.counts, cnt_bytes, hipMemcpyDeviceToHost, c->s)) &&
        ok(hipStreamSynchronize(c->s))))
    return e;
  float ms = 0;
  if (hipEventElapsedTime(&ms, c->ev_req[0], c->ev_req[1]) == hipSuccess) R->ms_kernel = ms;
  if (R->n_dirs && hipEventElapsedTime(&ms, c->ev_skip[2], c->ev_skip[3]) == hipSuccess) R->ms_skip += ms;
  R->counts = reinterpret_cast<const TarRequiredCounts*>(c->h_req + L.tables_bytes);
  R->n_recs = R->blob_bytes = R->bad = 0;
  for (uint32_t k = 0; k < n_layers; k++) {
    if (R->counts[k].rec_first != R->n_recs || R->counts[k].path_first != R->blob_bytes) return hipErrorUnknown;
    R->n_recs += R->counts[k].records;
    R->blob_bytes += R->counts[k].path_bytes;
    R->bad += R->counts[k].bad;
  }
  if (R->n_recs > n || R->blob_bytes > L.blob_cap) return hipErrorUnknown;  // (the sums are over n decisions)
  const uint64_t rec_bytes = (R->n_recs * sizeof(tsg_tar_file_rec) + 255) & ~uint64_t(255);
  const double t1 = NowMs();
  if (!Grow(&c->h_out, &c->cap_hout, rec_bytes + R->blob_bytes + 256, true, &e)) return e;
  if ((R->n_recs == 0 || ok(hipMemcpyAsync(c->h_out, c->d_req + L.recs, R->n_recs * sizeof(tsg_tar_file_rec),
                                           hipMemcpyDeviceToHost, c->s))) &&
      (R->blob_bytes == 0 || ok(hipMemcpyAsync(c->h_out + rec_bytes, c->d_req + L.blob, R->blob_bytes,
                                               hipMemcpyDeviceToHost, c->s))))
    ok(hipStreamSynchronize(c->s));
  if (ok(e) && keep_dec && n) {
    keep_dec->resize(size_t(n) * 16);
    ok(hipMemcpy(keep_dec->data(), c->d_req + L.dec, size_t(n) * 16, hipMemcpyDeviceToHost));
  }
  R->ms_copy = NowMs() - t1;
  R->recs = reinterpret_cast<const tsg_tar_file_rec*>(c->h_out);
  R->blob = c->h_out + rec_bytes;
  return e;
}

// The host half over one layer's file records (IndexTarFiles): the index, the V1 stats of mode 1 and
// the required stats' counts.  -1: the records contradict the blob or the counts (error set).
// skip: the options the stage honoured (NULL: none); then 1: an asked name is a skipped directory --
// nothing was added, and the caller indexes the layer from the walk's records (reason 5).
int FilesToIndex(tsg_analyzer* a, const TarRequiredCounts& cnt, const tsg_tar_file_rec* recs, const uint8_t* blob,
                 const tsg_tar_stop& stop, uint64_t n_bytes, uint64_t candidates, TarIndexData* d,
                 tsg_device_tar_stats* st, tsg_tar_required_stats* rs, const TarSkipOpts* skip = nullptr) {
  const SecretScanner* sc = a->s->s.get();
  TarRequiredHostStats hs;
  const int rc = IndexTarFiles(
          recs, cnt.records, blob, cnt.path_bytes, cnt,
          [sc](const char* p, uint64_t len, uint64_t rules) {
            return sc->AllowPathMasked(reinterpret_cast<const uint8_t*>(p), size_t(len), rules);
          },
          [sc](const char* p, uint64_t len) { return sc->AllowPath(reinterpret_cast<const uint8_t*>(p), size_t(len)); },
          [a](const char* p, uint64_t len, int64_t size) { return RequiredPath(a, p, len, size); }, d, EntriesPar(),
          &hs, skip);
  if (rc != 0) return rc;
  if (st) {
    const uint64_t on_chain = stop.ext_visited + cnt.ext_headers + cnt.entries;  // as EntriesToIndex counts them
    st->tar = d->tar;
    st->blocks = n_bytes / 512;
    st->candidates = candidates;
    st->off_chain = candidates > on_chain ? candidates - on_chain : 0;
    st->block_fetches = 0;
    st->ext_bytes = 0;
  }
  if (rs) {
    rs->mode = 1;
    rs->reason = kReqUsedGpu;
    rs->entries = cnt.entries;
    rs->kept = cnt.kept;
    rs->dropped = cnt.dropped;
    rs->ask_allow = cnt.ask_allow;
    rs->ask_name = cnt.ask_name;
    rs->ask_dropped = hs.ask_dropped;
    rs->path_bytes = cnt.path_bytes;
  }
  return 0;
}

// A layer whose asked names hold a skipped directory (FilesToIndex returned 1): its entry records
// and names are still where the compaction wrote them in c->d_out (the records of all layers, then
// from rec_bytes_all on the names); they are copied out and the host half of the walk indexes it.
int RefusedLayerToIndex(tsg_analyzer* a, TarIndexCtx* c, const std::string& who, uint64_t rec_bytes_all, uint64_t rec0,
                        uint64_t name0, const TarChainHead& head, uint64_t n_bytes, TarIndexData* d,
                        tsg_device_tar_stats* st) {
  std::vector<uint8_t> buf(size_t(head.entries) * sizeof(tsg_tar_entry_rec) + size_t(head.name_bytes) + 1);
  uint8_t* names = buf.data() + size_t(head.entries) * sizeof(tsg_tar_entry_rec);
  hipError_t e = hipSuccess;
  if (head.entries)
    e = hipMemcpy(buf.data(), c->d_out + rec0 * sizeof(tsg_tar_entry_rec), size_t(head.entries) * sizeof(tsg_tar_entry_rec),
                  hipMemcpyDeviceToHost);
  if (e == hipSuccess && head.name_bytes)
    e = hipMemcpy(names, c->d_out + rec_bytes_all + name0, size_t(head.name_bytes), hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    SetError(who + ": " + hipGetErrorString(e));
    return -1;
  }
  return EntriesToIndex(a, reinterpret_cast<const tsg_tar_entry_rec*>(buf.data()), head.entries, names, head.name_bytes,
                        head.stop, n_bytes, head.candidates, d, st);
}

// The GPU half on the context's stream: 0 with *recs / *names (in c->h_out) and
// *head filled; 1 the chain is INCOMPLETE (or the pass does not take the layer):
// ws->fallback says why; -2 a HIP error, its text set.  n_bytes >= 512.
int ChainOnGpu(TarIndexCtx* c, const uint8_t* dev_tar, uint64_t n_bytes, uint32_t segment_blocks, uint32_t grid_cap,
               const std::string& who, TarChainHead* head, const tsg_tar_entry_rec** recs, const uint8_t** names,
               tsg_tar_walk_stats* ws, ReqPass* rq = nullptr) {
  // rq != NULL: the Required stage runs behind the compaction, and what comes back is rq's file
  // records and paths; the entry records and the names stay in HBM (*recs and *names are NULL).
  TarChainLayout L;
  if (!TarChainPlan(n_bytes, segment_blocks, &L)) {
    if (segment_blocks) {
      SetError(who + ": segment_blocks must be a power of two from 8 to 8192");
      return -2;
    }
    ws->fallback = kTarTooLarge;
    return 1;
  }
  hipError_t e = hipSuccess;
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  for (hipEvent_t& v : c->ev)
    if (!v) ok(hipEventCreate(&v));
  if (ok(e) && !c->h_head) ok(hipHostMalloc(reinterpret_cast<void**>(&c->h_head), sizeof(TarChainHead), hipHostMallocDefault));
  if (ok(e)) Grow(&c->d_work, &c->cap_work, L.bytes, false, &e);
  ws->segments = L.n_segments;
  ws->device_bytes = L.bytes;
  uint64_t rec_bytes = 0, out_bytes = 0;
  bool incomplete = false;
  if (ok(e) && ok(TarChainWalk(dev_tar, n_bytes, L, c->d_work, grid_cap, c->s, c->ev)) &&
      ok(hipMemcpyAsync(c->h_head, c->d_work + L.head, sizeof(TarChainHead), hipMemcpyDeviceToHost, c->s)) &&
      ok(hipStreamSynchronize(c->s))) {
    *head = *c->h_head;
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) ws->ms_candidates = ms;
    if (hipEventElapsedTime(&ms, c->ev[1], c->ev[2]) == hipSuccess) ws->ms_entries = ms;
    if (hipEventElapsedTime(&ms, c->ev[2], c->ev[3]) == hipSuccess) ws->ms_mark = ms;
    incomplete = head->stop.kind != kTarStopEnd;
    if (incomplete) ws->fallback = head->stop.reason ? head->stop.reason : uint32_t(kTarNotCandidate);
    rec_bytes = (head->entries * sizeof(tsg_tar_entry_rec) + 255) & ~uint64_t(255);
    out_bytes = rec_bytes + head->name_bytes + 256;
  }
  if (ok(e) && !incomplete) {
    ws->chain_entries = head->entries;
    ws->name_bytes = head->name_bytes;
    ws->device_bytes = L.bytes + out_bytes;
    // (ev[0] again: the allocations above the kernel are not its time)
    if (rq) {
      const uint64_t rec_base[2] = {0, head->entries}, name_base[2] = {0, head->name_bytes};
      if (Grow(&c->d_out, &c->cap_out, out_bytes, false, &e) && ok(hipEventRecord(c->ev[0], c->s)) &&
          ok(TarChainCompact(dev_tar, n_bytes, L, c->d_work, head->entries, head->name_bytes, c->d_out,
                             c->d_out + rec_bytes, grid_cap, c->s)) &&
          ok(hipEventRecord(c->ev[4], c->s)) &&
          ok(RequiredOnGpu(c, rq, c->d_out, c->d_out + rec_bytes, head->entries, head->name_bytes, rec_base, name_base,
                           1, grid_cap))) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, c->ev[0], c->ev[4]) == hipSuccess) ws->ms_compact = ms;
        ws->ms_copy = rq->ms_copy;
        ws->device_bytes += rq->L.bytes;
      }
    } else if (Grow(&c->d_out, &c->cap_out, out_bytes, false, &e) && Grow(&c->h_out, &c->cap_hout, out_bytes, true, &e) &&
        ok(hipEventRecord(c->ev[0], c->s)) &&
        ok(TarChainCompact(dev_tar, n_bytes, L, c->d_work, head->entries, head->name_bytes, c->d_out,
                           c->d_out + rec_bytes, grid_cap, c->s)) &&
        ok(hipEventRecord(c->ev[4], c->s)) && ok(hipStreamSynchronize(c->s))) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, c->ev[0], c->ev[4]) == hipSuccess) ws->ms_compact = ms;
      const double t1 = NowMs();
      // one copy of the records, one of the names
      if ((head->entries == 0 || ok(hipMemcpyAsync(c->h_out, c->d_out, head->entries * sizeof(tsg_tar_entry_rec),
                                                   hipMemcpyDeviceToHost, c->s))) &&
          (head->name_bytes == 0 || ok(hipMemcpyAsync(c->h_out + rec_bytes, c->d_out + rec_bytes, head->name_bytes,
                                                      hipMemcpyDeviceToHost, c->s))))
        ok(hipStreamSynchronize(c->s));
      ws->ms_copy = NowMs() - t1;
    }
  }
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(c->s);  // nothing of a failed pass is left queued on a pooled stream
    SetError(who + ": " + hipGetErrorString(e));
    return -2;
  }
  if (incomplete) return 1;
  *recs = rq ? nullptr : reinterpret_cast<const tsg_tar_entry_rec*>(c->h_out);
  *names = rq ? nullptr : c->h_out + rec_bytes;
  return 0;
}

// One forest pass (tarforest.h) over n layers on the context's stream: 0 with the heads (in c->h_heads),
// every layer's record and name base, and *recs / *names (in c->h_out) for all of them; -2 a HIP error or
// a segment size that is none, its text set.  The layers fit one pass (TarForestCut).  Two
// synchronisations: after the head copy, and after the compaction and the two copies.
struct ForestPass {
  TarForestLayout L;
  const TarChainHead* heads = nullptr;
  std::vector<uint64_t> rec_base, name_base;  // n + 1 each
  const tsg_tar_entry_rec* recs = nullptr;
  const uint8_t* names = nullptr;
};
int ForestOnGpu(TarIndexCtx* c, const void* const* ptrs, const uint64_t* n_bytes, uint32_t n, uint32_t segment_blocks,
                uint32_t grid_cap, const std::string& who, ForestPass* P, tsg_tar_forest_stats* fs,
                ReqPass* rq = nullptr) {
  TarForestLayout& L = P->L;
  if (!TarForestPlan(n_bytes, n, segment_blocks, &L)) {
    SetError(who + ": segment_blocks must be a power of two from 8 to 8192, and the layers must fit one pass");
    return -2;
  }
  hipError_t e = hipSuccess;
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  for (hipEvent_t& v : c->ev)
    if (!v) ok(hipEventCreate(&v));
  const uint64_t head_bytes = uint64_t(n) * sizeof(TarChainHead);
  if (ok(e)) Grow(&c->h_heads, &c->cap_heads, head_bytes, true, &e);
  if (ok(e)) Grow(&c->h_tables, &c->cap_tables, L.tables_bytes, true, &e);
  if (ok(e)) Grow(&c->d_work, &c->cap_work, L.bytes, false, &e);
  uint64_t rec_bytes = 0, out_bytes = 0, entries = 0, name_bytes = 0;
  if (ok(e)) {
    TarForestTables(L, ptrs, n_bytes, c->h_tables);
    if (ok(TarForestWalk(L, c->h_tables, c->d_work, grid_cap, c->s, c->ev)) &&
        ok(hipMemcpyAsync(c->h_heads, c->d_work + L.heads, head_bytes, hipMemcpyDeviceToHost, c->s)))
      ok(hipStreamSynchronize(c->s));
  }
  if (ok(e)) {
    P->heads = reinterpret_cast<const TarChainHead*>(c->h_heads);
    constexpr size_t kHeadWords = sizeof(TarChainHead) / 8;
    TarForestBases(&P->heads[0].entries, kHeadWords, n, &P->rec_base);
    TarForestBases(&P->heads[0].name_bytes, kHeadWords, n, &P->name_base);
    entries = P->rec_base[n];
    name_bytes = P->name_base[n];
    rec_bytes = (entries * sizeof(tsg_tar_entry_rec) + 255) & ~uint64_t(255);
    out_bytes = rec_bytes + name_bytes + 256;
    // one compaction, one copy of all records, one of all names, one synchronisation
    if (rq) {  // the Required stage behind the compaction: its file records and paths come back instead
      if (Grow(&c->d_out, &c->cap_out, out_bytes, false, &e) && ok(hipEventRecord(c->ev[5], c->s)) &&
          ok(TarForestCompact(L, c->d_work, entries, name_bytes, c->d_out, c->d_out + rec_bytes, grid_cap, c->s)) &&
          ok(hipEventRecord(c->ev[4], c->s)) && ok(hipEventRecord(c->ev[6], c->s)))
        ok(RequiredOnGpu(c, rq, c->d_out, c->d_out + rec_bytes, entries, name_bytes, P->rec_base.data(),
                         P->name_base.data(), n, grid_cap));
    } else if (Grow(&c->d_out, &c->cap_out, out_bytes, false, &e) && Grow(&c->h_out, &c->cap_hout, out_bytes, true, &e) &&
        ok(hipEventRecord(c->ev[5], c->s)) &&
        ok(TarForestCompact(L, c->d_work, entries, name_bytes, c->d_out, c->d_out + rec_bytes, grid_cap, c->s)) &&
        ok(hipEventRecord(c->ev[4], c->s)) &&
        (entries == 0 || ok(hipMemcpyAsync(c->h_out, c->d_out, entries * sizeof(tsg_tar_entry_rec),
                                           hipMemcpyDeviceToHost, c->s))) &&
        (name_bytes == 0 || ok(hipMemcpyAsync(c->h_out + rec_bytes, c->d_out + rec_bytes, name_bytes,
                                              hipMemcpyDeviceToHost, c->s))) &&
        ok(hipEventRecord(c->ev[6], c->s)))
      ok(hipStreamSynchronize(c->s));
  }
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(c->s);  // nothing of a failed pass is left queued on a pooled stream
    SetError(who + ": " + hipGetErrorString(e));
    return -2;
  }
  P->recs = rq ? nullptr : reinterpret_cast<const tsg_tar_entry_rec*>(c->h_out);  // (rq: they stay in HBM)
  P->names = rq ? nullptr : c->h_out + rec_bytes;
  if (rq) out_bytes += rq->L.bytes;
  if (fs && rq) fs->ms_copy += rq->ms_copy;
  if (fs) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) fs->ms_candidates += ms;
    if (hipEventElapsedTime(&ms, c->ev[1], c->ev[2]) == hipSuccess) fs->ms_entries += ms;
    if (hipEventElapsedTime(&ms, c->ev[2], c->ev[3]) == hipSuccess) fs->ms_mark += ms;
    if (hipEventElapsedTime(&ms, c->ev[5], c->ev[4]) == hipSuccess) fs->ms_compact += ms;
    if (hipEventElapsedTime(&ms, c->ev[4], c->ev[6]) == hipSuccess) fs->ms_copy += ms;
    fs->passes++;
    fs->virtual_blocks += L.v_blocks;
    fs->segments += L.n_segments;
    fs->device_bytes = std::max<uint64_t>(fs->device_bytes, L.bytes + out_bytes);
  }
  return 0;
}

}  // namespace
}  // namespace tsg

extern "C" {

// The checks of one tsg_device_tar; `who` names the call (and the layer, where there are several).
static bool DeviceTarOk(const std::string& who, const tsg_device_tar* t) {
  using namespace tsg;
  if (t->struct_size != TSG_DEVICE_TAR_SIZE_V1) {
    SetError(who + ": tsg_device_tar.struct_size " + std::to_string(t->struct_size) +
             " is not a size this library knows (v1 = " + std::to_string(TSG_DEVICE_TAR_SIZE_V1) + ")");
    return false;
  }
  if (!t->dev_tar) {
    SetError(who + ": dev_tar is NULL (the layer's bytes, resident in HBM)");
    return false;
  }
  if (reinterpret_cast<uintptr_t>(t->dev_tar) % 16 != 0) {
    SetError(who + ": dev_tar must be 16-B aligned");
    return false;
  }
  if ((t->n_bytes / 512) >> 32) {
    SetError(who + ": a layer of " + std::to_string(t->n_bytes) + " bytes has 2^32 or more 512-B blocks");
    return false;
  }
  return true;
}

// One layer by the single-layer path, its arguments checked: tsg_analyzer_index_device_tar's work.
// forced_fallback != NULL: the layer is one a forest pass (tsg_analyzer_index_device_tars) did not
// complete for that reason -- mode 0 indexes it, and the index says walk 1 with that fallback.
static int IndexOneLayer(tsg_analyzer* a, const std::string& who, const uint8_t* dev_tar, uint64_t n_bytes,
                         const uint32_t* forced_fallback, tsg_tar_index** out, tsg_device_tar_stats* st) {
  using namespace tsg;
  const int device = a->s->s->device();
  if (device < 0) {
    SetError(who + ": no GPU engine bound to this analyzer's scanner");
    return -2;
  }
  const double t0 = NowMs();
  hipError_t e = hipSetDevice(device);
  std::unique_ptr<TarIndexCtx> c = e == hipSuccess ? TakeCtx(a) : nullptr;
  if (!c) {
    SetError(who + ": stream / events");
    return -2;
  }
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  tsg_tar_walk_stats ws{};
  ws.walk = forced_fallback ? 1u : uint32_t(a->tar_walk.load());
  if (forced_fallback) ws.fallback = *forced_fallback;
  // Required on the GPU (tsg_analyzer_set_tar_required): only behind a GPU walk that completes the layer
  tsg_tar_required_stats rs{};
  uint32_t skip_reason = 0;
  std::shared_ptr<const TarSkipOpts> with_skip;
  rs.reason = RequiredReason(a, int(ws.walk), &skip_reason, &with_skip);
  if (rs.reason == kReqUsedGpu && forced_fallback) {
    rs.reason = kReqLayerFellBack;
    if (skip_reason == kSkipRan) skip_reason = kSkipNoStage;
  }
  tsg_tar_required_skip_stats ss{};
  SkipStatsInit(a, skip_reason, &ss);
  if (ws.walk == 1 && !forced_fallback) {
    // The chain walk on the GPU.  A layer it does not complete falls through to the host walk below,
    // from scratch: that path alone words what is wrong with a malformed archive.
    std::unique_ptr<tsg_tar_index> ix(new tsg_tar_index());
    ix->dev_tar = dev_tar;
    ix->n_bytes = n_bytes;
    TarChainHead head{};
    const tsg_tar_entry_rec* recs = nullptr;
    const uint8_t* names = nullptr;
    int rc = 0;
    ReqPass rq;
    bool on_gpu = false;  // the Required stage ran
    if (n_bytes < 512) {  // no complete block: the empty archive, or a truncated header
      rc = n_bytes ? 1 : 0;
      if (rc) ws.fallback = kTarTruncated;
    } else {
      on_gpu = rs.reason == kReqUsedGpu;
      if (on_gpu) ReqPassInit(a, &rq);
      if (on_gpu) rq.skip = with_skip;
      rc = ChainOnGpu(c.get(), dev_tar, n_bytes, 0, 0, who, &head, &recs, &names, &ws, on_gpu ? &rq : nullptr);
    }
    a->tar_fallback_last.store(ws.fallback);
    if (rc < 0) {
      GiveCtx(a, std::move(c));
      return -2;
    }
    if (rc == 1 && rs.reason == kReqUsedGpu) {
      rs.reason = kReqLayerFellBack;
      if (ss.reason == kSkipRan) ss.reason = kSkipNoStage;
    }
    if (rc == 0) {
      const double th = NowMs();
      tsg_device_tar_stats tmp{};
      double hm[3] = {0, 0, 0};
      if (on_gpu) {
        rc = FilesToIndex(a, rq.counts[0], rq.recs, rq.blob, head.stop, n_bytes, head.candidates, &ix->d,
                          st ? st : &tmp, &rs, rq.skip.get());
        if (rc == 1) {  // an asked name is a skipped directory: the host half of the walk, from its records
          rs = tsg_tar_required_stats{};
          rs.reason = kReqAskedSkipDir;
          ss.reason = kSkipAskedDir;
          rc = RefusedLayerToIndex(a, c.get(), who, (head.entries * sizeof(tsg_tar_entry_rec) + 255) & ~uint64_t(255), 0,
                                   0, head, n_bytes, &ix->d, st ? st : &tmp);
        } else if (rq.skip) {
          ss.table_slots = rq.slots;
          ss.ms_kernel = rq.ms_skip;
        }
        rs.ms_kernel = rq.ms_kernel;
        rs.ms_copy = rq.ms_copy;
        rs.ms_host = NowMs() - th;
      } else {
        if (rs.reason == kReqUsedGpu) rs.mode = 1;  // (an archive without a block: nothing to decide)
        rc = EntriesToIndex(a, recs, head.entries, names, head.name_bytes, head.stop, n_bytes, head.candidates, &ix->d,
                            st ? st : &tmp, hm);
      }
      ws.ms_host = NowMs() - th;
      GiveCtx(a, std::move(c));
      if (rc < 0) return -2;  // (records that contradict the name blob: the layer changed under the pass)
      if (st) {
        st->kernel_runs = 1;
        st->ms_kernel = ws.ms_candidates + ws.ms_entries + ws.ms_mark + ws.ms_compact;
        st->ms_total = NowMs() - t0;
      }
      if (std::getenv("TSG_WALK_DEBUG"))
        std::fprintf(stderr, "device tar index (gpu walk): candidates %.2f ms, entries %.2f ms, mark %.2f ms, compact %.2f ms, "
                     "copy %.2f ms, host %.2f ms (classify %.1f, join %.1f, Required + index %.1f), total %.1f ms (%llu entries)\n",
                     ws.ms_candidates, ws.ms_entries, ws.ms_mark, ws.ms_compact, ws.ms_copy, ws.ms_host, hm[0], hm[1],
                     hm[2], NowMs() - t0,
                     static_cast<unsigned long long>(head.entries));
      ix->ws = ws;
      ix->rs = rs;
      ix->ss = ss;
      *out = ix.release();
      return 0;
    }
  }
  uint64_t capacity = g_tar_capacity.load() ? g_tar_capacity.load() : n_bytes / 4096 + 1024;
  uint64_t count = 0, runs = 0;
  double ms_kernel = 0;
  for (; runs < 2 && ok(e); ) {
    if (c->cap_rec < capacity) {
      if (c->d_rec) (void)hipFree(c->d_rec);
      c->d_rec = nullptr;
      c->cap_rec = 0;
      if (ok(hipMalloc(&c->d_rec, capacity * kTarRecordBytes))) c->cap_rec = capacity;
    }
    if (ok(e) && ok(hipMemsetAsync(c->d_count, 0, 4, c->s)) && ok(hipEventRecord(c->e0, c->s)) &&
        ok(TarHeaders(dev_tar, n_bytes, static_cast<uint8_t*>(c->d_rec), uint32_t(capacity), c->d_count, 0, c->s)) &&
        ok(hipEventRecord(c->e1, c->s)) &&
        ok(hipMemcpyAsync(c->h_count, c->d_count, 4, hipMemcpyDeviceToHost, c->s)) && ok(hipStreamSynchronize(c->s))) {
      runs++;
      count = *c->h_count;
      float ms = 0;
      if (hipEventElapsedTime(&ms, c->e0, c->e1) == hipSuccess) ms_kernel += ms;
      if (count <= capacity) break;
      capacity = count;  // the buffer was too small: once more, with room for every candidate
    }
  }
  const double t_kernel = NowMs();
  if (ok(e) && count > capacity) e = hipErrorUnknown;  // (the layer changed between the runs)
  if (ok(e) && c->cap_h < count) {
    if (c->h_rec) (void)hipHostFree(c->h_rec);
    c->h_rec = nullptr;
    c->cap_h = 0;
    const uint64_t want = count + 64;
    if (ok(hipHostMalloc(reinterpret_cast<void**>(&c->h_rec), want * kTarRecordBytes, hipHostMallocDefault)))
      c->cap_h = want;
  }
  if (ok(e) && count)
    ok(hipMemcpyAsync(c->h_rec, c->d_rec, count * kTarRecordBytes, hipMemcpyDeviceToHost, c->s)) &&
        ok(hipStreamSynchronize(c->s));
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(c->s);  // nothing of a failed pass is left queued on a pooled stream
    SetError(who + ": " + hipGetErrorString(e));
    return -2;
  }
  hipStream_t s = c->s;
  const double t_back = NowMs();
  IndexedTarSrc src(reinterpret_cast<const TarRecord*>(c->h_rec), size_t(count),
                    [&](uint64_t off, uint64_t len, uint8_t* dst) {
                      hipError_t r = hipMemcpyAsync(dst, dev_tar + off, len, hipMemcpyDeviceToHost, s);
                      if (r == hipSuccess) r = hipStreamSynchronize(s);
                      if (r != hipSuccess) SetError(who + ": " + hipGetErrorString(r));
                      return r == hipSuccess;
                    });
  std::unique_ptr<tsg_tar_index> ix(new tsg_tar_index());
  ix->dev_tar = dev_tar;
  ix->n_bytes = n_bytes;
  const double t_sort = NowMs();
  const int rc = WalkRecords(a, src, n_bytes, &ix->d);
  const bool copy_failed = src.failed();  // (a HIP error, its text set: not a malformed archive)
  GiveCtx(a, std::move(c));
  if (std::getenv("TSG_WALK_DEBUG"))  // where an index call's time goes
    std::fprintf(stderr, "device tar index: kernel runs + buffers %.1f ms, records back %.1f ms (%llu), sort %.1f ms, "
                 "chain walk + Required %.1f ms\n", t_kernel - t0, t_back - t_kernel,
                 static_cast<unsigned long long>(count), t_sort - t_back, NowMs() - t_sort);
  if (rc < 0) return copy_failed ? -2 : -3;
  FillStats(st, ix->d, src, n_bytes, count, runs, ms_kernel, NowMs() - t0);
  ix->ws = ws;
  ix->rs = rs;  // (mode 0: the reason says why Required ran on the host)
  ix->ss = ss;
  *out = ix.release();
  return 0;
}

int tsg_analyzer_index_device_tar(tsg_analyzer* a, const tsg_device_tar* t, tsg_tar_index** out,
                                  tsg_device_tar_stats* st) {
  using namespace tsg;
  const std::string who = "tsg_analyzer_index_device_tar";
  if (out) *out = nullptr;
  if (!a || !t || !out) {
    SetError(who + ": NULL analyzer, tar or out");
    return -1;
  }
  if (t->struct_size == TSG_DEVICE_TAR_SIZE_V1 && !StatsSizeOk(st, who.c_str())) return -1;
  if (!DeviceTarOk(who, t)) return -1;
  return IndexOneLayer(a, who, static_cast<const uint8_t*>(t->dev_tar), t->n_bytes, nullptr, out, st);
}

int tsg_analyzer_index_device_tars(tsg_analyzer* a, const tsg_device_tars* t, tsg_tar_index** out,
                                   tsg_device_tar_stats* st, tsg_tar_forest_stats* fs, uint32_t* bad_layer) {
  using namespace tsg;
  const std::string who = "tsg_analyzer_index_device_tars";
  if (!a || !t || !out) {
    SetError(who + ": NULL analyzer, tars or out");
    return -1;
  }
  if (t->struct_size != TSG_DEVICE_TARS_SIZE_V1) {
    SetError(who + ": tsg_device_tars.struct_size " + std::to_string(t->struct_size) +
             " is not a size this library knows (v1 = " + std::to_string(TSG_DEVICE_TARS_SIZE_V1) + ")");
    return -1;
  }
  if (t->n_layers == 0 || t->n_layers > TSG_DEVICE_TARS_MAX_LAYERS) {
    SetError(who + ": n_layers " + std::to_string(t->n_layers) + " is not from 1 to " +
             std::to_string(TSG_DEVICE_TARS_MAX_LAYERS));
    return -1;
  }
  const uint32_t n = t->n_layers;
  for (uint32_t k = 0; k < n; k++) out[k] = nullptr;
  if (!t->layers) {
    SetError(who + ": layers is NULL");
    return -1;
  }
  if (fs && fs->struct_size != TSG_TAR_FOREST_STATS_SIZE_V1) {
    SetError(who + ": tsg_tar_forest_stats.struct_size " + std::to_string(fs->struct_size) +
             " is not a size this library knows (v1 = " + std::to_string(TSG_TAR_FOREST_STATS_SIZE_V1) + ")");
    return -1;
  }
  for (uint32_t k = 0; k < n; k++) {
    const std::string lw = who + ": layer " + std::to_string(k);
    if (t->layers[k].struct_size == TSG_DEVICE_TAR_SIZE_V1 && st && !StatsSizeOk(&st[k], lw.c_str())) return -1;
    if (!DeviceTarOk(lw, &t->layers[k])) return -1;
  }
  const double t0 = NowMs();
  tsg_tar_forest_stats F{};
  F.struct_size = TSG_TAR_FOREST_STATS_SIZE_V1;
  F.layers = n;
  std::vector<std::unique_ptr<tsg_tar_index>> ixs(n);  // (an error return frees what was made)
  std::vector<const void*> ptrs(n);
  std::vector<uint64_t> nb(n);
  for (uint32_t k = 0; k < n; k++) {
    ptrs[k] = t->layers[k].dev_tar;
    nb[k] = t->layers[k].n_bytes;
  }
  const int mode = a->tar_walk.load();
  std::vector<uint8_t> single(n, mode == 1 ? 0 : 1);  // layers the single-layer path indexes
  std::vector<uint32_t> fallback(n, 0);
  if (mode == 1) {
    const int device = a->s->s->device();
    if (device < 0) {
      SetError(who + ": no GPU engine bound to this analyzer's scanner");
      return -2;
    }
    std::unique_ptr<TarIndexCtx> c = hipSetDevice(device) == hipSuccess ? TakeCtx(a) : nullptr;
    if (!c) {
      SetError(who + ": stream / events");
      return -2;
    }
    for (uint32_t first = 0; first < n;) {
      const uint32_t cnt = TarForestCut(nb.data(), n, first, kTarDefaultSegment);
      if (cnt == 0) {  // too large for a pass of its own
        single[first] = 1;
        fallback[first++] = kTarTooLarge;
        continue;
      }
      ForestPass P;
      ReqPass rq;  // Required on the GPU (tsg_analyzer_set_tar_required): one stage for the pass's layers
      uint32_t skip_reason = 0;
      std::shared_ptr<const TarSkipOpts> with_skip;
      const uint32_t req_reason = RequiredReason(a, 1, &skip_reason, &with_skip);
      const bool on_gpu = req_reason == kReqUsedGpu;
      if (on_gpu) ReqPassInit(a, &rq);
      if (on_gpu) rq.skip = with_skip;
      std::vector<uint8_t> refused(cnt, 0);  // layers whose asked names hold a skipped directory
      if (ForestOnGpu(c.get(), ptrs.data() + first, nb.data() + first, cnt, 0, 0, who, &P, &F, on_gpu ? &rq : nullptr) <
          0) {
        GiveCtx(a, std::move(c));
        return -2;
      }
      // the host half per layer, the layers side by side on the host pool
      std::vector<int> rcs(cnt, 0);
      const double th = NowMs();
      ParallelFor(cnt, 16, [&](size_t j) {
        const uint32_t k = first + uint32_t(j);
        const TarChainHead& head = P.heads[j];
        if (head.stop.kind != kTarStopEnd) {
          single[k] = 1;
          fallback[k] = head.stop.reason ? head.stop.reason : uint32_t(kTarNotCandidate);
          return;
        }
        const double tl = NowMs();
        std::unique_ptr<tsg_tar_index> ix(new tsg_tar_index());
        ix->dev_tar = static_cast<const uint8_t*>(ptrs[k]);
        ix->n_bytes = nb[k];
        tsg_device_tar_stats tmp{};
        tsg_device_tar_stats* sk = st ? &st[k] : &tmp;
        ix->rs.reason = req_reason;
        SkipStatsInit(a, skip_reason, &ix->ss);
        if (on_gpu) {
          const TarRequiredCounts& cn = rq.counts[j];
          rcs[j] = FilesToIndex(a, cn, rq.recs + cn.rec_first, rq.blob + cn.path_first, head.stop, nb[k],
                                head.candidates, &ix->d, sk, &ix->rs, rq.skip.get());
          if (rcs[j] == 1) {  // (indexed below, on this thread: the copies are HIP calls)
            refused[j] = 1;
            rcs[j] = 0;
          } else if (rq.skip) {
            ix->ss.table_slots = rq.slots;  // (shared by the pass's layers, as ms_kernel is)
            ix->ss.ms_kernel = rq.ms_skip;
          }
          ix->rs.ms_kernel = rq.ms_kernel;  // (the stage is shared by the pass's layers, as its copies are)
          ix->rs.ms_copy = rq.ms_copy;
          ix->rs.ms_host = NowMs() - tl;
        } else {
          rcs[j] = EntriesToIndex(a, P.recs + P.rec_base[j], head.entries, P.names + P.name_base[j], head.name_bytes,
                                  head.stop, nb[k], head.candidates, &ix->d, sk);
        }
        if (rcs[j] < 0) return;
        ix->ws.walk = 1;
        ix->ws.chain_entries = head.entries;
        ix->ws.name_bytes = head.name_bytes;
        ix->ws.segments = (nb[k] / 512 + P.L.segment - 1) / P.L.segment;
        ix->ws.ms_host = NowMs() - tl;
        sk->kernel_runs = 1;
        sk->ms_kernel = 0;  // (the kernels are shared by the layers: tsg_tar_forest_stats)
        sk->ms_total = ix->ws.ms_host;
        ixs[k] = std::move(ix);
      });
      for (uint32_t j = 0; j < cnt; j++) {
        if (!refused[j] || rcs[j] < 0) continue;
        tsg_tar_index* ix = ixs[first + j].get();
        tsg_device_tar_stats tmp{};
        ix->rs = tsg_tar_required_stats{};
        ix->rs.reason = kReqAskedSkipDir;
        ix->ss.reason = kSkipAskedDir;
        const uint64_t rec_bytes_all = (P.rec_base[cnt] * sizeof(tsg_tar_entry_rec) + 255) & ~uint64_t(255);
        rcs[j] = RefusedLayerToIndex(a, c.get(), who, rec_bytes_all, P.rec_base[j], P.name_base[j], P.heads[j],
                                     nb[first + j], &ix->d, st ? &st[first + j] : &tmp);
      }
      F.ms_host += NowMs() - th;
      for (uint32_t j = 0; j < cnt; j++) {
        if (rcs[j] < 0) {  // (records that contradict the name blob: the layer changed under the pass)
          GiveCtx(a, std::move(c));
          SetError(who + ": layer " + std::to_string(first + j) + ": the entry records contradict the name blob");
          return -2;
        }
        if (ixs[first + j]) F.batched++;
      }
      first += cnt;
    }
    GiveCtx(a, std::move(c));  // (buffers above 16 MiB are freed here: once per image)
    uint32_t last = 0;
    for (uint32_t k = 0; k < n && !last; k++) last = fallback[k];
    a->tar_fallback_last.store(last);
  }
  // The layers left to the single-layer path, in order: the first malformed one ends the call.
  for (uint32_t k = 0; k < n; k++) {
    if (!single[k]) continue;
    tsg_tar_index* ix = nullptr;
    const int rc = IndexOneLayer(a, who, static_cast<const uint8_t*>(ptrs[k]), nb[k], mode == 1 ? &fallback[k] : nullptr,
                                 &ix, st ? &st[k] : nullptr);
    if (rc != 0) {
      const std::string msg = tsg_last_error();
      SetError("layer " + std::to_string(k) + ": " + msg);
      if (rc == -3 && bad_layer) *bad_layer = k;  // (a -2 names its layer in the text only)
      return rc;
    }
    ixs[k].reset(ix);
    if (mode == 1) F.fallbacks++;
  }
  for (uint32_t k = 0; k < n; k++) out[k] = ixs[k].release();
  F.ms_total = NowMs() - t0;
  if (fs) *fs = F;
  return 0;
}

int tsg_debug_tar_forest_layout(const uint64_t* n_bytes, uint32_t n_layers, uint32_t segment_blocks, uint64_t* v0_out,
                                uint64_t* v_blocks_out, uint32_t* first_pass_out) {
  using namespace tsg;
  const uint32_t seg = segment_blocks ? segment_blocks : kTarDefaultSegment;
  if (!n_bytes || !v0_out || !v_blocks_out || !first_pass_out || n_layers == 0 || n_layers > kTarForestMaxLayers ||
      seg < kTarMinSegment || (seg & (seg - 1))) {
    SetError("tsg_debug_tar_forest_layout: NULL argument, a layer count out of range, or no segment size");
    return -1;
  }
  uint64_t v = 0;
  for (uint32_t k = 0; k < n_layers; k++) {
    v0_out[k] = v;
    v += TarForestSpan(n_bytes[k], seg);
  }
  *v_blocks_out = v;
  *first_pass_out = TarForestCut(n_bytes, n_layers, 0, seg);
  return 0;
}

int tsg_debug_tar_forest(int device, const void* const* dev_tars, const uint64_t* n_bytes, uint32_t n_layers,
                         uint32_t segment_blocks, uint32_t grid_cap, uint64_t* heads_out, uint64_t* rec_base_out,
                         uint64_t* name_base_out, void* records_out, uint64_t rec_cap, uint64_t* n_records,
                         uint8_t* names_out, uint64_t name_cap, uint64_t* name_bytes) {
  using namespace tsg;
  const std::string who = "tsg_debug_tar_forest";
  bool bad = !dev_tars || !n_bytes || !heads_out || !rec_base_out || !name_base_out || !n_records || !name_bytes ||
             n_layers == 0 || n_layers > kTarForestMaxLayers || (rec_cap && !records_out) || (name_cap && !names_out);
  for (uint32_t k = 0; !bad && k < n_layers; k++)
    bad = (n_bytes[k] >= 512 && !dev_tars[k]) || reinterpret_cast<uintptr_t>(dev_tars[k]) % 16 != 0;
  if (bad) {
    SetError(who + ": NULL or misaligned pointer, or a layer count out of range");
    return -2;
  }
  *n_records = *name_bytes = 0;
  TarIndexCtx c;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c.s, hipStreamNonBlocking);
  if (e != hipSuccess) {
    SetError(who + ": " + hipGetErrorString(e));
    return -2;
  }
  ForestPass P;
  if (ForestOnGpu(&c, dev_tars, n_bytes, n_layers, segment_blocks, grid_cap, who, &P, nullptr) < 0) return -2;
  std::memcpy(heads_out, P.heads, size_t(n_layers) * sizeof(TarChainHead));
  std::memcpy(rec_base_out, P.rec_base.data(), size_t(n_layers) * 8);
  std::memcpy(name_base_out, P.name_base.data(), size_t(n_layers) * 8);
  *n_records = P.rec_base[n_layers];
  *name_bytes = P.name_base[n_layers];
  if (*n_records > rec_cap || *name_bytes > name_cap) {
    SetError(who + ": the output buffers are too small");
    return -3;
  }
  if (*n_records) std::memcpy(records_out, P.recs, size_t(*n_records) * sizeof(tsg_tar_entry_rec));
  if (*name_bytes) std::memcpy(names_out, P.names, size_t(*name_bytes));
  return 0;
}

int tsg_analyzer_set_tar_walk(tsg_analyzer* a, int mode) {
  if (!a) {
    tsg::SetError("tsg_analyzer_set_tar_walk: NULL analyzer");
    return -1;
  }
  if (mode != 0 && mode != 1) {
    tsg::SetError("tsg_analyzer_set_tar_walk: mode " + std::to_string(mode) + " is not 0 (host) or 1 (gpu)");
    return -1;
  }
  a->tar_walk.store(mode);
  return 0;
}

int tsg_analyzer_get_tar_walk(const tsg_analyzer* a, int* mode) {
  if (!a || !mode) {
    tsg::SetError("tsg_analyzer_get_tar_walk: NULL argument");
    return -1;
  }
  *mode = a->tar_walk.load();
  return 0;
}

int tsg_analyzer_set_tar_required(tsg_analyzer* a, int mode) {
  if (!a) {
    tsg::SetError("tsg_analyzer_set_tar_required: NULL analyzer");
    return -1;
  }
  if (mode != 0 && mode != 1) {
    tsg::SetError("tsg_analyzer_set_tar_required: mode " + std::to_string(mode) + " is not 0 (host) or 1 (gpu)");
    return -1;
  }
  a->tar_required.store(mode);
  return 0;
}

int tsg_analyzer_get_tar_required(const tsg_analyzer* a, int* mode) {
  if (!a || !mode) {
    tsg::SetError("tsg_analyzer_get_tar_required: NULL argument");
    return -1;
  }
  *mode = a->tar_required.load();
  return 0;
}

int tsg_analyzer_set_tar_required_skip(tsg_analyzer* a, int mode) {
  if (!a) {
    tsg::SetError("tsg_analyzer_set_tar_required_skip: NULL analyzer");
    return -1;
  }
  if (mode != 0 && mode != 1) {
    tsg::SetError("tsg_analyzer_set_tar_required_skip: mode " + std::to_string(mode) + " is not 0 (host) or 1 (gpu)");
    return -1;
  }
  a->tar_required_skip.store(mode);
  return 0;
}

int tsg_analyzer_get_tar_required_skip(const tsg_analyzer* a, int* mode) {
  if (!a || !mode) {
    tsg::SetError("tsg_analyzer_get_tar_required_skip: NULL argument");
    return -1;
  }
  *mode = a->tar_required_skip.load();
  return 0;
}

int tsg_tar_index_required_skip_stats(const tsg_tar_index* ix, tsg_tar_required_skip_stats* out) {
  if (!ix || !out) {
    tsg::SetError("tsg_tar_index_required_skip_stats: NULL argument");
    return -1;
  }
  if (out->struct_size != TSG_TAR_REQUIRED_SKIP_STATS_SIZE_V1) {
    tsg::SetError("tsg_tar_index_required_skip_stats: tsg_tar_required_skip_stats.struct_size " +
                  std::to_string(out->struct_size) + " is not a size this library knows (v1 = " +
                  std::to_string(TSG_TAR_REQUIRED_SKIP_STATS_SIZE_V1) + ")");
    return -1;
  }
  *out = ix->ss;
  out->struct_size = TSG_TAR_REQUIRED_SKIP_STATS_SIZE_V1;
  out->reserved = 0;
  out->skipped_dirs = ix->d.skip.skipped_dirs;  // (whichever half produced them)
  out->skipped_files = ix->d.skip.skipped_files;
  out->under_skipped_dir = ix->d.skip.under_skipped_dir;
  return 0;
}

int tsg_tar_index_required_stats(const tsg_tar_index* ix, tsg_tar_required_stats* out) {
  if (!ix || !out) {
    tsg::SetError("tsg_tar_index_required_stats: NULL argument");
    return -1;
  }
  if (out->struct_size != TSG_TAR_REQUIRED_STATS_SIZE_V1) {
    tsg::SetError("tsg_tar_index_required_stats: tsg_tar_required_stats.struct_size " +
                  std::to_string(out->struct_size) + " is not a size this library knows (v1 = " +
                  std::to_string(TSG_TAR_REQUIRED_STATS_SIZE_V1) + ")");
    return -1;
  }
  *out = ix->rs;
  out->struct_size = TSG_TAR_REQUIRED_STATS_SIZE_V1;
  out->reserved = 0;
  return 0;
}

int tsg_debug_tar_required_tables(const tsg_analyzer* a, void* path_table_out, uint64_t path_cap, void* sure_table_out,
                                  uint64_t sure_cap, uint32_t* have_out) {
  using namespace tsg;
  if (!a || !have_out || (path_cap && !path_table_out) || (sure_cap && !sure_table_out)) {
    SetError("tsg_debug_tar_required_tables: NULL argument");
    return -1;
  }
  const SecretScanner::AllowTables t = a->s->s->allow_tables();
  *have_out = 0;
  if (t.host_path) {
    if (path_cap < sizeof(PathTable)) {
      SetError("tsg_debug_tar_required_tables: the path table takes " + std::to_string(sizeof(PathTable)) + " bytes");
      return -1;
    }
    std::memcpy(path_table_out, t.host_path, sizeof(PathTable));
    *have_out |= 1u;
  }
  if (t.host_path && t.host_sure) {
    if (sure_cap < sizeof(SureTable)) {
      SetError("tsg_debug_tar_required_tables: the sure table takes " + std::to_string(sizeof(SureTable)) + " bytes");
      return -1;
    }
    std::memcpy(sure_table_out, t.host_sure, sizeof(SureTable));
    *have_out |= 2u;
  }
  return 0;
}

// tsg_debug_tar_required, and with skip options tsg_debug_tar_required_skip.
static int DebugTarRequired(const std::string& who, tsg_analyzer* a, const void* records, uint64_t n_records,
                            const uint8_t* names, uint64_t name_bytes, const uint64_t* rec_base,
                            const uint64_t* name_base, uint32_t n_layers, uint32_t grid_cap,
                            std::shared_ptr<const tsg::TarSkipOpts> skip, uint64_t forced_slots, uint8_t* verdicts_out,
                            void* file_recs_out, uint64_t rec_cap, uint64_t* n_file_recs, uint8_t* blob_out,
                            uint64_t blob_cap, uint64_t* blob_bytes, uint64_t* counts_out, uint64_t* slots_out) {
  using namespace tsg;
  if (!a || !rec_base || !name_base || n_layers == 0 || !n_file_recs || !blob_bytes || !counts_out ||
      (n_records && (!records || !verdicts_out)) || (name_bytes && !names) || (rec_cap && !file_recs_out) ||
      (blob_cap && !blob_out) || n_records >= (uint64_t(1) << 31)) {
    SetError(who + ": NULL argument, no layer, or too many records");
    return -2;
  }
  // the table the stage searches: ascending, from (0, 0) to (n_records, name_bytes)
  bool rows_ok = rec_base[0] == 0 && name_base[0] == 0 && rec_base[n_layers] == n_records &&
                 name_base[n_layers] == name_bytes;
  for (uint32_t k = 0; rows_ok && k < n_layers; k++)
    rows_ok = rec_base[k] <= rec_base[k + 1] && name_base[k] <= name_base[k + 1];
  if (!rows_ok) {
    SetError(who + ": the layer table does not ascend from (0, 0) to (n_records, name_bytes)");
    return -2;
  }
  *n_file_recs = *blob_bytes = 0;
  const int device = a->s->s->device();
  if (device < 0) {
    SetError(who + ": no GPU engine bound to this analyzer's scanner");
    return -2;
  }
  TarIndexCtx c;
  uint8_t* d_in = nullptr;
  const uint64_t rec_bytes = (n_records * sizeof(tsg_tar_entry_rec) + 255) & ~uint64_t(255);
  hipError_t e = hipSetDevice(device);
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  ReqPass R;
  ReqPassInit(a, &R);
  R.skip = skip;
  R.forced_slots = forced_slots;
  std::vector<uint8_t> dec;
  if (ok(e) && ok(hipStreamCreateWithFlags(&c.s, hipStreamNonBlocking)) &&
      ok(hipMalloc(reinterpret_cast<void**>(&d_in), rec_bytes + name_bytes + 256)) &&
      (n_records == 0 || ok(hipMemcpy(d_in, records, n_records * sizeof(tsg_tar_entry_rec), hipMemcpyHostToDevice))) &&
      (name_bytes == 0 || ok(hipMemcpy(d_in + rec_bytes, names, name_bytes, hipMemcpyHostToDevice))))
    ok(RequiredOnGpu(&c, &R, d_in, d_in + rec_bytes, n_records, name_bytes, rec_base, name_base, n_layers, grid_cap, &dec));
  if (c.s) (void)hipStreamSynchronize(c.s);
  if (d_in) (void)hipFree(d_in);
  if (R.bad_slots) {
    SetError(who + ": table_slots " + std::to_string(forced_slots) + " is no power of two of at least " +
             std::to_string(4 * R.n_dirs) + " (twice the keys of " + std::to_string(R.n_dirs) + " recorded directories)");
    return -1;
  }
  if (e != hipSuccess) {
    SetError(who + ": " + hipGetErrorString(e));
    return -2;
  }
  if (slots_out) *slots_out = R.slots;
  for (uint64_t i = 0; i < n_records; i++) verdicts_out[i] = dec[size_t(i) * 16 + 12];
  std::memcpy(counts_out, R.counts, size_t(n_layers) * sizeof(TarRequiredCounts));
  *n_file_recs = R.n_recs;
  *blob_bytes = R.blob_bytes;
  if (R.n_recs > rec_cap || R.blob_bytes > blob_cap) {
    SetError(who + ": the output buffers are too small");
    return -3;
  }
  if (R.n_recs) std::memcpy(file_recs_out, R.recs, size_t(R.n_recs) * sizeof(tsg_tar_file_rec));
  if (R.blob_bytes) std::memcpy(blob_out, R.blob, size_t(R.blob_bytes));
  if (R.bad) {
    SetError(who + ": " + std::to_string(R.bad) + " record(s) have their name outside their layer's name blob");
    return -4;
  }
  return 0;
}

int tsg_debug_tar_required(tsg_analyzer* a, const void* records, uint64_t n_records, const uint8_t* names,
                           uint64_t name_bytes, const uint64_t* rec_base, const uint64_t* name_base, uint32_t n_layers,
                           uint32_t grid_cap, uint8_t* verdicts_out, void* file_recs_out, uint64_t rec_cap,
                           uint64_t* n_file_recs, uint8_t* blob_out, uint64_t blob_cap, uint64_t* blob_bytes,
                           uint64_t* counts_out) {
  return DebugTarRequired("tsg_debug_tar_required", a, records, n_records, names, name_bytes, rec_base, name_base,
                          n_layers, grid_cap, nullptr, 0, verdicts_out, file_recs_out, rec_cap, n_file_recs, blob_out,
                          blob_cap, blob_bytes, counts_out, nullptr);
}

int tsg_debug_tar_required_skip(tsg_analyzer* a, const void* records, uint64_t n_records, const uint8_t* names,
                                uint64_t name_bytes, const uint64_t* rec_base, const uint64_t* name_base,
                                uint32_t n_layers, uint32_t grid_cap, const char* const* skip_dirs, uint32_t n_dirs,
                                const char* const* skip_files, uint32_t n_files, uint64_t table_slots,
                                uint8_t* verdicts_out, void* file_recs_out, uint64_t rec_cap, uint64_t* n_file_recs,
                                uint8_t* blob_out, uint64_t blob_cap, uint64_t* blob_bytes, uint64_t* counts_out,
                                uint64_t* table_slots_out) {
  using namespace tsg;
  const std::string who = "tsg_debug_tar_required_skip";
  bool bad = (n_dirs && !skip_dirs) || (n_files && !skip_files) || (n_dirs == 0 && n_files == 0);
  for (uint32_t k = 0; !bad && k < n_dirs; k++) bad = !skip_dirs[k];
  for (uint32_t k = 0; !bad && k < n_files; k++) bad = !skip_files[k];
  if (bad) {
    SetError(who + ": no pattern, or a NULL pattern");
    return -1;
  }
  auto o = std::make_shared<TarSkipOpts>();
  o->dirs.assign(skip_dirs, skip_dirs + n_dirs);
  o->files.assign(skip_files, skip_files + n_files);
  o->Classify();
  if (!o->dev_ok) {
    SetError(who + ": a pattern, or the set, is outside what the device takes");
    return -1;
  }
  if (table_slots_out) *table_slots_out = 0;
  return DebugTarRequired(who, a, records, n_records, names, name_bytes, rec_base, name_base, n_layers, grid_cap, o,
                          table_slots, verdicts_out, file_recs_out, rec_cap, n_file_recs, blob_out, blob_cap, blob_bytes,
                          counts_out, table_slots_out);
}

int tsg_debug_tar_skip_classify(const char* const* skip_dirs, uint32_t n_dirs, const char* const* skip_files,
                                uint32_t n_files, uint8_t* forms_out) {
  using namespace tsg;
  if ((n_dirs && !skip_dirs) || (n_files && !skip_files)) {
    SetError("tsg_debug_tar_skip_classify: NULL pattern array with a non-zero count");
    return -1;
  }
  TarSkipOpts o;
  o.dirs.assign(skip_dirs, skip_dirs + n_dirs);
  o.files.assign(skip_files, skip_files + n_files);
  o.Classify();
  if (!o.dev_ok) return 0;
  for (uint32_t k = 0; forms_out && k < n_dirs; k++) forms_out[k] = o.dev.pat[k].form;
  for (uint32_t k = 0; forms_out && k < n_files; k++) forms_out[n_dirs + k] = o.dev.pat[kTarSkipMaxPatterns + k].form;
  return 1;
}

int tsg_debug_tar_skip_match(const char* pattern, const uint8_t* fp, uint32_t len) {
  using namespace tsg;
  if (!pattern || (len && !fp)) {
    SetError("tsg_debug_tar_skip_match: NULL argument");
    return -1;
  }
  TarSkipTable t;
  if (!TarSkipClassify({std::string(pattern)}, {}, &t)) return -1;
  return TarSkipMatch(&t, false, fp, len) ? 1 : 0;
}

int tsg_debug_index_tar_files(tsg_analyzer* a, const void* file_recs, uint64_t n_recs, const uint8_t* blob,
                              uint64_t blob_bytes, const uint64_t* counts, const uint64_t* stop, uint64_t n_bytes,
                              uint64_t candidates_given, tsg_tar_index** out, tsg_device_tar_stats* st) {
  using namespace tsg;
  const char* who = "tsg_debug_index_tar_files";
  if (out) *out = nullptr;
  if (!a || !out || !stop || !counts || (n_recs && !file_recs) || (blob_bytes && !blob)) {
    SetError(std::string(who) + ": NULL argument");
    return -1;
  }
  if (!StatsSizeOk(st, who)) return -1;
  if (stop[0] != kTarStopEnd) {
    SetError(std::string(who) + ": the stop is not END (an INCOMPLETE chain is walked by the host walk)");
    return -1;
  }
  const double t0 = NowMs();
  tsg_tar_stop sp{};
  sp.kind = uint32_t(stop[0]);
  sp.reason = uint32_t(stop[1]);
  sp.offset = stop[2];
  sp.ext_visited = stop[3];
  TarRequiredCounts cnt;
  std::memcpy(&cnt, counts, sizeof(cnt));
  if (cnt.records != n_recs || cnt.path_bytes != blob_bytes) {
    SetError(std::string(who) + ": the counts contradict the file records");
    return -1;
  }
  std::unique_ptr<tsg_tar_index> ix(new tsg_tar_index());
  ix->n_bytes = n_bytes;
  tsg_device_tar_stats tmp{};
  // (with tsg_analyzer_set_tar_required_skip mode 1 and options the device takes, the records are
  // those of a stage that ran its skip stage)
  uint32_t skip_reason = 0;
  std::shared_ptr<const TarSkipOpts> with_skip;
  const std::shared_ptr<const TarSkipOpts> opts = a->TarSkip();
  if (a->tar_required_skip.load() == 1 && opts && opts->any() && opts->dev_ok) with_skip = opts;
  skip_reason = a->tar_required_skip.load() != 1 ? kSkipSetterOff : !(opts && opts->any()) ? kSkipNoOptions
                : !opts->dev_ok ? kSkipPatterns : kSkipRan;
  const int rc = FilesToIndex(a, cnt, static_cast<const tsg_tar_file_rec*>(file_recs), blob, sp, n_bytes, candidates_given,
                              &ix->d, st ? st : &tmp, &ix->rs, with_skip.get());
  if (rc == 1) {
    SetError(std::string(who) + ": an asked name is a skipped directory (the layer is indexed from the walk's records)");
    return 1;
  }
  if (rc < 0) return -1;
  SkipStatsInit(a, skip_reason, &ix->ss);
  ix->rs.ms_host = NowMs() - t0;
  if (st) {
    st->kernel_runs = 0;
    st->ms_kernel = 0;
    st->ms_total = NowMs() - t0;
  }
  ix->ws.walk = 1;
  ix->ws.chain_entries = cnt.entries;
  *out = ix.release();
  return 0;
}

int tsg_tar_index_walk_stats(const tsg_tar_index* ix, tsg_tar_walk_stats* out) {
  if (!ix || !out) {
    tsg::SetError("tsg_tar_index_walk_stats: NULL argument");
    return -1;
  }
  if (out->struct_size != TSG_TAR_WALK_STATS_SIZE_V1) {
    tsg::SetError("tsg_tar_index_walk_stats: tsg_tar_walk_stats.struct_size " + std::to_string(out->struct_size) +
                  " is not a size this library knows (v1 = " + std::to_string(TSG_TAR_WALK_STATS_SIZE_V1) + ")");
    return -1;
  }
  *out = ix->ws;
  out->struct_size = TSG_TAR_WALK_STATS_SIZE_V1;
  out->reserved = 0;
  return 0;
}

int tsg_tar_index_skip_stats(const tsg_tar_index* ix, tsg_tar_skip_stats* out) {
  if (!ix || !out) {
    tsg::SetError("tsg_tar_index_skip_stats: NULL argument");
    return -1;
  }
  if (out->struct_size != TSG_TAR_SKIP_STATS_SIZE_V1) {
    tsg::SetError("tsg_tar_index_skip_stats: tsg_tar_skip_stats.struct_size " + std::to_string(out->struct_size) +
                  " is not a size this library knows (v1 = " + std::to_string(TSG_TAR_SKIP_STATS_SIZE_V1) + ")");
    return -1;
  }
  out->reserved = 0;
  out->skipped_dirs = ix->d.skip.skipped_dirs;
  out->skipped_files = ix->d.skip.skipped_files;
  out->under_skipped_dir = ix->d.skip.under_skipped_dir;
  return 0;
}

uint32_t tsg_tar_index_files(const tsg_tar_index* ix) { return ix ? uint32_t(ix->d.files.size()) : 0; }

int tsg_tar_index_file(const tsg_tar_index* ix, uint32_t i, const char** path, uint64_t* path_len,
                       uint64_t* data_off, uint64_t* size) {
  if (!ix || i >= ix->d.files.size()) return -1;
  const tsg::TarIndexFile& f = ix->d.files[i];
  if (path) *path = ix->d.pool.data() + f.path_off;
  if (path_len) *path_len = f.path_len;
  if (data_off) *data_off = f.data_off;
  if (size) *size = f.size;
  return 0;
}

int tsg_tar_index_spans(const tsg_tar_index* ix, uint64_t* start, uint64_t* data_off, uint64_t* size) {
  if (!ix) return -1;
  for (size_t i = 0; i < ix->d.files.size(); i++) {
    if (start) start[i] = ix->d.files[i].start;
    if (data_off) data_off[i] = ix->d.files[i].data_off;
    if (size) size[i] = ix->d.files[i].size;
  }
  return 0;
}

void tsg_tar_index_free(tsg_tar_index* ix) { delete ix; }

int tsg_analyzer_submit_device_tar(tsg_analyzer* a, const tsg_tar_index* ix, uint32_t first, uint32_t count,
                                   tsg_pending** out) {
  using namespace tsg;
  const std::string who = "tsg_analyzer_submit_device_tar";
  if (out) *out = nullptr;
  if (!a || !ix || !out) {
    SetError(who + ": NULL analyzer, index or out");
    return -1;
  }
  if (uint64_t(first) + count > ix->d.files.size()) {
    SetError(who + ": files [" + std::to_string(first) + ", " + std::to_string(uint64_t(first) + count) +
             ") are outside the index of " + std::to_string(ix->d.files.size()));
    return -1;
  }
  if (2 * uint64_t(count) + 1 > 0xFFFFFFFFull) {
    SetError(who + ": too many files for one batch");
    return -1;
  }
  if (!ix->dev_tar) {
    SetError(who + ": the index has no device layer (it was made from given records)");
    return -1;
  }
  if (a->s->s->device() < 0) {
    SetError(who + ": no GPU engine bound to this analyzer's scanner");
    return -2;
  }
  auto plan = std::make_shared<TarBatchPlan>();
  PlanTarBatch(ix->d, first, count, plan.get());
  std::unique_ptr<tsg_pending> p(new tsg_pending());
  p->owned = plan;
  tsg_pending* pp = p.get();
  TarBatchPlan* pl = plan.get();
  const uint8_t* arena = ix->dev_tar + pl->base;
  pp->th = std::thread([a, pl, pp, arena] {
    pthread_setname_np(pthread_self(), "tsg-layer-dev");
    const uint32_t n = uint32_t(pl->path_ptrs.size());
    tsg_device_files f{};
    f.struct_size = TSG_DEVICE_FILES_SIZE_V1;
    f.n_files = n;
    f.dev_arena = arena;
    f.host_offsets = pl->offs.data();
    pl->flags.assign(n, 0);
    std::string err;
    double ms = 0;
    if (!ClassifyOnGpu(a, f, pl->flags.data(), &ms, &err)) {
      pp->rc = -1;
      pp->err = err;
      return;
    }
    TarBatchKinds(pl);
    tsg_batch b{};
    b.n_files = n;
    b.host_arena = nullptr;  // device-only: the candidate files are fetched from HBM
    b.host_offsets = pl->offs.data();
    b.dev_arena = arena;
    b.paths = pl->path_ptrs.data();
    b.path_lens = pl->path_lens.data();
    b.binary = pl->binary.data();
    b.transform = pl->kinds.data();
    pp->rc = tsg_scan(const_cast<tsg_scanner*>(a->s), &b, &pp->r);
    if (pp->rc != 0) {
      pp->err = tsg_last_error();
      return;
    }
    for (uint32_t i = 0; i < n && i < pp->r->files.kind.size(); i++)  // a dropped pseudo-file is types.Secret{}
      if (pl->kinds[i] == kXformDrop) pp->r->files.kind[i] = 0;
  });
  *out = p.release();
  return 0;
}

int tsg_debug_tar_headers(int device, const void* dev_tar, uint64_t n_bytes, uint64_t capacity, uint32_t grid_cap,
                          void* records_out, uint64_t* count_out, double* ms_out) {
  const std::string who = "tsg_debug_tar_headers";
  if (!count_out || (n_bytes >= 512 && !dev_tar) || (capacity && !records_out) ||
      reinterpret_cast<uintptr_t>(dev_tar) % 16 != 0 || reinterpret_cast<uintptr_t>(records_out) % 16 != 0 ||
      ((n_bytes / 512) >> 32) || (capacity >> 32)) {
    tsg::SetError(who + ": NULL or misaligned pointer, or a size out of range");
    return -2;
  }
  hipStream_t s = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  uint32_t* d_count = nullptr;
  uint32_t h_count = 0;
  hipError_t e = hipSetDevice(device);
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  if (ok(e) && ok(hipStreamCreate(&s)) && ok(hipEventCreate(&e0)) && ok(hipEventCreate(&e1)) &&
      ok(hipMalloc(reinterpret_cast<void**>(&d_count), 16)) && ok(hipMemsetAsync(d_count, 0, 4, s)) &&
      ok(hipEventRecord(e0, s)) &&
      ok(tsg::TarHeaders(static_cast<const uint8_t*>(dev_tar), n_bytes, static_cast<uint8_t*>(records_out),
                         uint32_t(capacity), d_count, grid_cap, s)) &&
      ok(hipEventRecord(e1, s)) && ok(hipMemcpyAsync(&h_count, d_count, 4, hipMemcpyDeviceToHost, s)) &&
      ok(hipStreamSynchronize(s))) {
    *count_out = h_count;
    float ms = 0;
    if (ms_out && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) *ms_out = ms;
  }
  if (d_count) (void)hipFree(d_count);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (s) (void)hipStreamDestroy(s);
  if (e != hipSuccess) {
    tsg::SetError(who + ": " + hipGetErrorString(e));
    return -1;
  }
  return 0;
}

void tsg_debug_set_tar_capacity(uint64_t records) { tsg::g_tar_capacity.store(records); }

int tsg_debug_index_tar_records(tsg_analyzer* a, const uint8_t* host_tar, uint64_t n_bytes, const void* records,
                                uint64_t n_records, tsg_tar_index** out, tsg_device_tar_stats* st) {
  using namespace tsg;
  const char* who = "tsg_debug_index_tar_records";
  if (out) *out = nullptr;
  if (!a || !out || (n_bytes && !host_tar) || (n_records && !records)) {
    SetError(std::string(who) + ": NULL argument");
    return -1;
  }
  if (!StatsSizeOk(st, who)) return -1;
  const double t0 = NowMs();
  IndexedTarSrc src(static_cast<const TarRecord*>(records), size_t(n_records),
                    [&](uint64_t off, uint64_t len, uint8_t* dst) {
                      if (off > n_bytes || len > n_bytes - off) {
                        SetError(std::string(who) + ": the walk asked for bytes outside the layer");
                        return false;
                      }
                      std::memcpy(dst, host_tar + off, size_t(len));
                      return true;
                    });
  std::unique_ptr<tsg_tar_index> ix(new tsg_tar_index());
  ix->n_bytes = n_bytes;
  if (WalkRecords(a, src, n_bytes, &ix->d) < 0) return src.failed() ? -2 : -3;
  FillStats(st, ix->d, src, n_bytes, n_records, 0, 0, NowMs() - t0);
  uint32_t skip_reason = 0;
  ix->rs.reason = std::max<uint32_t>(RequiredReason(a, 0, &skip_reason), kReqSetterOff);
  SkipStatsInit(a, skip_reason == kSkipRan ? uint32_t(kSkipNoStage) : skip_reason, &ix->ss);
  *out = ix.release();
  return 0;
}

int tsg_debug_tar_chain(int device, const void* dev_tar, uint64_t n_bytes, uint32_t segment_blocks, uint32_t grid_cap,
                        void* records_out, uint64_t rec_cap, uint64_t* n_records, uint8_t* names_out,
                        uint64_t name_cap, uint64_t* name_bytes, uint64_t* stop_out, uint64_t* candidates_out) {
  using namespace tsg;
  const std::string who = "tsg_debug_tar_chain";
  if (!n_records || !name_bytes || !stop_out || !candidates_out || (n_bytes >= 512 && !dev_tar) ||
      (rec_cap && !records_out) || (name_cap && !names_out) || reinterpret_cast<uintptr_t>(dev_tar) % 16 != 0) {
    SetError(who + ": NULL or misaligned pointer");
    return -2;
  }
  *n_records = *name_bytes = *candidates_out = 0;
  stop_out[0] = stop_out[1] = stop_out[2] = stop_out[3] = 0;
  if (n_bytes < 512) {  // no complete block: END at 0, or a truncated header
    if (n_bytes) {
      stop_out[0] = kTarStopIncomplete;
      stop_out[1] = kTarTruncated;
    }
    return 0;
  }
  TarIndexCtx c;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c.s, hipStreamNonBlocking);
  if (e != hipSuccess) {
    SetError(who + ": " + hipGetErrorString(e));
    return -2;
  }
  TarChainHead head{};
  const tsg_tar_entry_rec* recs = nullptr;
  const uint8_t* names = nullptr;
  tsg_tar_walk_stats ws{};
  const int rc = ChainOnGpu(&c, static_cast<const uint8_t*>(dev_tar), n_bytes, segment_blocks, grid_cap, who, &head, &recs,
                            &names, &ws);
  if (rc < 0) return -2;
  if (rc == 1 && ws.fallback == kTarTooLarge) {
    SetError(who + ": the layer has too many blocks");
    return -2;
  }
  stop_out[0] = head.stop.kind;
  stop_out[1] = head.stop.reason;
  stop_out[2] = head.stop.offset;
  stop_out[3] = head.stop.ext_visited;
  *candidates_out = head.candidates;
  if (rc == 1) return 0;
  *n_records = head.entries;
  *name_bytes = head.name_bytes;
  if (head.entries > rec_cap || head.name_bytes > name_cap) {
    SetError(who + ": the output buffers are too small");
    return -3;
  }
  if (head.entries) std::memcpy(records_out, recs, size_t(head.entries) * sizeof(tsg_tar_entry_rec));
  if (head.name_bytes) std::memcpy(names_out, names, size_t(head.name_bytes));
  return 0;
}

int tsg_debug_tar_walk_last_fallback(const tsg_analyzer* a) { return a ? int(a->tar_fallback_last.load()) : -1; }

int tsg_debug_index_tar_entries(tsg_analyzer* a, const void* records, uint64_t n_records, const uint8_t* names,
                                uint64_t name_bytes, const uint64_t* stop, uint64_t n_bytes, uint64_t candidates_given,
                                tsg_tar_index** out, tsg_device_tar_stats* st) {
  using namespace tsg;
  const char* who = "tsg_debug_index_tar_entries";
  if (out) *out = nullptr;
  if (!a || !out || !stop || (n_records && !records) || (name_bytes && !names)) {
    SetError(std::string(who) + ": NULL argument");
    return -1;
  }
  if (!StatsSizeOk(st, who)) return -1;
  if (stop[0] != kTarStopEnd) {
    SetError(std::string(who) + ": the stop is not END (an INCOMPLETE chain is walked by the host walk)");
    return -1;
  }
  const double t0 = NowMs();
  tsg_tar_stop sp{};
  sp.kind = uint32_t(stop[0]);
  sp.reason = uint32_t(stop[1]);
  sp.offset = stop[2];
  sp.ext_visited = stop[3];
  std::unique_ptr<tsg_tar_index> ix(new tsg_tar_index());
  ix->n_bytes = n_bytes;
  tsg_device_tar_stats tmp{};
  double hm[3] = {0, 0, 0};
  if (EntriesToIndex(a, static_cast<const tsg_tar_entry_rec*>(records), n_records, names, name_bytes, sp, n_bytes,
                     candidates_given, &ix->d, st ? st : &tmp, hm) < 0)
    return -1;
  if (std::getenv("TSG_WALK_DEBUG"))
    std::fprintf(stderr, "tar entries host half: classify %.1f ms, join %.1f ms, Required + index %.1f ms\n", hm[0], hm[1],
                 hm[2]);
  if (st) {
    st->kernel_runs = 0;
    st->ms_kernel = 0;
    st->ms_total = NowMs() - t0;
  }
  ix->ws.walk = 1;
  ix->ws.chain_entries = n_records;
  ix->ws.name_bytes = name_bytes;
  uint32_t skip_reason = 0;
  ix->rs.reason = std::max<uint32_t>(RequiredReason(a, 1, &skip_reason), kReqSetterOff);  // (this hook is the host half)
  SkipStatsInit(a, skip_reason == kSkipRan ? uint32_t(kSkipNoStage) : skip_reason, &ix->ss);
  *out = ix.release();
  return 0;
}

int tsg_debug_tar_batch_plan(const tsg_tar_index* ix, uint32_t first, uint32_t count, const uint8_t* flags,
                             uint64_t* base, uint64_t* offs, uint8_t* kinds, uint8_t* binary) {
  if (!ix || uint64_t(first) + count > ix->d.files.size() || !flags || !base || !offs || !kinds || !binary) {
    tsg::SetError("tsg_debug_tar_batch_plan: NULL argument, or files outside the index");
    return -1;
  }
  tsg::TarBatchPlan p;
  tsg::PlanTarBatch(ix->d, first, count, &p);
  const size_t n = p.path_ptrs.size();
  p.flags.assign(flags, flags + n);
  tsg::TarBatchKinds(&p);
  *base = p.base;
  std::memcpy(offs, p.offs.data(), (n + 1) * 8);
  std::memcpy(kinds, p.kinds.data(), n);
  std::memcpy(binary, p.binary.data(), n);
  return 0;
}

}  // extern "C"
