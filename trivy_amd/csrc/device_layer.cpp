// Analyze for a tar layer whose bytes exist only in HBM (include/tsg_analyzer.h:
// tsg_analyzer_index_device_tar, tsg_analyzer_submit_device_tar).  The GPU finds
// the blocks that parse as headers (tarindex.hip); the chain walk over them,
// the plan of a batch whose arena is the layer itself, and the kinds are the
// host half (tar_index_host.h, plain C++); this file is the glue: argument
// checks, the pooled stream and buffers of an index pass, the copies of single
// blocks and ranges the walk asks for, and the pending of a submit.
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
#include "tarindex.h"
#include "tsg_debug.h"
#include "xform.h"

struct tsg_tar_index {
  const uint8_t* dev_tar = nullptr;  // NULL: made from given records (tsg_debug_index_tar_records)
  uint64_t n_bytes = 0;
  tsg::TarIndexData d;
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
  ~TarIndexCtx() {
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

int WalkRecords(tsg_analyzer* a, const IndexedTarSrc& src, uint64_t n_bytes, TarIndexData* d) {
  return WalkTarIndex(
      src, n_bytes, [a](const char* p, uint64_t len, int64_t size) { return RequiredPath(a, p, len, size); }, d,
      [](size_t n, const std::function<void(size_t)>& fn) {
        const size_t blocks = (n + 1023) / 1024;
        ParallelFor(blocks, 16, [&](size_t b) {
          for (size_t i = b * 1024; i < std::min(n, (b + 1) * 1024); i++) fn(i);
        });
      });
}

}  // namespace
}  // namespace tsg

extern "C" {

int tsg_analyzer_index_device_tar(tsg_analyzer* a, const tsg_device_tar* t, tsg_tar_index** out,
                                  tsg_device_tar_stats* st) {
  using namespace tsg;
  const std::string who = "tsg_analyzer_index_device_tar";
  if (out) *out = nullptr;
  if (!a || !t || !out) {
    SetError(who + ": NULL analyzer, tar or out");
    return -1;
  }
  if (t->struct_size != TSG_DEVICE_TAR_SIZE_V1) {
    SetError(who + ": tsg_device_tar.struct_size " + std::to_string(t->struct_size) +
             " is not a size this library knows (v1 = " + std::to_string(TSG_DEVICE_TAR_SIZE_V1) + ")");
    return -1;
  }
  if (!StatsSizeOk(st, who.c_str())) return -1;
  if (!t->dev_tar) {
    SetError(who + ": dev_tar is NULL (the layer's bytes, resident in HBM)");
    return -1;
  }
  if (reinterpret_cast<uintptr_t>(t->dev_tar) % 16 != 0) {
    SetError(who + ": dev_tar must be 16-B aligned");
    return -1;
  }
  if ((t->n_bytes / 512) >> 32) {
    SetError(who + ": a layer of " + std::to_string(t->n_bytes) + " bytes has 2^32 or more 512-B blocks");
    return -1;
  }
  const int device = a->s->s->device();
  if (device < 0) {
    SetError(who + ": no GPU engine bound to this analyzer's scanner");
    return -2;
  }
  const double t0 = NowMs();
  const uint8_t* dev_tar = static_cast<const uint8_t*>(t->dev_tar);
  const uint64_t n_bytes = t->n_bytes;
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
  *out = ix.release();
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
