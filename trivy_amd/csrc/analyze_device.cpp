// Analyze for files whose bytes exist only in HBM (include/tsg_analyzer.h:
// tsg_analyzer_classify_device, tsg_analyzer_submit_device).  What Analyze
// decides per file before Scan (secret.go:103-136) needs the path and the size
// -- the host has both -- and IsBinary over the file's head, which needs the
// bytes: that runs on the GPU over the resident arena (classify.hip) and only
// the flags come back.  A skipped file stays in the arena and is dropped by the
// pre-transform (kind 3, xform.hip).
#include "analyze_device.h"

#include <hip/hip_runtime_api.h>
#include <pthread.h>

#include <atomic>
#include <chrono>
#include <cstring>
#include <memory>
#include <mutex>

#include "capi_internal.h"
#include "classify.h"
#include "collector.h"
#include "parallel.h"
#include "tsg_debug.h"
#include "xform.h"

namespace tsg {
bool RequiredPath(const tsg_analyzer* a, const char* path, uint64_t len, int64_t size);  // analyzer.cpp

// One classify pass's stream, events and buffers.  A pass takes a context from
// the analyzer's pool and gives it back, so passes of several submits in flight
// run side by side, each on its own stream, and none takes the scanner's GPU
// lock: the wait for the read-back holds nothing a scan needs.
struct ClassifyCtx {
  hipStream_t s = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  void* d_flags = nullptr;
  void* d_off = nullptr;
  uint8_t* h_flags = nullptr;  // pinned
  size_t cap_flags = 0, cap_off = 0, cap_h = 0;
  ~ClassifyCtx() {
    if (d_flags) (void)hipFree(d_flags);
    if (d_off) (void)hipFree(d_off);
    if (h_flags) (void)hipHostFree(h_flags);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (s) (void)hipStreamDestroy(s);
  }
};
struct ClassifyPool {
  std::mutex mu;
  std::vector<std::unique_ptr<ClassifyCtx>> free;
};
void FreeClassifyPool(ClassifyPool* p) { delete p; }

namespace {

uint64_t PathLen(const tsg_device_files& f, uint32_t i) {
  return f.path_lens ? f.path_lens[i] : uint64_t(std::strlen(f.paths[i]));
}

// filepath.Ext(path) == ".pyc" (the allowed binaries, secret.go:59-61)
bool IsPyc(const char* p, uint64_t n) {
  for (uint64_t i = n; i-- > 0 && p[i] != '/';)
    if (p[i] == '.') return n - i == 4 && std::memcmp(p + i, ".pyc", 4) == 0;
  return false;
}

bool ImageFile(const tsg_device_files& f) { return !f.dir || !*f.dir; }

std::unique_ptr<ClassifyCtx> TakeCtx(tsg_analyzer* a) {
  {
    std::lock_guard<std::mutex> g(a->classify_mu);
    if (!a->classify) a->classify = new ClassifyPool();
    std::lock_guard<std::mutex> g2(a->classify->mu);
    if (!a->classify->free.empty()) {
      std::unique_ptr<ClassifyCtx> c = std::move(a->classify->free.back());
      a->classify->free.pop_back();
      return c;
    }
  }
  std::unique_ptr<ClassifyCtx> c(new ClassifyCtx());
  if (hipStreamCreateWithFlags(&c->s, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&c->e0) != hipSuccess ||
      hipEventCreate(&c->e1) != hipSuccess)
    return nullptr;
  return c;
}

void GiveCtx(tsg_analyzer* a, std::unique_ptr<ClassifyCtx> c) {
  std::lock_guard<std::mutex> g(a->classify->mu);
  if (a->classify->free.size() < 4) a->classify->free.push_back(std::move(c));  // (else freed here)
}

}  // namespace

// The GPU half: flags[f] = IsBinary over file f's head.  ms_kernel from HIP events.
bool ClassifyOnGpu(tsg_analyzer* a, const tsg_device_files& f, uint8_t* flags, double* ms_kernel, std::string* err) {
  *ms_kernel = 0;
  if (f.n_files == 0) return true;
  const int device = a->s->s->device();
  if (device < 0) {
    *err = "no GPU engine bound to this analyzer's scanner";
    return false;
  }
  hipError_t e = hipSetDevice(device);
  std::unique_ptr<ClassifyCtx> c = e == hipSuccess ? TakeCtx(a) : nullptr;
  if (!c) {
    *err = "classify: stream / events";
    return false;
  }
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  const size_t n = f.n_files, off_bytes = (n + 1) * 8;
  if (c->cap_flags < n) {
    if (c->d_flags) (void)hipFree(c->d_flags);
    c->d_flags = nullptr;
    c->cap_flags = 0;
    if (ok(hipMalloc(&c->d_flags, n + n / 4 + 256))) c->cap_flags = n + n / 4 + 256;
  }
  if (ok(e) && c->cap_h < n) {
    if (c->h_flags) (void)hipHostFree(c->h_flags);
    c->h_flags = nullptr;
    c->cap_h = 0;
    if (ok(hipHostMalloc(reinterpret_cast<void**>(&c->h_flags), n + n / 4 + 256, hipHostMallocDefault)))
      c->cap_h = n + n / 4 + 256;
  }
  const uint64_t* d_off = static_cast<const uint64_t*>(f.dev_offsets);
  if (ok(e) && !d_off) {  // no device copy of the offsets given: upload one for this pass
    if (c->cap_off < off_bytes) {
      if (c->d_off) (void)hipFree(c->d_off);
      c->d_off = nullptr;
      c->cap_off = 0;
      if (ok(hipMalloc(&c->d_off, off_bytes + off_bytes / 4))) c->cap_off = off_bytes + off_bytes / 4;
    }
    if (ok(e)) ok(hipMemcpyAsync(c->d_off, f.host_offsets, off_bytes, hipMemcpyHostToDevice, c->s));
    d_off = static_cast<const uint64_t*>(c->d_off);
  }
  if (ok(e) && ok(hipEventRecord(c->e0, c->s)) &&
      ok(ClassifyHeads(static_cast<const uint8_t*>(f.dev_arena), d_off, f.n_files, static_cast<uint8_t*>(c->d_flags),
                       c->s)) &&
      ok(hipEventRecord(c->e1, c->s)) &&
      ok(hipMemcpyAsync(c->h_flags, c->d_flags, n, hipMemcpyDeviceToHost, c->s)) &&  // through pinned memory
      ok(hipStreamSynchronize(c->s))) {
    std::memcpy(flags, c->h_flags, n);
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->e0, c->e1) == hipSuccess) *ms_kernel = ms;
  }
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(c->s);  // nothing of a failed pass is left queued on a pooled stream
    *err = std::string("classify: ") + hipGetErrorString(e);
    return false;
  }
  GiveCtx(a, std::move(c));
  return true;
}

namespace {

double NowMs() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

bool StatsSizeOk(const tsg_device_classify_stats* st, const char* who) {
  if (!st || st->struct_size == TSG_DEVICE_CLASSIFY_STATS_SIZE_V1) return true;
  SetError(std::string(who) + ": tsg_device_classify_stats.struct_size " + std::to_string(st->struct_size) +
           " is not a size this library knows (v1 = " + std::to_string(TSG_DEVICE_CLASSIFY_STATS_SIZE_V1) + ")");
  return false;
}

// The pending of a device submit: classify (or the flags given), the kinds,
// the scan paths, then the scan itself -- all on the pending's thread.
int Submit(tsg_analyzer* a, const tsg_device_files* f, const uint8_t* given_flags, tsg_pending** out,
           const char* who) {
  if (!out) {
    SetError(std::string(who) + ": NULL out");
    return -1;
  }
  *out = nullptr;
  if (!CheckDeviceFiles(a, f, who)) return -1;
  const tsg_device_files fc = *f;  // the struct is the caller's only for the call; its arrays stay borrowed
  auto plan = std::make_shared<DevicePlan>();
  if (given_flags) plan->flags.assign(given_flags, given_flags + fc.n_files);
  const bool have_flags = given_flags != nullptr;
  std::unique_ptr<tsg_pending> p(new tsg_pending());
  p->owned = plan;
  tsg_pending* pp = p.get();
  DevicePlan* pl = plan.get();
  pp->th = std::thread([a, fc, pl, pp, have_flags] {
    pthread_setname_np(pthread_self(), "tsg-analyze-dev");
    std::string err;
    double ms = 0;
    if (!have_flags) {
      pl->flags.assign(fc.n_files, 0);
      if (!ClassifyOnGpu(a, fc, pl->flags.data(), &ms, &err)) {
        pp->rc = -1;
        pp->err = err;
        return;
      }
    }
    pl->kinds.assign(fc.n_files, 0);
    pl->binary.assign(fc.n_files, 0);
    DeviceKinds(a, fc, pl->flags.data(), pl->kinds.data(), pl->binary.data(), nullptr);
    BuildScanPaths(fc, pl);
    tsg_batch b{};
    b.n_files = fc.n_files;
    b.host_arena = nullptr;  // device-only: the candidate files are fetched from HBM
    b.host_offsets = fc.host_offsets;
    b.dev_arena = fc.dev_arena;
    b.dev_offsets = fc.dev_offsets;
    b.paths = pl->path_ptrs.data();
    b.path_lens = pl->path_lens.data();
    b.binary = pl->binary.data();
    b.transform = pl->kinds.data();
    pp->rc = tsg_scan(const_cast<tsg_scanner*>(a->s), &b, &pp->r);
    if (pp->rc != 0) {
      pp->err = tsg_last_error();
      return;
    }
    // a dropped file's result is types.Secret{} whatever its path (a globally
    // allowed path is why Required dropped it; Analyze never scanned it)
    for (uint32_t i = 0; i < fc.n_files && i < pp->r->files.kind.size(); i++)
      if (pl->kinds[i] == kXformDrop) pp->r->files.kind[i] = 0;
  });
  *out = p.release();
  return 0;
}

}  // namespace

bool CheckDeviceFiles(const tsg_analyzer* a, const tsg_device_files* f, const char* who) {
  const std::string w(who);
  if (!a || !f) {
    SetError(w + ": NULL analyzer or files");
    return false;
  }
  if (f->struct_size != TSG_DEVICE_FILES_SIZE_V1) {
    SetError(w + ": tsg_device_files.struct_size " + std::to_string(f->struct_size) +
             " is not a size this library knows (v1 = " + std::to_string(TSG_DEVICE_FILES_SIZE_V1) + ")");
    return false;
  }
  if (!f->host_offsets) {
    SetError(w + ": host_offsets is required (the host needs the sizes)");
    return false;
  }
  if (!f->dev_arena) {
    SetError(w + ": dev_arena is NULL (the files' bytes, resident in HBM)");
    return false;
  }
  if (!f->paths) {
    SetError(w + ": paths is NULL (Required and the scan need each file's path)");
    return false;
  }
  if (reinterpret_cast<uintptr_t>(f->dev_arena) % 16 != 0) {
    SetError(w + ": dev_arena must be 16-B aligned");
    return false;
  }
  if (f->host_offsets[0] != 0) {
    SetError(w + ": host_offsets must ascend from 0");
    return false;
  }
  for (uint32_t i = 0; i < f->n_files; i++)
    if (f->host_offsets[i + 1] < f->host_offsets[i]) {
      SetError(w + ": host_offsets must ascend from 0 (file " + std::to_string(i) + " ends before it starts)");
      return false;
    }
  return true;
}

void DeviceKinds(const tsg_analyzer* a, const tsg_device_files& f, const uint8_t* flags, uint8_t* kind,
                 uint8_t* binary, tsg_device_classify_stats* st) {
  std::atomic<uint64_t> required{0}, skipped{0}, pyc{0};
  const size_t blocks = (size_t(f.n_files) + 4095) / 4096;
  ParallelFor(blocks, 16, [&](size_t b) {
    uint64_t rq = 0, sk = 0, py = 0;
    const size_t lo = b * 4096, hi = std::min<size_t>(lo + 4096, f.n_files);
    for (size_t i = lo; i < hi; i++) {
      const uint64_t len = f.host_offsets[i + 1] - f.host_offsets[i];
      const uint64_t plen = PathLen(f, uint32_t(i));
      uint8_t k = kXformStripCR, bn = 0;
      if (!RequiredPath(a, f.paths[i], plen, int64_t(len))) {
        k = kXformDrop;
      } else {
        rq++;
        if (flags[i]) {
          if (IsPyc(f.paths[i], plen)) {
            k = kXformPrintable;
            bn = 1;
            py++;
          } else {
            k = kXformDrop;
            sk++;
          }
        }
      }
      kind[i] = k;
      binary[i] = bn;
    }
    required += rq;
    skipped += sk;
    pyc += py;
  });
  if (st) {
    st->files = f.n_files;
    st->required = required.load();
    st->skipped_binary = skipped.load();
    st->pyc = pyc.load();
  }
}

void BuildScanPaths(const tsg_device_files& f, DevicePlan* p) {
  const bool image = ImageFile(f);
  const uint32_t n = f.n_files;
  p->path_off.assign(size_t(n) + 1, 0);
  p->path_lens.resize(n);
  for (uint32_t i = 0; i < n; i++) {
    p->path_lens[i] = PathLen(f, i) + (image ? 1 : 0);
    p->path_off[i + 1] = p->path_off[i] + p->path_lens[i] + 1;  // NUL-terminated: the result's paths are C strings
  }
  p->path_pool.assign(size_t(p->path_off[n]), '\0');
  p->path_ptrs.resize(n);
  for (uint32_t i = 0; i < n; i++) {
    char* d = &p->path_pool[size_t(p->path_off[i])];
    p->path_ptrs[i] = d;
    if (image) *d++ = '/';
    std::memcpy(d, f.paths[i], size_t(PathLen(f, i)));
  }
}

int SubmitDeviceWithFlags(tsg_analyzer* a, const tsg_device_files* f, const uint8_t* flags, tsg_pending** out) {
  if (!flags) {
    SetError("SubmitDeviceWithFlags: NULL flags");
    return -1;
  }
  return Submit(a, f, flags, out, "tsg_analyzer_submit_device");
}

}  // namespace tsg

extern "C" {

int tsg_analyzer_classify_device(tsg_analyzer* a, const tsg_device_files* f, uint8_t* kind_out, uint8_t* binary_out,
                                 tsg_device_classify_stats* st) {
  const char* who = "tsg_analyzer_classify_device";
  if (!tsg::CheckDeviceFiles(a, f, who) || !tsg::StatsSizeOk(st, who)) return -1;
  if (f->n_files && (!kind_out || !binary_out)) {
    tsg::SetError(std::string(who) + ": NULL kind_out or binary_out");
    return -1;
  }
  const double t0 = tsg::NowMs();
  std::vector<uint8_t> flags(f->n_files, 0);
  std::string err;
  double ms_kernel = 0;
  if (!tsg::ClassifyOnGpu(a, *f, flags.data(), &ms_kernel, &err)) {
    tsg::SetError(std::string(who) + ": " + err);
    return -2;
  }
  tsg::DeviceKinds(a, *f, flags.data(), kind_out, binary_out, st);
  if (st) {
    st->ms_kernel = ms_kernel;
    st->ms_total = tsg::NowMs() - t0;
  }
  return 0;
}

int tsg_analyzer_submit_device(tsg_analyzer* a, const tsg_device_files* f, tsg_pending** out) {
  const char* who = "tsg_analyzer_submit_device";
  if (out) *out = nullptr;
  if (!tsg::CheckDeviceFiles(a, f, who)) return -1;
  if (a->s->s->device() < 0) {  // (the classify pass needs the scanner's device)
    tsg::SetError(std::string(who) + ": no GPU engine bound to this analyzer's scanner");
    return -2;
  }
  return tsg::Submit(a, f, nullptr, out, who);
}

}  // extern "C"
