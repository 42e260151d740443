// C-ABI for host-logic inspection (include/tsg_debug.h).
#include "tsg_debug.h"

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "capi_internal.h"
#include "census.h"
#include "classify.h"
#include "fetch.h"
#include "fetch_host.h"
#include "fetch_windows.h"
#include "filter.h"
#include "goregex.h"
#include "k1_orform.h"
#include "materialize.h"
#include "parallel.h"
#include "pathfilter.h"
#include "xform.h"

namespace tsg {
extern std::atomic<int> g_regex_engine;
thread_local std::string g_last_error;
void SetError(const std::string& e) { g_last_error = e; }
}  // namespace tsg

extern "C" {

const char* tsg_last_error(void) { return tsg::g_last_error.c_str(); }

int tsg_regex_find_all(const char* pattern, const uint8_t* text, uint64_t n, int submatch,
                       const int64_t* windows, uint32_t n_windows, int64_t* out, uint64_t out_cap,
                       uint64_t* out_len, int32_t* num_cap) {
  std::string err;
  auto re = tsg::Regex::Compile(pattern, &err);
  if (!re) {
    tsg::SetError(err);
    return -1;
  }
  std::vector<tsg::Window> wins;
  for (uint32_t i = 0; i < n_windows; i++) wins.push_back({windows[2 * i], windows[2 * i + 1]});
  std::vector<int64_t> res;
  re->FindAll(text, int64_t(n), submatch != 0, windows ? &wins : nullptr, &res);
  *out_len = res.size();
  *num_cap = re->num_cap();
  if (!res.empty()) std::memcpy(out, res.data(), sizeof(int64_t) * (res.size() < out_cap ? res.size() : out_cap));
  return 0;
}

void tsg_debug_regex_engine(int mode) { tsg::g_regex_engine.store(mode); }

int tsg_debug_xform(int device, const uint8_t* raw, uint64_t n_bytes, const uint64_t* offsets, uint32_t n_files,
                    const uint8_t* kinds, uint8_t* out, uint64_t out_cap, uint64_t* xoff) {
  if (offsets[0] != 0 || offsets[n_files] != n_bytes) {
    tsg::SetError("offsets must run from 0 to n_bytes");
    return -2;
  }
  void *d_raw = nullptr, *d_off = nullptr, *d_kind = nullptr, *d_xoff = nullptr, *d_out = nullptr, *d_sc = nullptr;
  hipStream_t s = nullptr;
  hipError_t e = hipSetDevice(device);
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  const size_t sc_bytes = tsg::XformScratchBytes(n_bytes, n_files);
  if (ok(e) && ok(hipStreamCreate(&s)) && ok(hipMalloc(&d_raw, n_bytes + 64)) &&
      ok(hipMalloc(&d_off, (size_t(n_files) + 1) * 8)) && ok(hipMalloc(&d_kind, size_t(n_files) + 1)) &&
      ok(hipMalloc(&d_xoff, (size_t(n_files) + 1) * 8)) && ok(hipMalloc(&d_sc, sc_bytes)) &&
      ok(hipMemset(d_raw, 0, n_bytes + 64)) && ok(hipMemcpy(d_raw, raw, n_bytes, hipMemcpyHostToDevice)) &&
      ok(hipMemcpy(d_off, offsets, (size_t(n_files) + 1) * 8, hipMemcpyHostToDevice)) &&
      ok(hipMemcpy(d_kind, kinds, n_files, hipMemcpyHostToDevice)) && tsg::XformOnePassOn()) {
    const uint64_t cap = tsg::XformMaxOut(n_bytes, n_files) + 64;  // (the engine's bound)
    if (ok(hipMalloc(&d_out, cap)) &&
        ok(tsg::XformOnePass(static_cast<const uint8_t*>(d_raw), n_bytes, static_cast<const uint64_t*>(d_off),
                             static_cast<const uint8_t*>(d_kind), n_files, d_sc, static_cast<uint64_t*>(d_xoff),
                             static_cast<uint8_t*>(d_out), cap, s)) &&
        ok(hipMemcpyAsync(xoff, d_xoff, (size_t(n_files) + 1) * 8, hipMemcpyDeviceToHost, s)) &&
        ok(hipStreamSynchronize(s)) &&
        ok(tsg::XformErrorWord(n_bytes, n_files, d_sc, s) == 0 ? hipSuccess : hipErrorIllegalAddress))
      ok(hipMemcpy(out, d_out, std::min<uint64_t>(out_cap, xoff[n_files]), hipMemcpyDeviceToHost));
  } else if (ok(e) &&
      ok(tsg::XformPlan(static_cast<const uint8_t*>(d_raw), n_bytes, static_cast<const uint64_t*>(d_off),
                        static_cast<const uint8_t*>(d_kind), n_files, d_sc, static_cast<uint64_t*>(d_xoff), s)) &&
      ok(hipMemcpyAsync(xoff, d_xoff, (size_t(n_files) + 1) * 8, hipMemcpyDeviceToHost, s)) &&
      ok(hipStreamSynchronize(s)) && ok(hipMalloc(&d_out, xoff[n_files] + 64)) &&
      ok(tsg::XformWrite(static_cast<const uint8_t*>(d_raw), n_bytes, static_cast<const uint64_t*>(d_off),
                         static_cast<const uint8_t*>(d_kind), n_files, d_sc, static_cast<uint8_t*>(d_out),
                         xoff[n_files] + 64, s)) &&
      ok(hipStreamSynchronize(s)) &&
      ok(tsg::XformErrorWord(n_bytes, n_files, d_sc, s) == 0 ? hipSuccess : hipErrorIllegalAddress))
    ok(hipMemcpy(out, d_out, std::min<uint64_t>(out_cap, xoff[n_files]), hipMemcpyDeviceToHost));
  for (void* p : {d_raw, d_off, d_kind, d_xoff, d_out, d_sc})
    if (p) (void)hipFree(p);
  if (s) (void)hipStreamDestroy(s);
  if (e != hipSuccess) {
    tsg::SetError(std::string("tsg_debug_xform: ") + hipGetErrorString(e));
    return -1;
  }
  return 0;
}

int tsg_debug_classify(int device, const uint8_t* raw, uint64_t n_bytes, const uint64_t* offsets, uint32_t n_files,
                       uint8_t* flags) {
  if (!offsets || offsets[0] != 0 || offsets[n_files] != n_bytes) {
    tsg::SetError("offsets must run from 0 to n_bytes");
    return -2;
  }
  for (uint32_t f = 0; f < n_files; f++)
    if (offsets[f + 1] < offsets[f]) {
      tsg::SetError("offsets must ascend");
      return -2;
    }
  void *d_raw = nullptr, *d_off = nullptr, *d_flags = nullptr;
  hipStream_t s = nullptr;
  hipError_t e = hipSetDevice(device);
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  if (ok(e) && ok(hipStreamCreate(&s)) && ok(hipMalloc(&d_raw, n_bytes + 64)) &&
      ok(hipMalloc(&d_off, (size_t(n_files) + 1) * 8)) && ok(hipMalloc(&d_flags, size_t(n_files) + 1)) &&
      ok(hipMemset(d_raw, 0, n_bytes + 64)) && ok(hipMemcpy(d_raw, raw, n_bytes, hipMemcpyHostToDevice)) &&
      ok(hipMemcpy(d_off, offsets, (size_t(n_files) + 1) * 8, hipMemcpyHostToDevice)) &&
      ok(hipMemset(d_flags, 0xEE, size_t(n_files) + 1)) &&  // (a flag the kernel leaves unwritten shows up)
      ok(tsg::ClassifyHeads(static_cast<const uint8_t*>(d_raw), static_cast<const uint64_t*>(d_off), n_files,
                            static_cast<uint8_t*>(d_flags), s)) &&
      ok(hipStreamSynchronize(s)))
    ok(hipMemcpy(flags, d_flags, n_files, hipMemcpyDeviceToHost));
  for (void* p : {d_raw, d_off, d_flags})
    if (p) (void)hipFree(p);
  if (s) (void)hipStreamDestroy(s);
  if (e != hipSuccess) {
    tsg::SetError(std::string("tsg_debug_classify: ") + hipGetErrorString(e));
    return -1;
  }
  return 0;
}

int tsg_debug_transform_census(int device, const uint8_t* raw, uint64_t n_bytes, const uint64_t* offsets,
                                uint32_t n_files, const uint8_t* kinds, uint8_t* mark_out) {
  if (!offsets || offsets[0] != 0 || offsets[n_files] != n_bytes) {
    tsg::SetError("offsets must run from 0 to n_bytes");
    return -2;
  }
  for (uint32_t f = 0; f < n_files; f++)
    if (offsets[f + 1] < offsets[f]) {
      tsg::SetError("offsets must ascend");
      return -2;
    }
  void *d_raw = nullptr, *d_off = nullptr, *d_kind = nullptr, *d_mark = nullptr;
  hipStream_t s = nullptr;
  hipError_t e = hipSetDevice(device);
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  if (ok(e) && ok(hipStreamCreate(&s)) && ok(hipMalloc(&d_raw, n_bytes + 64)) &&
      ok(hipMalloc(&d_off, (size_t(n_files) + 1) * 8)) && ok(hipMalloc(&d_kind, size_t(n_files) + 1)) &&
      ok(hipMalloc(&d_mark, size_t(n_files) + 1)) &&
      ok(hipMemcpy(d_raw, raw, n_bytes + 64, hipMemcpyHostToDevice)) &&  // (the caller's tail with it)
      ok(hipMemcpy(d_off, offsets, (size_t(n_files) + 1) * 8, hipMemcpyHostToDevice)) &&
      ok(hipMemcpy(d_kind, kinds, n_files, hipMemcpyHostToDevice)) &&
      ok(hipMemset(d_mark, 0xEE, size_t(n_files) + 1)) &&  // (a mark the kernels leave unwritten shows up)
      ok(tsg::TransformCensus(static_cast<const uint8_t*>(d_raw), n_bytes, static_cast<const uint64_t*>(d_off),
                              static_cast<const uint8_t*>(d_kind), n_files, static_cast<uint8_t*>(d_mark), s)) &&
      ok(hipStreamSynchronize(s)))
    ok(hipMemcpy(mark_out, d_mark, n_files, hipMemcpyDeviceToHost));
  for (void* p : {d_raw, d_off, d_kind, d_mark})
    if (p) (void)hipFree(p);
  if (s) (void)hipStreamDestroy(s);
  if (e != hipSuccess) {
    tsg::SetError(std::string("tsg_debug_transform_census: ") + hipGetErrorString(e));
    return -1;
  }
  return 0;
}

int tsg_debug_gather_device(int device, const uint8_t* raw, uint64_t n_bytes, const uint64_t* src_off,
                            const uint64_t* dst_off, uint32_t n_files, uint8_t* out) {
  if (!src_off || !dst_off) {
    tsg::SetError("tsg_debug_gather_device: offsets missing");
    return -2;
  }
  std::vector<tsg::GatherItem> items;
  for (uint32_t f = 0; f < n_files; f++) {
    if (dst_off[f + 1] < dst_off[f]) {
      tsg::SetError("tsg_debug_gather_device: destination offsets must ascend");
      return -2;
    }
    const uint64_t len = dst_off[f + 1] - dst_off[f];
    if (src_off[f] > n_bytes || len > n_bytes - src_off[f]) {
      tsg::SetError("tsg_debug_gather_device: a file leaves the arena");
      return -2;
    }
    for (uint32_t q = 0; uint64_t(q) * tsg::kGatherPiece < len; q++) items.push_back(tsg::GatherItem{f, q});
  }
  const uint64_t out_bytes = dst_off[n_files] + 64;
  const size_t item_bytes = items.size() * sizeof(tsg::GatherItem);
  void *d_raw = nullptr, *d_src = nullptr, *d_dst = nullptr, *d_items = nullptr, *d_out = nullptr;
  hipStream_t s = nullptr;
  hipError_t e = hipSetDevice(device);
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  if (ok(e) && ok(hipStreamCreate(&s)) && ok(hipMalloc(&d_raw, n_bytes + 64)) &&
      ok(hipMalloc(&d_src, (size_t(n_files) + 1) * 8)) && ok(hipMalloc(&d_dst, (size_t(n_files) + 1) * 8)) &&
      ok(hipMalloc(&d_items, item_bytes + 8)) && ok(hipMalloc(&d_out, out_bytes)) &&
      ok(hipMemcpy(d_raw, raw, n_bytes + 64, hipMemcpyHostToDevice)) &&
      ok(hipMemcpy(d_src, src_off, size_t(n_files) * 8, hipMemcpyHostToDevice)) &&
      ok(hipMemcpy(d_dst, dst_off, (size_t(n_files) + 1) * 8, hipMemcpyHostToDevice)) &&
      (items.empty() || ok(hipMemcpy(d_items, items.data(), item_bytes, hipMemcpyHostToDevice))) &&
      ok(hipMemcpy(d_out, out, out_bytes, hipMemcpyHostToDevice)) &&  // (what no file owns comes back as it was)
      ok(tsg::GatherDeviceFiles(static_cast<const uint8_t*>(d_raw), static_cast<const uint64_t*>(d_src),
                                static_cast<const uint64_t*>(d_dst), static_cast<const tsg::GatherItem*>(d_items),
                                uint32_t(items.size()), static_cast<uint8_t*>(d_out), s)) &&
      ok(hipStreamSynchronize(s)))
    ok(hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost));
  for (void* p : {d_raw, d_src, d_dst, d_items, d_out})
    if (p) (void)hipFree(p);
  if (s) (void)hipStreamDestroy(s);
  if (e != hipSuccess) {
    tsg::SetError(std::string("tsg_debug_gather_device: ") + hipGetErrorString(e));
    return -1;
  }
  return 0;
}

// The destinations [dst_off[i], dst_off[i] + len(i)) lie inside dst_bytes and no two of them share a byte.
static bool GatherDstOk(const char* who, const uint64_t* dst_off, const std::vector<uint64_t>& len,
                        uint64_t dst_bytes) {
  std::vector<std::pair<uint64_t, uint64_t>> span;
  for (size_t i = 0; i < len.size(); i++) {
    if (dst_off[i] > dst_bytes || len[i] > dst_bytes - dst_off[i]) {
      tsg::SetError(std::string(who) + ": a destination leaves the output");
      return false;
    }
    if (len[i]) span.emplace_back(dst_off[i], dst_off[i] + len[i]);
  }
  std::sort(span.begin(), span.end());
  for (size_t i = 1; i < span.size(); i++)
    if (span[i].first < span[i - 1].second) {
      tsg::SetError(std::string(who) + ": two destinations overlap");
      return false;
    }
  return true;
}

int tsg_debug_gather_files(int device, const uint8_t* src, uint64_t n_bytes, const uint64_t* xoff, uint32_t n_files,
                           const uint32_t* files, const uint64_t* dst_off, uint32_t n, uint8_t* out,
                           uint64_t dst_bytes) {
  const char* who = "tsg_debug_gather_files";
  if (!src || !xoff || !out || (n && (!files || !dst_off))) {
    tsg::SetError(std::string(who) + ": NULL argument");
    return -2;
  }
  for (uint32_t f = 0; f < n_files; f++)
    if (xoff[f + 1] < xoff[f]) {
      tsg::SetError(std::string(who) + ": offsets must ascend");
      return -2;
    }
  if (xoff[n_files] > n_bytes) {
    tsg::SetError(std::string(who) + ": a file leaves the arena");
    return -2;
  }
  std::vector<uint64_t> len(n);
  for (uint32_t i = 0; i < n; i++) {
    if (files[i] >= n_files) {
      tsg::SetError(std::string(who) + ": no such file");
      return -2;
    }
    len[i] = xoff[files[i] + 1] - xoff[files[i]];
  }
  if (!GatherDstOk(who, dst_off, len, dst_bytes)) return -2;
  void *d_src = nullptr, *d_xoff = nullptr, *d_files = nullptr, *d_dst = nullptr, *d_out = nullptr;
  hipStream_t s = nullptr;
  hipError_t e = hipSetDevice(device);
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  if (ok(e) && ok(hipStreamCreate(&s)) && ok(hipMalloc(&d_src, n_bytes + 64)) &&
      ok(hipMalloc(&d_xoff, (size_t(n_files) + 1) * 8)) && ok(hipMalloc(&d_files, (size_t(n) + 1) * 4)) &&
      ok(hipMalloc(&d_dst, (size_t(n) + 1) * 8)) && ok(hipMalloc(&d_out, dst_bytes + 64)) &&
      ok(hipMemcpy(d_src, src, n_bytes + 64, hipMemcpyHostToDevice)) &&  // (the caller's tail with it)
      ok(hipMemcpy(d_xoff, xoff, (size_t(n_files) + 1) * 8, hipMemcpyHostToDevice)) &&
      (n == 0 || (ok(hipMemcpy(d_files, files, size_t(n) * 4, hipMemcpyHostToDevice)) &&
                  ok(hipMemcpy(d_dst, dst_off, size_t(n) * 8, hipMemcpyHostToDevice)))) &&
      ok(hipMemcpy(d_out, out, dst_bytes + 64, hipMemcpyHostToDevice)) &&  // (what no file owns comes back as it was)
      ok(tsg::GatherFiles(static_cast<const uint8_t*>(d_src), static_cast<const uint64_t*>(d_xoff),
                          static_cast<const uint32_t*>(d_files), static_cast<const uint64_t*>(d_dst), n,
                          static_cast<uint8_t*>(d_out), s)) &&
      ok(hipStreamSynchronize(s)))
    ok(hipMemcpy(out, d_out, dst_bytes + 64, hipMemcpyDeviceToHost));
  for (void* p : {d_src, d_xoff, d_files, d_dst, d_out})
    if (p) (void)hipFree(p);
  if (s) (void)hipStreamDestroy(s);
  if (e != hipSuccess) {
    tsg::SetError(std::string(who) + ": " + hipGetErrorString(e));
    return -1;
  }
  return 0;
}

// gather_host_kernel's read contract (xform.hip), per item [d0, d1) of a file whose byte d0 has the
// source s0: with b_lo = d0 & ~15 the first destination block's source is b_lo + s0 - d0 = s0 - (d0 & 15)
// >= s0 - 15, and a_lo is that rounded down to 16, so a_lo >= s0 - 15 - 15: up to 30 bytes before the
// item (before the file, for its first item).  A lane loads block j at a_lo + 16 j while b_lo + 16 j <
// d1 + 16, i.e. b_lo + 16 j <= d1 + 15 -- lane 63's extra load obeys the same bound -- and a_lo <= b_lo +
// s0 - d0, so the load ends at a_lo + 16 j + 16 <= (d1 + s0 - d0) + 15 + 16: up to 31 bytes past the
// item's last source byte (past the file, for its last item).  The hook asks for 32 on either side.
int tsg_debug_gather_host(int device, const uint8_t* src, uint64_t n_bytes, const uint64_t* src_off,
                          const uint64_t* len, const uint64_t* dst_off, uint32_t n_files, uint8_t* out,
                          uint64_t dst_bytes) {
  const char* who = "tsg_debug_gather_host";
  if (!out || (n_bytes && !src) || (n_files && (!src_off || !len || !dst_off)) || n_files > 0x7FFFFFFFu) {
    tsg::SetError(std::string(who) + ": NULL argument");
    return -2;
  }
  // The kernel takes a file's end from the next file's start.  Here a file is entry 2 i of the offsets
  // and entry 2 i + 1 (a file without items) holds its end, so the destinations need not be contiguous.
  std::vector<uint64_t> so(2 * size_t(n_files) + 1, 0), dofs(2 * size_t(n_files) + 1, 0);
  std::vector<tsg::GatherItem> items;
  for (uint32_t f = 0; f < n_files; f++) {
    if (src_off[f] < 32 || src_off[f] > n_bytes || len[f] > n_bytes - src_off[f] ||
        n_bytes - src_off[f] - len[f] < 32) {
      tsg::SetError(std::string(who) + ": file " + std::to_string(f) +
                    " lacks the 32 readable bytes before or after it");
      return -2;
    }
    so[2 * size_t(f)] = src_off[f];
    dofs[2 * size_t(f)] = dst_off[f];
    dofs[2 * size_t(f) + 1] = dst_off[f] + len[f];
    for (uint32_t q = 0; uint64_t(q) * tsg::kGatherPiece < len[f]; q++) items.push_back(tsg::GatherItem{2 * f, q});
  }
  if (!GatherDstOk(who, dst_off, std::vector<uint64_t>(len, len + n_files), dst_bytes)) return -2;
  const size_t item_bytes = items.size() * sizeof(tsg::GatherItem);
  void *h_src = nullptr, *d_view = nullptr, *d_so = nullptr, *d_dofs = nullptr, *d_items = nullptr, *d_out = nullptr;
  hipStream_t s = nullptr;
  hipError_t e = hipSetDevice(device);
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  // the source as production has it: page-locked host memory mapped into the device's address space
  if (ok(e) && ok(hipStreamCreate(&s)) &&
      ok(hipHostMalloc(&h_src, std::max<uint64_t>(n_bytes, 1), hipHostMallocMapped)) &&
      ok(hipHostGetDevicePointer(&d_view, h_src, 0)) && ok(hipMalloc(&d_so, so.size() * 8)) &&
      ok(hipMalloc(&d_dofs, dofs.size() * 8)) && ok(hipMalloc(&d_items, item_bytes + 8)) &&
      ok(hipMalloc(&d_out, dst_bytes + 64))) {
    if (n_bytes) std::memcpy(h_src, src, n_bytes);
    if (ok(hipMemcpy(d_so, so.data(), so.size() * 8, hipMemcpyHostToDevice)) &&
        ok(hipMemcpy(d_dofs, dofs.data(), dofs.size() * 8, hipMemcpyHostToDevice)) &&
        (items.empty() || ok(hipMemcpy(d_items, items.data(), item_bytes, hipMemcpyHostToDevice))) &&
        ok(hipMemcpy(d_out, out, dst_bytes + 64, hipMemcpyHostToDevice)) &&  // (what no file owns comes back as it was)
        ok(tsg::GatherHostFiles(static_cast<const uint8_t*>(d_view), static_cast<const uint64_t*>(d_so),
                                static_cast<const uint64_t*>(d_dofs), static_cast<const tsg::GatherItem*>(d_items),
                                uint32_t(items.size()), static_cast<uint8_t*>(d_out), s)) &&
        ok(hipStreamSynchronize(s)))
      ok(hipMemcpy(out, d_out, dst_bytes + 64, hipMemcpyDeviceToHost));
  }
  for (void* p : {d_so, d_dofs, d_items, d_out})
    if (p) (void)hipFree(p);
  if (h_src) (void)hipHostFree(h_src);
  if (s) (void)hipStreamDestroy(s);
  if (e != hipSuccess) {
    tsg::SetError(std::string(who) + ": " + hipGetErrorString(e));
    return -1;
  }
  return 0;
}

// FetchPlan and the FetchPack rounds of GpuEngine::IssueFetch on one stream, each round waited for and
// read back whole: the staging buffer has 64 bytes more than a round may fill, and what a round leaves of
// the 0xA5 it was filled with shows where the kernel stored.
int tsg_debug_fetch_files_device(int device, const uint8_t* arena, uint64_t n_bytes, const uint64_t* offsets,
                                 uint32_t n_files, const void* cands, uint64_t n_cands, uint32_t cand_cap,
                                 const uint32_t* flags, uint64_t direct_bytes, uint64_t stage_bytes,
                                 uint64_t copy_bytes, uint8_t* packed_out, uint64_t packed_cap, uint32_t* list_out,
                                 uint64_t* lpoff_out, uint64_t counters[6]) {
  const char* who = "tsg_debug_fetch_files_device";
  auto refuse = [&](const char* why) {
    tsg::SetError(std::string(who) + ": " + why);
    return -2;
  };
  if (!offsets || !packed_out || !list_out || !lpoff_out || !counters || (n_bytes && !arena))
    return refuse("NULL argument");
  if (offsets[0] != 0) return refuse("offsets must start at 0");
  for (uint32_t f = 0; f < n_files; f++)
    if (offsets[f + 1] < offsets[f]) return refuse("offsets must ascend");
  if (offsets[n_files] != n_bytes) return refuse("offsets must end at n_bytes");
  if (flags && (cands || n_cands)) return refuse("candidate records or file flags, not both");
  if (n_cands > 0xFFFFFFFFull) return refuse("more candidates than the device count holds");
  const size_t held = size_t(std::min<uint64_t>(n_cands, cand_cap));
  if (!flags && held && !cands) return refuse("candidate records missing");
  if (copy_bytes % 16) return refuse("copy_bytes must be a multiple of 16");
  stage_bytes = std::max<uint64_t>(stage_bytes / tsg::kFetchSeg, 1) * tsg::kFetchSeg;
  const uint32_t count = uint32_t(n_cands);
  const size_t stage_alloc = size_t(stage_bytes) + 64;
  void *d_arena = nullptr, *d_off = nullptr, *d_cands = nullptr, *d_count = nullptr, *d_sc = nullptr, *d_ctr = nullptr,
       *d_stage = nullptr;
  hipStream_t s = nullptr;
  int rc = 0;
  hipError_t e = hipSetDevice(device);
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  tsg::FetchCounters ctr = {};
  // the arena as the library's callers give it: n_bytes + 64 readable bytes and no more (0xEE: not file bytes)
  if (ok(e) && ok(hipStreamCreate(&s)) && ok(hipMalloc(&d_arena, n_bytes + 64)) &&
      ok(hipMalloc(&d_off, (size_t(n_files) + 1) * 8)) && ok(hipMalloc(&d_cands, (held + 1) * sizeof(tsg::Candidate))) &&
      ok(hipMalloc(&d_count, 4)) && ok(hipMalloc(&d_sc, tsg::FetchScratchBytes(n_files))) &&
      ok(hipMalloc(&d_ctr, sizeof ctr)) && ok(hipMalloc(&d_stage, stage_alloc)) &&
      ok(hipMemset(d_arena, 0xEE, n_bytes + 64)) &&
      (n_bytes == 0 || ok(hipMemcpy(d_arena, arena, n_bytes, hipMemcpyHostToDevice))) &&
      ok(hipMemcpy(d_off, offsets, (size_t(n_files) + 1) * 8, hipMemcpyHostToDevice)) &&
      (held == 0 || ok(hipMemcpy(d_cands, cands, held * sizeof(tsg::Candidate), hipMemcpyHostToDevice))) &&
      ok(hipMemcpy(d_count, &count, 4, hipMemcpyHostToDevice)) &&
      (!flags || n_files == 0 ||
       ok(hipMemcpy(tsg::FetchFlags(d_sc, n_files), flags, size_t(n_files) * 4, hipMemcpyHostToDevice))) &&
      ok(tsg::FetchPlan(flags ? nullptr : static_cast<const tsg::Candidate*>(d_cands),
                        static_cast<const uint32_t*>(d_count), cand_cap, static_cast<const uint64_t*>(d_off), n_files,
                        direct_bytes, d_sc, static_cast<tsg::FetchCounters*>(d_ctr), s)) &&
      ok(hipMemcpyAsync(&ctr, d_ctr, sizeof ctr, hipMemcpyDeviceToHost, s)) && ok(hipStreamSynchronize(s))) {
    const uint64_t copy = copy_bytes ? copy_bytes : ctr.packed_bytes;
    uint64_t rounds = 0;
    if (ctr.n_packed > n_files || copy > packed_cap) {
      tsg::SetError(std::string(who) + (copy > packed_cap ? ": packed_cap is below the bytes to copy"
                                                          : ": the plan packs more files than there are"));
      rc = -3;
    }
    std::vector<uint8_t> round(rc == 0 ? stage_alloc : 0);
    for (uint64_t w0 = 0; rc == 0 && w0 < copy && e == hipSuccess; w0 += stage_bytes, rounds++) {
      const uint64_t w1 = std::min(w0 + stage_bytes, copy);
      if (!(ok(hipMemsetAsync(d_stage, 0xA5, stage_alloc, s)) &&
            ok(tsg::FetchPack(static_cast<const uint8_t*>(d_arena), static_cast<const uint64_t*>(d_off), n_files, d_sc,
                              static_cast<const tsg::FetchCounters*>(d_ctr), w0, w1, static_cast<uint8_t*>(d_stage),
                              s)) &&
            ok(hipStreamSynchronize(s)) && ok(hipMemcpy(round.data(), d_stage, stage_alloc, hipMemcpyDeviceToHost))))
        break;
      std::memcpy(packed_out + w0, round.data(), size_t(w1 - w0));
      for (size_t i = size_t(w1 - w0); i < stage_alloc; i++)
        if (round[i] != 0xA5) {  // a store past the round's bytes
          tsg::SetError(std::string(who) + ": round " + std::to_string(rounds) + " wrote staging byte " +
                        std::to_string(i) + ", past its " + std::to_string(w1 - w0));
          rc = -4;
          break;
        }
    }
    if (rc == 0 && e == hipSuccess && ctr.n_packed)
      ok(hipMemcpy(list_out, tsg::FetchList(d_sc, n_files), size_t(ctr.n_packed) * 4, hipMemcpyDeviceToHost));
    if (rc == 0 && e == hipSuccess)
      ok(hipMemcpy(lpoff_out, tsg::FetchListOffsets(d_sc, n_files), (size_t(ctr.n_packed) + 1) * 8,
                   hipMemcpyDeviceToHost));
    counters[0] = ctr.packed_bytes;
    counters[1] = ctr.n_packed;
    counters[2] = ctr.n_direct;
    counters[3] = ctr.n_files;
    counters[4] = ctr.file_bytes;
    counters[5] = rounds;
  }
  for (void* p : {d_arena, d_off, d_cands, d_count, d_sc, d_ctr, d_stage})
    if (p) (void)hipFree(p);
  if (s) (void)hipStreamDestroy(s);
  if (e != hipSuccess) {
    tsg::SetError(std::string(who) + ": " + hipGetErrorString(e));
    return -1;
  }
  return rc;
}

int tsg_regex_match(const char* pattern, const uint8_t* text, uint64_t n) {
  std::string err;
  auto re = tsg::Regex::Compile(pattern, &err);
  if (!re) {
    tsg::SetError(err);
    return -1;
  }
  return re->Match(text, int64_t(n)) ? 1 : 0;
}

int64_t tsg_go_bytes_to_lower(const uint8_t* s, uint64_t n, uint8_t* out, uint64_t out_cap) {
  std::string l = tsg::GoBytesToLower(s, n);
  std::memcpy(out, l.data(), l.size() < out_cap ? l.size() : out_cap);
  return int64_t(l.size());
}

int tsg_regex_find_all_bounded(const char* pattern, const uint8_t* text, uint64_t true_len, uint64_t lo, uint64_t hi,
                               int submatch, const int64_t* windows, uint32_t n_windows, int64_t* out,
                               uint64_t out_cap, uint64_t* out_len, int32_t* num_cap, int32_t* hit_limit) {
  if (lo > hi || hi > true_len) {
    tsg::SetError("tsg_regex_find_all_bounded: need lo <= hi <= true_len");
    return -2;
  }
  std::string err;
  auto re = tsg::Regex::Compile(pattern, &err);
  if (!re) {
    tsg::SetError(err);
    return -1;
  }
  std::vector<tsg::Window> wins;
  for (uint32_t i = 0; i < n_windows; i++) wins.push_back({windows[2 * i], windows[2 * i + 1]});
  // the engine gets the piece alone, in a block of exactly its size
  std::unique_ptr<uint8_t[]> piece(new uint8_t[size_t(hi - lo)]);
  if (hi > lo) std::memcpy(piece.get(), text + lo, size_t(hi - lo));
  std::vector<int64_t> res;
  bool hit = false;
  re->FindAllBounded(piece.get(), int64_t(lo), int64_t(hi), int64_t(true_len), submatch != 0,
                     windows ? &wins : nullptr, &res, &hit);
  *out_len = res.size();
  *num_cap = re->num_cap();
  *hit_limit = hit ? 1 : 0;
  if (!res.empty()) std::memcpy(out, res.data(), sizeof(int64_t) * (res.size() < out_cap ? res.size() : out_cap));
  return 0;
}

static tsg::FetchWinParams WinParamsOf(const uint32_t* opts) {
  tsg::FetchWinParams p;
  if (opts) {
    if (opts[0]) p.back = opts[0];
    if (opts[1]) p.fwd_bytes = opts[1];
    if (opts[2]) p.fwd_cap = opts[2];
    if (opts[3]) p.max_span = opts[3];
  }
  return p;
}

static bool WinArgsOk(const char* who, const uint64_t* offsets, uint32_t n_files, const uint32_t* opts) {
  if (!offsets || offsets[0] != 0) {
    tsg::SetError(std::string(who) + ": offsets must start at 0");
    return false;
  }
  for (uint32_t f = 0; f < n_files; f++)
    if (offsets[f + 1] < offsets[f]) {
      tsg::SetError(std::string(who) + ": offsets must ascend");
      return false;
    }
  if (opts && opts[0] && opts[0] < tsg::kFetchBackMin) {
    tsg::SetError(std::string(who) + ": back_bytes below 4 (the engine looks back one rune)");
    return false;
  }
  return true;
}

int tsg_debug_fetch_windows_plan(const uint64_t* offsets, uint32_t n_files, const void* cands, uint64_t n_cands,
                                 const uint32_t* rule_max_len, uint32_t n_rules, const uint32_t* opts, uint64_t* runs,
                                 uint64_t runs_cap, uint64_t* n_runs, uint64_t* views, uint64_t views_cap,
                                 uint64_t* n_views, uint64_t totals[4]) {
  if (!WinArgsOk("tsg_debug_fetch_windows_plan", offsets, n_files, opts)) return -2;
  tsg::HostWindowPlan P;
  tsg::PlanWindowsOnHost(static_cast<const tsg::Candidate*>(cands), size_t(n_cands), offsets, n_files, rule_max_len,
                         n_rules, WinParamsOf(opts), &P);
  *n_runs = P.runs.size();
  for (size_t k = 0; k < P.runs.size() && k < runs_cap; k++) {
    runs[3 * k] = P.runs[k].g0;
    runs[3 * k + 1] = P.runs[k].g1;
    runs[3 * k + 2] = P.runs[k].packed;
  }
  uint64_t nv = 0;
  size_t from = 0;
  std::vector<tsg::FilePiece> v;
  for (uint32_t f = 0; f < n_files; f++) {
    v.clear();
    from = tsg::FileViewOf(P, offsets[f], offsets[f + 1], from, &v);
    for (const tsg::FilePiece& p : v) {
      if (nv < views_cap) {
        views[4 * nv] = f;
        views[4 * nv + 1] = p.lo;
        views[4 * nv + 2] = p.hi;
        views[4 * nv + 3] = p.packed;
      }
      nv++;
    }
  }
  *n_views = nv;
  totals[0] = P.granules;
  totals[1] = P.runs.size();
  totals[2] = P.whole_files;
  totals[3] = P.packed_bytes();
  return 0;
}

int tsg_debug_fetch_windows_device(int device, const uint8_t* arena, uint64_t n_bytes, const uint64_t* offsets,
                                   uint32_t n_files, const void* cands, uint64_t n_cands, uint32_t cand_cap,
                                   const uint32_t* rule_max_len, uint32_t n_rules, const uint32_t* opts,
                                   uint64_t stage_bytes, uint8_t* packed, uint64_t packed_cap, uint64_t counters[4]) {
  if (!WinArgsOk("tsg_debug_fetch_windows_device", offsets, n_files, opts)) return -2;
  if (offsets[n_files] != n_bytes || n_cands > 0xFFFFFFFFull) {
    tsg::SetError("tsg_debug_fetch_windows_device: offsets must end at n_bytes");
    return -2;
  }
  stage_bytes = std::max<uint64_t>(stage_bytes / tsg::kFetchGranule, 1) * tsg::kFetchGranule;
  const uint32_t count = uint32_t(n_cands);
  const size_t held = size_t(std::min<uint64_t>(n_cands, cand_cap));
  void *d_arena = nullptr, *d_off = nullptr, *d_cands = nullptr, *d_count = nullptr, *d_ml = nullptr, *d_sc = nullptr,
       *d_ctr = nullptr, *d_stage = nullptr;
  hipStream_t s = nullptr;
  hipError_t e = hipSetDevice(device);
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  tsg::FetchWinCounters ctr = {};
  const size_t sc_bytes = tsg::FetchWinScratchBytes(n_bytes, n_files);
  // the arena as the library's callers give it: n_bytes + 64 readable bytes and no more (0xEE: not file bytes)
  if (ok(e) && ok(hipStreamCreate(&s)) && ok(hipMalloc(&d_arena, n_bytes + 64)) &&
      ok(hipMalloc(&d_off, (size_t(n_files) + 1) * 8)) && ok(hipMalloc(&d_cands, (held + 1) * sizeof(tsg::Candidate))) &&
      ok(hipMalloc(&d_count, 4)) && ok(hipMalloc(&d_ml, (size_t(n_rules) + 1) * 4)) && ok(hipMalloc(&d_sc, sc_bytes)) &&
      ok(hipMalloc(&d_ctr, sizeof ctr)) && ok(hipMalloc(&d_stage, stage_bytes)) &&
      ok(hipMemset(d_arena, 0xEE, n_bytes + 64)) && ok(hipMemcpy(d_arena, arena, n_bytes, hipMemcpyHostToDevice)) &&
      ok(hipMemcpy(d_off, offsets, (size_t(n_files) + 1) * 8, hipMemcpyHostToDevice)) &&
      ok(hipMemcpy(d_cands, cands, held * sizeof(tsg::Candidate), hipMemcpyHostToDevice)) &&
      ok(hipMemcpy(d_count, &count, 4, hipMemcpyHostToDevice)) &&
      ok(hipMemcpy(d_ml, rule_max_len, size_t(n_rules) * 4, hipMemcpyHostToDevice)) &&
      ok(tsg::FetchWinPlan(static_cast<const tsg::Candidate*>(d_cands), static_cast<const uint32_t*>(d_count), cand_cap,
                           static_cast<const uint64_t*>(d_off), n_files, n_bytes, static_cast<const uint32_t*>(d_ml),
                           n_rules, WinParamsOf(opts), d_sc, static_cast<tsg::FetchWinCounters*>(d_ctr), s)) &&
      ok(hipMemcpyAsync(&ctr, d_ctr, sizeof ctr, hipMemcpyDeviceToHost, s)) && ok(hipStreamSynchronize(s))) {
    const uint64_t total = ctr.granules * tsg::kFetchGranule;
    uint64_t rounds = 0;
    for (uint64_t w0 = 0; w0 < total && e == hipSuccess; w0 += stage_bytes, rounds++) {
      const uint64_t w1 = std::min(w0 + stage_bytes, total);
      // (the bytes the pack leaves alone -- the last granule's blocks past the arena -- read as 0)
      if (ok(hipMemsetAsync(d_stage, 0, stage_bytes, s)) &&
          ok(tsg::FetchWinPack(static_cast<const uint8_t*>(d_arena), n_bytes, d_sc, n_files,
                               static_cast<const tsg::FetchWinCounters*>(d_ctr), w0, w1, static_cast<uint8_t*>(d_stage),
                               s)) &&
          ok(hipStreamSynchronize(s)) && w0 < packed_cap)
        ok(hipMemcpy(packed + w0, d_stage, std::min(w1, packed_cap) - w0, hipMemcpyDeviceToHost));
    }
    counters[0] = ctr.granules;
    counters[1] = ctr.runs;
    counters[2] = ctr.whole_files;
    counters[3] = rounds;
  }
  for (void* p : {d_arena, d_off, d_cands, d_count, d_ml, d_sc, d_ctr, d_stage})
    if (p) (void)hipFree(p);
  if (s) (void)hipStreamDestroy(s);
  if (e != hipSuccess) {
    tsg::SetError(std::string("tsg_debug_fetch_windows_device: ") + hipGetErrorString(e));
    return -1;
  }
  return 0;
}

int tsg_debug_sparse_tail(const tsg_global* g, const tsg_batch* b, const void* cands, uint64_t n_cands,
                          const uint32_t* opts, tsg_result** out, tsg_fetch_window_stats* window_stats) {
  if (!g || !b || !out || !window_stats || !b->host_arena || !b->host_offsets) {
    tsg::SetError("tsg_debug_sparse_tail: NULL argument (a host batch is required)");
    return -2;
  }
  if (window_stats->struct_size != TSG_FETCH_WINDOW_STATS_SIZE_V1) {
    tsg::SetError("tsg_debug_sparse_tail: unknown tsg_fetch_window_stats.struct_size");
    return -2;
  }
  if (!WinArgsOk("tsg_debug_sparse_tail", b->host_offsets, b->n_files, opts)) return -2;
  std::string err;
  std::vector<tsg::RuleSpec> rules;
  std::vector<tsg::AllowRuleSpec> allow;
  std::vector<std::unique_ptr<tsg::Regex>> exclude;
  if (!tsg::MakeRules(g, &rules, &err) || !tsg::MakeAllow(g->allow_rules, g->n_allow_rules, &allow, &err) ||
      !tsg::MakeExclude(g->exclude_regexes, g->n_exclude_regexes, &exclude, &err)) {
    tsg::SetError(err);
    return -1;
  }
  std::unique_ptr<tsg::SecretScanner> sc(
      new tsg::SecretScanner(std::move(rules), std::move(allow), std::move(exclude), -1, &err));
  if (!sc->ok()) {
    tsg::SetError(err.empty() ? sc->error() : err);
    return -1;
  }
  std::vector<tsg::Candidate> cv(n_cands);
  if (n_cands) std::memcpy(cv.data(), cands, n_cands * sizeof(tsg::Candidate));
  for (const auto& c : cv)
    if (c.file >= b->n_files || c.rule >= sc->compiled().rules.size()) {
      tsg::SetError("candidate out of range");
      return -3;
    }
  tsg::BatchInput in;
  in.n_files = b->n_files;
  in.host_arena = b->host_arena;
  in.host_offsets = b->host_offsets;
  in.paths = b->paths;
  in.path_lens = b->path_lens;
  in.binary = b->binary;
  std::unique_ptr<tsg_result> r(new tsg_result());
  tsg::HostStats hs;
  if (!sc->SparseTail(in, &cv, WinParamsOf(opts), &r->files, &hs, &r->win, &err)) {
    tsg::SetError(err);
    return -1;
  }
  std::memset(&r->stats, 0, sizeof(r->stats));
  r->stats.bytes = in.n_files ? in.host_offsets[in.n_files] : 0;
  r->stats.files = in.n_files;
  r->stats.findings = hs.findings;
  r->stats.candidates = hs.candidates;
  r->owner = sc.get();
  r->owned = std::move(sc);
  window_stats->mode_used = r->win.mode_used;
  window_stats->granules = r->win.granules;
  window_stats->runs = r->win.runs;
  window_stats->window_bytes = r->win.window_bytes;
  window_stats->sparse_files = r->win.sparse_files;
  window_stats->whole_files = r->win.whole_files;
  window_stats->fallback_files = r->win.fallback_files;
  window_stats->fallback_bytes = r->win.fallback_bytes;
  window_stats->ms_fallback = r->win.ms_fallback;
  *out = r.release();
  return 0;
}

int tsg_debug_engine_stages(const tsg_compiled* c, int device, const uint8_t* arena, uint64_t n_bytes,
                            const uint64_t* offsets, uint32_t n_files, const uint8_t tail[64],
                            tsg_debug_stage_dump* out) {
  return tsg_debug_engine_stages_skip(c, device, arena, n_bytes, offsets, n_files, tail, nullptr, out);
}

int tsg_debug_engine_stages_skip(const tsg_compiled* c, int device, const uint8_t* arena, uint64_t n_bytes,
                                 const uint64_t* offsets, uint32_t n_files, const uint8_t tail[64],
                                 const uint8_t* skip, tsg_debug_stage_dump* out) {
  if (!c || !offsets || !tail || !out || (n_bytes && !arena)) {
    tsg::SetError("tsg_debug_engine_stages: NULL argument");
    return -2;
  }
  if (out->struct_size != sizeof(tsg_debug_stage_dump)) {
    tsg::SetError("tsg_debug_engine_stages: unknown tsg_debug_stage_dump.struct_size");
    return -2;
  }
  if (!WinArgsOk("tsg_debug_engine_stages", offsets, n_files, nullptr)) return -2;
  if (offsets[n_files] != n_bytes) {
    tsg::SetError("tsg_debug_engine_stages: offsets must end at n_bytes");
    return -2;
  }
  void *d_arena = nullptr, *d_off = nullptr, *d_skip = nullptr;
  hipError_t e = hipSetDevice(device);
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  tsg::StageDump d;
  std::string run_err;
  // the arena as the library's callers give it: n_bytes + 64 readable bytes and no more
  if (ok(e) && ok(hipMalloc(&d_arena, n_bytes + 64)) && ok(hipMalloc(&d_off, (size_t(n_files) + 1) * 8)) &&
      ok(hipMemcpy(static_cast<uint8_t*>(d_arena) + n_bytes, tail, 64, hipMemcpyHostToDevice)) &&
      (n_bytes == 0 || ok(hipMemcpy(d_arena, arena, n_bytes, hipMemcpyHostToDevice))) &&
      ok(hipMemcpy(d_off, offsets, (size_t(n_files) + 1) * 8, hipMemcpyHostToDevice)) &&
      (!skip || n_files == 0 ||
       (ok(hipMalloc(&d_skip, n_files)) && ok(hipMemcpy(d_skip, skip, n_files, hipMemcpyHostToDevice))))) {
    // a fresh engine per call: the TSG_* switches its constructor reads apply to this scan -- tests
    // that compare variants rely on it
    std::unique_ptr<tsg::GpuEngine> eng(new tsg::GpuEngine(c->cr, device));
    std::vector<tsg::Candidate> cands;
    tsg::SkipIn sk;
    sk.d_skip = static_cast<const uint8_t*>(d_skip);
    if (!eng->ok() || !eng->Run(static_cast<const uint8_t*>(d_arena), n_bytes, static_cast<const uint64_t*>(d_off),
                                n_files, &cands, nullptr, nullptr, d_skip ? &sk : nullptr, &d))
      run_err = eng->error().empty() ? "engine failed" : eng->error();
  }
  for (void* p : {d_arena, d_off, d_skip})
    if (p) (void)hipFree(p);
  if (e != hipSuccess || !run_err.empty()) {
    tsg::SetError(std::string("tsg_debug_engine_stages: ") + (e != hipSuccess ? hipGetErrorString(e) : run_err.c_str()));
    return -1;
  }
  out->kw_words = d.kw_words;
  static_assert(sizeof(out->counters) == tsg::kScanCtrBytes, "tsg_debug_stage_dump hands out the scan counters whole");
  std::memcpy(out->counters, d.counters, sizeof(out->counters));
  out->caps[0] = d.hit_cap;
  out->caps[1] = d.rec_cap;
  out->caps[2] = d.cand_cap;
  auto put = [](void* dst, uint64_t cap, uint64_t* n, const void* src, size_t count, size_t rec) {
    *n = count;
    const size_t k = size_t(std::min<uint64_t>(cap, count));
    if (dst && k) std::memcpy(dst, src, k * rec);
  };
  std::vector<uint64_t> hits(3 * d.hits.size());
  for (size_t i = 0; i < d.hits.size(); i++) {
    hits[3 * i] = d.hits[i].file;
    hits[3 * i + 1] = d.hits[i].end;
    hits[3 * i + 2] = d.hits[i].aid;
  }
  put(out->hits, out->hits_cap, &out->n_hits, hits.data(), d.hits.size(), 24);
  put(out->kw, out->kw_cap, &out->n_kw, d.kw.data(), d.kw.size(), 4);
  put(out->flags, out->flags_cap, &out->n_flags, d.flags.data(), d.flags.size(), 4);
  put(out->nl, out->nl_cap, &out->n_nl, d.nl.data(), d.nl.size(), 2);
  put(out->chunk_file, out->chunk_file_cap, &out->n_chunk_file, d.chunk_file.data(), d.chunk_file.size(), 4);
  put(out->recs, out->recs_cap, &out->n_recs, d.recs.data(), d.recs.size(), 4);
  put(out->cands, out->cands_cap, &out->n_cands, d.cands.data(), d.cands.size(), sizeof(tsg::Candidate));
  return 0;
}

int tsg_debug_scan_grow(const uint32_t* counters, const uint32_t* fs_counters, uint32_t caps[7]) {
  static_assert(tsg::kScanCtrWords == 16 && tsg::kNFsCtr == 6, "the sizes tsg_debug.h states");
  tsg::ScanCaps c;
  uint32_t* const field[7] = {&c.hit, &c.cand, &c.rec, &c.fold, &c.fs_pair, &c.fs_task, &c.fs_task_bytes};
  for (int i = 0; i < 7; i++) *field[i] = caps[i];
  const int which = tsg::GrowOverflowed(counters, fs_counters, &c);
  for (int i = 0; i < 7; i++) caps[i] = *field[i];
  return which;
}

int tsg_debug_pool_budget(void) { return tsg::PoolBudget(); }

int tsg_debug_filter_core(const tsg_compiled* c, uint32_t out[4]) {
  const auto* f = c->cr.filter.get();
  if (!f) return -1;
  const uint32_t n_groups = uint32_t(f->core.size() / 256);
  std::vector<std::vector<uint64_t>> cols;  // distinct byte columns of the core tables
  for (uint32_t b = 0; b < 256; b++) {
    std::vector<uint64_t> col(n_groups);
    for (uint32_t g = 0; g < n_groups; g++) col[g] = f->core[size_t(g) * 256 + b];
    if (std::find(cols.begin(), cols.end(), col) == cols.end()) cols.push_back(std::move(col));
  }
  uint32_t most = 0;
  for (uint32_t b = 0; b + 1 < f->bucket_groups.size(); b++) most = std::max(most, f->bucket_groups[b + 1] - f->bucket_groups[b]);
  out[0] = n_groups;
  out[1] = uint32_t(cols.size());
  out[2] = most;
  out[3] = uint32_t(f->hash_keys.size());
  return 0;
}

int tsg_debug_filter_orform(const tsg_compiled* c, uint32_t out[1024]) {
  const auto* f = c->cr.filter.get();
  if (!f || f->n_buckets != 16 || f->n_words != 4 || f->window > 6 || f->reach.size() != 256 * 4) return -1;
  for (uint32_t b = 0; b < 256; b++) tsg::OrFormRow(&f->reach[size_t(b) * 4], out + size_t(b) * 4);
  return 0;
}

int tsg_debug_sure_allow(const char* const* patterns, uint32_t n_patterns, const uint8_t* paths, const uint64_t* off,
                         uint32_t n_paths, uint8_t* sure, uint8_t* has_form) {
  std::vector<std::unique_ptr<tsg::Regex>> own;
  std::vector<const tsg::Regex*> res;
  for (uint32_t i = 0; i < n_patterns; i++) {
    std::string err;
    own.push_back(tsg::Regex::Compile(patterns[i], &err));
    if (!own.back()) {
      tsg::SetError(err);
      return -1;
    }
    res.push_back(own.back().get());
  }
  tsg::SureTable t;
  std::vector<uint8_t> form;
  tsg::SureTableOf(res, &t, &form);  // (none / no fit: words = 0, nothing is surely allowed)
  if (has_form && n_patterns) std::memcpy(has_form, form.data(), n_patterns);
  for (uint32_t i = 0; i < n_paths; i++) sure[i] = tsg::SureAllowHost(t, paths + off[i], off[i + 1] - off[i]) ? 1 : 0;
  return 0;
}

// ---- the findings kernels and the path filter ----

int tsg_debug_materialize(int device, const uint8_t* arena, uint64_t n_bytes, const uint64_t* offsets, uint32_t n_files,
                          const void* mat_files, uint32_t n_mat_files, const void* matches, uint32_t n_match,
                          const void* spans, uint32_t n_span, int guard, void* findings_out, uint64_t* pref_out,
                          void* lines_out, uint64_t lines_cap, uint8_t* text_out, uint64_t text_cap,
                          uint64_t totals[2]) {
  const char* who = "tsg_debug_materialize";
  auto refuse = [&](const std::string& why) {
    tsg::SetError(std::string(who) + ": " + why);
    return -2;
  };
  if (!arena || !offsets || !totals || (n_mat_files && !mat_files) || (n_match && (!matches || !findings_out)) ||
      !pref_out || (n_span && !spans) || (lines_cap && !lines_out) || (text_cap && !text_out))
    return refuse("NULL argument");
  totals[0] = totals[1] = 0;
  if (offsets[0] != 0) return refuse("offsets must start at 0");
  for (uint32_t f = 0; f < n_files; f++)
    if (offsets[f + 1] < offsets[f]) return refuse("offsets must ascend");
  if (offsets[n_files] != n_bytes) return refuse("offsets must end at n_bytes");
  const tsg::MatFile* F = static_cast<const tsg::MatFile*>(mat_files);
  const tsg::MatMatch* M = static_cast<const tsg::MatMatch*>(matches);
  const tsg::MatSpan* Sp = static_cast<const tsg::MatSpan*>(spans);
  // the records as the scanner builds them: each file's locations and spans follow those of the file before
  uint64_t m_at = 0, s_at = 0, text_bound = 0;
  for (uint32_t i = 0; i < n_mat_files; i++) {
    const std::string fi = "file record " + std::to_string(i);
    if (F[i].file >= n_files) return refuse(fi + ": no such file");
    if (F[i].m0 != m_at) return refuse(fi + ": m0 contradicts the locations of the records before it");
    if (F[i].s0 != s_at) return refuse(fi + ": s0 contradicts the spans of the records before it");
    m_at += F[i].nm;
    s_at += F[i].ns;
    if (m_at > n_match || s_at > n_span) return refuse(fi + ": its locations or spans leave the arrays");
    const int64_t len = int64_t(offsets[F[i].file + 1] - offsets[F[i].file]);
    const tsg::MatSpan* sp = Sp + F[i].s0;
    if (F[i].ns == 0 || sp[F[i].ns - 1].s != INT64_MAX || sp[F[i].ns - 1].e != INT64_MAX)
      return refuse(fi + ": its spans lack the sentinel");
    for (uint32_t k = 0; k + 1 < F[i].ns; k++) {
      if (sp[k].s < 0 || sp[k].e <= sp[k].s || sp[k].e > len) return refuse(fi + ": span " + std::to_string(k) + " is empty or outside its file");
      if (k && sp[k].s <= sp[k - 1].e)
        return refuse(fi + ": span " + std::to_string(k) + " is unsorted, touches or overlaps the one before");
    }
    for (uint32_t q = 0; q < F[i].nm; q++) {
      const tsg::MatMatch& m = M[F[i].m0 + q];
      const std::string mi = "location " + std::to_string(F[i].m0 + q);
      if (m.fidx != i) return refuse(mi + ": fidx contradicts the file record that holds it");
      if (m.e < m.s) return refuse(mi + ": e < s");
      if (m.s < 0 || m.e > len) return refuse(mi + ": outside its file");
      if (m.a_wlo < 0 || m.a_wlo > m.s || m.a_nl < 0) return refuse(mi + ": a_wlo > s (or a negative anchor)");
      if (m.e > m.s) {  // EndLine = StartLine holds because a location is censored whole
        bool covered = false;
        for (uint32_t k = 0; k + 1 < F[i].ns && !covered; k++) covered = sp[k].s <= m.s && m.e <= sp[k].e;
        if (!covered) return refuse(mi + ": no span covers it");
      }
      text_bound += tsg::MatTextBound(m.s, m.e);
    }
  }
  if (m_at != n_match || s_at != n_span) return refuse("locations or spans that no file record holds");
  void *d_arena = nullptr, *d_off = nullptr;
  hipError_t e = hipSetDevice(device);
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  int rc = 0;
  std::string err;
  // the arena as the caller gives it, tail included, in an allocation of exactly that size
  if (ok(e) && ok(hipMalloc(&d_arena, n_bytes + 64)) && ok(hipMalloc(&d_off, (size_t(n_files) + 1) * 8)) &&
      ok(hipMemcpy(d_arena, arena, n_bytes + 64, hipMemcpyHostToDevice)) &&
      ok(hipMemcpy(d_off, offsets, (size_t(n_files) + 1) * 8, hipMemcpyHostToDevice))) {
    std::unique_ptr<tsg::FindingMaterializer> mat(new tsg::FindingMaterializer(device));
    mat->set_guard(guard != 0);
    tsg::FindingMaterializer::Job* job = mat->ok() ? mat->Begin(n_mat_files, n_match, n_span, text_bound, &err) : nullptr;
    if (!job) {
      if (err.empty()) err = mat->error();
      rc = -1;
    } else {
      if (n_mat_files) std::memcpy(mat->files(job), F, size_t(n_mat_files) * sizeof(tsg::MatFile));
      if (n_match) std::memcpy(mat->matches(job), M, size_t(n_match) * sizeof(tsg::MatMatch));
      if (n_span) std::memcpy(mat->spans(job), Sp, size_t(n_span) * sizeof(tsg::MatSpan));
      const bool ran = mat->Run(job, static_cast<const uint8_t*>(d_arena), static_cast<const uint64_t*>(d_off), &err);
      const uint64_t tot = mat->totals(job);
      totals[0] = uint32_t(tot);
      totals[1] = tot >> 32;
      if (!ran) {
        switch (mat->fail(job)) {
          case tsg::FindingMaterializer::kSelfCheck: rc = -5; break;
          case tsg::FindingMaterializer::kGuard: rc = -4; break;
          case tsg::FindingMaterializer::kBounds: rc = -6; break;
          default: rc = -1;
        }
      } else if (n_match) {
        std::memcpy(findings_out, mat->findings(job), size_t(n_match) * sizeof(tsg::FindingOut));
        std::memcpy(pref_out, mat->pref(job), (size_t(n_match) + 1) * 8);
        if (totals[0] > lines_cap || totals[1] > text_cap) {
          err = "lines_cap or text_cap is below the totals";
          rc = -3;
        } else {
          if (totals[0]) std::memcpy(lines_out, mat->lines(job), size_t(totals[0]) * sizeof(tsg::LineOut));
          if (totals[1]) std::memcpy(text_out, mat->text(job), size_t(totals[1]));
        }
      } else {
        pref_out[0] = 0;
      }
      mat->End(job);
    }
  }
  for (void* p : {d_arena, d_off})
    if (p) (void)hipFree(p);
  if (e != hipSuccess) {
    tsg::SetError(std::string(who) + ": " + hipGetErrorString(e));
    return -1;
  }
  if (rc != 0) tsg::SetError(std::string(who) + ": " + err);
  return rc;
}

int tsg_debug_path_tables(const uint8_t* lit_bytes, const uint64_t* lit_off, const uint32_t* lit_rule, uint32_t n_lits,
                          const uint8_t* sure_pairs, const uint64_t* sure_off, const uint8_t* sure_flags,
                          uint32_t n_sure, void* path_table_out, uint64_t path_cap, void* sure_table_out,
                          uint64_t sure_cap) {
  if ((n_lits && (!lit_bytes || !lit_off || !lit_rule)) || (n_sure && (!sure_pairs || !sure_off || !sure_flags)) ||
      !path_table_out || !sure_table_out || path_cap < sizeof(tsg::PathTable) || sure_cap < sizeof(tsg::SureTable)) {
    tsg::SetError("tsg_debug_path_tables: NULL argument or a buffer too small");
    return -1;
  }
  std::vector<std::pair<std::string, uint32_t>> lits;
  for (uint32_t i = 0; i < n_lits; i++) {
    if (lit_off[i + 1] < lit_off[i]) {
      tsg::SetError("tsg_debug_path_tables: literal offsets must ascend");
      return -1;
    }
    lits.emplace_back(std::string(reinterpret_cast<const char*>(lit_bytes) + lit_off[i], size_t(lit_off[i + 1] - lit_off[i])),
                      lit_rule[i]);
  }
  std::vector<tsg::SureLit> sure;
  for (uint32_t i = 0; i < n_sure; i++) {
    if (sure_off[i + 1] < sure_off[i]) {
      tsg::SetError("tsg_debug_path_tables: literal offsets must ascend");
      return -1;
    }
    tsg::SureLit l;
    for (uint64_t p = sure_off[i]; p < sure_off[i + 1]; p++) l.pos.emplace_back(sure_pairs[2 * p], sure_pairs[2 * p + 1]);
    l.begin = (sure_flags[i] & 1) != 0;
    l.end = (sure_flags[i] & 2) != 0;
    sure.push_back(std::move(l));
  }
  tsg::PathTable pt;
  tsg::SureTable st;
  int have = 0;
  if (tsg::BuildPathTable(lits, &pt)) have |= 1;
  else std::memset(&pt, 0, sizeof pt);
  if (tsg::BuildSureTable(sure, &st)) have |= 2;
  std::memcpy(path_table_out, &pt, sizeof pt);
  std::memcpy(sure_table_out, &st, sizeof st);
  return have;
}

int tsg_debug_path_filter(int device, const void* path_table, const void* sure_table, const uint8_t* paths,
                          const uint64_t* off, const uint32_t* batch_first, uint32_t n_batches, uint32_t flags,
                          void* hits_out, uint32_t* n_hits_out, uint8_t* skip_out, uint8_t* have_skip_out) {
  const char* who = "tsg_debug_path_filter";
  auto refuse = [&](const char* why) {
    tsg::SetError(std::string(who) + ": " + why);
    return -2;
  };
  if (!path_table || !off || !batch_first || !hits_out || !n_hits_out || !skip_out || !have_skip_out || (flags & ~3u))
    return refuse("NULL argument or an unknown flag");
  for (uint32_t b = 0; b < n_batches; b++)
    if (batch_first[b + 1] < batch_first[b]) return refuse("batch_first must ascend");
  const uint32_t n_paths = batch_first[n_batches];
  for (uint32_t i = batch_first[0]; i < n_paths; i++)
    if (off[i + 1] < off[i]) return refuse("off must ascend");
  if (n_paths > batch_first[0] && off[n_paths] > off[batch_first[0]] && !paths) return refuse("paths missing");
  tsg::PathTable pt;
  std::memcpy(&pt, path_table, sizeof pt);
  if (pt.words < 1 || pt.words > 4) return refuse("the path table's words must be 1..4");
  for (uint32_t i = 0; i < 256; i++)
    if (pt.rule_of[i] >= 64) return refuse("the path table names a rule past 63");
  tsg::SureTable st;
  if (sure_table) {
    std::memcpy(&st, sure_table, sizeof st);
    if (st.words < 1 || st.words > 4) return refuse("the sure table's words must be 1..4");
  }
  const bool host_packed = (flags & 1u) != 0, want_skip = (flags & 2u) != 0;
  hipError_t e = hipSetDevice(device);
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  std::string err;
  int rc = 0;
  if (ok(e)) {
    // one filter for the whole sequence: the slot, its counter parity and the last count carry over
    std::unique_ptr<tsg::PathFilter> pf(new tsg::PathFilter(device, pt));
    if (sure_table) pf->SetSureTable(st);
    pf->set_skip_fill(true);
    if (!pf->ok() || (sure_table && !pf->has_sure())) {
      err = pf->ok() ? "the sure table did not reach the device" : pf->error();
      rc = -1;
    }
    std::vector<tsg::PathHit> hits;
    std::vector<uint64_t> rel;
    for (uint32_t b = 0; rc == 0 && e == hipSuccess && b < n_batches; b++) {
      const uint32_t first = batch_first[b], n = batch_first[b + 1] - first;
      const uint64_t p0 = off[first], nb = off[first + n] - p0;
      void *d_paths = nullptr, *d_off = nullptr;
      tsg::PathFilter::Pending p;
      bool done = false;
      if (host_packed) {
        done = pf->Submit(nullptr, nullptr, paths, off + first, n, want_skip, &p, &err);
      } else {
        // the paths in an allocation of exactly their bytes, the offsets from 0
        rel.resize(size_t(n) + 1);
        for (uint32_t i = 0; i <= n; i++) rel[i] = off[first + i] - p0;
        if ((nb == 0 || (ok(hipMalloc(&d_paths, nb)) && ok(hipMemcpy(d_paths, paths + p0, nb, hipMemcpyHostToDevice)))) &&
            ok(hipMalloc(&d_off, rel.size() * 8)) && ok(hipMemcpy(d_off, rel.data(), rel.size() * 8, hipMemcpyHostToDevice)))
          done = pf->Submit(static_cast<const uint8_t*>(d_paths), static_cast<const uint64_t*>(d_off), nullptr, nullptr, n,
                            want_skip, &p, &err);
      }
      have_skip_out[b] = 0;
      if (done && p.d_skip) {  // as the scan's stream does: behind `ready`
        if (ok(hipEventSynchronize(p.ready)) && ok(hipMemcpy(skip_out + first, p.d_skip, n, hipMemcpyDeviceToHost)))
          have_skip_out[b] = 1;
      }
      if (done && e == hipSuccess) done = pf->Finish(&p, &hits, &err);
      pf->Release(&p);
      if (e == hipSuccess && !done) rc = -1;
      if (rc == 0 && e == hipSuccess) {
        n_hits_out[b] = uint32_t(hits.size());
        if (!hits.empty())  // (Finish refuses a count above n)
          std::memcpy(static_cast<tsg::PathHit*>(hits_out) + first, hits.data(), hits.size() * sizeof(tsg::PathHit));
      }
      for (void* q : {d_paths, d_off})
        if (q) (void)hipFree(q);
    }
  }
  if (e != hipSuccess) {
    tsg::SetError(std::string(who) + ": " + hipGetErrorString(e));
    return -1;
  }
  if (rc != 0) tsg::SetError(std::string(who) + ": " + err);
  return rc;
}

int tsg_debug_result_skip(const struct tsg_result* r, uint64_t out[6]) {
  if (!r) return -1;
  std::memcpy(out, r->skip, sizeof(r->skip));
  return 0;
}

int tsg_debug_result_k0(const struct tsg_result* r, double* ms_k0) {
  if (!r || !ms_k0) return -1;
  *ms_k0 = r->ms_k0;
  return 0;
}
}
