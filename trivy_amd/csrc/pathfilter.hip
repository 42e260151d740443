// GPU allow-path prefilter (pathfilter.h).
#include "pathfilter.h"

#include <chrono>
#include <cstring>
#include <thread>

namespace tsg {

bool BuildPathTable(const std::vector<std::pair<std::string, uint32_t>>& lits, PathTable* t) {
  std::memset(t, 0, sizeof(*t));
  uint32_t w = 0, bit = 0;
  for (auto& [lit, rule] : lits) {
    const size_t k = lit.size();
    if (k < 2 || k > 64 || rule >= 64) return false;
    if (bit + k > 64) {  // a literal never crosses a word
      w++;
      bit = 0;
    }
    if (w >= 4) return false;
    t->S[w] |= uint64_t(1) << bit;
    for (size_t j = 0; j < k; j++) {
      const uint8_t c = uint8_t(lit[j]);
      if (c >= 'A' && c <= 'Z') return false;  // the literals are lowercased (Matcher::lits)
      t->B[c][w] |= uint64_t(1) << (bit + j);
    }
    t->E[w] |= uint64_t(1) << (bit + k - 1);
    t->rule_of[w * 64 + bit + k - 1] = uint8_t(rule);
    bit += uint32_t(k);
  }
  t->words = w + 1;
  return !lits.empty();
}

bool BuildSureTable(const std::vector<SureLit>& lits, SureTable* t) {
  std::memset(t, 0, sizeof(*t));
  uint32_t w = 0, bit = 0;
  for (const SureLit& l : lits) {
    const size_t k = l.pos.size();
    if (k < 1 || k > 64) continue;  // (ExactPathLiterals makes none such)
    if (bit + k > 64) {  // a literal never crosses a word
      w++;
      bit = 0;
    }
    if (w >= 4) {
      std::memset(t, 0, sizeof(*t));
      return false;
    }
    (l.begin ? t->S0 : t->S)[w] |= uint64_t(1) << bit;
    for (size_t j = 0; j < k; j++) {
      t->B[l.pos[j].first][w] |= uint64_t(1) << (bit + j);
      t->B[l.pos[j].second][w] |= uint64_t(1) << (bit + j);
    }
    (l.end ? t->EZ : t->E)[w] |= uint64_t(1) << (bit + k - 1);
    bit += uint32_t(k);
  }
  if (w == 0 && bit == 0) return false;
  t->words = w + 1;
  return true;
}

bool SureAllowHost(const SureTable& t, const uint8_t* p, uint64_t n) {
  if (t.words == 0 || n == 0 || n > kSureMaxPath) return false;
  uint64_t D[4] = {0, 0, 0, 0}, H = 0;
  uint32_t high = 0;
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t c = p[i];
    high |= c;
    for (int w = 0; w < 4; w++) {
      D[w] = TSG_SURE_STEP(D[w], w, c, i == 0, t.B, t.S, t.S0, t.E, t.EZ);
      H |= D[w] & (t.E[w] | (i + 1 == n ? t.EZ[w] : 0));
    }
  }
  return H != 0 && !(high & 0x80u);
}

namespace {

constexpr int kPathThreads = 256;

// kSure: also the exact shift-and of the sure table X, one skip byte per path.
template <bool kSure>
__global__ __launch_bounds__(kPathThreads) void path_filter_kernel(const uint8_t* __restrict__ paths,
                                                                   const uint64_t* __restrict__ off, uint32_t n,
                                                                   const PathTable* __restrict__ T,
                                                                   const SureTable* __restrict__ X,
                                                                   uint8_t* __restrict__ skip,
                                                                   uint32_t* __restrict__ cnt,
                                                                   uint32_t* __restrict__ cnt_next,
                                                                   PathHit* __restrict__ out) {
  // the counter of this slot's next launch (stream-ordered after this one): no
  // fill kernel per call
  if (blockIdx.x == 0 && threadIdx.x == 0) *cnt_next = 0;
  __shared__ uint64_t sB[256][4];
  __shared__ uint64_t sX[kSure ? 256 : 1][4];
  __shared__ uint8_t s_rule[256];
  for (uint32_t i = threadIdx.x; i < 256 * 4; i += kPathThreads) (&sB[0][0])[i] = (&T->B[0][0])[i];
  if (kSure)
    for (uint32_t i = threadIdx.x; i < 256 * 4; i += kPathThreads) (&sX[0][0])[i] = (&X->B[0][0])[i];
  for (uint32_t i = threadIdx.x; i < 256; i += kPathThreads) s_rule[i] = T->rule_of[i];
  __syncthreads();
  uint64_t S[4], E[4];
  uint64_t XS[4] = {}, XS0[4] = {}, XE[4] = {}, XEZ[4] = {};
#pragma unroll
  for (int w = 0; w < 4; w++) {
    S[w] = T->S[w];
    E[w] = T->E[w];
    if (kSure) {
      XS[w] = X->S[w];
      XS0[w] = X->S0[w];
      XE[w] = X->E[w];
      XEZ[w] = X->EZ[w];
    }
  }
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t stride = gridDim.x * kPathThreads;
  // whole waves iterate together (the ballot below needs every lane)
  for (uint32_t base = blockIdx.x * kPathThreads + (threadIdx.x & ~63u); base < n; base += stride) {
    const uint32_t i = base + lane;
    uint32_t rec = 0;
    uint64_t rules = 0;
    bool emit = false;
    if (i < n) {
      uint64_t D[4] = {0, 0, 0, 0}, H[4] = {0, 0, 0, 0};
      uint64_t XD[4] = {0, 0, 0, 0}, XH = 0;
      uint32_t high = 0;
      const uint64_t b = off[i], e = off[i + 1];
      for (uint64_t p = b; p < e; p++) {
        const uint32_t r = paths[p];
        high |= r;
        const uint32_t c = r + ((r - 'A') < 26u ? 32u : 0u);
#pragma unroll
        for (int w = 0; w < 4; w++) {
          D[w] = TSG_PATH_STEP(D[w], w, c, sB, S);
          H[w] |= D[w] & E[w];
        }
        if (kSure) {
#pragma unroll
          for (int w = 0; w < 4; w++) {
            XD[w] = TSG_SURE_STEP(XD[w], w, r, p == b, sX, XS, XS0, XE, XEZ);
            XH |= XD[w] & (XE[w] | (p + 1 == e ? XEZ[w] : 0));
          }
        }
      }
      if (kSure) skip[i] = (XH != 0 && !(high & 0x80u) && e - b <= kSureMaxPath) ? 1 : 0;
      if (high & 0x80u) {
        rec = i | kPathNonAscii;
        emit = true;
      } else {
#pragma unroll
        for (int w = 0; w < 4; w++)
          for (uint64_t h = H[w]; h; h &= h - 1) rules |= uint64_t(1) << s_rule[w * 64 + __builtin_ctzll(h)];
        rec = i;
        emit = rules != 0;
      }
    }
    const uint64_t m = __ballot(emit);
    if (m) {
      uint32_t at = 0;
      if (lane == 0) at = atomicAdd(cnt, uint32_t(__popcll(m)));
      at = __shfl(at, 0);
      if (emit) {
        const uint32_t below = __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
        PathHit h;
        h.file = rec;
        h.pad = 0;
        h.rules = rules;
        out[at + below] = h;
      }
    }
  }
}

}  // namespace

PathFilter::PathFilter(int device, const PathTable& t) : device_(device) {
  int lo = 0, hi = 0;
  if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) lo = hi = 0;
  bool ok = hipSetDevice(device) == hipSuccess &&
            hipMalloc(reinterpret_cast<void**>(&d_table_), sizeof(PathTable)) == hipSuccess &&
            hipMemcpy(d_table_, &t, sizeof(PathTable), hipMemcpyHostToDevice) == hipSuccess;
  for (Slot& S : slots_)
    ok = ok && hipStreamCreateWithPriority(&S.stream, hipStreamNonBlocking, hi) == hipSuccess &&
         hipEventCreateWithFlags(&S.done, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&S.ready, hipEventDisableTiming) == hipSuccess &&
         hipMalloc(reinterpret_cast<void**>(&S.d_cnt), 64) == hipSuccess &&
         hipMemset(S.d_cnt, 0, 64) == hipSuccess &&
         hipHostMalloc(reinterpret_cast<void**>(&S.h_cnt), 64, hipHostMallocDefault) == hipSuccess;
  if (!ok) err_ = "PathFilter: HIP setup failed";
}

void PathFilter::SetSureTable(const SureTable& t) {
  if (t.words == 0 || d_sure_ || !err_.empty()) return;
  SureTable* d = nullptr;
  if (hipSetDevice(device_) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&d), sizeof(SureTable)) == hipSuccess) {
    if (hipMemcpy(d, &t, sizeof(SureTable), hipMemcpyHostToDevice) == hipSuccess) d_sure_ = d;
    else (void)hipFree(d);
  }
}

PathFilter::~PathFilter() {
  (void)hipSetDevice(device_);
  for (Slot& S : slots_) {
    if (S.stream) (void)hipStreamSynchronize(S.stream);
    if (S.d_out) (void)hipFree(S.d_out);
    if (S.h_out) (void)hipHostFree(S.h_out);
    if (S.d_paths) (void)hipFree(S.d_paths);
    if (S.h_stage) (void)hipHostFree(S.h_stage);
    if (S.d_skip) (void)hipFree(S.d_skip);
    if (S.d_cnt) (void)hipFree(S.d_cnt);
    if (S.h_cnt) (void)hipHostFree(S.h_cnt);
    if (S.done) (void)hipEventDestroy(S.done);
    if (S.ready) (void)hipEventDestroy(S.ready);
    if (S.stream) (void)hipStreamDestroy(S.stream);
  }
  if (d_table_) (void)hipFree(d_table_);
  if (d_sure_) (void)hipFree(d_sure_);
}

void PathFilter::Release(Pending* p) {
  if (p->slot < 0) return;
  {
    std::lock_guard<std::mutex> g(mu_);
    slots_[p->slot].busy = false;
  }
  cv_.notify_one();
  *p = Pending();
}

bool PathFilter::Submit(const uint8_t* d_paths, const uint64_t* d_off, const uint8_t* h_paths, const uint64_t* h_off,
                        uint32_t n, bool want_skip, Pending* p, std::string* err) {
  *p = Pending();
  p->n = n;
  if (n == 0) return true;
  Slot* S = nullptr;
  {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] {
      for (Slot& x : slots_)
        if (!x.busy) return true;
      return false;
    });
    for (Slot& x : slots_)
      if (!x.busy) {
        S = &x;
        break;
      }
    S->busy = true;
  }
  p->slot = int(S - slots_);
  auto fail = [&](const char* what, hipError_t e) {
    *err = std::string("PathFilter: ") + what + ": " + hipGetErrorString(e);
    Release(p);
    return false;
  };
  hipError_t e = hipSetDevice(device_);
  if (e != hipSuccess) return fail("hipSetDevice", e);
  if (S->cap < n) {
    if (S->d_out) (void)hipFree(S->d_out);
    if (S->h_out) (void)hipHostFree(S->h_out);
    S->d_out = nullptr;
    S->h_out = nullptr;
    S->cap = 0;
    if ((e = hipMalloc(reinterpret_cast<void**>(&S->d_out), size_t(n) * sizeof(PathHit))) != hipSuccess ||
        (e = hipHostMalloc(reinterpret_cast<void**>(&S->h_out), size_t(n) * sizeof(PathHit), hipHostMallocDefault)) !=
            hipSuccess)
      return fail("hipMalloc", e);
    S->cap = n;
  }
  const bool sure = want_skip && d_sure_ != nullptr;
  if (sure && S->skip_cap < n) {
    if (S->d_skip) (void)hipFree(S->d_skip);
    S->d_skip = nullptr;
    S->skip_cap = 0;
    const size_t cap = size_t(n) + size_t(n) / 4 + 256;
    if ((e = hipMalloc(reinterpret_cast<void**>(&S->d_skip), cap)) != hipSuccess) return fail("hipMalloc (skip)", e);
    if (skip_fill_ && (e = hipMemsetAsync(S->d_skip, 0xEE, cap, S->stream)) != hipSuccess)
      return fail("hipMemsetAsync (skip)", e);
    S->skip_cap = cap;
  }
  if (h_paths) {  // host-packed paths: offsets (rebased to 0) and bytes via pinned staging to HBM
    const uint64_t p0 = h_off[0], nb = h_off[n] - p0, ob = (uint64_t(n) + 1) * 8;
    const uint64_t need = ((ob + 15) & ~uint64_t(15)) + nb;
    if (S->paths_cap < need) {
      if (S->d_paths) (void)hipFree(S->d_paths);
      if (S->h_stage) (void)hipHostFree(S->h_stage);
      S->d_paths = nullptr;
      S->h_stage = nullptr;
      S->paths_cap = S->stage_cap = 0;
      const size_t cap = size_t(need + need / 4 + 4096);
      if ((e = hipMalloc(reinterpret_cast<void**>(&S->d_paths), cap)) != hipSuccess ||
          (e = hipHostMalloc(reinterpret_cast<void**>(&S->h_stage), cap, hipHostMallocDefault)) != hipSuccess)
        return fail("hipMalloc (paths)", e);
      S->paths_cap = S->stage_cap = cap;
    }
    // the previous call's copy out of the staging buffer is done: that call waited for its stream
    uint64_t* so = reinterpret_cast<uint64_t*>(S->h_stage);
    for (uint32_t i = 0; i <= n; i++) so[i] = h_off[i] - p0;
    const uint64_t pb = (ob + 15) & ~uint64_t(15);
    std::memcpy(S->h_stage + pb, h_paths + p0, size_t(nb));
    if ((e = hipMemcpyAsync(S->d_paths, S->h_stage, size_t(pb + nb), hipMemcpyHostToDevice, S->stream)) !=
        hipSuccess)
      return fail("hipMemcpyAsync (paths)", e);
    d_off = reinterpret_cast<const uint64_t*>(S->d_paths);
    d_paths = S->d_paths + pb;
  }
  // this launch's counter was zeroed by the slot's previous launch (or at set-up)
  uint32_t* cnt = S->d_cnt + S->parity;
  uint32_t* cnt_next = S->d_cnt + (1 - S->parity);
  S->parity ^= 1u;
  const uint32_t grid = uint32_t(std::min<uint64_t>((uint64_t(n) + kPathThreads - 1) / kPathThreads, 4096));
  if (sure)
    path_filter_kernel<true><<<grid, kPathThreads, 0, S->stream>>>(d_paths, d_off, n, d_table_, d_sure_, S->d_skip, cnt,
                                                                   cnt_next, S->d_out);
  else
    path_filter_kernel<false><<<grid, kPathThreads, 0, S->stream>>>(d_paths, d_off, n, d_table_, nullptr, nullptr, cnt,
                                                                    cnt_next, S->d_out);
  if ((e = hipGetLastError()) != hipSuccess) {
    (void)hipStreamSynchronize(S->stream);  // (a failed launch left cnt_next as it was: clear it for the next call)
    (void)hipMemset(cnt_next, 0, 4);
    return fail("path_filter_kernel", e);
  }
  if (sure) {
    if ((e = hipEventRecord(S->ready, S->stream)) != hipSuccess) {
      (void)hipStreamSynchronize(S->stream);
      return fail("hipEventRecord", e);
    }
    p->d_skip = S->d_skip;
    p->ready = S->ready;
  }
  // the count and as many records as the last call had (+1/8): one round trip when the paths repeat
  p->guess = std::min<uint32_t>(n, last_k_.load() + last_k_.load() / 8 + 1024);
  if ((e = hipMemcpyAsync(S->h_cnt, cnt, 4, hipMemcpyDeviceToHost, S->stream)) != hipSuccess ||
      (e = hipMemcpyAsync(S->h_out, S->d_out, size_t(p->guess) * sizeof(PathHit), hipMemcpyDeviceToHost,
                          S->stream)) != hipSuccess ||
      (e = hipEventRecord(S->done, S->stream)) != hipSuccess) {
    (void)hipStreamSynchronize(S->stream);
    return fail("read-back", e);
  }
  return true;
}

bool PathFilter::Finish(Pending* p, std::vector<PathHit>* out, std::string* err) {
  out->clear();
  if (p->n == 0) return true;
  if (p->slot < 0) {
    *err = "PathFilter: nothing submitted";
    return false;
  }
  Slot* S = &slots_[p->slot];
  auto fail = [&](const char* what, hipError_t e) {
    *err = std::string("PathFilter: ") + what + ": " + hipGetErrorString(e);
    return false;
  };
  // sleep-poll (as GpuEngine::WaitEvent): a spinning wait takes a core from the host pool
  auto wait = [&]() {
    hipError_t e;
    while ((e = hipEventQuery(S->done)) == hipErrorNotReady) std::this_thread::sleep_for(std::chrono::microseconds(100));
    return e;
  };
  hipError_t e = hipSetDevice(device_);
  if (e != hipSuccess) return fail("hipSetDevice", e);
  if ((e = wait()) != hipSuccess) return fail("read-back", e);
  const uint32_t k = *S->h_cnt;
  if (k > p->n) {
    *err = "PathFilter: record count out of range";
    return false;
  }
  if (k > p->guess &&
      ((e = hipMemcpyAsync(S->h_out + p->guess, S->d_out + p->guess, size_t(k - p->guess) * sizeof(PathHit),
                           hipMemcpyDeviceToHost, S->stream)) != hipSuccess ||
       (e = hipEventRecord(S->done, S->stream)) != hipSuccess || (e = wait()) != hipSuccess))
    return fail("record read-back", e);
  last_k_.store(k);
  out->assign(S->h_out, S->h_out + k);
  return true;
}

}  // namespace tsg
