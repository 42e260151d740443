// Streaming prefilter tables (see filter.h).
#include "filter.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cmath>
#include <limits>
#include <cstdlib>
#include <functional>
#include <map>

#include "parallel.h"

namespace tsg {

const std::vector<double>& BytePrior() {
  static const std::vector<double> prior = [] {
    std::vector<double> f(256, 1e-6);
    static const double en[26] = {8.2, 1.5, 2.8, 4.3, 12.7, 2.2, 2.0, 6.1, 7.0, 0.15, 0.8, 4.0, 2.4,
                                  6.7, 7.5, 1.9, 0.1, 6.0, 6.3, 9.1, 2.8, 1.0, 2.4, 0.15, 2.0, 0.07};
    double tot = 0;
    for (double x : en) tot += x;
    for (int i = 0; i < 26; i++) {
      f['a' + i] = 0.50 * en[i] / tot;
      f['A' + i] = 0.06 * en[i] / tot;
    }
    for (int d = '0'; d <= '9'; d++) f[d] = 0.006;
    for (int c = 0x21; c < 0x7F; c++)
      if (f[c] < 1e-4) f[c] = 0.001;
    f[' '] = 0.14;
    f['\n'] = 0.025;
    f['\t'] = 0.005;
    const std::pair<char, double> punct[] = {{'_', 0.015}, {'.', 0.012}, {',', 0.008}, {'"', 0.01}, {'\'', 0.006},
                                             {'(', 0.008}, {')', 0.008}, {'=', 0.008}, {':', 0.006}, {'-', 0.006},
                                             {'/', 0.005}, {';', 0.004}, {'{', 0.003}, {'}', 0.003}, {'[', 0.002},
                                             {']', 0.002}};
    for (auto& p : punct) f[uint8_t(p.first)] = p.second;
    for (int b = 0x80; b < 0x100; b++) f[b] = 1e-4;
    double s = 0;
    for (double x : f) s += x;
    for (double& x : f) x /= s;
    return f;
  }();
  return prior;
}

namespace {

// 256-bit byte set as four words (the clustering's working type).
struct B256 {
  uint64_t w[4];
  void set_all() { w[0] = w[1] = w[2] = w[3] = ~uint64_t(0); }
  bool test(int b) const { return (w[b >> 6] >> (b & 63)) & 1; }
  bool all() const { return (w[0] & w[1] & w[2] & w[3]) == ~uint64_t(0); }
};
B256 ToB256(const ByteSet& s) {
  B256 r{};
  for (int b = 0; b < 256; b++)
    if (s.test(size_t(b))) r.w[b >> 6] |= uint64_t(1) << (b & 63);
  return r;
}

// T[g * 256 + m] = prior mass of mask m over bytes 8g..8g+7
std::vector<double> PriorTable(const std::vector<double>& f) {
  std::vector<double> t(32 * 256, 0.0);
  for (int g = 0; g < 32; g++)
    for (int m = 0; m < 256; m++)
      for (int k = 0; k < 8; k++)
        if ((m >> k) & 1) t[size_t(g) * 256 + size_t(m)] += f[size_t(8 * g + k)];
  return t;
}

// The prior of the BuildFilter / ItemWindow call running on this thread: the
// static one, or a calibration sample's byte frequencies (CompileOptions).
thread_local const std::vector<double>* t_prior_table = nullptr;

struct PriorScope {
  std::vector<double> table;
  const std::vector<double>* saved;
  explicit PriorScope(const std::vector<double>* prior) : saved(t_prior_table) {
    if (prior) {
      table = PriorTable(*prior);
      t_prior_table = &table;
    }
  }
  ~PriorScope() { t_prior_table = saved; }
};

// P(byte in s) under the prior table T: 32 lookups of 8-byte groups.
double SetProbT(const B256& s, const std::vector<double>& T) {
  if (s.all()) return 1.0;
  double p = 0;
  for (int g = 0; g < 32; g++) p += T[size_t(g) * 256 + ((s.w[g >> 3] >> (8 * (g & 7))) & 0xFF)];
  return std::min(p, 1.0);
}
double SetProb(const B256& s) {
  static const std::vector<double> T_static = PriorTable(BytePrior());
  return SetProbT(s, t_prior_table ? *t_prior_table : T_static);
}

struct Cluster {
  B256 u[kFilterSlots];
  std::vector<uint32_t> members;
  double cost = 0;
};

// Window probability under the prior, with runs of one repeated non-letter
// byte rated as runs: text repeats punctuation and digits ("-----", "=====",
// "0000"), so each further copy of the same single byte counts as at least
// kRepeatProb instead of the independent byte's probability.
constexpr double kRepeatProb = 0.3;
bool SameSingleNonLetter(const B256& a, const B256& b) {
  int n = 0, x = -1;
  for (int k = 0; k < 4; k++) {
    if (a.w[k] != b.w[k]) return false;
    n += __builtin_popcountll(a.w[k]);
    if (a.w[k]) x = 64 * k + __builtin_ctzll(a.w[k]);
  }
  return n == 1 && !((x | 0x20) >= 'a' && (x | 0x20) <= 'z');
}
double WindowProb(const B256* u, int n) {
  double c = 1.0;
  for (int s = 0; s < n; s++) {
    double p = SetProb(u[s]);
    if (s > 0 && SameSingleNonLetter(u[s], u[s - 1])) p = std::max(p, kRepeatProb);
    c *= p;
  }
  return c;
}

double Cost(const B256* u) { return WindowProb(u, kFilterSlots); }  // unused slots stay "any" (P = 1)

// ---- clustering by measurement on a calibration sample ----
//
// Over a prefix of the sample every byte class has a bit column (bit t: byte
// t is in the class).  Slot s of a window is its class's column delayed by
// window - 1 - s positions, a bucket's slot the OR of its members', and the
// bucket's measured fires the popcount of the AND over the slots: what K1
// would flag on the prefix.  A bucket costs
//   (fires + lambda * positions * prod_s P(slot union)) * ceil(items / 8)
// -- the product under the sample's byte frequencies regularises the rare
// counts, the factor is K2's core-group lookups per fire (phase B).
constexpr uint64_t kCalibPrefixBytes = 2u << 20;  // bytes of the sample the columns cover
constexpr double kCalibLambda = 0.03;             // weight of the prior term
using Col = std::vector<uint64_t>;
struct SlotCol {
  const uint64_t* p;
  unsigned sh;
};
inline uint64_t Ld(const SlotCol& c, size_t w) {
  return c.sh ? (c.p[w] << c.sh) | (w ? c.p[w - 1] >> (64 - c.sh) : 0) : c.p[w];
}
// Words [w0, w0 + cnt) of a column, cnt <= kColBlock: in place, or shifted into buf.
constexpr size_t kColBlock = 256;
inline const uint64_t* LdBlock(const SlotCol& c, size_t w0, size_t cnt, uint64_t* buf) {
  if (!c.sh) return c.p + w0;
  size_t k = 0;
  if (w0 == 0) {
    buf[0] = c.p[0] << c.sh;
    k = 1;
  }
  const unsigned sh = c.sh, rs = 64 - c.sh;
  const uint64_t* p = c.p + w0;
  for (; k < cnt; k++) buf[k] = (p[k] << sh) | (p[k - 1] >> rs);
  return buf;
}
inline uint64_t PopBlock(const uint64_t* v, size_t cnt) {
  uint64_t n = 0;
  for (size_t k = 0; k < cnt; k++) n += uint64_t(__builtin_popcountll(v[k]));
  return n;
}

struct Win {  // one window of one item
  size_t start = 0, len = 0;
  SlotCol c[kFilterSlots];
  B256 u[kFilterSlots];
};

struct Calib {
  uint32_t S = 0;
  size_t words = 0;
  double n_pos = 0, lambda = 0;
  std::vector<double> ptab;  // PriorTable of the sample's (smoothed) byte frequencies
  std::vector<Col> base;     // per class
  std::vector<B256> cls_set;
  Col ones;
  int threads = 1;
  bool static_reg = false;

  double Reg(const B256* u) const {
    if (static_reg) return lambda * n_pos * WindowProb(u, int(S));
    double p = lambda * n_pos;
    for (uint32_t s = 0; s < S; s++) p *= SetProbT(u[s], ptab);
    return p;
  }
  static double Groups(size_t k) { return double((k + 7) / 8); }
  double Obj(uint64_t fires, const B256* u, size_t k) const { return (double(fires) + Reg(u)) * Groups(k); }

  Win MakeWin(const uint8_t* cls, size_t start, size_t len) const {
    Win w;
    w.start = start;
    w.len = len;
    for (int s = 0; s < kFilterSlots; s++) {
      w.c[s] = {ones.data(), 0};
      w.u[s].set_all();
    }
    for (size_t q = 0; q < len; q++) {
      const size_t sl = S - len + q;
      w.c[sl] = {base[cls[start + q]].data(), unsigned(S - 1 - sl)};
      w.u[sl] = cls_set[cls[start + q]];
    }
    return w;
  }
  uint64_t Fires(const SlotCol* a) const {
    uint64_t n = 0, acc[kColBlock], bx[kColBlock];
    for (size_t w0 = 0; w0 < words; w0 += kColBlock) {
      const size_t cnt = std::min(kColBlock, words - w0);
      for (size_t k = 0; k < cnt; k++) acc[k] = ~uint64_t(0);
      for (uint32_t s = 0; s < S; s++) {
        const uint64_t* x = LdBlock(a[s], w0, cnt, bx);
        for (size_t k = 0; k < cnt; k++) acc[k] &= x[k];
      }
      n += PopBlock(acc, cnt);
    }
    return n;
  }
  uint64_t PairFires(const SlotCol* a, const SlotCol* b) const {
    uint64_t n = 0, acc[kColBlock], bx[kColBlock], by[kColBlock];
    for (size_t w0 = 0; w0 < words; w0 += kColBlock) {
      const size_t cnt = std::min(kColBlock, words - w0);
      for (size_t k = 0; k < cnt; k++) acc[k] = ~uint64_t(0);
      for (uint32_t s = 0; s < S; s++) {
        const uint64_t* x = LdBlock(a[s], w0, cnt, bx);
        const uint64_t* y = LdBlock(b[s], w0, cnt, by);
        for (size_t k = 0; k < cnt; k++) acc[k] &= x[k] | y[k];
      }
      n += PopBlock(acc, cnt);
    }
    return n;
  }
};

struct MCluster {  // the greedy pass's cluster
  SlotCol c[kFilterSlots];
  std::vector<Col> own;  // a merged cluster's columns
  B256 u[kFilterSlots];
  std::vector<uint32_t> members;
  double obj = 0;
};

struct MBucket {  // the refinement's bucket: per slot the bits >= 1 and >= 2 members cover
  std::vector<uint32_t> members;
  std::vector<Col> U, U2;
  double obj = 0;
};

// Fires of bucket b without window `rem` (one of its members') and with `add`.
uint64_t FiresRemAdd(const Calib& C, const MBucket& b, const Win* rem, const Win* add) {
  uint64_t n = 0, acc[kColBlock], bx[kColBlock], by[kColBlock];
  for (size_t w0 = 0; w0 < C.words; w0 += kColBlock) {
    const size_t cnt = std::min(kColBlock, C.words - w0);
    for (size_t k = 0; k < cnt; k++) acc[k] = ~uint64_t(0);
    for (uint32_t s = 0; s < C.S; s++) {
      const uint64_t* U = b.U[s].data() + w0;
      const uint64_t* U2 = b.U2[s].data() + w0;
      const uint64_t* x = rem ? LdBlock(rem->c[s], w0, cnt, bx) : nullptr;
      const uint64_t* y = add ? LdBlock(add->c[s], w0, cnt, by) : nullptr;
      if (x && y) {
        for (size_t k = 0; k < cnt; k++) acc[k] &= U2[k] | (U[k] & ~x[k]) | y[k];
      } else if (x) {
        for (size_t k = 0; k < cnt; k++) acc[k] &= U2[k] | (U[k] & ~x[k]);
      } else if (y) {
        for (size_t k = 0; k < cnt; k++) acc[k] &= U[k] | y[k];
      } else {
        for (size_t k = 0; k < cnt; k++) acc[k] &= U[k];
      }
    }
    n += PopBlock(acc, cnt);
  }
  return n;
}
double ObjRemAdd(const Calib& C, const std::vector<Win>& win, const MBucket& b, int64_t rem, const Win* add) {
  B256 u[kFilterSlots] = {};
  size_t k = 0;
  for (uint32_t m : b.members) {
    if (int64_t(m) == rem) continue;
    k++;
    for (uint32_t s = 0; s < C.S; s++)
      for (int q = 0; q < 4; q++) u[s].w[q] |= win[m].u[s].w[q];
  }
  if (add) {
    k++;
    for (uint32_t s = 0; s < C.S; s++)
      for (int q = 0; q < 4; q++) u[s].w[q] |= add->u[s].w[q];
  }
  if (k == 0) return 0;
  return C.Obj(FiresRemAdd(C, b, rem >= 0 ? &win[size_t(rem)] : nullptr, add), u, k);
}
void Rebuild(const Calib& C, const std::vector<Win>& win, MBucket* b) {
  b->U.assign(C.S, Col(C.words, 0));
  b->U2.assign(C.S, Col(C.words, 0));
  for (uint32_t m : b->members)
    for (uint32_t s = 0; s < C.S; s++) {
      uint64_t* U = b->U[s].data();
      uint64_t* U2 = b->U2[s].data();
      for (size_t w = 0; w < C.words; w++) {
        const uint64_t x = Ld(win[m].c[s], w);
        U2[w] |= U[w] & x;
        U[w] |= x;
      }
    }
  b->obj = ObjRemAdd(C, win, *b, -1, nullptr);
}

// sample -> per-item windows (*wstart, *wlen) and the bucket member lists.
// may_share(i, j): the two items may sit in one bucket; fixed[i]: the item
// keeps a bucket of its own.  Every parallel step writes per-index results
// that are reduced in index order, so the outcome is the same on any number
// of threads.
void MeasuredBuckets(const std::vector<FilterItem>& uniq, const std::vector<uint8_t>& item_cls,
                     const std::vector<uint32_t>& cls_off, const std::vector<ByteSet>& classes, uint32_t S,
                     uint32_t n_item_buckets, const uint8_t* sample, uint64_t sample_n,
                     const std::function<bool(size_t, size_t)>& may_share, const std::vector<bool>& fixed,
                     std::vector<size_t>* wstart, std::vector<size_t>* wlen, std::vector<std::vector<uint32_t>>* buckets) {
  const size_t n = uniq.size();
  Calib C;
  C.S = S;
  const bool debug = std::getenv("TSG_CALIB_DEBUG") != nullptr;
  auto t0 = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (!debug) return;
    const auto t1 = std::chrono::steady_clock::now();
    std::fprintf(stderr, "calib buckets: %s %.3f s\n", what, std::chrono::duration<double>(t1 - t0).count());
    t0 = t1;
  };
  uint64_t prefix = kCalibPrefixBytes;
  if (const char* e = std::getenv("TSG_CALIB_PREFIX_KB")) prefix = uint64_t(std::atoll(e)) << 10;  // tuning
  const uint64_t N = std::min<uint64_t>(sample_n, std::max<uint64_t>(prefix, 64));
  C.words = size_t((N + 63) / 64);
  C.n_pos = double(N);
  C.lambda = kCalibLambda;
  if (const char* e = std::getenv("TSG_CALIB_LAMBDA")) C.lambda = std::atof(e);  // tuning
  if (const char* e = std::getenv("TSG_CALIB_REG")) C.static_reg = std::atoi(e) == 1;  // tuning
  C.threads = 16;
  if (const char* e = std::getenv("TSG_COMPILE_THREADS")) C.threads = std::max(1, std::atoi(e));
  {  // byte frequencies of the whole sample, smoothed by the static prior
    std::vector<uint64_t> h(256, 0);
    for (uint64_t i = 0; i < sample_n; i++) h[sample[i]]++;
    const double K = 65536.0;
    std::vector<double> f(256);
    for (int b = 0; b < 256; b++) f[size_t(b)] = (double(h[size_t(b)]) + K * BytePrior()[size_t(b)]) / (double(sample_n) + K);
    C.ptab = PriorTable(f);
  }
  C.ones.assign(C.words, ~uint64_t(0));
  C.base.assign(classes.size(), Col());
  C.cls_set.resize(classes.size());
  ParallelFor(classes.size(), C.threads, [&](size_t k) {
    C.cls_set[k] = ToB256(classes[k]);
    uint8_t in[256];
    for (int b = 0; b < 256; b++) in[b] = classes[k].test(size_t(b)) ? 1 : 0;
    Col& col = C.base[k];
    col.assign(C.words, 0);
    for (uint64_t t = 0; t < N; t++) col[size_t(t >> 6)] |= uint64_t(in[sample[t]]) << (t & 63);
  });
  lap("columns");
  const bool measure_windows = !std::getenv("TSG_CALIB_WINDOWS") || std::atoi(std::getenv("TSG_CALIB_WINDOWS")) != 0;
  // windows: the candidate with the lowest cost as a bucket of its own; ties go
  // to the prior's choice, then to the earliest
  std::vector<Win> win(n);
  std::vector<std::vector<Win>> cands(n);
  ParallelFor(n, C.threads, [&](size_t i) {
    const uint8_t* cls = item_cls.data() + cls_off[i];
    const size_t m = uniq[i].sets.size(), wl = (*wlen)[i];
    win[i] = C.MakeWin(cls, (*wstart)[i], wl);
    if (!measure_windows) return;
    double best = C.Obj(C.Fires(win[i].c), win[i].u, 1);
    for (size_t s = 0; s + wl <= m; s++) {
      cands[i].push_back(C.MakeWin(cls, s, wl));
      if (s == (*wstart)[i]) continue;
      const double o = C.Obj(C.Fires(cands[i].back().c), cands[i].back().u, 1);
      if (o < best) {
        best = o;
        win[i] = cands[i].back();
      }
    }
  });
  lap("windows");
  // greedy agglomeration by the measured increase of the cost
  std::vector<MCluster> mc(n);
  for (size_t i = 0; i < n; i++) {
    for (int s = 0; s < kFilterSlots; s++) {
      mc[i].c[s] = win[i].c[s];
      mc[i].u[s] = win[i].u[s];
    }
    mc[i].members = {uint32_t(i)};
  }
  ParallelFor(n, C.threads, [&](size_t i) { mc[i].obj = C.Obj(C.Fires(mc[i].c), mc[i].u, 1); });
  const double kInf = std::numeric_limits<double>::infinity();
  std::vector<bool> alive(n, true);
  auto cluster_ok = [&](size_t i, size_t j) {
    for (uint32_t a : mc[i].members)
      for (uint32_t b : mc[j].members)
        if (fixed[a] || fixed[b] || !may_share(a, b)) return false;
    return true;
  };
  auto delta_of = [&](size_t i, size_t j) {
    if (!cluster_ok(i, j)) return kInf;
    B256 u[kFilterSlots];
    for (int s = 0; s < kFilterSlots; s++)
      for (int k = 0; k < 4; k++) u[s].w[k] = mc[i].u[s].w[k] | mc[j].u[s].w[k];
    return C.Obj(C.PairFires(mc[i].c, mc[j].c), u, mc[i].members.size() + mc[j].members.size()) - mc[i].obj - mc[j].obj;
  };
  std::vector<double> delta(n > 1 ? n * n : 1, 0.0);
  ParallelFor(n, C.threads, [&](size_t i) {
    for (size_t j = i + 1; j < n; j++) delta[i * n + j] = delta_of(i, j);
  });
  for (size_t i = 0; i < n; i++)
    for (size_t j = i + 1; j < n; j++) delta[j * n + i] = delta[i * n + j];
  size_t n_alive = n;
  while (n_alive > n_item_buckets) {
    size_t bi = 0, bj = 0;
    double bd = kInf;
    for (size_t i = 0; i < n; i++)
      for (size_t j = i + 1; j < n; j++)
        if (alive[i] && alive[j] && delta[i * n + j] < bd) {
          bd = delta[i * n + j];
          bi = i;
          bj = j;
        }
    if (bd == kInf) break;  // (the caller reports it)
    std::vector<Col> own(S, Col(C.words));
    for (uint32_t s = 0; s < S; s++)
      for (size_t w = 0; w < C.words; w++) own[s][w] = Ld(mc[bi].c[s], w) | Ld(mc[bj].c[s], w);
    mc[bi].own.swap(own);
    for (uint32_t s = 0; s < S; s++) {
      mc[bi].c[s] = {mc[bi].own[s].data(), 0};
      for (int k = 0; k < 4; k++) mc[bi].u[s].w[k] |= mc[bj].u[s].w[k];
    }
    mc[bi].members.insert(mc[bi].members.end(), mc[bj].members.begin(), mc[bj].members.end());
    mc[bi].obj = C.Obj(C.Fires(mc[bi].c), mc[bi].u, mc[bi].members.size());
    mc[bj].own.clear();
    alive[bj] = false;
    n_alive--;
    ParallelFor(n, C.threads, [&](size_t k) {
      if (!alive[k] || k == bi) return;
      delta[k * n + bi] = delta[bi * n + k] = delta_of(bi, k);
    });
  }
  lap("greedy");
  // refinement: single items moved, an item's window reconsidered inside its
  // bucket (once), pairs swapped, while the total cost falls.  A step applies
  // the best changes that touch disjoint buckets, so each one's gain is exact.
  std::vector<MBucket> bk;
  std::vector<uint32_t> bof(n, 0);
  for (size_t i = 0; i < n; i++)
    if (alive[i]) {
      for (uint32_t m : mc[i].members) bof[m] = uint32_t(bk.size());
      bk.emplace_back();
      bk.back().members = mc[i].members;
    }
  mc.clear();
  ParallelFor(bk.size(), C.threads, [&](size_t b) { Rebuild(C, win, &bk[b]); });
  struct Change {
    double d = 0;
    uint32_t x = 0, y = 0xFFFFFFFFu, to = 0;  // item x to bucket `to` (y: the item that comes back)
    size_t cand = size_t(-1);                 // or: x takes its candidate window `cand`
  };
  const bool refine = !std::getenv("TSG_CALIB_REFINE") || std::atoi(std::getenv("TSG_CALIB_REFINE")) != 0;
  bool windows_done = !measure_windows;
  auto movable = [&](size_t x, size_t b) {
    if (fixed[x]) return false;
    for (uint32_t m : bk[b].members)
      if (m != x && (fixed[m] || !may_share(x, m))) return false;
    return true;
  };
  std::vector<double> mcost(n * bk.size(), 0.0), mgain(n, 0.0);
  std::vector<uint32_t> mcost_v(n * bk.size(), 0), mgain_v(n, 0);  // the bucket versions the kept values saw
  std::vector<uint32_t> bver(bk.size(), 1), sw_b(n, 0xFFFFFFFFu), sw_va(n, 0), sw_vb(n, 0);
  std::vector<Change> sw_ch(n);
  int n_rounds = 0, n_changes[3] = {0, 0, 0};
  for (int round = 0; refine && round < 400; round++) {
    n_rounds++;
    double total = 0;
    for (auto& b : bk) total += b.obj;
    const double eps = 1e-9 * (total + 1.0);
    std::vector<Change> ch(n);
    std::vector<uint32_t> pref(n, 0xFFFFFFFFu);  // the bucket that takes x at the lowest cost
    auto apply = [&](int phase) {
      std::vector<size_t> order;
      for (size_t i = 0; i < n; i++)
        if (ch[i].d < -eps) order.push_back(i);
      std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return ch[a].d != ch[b].d ? ch[a].d < ch[b].d : a < b; });
      std::vector<bool> touched(bk.size(), false);
      std::vector<size_t> dirty;
      for (size_t i : order) {
        const Change& c = ch[i];
        const uint32_t A = bof[c.x], B = phase == 1 ? A : c.to;
        if (touched[A] || touched[B]) continue;
        touched[A] = touched[B] = true;
        bver[A]++;
        if (B != A) bver[B]++;
        n_changes[phase]++;
        dirty.push_back(A);
        if (phase == 1) {
          for (size_t b = 0; b < bk.size(); b++) mcost_v[c.x * bk.size() + b] = 0;
          win[c.x] = cands[c.x][c.cand];
          continue;
        }
        dirty.push_back(B);
        auto& ma = bk[A].members;
        ma.erase(std::find(ma.begin(), ma.end(), c.x));
        bk[B].members.push_back(c.x);
        bof[c.x] = B;
        if (phase == 2) {
          auto& mb = bk[B].members;
          mb.erase(std::find(mb.begin(), mb.end(), c.y));
          ma.push_back(c.y);
          bof[c.y] = A;
        }
      }
      ParallelFor(dirty.size(), C.threads, [&](size_t k) { Rebuild(C, win, &bk[dirty[k]]); });
      return !dirty.empty();
    };
    // moves (what a bucket charges for an item is kept until the bucket or the item's window changes)
    ParallelFor(n, C.threads, [&](size_t x) {
      const uint32_t A = bof[x];
      if (fixed[x] || bk[A].members.size() < 2) return;
      if (mgain_v[x] != bver[A]) {
        mgain[x] = bk[A].obj - ObjRemAdd(C, win, bk[A], int64_t(x), nullptr);
        mgain_v[x] = bver[A];
      }
      const double gain = mgain[x];
      double best = kInf;
      for (uint32_t B = 0; B < bk.size(); B++) {
        if (B == A || !movable(x, B)) continue;
        if (mcost_v[x * bk.size() + B] != bver[B]) {
          mcost[x * bk.size() + B] = ObjRemAdd(C, win, bk[B], -1, &win[x]) - bk[B].obj;
          mcost_v[x * bk.size() + B] = bver[B];
        }
        const double cost = mcost[x * bk.size() + B];
        if (cost < best) {
          best = cost;
          pref[x] = B;
        }
      }
      if (pref[x] != 0xFFFFFFFFu) {
        ch[x].d = best - gain;
        ch[x].x = uint32_t(x);
        ch[x].to = pref[x];
      }
    });
    if (apply(0)) continue;
    if (!windows_done) {  // an item's other windows, inside its bucket
      windows_done = true;
      ch.assign(n, Change());
      ParallelFor(n, C.threads, [&](size_t x) {
        const MBucket& A = bk[bof[x]];
        for (size_t k = 0; k < cands[x].size(); k++) {
          if (cands[x][k].start == win[x].start) continue;
          const double d = ObjRemAdd(C, win, A, int64_t(x), &cands[x][k]) - A.obj;
          if (d < ch[x].d) {
            ch[x].d = d;
            ch[x].x = uint32_t(x);
            ch[x].cand = k;
          }
        }
      });
      if (apply(1)) continue;
    }
    // swaps of x with a member of the bucket that takes it at the lowest cost
    // (an item's best swap is kept while neither bucket has changed)
    ch.assign(n, Change());
    ParallelFor(n, C.threads, [&](size_t x) {
      const uint32_t A = bof[x], B = pref[x];
      if (B == 0xFFFFFFFFu) return;
      if (sw_b[x] == B && sw_va[x] == bver[A] && sw_vb[x] == bver[B]) {
        ch[x] = sw_ch[x];
        return;
      }
      sw_b[x] = B;
      sw_va[x] = bver[A];
      sw_vb[x] = bver[B];
      sw_ch[x] = Change();
      for (uint32_t y : bk[B].members) {
        if (fixed[y]) continue;
        bool ok = true;
        for (uint32_t m : bk[A].members)
          if (m != x && !may_share(y, m)) ok = false;
        for (uint32_t m : bk[B].members)
          if (m != y && !may_share(x, m)) ok = false;
        if (!ok) continue;
        const double d = ObjRemAdd(C, win, bk[A], int64_t(x), &win[y]) + ObjRemAdd(C, win, bk[B], int64_t(y), &win[x]) -
                         bk[A].obj - bk[B].obj;
        if (d < ch[x].d) {
          ch[x].d = d;
          ch[x].x = uint32_t(x);
          ch[x].y = y;
          ch[x].to = B;
        }
      }
      sw_ch[x] = ch[x];
    });
    if (!apply(2)) break;
  }
  lap("refinement");
  if (debug)
    std::fprintf(stderr, "calib buckets: %d rounds, %d moves, %d windows, %d swaps\n", n_rounds, n_changes[0], n_changes[1],
                 n_changes[2]);
  for (size_t i = 0; i < n; i++) {
    (*wstart)[i] = win[i].start;
    (*wlen)[i] = win[i].len;
  }
  buckets->clear();
  for (auto& b : bk) {
    std::sort(b.members.begin(), b.members.end());
    buckets->push_back(b.members);
  }
  std::sort(buckets->begin(), buckets->end());  // by lowest member
}

}  // namespace

void ItemWindow(const FilterItem& it, uint32_t window, size_t* start, size_t* len, const std::vector<double>* prior) {
  PriorScope scope(prior);
  const size_t m = it.sets.size();
  size_t w = 0, wl = std::min<size_t>(m, window);
  double best = std::numeric_limits<double>::infinity();
  for (size_t s = 0; s + wl <= m; s++) {
    B256 win[kFilterSlots];
    for (size_t q = s; q < s + wl; q++) win[q - s] = ToB256(it.sets[q]);
    const double c = WindowProb(win, int(wl));
    if (c < best) {
      best = c;
      w = s;
    }
  }
  *start = w;
  *len = wl;
}

bool BuildFilter(const std::vector<FilterItem>& items, uint32_t window, uint32_t n_buckets, FilterTables* out,
                 std::string* err, const std::vector<double>* prior, const uint8_t* sample, uint64_t sample_n) {
  PriorScope scope(prior);
  if ((n_buckets != 8 && n_buckets != 16) || window < 2 || window > uint32_t(kFilterSlots)) {
    *err = "unsupported prefilter shape";
    return false;
  }
  *out = FilterTables();
  out->n_buckets = n_buckets;
  out->n_words = n_buckets / 4;
  out->window = window;
  out->nl_bucket = n_buckets - 1;
  const uint32_t n_item_buckets = n_buckets - 1;
  const uint32_t S = window;
  // identical byte-set sequences (rules sharing an anchor) become one item
  std::vector<FilterItem> uniq;
  std::vector<std::vector<uint32_t>> ids;
  {
    std::map<std::string, size_t> seen;
    for (auto& it : items) {
      std::string key(1, char(it.kind));
      key += char('0' + it.group);
      key += std::to_string(it.lit_end) + ":";
      for (auto& b : it.sets) key += b.to_string();
      auto f = seen.find(key);
      if (f != seen.end() && ids[f->second].size() < 255) {
        ids[f->second].push_back(it.id);
        continue;
      }
      seen[key] = uniq.size();
      uniq.push_back(it);
      ids.push_back({it.id});
    }
  }
  const size_t n = uniq.size();
  // classes (deduplicated byte sets) and per-item windows
  std::map<std::string, uint32_t> cls_ids;
  std::vector<ByteSet> classes;
  std::vector<Cluster> cl(n);
  std::vector<size_t> wstart(n, 0), wlen(n, 0);
  std::vector<uint32_t> cls_off(n, 0);
  for (size_t i = 0; i < n; i++) {
    const FilterItem& it = uniq[i];
    if (it.sets.empty() || it.sets.size() > 0xFFFF) {
      *err = "prefilter item with no (or too many) positions";
      return false;
    }
    const size_t m = it.sets.size();
    // least frequent window of <= kFilterSlots positions
    size_t w = 0, wl = 0;
    ItemWindow(it, S, &w, &wl, nullptr);  // (under this call's prior)
    wstart[i] = w;
    wlen[i] = wl;
    cls_off[i] = uint32_t(out->item_cls.size());
    for (int s = 0; s < kFilterSlots; s++) cl[i].u[s].set_all();
    for (size_t q = 0; q < wl; q++) cl[i].u[S - wl + q] = ToB256(it.sets[w + q]);
    cl[i].members = {uint32_t(i)};
    cl[i].cost = Cost(cl[i].u);
    FilterItemGpu g{};
    g.n = uint16_t(m);
    g.back = uint16_t(w + wl);
    g.lit_end = uint16_t(it.lit_end);
    g.kind = it.kind;
    g.n_ids = uint8_t(ids[i].size());
    g.ids_off = uint32_t(out->item_ids.size());
    out->item_ids.insert(out->item_ids.end(), ids[i].begin(), ids[i].end());
    g.cls_off = uint32_t(out->item_cls.size());
    out->max_after = std::max<uint32_t>(out->max_after, uint32_t(m - (w + wl)));
    for (auto& b : it.sets) {
      std::string key = b.to_string();
      auto f = cls_ids.find(key);
      uint32_t id;
      if (f == cls_ids.end()) {
        id = uint32_t(classes.size());
        if (id >= 256) {
          *err = "prefilter needs more than 256 distinct byte classes";
          return false;
        }
        cls_ids[key] = id;
        classes.push_back(b);
      } else {
        id = f->second;
      }
      out->item_cls.push_back(uint8_t(id));
    }
    out->items.push_back(g);
  }
  // agglomerative clustering down to n_buckets: always merge the pair whose
  // union adds the least estimated fire rate.  Each row caches its best
  // partner; after a merge only rows whose partner died are rescanned
  // (O(n^2) in practice instead of a full O(n^2) scan per merge).
  std::vector<bool> alive(n, true);
  size_t n_alive = n;
  auto merged = [&](const Cluster& a, const Cluster& b, B256* u) {
    for (int s = 0; s < kFilterSlots; s++)
      for (int k = 0; k < 4; k++) u[s].w[k] = a.u[s].w[k] | b.u[s].w[k];
    return Cost(u);
  };
  std::vector<bool> solo(n, false);
  if (const char* e = std::getenv("TSG_FILTER_SOLO")) {  // experiment: items kept in buckets of their own
    for (const char* q = e; *q;) {
      char* end = nullptr;
      const unsigned long v = std::strtoul(q, &end, 10);
      if (end == q) break;
      if (v < n) solo[v] = true;
      q = *end ? end + 1 : end;
    }
  }
  auto delta_of = [&](size_t i, size_t j) {
    if (solo[i] || solo[j] || uniq[i].group != uniq[j].group) return std::numeric_limits<double>::infinity();
    B256 u[kFilterSlots];
    return merged(cl[i], cl[j], u) - cl[i].cost - cl[j].cost;
  };
  std::vector<double> delta(n > 1 ? n * n : 1, 0.0);  // symmetric, rows of n
  for (size_t i = 0; i < n; i++)
    for (size_t j = i + 1; j < n; j++) delta[i * n + j] = delta[j * n + i] = delta_of(i, j);
  const double kInf = std::numeric_limits<double>::infinity();
  std::vector<size_t> best(n, 0);
  std::vector<double> best_d(n, kInf);
  auto rescan = [&](size_t i) {
    best_d[i] = kInf;
    for (size_t j = 0; j < n; j++)
      if (j != i && alive[j] && delta[i * n + j] < best_d[i]) {
        best_d[i] = delta[i * n + j];
        best[i] = j;
      }
  };
  for (size_t i = 0; i < n; i++) rescan(i);
  // With a calibration sample the windows and the buckets come from measured
  // fires instead (MeasuredBuckets above).  Builtin-sized rule sets only: the
  // columns and the pair matrix grow with the items, and large sets confirm by
  // the window hash, whose cost the core-group factor does not describe.
  const bool measured = sample && sample_n >= 4096 && n <= 256;
  if (measured) {
    std::vector<std::vector<uint32_t>> buckets;
    const char* ge = std::getenv("TSG_CALIB_GROUPS");  // 1: FilterItem::group splits the measured buckets too (A/B)
    const bool keep_groups = ge && std::atoi(ge) != 0;
    MeasuredBuckets(uniq, out->item_cls, cls_off, classes, S, n_item_buckets, sample, sample_n,
                    [&](size_t a, size_t b) { return !keep_groups || uniq[a].group == uniq[b].group; }, solo, &wstart,
                    &wlen, &buckets);
    if (buckets.size() > n_item_buckets) {
      *err = "prefilter: no bucket merge left (solo items or groups exceed the buckets)";
      return false;
    }
    out->max_after = 0;
    for (size_t i = 0; i < n; i++) {
      alive[i] = false;
      const size_t m = uniq[i].sets.size(), w = wstart[i], wl = wlen[i];
      for (int s = 0; s < kFilterSlots; s++) cl[i].u[s].set_all();
      for (size_t q = 0; q < wl; q++) cl[i].u[S - wl + q] = ToB256(uniq[i].sets[w + q]);
      out->items[i].back = uint16_t(w + wl);
      out->max_after = std::max<uint32_t>(out->max_after, uint32_t(m - (w + wl)));
    }
    for (auto& b : buckets) {
      Cluster& c = cl[b[0]];
      for (size_t k = 1; k < b.size(); k++)
        for (int s = 0; s < kFilterSlots; s++)
          for (int q = 0; q < 4; q++) c.u[s].w[q] |= cl[b[k]].u[s].w[q];
      c.members = b;
      c.cost = Cost(c.u);
      alive[b[0]] = true;
    }
    n_alive = buckets.size();
  }
  while (!measured && n_alive > n_item_buckets) {
    size_t bi = 0, bj = 0;
    double bd = kInf;
    for (size_t i = 0; i < n; i++)
      if (alive[i] && best_d[i] < bd) {
        bd = best_d[i];
        bi = i;
        bj = best[i];
      }
    if (bd == kInf) {  // (more solo items / groups than buckets)
      *err = "prefilter: no bucket merge left (solo items or groups exceed the buckets)";
      return false;
    }
    if (bj < bi) std::swap(bi, bj);
    B256 u[kFilterSlots];
    double c = merged(cl[bi], cl[bj], u);
    for (int s = 0; s < kFilterSlots; s++) cl[bi].u[s] = u[s];
    cl[bi].cost = c;
    cl[bi].members.insert(cl[bi].members.end(), cl[bj].members.begin(), cl[bj].members.end());
    alive[bj] = false;
    n_alive--;
    for (size_t k = 0; k < n; k++) {
      if (!alive[k] || k == bi) continue;
      const double d = delta_of(bi, k);
      delta[k * n + bi] = delta[bi * n + k] = d;
    }
    rescan(bi);
    for (size_t k = 0; k < n; k++) {
      if (!alive[k] || k == bi) continue;
      if (best[k] == bi || best[k] == bj) {
        rescan(k);  // its partner changed or died
      } else if (delta[k * n + bi] < best_d[k]) {
        best_d[k] = delta[k * n + bi];
        best[k] = bi;
      }
    }
  }
  // reach table
  const uint32_t W = out->n_words;
  out->reach.assign(256 * W, ~0u);
  auto allow = [&](uint32_t b, uint32_t j, uint32_t slot) { out->reach[size_t(b) * W + j / 4] &= ~(1u << (4 * slot + j % 4)); };
  out->bucket_off.push_back(0);
  uint32_t j = 0;
  for (size_t i = 0; i < n; i++) {
    if (!alive[i]) continue;
    out->est_fp += cl[i].cost;
    for (uint32_t sl = 0; sl < uint32_t(kFilterSlots); sl++)  // slots >= window: all bytes allowed (carry the fire)
      for (int b = 0; b < 256; b++)
        if (sl >= S || cl[i].u[sl].test(b)) allow(uint32_t(b), j, sl);
    for (uint32_t m : cl[i].members) out->bucket_items.push_back(m);
    out->bucket_off.push_back(uint32_t(out->bucket_items.size()));
    j++;
  }
  for (; j < n_buckets; j++) {  // empty item buckets never fire; the newline bucket allows '\n' at slot 0
    if (j == out->nl_bucket) {  // slot 0: '\n' only; slots 1-3 carry; slots 4-7 never allow (no fires)
      allow('\n', j, 0);
      for (uint32_t sl = 1; sl < 4; sl++)
        for (int b = 0; b < 256; b++) allow(uint32_t(b), j, sl);
    }
    out->bucket_off.push_back(uint32_t(out->bucket_items.size()));
  }
  // literal windows -> hash table (filter.h); the rest -> core groups
  std::vector<uint8_t> hashed(n, 0);
  std::vector<std::pair<uint64_t, uint32_t>> hkeys;
  const char* hash_env = std::getenv("TSG_WINDOW_HASH");  // 0: core groups only (A/B)
  // Large rule sets only: builtin-sized buckets hold 1-2 groups, whose LDS core
  // lookups beat a probe plus the full position check (C2 confirm 5.08 vs 5.35
  // ms with hashing; C3, 2,108 items: 25.0 -> 4.0 ms, profiles/r02_wl/wl_r02h_*)
  const bool use_hash = hash_env ? std::atoi(hash_env) != 0 && S == 6 : (S == 6 && n > 256);
  for (size_t i = 0; i < n && use_hash; i++) {
    const FilterItemGpu& g = out->items[i];
    if (g.back < 6) continue;
    uint64_t key = 0;
    bool ok = true;
    for (int q = 0; q < 6 && ok; q++) {
      const ByteSet& b = uniq[i].sets[size_t(g.back - 6 + q)];
      const size_t pc = b.count();
      int c = -1;
      for (int x = 0; x < 128 && pc <= 2; x++)
        if (b.test(size_t(x))) {
          c = x;
          break;
        }
      if (c < 0 || pc > 2) {
        ok = false;
        break;
      }
      for (int x = 128; x < 256; x++)
        if (b.test(size_t(x))) ok = false;
      if (pc == 2) ok = ok && c >= 'A' && c <= 'Z' && b.test(size_t(c + 32));
      const int lc = (c >= 'A' && c <= 'Z') ? c + 32 : c;
      key |= uint64_t(lc) << (8 * q);
    }
    if (!ok) continue;
    hashed[i] = 1;
    hkeys.push_back({key, uint32_t(i)});
  }
  if (!hkeys.empty()) {
    uint32_t bits = 4;
    while ((size_t(1) << bits) < 2 * hkeys.size()) bits++;
    out->hash_bits = bits;
    out->hash_keys.assign(size_t(1) << bits, 0);
    out->hash_items.assign(size_t(1) << bits, 0);
    for (auto& kv : hkeys) {
      uint32_t slot = WindowHash(kv.first, bits);
      while (out->hash_keys[slot]) slot = (slot + 1) & ((1u << bits) - 1);
      out->hash_keys[slot] = kv.first | (uint64_t(1) << 63);
      out->hash_items[slot] = kv.second;
    }
    for (uint32_t b = 0; b < n_buckets; b++)
      for (uint32_t k = out->bucket_off[b]; k < out->bucket_off[b + 1]; k++)
        if (hashed[out->bucket_items[k]]) out->hash_buckets |= 1u << b;
  }
  // core tables (filter.h), over the items not hashed
  out->bucket_groups.push_back(0);
  uint32_t n_groups = 0;
  for (uint32_t b = 0; b < n_buckets; b++) {
    std::vector<uint32_t> grp;
    for (uint32_t k = out->bucket_off[b]; k < out->bucket_off[b + 1]; k++)
      if (!hashed[out->bucket_items[k]]) grp.push_back(out->bucket_items[k]);
    const uint32_t lo = 0, hi = uint32_t(grp.size());
    for (uint32_t g0 = lo; g0 < hi; g0 += 8) {
      std::vector<uint64_t> tab(256, 0);
      for (uint32_t i = 0; i < 8; i++) {
        if (g0 + i >= hi) {
          out->group_items.push_back(0xFFFFFFFFu);
          continue;
        }
        const uint32_t item = grp[g0 + i];
        out->group_items.push_back(item);
        const FilterItem& it = uniq[item];
        const int back = out->items[item].back;
        for (int sl = 0; sl < 8; sl++) {
          const int q = back - 8 + sl;
          for (int x = 0; x < 256; x++)
            if (q < 0 || it.sets[size_t(q)].test(size_t(x))) tab[size_t(x)] |= uint64_t(1) << (8 * sl + i);
        }
      }
      out->core.insert(out->core.end(), tab.begin(), tab.end());
      n_groups++;
    }
    out->bucket_groups.push_back(n_groups);
  }
  for (auto& b : classes) {
    uint32_t w[8] = {};
    for (int x = 0; x < 256; x++)
      if (b.test(x)) w[x >> 5] |= 1u << (x & 31);
    out->classes.insert(out->classes.end(), w, w + 8);
  }
  return true;
}

}  // namespace tsg
