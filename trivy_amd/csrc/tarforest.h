// The header chains of all layers of an image resident in HBM, walked in one
// GPU pass (tarforest.hip; tsg_analyzer_index_device_tars in walk mode 1).
// This header is plain C++: the layout of the pass's virtual block space and
// what it hands to the host half.  Per layer the pass decides exactly what the
// single-layer pass decides for that layer alone (tarchain.h); a set of layers
// is a forest of chains, one root per layer.
//
// Virtual block space.  With segments of S blocks (as in TarChainPlan), layer k
// of B_k = n_bytes_k / 512 complete blocks owns the virtual blocks
// [V_k, V_k + B_k), V_0 = 0, V_{k+1} = V_k + roundup(max(B_k, 1), S): every
// segment belongs to one layer, named by a u32 per segment, and the blocks
// between V_k + B_k and V_{k+1} are padding that is never read.  Every offset,
// bound and successor inside a layer is local to it; the bound is n_bytes_k.
// The pass takes 20 B per virtual block of HBM plus its tables.
//
// Hand-over.  A TarChainHead per layer (tarindex.h): the stop, and the entries,
// name bytes and candidates of that layer.  The 64-B records of all layers lie
// in one buffer and their raw names in another, layer after layer in walk
// order; layer k's records start at the sum of the entries of the layers before
// it, its names at the sum of their name bytes, and name_off is relative to
// that name base -- layer k's slice is what the single-layer pass writes for it.
// An INCOMPLETE layer hands nothing over (entries = name_bytes = 0).
#pragma once
#include <cstdint>
#include <vector>

#include "tarchain.h"

namespace tsg {

constexpr uint32_t kTarForestMaxLayers = 65536;

// One layer of a pass, as the kernels read it (32 B).
struct TarForestLayer {
  const uint8_t* ptr;  // 16-B aligned; blocks b < n_blocks are read, nothing else
  uint64_t n_bytes;
  uint64_t n_blocks;   // n_bytes / 512
  uint64_t v0;         // V_k, a multiple of the segment size
};
static_assert(sizeof(TarForestLayer) == 32, "two 16-B words");

// The virtual blocks a layer of n_bytes takes with segments of `seg` blocks.
inline uint64_t TarForestSpan(uint64_t n_bytes, uint32_t seg) {
  const uint64_t b = n_bytes / 512 ? n_bytes / 512 : 1;
  return (b + seg - 1) / seg * seg;
}

// How many of the layers from `first` on fit one pass: their spans stay below
// kTarMaxBlocks - 2.  0: layer `first` alone does not fit (kTarTooLarge).
inline uint32_t TarForestCut(const uint64_t* n_bytes, uint32_t n_layers, uint32_t first, uint32_t seg) {
  uint64_t v = 0;
  uint32_t k = first;
  for (; k < n_layers; k++) {
    if (n_bytes[k] / 512 >= kTarMaxBlocks) break;
    const uint64_t span = TarForestSpan(n_bytes[k], seg);
    if (v + span + 2 >= kTarMaxBlocks) break;
    v += span;
  }
  return k - first;
}

// Record and name bases of the layers from their heads' counts: base[k] is the
// sum over the layers before k; base[n] the total.
inline void TarForestBases(const uint64_t* counts, size_t stride_words, uint32_t n, std::vector<uint64_t>* base) {
  base->assign(size_t(n) + 1, 0);
  for (uint32_t k = 0; k < n; k++) (*base)[k + 1] = (*base)[k] + counts[size_t(k) * stride_words];
}

}  // namespace tsg
