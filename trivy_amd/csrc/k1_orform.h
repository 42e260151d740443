// K1's OR-form table row: the streaming filter's reach row of
// a byte (filter.h layout, 16 buckets, window <= 6) re-laid as slot pairs, so
// a window is an OR of independent lookups instead of a shift-or recurrence.
//
// m_s[b] is the 16-bit "not allowed" mask of slot s over the 16 buckets: bit
// 4r + q is bit 4s + q of reach[b][r].  A bucket fires at position i iff its
// bit of  m_0[b_{i-5}] | m_1[b_{i-4}] | ... | m_5[b_i]  is zero.  The row is
//   W_k[b] = m_{2k+1}[b] << 16 | m_{2k}[b]   (k = 0..2)
//   W_3[b] = 1 when b is '\n' (the newline bucket's slot-0 bit is 0), else 0
// Slots 6-7 (all-allowed carries of the shift-or form) are dropped.
// Shared by the filter kernel (device) and the debug hook (host).
#pragma once
#include <cstdint>

#include "filter.h"

namespace tsg {

TSG_HOST_DEVICE inline void OrFormRow(const uint32_t reach[4], uint32_t out[4]) {
  for (uint32_t k = 0; k < 3; k++) {
    uint32_t w = 0;
    for (uint32_t h = 0; h < 2; h++) {
      const uint32_t s = 2 * k + h;
      uint32_t m = 0;
      for (uint32_t r = 0; r < 4; r++) m |= ((reach[r] >> (4 * s)) & 0xFu) << (4 * r);
      w |= m << (16 * h);
    }
    out[k] = w;
  }
  out[3] = (~reach[3] >> 3) & 1u;  // bucket 15 = word 3, nibble lane 3, slot 0
}

}  // namespace tsg
