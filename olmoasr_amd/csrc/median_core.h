// Median of W values (W odd, <= 15) held in registers, by fixed compare-exchange networks: no data-dependent branch, no indexing by
// a runtime value.  W = 7 (whisper's median filter width) is the 13-exchange selection network; W = 3 is three exchanges; the other
// widths run an odd-even transposition sort, W rounds of neighbour exchanges.  Plain C++ so that a host program can check the networks
// exhaustively (0/1 principle: a network that selects the median of every 0/1 input selects it for every input).
#pragma once
#include "core_hd.h"

OASR_HD void med_cx(float& a, float& b) {  // a <= b afterwards
  const float lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo;
  b = hi;
}

template <int W>
OASR_HD float median_net(float (&p)[W]) {
  static_assert(W % 2 == 1 && W >= 1 && W <= 15, "odd widths up to 15");
  if (W == 1) return p[0];
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int r = 0; r < W; ++r) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = r & 1; k + 1 < W; k += 2) med_cx(p[k], p[k + 1]);
  }
  return p[W / 2];
}
template <>
OASR_HD float median_net<3>(float (&p)[3]) {
  med_cx(p[0], p[1]);
  med_cx(p[1], p[2]);
  med_cx(p[0], p[1]);
  return p[1];
}
template <>
OASR_HD float median_net<7>(float (&p)[7]) {
  med_cx(p[0], p[5]);
  med_cx(p[0], p[3]);
  med_cx(p[1], p[6]);
  med_cx(p[2], p[4]);
  med_cx(p[0], p[1]);
  med_cx(p[3], p[5]);
  med_cx(p[2], p[6]);
  med_cx(p[2], p[3]);
  med_cx(p[3], p[6]);
  med_cx(p[4], p[5]);
  med_cx(p[1], p[4]);
  med_cx(p[1], p[3]);
  med_cx(p[3], p[4]);
  return p[3];
}
