// Device row I/O of the int16 PCM kernels (speed.hip, noise.hip, reverb.hip, telephone.hip): eight samples at a time.  The kernels lay their tiles on the
// 16-byte grid of the OUTPUT row's address (a row may start at any even address), so every store is one aligned 16-byte store but for a
// row's first and last few samples.  The input row sits at another offset from that grid, so its eight samples come by one 16-byte load
// that is only 2-byte aligned: global memory takes it as it comes, and a wave still covers one contiguous kilobyte.
#pragma once
#include "common.h"

// samples between the 16-byte boundary at or before p and p
__device__ __forceinline__ int pcm_lead(const int16_t* p) { return (int)(((uintptr_t)p >> 1) & 7); }

// samples [i0, i0 + 8) of a row where 0 <= i < hi, zero elsewhere (row + i0 is 2-byte aligned only); I = int or long
template <class I>
__device__ __forceinline__ s16x8_t pcm_load8(const int16_t* row, I i0, int hi) {
  s16x8_t v;
  if (i0 >= 0 && i0 + 8 <= hi) {
    __builtin_memcpy(&v, row + i0, sizeof(v));
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (i0 + e >= 0 && i0 + e < hi) ? row[i0 + e] : (int16_t)0;
  }
  return v;
}

// samples [n0, n0 + 8) of a row of N as one aligned 16-byte store where all eight exist, else one by one (y + n0 is 16-byte aligned)
__device__ __forceinline__ void pcm_store8(int16_t* y, int n0, int N, s16x8_t v) {
  if (n0 >= 0 && n0 + 8 <= N) {
    *(s16x8_t*)(y + n0) = v;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (n0 + e >= 0 && n0 + e < N) y[n0 + e] = v[e];
  }
}
