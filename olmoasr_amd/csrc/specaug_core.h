// SpecAugment's mask rule (include/oasr.h at oasr_spec_augment): the ONE text that the device kernel (specaug.hip) and the host twin
// (specaug_host.cpp, oasr_spec_augment_plan) share, so that a plan computed on the CPU is the plan the kernel applies, bit for bit.
// Plain C++: no HIP header is needed to include this file.
//
// Everything is unsigned 64-bit integer arithmetic with wrap-around; no floating point enters a plan.  A clip's masks are a pure function
// of (seed, clip stream id, policy, shape): they do not depend on the batch the clip sits in or on how many calls came before.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SPECAUG_HD __host__ __device__ __forceinline__
#else
#define SPECAUG_HD inline
#endif

#define SPECAUG_MAX_MASKS 8  // == OASR_SPECAUG_MAX_MASKS (include/oasr.h), per kind
enum { SPECAUG_FREQ = 1, SPECAUG_TIME = 2 };

// splitmix64's finalizer on z + golden ratio
SPECAUG_HD uint64_t specaug_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the per-clip key every interval of that clip is drawn from
SPECAUG_HD uint64_t specaug_clip_hash(uint64_t seed, uint64_t clip) { return specaug_mix(specaug_mix(seed) ^ clip); }

// mask i of `kind` along an axis of length L >= 1 with policy width W >= 0: [*start, *start + *width), width in [0, min(W, L)],
// start in [0, L - width]
SPECAUG_HD void specaug_interval(uint64_t h, int kind, int i, int W, int L, int* start, int* width) {
  const uint64_t w = (uint64_t)(W < L ? W : L);
  const uint64_t tag = ((uint64_t)kind << 16) | ((uint64_t)i << 1);
  const uint64_t width_ = specaug_mix(h ^ tag) % (w + 1);
  *width = (int)width_;
  *start = (int)(specaug_mix(h ^ (tag | 1)) % ((uint64_t)L - width_ + 1));
}

// what is wrong with a policy's counts and widths, or nullptr
SPECAUG_HD const char* specaug_policy_error(int freq_masks, int freq_width, int time_masks, int time_width) {
  if (freq_masks < 0 || time_masks < 0) return "a negative mask count";
  if (freq_masks > SPECAUG_MAX_MASKS || time_masks > SPECAUG_MAX_MASKS) return "more than OASR_SPECAUG_MAX_MASKS (8) masks of one kind";
  if (freq_width < 0 || time_width < 0) return "a negative mask width";
  return nullptr;
}
