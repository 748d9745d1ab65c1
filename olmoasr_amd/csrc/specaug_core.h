// SpecAugment's mask rule (include/oasr.h at oasr_spec_augment): the ONE text that the device kernel (specaug.hip) and the host twin
// (specaug_host.cpp, oasr_spec_augment_plan) share, so that a plan computed on the CPU is the plan the kernel applies, bit for bit.
// Plain C++: no HIP header is needed to include this file.
//
// A clip's masks are a pure function of (seed, clip stream id, policy, shape), drawn from the clip's stream (draw_core.h) under the kinds
// DRAW_FREQ_MASK and DRAW_TIME_MASK.
#pragma once
#include <stdint.h>

#include "draw_core.h"

#define SPECAUG_MAX_MASKS 8  // == OASR_SPECAUG_MAX_MASKS (include/oasr.h), per kind

// mask i of `kind` along an axis of length L >= 1 with policy width W >= 0: [*start, *start + *width), width in [0, min(W, L)],
// start in [0, L - width]; the width is slot 2 i of the kind, the start slot 2 i + 1
OASR_HD void specaug_interval(uint64_t h, int kind, int i, int W, int L, int* start, int* width) {
  const uint64_t w = (uint64_t)(W < L ? W : L), slot = (uint64_t)i << 1;
  const uint64_t width_ = draw_slot(h, kind, slot) % (w + 1);
  *width = (int)width_;
  *start = (int)(draw_slot(h, kind, slot | 1) % ((uint64_t)L - width_ + 1));
}

// what is wrong with a policy's counts and widths, or nullptr
OASR_HD const char* specaug_policy_error(int freq_masks, int freq_width, int time_masks, int time_width) {
  if (freq_masks < 0 || time_masks < 0) return "a negative mask count";
  if (freq_masks > SPECAUG_MAX_MASKS || time_masks > SPECAUG_MAX_MASKS) return "more than OASR_SPECAUG_MAX_MASKS (8) masks of one kind";
  if (freq_width < 0 || time_width < 0) return "a negative mask width";
  return nullptr;
}
