// The seeded per-clip draw stream of the augmentation operators (include/oasr.h at oasr_spec_augment, oasr_speed_perturb, oasr_noise_mix,
// oasr_reverb, oasr_telephone): the ONE text that the device kernels and the host twins share.  Plain C++: no HIP header is needed to include this file.
//
// Everything is unsigned 64-bit integer arithmetic with wrap-around; no floating point enters a draw.  What a clip draws is a pure function
// of (seed, clip stream id, kind, slot): it does not depend on the batch the clip sits in or on how many calls came before.
#pragma once
#include <stdint.h>

#include "core_hd.h"

// The registry of kinds: each operator draws under a kind of its own, so no two operators read the same value of a clip's stream.  A new
// operator takes the next number; the numbers below are part of what a seed means and never change.
enum { DRAW_FREQ_MASK = 1, DRAW_TIME_MASK = 2, DRAW_SPEED = 3, DRAW_NOISE = 4, DRAW_REVERB = 5, DRAW_TELEPHONE = 6 };
static_assert(DRAW_FREQ_MASK == 1 && DRAW_TIME_MASK == 2 && DRAW_SPEED == 3 && DRAW_NOISE == 4 && DRAW_REVERB == 5 && DRAW_TELEPHONE == 6,
              "the kinds are fixed");

// splitmix64's finalizer on z + golden ratio
OASR_HD uint64_t draw_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the per-clip key every draw of that clip comes from
OASR_HD uint64_t draw_clip_hash(uint64_t seed, uint64_t clip) { return draw_mix(draw_mix(seed) ^ clip); }

// the value of slot i (below 2^16) of a kind
OASR_HD uint64_t draw_slot(uint64_t h, int kind, uint64_t i) { return draw_mix(h ^ (((uint64_t)kind << 16) | i)); }
// slot i as a uniform integer below n >= 1
OASR_HD int draw_below(uint64_t h, int kind, uint64_t i, int n) { return (int)(draw_slot(h, kind, i) % (uint64_t)n); }
// slot i as a Bernoulli draw with probability prob_q16 / 65536
OASR_HD bool draw_chance(uint64_t h, int kind, uint64_t i, int prob_q16) { return draw_slot(h, kind, i) % 65536u < (uint64_t)prob_q16; }
