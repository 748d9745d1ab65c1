// Reverberation's rule (include/oasr.h at oasr_reverb): the ONE text that the device kernels (reverb.hip) and the host twin (reverb_host.cpp:
// oasr_reverb_host, oasr_reverb_plan) share, so that a clip reverberated on the CPU is the clip the kernels write, bit for bit.  Plain C++: no
// HIP header is needed to include this file.
//
// The operator is an integer function of its input: int16 samples, Q15 int16 taps clamped to +-32639, an exact sum below 2^44, one rounding
// shift per sample (pcm_round_q15).  What a clip draws is a pure function of (seed, clip stream id, prob_q16, R), from the clip's stream
// (draw_core.h) under the kind DRAW_REVERB.  The PCM row contract is pcm_core.h's.
//
// The device evaluates the sum on the matrix cores from signed BYTE digits of both operands (reverb_tap_lo / _hi, reverb_x_hi / _lo and
// reverb_combine below are that identity; the host check holds it to the plain product over every tap against the extremes of x).
#pragma once
#include <stdint.h>

#include "draw_core.h"
#include "pcm_core.h"

#define REVERB_MAX_K 8192      // 0.512 s at 16 kHz: |S| <= 8192 * 32639 * 32768 < 2^44
#define REVERB_TAP_MAX 32639   // 127 * 256 + 127: both byte digits of a clamped tap fit a signed byte

struct ReverbPlan {
  bool drawn;  // the clip is reverberated (if its n_valid lies in [1, N])
  int r;       // the bank row
};

// what a clip draws (include/oasr.h: "Draws per clip"); 1 <= R, prob_q16 in [0, 65536]
OASR_HD ReverbPlan reverb_plan(uint64_t seed, uint64_t clip, int prob_q16, int R) {
  const uint64_t h = draw_clip_hash(seed, clip);
  ReverbPlan pl;
  pl.drawn = draw_chance(h, DRAW_REVERB, 0, prob_q16);
  pl.r = draw_below(h, DRAW_REVERB, 1, R);
  return pl;
}

// the contract's two clamps: they make the rule total over whatever the bank's memory holds
OASR_HD int reverb_tap(int raw) { return raw < -REVERB_TAP_MAX ? -REVERB_TAP_MAX : raw > REVERB_TAP_MAX ? REVERB_TAP_MAX : raw; }
OASR_HD int reverb_delay(int raw, int K) { return raw < 0 ? 0 : raw > K - 1 ? K - 1 : raw; }

// the byte digits: tap = 256 hi + lo with both in [-127, 127] (|tap| <= 32639);  x = 256 hi + lo + 128 with both in [-128, 127]
OASR_HD int reverb_tap_lo(int tap) { return ((tap + 128) & 255) - 128; }
OASR_HD int reverb_tap_hi(int tap) { return (tap - reverb_tap_lo(tap)) >> 8; }
OASR_HD int reverb_x_hi(int x) { return x >> 8; }
OASR_HD int reverb_x_lo(int x) { return (x & 255) - 128; }
// S from the digit products p_hh = sum hi(tap) hi(x), p_mid = sum lo(tap) hi(x) + hi(tap) lo(x), p_ll = sum lo(tap) lo(x) (each below 2^29 in
// magnitude at K = 8192) and tap_sum = sum tap
OASR_HD int64_t reverb_combine(int32_t p_hh, int32_t p_mid, int32_t p_ll, int64_t tap_sum) {
  return (int64_t)p_hh * 65536 + (int64_t)p_mid * 256 + (int64_t)p_ll + 128 * tap_sum;
}

// one output sample, the rule as written: S[n] = sum_k tap(k) x(n + d - k), x = 0 outside [0, n_valid); 0 <= n < n_valid <= N, d clamped
OASR_HD int64_t reverb_sum(const int16_t* x, int n_valid, const int16_t* taps, int K, int d, int n) {
  // 0 <= n + d - k < n_valid  <=>  n + d - n_valid < k <= n + d
  const int k_lo = n + d - n_valid + 1 > 0 ? n + d - n_valid + 1 : 0, k_hi = n + d < K - 1 ? n + d : K - 1;
  int64_t S = 0;
  for (int k = k_lo; k <= k_hi; ++k) S += (int64_t)reverb_tap(taps[k]) * (int64_t)x[n + d - k];
  return S;
}

// what is wrong with an argument block apart from what the device's memory holds and the device's workspace, or nullptr (A =
// oasr_reverb_args; a template so that this file needs no include/oasr.h)
template <class A>
inline const char* reverb_args_error(const A* a) {
  if (const char* why = pcm_args_error(a, false, &A::rir)) return why;
  if (!a->pcm_in || !a->pcm_out || !a->n_valid || !a->rir || !a->delay) return "null pcm_in, pcm_out, n_valid, rir or delay";
  if (a->R < 1 || a->R > PCM_MAX_ROWS) return "R outside [1, 65535]";
  if (a->K < 1 || a->K > REVERB_MAX_K) return "K outside [1, 8192]";
  if (a->ld_rir < a->K) return "a bank row stride below K";
  if (((uintptr_t)a->n_valid | (uintptr_t)a->delay | (uintptr_t)a->row_out) & 3) return "an int32 operand that is not 4-byte aligned";
  if (pcm_overlaps_out(a, a->rir, a->R, a->K, a->ld_rir)) return "rir and pcm_out overlap";
  if (a->policy.prob_q16 < 0 || a->policy.prob_q16 > 65536) return "prob_q16 outside [0, 65536]";
  return nullptr;
}
