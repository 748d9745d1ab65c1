// Noise mixing's rule (include/oasr.h at oasr_noise_mix): the ONE text that the device kernels (noise.hip) and the host twin (noise_host.cpp:
// oasr_noise_mix_host, oasr_noise_plan) share, so that a clip mixed on the CPU is the clip the kernels write, bit for bit.  Plain C++: no HIP
// header is needed to include this file.
//
// The operator is an integer function of its input: int16 samples, two exact 64-bit energies, one 64-bit division, a 32-step integer square
// root, a table of 61 integer amplitudes, one rounding shift per sample.  Unsigned and signed 64-bit integers only: no floating point, on
// the host either, and no 128-bit type.  What a clip draws is a pure function of (seed, clip stream id, policy, M, L), from the clip's
// stream (draw_core.h) under the kind DRAW_NOISE.  The PCM row contract is pcm_core.h's: a row's energy stays <= 2^26 * 2^30 = 2^56, and
// o + n below 2^27.
#pragma once
#include <stdint.h>

#include "draw_core.h"
#include "pcm_core.h"

#define NOISE_SNR_MIN (-10)
#define NOISE_SNR_MAX 50
#define NOISE_NONE (-128)      // == OASR_NOISE_NONE (include/oasr.h): snr_out of a clip that is not mixed

// A[s + 10] = round(10^(-s / 20) * 2^15), s = -10 .. 50 dB: the noise's amplitude relative to the clip's, Q15
OASR_HD int64_t noise_amplitude(int s) {
  constexpr int32_t A[NOISE_SNR_MAX - NOISE_SNR_MIN + 1] = {
      103622, 92353, 82309, 73358, 65381, 58271, 51934, 46286, 41252, 36766,  // -10 .. -1
      32768,  29205, 26029, 23198, 20675, 18427, 16423, 14637, 13045, 11627,  //   0 ..  9
      10362,  9235,  8231,  7336,  6538,  5827,  5193,  4629,  4125,  3677,   //  10 .. 19
      3277,   2920,  2603,  2320,  2068,  1843,  1642,  1464,  1305,  1163,   //  20 .. 29
      1036,   924,   823,   734,   654,   583,   519,   463,   413,   368,    //  30 .. 39
      328,    292,   260,   232,   207,   184,   164,   146,   130,   116,    //  40 .. 49
      104};                                                                   //  50
  return A[s - NOISE_SNR_MIN];
}

// what is wrong with a policy, or nullptr
OASR_HD const char* noise_policy_error(int prob_q16, int snr_lo_db, int snr_hi_db) {
  if (prob_q16 < 0 || prob_q16 > 65536) return "prob_q16 outside [0, 65536]";
  if (snr_lo_db < NOISE_SNR_MIN || snr_hi_db > NOISE_SNR_MAX) return "an SNR outside [-10, 50] dB";
  if (snr_lo_db > snr_hi_db) return "snr_lo_db above snr_hi_db";
  return nullptr;
}

struct NoisePlan {
  bool drawn;  // the clip takes noise (if its audio and the bank row's are not silent)
  int m;       // the bank row
  int o;       // the offset into that row of the clip's sample 0
  int s;       // the SNR in whole dB
};

// what a clip draws (include/oasr.h: "Draws per clip"); 1 <= M, 1 <= L, a valid policy
OASR_HD NoisePlan noise_plan(uint64_t seed, uint64_t clip, int prob_q16, int snr_lo_db, int snr_hi_db, int M, int L) {
  const uint64_t h = draw_clip_hash(seed, clip);
  NoisePlan pl;
  pl.drawn = draw_chance(h, DRAW_NOISE, 0, prob_q16);
  pl.m = draw_below(h, DRAW_NOISE, 1, M);
  pl.o = draw_below(h, DRAW_NOISE, 2, L);
  // (not draw_below: with the span taken before the hash the kernels' instructions come out in another order)
  pl.s = snr_lo_db + (int)(draw_slot(h, DRAW_NOISE, 3) % (uint64_t)(snr_hi_db - snr_lo_db + 1));
  return pl;
}

// the number of bits of v (0 for 0)
OASR_HD int noise_bitlength(uint64_t v) {
  int n = 0;
  for (int step = 32; step > 0; step >>= 1)
    if (v >> step) v >>= step, n += step;
  return n + (int)v;  // (v is 0 or 1 here)
}

// floor(sqrt(v)): one result bit per step, from bit 31 down
OASR_HD uint64_t noise_isqrt(uint64_t v) {
  uint32_t r = 0;
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t c = r | (1u << bit);
    if ((uint64_t)c * c <= v) r = c;  // (c < 2^32: the square fits)
  }
  return r;
}

// the gain of a drawn clip with energies Ex (the clip) and Ev (the noise under it), both <= 2^56, at s dB: true and the Q16 gain (below
// 2^34; it may be 0) where the clip is mixed, false where either energy vanishes at the common scale
OASR_HD bool noise_gain(uint64_t Ex, uint64_t Ev, int s, int64_t* g) {
  *g = 0;
  const int bits = noise_bitlength(Ex | Ev), sh = bits > 31 ? bits - 31 : 0;
  const uint64_t ex = Ex >> sh, ev = Ev >> sh;  // both below 2^31
  if (ex == 0 || ev == 0) return false;
  const uint64_t g0 = noise_isqrt((ex << 32) / ev);                // Q16, below 2^31.5
  *g = (int64_t)((g0 * (uint64_t)noise_amplitude(s) + 16384) >> 15);  // g0 * A below 2^48.5
  return true;
}

// y = clamp(x + ((v g + 2^15) >> 16)) (an arithmetic shift: floor); v = 0 gives x
OASR_HD int16_t noise_sample(int x, int v, int64_t g) { return pcm_clamp((int64_t)x + (((int64_t)v * g + 32768) >> 16)); }

// what is wrong with an argument block apart from the lengths it points to and the device's workspace, or nullptr (A = oasr_noise_args; a
// template so that this file needs no include/oasr.h)
template <class A>
inline const char* noise_args_error(const A* a) {
  if (const char* why = pcm_args_error(a, true, &A::bank)) return why;
  if (!a->pcm_in || !a->pcm_out || !a->n_valid || !a->bank) return "null pcm_in, pcm_out, n_valid or bank";
  if (a->M < 1 || a->M > PCM_MAX_ROWS) return "M outside [1, 65535]";
  if (a->L < 1 || a->L > PCM_MAX_N) return "L outside [1, 2^26]";
  if (a->ld_bank < a->L) return "a bank row stride below L";
  if (((uintptr_t)a->n_valid | (uintptr_t)a->row_out | (uintptr_t)a->snr_out) & 3) return "an int32 operand that is not 4-byte aligned";
  if ((uintptr_t)a->gain_out & 7) return "gain_out that is not 8-byte aligned";
  if (pcm_overlaps_out(a, a->bank, a->M, a->L, a->ld_bank)) return "bank and pcm_out overlap";
  return noise_policy_error(a->policy.prob_q16, a->policy.snr_lo_db, a->policy.snr_hi_db);
}
