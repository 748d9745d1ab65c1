// The row contract of the int16 PCM operators (include/oasr.h at oasr_speed_perturb, oasr_noise_mix, oasr_reverb): pcm_in / pcm_out are
// [B, N] int16 with row strides ld_in / ld_out >= N.  The bounds, the two roundings, the byte spans and the argument checks that the three
// rules (speed_core.h, noise_core.h, reverb_core.h) have in common, in the ONE text that the device kernels and the host twins share.
// Plain C++: no HIP header is needed to include this file.
#pragma once
#include <stdint.h>
#include <string.h>

#include "core_hd.h"

#define PCM_MAX_N (1 << 26)  // samples of a row (of a bank row too): n * 32 stays below 2^31, a row's energy <= 2^26 * 2^30 = 2^56
#define PCM_MAX_ROWS 65535   // rows of a batch or of a bank: one grid dimension

OASR_HD int16_t pcm_clamp(int64_t v) {
  v = v < -32768 ? -32768 : v;
  v = v > 32767 ? 32767 : v;
  return (int16_t)v;
}

// y = clamp((S + 2^14) >> 15) of an exact Q15 sum (an arithmetic shift: floor)
OASR_HD int16_t pcm_round_q15(int64_t S) { return pcm_clamp((S + 16384) >> 15); }

// the bytes [*lo, *hi) that a [rows, cols] int16 matrix with row stride ld occupies
inline void pcm_span(const int16_t* p, int rows, int cols, int ld, uintptr_t* lo, uintptr_t* hi) {
  *lo = (uintptr_t)p, *hi = *lo + 2 * ((uintptr_t)(rows - 1) * (uintptr_t)ld + (uintptr_t)cols);
}
// a [rows, cols] bank under the [B, N] output of an argument block
template <class A>
inline bool pcm_overlaps_out(const A* a, const int16_t* bank, int rows, int cols, int ld) {
  uintptr_t out0, out1, bank0, bank1;
  pcm_span(a->pcm_out, a->B, a->N, a->ld_out, &out0, &out1), pcm_span(bank, rows, cols, ld, &bank0, &bank1);
  return bank0 < out1 && out0 < bank1;
}

// what is wrong with an argument block (A = oasr_speed_args, oasr_noise_args, oasr_reverb_args) as far as its PCM rows go, or nullptr.
// in_place: pcm_out may be pcm_in itself with the same stride.  bank: the member that holds the operator's int16 bank, which is held to the
// same 2-byte alignment, or nullptr where it has none.  Nothing is dereferenced: which pointers may not be null is the caller's to say.
template <class A>
inline const char* pcm_args_error(const A* a, bool in_place, const int16_t* A::*bank = nullptr) {
  if (!a) return "null argument block";
  if (a->B < 1 || a->B > PCM_MAX_ROWS) return "B outside [1, 65535]";
  if (a->N < 1 || a->N > PCM_MAX_N) return "N outside [1, 2^26]";
  if (a->ld_in < a->N || a->ld_out < a->N) return "a PCM row stride below N";
  if (((uintptr_t)a->pcm_in | (uintptr_t)a->pcm_out | (uintptr_t)(bank ? a->*bank : nullptr)) & 1)
    return bank ? "PCM or bank that is not 2-byte aligned" : "PCM that is not 2-byte aligned";
  uintptr_t in0, in1, out0, out1;
  pcm_span(a->pcm_in, a->B, a->N, a->ld_in, &in0, &in1), pcm_span(a->pcm_out, a->B, a->N, a->ld_out, &out0, &out1);
  if (in0 < out1 && out0 < in1) {
    if (!in_place) return "pcm_in and pcm_out overlap (the operator works out of place)";
    if (!(in0 == out0 && a->ld_in == a->ld_out)) return "pcm_in and pcm_out overlap without being the same buffer with the same stride";
  }
  return nullptr;
}

// samples [from, N) of a row as they are (the host twins' copy of a row, or of its tail behind n_valid); nothing to do in place
inline void pcm_copy_row(int16_t* y, const int16_t* x, int from, int N) {
  if (y != x) memcpy(y + from, x + from, sizeof(int16_t) * (size_t)(N - from));
}
