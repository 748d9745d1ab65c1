// Speed perturbation's rule (include/oasr.h at oasr_speed_perturb): the ONE text that the device kernel (speed.hip) and the host twin
// (speed_host.cpp: oasr_speed_perturb_host, oasr_speed_plan, oasr_speed_table) share, so that a clip resampled on the CPU is the clip the
// kernel writes, bit for bit.  Plain C++: no HIP header is needed to include this file.
//
// The operator is an integer function of its input: int16 samples, Q15 integer taps that sum to 2^15 per phase, an exact 64-bit sum, one
// rounding shift.  Floating point (double) enters only where the HOST builds a (P, Q) tap table, once; the kernel and the host twin read
// the same integers.  The factor a clip takes is a pure function of (seed, clip stream id, policy, n_valid, N), drawn from the clip's
// stream (draw_core.h) under the kind DRAW_SPEED.  The PCM row contract is pcm_core.h's.
#pragma once
#include <math.h>
#include <stdint.h>

#include "draw_core.h"
#include "pcm_core.h"

#define SPEED_MAX_FACTORS 8  // == OASR_SPEED_MAX_FACTORS (include/oasr.h)
#define SPEED_MAX_PQ 32      // 1 <= P, Q <= 32
#define SPEED_MAX_H 34       // H = floor(16 / fc) + 1 with fc >= 0.95 / 2 (P <= 2 Q)
static_assert((int64_t)PCM_MAX_N * SPEED_MAX_PQ <= (int64_t)1 << 31, "n * P and n_valid * Q stay below 2^31");

// what is wrong with a policy, or nullptr
OASR_HD const char* speed_policy_error(int n_factors, const int32_t* P, const int32_t* Q) {
  if (n_factors < 1 || n_factors > SPEED_MAX_FACTORS) return "n_factors outside [1, OASR_SPEED_MAX_FACTORS (8)]";
  for (int i = 0; i < n_factors; ++i) {
    const int p = P[i], q = Q[i];
    if (p < 1 || q < 1 || p > SPEED_MAX_PQ || q > SPEED_MAX_PQ) return "P or Q outside [1, 32]";
    int a = p, b = q;
    while (b) {
      const int t = a % b;
      a = b, b = t;
    }
    if (a != 1) return "P and Q are not coprime";
    if (q > 2 * p || p > 2 * q) return "a ratio outside [1/2, 2]";
  }
  return nullptr;
}

struct SpeedPlan {
  int P, Q;     // the ratio the row is resampled by (1, 1: a copy of the row)
  int n_out;    // leading samples of the output row that carry audio
  int factor;   // index into the policy, or -1 where the row falls back to the identity
  bool valid;   // n_valid inside [0, N]
};

// the index of the factor a clip draws (include/oasr.h: "Choice per clip")
OASR_HD int speed_choice(uint64_t seed, uint64_t clip, int n_factors) {
  return draw_below(draw_clip_hash(seed, clip), DRAW_SPEED, 0, n_factors);
}

// the plan of a clip that drew factor i = P / Q
OASR_HD SpeedPlan speed_plan_of(int i, int P, int Q, int n_valid, int N) {
  SpeedPlan pl;
  if (n_valid < 0 || n_valid > N) {
    pl.P = pl.Q = 1, pl.factor = -1, pl.valid = false;
    pl.n_out = n_valid < 0 ? 0 : N;
    return pl;
  }
  const int64_t n_out = ((int64_t)n_valid * Q) / P;
  pl.valid = true;
  if (n_out > N) {  // a slow-down that would push audio past the end of the row
    pl.P = pl.Q = 1, pl.factor = -1, pl.n_out = n_valid;
    return pl;
  }
  pl.P = P, pl.Q = Q, pl.factor = i, pl.n_out = (int)n_out;
  return pl;
}

OASR_HD SpeedPlan speed_plan(int n_factors, const int32_t* P, const int32_t* Q, uint64_t seed, uint64_t clip, int n_valid, int N) {
  const int i = speed_choice(seed, clip, n_factors);
  return speed_plan_of(i, P[i], Q[i], n_valid, N);
}

// a timestamp token under the ratio P / Q; every other token as it is
OASR_HD int64_t speed_token(int64_t t, int64_t ts_begin, int64_t ts_max, int P, int Q) {
  if (t < ts_begin || t > ts_begin + ts_max) return t;
  const int64_t k = (2 * (t - ts_begin) * Q + P) / (2 * P);
  return ts_begin + (k < ts_max ? k : ts_max);
}

// ---- the tap table: HOST only (double precision libm), built once per (P, Q) --------------------------------------------------------
// H of a ratio: fc = 0.95 min(1, Q / P), Wd = 16 / fc, H = floor(Wd) + 1
inline int speed_half_width(int P, int Q) {
  const double fc = 0.95 * (Q < P ? (double)Q / (double)P : 1.0);
  return (int)floor(16.0 / fc) + 1;
}

// out int32 [Q][2 H]: the Hann-windowed sinc of cutoff fc in Q15, every phase summing to exactly 2^15
inline void speed_build_table(int P, int Q, int32_t* out) {
  const double pi = 3.14159265358979323846;
  const double fc = 0.95 * (Q < P ? (double)Q / (double)P : 1.0), Wd = 16.0 / fc;
  const int H = (int)floor(Wd) + 1;
  for (int r = 0; r < Q; ++r) {
    int32_t* row = out + (size_t)r * 2 * H;
    int64_t sum = 0;
    int best = 0;
    for (int j = 0; j < 2 * H; ++j) {
      const int k = j - H + 1;
      const double u = (double)k - (double)r / (double)Q;
      double c = 0.0;
      if (fabs(u) < Wd) {
        const double x = pi * fc * u;
        const double sinc = x == 0.0 ? 1.0 : sin(x) / x;
        c = fc * sinc * (0.5 + 0.5 * cos(pi * u / Wd));
      }
      row[j] = (int32_t)floor(c * 32768.0 + 0.5);
      sum += row[j];
      if (row[j] > row[best]) best = j;  // (strictly larger: the first of equal maxima)
    }
    row[best] += (int32_t)(32768 - sum);
  }
}

// the library's table of a ratio (speed_host.cpp): built on first use, never freed or moved; P != Q, both inside the policy's bounds
const int32_t* speed_table_cached(int P, int Q, int* H);

// what is wrong with an argument block apart from the lengths it points to, or nullptr (A = oasr_speed_args; a template so that this
// file needs no include/oasr.h)
template <class A>
inline const char* speed_args_error(const A* a) {
  if (const char* why = pcm_args_error(a, false)) return why;
  if (!a->pcm_in || !a->pcm_out || !a->n_valid) return "null pcm_in, pcm_out or n_valid";
  if (((uintptr_t)a->n_valid | (uintptr_t)a->n_out | (uintptr_t)a->factor_out) & 3) return "an int32 operand that is not 4-byte aligned";
  if (a->tokens_a || a->tokens_b) {
    if (a->S < 1) return "tokens with S < 1";
    if ((a->tokens_a && a->ld_tokens_a < a->S) || (a->tokens_b && a->ld_tokens_b < a->S)) return "a token row stride below S";
    if (((uintptr_t)a->tokens_a | (uintptr_t)a->tokens_b) & 7) return "tokens that are not 8-byte aligned";
    if (a->ts_begin < 0 || a->ts_max < 0 || a->ts_max > (1 << 24)) return "ts_begin < 0 or ts_max outside [0, 2^24]";
  }
  return speed_policy_error(a->policy.n_factors, a->policy.P, a->policy.Q);
}

// one output sample of a resampled row (include/oasr.h: "Sample"): x zero outside [0, n_valid), T the ratio's table
OASR_HD int16_t speed_sample(const int16_t* x, int n_valid, const int32_t* T, int H, int P, int Q, int n) {
  const int m = (int)(((int64_t)n * P) / Q), r = (int)(((int64_t)n * P) % Q);
  const int32_t* row = T + (size_t)r * 2 * H;
  int64_t acc = 0;
  for (int j = 0; j < 2 * H; ++j) {
    const int i = m + j - H + 1;
    if (i >= 0 && i < n_valid) acc += (int64_t)x[i] * row[j];
  }
  return pcm_round_q15(acc);
}
