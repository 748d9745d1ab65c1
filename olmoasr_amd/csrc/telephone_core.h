// The telephone channel's rule (include/oasr.h at oasr_telephone): the ONE text that the device kernel (telephone.hip) and the host twin
// (telephone_host.cpp: oasr_telephone_host, oasr_telephone_plan, oasr_telephone_tables, oasr_telephone_quantize_host) share, so that a clip
// sent through the channel on the CPU is the clip the kernel writes, bit for bit.  Plain C++: no HIP header is needed to include this file.
//
// The operator is an integer function of its input: int16 samples at 16 kHz, a 129-tap Q15 band-pass (300 - 3400 Hz) evaluated at every
// second sample (8 kHz), a G.711 quantiser in closed form (mu-law, A-law, or none), a 32-tap Q15 half-sample interpolator back to 16 kHz;
// exact sums, one rounding shift each.  Both filters are symmetric about their output sample (zero phase): lengths, n_valid and timestamps
// stay.  Floating point (double) enters only where the HOST builds the two tap tables, once; the kernel and the host twin read the same
// integers.  What a clip draws is a pure function of (seed, clip stream id, policy), from the clip's stream (draw_core.h) under the kind
// DRAW_TELEPHONE.  The PCM row contract is pcm_core.h's.
#pragma once
#include <math.h>
#include <stdint.h>

#include "draw_core.h"
#include "pcm_core.h"

#define TEL_MAX_CODECS 8  // == OASR_TELEPHONE_MAX_CODECS (include/oasr.h)
#define TEL_LINEAR 0      // == OASR_TELEPHONE_LINEAR, _MULAW, _ALAW
#define TEL_MULAW 1
#define TEL_ALAW 2
#define TEL_BP_HALF 64                  // the band-pass h[k], k = -64 .. 64, kept as h[k + 64]
#define TEL_BP_TAPS (2 * TEL_BP_HALF + 1)
#define TEL_UP_TAPS 32                  // the interpolator's odd phase u[j], j = 0 .. 31, over c[m + j - 15]
#define TEL_UP_LEFT 15

// what is wrong with a policy, or nullptr
OASR_HD const char* tel_policy_error(int prob_q16, int n_codecs, const int32_t* codecs, int bandpass) {
  if (prob_q16 < 0 || prob_q16 > 65536) return "prob_q16 outside [0, 65536]";
  if (n_codecs < 1 || n_codecs > TEL_MAX_CODECS) return "n_codecs outside [1, OASR_TELEPHONE_MAX_CODECS (8)]";
  for (int i = 0; i < n_codecs; ++i)
    if (codecs[i] < TEL_LINEAR || codecs[i] > TEL_ALAW) return "a codec outside {0 linear, 1 mu-law, 2 A-law}";
  if (bandpass != 0 && bandpass != 1) return "bandpass outside {0, 1}";
  return nullptr;
}

struct TelPlan {
  bool drawn;  // the clip goes through the channel (if its n_valid is inside [1, N])
  int choice;  // the index into the policy's codecs
};

// what a clip draws (include/oasr.h: "Draws per clip"); a valid policy
OASR_HD TelPlan tel_plan(uint64_t seed, uint64_t clip, int prob_q16, int n_codecs) {
  const uint64_t h = draw_clip_hash(seed, clip);
  TelPlan pl;
  pl.drawn = draw_chance(h, DRAW_TELEPHONE, 0, prob_q16);
  pl.choice = draw_below(h, DRAW_TELEPHONE, 1, n_codecs);
  return pl;
}

// codecs[i] (a select per slot: on the device no indexed copy of the policy goes to scratch)
OASR_HD int tel_codec_at(const int32_t* codecs, int i) {
  int c = TEL_LINEAR;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int s = 0; s < TEL_MAX_CODECS; ++s)
    if (s == i) c = codecs[s];
  return c;
}

// the codec a row takes, or -1 where it is copied: not drawn, or n_valid outside [1, N]
OASR_HD int tel_row_codec(uint64_t seed, uint64_t clip, int prob_q16, int n_codecs, const int32_t* codecs, int n_valid, int N) {
  const TelPlan pl = tel_plan(seed, clip, prob_q16, n_codecs);
  return (pl.drawn && n_valid >= 1 && n_valid <= N) ? tel_codec_at(codecs, pl.choice) : -1;
}

// floor(log2 a), a >= 1
OASR_HD int tel_log2(uint32_t a) { return 31 - __builtin_clz(a); }

// G.711 mu-law as expand(compress(x)) on the 16-bit value: 255 levels inside +-32124
OASR_HD int tel_mulaw(int x) {
  const bool s = x < 0;
  int a = s ? -x : x;
  a = (a > 32635 ? 32635 : a) + 132;  // 132 .. 32767
  const int e = tel_log2((uint32_t)a) - 7;  // 0 .. 7
  const int m = (a >> (e + 3)) & 15;
  const int y = (((m << 3) + 132) << e) - 132;
  return s ? -y : y;
}

// G.711 A-law as expand(compress(x)) on the 16-bit value: 256 levels inside +-32256, none of them 0
OASR_HD int tel_alaw(int x) {
  const bool s = x < 0;
  const int a = s ? -x - 1 : x;  // 0 .. 32767
  const int v = a >> 3;
  const int g = v < 32 ? 0 : tel_log2((uint32_t)v) - 4;  // 0 .. 7
  const int m = g < 2 ? (v >> 1) & 15 : (v >> g) & 15;
  const int y = g == 0 ? (m << 4) + 8 : ((m << 4) + 264) << (g - 1);
  return s ? -y : y;
}

OASR_HD int16_t tel_quantize(int x, int codec) { return (int16_t)(codec == TEL_MULAW ? tel_mulaw(x) : codec == TEL_ALAW ? tel_alaw(x) : x); }

// ---- the tap tables: HOST only (double precision libm), built once -------------------------------------------------------------------
struct TelTables {
  int32_t h[TEL_BP_TAPS];  // h[k + 64]
  int32_t u[TEL_UP_TAPS];
};

inline void tel_build_tables(int32_t* h, int32_t* u) {
  const double pi = 3.14159265358979323846;
  auto sinc = [pi](double t) { return t == 0.0 ? 1.0 : sin(pi * t) / (pi * t); };
  auto lp = [&sinc](double f, int k) { return (2.0 * f / 16000.0) * sinc(2.0 * f * (double)k / 16000.0); };
  for (int k = -TEL_BP_HALF; k <= TEL_BP_HALF; ++k) {
    const double c = (lp(3400.0, k) - lp(300.0, k)) * (0.5 + 0.5 * cos(pi * (double)k / 65.0));
    h[k + TEL_BP_HALF] = (int32_t)floor(c * 32768.0 + 0.5);  // (no sum fix-up: a band-pass has no gain at 0 Hz to hold)
  }
  int64_t sum = 0;
  int best = 0;
  for (int j = 0; j < TEL_UP_TAPS; ++j) {
    const double t = (double)(j - TEL_UP_LEFT) - 0.5;
    u[j] = (int32_t)floor(sinc(t) * (0.5 + 0.5 * cos(pi * t / 16.0)) * 32768.0 + 0.5);
    sum += u[j];
    if (u[j] > u[best]) best = j;  // (strictly larger: the first of equal maxima)
  }
  u[best] += (int32_t)(32768 - sum);
}

// What the kernel's 32-bit partial accumulators need: it sums the band-pass's even and odd taps apart, and the interpolator's two halves
// apart, each over samples of magnitude <= 2^15, so each group's sum of |tap| must stay <= 65535 (65535 * 2^15 < 2^31); and every tap must
// fit the int16 operand of the packed dot product.  The whole sums (76960 and 81604) do not fit: a single 32-bit accumulator would wrap.
inline bool tel_tables_bounded(const int32_t* h, const int32_t* u) {
  int64_t group[4] = {0, 0, 0, 0};
  for (int i = 0; i < TEL_BP_TAPS; ++i) group[i & 1] += h[i] < 0 ? -(int64_t)h[i] : h[i];
  for (int j = 0; j < TEL_UP_TAPS; ++j) group[2 + j / (TEL_UP_TAPS / 2)] += u[j] < 0 ? -(int64_t)u[j] : u[j];
  for (int64_t g : group)
    if (g > 65535) return false;
  for (int i = 0; i < TEL_BP_TAPS; ++i)
    if (h[i] < -32768 || h[i] > 32767) return false;
  for (int j = 0; j < TEL_UP_TAPS; ++j)
    if (u[j] < -32768 || u[j] > 32767) return false;
  return true;
}

// the library's tables (telephone_host.cpp): built on first use, never freed or moved; nullptr if they miss tel_tables_bounded
const TelTables* tel_tables_cached();

// what is wrong with an argument block apart from the lengths it points to, or nullptr (A = oasr_telephone_args; a template so that this
// file needs no include/oasr.h)
template <class A>
inline const char* tel_args_error(const A* a) {
  if (const char* why = pcm_args_error(a, false)) return why;
  if (!a->pcm_in || !a->pcm_out || !a->n_valid) return "null pcm_in, pcm_out or n_valid";
  if (((uintptr_t)a->n_valid | (uintptr_t)a->codec_out) & 3) return "an int32 operand that is not 4-byte aligned";
  return tel_policy_error(a->policy.prob_q16, a->policy.n_codecs, a->policy.codecs, a->policy.bandpass);
}

// ---- samples (include/oasr.h: "Samples"): x zero outside [0, n_valid) ---------------------------------------------------------------------
// z[m], 0 <= m < ceil(n_valid / 2): the band-passed clip at 8 kHz (or, without the band-pass, its even samples)
OASR_HD int16_t tel_decimated(const int16_t* x, int n_valid, const int32_t* h, int bandpass, int m) {
  if (!bandpass) return x[2 * m];
  int64_t acc = 0;
  for (int k = -TEL_BP_HALF; k <= TEL_BP_HALF; ++k) {
    const int i = 2 * m - k;
    if (i >= 0 && i < n_valid) acc += (int64_t)h[k + TEL_BP_HALF] * x[i];
  }
  return pcm_round_q15(acc);
}

// y[2 m + 1] from the companded 8 kHz samples c[0 .. M), zero outside
OASR_HD int16_t tel_interpolated(const int16_t* c, int M, const int32_t* u, int m) {
  int64_t acc = 0;
  for (int j = 0; j < TEL_UP_TAPS; ++j) {
    const int i = m + j - TEL_UP_LEFT;
    if (i >= 0 && i < M) acc += (int64_t)u[j] * c[i];
  }
  return pcm_round_q15(acc);
}
