// The host half of noise mixing (include/oasr.h at oasr_noise_mix): oasr_noise_plan and oasr_noise_mix_host -- the twin of noise.hip from the
// same text (noise_core.h).  Plain C++ (no HIP, no GPU call), so it serves where there is no device and builds alone under a host sanitizer
// (tools/noise_host_check.cpp).
#include "../../include/oasr.h"
#include "noise_core.h"

void oasr_set_error(const char* fmt, ...);

static_assert(OASR_NOISE_NONE == NOISE_NONE, "include/oasr.h and noise_core.h disagree");

extern "C" int oasr_noise_plan(const oasr_noise* p, uint64_t seed, uint64_t clip, int M, int L, int* drawn, int* row, int* offset, int* snr_db) {
  const char* why = p ? noise_policy_error(p->prob_q16, p->snr_lo_db, p->snr_hi_db) : "null policy";
  if (why) {
    oasr_set_error("oasr_noise_plan: %s", why);
    return OASR_EINVAL;
  }
  if (M < 1 || M > PCM_MAX_ROWS || L < 1 || L > PCM_MAX_N) {
    oasr_set_error("oasr_noise_plan: M = %d outside [1, 65535] or L = %d outside [1, 2^26]", M, L);
    return OASR_EINVAL;
  }
  const NoisePlan pl = noise_plan(seed, clip, p->prob_q16, p->snr_lo_db, p->snr_hi_db, M, L);
  if (drawn) *drawn = pl.drawn ? 1 : 0;
  if (row) *row = pl.m;
  if (offset) *offset = pl.o;
  if (snr_db) *snr_db = pl.s;
  return OASR_OK;
}

extern "C" int oasr_noise_mix_host(const oasr_noise_args* a) {
  const char* why = noise_args_error(a);
  if (why) {
    oasr_set_error("oasr_noise_mix_host: %s", why);
    return OASR_EINVAL;
  }
  for (int b = 0; b < a->B; ++b) {
    const NoisePlan pl = noise_plan(a->seed, a->first_clip + (uint64_t)b, a->policy.prob_q16, a->policy.snr_lo_db, a->policy.snr_hi_db, a->M, a->L);
    const int16_t* x = a->pcm_in + (size_t)b * (size_t)a->ld_in;
    int16_t* y = a->pcm_out + (size_t)b * (size_t)a->ld_out;
    const int16_t* v = a->bank + (size_t)pl.m * (size_t)a->ld_bank;
    const int nv = a->n_valid[b];
    int64_t g = 0;
    bool mixed = false;
    if (pl.drawn && nv >= 1 && nv <= a->N) {
      uint64_t Ex = 0, Ev = 0;
      for (int n = 0, p = pl.o; n < nv; ++n) {
        Ex += (uint64_t)((int64_t)x[n] * x[n]);
        Ev += (uint64_t)((int64_t)v[p] * v[p]);
        if (++p == a->L) p = 0;
      }
      mixed = noise_gain(Ex, Ev, pl.s, &g);
    }
    if (a->row_out) a->row_out[b] = mixed ? pl.m : -1;
    if (a->snr_out) a->snr_out[b] = mixed ? pl.s : NOISE_NONE;
    if (a->gain_out) a->gain_out[b] = g;
    if (!mixed) {
      pcm_copy_row(y, x, 0, a->N);
      continue;
    }
    for (int n = 0, p = pl.o; n < nv; ++n) {
      y[n] = noise_sample(x[n], v[p], g);
      if (++p == a->L) p = 0;
    }
    pcm_copy_row(y, x, nv, a->N);
  }
  return OASR_OK;
}
