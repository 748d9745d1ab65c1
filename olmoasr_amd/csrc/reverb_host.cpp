// The host half of reverberation (include/oasr.h at oasr_reverb): oasr_reverb_plan and oasr_reverb_host -- the twin of reverb.hip from the
// same text (reverb_core.h).  Plain C++ (no HIP, no GPU call), so it serves where there is no device and builds alone under a host sanitizer
// (tools/reverb_host_check.cpp).  It evaluates the sum as the rule writes it, tap by sample in 64-bit integers: the byte digits are the
// device's way to the same number.
#include "../../include/oasr.h"
#include "reverb_core.h"

void oasr_set_error(const char* fmt, ...);

extern "C" int oasr_reverb_plan(const struct oasr_reverb* p, uint64_t seed, uint64_t clip, int R, int* drawn, int* row) {
  if (!p || p->prob_q16 < 0 || p->prob_q16 > 65536) {
    oasr_set_error("oasr_reverb_plan: %s", p ? "prob_q16 outside [0, 65536]" : "null policy");
    return OASR_EINVAL;
  }
  if (R < 1 || R > PCM_MAX_ROWS) {
    oasr_set_error("oasr_reverb_plan: R = %d outside [1, 65535]", R);
    return OASR_EINVAL;
  }
  const ReverbPlan pl = reverb_plan(seed, clip, p->prob_q16, R);
  if (drawn) *drawn = pl.drawn ? 1 : 0;
  if (row) *row = pl.r;
  return OASR_OK;
}

extern "C" int oasr_reverb_host(const oasr_reverb_args* a) {
  const char* why = reverb_args_error(a);
  if (why) {
    oasr_set_error("oasr_reverb_host: %s", why);
    return OASR_EINVAL;
  }
  for (int b = 0; b < a->B; ++b) {
    const ReverbPlan pl = reverb_plan(a->seed, a->first_clip + (uint64_t)b, a->policy.prob_q16, a->R);
    const int16_t* x = a->pcm_in + (size_t)b * (size_t)a->ld_in;
    int16_t* y = a->pcm_out + (size_t)b * (size_t)a->ld_out;
    const int nv = a->n_valid[b];
    const bool wet = pl.drawn && nv >= 1 && nv <= a->N;
    if (a->row_out) a->row_out[b] = wet ? pl.r : -1;
    if (!wet) {
      pcm_copy_row(y, x, 0, a->N);
      continue;
    }
    const int16_t* taps = a->rir + (size_t)pl.r * (size_t)a->ld_rir;
    const int d = reverb_delay(a->delay[pl.r], a->K);
    for (int n = 0; n < nv; ++n) y[n] = pcm_round_q15(reverb_sum(x, nv, taps, a->K, d, n));
    pcm_copy_row(y, x, nv, a->N);
  }
  return OASR_OK;
}
