// The host half of speed perturbation (include/oasr.h at oasr_speed_perturb): the library's tap tables (built once per ratio, read by the
// kernel's launcher and by the twin alike), oasr_speed_table, oasr_speed_plan and oasr_speed_perturb_host -- the twin of speed.hip from
// the same text (speed_core.h).  Plain C++ (no HIP, no GPU call), so it serves where there is no device and builds alone under a host
// sanitizer (tools/speed_host_check.cpp).
#include <string.h>

#include <map>
#include <memory>
#include <mutex>
#include <utility>

#include "../../include/oasr.h"
#include "speed_core.h"

void oasr_set_error(const char* fmt, ...);

static_assert(OASR_SPEED_MAX_FACTORS == SPEED_MAX_FACTORS, "include/oasr.h and speed_core.h disagree");

const int32_t* speed_table_cached(int P, int Q, int* H) {
  static std::mutex mu;
  static std::map<std::pair<int, int>, std::unique_ptr<int32_t[]>> tables;
  std::lock_guard<std::mutex> lock(mu);
  *H = speed_half_width(P, Q);
  std::unique_ptr<int32_t[]>& t = tables[{P, Q}];
  if (!t) {
    t.reset(new int32_t[(size_t)Q * 2 * *H]);
    speed_build_table(P, Q, t.get());
  }
  return t.get();
}

static const char* pair_error(int P, int Q) {
  const int32_t p[1] = {P}, q[1] = {Q};
  const char* why = speed_policy_error(1, p, q);
  return why ? why : (P == Q ? "P == Q is the identity: it has no table" : nullptr);
}

extern "C" int oasr_speed_table(int P, int Q, int32_t* out, int* H) {
  const char* why = pair_error(P, Q);
  if (why || !H) {
    oasr_set_error("oasr_speed_table: %s (P = %d, Q = %d)", why ? why : "null H", P, Q);
    return OASR_EINVAL;
  }
  const int32_t* t = speed_table_cached(P, Q, H);
  if (out) memcpy(out, t, sizeof(int32_t) * (size_t)Q * 2 * (size_t)*H);
  return OASR_OK;
}

extern "C" int oasr_speed_plan(const oasr_speed* p, uint64_t seed, uint64_t clip, int n_valid, int N, int* P, int* Q, int* n_out, int* factor) {
  const char* why = p ? speed_policy_error(p->n_factors, p->P, p->Q) : "null policy";
  if (why) {
    oasr_set_error("oasr_speed_plan: %s", why);
    return OASR_EINVAL;
  }
  if (N < 1 || N > PCM_MAX_N || n_valid < 0 || n_valid > N) {
    oasr_set_error("oasr_speed_plan: N = %d outside [1, 2^26] or n_valid = %d outside [0, N]", N, n_valid);
    return OASR_EINVAL;
  }
  const SpeedPlan pl = speed_plan(p->n_factors, p->P, p->Q, seed, clip, n_valid, N);
  if (P) *P = pl.P;
  if (Q) *Q = pl.Q;
  if (n_out) *n_out = pl.n_out;
  if (factor) *factor = pl.factor;
  return OASR_OK;
}

extern "C" int oasr_speed_perturb_host(const oasr_speed_args* a) {
  const char* why = speed_args_error(a);
  if (why) {
    oasr_set_error("oasr_speed_perturb_host: %s", why);
    return OASR_EINVAL;
  }
  for (int b = 0; b < a->B; ++b)
    if (a->n_valid[b] < 0 || a->n_valid[b] > a->N) {
      oasr_set_error("oasr_speed_perturb_host: n_valid[%d] = %d outside [0, N = %d]", b, a->n_valid[b], a->N);
      return OASR_EINVAL;
    }
  for (int b = 0; b < a->B; ++b) {
    const SpeedPlan pl = speed_plan(a->policy.n_factors, a->policy.P, a->policy.Q, a->seed, a->first_clip + (uint64_t)b, a->n_valid[b], a->N);
    const int16_t* x = a->pcm_in + (size_t)b * (size_t)a->ld_in;
    int16_t* y = a->pcm_out + (size_t)b * (size_t)a->ld_out;
    if (a->n_out) a->n_out[b] = pl.n_out;
    if (a->factor_out) a->factor_out[b] = pl.factor;
    if (pl.P == pl.Q) {
      pcm_copy_row(y, x, 0, a->N);
      continue;
    }
    int H = 0;
    const int32_t* T = speed_table_cached(pl.P, pl.Q, &H);
    for (int n = 0; n < pl.n_out; ++n) y[n] = speed_sample(x, a->n_valid[b], T, H, pl.P, pl.Q, n);
    for (int n = pl.n_out; n < a->N; ++n) y[n] = 0;
    int64_t* rows[2] = {a->tokens_a ? a->tokens_a + (size_t)b * (size_t)a->ld_tokens_a : nullptr,
                        a->tokens_b ? a->tokens_b + (size_t)b * (size_t)a->ld_tokens_b : nullptr};
    for (int64_t* row : rows)
      if (row)
        for (int s = 0; s < a->S; ++s) row[s] = speed_token(row[s], a->ts_begin, a->ts_max, pl.P, pl.Q);
  }
  return OASR_OK;
}
