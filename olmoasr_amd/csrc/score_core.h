// Per-sample totals of a teacher-forced score (include/oasr.h at oasr_score_reduce): the rule the device kernel (score.hip) and the host
// twin (score_host.cpp, oasr_score_reduce_host) share, so that which rows count, the order of the sum and its one rounding are ONE text
// that the CPU suite exercises without a GPU.  Plain C++: no HIP header is needed to include this file.
//
// Row (b, s) is COUNTED when s < min(span[b], S) and its target is valid: 0 <= t < V and t != ignore.  Over the counted rows of a sample,
// walked in ascending s:
//   nll_sum  the row_nll values added one after the other into a double, rounded once to f32
//   nll_max  the largest row_nll (a NaN never replaces a number); 0 when nothing is counted
//   n_tok    how many rows are counted          n_hit    how many of them have pred == target
// Rows that are not counted are not added (score_rows writes an exact 0 there, so adding them would change nothing).
#pragma once
#include <stdint.h>

#include "core_hd.h"

// the validity rule of ce_kernel and count_valid_kernel (loss.hip): an id outside [0, V) counts as ignored
OASR_HD bool sc_valid(int64_t t, int V, int64_t ignore) { return t != ignore && t >= 0 && t < (int64_t)V; }

#define SC_COUNTED 1u
#define SC_HIT 2u
// what a row adds: bit 0 = counted, bit 1 = counted and predicted right (the caller has already tested s against the span)
OASR_HD uint32_t sc_flags(int64_t t, int32_t pred, int V, int64_t ignore) {
  if (!sc_valid(t, V, ignore)) return 0u;
  return SC_COUNTED | ((int64_t)pred == t ? SC_HIT : 0u);
}

struct ScoreAcc {
  double sum;
  float mx;
  int32_t n_tok, n_hit;
};
OASR_HD void sc_init(ScoreAcc& a) { a.sum = 0.0, a.mx = 0.f, a.n_tok = 0, a.n_hit = 0; }
// one row, in ascending s
OASR_HD void sc_add(ScoreAcc& a, float nll, uint32_t flags) {
  if (!(flags & SC_COUNTED)) return;
  a.sum += (double)nll;
  if (a.n_tok == 0 || nll > a.mx) a.mx = nll;
  a.n_tok += 1;
  a.n_hit += (flags & SC_HIT) ? 1 : 0;
}
OASR_HD void sc_finish(const ScoreAcc& a, float* nll_sum, float* nll_max, int32_t* n_tok, int32_t* n_hit) {
  *nll_sum = (float)a.sum;
  *nll_max = a.n_tok ? a.mx : 0.f;
  *n_tok = a.n_tok;
  *n_hit = a.n_hit;
}
// rows of sample b that can count: span clipped to [0, S]
OASR_HD int sc_rows(int32_t span, int S) { return span < 0 ? 0 : (span > S ? S : span); }

// what both reduce entries refuse; null = fine
inline const char* sc_reduce_args_error(const void* row_nll, const void* pred, const void* targets, const void* span, int B, int S, int V,
                                        const void* nll_sum, const void* nll_max, const void* n_tok, const void* n_hit) {
  if (!row_nll || !pred || !targets || !span) return "null row_nll, pred, targets or span";
  if (!nll_sum || !nll_max || !n_tok || !n_hit) return "null output";
  if (B < 1 || S < 1 || V < 1) return "B, S and V must be positive";
  return nullptr;
}
