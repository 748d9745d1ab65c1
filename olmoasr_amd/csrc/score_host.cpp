// oasr_score_reduce_host (include/oasr.h): the host twin of score_reduce_kernel (score.hip) -- the same counting rule, sum order and rounding
// (score_core.h) walked row by row.  The kernel's staging through LDS is covered by the GPU suite only.  Plain C++ (no HIP, no GPU call), so
// it serves CPU tensors and builds alone under a host sanitizer (tools/score_host_check.cpp).
#include "../../include/oasr.h"
#include "score_core.h"

void oasr_set_error(const char* fmt, ...);

extern "C" size_t oasr_sizeof_score_args(void) { return sizeof(oasr_score_args); }

extern "C" int oasr_score_reduce_host(const float* row_nll, const int32_t* pred, const int64_t* targets, const int32_t* span, int B, int S, int V,
                                      int64_t ignore, float* nll_sum, float* nll_max, int32_t* n_tok, int32_t* n_hit) {
  if (const char* why = sc_reduce_args_error(row_nll, pred, targets, span, B, S, V, nll_sum, nll_max, n_tok, n_hit)) {
    oasr_set_error("oasr_score_reduce_host: %s", why);
    return OASR_EINVAL;
  }
  for (int b = 0; b < B; ++b) {
    const int n = sc_rows(span[b], S);
    const int64_t base = (int64_t)b * S;
    ScoreAcc acc;
    sc_init(acc);
    for (int s = 0; s < n; ++s) sc_add(acc, row_nll[base + s], sc_flags(targets[base + s], pred[base + s], V, ignore));
    sc_finish(acc, nll_sum + b, nll_max + b, n_tok + b, n_hit + b);
  }
  return OASR_OK;
}
