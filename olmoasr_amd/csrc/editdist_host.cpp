// oasr_edit_counts_host (include/oasr.h): the host twin of editdist.hip -- the same cell rule, borders and packing (editdist_core.h) walked
// row by row with two rows of cells.  The kernel's anti-diagonal order, its LDS hand-off and its token staging are covered by the GPU suite
// only.  Plain C++ (no HIP, no GPU call), so it serves CPU tensors and builds alone under a host sanitizer (tools/editdist_host_check.cpp).
#include <vector>

#include "../../include/oasr.h"
#include "editdist_core.h"

void oasr_set_error(const char* fmt, ...);

static_assert(OASR_EDIT_MAX_LEN == ED_MAX_LEN, "include/oasr.h and editdist_core.h disagree");

extern "C" size_t oasr_sizeof_edit_args(void) { return sizeof(oasr_edit_args); }

extern "C" int oasr_edit_counts_host(const oasr_edit_args* a) {
  if (const char* why = ed_args_error(a)) {
    oasr_set_error("oasr_edit_counts_host: %s", why);
    return OASR_EINVAL;
  }
  for (int b = 0; b < a->B; ++b)  // every length first: nothing is written when one is refused
    if (!ed_len_ok(a->hyp_len[b], a->Lh) || !ed_len_ok(a->ref_len[b], a->Lr)) {
      oasr_set_error("oasr_edit_counts_host: pair %d has lengths %d / %d: 0 <= length <= min(%d, row width %d / %d)", b, a->hyp_len[b],
                     a->ref_len[b], ED_MAX_LEN, a->Lh, a->Lr);
      return OASR_EINVAL;
    }
  std::vector<uint32_t> row(ED_MAX_LEN + 1);
  for (int b = 0; b < a->B; ++b) {
    const int n = a->hyp_len[b], m = a->ref_len[b];
    const int32_t* h = a->hyp + (int64_t)b * a->ld_hyp;
    const int32_t* r = a->ref + (int64_t)b * a->ld_ref;
    for (int j = 0; j <= m; ++j) row[j] = ed_row0(j);
    for (int i = 1; i <= n; ++i) {
      uint32_t diag = row[0], left = ed_col0(i);
      row[0] = left;
      for (int j = 1; j <= m; ++j) {
        const uint32_t up = row[j];
        left = ed_cell(diag, left, up, h[i - 1] != r[j - 1]);
        row[j] = left;
        diag = up;
      }
    }
    ed_unpack(row[m], m, a->out + 4 * (int64_t)b);
  }
  return OASR_OK;
}
