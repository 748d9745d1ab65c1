// Edit distance with substitution / deletion / insertion counts (include/oasr.h at oasr_edit_counts): the rule the device kernel
// (editdist.hip) and the host twin (editdist_host.cpp, oasr_edit_counts_host) share, so that the cell update, the borders and the tie order
// are ONE text that the CPU suite exercises without a GPU.  Plain C++: no HIP header is needed to include this file.
//
// Cell (i, j) covers the first i tokens of hyp and the first j tokens of ref and carries (S, D, I); its cost is S + D + I.
//   borders   (0, j) = (0, j, 0)     (i, 0) = (0, 0, i)
//   interior  cd = cost(i-1, j-1) + (hyp[i-1] != ref[j-1])      a hit or a substitution
//             cl = cost(i, j-1) + 1                             a deletion: ref[j-1] is missing from hyp
//             cu = cost(i-1, j) + 1                             an insertion: hyp[i-1] is not in ref
//             the minimum wins; on a tie the diagonal, then the deletion, then the insertion.  The cell takes the chosen predecessor's counts
//             and adds its own step -- the counts are carried forward, there is no trace and no backtrace.
// The answer is cell (hyp_len, ref_len); hits = ref_len - S - D.
//
// A cell is one 32-bit word: cost << 20 | S << 10 | D, every field < 1024 (lengths <= ED_MAX_LEN); I = cost - S - D.  A step is then one
// integer add and the cost one shift.
#pragma once
#include <stdint.h>

#include "../../include/oasr.h"
#include "core_hd.h"

#define ED_MAX_LEN 1023  // cost, S and D each fit 10 bits

#define ED_STEP_SUB ((1u << 20) | (1u << 10))
#define ED_STEP_DEL ((1u << 20) | 1u)
#define ED_STEP_INS (1u << 20)

OASR_HD uint32_t ed_row0(int j) { return ((uint32_t)j << 20) | (uint32_t)j; }  // (0, j): j deletions
OASR_HD uint32_t ed_col0(int i) { return (uint32_t)i << 20; }                   // (i, 0): i insertions
OASR_HD uint32_t ed_cost(uint32_t c) { return c >> 20; }

// diag = (i-1, j-1), left = (i, j-1), up = (i-1, j); neq = hyp[i-1] != ref[j-1]
OASR_HD uint32_t ed_cell(uint32_t diag, uint32_t left, uint32_t up, bool neq) {
  const uint32_t cd = ed_cost(diag) + (neq ? 1u : 0u), cl = ed_cost(left) + 1u, cu = ed_cost(up) + 1u;
  if (cd <= cl && cd <= cu) return diag + (neq ? ED_STEP_SUB : 0u);
  if (cl <= cu) return left + ED_STEP_DEL;
  return up + ED_STEP_INS;
}

// out[0 .. 4) = (S, D, I, H) of the final cell
OASR_HD void ed_unpack(uint32_t c, int ref_len, int32_t* out) {
  const int s = (int)((c >> 10) & 1023u), d = (int)(c & 1023u);
  out[0] = s, out[1] = d, out[2] = (int)ed_cost(c) - s - d, out[3] = ref_len - s - d;
}

// a length the contract allows for a row of `width` tokens
OASR_HD bool ed_len_ok(int len, int64_t width) { return len >= 0 && len <= ED_MAX_LEN && (int64_t)len <= width; }

// what both entry points refuse without looking at the lengths (which the device entry cannot read on the host); null = fine
inline const char* ed_args_error(const oasr_edit_args* a) {
  if (!a) return "null argument block";
  if (a->B < 1 || a->Lh < 0 || a->Lr < 0) return "B >= 1 and row widths >= 0";
  if (!a->hyp_len || !a->ref_len || !a->out) return "null lengths or output";
  if ((a->Lh > 0 && !a->hyp) || (a->Lr > 0 && !a->ref)) return "null token matrix";
  if (a->B > 1 && (a->ld_hyp < a->Lh || a->ld_ref < a->Lr)) return "row stride below the row width";
  return nullptr;
}
