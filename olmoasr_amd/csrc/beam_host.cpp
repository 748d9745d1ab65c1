// oasr_beam_update_host / oasr_decode_reorder_host (include/oasr.h): the host twins of beam.hip -- the same duplicate rule, ranking, walk,
// pool cap and latch (beam_core.h), applied window by window.  The kernel's wave-parallel prefix comparison, its LDS hand-off and its
// coalesced row copies are covered by the GPU suite only.  Plain C++ (no HIP, no GPU call), so it serves CPU tensors and builds alone under
// a host sanitizer (tools/beam_host_check.cpp).
#include <string.h>

#include <vector>

#include "../../include/oasr.h"
#include "beam_core.h"

void oasr_set_error(const char* fmt, ...);

static_assert(OASR_BEAM_MAX == BEAM_MAX && OASR_BEAM_NOT_FULL == BEAM_NOT_FULL, "include/oasr.h and beam_core.h disagree");

extern "C" size_t oasr_sizeof_beam_args(void) { return sizeof(oasr_beam_args); }

extern "C" int oasr_beam_update_host(const oasr_beam_args* a) {
  if (const char* why = beam_args_error(a)) {
    oasr_set_error("oasr_beam_update_host: %s", why);
    return OASR_EINVAL;
  }
  const int B = a->beam, K = B + 1, n = B * K, len = a->len, C = a->max_candidates;
  const int64_t ld = a->n_ctx;
  const bool latched = beam_latched(a->pool_full_len, a->n_audio, len);  // (before any window of this step writes its word)
  for (int w = 0; w < a->n_audio; ++w) {
    const int64_t row0 = (int64_t)w * B;
    if (a->short_step[w]) continue;
    if (latched) {
      for (int j = 0; j < B; ++j) {
        memcpy(a->tokens_out + (row0 + j) * ld, a->tokens_in + (row0 + j) * ld, sizeof(int64_t) * len);
        a->sources[row0 + j] = (int32_t)(row0 + j);
      }
      continue;
    }
    int64_t tok[BEAM_MAX_CAND];
    double score[BEAM_MAX_CAND], escore[BEAM_MAX_CAND];
    uint8_t eq[BEAM_MAX * BEAM_MAX], first[BEAM_MAX_CAND];
    int16_t origin[BEAM_MAX_CAND], order[BEAM_MAX_CAND];
    for (int c = 0; c < n; ++c) {
      tok[c] = a->top_token[row0 * K + c];
      score[c] = beam_score(a->sums[row0 + c / K], a->top_logprob[row0 * K + c]);
    }
    for (int j1 = 0; j1 < B; ++j1)
      for (int j2 = 0; j2 < B; ++j2)
        eq[j1 * B + j2] = memcmp(a->tokens_in + (row0 + j1) * ld, a->tokens_in + (row0 + j2) * ld, sizeof(int64_t) * len) == 0;
    for (int c = 0; c < n; ++c) {
      int last = c;
      first[c] = beam_resolve(c, B, tok, eq, &last);
      escore[c] = score[last];
      origin[c] = (int16_t)(last / K);
      order[c] = -1;
    }
    for (int c = 0; c < n; ++c)
      if (first[c]) order[beam_rank(c, n, first, escore)] = (int16_t)c;
    const int count = a->pool_count[w];
    BeamWalk wk;
    beam_walk(order, n, tok, a->eot, B, count < C ? C - count : 0, &wk);
    if (wk.n_cont < B) {  // the host path's ragged tensor: nothing of the window is written
      a->short_step[w] = 1;
      continue;
    }
    for (int m = 0; m < B; ++m) {
      const int c = wk.cont[m];
      int64_t* out = a->tokens_out + (row0 + m) * ld;
      memcpy(out, a->tokens_in + (row0 + origin[c]) * ld, sizeof(int64_t) * len);
      out[len] = tok[c];
      a->sources[row0 + m] = (int32_t)(row0 + origin[c]);
      a->last_token[row0 + m] = tok[c];
    }
    for (int m = 0; m < B; ++m) a->sums[row0 + m] = (float)escore[wk.cont[m]];  // (every old sum was read into score[] above)
    for (int f = 0; f < wk.n_fin; ++f) {
      const int c = wk.fin[f];
      const int64_t slot = (int64_t)w * C + count + f;
      int64_t* out = a->pool_tokens + slot * ld;
      memcpy(out, a->tokens_in + (row0 + origin[c]) * ld, sizeof(int64_t) * len);
      out[len] = a->eot;
      a->pool_len[slot] = len + 1;
      a->pool_score[slot] = escore[c];
    }
    a->pool_count[w] = count + wk.n_fin;
    if (count < C && count + wk.n_fin >= C) a->pool_full_len[w] = len;
  }
  return OASR_OK;
}

extern "C" int oasr_decode_reorder_host(void* rows, int64_t layer_stride, int L, int B, int n_ctx, int d, int elem_size, int pos, int group,
                                        const int32_t* sources) {
  if (!rows || !sources || L < 1 || B < 1 || n_ctx < 1 || d < 1 || (elem_size != 2 && elem_size != 4) || pos < 0 || pos > n_ctx || group < 1 ||
      group > BEAM_MAX || B % group != 0 || layer_stride < (int64_t)B * n_ctx * 3 * d * elem_size) {
    oasr_set_error("oasr_decode_reorder_host: bad args (1 <= group <= %d dividing B, 0 <= pos <= n_ctx, elem_size 2 or 4, layer_stride >= one layer)", BEAM_MAX);
    return OASR_EINVAL;
  }
  const int bad = beam_sources_error(sources, B, group);
  if (bad >= 0) {
    oasr_set_error("oasr_decode_reorder_host: row %d continues row %d, outside its group of %d rows (beams never cross windows)", bad, sources[bad], group);
    return OASR_EINVAL;
  }
  const size_t kv = (size_t)2 * d * elem_size, row = (size_t)3 * d * elem_size;  // the k | v columns of one position
  std::vector<char> held((size_t)group * kv);
  for (int l = 0; l < L; ++l)
    for (int g0 = 0; g0 < B; g0 += group)
      for (int p = 0; p < pos; ++p) {
        char* base = (char*)rows + (size_t)l * layer_stride + (size_t)p * row + (size_t)d * elem_size;
        for (int g = 0; g < group; ++g) memcpy(&held[g * kv], base + (size_t)sources[g0 + g] * n_ctx * row, kv);  // every source first
        for (int g = 0; g < group; ++g) memcpy(base + (size_t)(g0 + g) * n_ctx * row, &held[g * kv], kv);
      }
  return OASR_OK;
}
