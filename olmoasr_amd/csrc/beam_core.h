// One beam-search update for one audio window (include/oasr.h at oasr_beam_update): the rule the device kernel (beam.hip) and the host
// twin (beam_host.cpp, oasr_beam_update_host) share, so that duplicate resolution, ranking, the walk, the pool cap and the completion
// latch are ONE text that the CPU suite exercises without a GPU.  Plain C++: no HIP header is needed to include this file.
//
// It restates whisper's BeamSearchDecoder.update as olmoasr_amd/decoding.py runs it on the host (dicts of tuples):
//   candidates   c = j * K + k for row j of the window and entry k of its top-K (K = B + 1), in that order.  The key of c is (prefix of row
//                j, token of c); its score is (double)sum_j + (double)logprob_c; its origin is j.
//   duplicates   equal keys collapse to ONE entry at the position of the first occurrence with the score and origin of the LAST (dict
//                assignment).  At the first sampled position every row is the same prefix; a row with fewer than K survivors returns
//                (0, -inf) more than once.
//   order        score descending, ties by position ascending (a stable sort; -inf == -inf).  NaN is outside the contract -- ranks may then
//                collide, which leaves a slot of the order empty and the walk skips it: nothing is ever indexed by a NaN.
//   walk         an entry whose token is eot is newly finished; any other is a continuation, the m-th becoming row m of the next step.  The
//                walk ends behind the B-th continuation.  Fewer than B continuations: the step is SHORT (the host path fails there).
//   pool         newly finished entries enter the window's pool in walk order while it holds fewer than C = max_candidates.
//   latch        pool_full_len[a] = the prefix length `len` of the step that filled window a's pool (BEAM_NOT_FULL before).  A step whose `len`
//                exceeds every window's pool_full_len is latched: it moves nothing.  The comparison with the step's own `len` is what makes the
//                word safe to read while other windows of the same step write theirs (they write `len` itself, which does not latch).
#pragma once
#include <stdint.h>

#include "../../include/oasr.h"
#include "core_hd.h"

#define BEAM_MAX 15                             // beams per window: the selection kernel returns K = B + 1 <= 16 candidates per row
#define BEAM_MAX_CAND (BEAM_MAX * (BEAM_MAX + 1))  // 240 candidates per window
#define BEAM_NOT_FULL 0x7fffffff

// what one walk decides: the candidates that continue (in row order of the next step) and the ones that enter the pool (in pool order)
struct BeamWalk {
  int32_t n_cont, n_fin;
  int16_t cont[BEAM_MAX];
  int16_t fin[BEAM_MAX];  // at most one eot entry per distinct prefix
};

OASR_HD double beam_score(float sum, float logprob) { return (double)sum + (double)logprob; }

// eq: B x B bytes, eq[j1 * B + j2] = the prefixes of rows j1 and j2 are equal over all `len` tokens
OASR_HD bool beam_same_key(int c1, int c2, int B, const int64_t* tok, const uint8_t* eq) {
  const int K = B + 1;
  return tok[c1] == tok[c2] && eq[(c1 / K) * B + c2 / K] != 0;
}

// Is candidate c the first occurrence of its key?  Then *last = the last occurrence (whose score and origin the entry takes).
OASR_HD bool beam_resolve(int c, int B, const int64_t* tok, const uint8_t* eq, int* last) {
  const int n = B * (B + 1);
  for (int p = 0; p < c; ++p)
    if (beam_same_key(p, c, B, tok, eq)) return false;
  int l = c;
  for (int q = c + 1; q < n; ++q)
    if (beam_same_key(c, q, B, tok, eq)) l = q;
  *last = l;
  return true;
}

// rank of entry c: how many entries precede it.  first[p] != 0 marks the entries, score[p] is an entry's (resolved) score.
OASR_HD int beam_rank(int c, int n, const uint8_t* first, const double* score) {
  const double s = score[c];
  int r = 0;
  for (int p = 0; p < n; ++p)
    if (first[p] && p != c && (score[p] > s || (score[p] == s && p < c))) ++r;
  return r;
}

// order[r] = the entry of rank r, or -1.  room = what the pool still takes (C - count, not below 0).
OASR_HD void beam_walk(const int16_t* order, int n, const int64_t* tok, int64_t eot, int B, int room, BeamWalk* w) {
  w->n_cont = 0, w->n_fin = 0;
  for (int r = 0; r < n; ++r) {
    const int c = order[r];
    if (c < 0) continue;
    if (tok[c] == eot) {
      if (w->n_fin < room && w->n_fin < BEAM_MAX) w->fin[w->n_fin++] = (int16_t)c;
    } else {
      w->cont[w->n_cont++] = (int16_t)c;
      if (w->n_cont == B) break;
    }
  }
}

// is a step at prefix length `len` latched?  (pool_full_len: int32 [n_audio])
OASR_HD bool beam_latched(const int32_t* pool_full_len, int n_audio, int len) {
  for (int a = 0; a < n_audio; ++a)
    if (pool_full_len[a] >= len) return false;
  return true;
}

// what both entry points refuse before anything is read or launched; null = fine
inline const char* beam_args_error(const oasr_beam_args* a) {
  if (!a) return "null argument block";
  if (a->n_audio < 1 || a->beam < 1 || a->beam > BEAM_MAX) return "n_audio >= 1 and 1 <= beam <= 15";
  if (a->max_candidates < 1) return "max_candidates >= 1";
  if (a->len < 1 || a->n_ctx < 2 || a->len >= a->n_ctx) return "1 <= len < n_ctx (the step appends one token)";
  if ((int64_t)a->n_audio * a->beam > 0x7fffffff / 16) return "n_audio * beam too large";
  if (!a->top_logprob || !a->top_token || !a->tokens_in || !a->tokens_out || a->tokens_in == a->tokens_out) return "null or aliased token buffers / candidates";
  if (!a->sums || !a->sources || !a->last_token) return "null sums, sources or last tokens";
  if (!a->pool_tokens || !a->pool_len || !a->pool_score || !a->pool_count || !a->pool_full_len || !a->short_step) return "null pool or status words";
  return nullptr;
}

// row j of a reorder continues row sources[j]: every source must lie in its destination's group of `group` rows (beams never cross
// windows: the cross-attention K/V do not move).  -1 = fine, else the first offending row.
OASR_HD int beam_sources_error(const int32_t* sources, int B, int group) {
  for (int j = 0; j < B; ++j) {
    const int lo = j / group * group;
    if (sources[j] < lo || sources[j] >= lo + group) return j;
  }
  return -1;
}
