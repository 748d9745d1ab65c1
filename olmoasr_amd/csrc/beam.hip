// Device-resident beam search (include/oasr.h at oasr_beam_update / oasr_decode_reorder; the rule: beam_core.h).
//
// beam_update_kernel: ONE 256-thread workgroup per audio window, one thread per candidate (B * K <= 240).  The B x B prefix-equality matrix
// is built in LDS by the four waves (a wave strides over the `len` tokens of a pair and votes); each candidate thread then resolves its
// duplicates and counts its rank with the functions the host twin uses, thread 0 walks the ranked entries, and the whole workgroup copies
// the B source rows (and the pool's new rows) coalesced into the OTHER token buffer -- rows are gathered, so they cannot move in place.
// Every sum is read into LDS (as a candidate's double score) before any is written.  Windows never talk to each other inside a launch:
// the completion latch compares the other windows' pool_full_len with this step's own `len` (beam_core.h), which a concurrent writer
// cannot flip.
//
// kv_reorder_kernel: rearrange_kv_cache in place.  One thread owns one 16-byte column chunk of one (layer, group, position): it loads that
// chunk from the source row of every row of its group (at most 15 x 16 B in registers) and only then stores, so a row that is both a
// source and a destination is safe, and no other thread touches those bytes.
#include <hip/hip_runtime.h>

#include "../../include/oasr.h"
#include "beam_core.h"
#include "kernels.h"

static_assert(OASR_BEAM_MAX == BEAM_MAX && OASR_BEAM_NOT_FULL == BEAM_NOT_FULL, "include/oasr.h and beam_core.h disagree");

namespace {

constexpr int BEAM_THREADS = 256;

__global__ __launch_bounds__(BEAM_THREADS) void beam_update_kernel(oasr_beam_args a) {
  __shared__ int64_t tok[BEAM_MAX_CAND];
  __shared__ double escore[BEAM_MAX_CAND];  // a candidate's own score, then (behind the barrier) its entry's resolved score
  __shared__ double score[BEAM_MAX_CAND];
  __shared__ uint8_t eq[BEAM_MAX * BEAM_MAX], first[BEAM_MAX_CAND];
  __shared__ int16_t origin[BEAM_MAX_CAND], order[BEAM_MAX_CAND];
  __shared__ BeamWalk wk;
  __shared__ int s_latched, s_count;
  const int w = blockIdx.x, tid = threadIdx.x;
  const int B = a.beam, K = B + 1, n = B * K, len = a.len, C = a.max_candidates;
  const int64_t ld = a.n_ctx, row0 = (int64_t)w * B;
  if (a.short_step[w]) return;  // (uniform; written by this window's own workgroup in an earlier launch only)
  if (tid == 0) s_latched = beam_latched(a.pool_full_len, a.n_audio, len), s_count = a.pool_count[w];
  if (tid < n) {
    tok[tid] = a.top_token[row0 * K + tid];
    score[tid] = beam_score(a.sums[row0 + tid / K], a.top_logprob[row0 * K + tid]);
  }
  __syncthreads();
  if (s_latched) {  // every pool was full before this step: the rows pass through unchanged
    for (int j = 0; j < B; ++j)
      for (int i = tid; i < len; i += BEAM_THREADS) a.tokens_out[(row0 + j) * ld + i] = a.tokens_in[(row0 + j) * ld + i];
    if (tid < B) a.sources[row0 + tid] = (int32_t)(row0 + tid);
    return;
  }
  // prefix equality: pair p = (j1 < j2) by wave, tokens by lane
  {
    const int wave = tid >> 6, lane = tid & 63;
    int p = 0;
    for (int j1 = 0; j1 < B; ++j1)
      for (int j2 = j1; j2 < B; ++j2, ++p) {
        if ((p & 3) != wave) continue;  // (uniform per wave)
        int diff = 0;
        if (j1 != j2)
          for (int i = lane; i < len; i += 64) diff |= a.tokens_in[(row0 + j1) * ld + i] != a.tokens_in[(row0 + j2) * ld + i];
        const bool same = !__any(diff);
        if (lane == 0) eq[j1 * B + j2] = same, eq[j2 * B + j1] = same;
      }
  }
  __syncthreads();
  if (tid < n) {
    int last = tid;
    const bool f = beam_resolve(tid, B, tok, eq, &last);
    first[tid] = f;
    escore[tid] = score[last];
    origin[tid] = (int16_t)(last / K);
    order[tid] = -1;
  }
  __syncthreads();
  if (tid < n && first[tid]) order[beam_rank(tid, n, first, escore)] = (int16_t)tid;
  __syncthreads();
  if (tid == 0) beam_walk(order, n, tok, a.eot, B, s_count < C ? C - s_count : 0, &wk);
  __syncthreads();
  if (wk.n_cont < B) {  // a short step: nothing of the window is written
    if (tid == 0) a.short_step[w] = 1;
    return;
  }
  for (int m = 0; m < B; ++m) {
    const int c = wk.cont[m];
    const int64_t* src = a.tokens_in + (row0 + origin[c]) * ld;
    int64_t* out = a.tokens_out + (row0 + m) * ld;
    for (int i = tid; i < len; i += BEAM_THREADS) out[i] = src[i];
    if (tid == 0) out[len] = tok[c];
  }
  if (tid < B) {
    const int c = wk.cont[tid];
    a.sums[row0 + tid] = (float)escore[c];  // (every old sum went into score[] before the first barrier)
    a.sources[row0 + tid] = (int32_t)(row0 + origin[c]);
    a.last_token[row0 + tid] = tok[c];
  }
  for (int f = 0; f < wk.n_fin; ++f) {
    const int c = wk.fin[f];
    const int64_t slot = (int64_t)w * C + s_count + f;
    const int64_t* src = a.tokens_in + (row0 + origin[c]) * ld;
    int64_t* out = a.pool_tokens + slot * ld;
    for (int i = tid; i < len; i += BEAM_THREADS) out[i] = src[i];
    if (tid == 0) out[len] = a.eot, a.pool_len[slot] = len + 1, a.pool_score[slot] = escore[c];
  }
  if (tid == 0 && wk.n_fin > 0) {
    a.pool_count[w] = s_count + wk.n_fin;
    if (s_count + wk.n_fin >= C) a.pool_full_len[w] = len;  // (s_count < C here: a full pool takes nothing)
  }
}

constexpr int REORDER_THREADS = 256;

// grid (chunk blocks, groups, layers); chunks = pos * chunks_per_row 16-byte chunks of the k | v columns
__global__ __launch_bounds__(REORDER_THREADS) void kv_reorder_kernel(char* rows, long layer_stride, long seq_stride, long pos_stride, long kv_offset,
                                                                     int chunks_per_row, long chunks, int group, const int32_t* sources) {
  const long chunk = (long)blockIdx.x * REORDER_THREADS + threadIdx.x;
  if (chunk >= chunks) return;
  const int g0 = blockIdx.y * group;
  int src[BEAM_MAX];
  bool moves = false, ok = true;
#pragma unroll
  for (int g = 0; g < BEAM_MAX; ++g) {
    src[g] = g0 + g;
    if (g < group) {
      src[g] = sources[g0 + g];
      ok &= src[g] >= g0 && src[g] < g0 + group;
      moves |= src[g] != g0 + g;
    }
  }
  if (!ok || !moves) return;  // the identity, or an index that leaves the group (refused on the host where it is readable): no store
  const long p = chunk / chunks_per_row, col = chunk % chunks_per_row;
  char* base = rows + (long)blockIdx.z * layer_stride + p * pos_stride + kv_offset + col * 16;
  uint4 held[BEAM_MAX];
#pragma unroll
  for (int g = 0; g < BEAM_MAX; ++g)
    if (g < group) held[g] = *(const uint4*)(base + (long)src[g] * seq_stride);
#pragma unroll
  for (int g = 0; g < BEAM_MAX; ++g)
    if (g < group && src[g] != g0 + g) *(uint4*)(base + (long)(g0 + g) * seq_stride) = held[g];
}

}  // namespace

int launch_beam_update(const oasr_beam_args* a, hipStream_t st) {
  const char* why = beam_args_error(a);
  OASR_REQUIRE(!why, "oasr_beam_update: %s", why);
  hipLaunchKernelGGL(beam_update_kernel, dim3(a->n_audio), dim3(BEAM_THREADS), 0, st, *a);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}

int launch_kv_reorder(void* rows, long layer_stride, int L, int B, int n_ctx, int d, int elem_size, int pos, int group, const int32_t* sources,
                      hipStream_t st) {
  OASR_REQUIRE(rows && sources && L >= 1 && L <= 65535 && B >= 1 && n_ctx >= 1 && d >= 1 && (elem_size == 2 || elem_size == 4),
               "oasr_decode_reorder: bad args");
  OASR_REQUIRE(group >= 1 && group <= BEAM_MAX && B % group == 0 && B / group <= 65535, "oasr_decode_reorder: 1 <= group <= %d must divide B = %d", BEAM_MAX, B);
  OASR_REQUIRE(pos >= 0 && pos <= n_ctx, "oasr_decode_reorder: pos = %d outside [0, %d]", pos, n_ctx);
  OASR_REQUIRE((long)d * elem_size % 16 == 0 && ((uintptr_t)rows & 15) == 0 && layer_stride % 16 == 0,
               "oasr_decode_reorder: the k | v columns must be 16-byte aligned (d = %d, %d-byte elements)", d, elem_size);
  if (pos == 0 || group == 1) return OASR_OK;  // nothing cached yet / a group of one row can only continue itself
  const int chunks_per_row = 2 * d * elem_size / 16;
  const long chunks = (long)pos * chunks_per_row, pos_stride = (long)3 * d * elem_size;
  hipLaunchKernelGGL(kv_reorder_kernel, dim3(cdiv(chunks, REORDER_THREADS), B / group, L), dim3(REORDER_THREADS), 0, st, (char*)rows, layer_stride,
                     pos_stride * n_ctx, pos_stride, (long)d * elem_size, chunks_per_row, chunks, group, sources);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}
