// Teacher-forced scoring of computed logits (include/oasr.h at oasr_score): per row the negative log-likelihood of its target and the argmax,
// from ONE read of the row, and per sample the totals of its rows.  Forward only: nothing is written but the caller's outputs.
//
// score_rows_kernel: one 1024-thread workgroup per position (b, s).  Positions at or past span[b] store (0, -1) and leave without reading
// their row.  The others read the row once in 16-byte pieces into registers (bf16: 7 pieces x 8 columns per thread, the width loss.hip
// measured for the cross-entropy kernel; fp32: 14 x 4); the piece that straddles V is built column by column with -inf in the columns
// [V, ld), which are never read -- they are no argmax candidate (the take is strict) and add exp(-inf) = 0 to the sum.  From those registers
// comes first the argmax (argmax.hip's rule: a thread walks its columns in ascending order and replaces its best only on a strictly greater
// value, the merges prefer the lower index, so the lowest index wins among equal maxima), whose value is the row maximum, and then, for a valid target only,
// sum_c exp(x_c - max) in the log2 domain as ce_kernel does.  row_nll = max + log(sum) - x_t with fp32 statistics; exactly 0 for an ignored
// or out-of-range target.  Rows that are not 16-byte aligned or longer than the registers hold (the fp32 validation engine keeps ld = V) go
// column by column and read the row a second time for the sum.  HBM-bound: 2 V bytes per active row in bf16, 8 bytes written.
//
// score_reduce_kernel: one wave per sample; the rule is score_core.h's, shared with the host twin.  The lanes stage the rows' values and
// flags into LDS, lane 0 adds them in ascending s -- the double sum is sequential by contract (bit-equal to the host twin), and S <= 448
// rows per sample are nothing beside the forward.
#include "kernels.h"
#include "score_core.h"

namespace {

constexpr int SC_THREADS = 1024;
constexpr int SC_WAVES = SC_THREADS / 64;
constexpr int SR_TILE = 512;

template <typename T>
struct Piece;
template <>
struct Piece<bf16_t> {
  using V4 = u32x4_t;
  static constexpr int N = 8, NP = 7;  // 7 * 1024 * 8 = 57344 columns
};
template <>
struct Piece<float> {
  using V4 = f32x4_t;
  static constexpr int N = 4, NP = 14;  // the same 57344 columns
};

struct Best {
  float v;
  int i;
};
__device__ __forceinline__ void sc_take(Best& a, float v, int i) {  // (ascending i within a thread: strict)
  if (v > a.v) a.v = v, a.i = i;
}
__device__ __forceinline__ void sc_merge(Best& a, float v, int i) {
  if (v > a.v || (v == a.v && i < a.i)) a.v = v, a.i = i;
}

// the piece that straddles V, starting at column c0: read column by column, the columns >= V are -inf and are not read
__device__ __forceinline__ u32x4_t sc_tail(const bf16_t* lr, int c0, int V) {
  u32x4_t p;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t lo = c0 + 2 * k < V ? (uint32_t)lr[c0 + 2 * k] : 0xff80u;
    const uint32_t hi = c0 + 2 * k + 1 < V ? (uint32_t)lr[c0 + 2 * k + 1] : 0xff80u;
    p[k] = lo | (hi << 16);
  }
  return p;
}
__device__ __forceinline__ f32x4_t sc_tail(const float* lr, int c0, int V) {
  f32x4_t p;
#pragma unroll
  for (int k = 0; k < 4; ++k) p[k] = c0 + k < V ? lr[c0 + k] : -__builtin_huge_valf();
  return p;
}
__device__ __forceinline__ void sc_piece_best(const u32x4_t& p, int c0, Best& best) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    sc_take(best, bf_lo(p[k]), c0 + 2 * k);
    sc_take(best, bf_hi(p[k]), c0 + 2 * k + 1);
  }
}
__device__ __forceinline__ void sc_piece_best(const f32x4_t& p, int c0, Best& best) {
#pragma unroll
  for (int k = 0; k < 4; ++k) sc_take(best, p[k], c0 + k);
}
constexpr float SC_L2E = 1.4426950408889634f;
__device__ __forceinline__ float sc_piece_exp(const u32x4_t& p, float nm2) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    s += __builtin_amdgcn_exp2f(fmaf(bf_lo(p[k]), SC_L2E, nm2)) + __builtin_amdgcn_exp2f(fmaf(bf_hi(p[k]), SC_L2E, nm2));
  return s;
}
__device__ __forceinline__ float sc_piece_exp(const f32x4_t& p, float nm2) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) s += __builtin_amdgcn_exp2f(fmaf(p[k], SC_L2E, nm2));
  return s;
}
__device__ __forceinline__ float sc_value(bf16_t x) { return bf2f(x); }
__device__ __forceinline__ float sc_value(float x) { return x; }

template <typename T, bool PIECES>
__global__ __launch_bounds__(SC_THREADS) void score_rows_kernel(const T* __restrict__ logits, long ld, int V, const int64_t* __restrict__ targets,
                                                                const int32_t* __restrict__ span, int S, long ignore,
                                                                float* __restrict__ row_nll, int32_t* __restrict__ pred) {
  using P = Piece<T>;
  __shared__ float bv[SC_WAVES];
  __shared__ int bi[SC_WAVES];
  __shared__ float red[SC_WAVES];
  const long r = blockIdx.x;
  const int b = (int)(r / S), s = (int)(r - (long)b * S);  // (uniform)
  if (s >= span[b]) {  // past the span: not computed, not read
    if (threadIdx.x == 0) row_nll[r] = 0.f, pred[r] = -1;
    return;
  }
  const T* lr = logits + r * ld;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long tgt = targets[r];
  const bool valid = sc_valid(tgt, V, ignore);  // (uniform)
  const int npiece = (V + P::N - 1) / P::N;     // (launcher, PIECES: npiece <= NP * SC_THREADS, rows 16-byte aligned)
  typename P::V4 v[P::NP];
  Best best{-__builtin_huge_valf(), 0x7fffffff};
  if (PIECES) {
#pragma unroll
    for (int c = 0; c < P::NP; ++c) {
      const int ch = threadIdx.x + SC_THREADS * c;
      if (ch < npiece) {
        if (ch * P::N + P::N > V) v[c] = sc_tail(lr, ch * P::N, V);  // (the last piece of the row only)
        else v[c] = *(const typename P::V4*)(lr + (long)ch * P::N);
        sc_piece_best(v[c], ch * P::N, best);
      }
    }
  } else {
    for (int c = threadIdx.x; c < V; c += SC_THREADS) sc_take(best, sc_value(lr[c]), c);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sc_merge(best, __shfl_xor(best.v, o, 64), __shfl_xor(best.i, o, 64));
  if (lane == 0) bv[wave] = best.v, bi[wave] = best.i;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < SC_WAVES; ++w) sc_merge(best, bv[w], bi[w]);  // (every thread: best.v is the row maximum)
  if (threadIdx.x == 0) pred[r] = best.i == 0x7fffffff ? 0 : best.i;  // (no column above -inf: index 0, as for an all-equal row)
  if (!valid) {
    if (threadIdx.x == 0) row_nll[r] = 0.f;
    return;
  }
  const float mx = best.v;
  const float nm2 = -mx * SC_L2E;
  float sum = 0.f;
  if (PIECES) {
#pragma unroll
    for (int c = 0; c < P::NP; ++c)
      if (threadIdx.x + SC_THREADS * c < npiece) sum += sc_piece_exp(v[c], nm2);
  } else {
    for (int c = threadIdx.x; c < V; c += SC_THREADS) sum += __builtin_amdgcn_exp2f(fmaf(sc_value(lr[c]), SC_L2E, nm2));
  }
  sum = wave_sum(sum);
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = red[0];
#pragma unroll
    for (int w = 1; w < SC_WAVES; ++w) tot += red[w];  // (fixed order: deterministic)
    row_nll[r] = (mx + __logf(tot)) - sc_value(lr[tgt]);
  }
}

__global__ __launch_bounds__(64) void score_reduce_kernel(const float* __restrict__ row_nll, const int32_t* __restrict__ pred,
                                                          const int64_t* __restrict__ targets, const int32_t* __restrict__ span, int S, int V,
                                                          long ignore, float* __restrict__ nll_sum, float* __restrict__ nll_max,
                                                          int32_t* __restrict__ n_tok, int32_t* __restrict__ n_hit) {
  __shared__ float nl[SR_TILE];
  __shared__ uint32_t fl[SR_TILE];
  const int b = blockIdx.x;
  const int n = sc_rows(span[b], S);  // (uniform)
  const long base = (long)b * S;
  ScoreAcc acc;
  sc_init(acc);
  for (int s0 = 0; s0 < n; s0 += SR_TILE) {
    const int m = n - s0 < SR_TILE ? n - s0 : SR_TILE;
    for (int i = threadIdx.x; i < m; i += 64) {
      const long at = base + s0 + i;
      nl[i] = row_nll[at];
      fl[i] = sc_flags(targets[at], pred[at], V, ignore);
    }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < m; ++i) sc_add(acc, nl[i], fl[i]);
    __syncthreads();
  }
  if (threadIdx.x == 0) sc_finish(acc, nll_sum + b, nll_max + b, n_tok + b, n_hit + b);
}

template <typename T>
int launch_score_rows_t(const T* logits, long ld, int V, const int64_t* targets, const int32_t* span, int B, int S, long ignore, float* row_nll,
                        int32_t* pred, hipStream_t st) {
  using P = Piece<T>;
  OASR_REQUIRE(logits && targets && span && row_nll && pred, "score_rows: null pointer");
  OASR_REQUIRE(B > 0 && S > 0 && (long)B * S <= 0x7fffffffL, "score_rows: B = %d and S = %d must be positive, B * S within one grid", B, S);
  OASR_REQUIRE(V > 0 && ld >= V, "score_rows: V = %d, ld = %ld (>= V)", V, ld);
  // 16-byte pieces held in registers when every row starts on a 16-byte boundary and fits the registers (no column >= V is read)
  const long npiece = ((long)V + P::N - 1) / P::N;
  const bool pieces = ld % P::N == 0 && ((uintptr_t)logits & 15) == 0 && npiece <= (long)P::NP * SC_THREADS;
  if (pieces)
    hipLaunchKernelGGL((score_rows_kernel<T, true>), dim3(B * S), dim3(SC_THREADS), 0, st, logits, ld, V, targets, span, S, ignore, row_nll, pred);
  else
    hipLaunchKernelGGL((score_rows_kernel<T, false>), dim3(B * S), dim3(SC_THREADS), 0, st, logits, ld, V, targets, span, S, ignore, row_nll, pred);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}

}  // namespace

int launch_score_rows(const bf16_t* logits, long ld, int V, const int64_t* targets, const int32_t* span, int B, int S, long ignore, float* row_nll,
                      int32_t* pred, hipStream_t st) {
  return launch_score_rows_t(logits, ld, V, targets, span, B, S, ignore, row_nll, pred, st);
}
int launch_score_rows(const float* logits, long ld, int V, const int64_t* targets, const int32_t* span, int B, int S, long ignore, float* row_nll,
                      int32_t* pred, hipStream_t st) {
  return launch_score_rows_t(logits, ld, V, targets, span, B, S, ignore, row_nll, pred, st);
}

int launch_score_reduce(const float* row_nll, const int32_t* pred, const int64_t* targets, const int32_t* span, int B, int S, int V, long ignore,
                        float* nll_sum, float* nll_max, int32_t* n_tok, int32_t* n_hit, hipStream_t st) {
  const char* why = sc_reduce_args_error(row_nll, pred, targets, span, B, S, V, nll_sum, nll_max, n_tok, n_hit);
  OASR_REQUIRE(!why, "oasr_score_reduce: %s", why);
  hipLaunchKernelGGL(score_reduce_kernel, dim3(B), dim3(64), 0, st, row_nll, pred, targets, span, S, V, ignore, nll_sum, nll_max, n_tok, n_hit);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}
