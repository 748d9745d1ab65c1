// Teacher-forced predictions of the span step (include/oasr.h at oasr_train_step_args.pred_out): pred[b, s] = argmax_c logits[row(b, s)][c]
// over c < V, the lowest index among equal maxima -- gen_pred's argmax (train_timestamps.py:1077) taken from the logits in the compute dtype
// before the cross-entropy overwrites them with their gradient.
//
// One 256-thread workgroup per LOGICAL position (b, s).  Positions at or past span[b] (a multiple of 64) store -1 and leave; the others find
// their row through the chunk-row table, rows[b][s >> 6] + (s & 63), the mapping build_span_tables_kernel and the embedding use, so the
// output needs no un-permutation.  The row is read once in 16-byte pieces (8 bf16 / 4 fp32 columns; column by column where the rows are not
// 16-byte aligned, as in the fp32 validation engine, whose ld is V itself); a thread walks its columns in ascending
// order and replaces its best only on a strictly greater value, the merges prefer the lower index on equal values, so the result is
// torch.argmax's on the same numbers.  Columns [V, ld) -- the padding of the tied head -- are never candidates.  HBM-bound: 2 V bytes per
// active row in bf16, 4 bytes written.
#include "kernels.h"

namespace {

constexpr int AM_THREADS = 256;

struct Best {
  float v;
  int i;
};
__device__ __forceinline__ void am_take(Best& a, float v, int i) {  // (ascending i within a thread: strict)
  if (v > a.v) a.v = v, a.i = i;
}
__device__ __forceinline__ void am_merge(Best& a, float v, int i) {
  if (v > a.v || (v == a.v && i < a.i)) a.v = v, a.i = i;
}

// the 16-byte piece `ch` of a row: columns [ch * N, ch * N + N), those >= V skipped
__device__ __forceinline__ void am_piece(const bf16_t* lr, int ch, int V, Best& best) {
  const u32x4_t p = *(const u32x4_t*)(lr + ch * 8);
  const int c0 = ch * 8;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (c0 + 2 * k < V) am_take(best, bf_lo(p[k]), c0 + 2 * k);
    if (c0 + 2 * k + 1 < V) am_take(best, bf_hi(p[k]), c0 + 2 * k + 1);
  }
}
__device__ __forceinline__ void am_piece(const float* lr, int ch, int V, Best& best) {
  const f32x4_t p = *(const f32x4_t*)(lr + ch * 4);
  const int c0 = ch * 4;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (c0 + k < V) am_take(best, p[k], c0 + k);
}

__device__ __forceinline__ float am_value(bf16_t x) { return bf2f(x); }
__device__ __forceinline__ float am_value(float x) { return x; }

template <typename T, bool PIECES>
__global__ __launch_bounds__(AM_THREADS) void argmax_rows_kernel(const T* __restrict__ logits, long ld, int V, long n_rows,
                                                                 const int32_t* __restrict__ rows, const int32_t* __restrict__ span, int S,
                                                                 int32_t* __restrict__ pred) {
  constexpr int N = 16 / (int)sizeof(T);  // columns per piece
  __shared__ float bv[AM_THREADS / 64];
  __shared__ int bi[AM_THREADS / 64];
  const int b = blockIdx.x / S, s = blockIdx.x - b * S;  // (uniform)
  long row = -1;
  if (s < span[b]) row = (long)rows[b * OASR_ROWTAB + (s >> 6)] + (s & 63);
  if (row < 0 || row >= n_rows) {  // past the span (or a table entry that points outside the matrix): not computed, not read
    if (threadIdx.x == 0) pred[blockIdx.x] = -1;
    return;
  }
  const T* lr = logits + row * ld;
  Best best{-__builtin_huge_valf(), 0x7fffffff};
  if (PIECES) {
    const int npiece = (V + N - 1) / N;  // (launcher: ld >= npiece * N, rows 16-byte aligned)
#pragma unroll 4
    for (int ch = threadIdx.x; ch < npiece; ch += AM_THREADS) am_piece(lr, ch, V, best);
  } else {  // rows that are not 16-byte aligned (the fp32 validation engine keeps ld = V): one column at a time
    for (int c = threadIdx.x; c < V; c += AM_THREADS) am_take(best, am_value(lr[c]), c);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) am_merge(best, __shfl_xor(best.v, o, 64), __shfl_xor(best.i, o, 64));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) bv[wave] = best.v, bi[wave] = best.i;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < AM_THREADS / 64; ++w) am_merge(best, bv[w], bi[w]);
    pred[blockIdx.x] = best.i == 0x7fffffff ? 0 : best.i;  // (no column above -inf: index 0, as for an all-equal row)
  }
}

template <typename T>
int launch_argmax_rows_t(const T* logits, long ld, int V, long n_rows, const int32_t* rows, const int32_t* span, int B, int S, int32_t* pred,
                         hipStream_t st) {
  constexpr int N = 16 / (int)sizeof(T);
  OASR_REQUIRE(logits && rows && span && pred, "argmax_rows: null pointer");
  OASR_REQUIRE(B > 0 && S > 0 && S % 64 == 0 && S <= 64 * OASR_ROWTAB && (long)B * S <= 0x7fffffffL,
               "argmax_rows: need S %% 64 == 0, S <= %d and B * S within one grid (B=%d S=%d)", 64 * OASR_ROWTAB, B, S);
  OASR_REQUIRE(V > 0 && n_rows > 0 && ld >= V, "argmax_rows: V = %d, n_rows = %ld, ld = %ld (>= V)", V, n_rows, ld);
  // 16-byte pieces when every row starts on a 16-byte boundary and holds its last piece whole (the bf16 engine: ld = V rounded up to 128)
  const bool pieces = ld % N == 0 && ld >= (long)(V + N - 1) / N * N && ((uintptr_t)logits & 15) == 0;
  if (pieces)
    hipLaunchKernelGGL((argmax_rows_kernel<T, true>), dim3(B * S), dim3(AM_THREADS), 0, st, logits, ld, V, n_rows, rows, span, S, pred);
  else
    hipLaunchKernelGGL((argmax_rows_kernel<T, false>), dim3(B * S), dim3(AM_THREADS), 0, st, logits, ld, V, n_rows, rows, span, S, pred);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}

}  // namespace

int launch_argmax_rows(const bf16_t* logits, long ld, int V, long n_rows, const int32_t* rows, const int32_t* span, int B, int S, int32_t* pred,
                       hipStream_t st) {
  return launch_argmax_rows_t(logits, ld, V, n_rows, rows, span, B, S, pred, st);
}
int launch_argmax_rows(const float* logits, long ld, int V, long n_rows, const int32_t* rows, const int32_t* span, int B, int S, int32_t* pred,
                       hipStream_t st) {
  return launch_argmax_rows_t(logits, ld, V, n_rows, rows, span, B, S, pred, st);
}
