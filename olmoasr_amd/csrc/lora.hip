// LoRA adapters in weight space.  An adapted Linear computes with W = W0 + s * B . A  (A [r, in], B [out, r],
// s = alpha / r).  The engine never runs the adapter as separate activation-side GEMMs: the compute copy of W is the effective weight
// (lora_merge), and the adapter gradients are projected out of the ordinary weight gradient dW = dL/dW (lora_grad):
//     dB = s * dW . A^T        dA = s * B^T . dW
// Both kernels are HBM-bound and deterministic (fixed summation orders, no float atomics).
#include "../../include/oasr.h"
#include "kernels.h"

namespace {

constexpr int MERGE_ROWS = 4;   // output rows per workgroup of lora_merge (each thread: 4 rows x 4 columns)
constexpr int GRAD_RG = 128;    // rows of dW per workgroup of lora_grad (a row group)
constexpr int GRAD_SUB = 32;    // rows staged in LDS at a time
constexpr int GRAD_SLAB = 256;  // columns per workgroup (a slab): one column per thread

// out[o][i] = fmaf(s, sum_k B[o][k] * A[k][i], W0[o][i]) with the k sum an fp32 FMA chain in ascending k.  out32 (fp32, may alias w0)
// or out16 (bf16, rounded like launch_cast_f32_bf16).  Every caller -- shadow refresh, master merge, module-level call -- runs this
// one expression, so a merged model's compute copy is bit-identical to the adapted model's.
__global__ __launch_bounds__(256) void lora_merge_kernel(const float* w0, const float* __restrict__ A, const float* __restrict__ Bm, float* out32,
                                                         bf16_t* __restrict__ out16, int rows, int cols, int r, float s) {
  const int o0 = blockIdx.x * MERGE_ROWS;
  const int i = (blockIdx.y * 256 + threadIdx.x) * 4;
  if (i >= cols) return;
  const int nrow = min(MERGE_ROWS, rows - o0);
  f32x4_t acc[MERGE_ROWS];
  for (int j = 0; j < MERGE_ROWS; ++j) acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < r; ++k) {
    const f32x4_t a = *(const f32x4_t*)(A + (long)k * cols + i);
#pragma unroll
    for (int j = 0; j < MERGE_ROWS; ++j) {
      const float b = j < nrow ? Bm[(long)(o0 + j) * r + k] : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[j][e] = fmaf(b, a[e], acc[j][e]);
    }
  }
  for (int j = 0; j < nrow; ++j) {
    const long at = (long)(o0 + j) * cols + i;
    const f32x4_t w = *(const f32x4_t*)(w0 + at);
    f32x4_t v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaf(s, acc[j][e], w[e]);
    if (out16) {
      uint32_t* o = (uint32_t*)(out16 + at);  // (at is a multiple of 4 elements: 8-byte aligned)
      o[0] = pack_bf2(v[0], v[1]);
      o[1] = pack_bf2(v[2], v[3]);
    } else {
      *(f32x4_t*)(out32 + at) = v;
    }
  }
}

// Pass 1 of lora_grad.  Workgroup (g, c) reads rows [g*128, +128) x columns [c*256, +256) of dW exactly once (32 rows at a time through
// LDS) and writes two partial sums:
//   partA[g][k][i]   = sum_{o in row group g} B[o][k] * dW[o][i]          (thread = column i, o ascending)
//   partB[c][o][k]   = sum_{i in column slab c} dW[o][i] * A[k][i]        (thread = (o, k) pairs, i ascending)
__global__ __launch_bounds__(256) void lora_grad_part_kernel(const float* __restrict__ dW, const float* __restrict__ A, const float* __restrict__ Bm,
                                                             float* __restrict__ partA, float* __restrict__ partB, int rows, int cols, int r) {
  // 107.5 KB at the largest rank: one workgroup per CU (a target launches 32-128 of them)
  __shared__ __attribute__((aligned(16))) float tile[GRAD_SUB * GRAD_SLAB];                     // [GRAD_SUB][GRAD_SLAB]
  __shared__ __attribute__((aligned(16))) float as[OASR_LORA_MAX_RANK * (GRAD_SLAB + 4)];      // [r][GRAD_SLAB + 4]: padded rows (the (o, k)
                                                                                               // pairs of a wave read r different rows)
  __shared__ float bs[GRAD_SUB * OASR_LORA_MAX_RANK];                                          // [GRAD_SUB][r]
  const int lda = GRAD_SLAB + 4;
  const int t = threadIdx.x, g = blockIdx.x, c = blockIdx.y;
  const int c0 = c * GRAD_SLAB, cn = min(GRAD_SLAB, cols - c0);
  const int i = c0 + t;
  for (int e = t; e < r * GRAD_SLAB; e += 256) {
    const int k = e / GRAD_SLAB, cc = e % GRAD_SLAB;
    as[k * lda + cc] = cc < cn ? A[(long)k * cols + c0 + cc] : 0.f;
  }
  float acc[OASR_LORA_MAX_RANK];
#pragma unroll
  for (int k = 0; k < OASR_LORA_MAX_RANK; ++k) acc[k] = 0.f;
  const int g0 = g * GRAD_RG, gn = min(GRAD_RG, rows - g0);
  for (int s0 = 0; s0 < gn; s0 += GRAD_SUB) {
    const int sn = min(GRAD_SUB, gn - s0);
    __syncthreads();  // (the previous sub-batch's readers are done with tile / bs)
    for (int e = t; e < GRAD_SUB * r; e += 256) {
      const int j = e / r, k = e % r;
      bs[e] = j < sn ? Bm[(long)(g0 + s0 + j) * r + k] : 0.f;
    }
    for (int j = 0; j < GRAD_SUB; ++j) tile[j * GRAD_SLAB + t] = (j < sn && t < cn) ? dW[(long)(g0 + s0 + j) * cols + i] : 0.f;
    __syncthreads();
    // dA partial of column i
#pragma unroll
    for (int k = 0; k < OASR_LORA_MAX_RANK; ++k) {
      if (k < r) {
        float a = acc[k];
        for (int j = 0; j < GRAD_SUB; ++j) a = fmaf(bs[j * r + k], tile[j * GRAD_SLAB + t], a);
        acc[k] = a;
      }
    }
    // dB partials of this sub-batch's (row, k) pairs over the slab
    for (int p = t; p < sn * r; p += 256) {
      const int j = p / r, k = p % r;
      const f32x4_t* tr = (const f32x4_t*)(tile + j * GRAD_SLAB);
      const f32x4_t* ar = (const f32x4_t*)(as + k * lda);
      float sum = 0.f;
      for (int q = 0; q < GRAD_SLAB / 4; ++q) {
        const f32x4_t x = tr[q], y = ar[q];
        sum = fmaf(x[0], y[0], sum);
        sum = fmaf(x[1], y[1], sum);
        sum = fmaf(x[2], y[2], sum);
        sum = fmaf(x[3], y[3], sum);
      }
      partB[((long)c * rows + g0 + s0 + j) * r + k] = sum;
    }
  }
  if (t < cn)
    for (int k = 0; k < r; ++k) partA[((long)g * r + k) * cols + i] = acc[k];
}

// Pass 2: dA[k][i] += s * sum_g partA[g][k][i], dB[o][k] += s * sum_c partB[c][o][k] (g, c ascending): one thread per output element
// (a null dA / dB: that adapter is frozen, its gradient range is left alone).
__global__ __launch_bounds__(256) void lora_grad_reduce_kernel(const float* __restrict__ partA, const float* __restrict__ partB, float* __restrict__ dA,
                                                               float* __restrict__ dB, long nA, long nB, int nG, int nC, float s) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e < nA) {
    if (!dA) return;
    float sum = 0.f;
    for (int g = 0; g < nG; ++g) sum += partA[(long)g * nA + e];
    dA[e] = fmaf(s, sum, dA[e]);
  } else if (e < nA + nB) {
    if (!dB) return;
    const long f = e - nA;
    float sum = 0.f;
    for (int c = 0; c < nC; ++c) sum += partB[(long)c * nB + f];
    dB[f] = fmaf(s, sum, dB[f]);
  }
}

}  // namespace

int launch_lora_merge(const float* w0, const float* A, const float* B, int rows, int cols, int r, float scale, float* out32, bf16_t* out16,
                      hipStream_t st) {
  OASR_REQUIRE(w0 && A && B && (out32 != nullptr) != (out16 != nullptr), "lora_merge: bad args (exactly one of out32 / out16)");
  OASR_REQUIRE(rows > 0 && cols > 0 && (cols % 4) == 0 && r >= 1 && r <= OASR_LORA_MAX_RANK,
               "lora_merge: rows %d, cols %d (multiple of 4), rank %d (1..%d)", rows, cols, r, OASR_LORA_MAX_RANK);
  hipLaunchKernelGGL(lora_merge_kernel, dim3(cdiv(rows, MERGE_ROWS), cdiv(cols, 1024)), dim3(256), 0, st, w0, A, B, out32, out16, rows, cols, r,
                     scale);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}

size_t lora_grad_scratch_floats(int rows, int cols, int r) {
  return (size_t)cdiv(rows, GRAD_RG) * r * cols + (size_t)cdiv(cols, GRAD_SLAB) * rows * r;
}

int launch_lora_grad(const float* dW, const float* A, const float* B, int rows, int cols, int r, float scale, float* dA, float* dB, float* scratch,
                     hipStream_t st) {
  OASR_REQUIRE(dW && A && B && (dA || dB) && scratch, "lora_grad: null");
  OASR_REQUIRE(rows > 0 && cols > 0 && (cols % 4) == 0 && r >= 1 && r <= OASR_LORA_MAX_RANK,
               "lora_grad: rows %d, cols %d (multiple of 4), rank %d (1..%d)", rows, cols, r, OASR_LORA_MAX_RANK);
  const int nG = cdiv(rows, GRAD_RG), nC = cdiv(cols, GRAD_SLAB);
  float* partA = scratch;
  float* partB = scratch + (size_t)nG * r * cols;
  hipLaunchKernelGGL(lora_grad_part_kernel, dim3(nG, nC), dim3(256), 0, st, dW, A, B, partA, partB, rows, cols, r);
  OASR_LAUNCH_CHECK();
  const long nA = (long)r * cols, nB = (long)rows * r;
  hipLaunchKernelGGL(lora_grad_reduce_kernel, dim3(cdiv(nA + nB, 256)), dim3(256), 0, st, partA, partB, dA, dB, nA, nB, nG, nC, scale);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}

// ---- unit operators (op-level tests; module-level calls of an adapted Linear) -------------------------------------------------------
extern "C" int oasr_lora_merge_op(const float* w0, const float* A, const float* B, int rows, int cols, int rank, float scale, int out_dtype,
                                  void* out, void* stream) {
  OASR_REQUIRE(out && (out_dtype == OASR_DTYPE_BF16 || out_dtype == OASR_DTYPE_F32), "oasr_lora_merge_op: out / out_dtype");
  return launch_lora_merge(w0, A, B, rows, cols, rank, scale, out_dtype == OASR_DTYPE_F32 ? (float*)out : nullptr,
                           out_dtype == OASR_DTYPE_BF16 ? (bf16_t*)out : nullptr, (hipStream_t)stream);
}
extern "C" size_t oasr_lora_grad_scratch_bytes(int rows, int cols, int rank) {
  return rows > 0 && cols > 0 && rank > 0 ? lora_grad_scratch_floats(rows, cols, rank) * sizeof(float) : 0;
}
extern "C" int oasr_lora_grad_op(const float* dW, const float* A, const float* B, int rows, int cols, int rank, float scale, float* dA, float* dB,
                                 void* scratch, void* stream) {
  return launch_lora_grad(dW, A, B, rows, cols, rank, scale, dA, dB, (float*)scratch, (hipStream_t)stream);
}
