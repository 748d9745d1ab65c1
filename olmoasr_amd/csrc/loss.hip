// Cross-entropy over the BPE vocabulary, forward + backward in one pass (gfx950, HBM-bound).
// Reference: F.cross_entropy(logits.view(-1, V+1), text_y.view(-1), ignore_index=51864) / accumulation_steps
// (scripts/training/train_timestamps.py:1444-1450) on logits that the reference produced in bf16 and then
// .float()-ed (olmoasr/model.py:768-770); the gradient it back-propagates into the tied-logits matmul is bf16.
// One 1024-thread workgroup per token row: the 51865 bf16 logits (104 KB) are read ONCE into registers
// (7 x 16 bytes per thread), softmax statistics in fp32, and (softmax - onehot) * g is written back in place
// as bf16 -> 2 * 2 * V bytes of HBM traffic per row, no fp32 logits tensor ever exists.
#include "kernels.h"

namespace {

// Workgroup width (scripts/ce_bench.py, [57344, 51968] bf16, every row valid, one MI355X): 256 threads x 26 chunks = 146 VGPRs, three rows
// per CU: 2.66 ms; 512 x 13: 2.54 ms; 1024 x 7 (62 VGPRs, 32 waves per CU): 2.42 ms = 4.93 TB/s = 0.62 of 8 TB/s.  (Round 2: 3.34 ms, with a
// per-element column test, a per-element onehot compare and the natural-base exponential in both passes.)
constexpr int CE_THREADS = 1024;
constexpr int CE_CHUNKS = 7;     // 7 * 1024 threads * 8 = 57344 >= 51968

// workgroup maximum / sum over the 8 waves of a cross-entropy workgroup, left in every thread (fixed combination order: deterministic)
__device__ __forceinline__ float block_reduce8(float v, float* red, bool is_max) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = is_max ? wave_max(v) : wave_sum(v);
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int w = 1; w < CE_THREADS / 64; ++w) r = is_max ? fmaxf(r, red[w]) : r + red[w];
  return r;
}

// REG = false is the plain objective and the kernel of every step that sets no regulariser.  REG = true (label smoothing eps, z-loss z;
// the formula: include/oasr.h at oasr_train_step_args.label_smoothing) is the same single pass with one more workgroup reduction, sum_{c<V} x_c,
// taken from the registers the maximum is taken from: full chunks add their eight values unguarded, and only the chunks that straddle V
// (the branch that already exists for the -inf overwrite) test columns -- there the padded columns add 0 to the sum and, in the epilogue,
// are written as exact zeros instead of -g eps / V (the tied-head GEMM reads them).
// The second __launch_bounds__ argument (waves per SIMD) holds REG at the plain kernel's two workgroups per CU: left alone it takes 66 VGPRs.
template <bool REG>
__global__ __launch_bounds__(CE_THREADS, REG ? 8 : 1) void ce_kernel(bf16_t* __restrict__ logits, long ld, int V, const int64_t* __restrict__ targets,
                                                 long ignore, float gscale, const int32_t* __restrict__ n_valid_dev,
                                                 float* __restrict__ row_loss, int write_grad, float eps, float zc,
                                                 float* __restrict__ parts, long parts_stride) {
  __shared__ float red[CE_THREADS / 64];
  const long row = blockIdx.x;
  bf16_t* lr = logits + row * ld;
  const long tgt = targets[row];
  const int nchunk = (int)(ld >> 3);
  // ignored row: zero gradient, zero loss (uniform branch).  A target outside [0, V) (F.cross_entropy would raise) is
  // treated the same way instead of reading / writing outside the row; hosts that want the raise validate ids up front.
  if (tgt == ignore || tgt < 0 || tgt >= V) {
    if (write_grad) {
      const u32x4_t z = {0u, 0u, 0u, 0u};
      for (int ch = threadIdx.x; ch < nchunk; ch += CE_THREADS) *(u32x4_t*)(lr + ch * 8) = z;
    }
    if (threadIdx.x == 0) {
      row_loss[row] = 0.f;
      if (REG && parts) parts[row] = parts[parts_stride + row] = 0.f;
    }
    return;
  }
  // The row is VALU-heavy once it sits in registers (two exponentials per logit), so the per-element work is kept minimal: columns
  // past V (the 128-padding of the tied head) are overwritten with -inf ONCE after the load -- they then drop out of the maximum,
  // contribute exp(-inf) = 0 to the sum and get a zero gradient without any per-element test -- the exponent runs in the log2
  // domain (one fma + v_exp_f32), and the "- onehot" of the target column is patched into the one chunk that holds it.
  constexpr float L2E = 1.4426950408889634f;
  u32x4_t v[CE_CHUNKS];
  float mx = -3.0e38f;
  float xs = 0.f;  // REG: this thread's share of sum_{c<V} x_c
#pragma unroll
  for (int c = 0; c < CE_CHUNKS; ++c) {
    const int ch = threadIdx.x + CE_THREADS * c;
    if (ch < nchunk) {
      v[c] = *(const u32x4_t*)(lr + ch * 8);
      if (ch * 8 + 8 > V) {  // (only the last ~13 chunks of a row)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int col = ch * 8 + 2 * i;
          if (REG) xs += (col < V ? bf_lo(v[c][i]) : 0.f) + (col + 1 < V ? bf_hi(v[c][i]) : 0.f);
          if (col >= V) v[c][i] = (v[c][i] & 0xffff0000u) | 0x0000ff80u;
          if (col + 1 >= V) v[c][i] = (v[c][i] & 0x0000ffffu) | 0xff800000u;
        }
      } else if (REG) {
#pragma unroll
        for (int i = 0; i < 4; ++i) xs += bf_lo(v[c][i]) + bf_hi(v[c][i]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) mx = fmaxf(mx, fmaxf(bf_lo(v[c][i]), bf_hi(v[c][i])));
    }
  }
  mx = block_reduce8(mx, red, true);
  const float nm2 = -mx * L2E;
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < CE_CHUNKS; ++c) {
    const int ch = threadIdx.x + CE_THREADS * c;
    if (ch < nchunk) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        sum += __builtin_amdgcn_exp2f(fmaf(bf_lo(v[c][i]), L2E, nm2)) + __builtin_amdgcn_exp2f(fmaf(bf_hi(v[c][i]), L2E, nm2));
    }
  }
  sum = block_reduce8(sum, red, false);
  // (here, next to its only use: reduced before the exponential pass, the sixteen partial sums stay live across it and spill)
  if (REG) xs = block_reduce8(xs, red, false);
  const float lse = mx + __logf(sum);
  const float ev = REG ? eps / (float)V : 0.f;  // eps / V: V is the class count, not ld
  if (threadIdx.x == 0) {
    const float nll = lse - bf2f(lr[tgt]);
    if (REG) {
      // lse - (1 - eps) x_t - eps / V sum x + z lse^2, written as the plain loss plus the two corrections
      row_loss[row] = nll + eps * bf2f(lr[tgt]) - ev * xs + zc * lse * lse;
      if (parts) {
        parts[row] = nll;
        parts[parts_stride + row] = lse * lse;
      }
    } else {
      row_loss[row] = nll;
    }
  }
  if (!write_grad) return;
  __syncthreads();  // lr[tgt] read above must precede the in-place overwrite
  const float g = gscale / (float)max(1, *n_valid_dev);
  const float sg = REG ? g * (1.f + 2.f * zc * lse) / sum : g / sum;  // softmax * g (* (1 + 2 z lse)) = exp2(..) * sg
  const float ge = g * ev, gt = REG ? g * (1.f - eps) : g;
  const int tch = (int)(tgt >> 3), tpos = (int)(tgt & 7);
#pragma unroll
  for (int c = 0; c < CE_CHUNKS; ++c) {
    const int ch = threadIdx.x + CE_THREADS * c;
    if (ch < nchunk) {
      float e[8];
      float tmin = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float t0 = fmaf(bf_lo(v[c][i]), L2E, nm2), t1 = fmaf(bf_hi(v[c][i]), L2E, nm2);
        tmin = fminf(tmin, fminf(t0, t1));
        e[2 * i] = __builtin_amdgcn_exp2f(t0) * sg;
        e[2 * i + 1] = __builtin_amdgcn_exp2f(t1) * sg;
      }
      // v_exp_f32 flushes a softmax below 2^-126 to zero, but its gradient is sg (up to ~gscale) times larger and can be a normal number:
      // a chunk that holds a logit more than 87 below the row maximum redoes those columns scaled by 2^64 (t + 64 is exact there).  Every
      // other chunk computes what it did before; the sum pass needs no such care (a flushed term is below 2^-126 of a sum >= 1).
      if (tmin < -126.f) {
        const float sgs = sg * 0x1p-64f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float t0 = fmaf(bf_lo(v[c][i]), L2E, nm2), t1 = fmaf(bf_hi(v[c][i]), L2E, nm2);
          if (t0 < -126.f) e[2 * i] = __builtin_amdgcn_exp2f(t0 + 64.f) * sgs;
          if (t1 < -126.f) e[2 * i + 1] = __builtin_amdgcn_exp2f(t1 + 64.f) * sgs;
        }
      }
      if (REG) {
#pragma unroll
        for (int i = 0; i < 8; ++i) e[i] -= ge;
        if (ch * 8 + 8 > V) {  // the padded columns' gradient stays bit-zero
#pragma unroll
          for (int i = 0; i < 8; ++i)
            if (ch * 8 + i >= V) e[i] = 0.f;
        }
      }
      if (ch == tch) {  // (one thread of the row)
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (i == tpos) e[i] -= gt;
      }
      u32x4_t o;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = pack_bf2(e[2 * i], e[2 * i + 1]);
      *(u32x4_t*)(lr + ch * 8) = o;
    }
  }
}

__global__ __launch_bounds__(256) void count_valid_kernel(const int64_t* __restrict__ t, long rows, long ignore, int V, int32_t* out) {
  __shared__ int red[4];
  int c = 0;
  // F.cross_entropy's denominator; the predicate is ce_kernel's (an id outside [0, V) contributes neither loss nor count)
  for (long i = threadIdx.x; i < rows; i += 256) c += (t[i] != ignore && t[i] >= 0 && t[i] < V) ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) *out = red[0] + red[1] + red[2] + red[3];
}

// deterministic single-block reduction (rows <= a few hundred thousand)
__global__ __launch_bounds__(256) void loss_reduce_kernel(const float* __restrict__ row_loss, long rows,
                                                          const int32_t* __restrict__ n_valid_dev, float mul,
                                                          float* __restrict__ loss_out, int accumulate) {
  __shared__ double red[4];
  double s = 0.0;
  for (long i = threadIdx.x; i < rows; i += 256) s += (double)row_loss[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double tot = (red[0] + red[1]) + (red[2] + red[3]);
    const float v = (float)(tot / (double)max(1, *n_valid_dev)) * mul;
    *loss_out = accumulate ? (*loss_out + v) : v;
  }
}

}  // namespace

int launch_count_valid(const int64_t* targets, long rows, long ignore, int V, int32_t* n_valid_dev, hipStream_t s) {
  OASR_REQUIRE(targets && n_valid_dev && rows > 0, "count_valid: bad args");
  hipLaunchKernelGGL(count_valid_kernel, dim3(1), dim3(256), 0, s, targets, rows, ignore, V, n_valid_dev);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}

int check_ce_reg(const char* who, float label_smoothing, float z_loss) {
  OASR_REQUIRE(label_smoothing >= 0.f && label_smoothing < 1.f, "%s: label_smoothing = %g must be finite and inside [0, 1)", who, (double)label_smoothing);
  OASR_REQUIRE(z_loss >= 0.f && z_loss <= 3.0e38f, "%s: z_loss = %g must be finite and >= 0", who, (double)z_loss);
  return OASR_OK;
}

int launch_cross_entropy(bf16_t* logits, long ld, int V, const int64_t* targets, long rows, long ignore, float gscale,
                         const int32_t* n_valid_dev, float* row_loss, int write_grad, hipStream_t s, const CeReg& reg) {
  OASR_REQUIRE(logits && targets && n_valid_dev && row_loss, "cross_entropy: null pointer");
  OASR_REQUIRE(ld % 8 == 0 && V <= ld && ld <= CE_CHUNKS * CE_THREADS * 8, "cross_entropy: ld=%ld V=%d unsupported", ld, V);
  OASR_REQUIRE(!reg.parts || reg.parts_stride >= rows, "cross_entropy: row_parts stride %ld below rows = %ld", reg.parts_stride, rows);
  if (rows <= 0) return OASR_OK;
  if (reg.on())
    hipLaunchKernelGGL(ce_kernel<true>, dim3((unsigned)rows), dim3(CE_THREADS), 0, s, logits, ld, V, targets, ignore, gscale, n_valid_dev,
                       row_loss, write_grad, reg.eps, reg.z, reg.parts, reg.parts_stride);
  else
    hipLaunchKernelGGL(ce_kernel<false>, dim3((unsigned)rows), dim3(CE_THREADS), 0, s, logits, ld, V, targets, ignore, gscale, n_valid_dev,
                       row_loss, write_grad, 0.f, 0.f, (float*)nullptr, 0L);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}

int launch_loss_reduce(const float* row_loss, long rows, const int32_t* n_valid_dev, float mul, float* loss_out, int accumulate,
                       hipStream_t s) {
  OASR_REQUIRE(row_loss && n_valid_dev && loss_out, "loss_reduce: null pointer");
  hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(256), 0, s, row_loss, rows, n_valid_dev, mul, loss_out, accumulate);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}
