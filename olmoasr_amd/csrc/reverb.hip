// Reverberation of int16 PCM (include/oasr.h at oasr_reverb; the rule: reverb_core.h): each drawn clip convolved with a bank row, exactly, on
// the integer matrix cores, in two launches with no host round trip, no memset and no atomics.
//
// The sum S[n] = sum_k tap(k) x(n + d - k) is a block-Toeplitz GEMM.  For a tile of 256 outputs n = n0 + 16 a + b (a, b < 16)
//     D[b, a] = sum_c sum_{j < 16} T_c[b, j] X_c[j, a],     T_c[b, j] = tap(16 c + b - j) (zero outside [0, K)),
//                                                           X_c[j, a] = x(n0 + d + 16 (a - c) + j),        c = 0 .. (K + 14) / 16,
// and four blocks c make one v_mfma_i32_16x16x64_i8: lane l (g = l >> 4) holds bytes j = 0 .. 15 of block c = 4 s + g of row / column l & 15
// in both operands, so the B fragment of a lane is 16 consecutive bytes of a byte plane of x at a 16-byte-aligned address in LDS.  (The
// result does not depend on which k the hardware gives a lane's byte j as long as it is the same k for A and B; the planted-tap tests cover
// every (b - j, c).)  Both operands go in as signed byte digits (reverb_core.h): three int32 accumulators per tile, four MFMAs per k-step,
// combined in 64 bits in the epilogue.
//   expand   one wave per (bank row, k-step): the A fragments of both tap digits, lane by lane as the MFMA takes them, into
//            workspace[row][k-step][digit][lane] (16 bytes each), and one more wave per row for sum_k tap(k).  It depends on the bank alone.
//   reverb   one workgroup of four waves per REVERB_WG_OUT = 4096 consecutive samples of a clip.  It evaluates the clip's plan itself (two
//            hashes), stages the x window [n0 + d - 16 (4 NS - 1), n0 + d + 4096) as two byte planes in LDS (zeros outside [0, n_valid) are
//            encoded like any sample), then each wave runs the NS k-steps over its four tiles: the A fragments come from the expanded image
//            (L2-resident: every workgroup of the call reads the same few rows), fetched one k-step ahead, the B fragments from LDS.  A clip
//            that is not reverberated, and samples at or behind n_valid, are copied.
#include "common.h"
#include "kernels.h"
#include "../../include/oasr.h"
#include "reverb_core.h"
#include "pcm_tile.h"

typedef __attribute__((ext_vector_type(4))) int i32x4_t;

#define REVERB_THREADS 256
#define REVERB_WAVES (REVERB_THREADS / 64)
#define REVERB_TILE 256  // outputs of one MFMA tile: D is 16 x 16
#define REVERB_TPW 4     // tiles per wave: an A fragment serves all of them
#define REVERB_WG_OUT (REVERB_WAVES * REVERB_TPW * REVERB_TILE)
#define REVERB_FRAG_BYTES (64 * 16)  // one operand of one MFMA: 16 bytes per lane

static inline int reverb_ksteps(int K) { return (((K + 14) / 16 + 1) + 3) / 4; }  // NS: blocks c = 0 .. (K + 14) / 16, four to a k-step
#define REVERB_MAX_KSTEPS 129                                                    // reverb_ksteps(REVERB_MAX_K)
#define REVERB_MAX_WIN (16 * (4 * REVERB_MAX_KSTEPS - 1) + REVERB_WG_OUT)        // samples of x one workgroup stages
__host__ __device__ static inline size_t reverb_image_offset(int R) { return ((size_t)R * sizeof(int64_t) + 15) & ~(size_t)15; }  // behind the R tap sums
size_t reverb_workspace_bytes(int R, int K) { return reverb_image_offset(R) + (size_t)R * (size_t)reverb_ksteps(K) * 2 * REVERB_FRAG_BYTES; }

__global__ __launch_bounds__(64) void reverb_expand_kernel(oasr_reverb_args a, int NS) {
  const int lane = threadIdx.x, r = blockIdx.y, s = blockIdx.x, K = a.K;
  const int16_t* taps = a.rir + (size_t)r * (size_t)a.ld_rir;
  if (s == NS) {  // the row's tap sum
    long long sum = 0;
    for (int k = lane; k < K; k += 64) sum += reverb_tap(taps[k]);
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) ((int64_t*)a.workspace)[r] = sum;
    return;
  }
  const int c = 4 * s + (lane >> 4), b = lane & 15;
  i32x4_t hi = {0, 0, 0, 0}, lo = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int k = 16 * c + b - j;
    const int tap = (k >= 0 && k < K) ? reverb_tap(taps[k]) : 0;
    hi[j >> 2] |= (reverb_tap_hi(tap) & 255) << (8 * (j & 3));
    lo[j >> 2] |= (reverb_tap_lo(tap) & 255) << (8 * (j & 3));
  }
  i32x4_t* img = (i32x4_t*)((char*)a.workspace + reverb_image_offset(a.R)) + ((size_t)r * (size_t)NS + (size_t)s) * 128;
  img[lane] = hi, img[64 + lane] = lo;
}

__global__ __launch_bounds__(REVERB_THREADS) void reverb_kernel(oasr_reverb_args a, int NS) {
  __shared__ __attribute__((aligned(16))) unsigned char s_xh[REVERB_MAX_WIN], s_xs[REVERB_MAX_WIN];
  const int tid = threadIdx.x, b = blockIdx.y, N = a.N;
  const int n0 = blockIdx.x * REVERB_WG_OUT;  // (N <= 2^26: no overflow)
  const int nv = a.n_valid[b];
  const ReverbPlan pl = reverb_plan(a.seed, a.first_clip + (uint64_t)b, a.policy.prob_q16, a.R);
  const bool wet = pl.drawn && nv >= 1 && nv <= N;  // (the same for every thread of the workgroup)
  if (blockIdx.x == 0 && tid == 0 && a.row_out) a.row_out[b] = wet ? pl.r : -1;
  const int16_t* __restrict__ x = a.pcm_in + (size_t)b * (size_t)a.ld_in;
  int16_t* __restrict__ y = a.pcm_out + (size_t)b * (size_t)a.ld_out;
  if (!wet || n0 >= nv) {
    const int end = n0 + REVERB_WG_OUT < N ? n0 + REVERB_WG_OUT : N;
    for (int n = n0 + tid; n < end; n += REVERB_THREADS) y[n] = x[n];
    return;
  }
  const int d = reverb_delay(a.delay[pl.r], a.K);
  const int back = 16 * (4 * NS - 1), win = back + REVERB_WG_OUT;  // win <= REVERB_MAX_WIN: NS <= REVERB_MAX_KSTEPS (the launcher's)
  const long w0 = (long)n0 + d - back;                            // the sample at byte 0 of both planes
  for (int p = 8 * tid; p < win; p += 8 * REVERB_THREADS) {       // (win is a multiple of 16)
    const s16x8_t v = pcm_load8(x, w0 + p, nv);
    u32x2_t h = {0, 0}, l = {0, 0};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const unsigned u = (unsigned short)v[e];
      h[e >> 2] |= (u >> 8) << (8 * (e & 3));             // reverb_x_hi as a signed byte
      l[e >> 2] |= ((u & 255u) ^ 128u) << (8 * (e & 3));  // reverb_x_lo = (x & 255) - 128 as a signed byte
    }
    *(u32x2_t*)(s_xh + p) = h, *(u32x2_t*)(s_xs + p) = l;
  }
  __syncthreads();

  const int lane = tid & 63, g = lane >> 4, col = lane & 15;
  const int tb = (tid >> 6) * (REVERB_TPW * REVERB_TILE);  // the wave's first output, from n0
  i32x4_t p_hh[REVERB_TPW], p_mid[REVERB_TPW], p_ll[REVERB_TPW];
#pragma unroll
  for (int t = 0; t < REVERB_TPW; ++t) p_hh[t] = p_mid[t] = p_ll[t] = i32x4_t{0, 0, 0, 0};
  if (n0 + tb < nv) {  // (per wave; a wave whose outputs all lie at or behind n_valid only copies)
    const i32x4_t* img = (const i32x4_t*)((const char*)a.workspace + reverb_image_offset(a.R)) + (size_t)pl.r * (size_t)NS * 128 + lane;
    i32x4_t a_hi = img[0], a_lo = img[64];
#pragma unroll 1
    for (int s = 0; s < NS; ++s) {
      const int nx = s + 1 < NS ? s + 1 : s;
      const i32x4_t n_hi = img[(size_t)nx * 128], n_lo = img[(size_t)nx * 128 + 64];
      const int base = back + tb + 16 * (col - (4 * s + g));  // >= 0 (4 s + g <= 4 NS - 1); base + 256 (TPW - 1) + 15 < win
#pragma unroll
      for (int t = 0; t < REVERB_TPW; ++t) {
        const i32x4_t x_hi = *(const i32x4_t*)(s_xh + base + REVERB_TILE * t), x_lo = *(const i32x4_t*)(s_xs + base + REVERB_TILE * t);
        p_hh[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_hi, x_hi, p_hh[t], 0, 0, 0);
        p_mid[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_lo, x_hi, p_mid[t], 0, 0, 0);
        p_mid[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_hi, x_lo, p_mid[t], 0, 0, 0);
        p_ll[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_lo, x_lo, p_ll[t], 0, 0, 0);
      }
      a_hi = n_hi, a_lo = n_lo;
    }
  }
  const int64_t tap_sum = ((const int64_t*)a.workspace)[pl.r];
#pragma unroll
  for (int t = 0; t < REVERB_TPW; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) {  // D[row 4 g + q][column col]: output 16 col + 4 g + q of the tile
      const int n = n0 + tb + REVERB_TILE * t + 16 * col + 4 * g + q;
      if (n < nv)
        y[n] = pcm_round_q15(reverb_combine(p_hh[t][q], p_mid[t][q], p_ll[t][q], tap_sum));
      else if (n < N)
        y[n] = x[n];
    }
}

int launch_reverb(const oasr_reverb_args* a, hipStream_t st) {
  const char* why = reverb_args_error(a);
  OASR_REQUIRE(!why, "oasr_reverb: %s", why);
  OASR_REQUIRE_WORKSPACE(a, 16, reverb_workspace_bytes(a->R, a->K), "oasr_reverb", "oasr_reverb_workspace_bytes");
  const int NS = reverb_ksteps(a->K);
  static_assert(REVERB_MAX_K == 8192 && REVERB_MAX_KSTEPS == ((8192 + 14) / 16 + 1 + 3) / 4, "REVERB_MAX_KSTEPS is reverb_ksteps(REVERB_MAX_K)");
  hipLaunchKernelGGL(reverb_expand_kernel, dim3((unsigned)NS + 1, (unsigned)a->R), dim3(64), 0, st, *a, NS);
  OASR_LAUNCH_CHECK();
  hipLaunchKernelGGL(reverb_kernel, dim3((unsigned)cdiv(a->N, REVERB_WG_OUT), (unsigned)a->B), dim3(REVERB_THREADS), 0, st, *a, NS);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}
