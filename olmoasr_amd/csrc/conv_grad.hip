// conv1 input gradient: d(mel) of the encoder stage's backward (engine_bwd.h, backward_encoder).
//
// conv1 runs as a GEMM over overlapping windows of the time-major mel with the packed kernel w1p [d][256] (column k*n_mels + c = tap k of
// channel c).  Its data gradient comes out of one dgrad GEMM as the window columns dcol [B*T1][256] = d(u1) . w1p; this kernel folds them
// back onto the frames:
//     dmel[b][c][t] = sum_{k=0..2, 0 <= t+1-k < T1} dcol[b*T1 + t+1-k][k*n_mels + c]     (fp32 sum, fp32 channel-major output)
// Windows outside the sample -- the conv's zero padding, or the neighbouring sample's rows -- contribute nothing: the fold reads per sample.
//
// One workgroup per (clip, 32-frame tile): the tile's 34 window rows (32 + a one-row halo on each side; rows outside the sample are zero) are
// read with 16-byte loads along the columns, converted to fp32 into LDS, and read back transposed so that every lane owns 4 consecutive
// frames of one channel and writes them with one 16-byte store (8 lanes = 128 contiguous bytes of a channel row).
// LDS banks (ds_write_b32 / ds_read_b32: bank = dword % 32 over 32-lane halves): the row pitch is = 1 mod 8 dwords, so the 8 frame quads of a
// half-wave (rows 4q + j) land on banks 4q + const, and its 4 channels on the 4 banks next to them; the 16-byte chunks are stored rotated by
// one slot per 32/VEC chunks, so the VEC scalar writes of consecutive chunks spread over all 32 banks instead of hitting the same 4.
#include "kernels.h"

namespace {

constexpr int C1_TILE = 32;            // output frames per workgroup
constexpr int C1_ROWS = C1_TILE + 2;   // window rows t0-1 .. t0+32
constexpr int C1_THREADS = 256;

__device__ __forceinline__ void load16(const bf16_t* p, float* v) {
  const u32x4_t q = *(const u32x4_t*)p;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[2 * j] = bf_lo(q[j]);
    v[2 * j + 1] = bf_hi(q[j]);
  }
}
__device__ __forceinline__ void load16(const float* p, float* v) {
  const f32x4_t q = *(const f32x4_t*)p;
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = q[j];
}

// position of column `col` inside an LDS row: chunk ch = col / VEC keeps its VEC slots, rotated by ch / (32 / VEC)
template <int VEC>
__device__ __forceinline__ int c1_slot(int col) {
  const int ch = col / VEC;
  return ch * VEC + ((col + ch / (32 / VEC)) & (VEC - 1));
}

template <typename T>
__global__ __launch_bounds__(C1_THREADS) void conv1_col2im_mel_kernel(const T* __restrict__ dcol, float* __restrict__ dmel, int T1, int nm,
                                                                      int pitch) {
  extern __shared__ float c1_lds[];  // [C1_ROWS][pitch]
  constexpr int VEC = 16 / sizeof(T);
  const int b = blockIdx.y, t0 = blockIdx.x * C1_TILE;
  const int nch = 3 * nm / VEC;
  const T* src = dcol + (long)b * T1 * 256;
  for (int idx = threadIdx.x; idx < C1_ROWS * nch; idx += C1_THREADS) {
    const int r = idx / nch, ch = idx - r * nch, t = t0 - 1 + r;
    float v[VEC];
    if (t >= 0 && t < T1) {
      load16(src + (long)t * 256 + ch * VEC, v);
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j) v[j] = 0.f;
    }
    float* row = c1_lds + r * pitch + ch * VEC;
    const int rot = ch / (32 / VEC);
#pragma unroll
    for (int j = 0; j < VEC; ++j) row[(j + rot) & (VEC - 1)] = v[j];
  }
  __syncthreads();
  constexpr int QUADS = C1_TILE / 4;
  for (int item = threadIdx.x; item < nm * QUADS; item += C1_THREADS) {
    const int c = item / QUADS, q = item - c * QUADS;
    float acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      // output frame t0 + 4q + j; tap k reads window row t + 1 - k = LDS row 4q + j + 2 - k
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 3; ++k) s += c1_lds[(4 * q + j + 2 - k) * pitch + c1_slot<VEC>(k * nm + c)];
      acc[j] = s;
    }
    const int t = t0 + 4 * q;
    float* dst = dmel + ((long)b * nm + c) * T1 + t;
    if ((T1 & 3) == 0 && t + 3 < T1) {
      f32x4_t o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = acc[j];
      *(f32x4_t*)dst = o;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (t + j < T1) dst[j] = acc[j];
    }
  }
}

template <typename T>
int launch_c1(const T* dcol, float* dmel, int B, int T1, int nm, hipStream_t s) {
  constexpr int VEC = 16 / sizeof(T);
  // (3 * n_mels columns in whole 16-byte chunks, inside the 256 of the packed kernel; grid.y = clips)
  OASR_REQUIRE(dcol && dmel && B > 0 && B <= 65535 && T1 > 0 && nm > 0 && (3 * nm) % 8 == 0 && 3 * nm <= 256,
               "conv1_col2im_mel: bad args (B=%d T1=%d n_mels=%d)", B, T1, nm);
  int pitch = 3 * nm;
  while ((pitch & 7) != 1) ++pitch;
  const size_t lds = (size_t)C1_ROWS * pitch * sizeof(float);
  hipLaunchKernelGGL(conv1_col2im_mel_kernel<T>, dim3(cdiv(T1, C1_TILE), B), dim3(C1_THREADS), lds, s, dcol, dmel, T1, nm, pitch);
  OASR_LAUNCH_CHECK();
  (void)VEC;
  return OASR_OK;
}

}  // namespace

int launch_conv1_col2im_mel(const bf16_t* dcol, float* dmel, int B, int T1, int nm, hipStream_t s) { return launch_c1(dcol, dmel, B, T1, nm, s); }
int launch_conv1_col2im_mel(const float* dcol, float* dmel, int B, int T1, int nm, hipStream_t s) { return launch_c1(dcol, dmel, B, T1, nm, s); }
