// logmel_main: the round-1/2 log-mel kernel, a dense folded DFT on the fp32 matrix pipe.  NOT the default (logmel.hip: the quad-lane kernel is);
// kept selectable (OASR_LOGMEL=mfma) as an A/B partner and as a cross-check that shares no transform code with the FFT kernels.
//
// Design: one workgroup = 64 frames of one clip.  The windowed DFT runs on the exact-f32 matrix pipe
// (v_mfma_f32_16x16x4_f32, k-ordered fmaf chain == f32 accuracy; bf16 MFMA cannot hold the 80 dB dynamic range the
// -8 floor needs) with the frame FOLDED about its centre first: the periodic hann window and cos are even, sin is odd
// under n -> 400 - n, so   Re X[k] = sum_{n=0..200} w[n] c[k][n] (x[n] + x[400-n])   (n = 0 and 200 counted once),
//                          Im X[k] = sum_{n=1..199} w[n] s[k][n] (x[n] - x[400-n]),
// i.e. two [64 x 208] x [208 x 208] products instead of one [64 x 400] x [400 x 416]: half the MFMA work of the
// dense DFT, same arithmetic.  The hann window is folded into the basis.  Power and the mel projection stay on chip (LDS), only
// PCM is read and log-mel written: algorithmic HBM bytes = 2*n (i16) + 4*80*n/160 per clip.
// The per-clip max (for the -8 floor) is an ordered-uint atomicMax; a second tiny pass applies it.
#include "logmel_common.h"

namespace {

constexpr int NBH = 208;           // bins padded to 13 tiles of 16
constexpr int NB = 2 * NBH;        // cos | sin columns
constexpr int FT = 64;             // frames per workgroup
constexpr int NS = FT * HOP + (NFFT - HOP);  // 10480 samples per workgroup
constexpr int SLAB_LD = 432;       // basis slab row stride (floats): 432 % 32 == 16 -> conflict-free b32 reads
constexpr int P_LD = 212;          // power row stride (floats): 53 16-B slots -> conflict-free b128 reads
constexpr int KS = 16;             // DFT k per slab
constexpr int NK = 208;            // folded sample index n = 0..200, padded to 13 slabs (rows > 200 of the basis are zero)

__device__ __forceinline__ int lds_sample_addr(int s) { return s + 4 * (s / HOP); }

template <typename PCM>
__global__ __launch_bounds__(256) void logmel_main(const PCM* __restrict__ pcm, int n_samples, int n_frames,
                                                   const float* __restrict__ basis,    // [208][416] folded basis: w[n] cos | w[n] sin
                                                   const float* __restrict__ melfilt,  // [208][80]
                                                   float* __restrict__ out,            // [B][80][n_frames] log10 values
                                                   unsigned* __restrict__ clipmax) {   // [B] ordered-uint max
  extern __shared__ __attribute__((aligned(16))) float smem[];
  // region 0: samples (10480 + 4*66 floats) -- later aliased by the per-wave power tiles
  // region 1: basis slab [16][432]
  constexpr int SAMP_FLOATS = NS + 4 * (NS / HOP + 1);
  constexpr int REG0 = (SAMP_FLOATS > 4 * 16 * P_LD ? SAMP_FLOATS : 4 * 16 * P_LD);
  float* samp = smem;
  float* slab = smem + ((REG0 + 3) & ~3);

  const int b = blockIdx.y;
  const int f0 = blockIdx.x * FT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const PCM* clip = pcm + (long)b * n_samples;

  // ---- stage the samples this frame block touches (reflect padding of torch.stft(center=True)) ----
  const long s_begin = (long)f0 * HOP - NFFT / 2;
  for (int s = tid; s < NS; s += 256) {
    samp[lds_sample_addr(s)] = load_pcm<PCM>(clip, reflect_index(s_begin + s, n_samples));
  }

  f32x4_t acc[26];
#pragma unroll
  for (int i = 0; i < 26; ++i) acc[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  const int frame_l = wave * 16 + c;  // A-operand row of this lane
  // basis slabs go L2 -> registers -> LDS one slab ahead: the loads of slab kb+1 are in flight under slab kb's MFMAs
  constexpr int SLAB_V4 = KS * (NB / 4), PER_T = (SLAB_V4 + 255) / 256;  // 1664 16-byte pieces, 7 per thread
  f32x4_t pre[PER_T];
  auto slab_fetch = [&](int kb) {
#pragma unroll
    for (int j = 0; j < PER_T; ++j) {
      const int i = tid + j * 256;
      if (i < SLAB_V4) pre[j] = *(const f32x4_t*)(basis + (long)(kb * KS + i / (NB / 4)) * NB + (i % (NB / 4)) * 4);
    }
  };
  slab_fetch(0);
  for (int kb = 0; kb < NK / KS; ++kb) {
    __syncthreads();  // previous slab fully consumed (and, first time, samples staged)
#pragma unroll
    for (int j = 0; j < PER_T; ++j) {
      const int i = tid + j * 256;
      if (i < SLAB_V4) *(f32x4_t*)(slab + (i / (NB / 4)) * SLAB_LD + (i % (NB / 4)) * 4) = pre[j];
    }
    __syncthreads();
    if (kb + 1 < NK / KS) slab_fetch(kb + 1);
    // this lane's 4 folded samples n0..n0+3: x[n] and its mirror x[400-n] (two aligned 16-byte reads around 400-n0)
    const int n0 = kb * KS + 4 * g;
    const f32x4_t xa = *(const f32x4_t*)(samp + lds_sample_addr(frame_l * HOP + n0));
    const f32x4_t g1 = *(const f32x4_t*)(samp + lds_sample_addr(frame_l * HOP + NFFT - n0 - 4));
    const float x_m = samp[lds_sample_addr(frame_l * HOP + NFFT - n0)];  // x[400 - n0]: outside the frame when n0 == 0
    const bool once = n0 == 0 || n0 == NFFT / 2;                           // n = 0 and n = 200 are their own mirror
    const float xr[4] = {once ? 0.f : x_m, g1[3], g1[2], g1[1]};
    float ev[4], od[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ev[i] = xa[i] + xr[i];
      od[i] = xa[i] - xr[i];
    }
#pragma unroll
    for (int nt = 0; nt < 13; ++nt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float bc = slab[(4 * g + i) * SLAB_LD + nt * 16 + c];
        const float bs = slab[(4 * g + i) * SLAB_LD + NBH + nt * 16 + c];
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ev[i], bc, acc[nt], 0, 0, 0);
        acc[13 + nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(od[i], bs, acc[13 + nt], 0, 0, 0);
      }
    }
  }
  __syncthreads();  // all waves done reading samples: region 0 becomes the power tiles

  // ---- power spectrum -> LDS [wave][16 frames][212] ------------------------------------------------
  float* pw = smem + wave * 16 * P_LD;
#pragma unroll
  for (int nt = 0; nt < 13; ++nt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float re = acc[nt][r], im = acc[13 + nt][r];
      pw[(g * 4 + r) * P_LD + nt * 16 + c] = re * re + im * im;
    }
  }
  __syncthreads();

  // ---- mel projection: [16 frames x 208] x [208 x 80] ---------------------------------------------
  f32x4_t macc[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) macc[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < NBH; k0 += 16) {
    const f32x4_t a4 = *(const f32x4_t*)(pw + c * P_LD + k0 + 4 * g);
#pragma unroll
    for (int nt = 0; nt < 5; ++nt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float bv = melfilt[(k0 + 4 * g + i) * NMEL + nt * 16 + c];
        macc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[i], bv, macc[nt], 0, 0, 0);
      }
    }
  }

  // ---- log10, per-clip max, store ------------------------------------------------------------------
  float vmax = -1e30f;
  const int t0 = f0 + wave * 16 + g * 4;
#pragma unroll
  for (int nt = 0; nt < 5; ++nt) {
    const int m = nt * 16 + c;
    float* dst = out + ((long)b * NMEL + m) * n_frames + t0;
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      v[r] = log10f(fmaxf(macc[nt][r], 1e-10f));
      if (t0 + r < n_frames) vmax = fmaxf(vmax, v[r]);
    }
    if (t0 + 3 < n_frames && ((n_frames & 3) == 0)) {
      *(f32x4_t*)dst = (f32x4_t){v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (t0 + r < n_frames) dst[r] = v[r];
    }
  }
  vmax = wave_max(vmax);
  if (lane == 0 && vmax > -1e29f) atomicMax(clipmax + b, f2ord(vmax));
}

static_assert(NK == BASIS_ROWS && NB == BASIS_COLS && NBH == MELFILT_ROWS, "logmel_tables.h builds the tables this kernel reads");

template <typename PCM>
int launch_main(const LogmelArgs& a) {
  constexpr int SAMP_FLOATS = NS + 4 * (NS / HOP + 1);
  constexpr int REG0 = (SAMP_FLOATS > 4 * 16 * P_LD ? SAMP_FLOATS : 4 * 16 * P_LD);
  const size_t lds = sizeof(float) * (((REG0 + 3) & ~3) + KS * SLAB_LD);
  const dim3 grid(cdiv(a.n_frames, FT), a.B);
  static LdsAttrOnce attr;
  const int rc = ensure_dynamic_lds(attr, (const void*)logmel_main<PCM>, (int)lds);
  if (rc) return rc;
  hipLaunchKernelGGL(logmel_main<PCM>, grid, dim3(256), lds, a.stream, (const PCM*)a.pcm, a.n_samples, a.n_frames, a.tab->basis,
                     a.tab->melfilt, a.out, a.clipmax);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}

}  // namespace

int launch_logmel_dft(const LogmelArgs& a) { return a.pcm_dtype == 1 ? launch_main<int16_t>(a) : launch_main<float>(a); }
