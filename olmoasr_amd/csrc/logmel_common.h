// What more than one of the log-mel kernel files shares (logmel.hip describes the kernels): the ordered-uint encoding of the per-clip
// maximum, the PCM load, the reflect-padding index, the complex helpers and the 5-point DFT, and the interface between logmel.hip -- which
// checks the arguments, owns the device tables and chooses the kernel -- and logmel_dft.hip, logmel_fft.hip, logmel_quad.hip, which own the
// kernels and their launch geometry.  The dimensions NFFT, HOP, NFREQ, NMEL come with logmel_tables.h: the host table builder needs them too.
// As in attention_common.h, a shared piece is one whose extraction left every kernel's instruction stream as it was
// (scripts/isa_compare.py, profiles/logmel_split_isa.txt).
#pragma once
#include "common.h"
#include "logmel_tables.h"

namespace {

__device__ __forceinline__ unsigned f2ord(float f) {
  unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

template <typename PCM>
__device__ __forceinline__ float load_pcm(const PCM* p, long i);
template <>
__device__ __forceinline__ float load_pcm<int16_t>(const int16_t* p, long i) { return (float)p[i] * (1.0f / 32768.0f); }
template <>
__device__ __forceinline__ float load_pcm<float>(const float* p, long i) { return p[i]; }

// sample idx of a clip under the reflect padding of torch.stft(center=True); clamped where one reflection does not reach
__device__ __forceinline__ long reflect_index(long idx, int n_samples) {
  if (idx < 0) idx = -idx;
  if (idx >= n_samples) idx = 2L * (n_samples - 1) - idx;
  return idx < 0 ? 0 : (idx >= n_samples ? n_samples - 1 : idx);
}

struct cf {
  float x, y;
};
__device__ __forceinline__ cf cadd(cf a, cf b) { return cf{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ cf csub(cf a, cf b) { return cf{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ cf cmul(cf a, cf b) { return cf{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ cf mni(cf a) { return cf{a.y, -a.x}; }  // -i a
__device__ __forceinline__ cf pli(cf a) { return cf{-a.y, a.x}; }  // +i a
__device__ __forceinline__ cf cscale(cf a, float s) { return cf{a.x * s, a.y * s}; }

__device__ __forceinline__ void dft5(cf x0, cf x1, cf x2, cf x3, cf x4, cf (&y)[5]) {  // forward
  constexpr float C1 = 0.30901699437494742f, C2 = -0.80901699437494742f, S1 = 0.95105651629515357f, S2 = 0.58778525229247313f;
  const cf t1 = cadd(x1, x4), t2 = cadd(x2, x3), t3 = csub(x1, x4), t4 = csub(x2, x3);
  y[0] = cadd(x0, cadd(t1, t2));
  const cf m1 = cf{x0.x + C1 * t1.x + C2 * t2.x, x0.y + C1 * t1.y + C2 * t2.y};
  const cf m2 = cf{x0.x + C2 * t1.x + C1 * t2.x, x0.y + C2 * t1.y + C1 * t2.y};
  const cf s1 = cf{S1 * t3.x + S2 * t4.x, S1 * t3.y + S2 * t4.y};
  const cf s2 = cf{S2 * t3.x - S1 * t4.x, S2 * t3.y - S1 * t4.y};
  y[1] = cadd(m1, mni(s1));
  y[2] = cadd(m2, mni(s2));
  y[3] = cadd(m2, pli(s2));
  y[4] = cadd(m1, pli(s1));
}

}  // namespace

// ---- logmel.hip -> the kernel files ------------------------------------------------------------------------------------------------
struct MelTables {  // one device's constant tables (logmel_tables.h gives their layout)
  float* basis = nullptr;     // [208][416] (folded)
  float* melfilt = nullptr;   // [208][80]
  float* fft_tab = nullptr;   // [XTAB] stage tables of the LDS FFT kernel (twiddles, window, sparse mel filters)
  float* quad_tab = nullptr;  // [QTAB] per-lane tables of the quad-lane kernel
  int mel_words = 0;          // used words of fft_tab's mel part
  int mel_span = 0;           // taps of the widest filter
};
struct LogmelArgs {
  const void* pcm;  // [B][n_samples], int16 (pcm_dtype 1) or f32 (0)
  int pcm_dtype, B, n_samples, n_frames;
  const MelTables* tab;
  float* out;         // [B][80][n_frames] log10 values
  unsigned* clipmax;  // [B] ordered-uint maxima, zeroed
  hipStream_t stream;
};
// each enqueues its kernel (grid and LDS size are the kernel file's business) and returns OASR_OK or the launch's error
int launch_logmel_quad(const LogmelArgs& a);
int launch_logmel_fft(const LogmelArgs& a, int frames_per_wg);  // 16 or 32
int launch_logmel_dft(const LogmelArgs& a);
