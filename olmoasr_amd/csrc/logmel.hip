// Log-mel front end on gfx950: PCM (int16 or f32) -> log-mel [B, 80, n_frames] f32.
//
// Replaces whisper.audio.log_mel_spectrogram as called by the reference at
// scripts/training/train_timestamps.py:196,214 and olmoasr/transcribe.py:148.
//   hann(400) STFT, hop 160, center/reflect pad, drop last frame -> |X|^2 [201, n/160]
//   -> 80x201 slaney mel filterbank -> log10(clamp 1e-10) -> max(x, clipmax-8) -> (x+4)/4
//
// What runs is logmel_quad (logmel_quad.hip): a frame's 400-point real FFT in the registers of four adjacent lanes, 64 frames per workgroup,
// only PCM read and log-mel written (algorithmic HBM bytes = 2*n (i16) + 4*80*n/160 per clip).  Every kernel leaves log10 of the mel power
// and the per-clip maximum (an ordered-uint atomicMax, for the -8 floor); a second tiny pass here applies the floor and the scale
// (logmel_finalize), or hands the maxima out for a consumer that applies them on the fly (logmel_clipmax_kernel).
// Two older kernels stay selectable through OASR_LOGMEL (read once per process, inert without OASR_TESTING_HOOKS=1): "fft" / "fft32", the
// round-3/5 LDS FFT (logmel_fft.hip) with 16 / 32 frames per workgroup, and "mfma", the round-1/2 dense folded DFT on the fp32 matrix pipe
// (logmel_dft.hip).  They stay because they are what the quad kernel is measured against and because three transforms that share no
// summation order cross-check each other (tests/test_gpu_logmel.py runs each).  This file checks the arguments, owns the per-device
// constant tables (built by logmel_host.cpp) and chooses the kernel; logmel_common.h is what the four files share.
#include "kernels.h"
#include "logmel_common.h"

namespace {

__global__ __launch_bounds__(256) void logmel_finalize(float* __restrict__ mel, const unsigned* __restrict__ clipmax,
                                                       long per_clip) {
  const int b = blockIdx.y;
  const float floor_v = ord2f(clipmax[b]) - 8.0f;
  float* p = mel + (long)b * per_clip;
  const long n4 = per_clip >> 2;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    f32x4_t v = ((f32x4_t*)p)[i];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = (fmaxf(v[r], floor_v) + 4.0f) * 0.25f;
    ((f32x4_t*)p)[i] = v;
  }
  if (blockIdx.x == 0)
    for (long i = (n4 << 2) + threadIdx.x; i < per_clip; i += 256) p[i] = (fmaxf(p[i], floor_v) + 4.0f) * 0.25f;
}

MelTables g_tables[16];  // per device; an entry is published whole or not at all

}  // namespace

static int upload(const std::vector<float>& h, float** d) {
  OASR_CHECK_HIP(hipMalloc((void**)d, sizeof(float) * h.size()));
  OASR_CHECK_HIP(hipMemcpy(*d, h.data(), sizeof(float) * h.size(), hipMemcpyHostToDevice));
  return OASR_OK;
}

static int ensure_tables(int device, const MelTables** t_out) {
  OASR_REQUIRE(device >= 0 && device < 16, "device index %d out of range", device);
  if (g_tables[device].basis == nullptr) {
    LogmelHostTables h;
    int rc = logmel_build_tables(h);
    if (rc) return rc;
    MelTables t;
    t.mel_words = h.mel_words;
    t.mel_span = h.mel_span;
    if ((rc = upload(h.basis, &t.basis)) || (rc = upload(h.melfilt, &t.melfilt)) || (rc = upload(h.fft_tab, &t.fft_tab)) ||
        (rc = upload(h.quad_tab, &t.quad_tab))) {
      for (float* p : {t.basis, t.melfilt, t.fft_tab, t.quad_tab}) (void)hipFree(p);  // (null: nothing to free)
      return rc;
    }
    g_tables[device] = t;
  }
  *t_out = &g_tables[device];
  return OASR_OK;
}

extern "C" size_t oasr_log_mel_workspace_bytes(int B) { return (size_t)((B * 4 + 255) / 256) * 256; }

__global__ __launch_bounds__(256) void logmel_clipmax_kernel(const unsigned* __restrict__ clipmax, float* __restrict__ out, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < B) out[b] = ord2f(clipmax[b]);
}

enum class MelKernel { quad, fft16, fft32, dft };

static int log_mel_impl(const void* pcm, int pcm_dtype, int B, int n_samples, float* mel, void* workspace, hipStream_t stream,
                        float* clip_max_out) {
  OASR_REQUIRE(pcm && mel && workspace, "null pointer");
  OASR_REQUIRE(pcm_dtype == 0 || pcm_dtype == 1, "pcm_dtype must be 0 (f32) or 1 (i16)");
  OASR_REQUIRE(B > 0 && n_samples > NFFT / 2, "need B > 0 and n_samples > 200 (reflect padding), got %d, %d", B, n_samples);
  const int n_frames = n_samples / HOP;
  OASR_REQUIRE(n_frames > 0, "n_samples %d shorter than one hop", n_samples);
  int device = 0;
  OASR_CHECK_HIP(hipGetDevice(&device));
  const MelTables* t = nullptr;
  int rc = ensure_tables(device, &t);
  if (rc) return rc;
  unsigned* clipmax = (unsigned*)workspace;
  OASR_CHECK_HIP(hipMemsetAsync(clipmax, 0, sizeof(unsigned) * B, stream));
  static const MelKernel which = [] {  // A/B and cross-check: the header of this file
    const char* e = oasr_experiment_env("OASR_LOGMEL");
    if (e && strcmp(e, "mfma") == 0) return MelKernel::dft;
    if (e && strcmp(e, "fft") == 0) return MelKernel::fft16;
    if (e && strcmp(e, "fft32") == 0) return MelKernel::fft32;
    return MelKernel::quad;
  }();
  const LogmelArgs a = {pcm, pcm_dtype, B, n_samples, n_frames, t, mel, clipmax, stream};
  switch (which) {
    case MelKernel::quad: rc = launch_logmel_quad(a); break;
    case MelKernel::fft16: rc = launch_logmel_fft(a, 16); break;
    case MelKernel::fft32: rc = launch_logmel_fft(a, 32); break;
    case MelKernel::dft: rc = launch_logmel_dft(a); break;
  }
  if (rc) return rc;
  const long per_clip = (long)NMEL * n_frames;
  const dim3 g2((unsigned)((per_clip / 4 + 255) / 256 > 64 ? 64 : (per_clip / 4 + 255) / 256 + 1), B);
  if (clip_max_out) hipLaunchKernelGGL(logmel_clipmax_kernel, dim3(cdiv(B, 256)), dim3(256), 0, stream, clipmax, clip_max_out, B);
  else hipLaunchKernelGGL(logmel_finalize, g2, dim3(256), 0, stream, mel, clipmax, per_clip);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}

extern "C" int oasr_log_mel(const void* pcm, int pcm_dtype, int B, int n_samples, float* mel, void* workspace,
                            hipStream_t stream) {
  return log_mel_impl(pcm, pcm_dtype, B, n_samples, mel, workspace, stream, nullptr);
}
// The same front end WITHOUT its last pass: mel_raw = log10(max(mel power, 1e-10)) and clip_max[b] = the clip's maximum of it (device
// f32 [B]).  whisper's last two lines -- log_spec = max(log_spec, log_spec.max() - 8); (log_spec + 4) / 4 -- need the clip maximum, i.e.
// a second pass over the tensor; a consumer that reads the tensor anyway applies them on the fly instead
// (oasr_train_step's mel_clip_max: the encoder's time-major transpose), which halves this front end's HBM traffic.
extern "C" int oasr_log_mel_raw(const void* pcm, int pcm_dtype, int B, int n_samples, float* mel_raw, float* clip_max, void* workspace,
                                hipStream_t stream) {
  OASR_REQUIRE(clip_max, "oasr_log_mel_raw: null clip_max");
  return log_mel_impl(pcm, pcm_dtype, B, n_samples, mel_raw, workspace, stream, clip_max);
}
