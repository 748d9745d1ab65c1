// SpecAugment on the finalized log-mel tensor (include/oasr.h at oasr_spec_augment): seeded frequency / time masks, in place, one launch.
//
// One 256-thread workgroup per (clip, mel bin) row of mel f32 [B, n_mels, T].  Its first freq_masks + time_masks threads each derive one
// interval of the clip by the rule of specaug_core.h from the clip's draw stream, draw_core.h (64-bit integer VALU math; the two 64-bit
// remainders per interval are the only expensive instructions and run once per workgroup, not per element) and leave it in LDS.  A row
// whose bin lies in a frequency mask is
// filled as a whole; any other row gets only its time intervals.  The kernel never loads from mel and stores to masked cells only, so every
// other cell keeps its bits.  There is no mask tensor and nothing comes from the host but the policy, the seed and the first stream id.
#include "common.h"
#include "kernels.h"
#include "../../include/oasr.h"
#include "specaug_core.h"

static_assert(OASR_SPECAUG_MAX_MASKS == SPECAUG_MAX_MASKS, "include/oasr.h and specaug_core.h disagree");

#define SPECAUG_THREADS 256

// p[0, n) = fill by the whole workgroup: scalar stores up to the first 16-byte boundary, 16-byte stores between, scalar stores for the rest
__device__ __forceinline__ void specaug_fill(float* p, int n, float fill, int tid) {
  const int to_boundary = (int)(((0 - (uintptr_t)p) & 15) >> 2);  // p is 4-byte aligned (launcher)
  const int head = to_boundary < n ? to_boundary : n;
  if (tid < head) p[tid] = fill;
  const int nq = (n - head) >> 2;
  f32x4_t* q = (f32x4_t*)(p + head);
  const f32x4_t v = {fill, fill, fill, fill};
  for (int i = tid; i < nq; i += SPECAUG_THREADS) q[i] = v;
  const int done = head + 4 * nq;  // n - done in [0, 3]
  if (tid < n - done) p[done + tid] = fill;
}

__global__ __launch_bounds__(SPECAUG_THREADS) void spec_augment_kernel(float* __restrict__ mel, int n_mels, int T, oasr_specaug pol, uint64_t seed,
                                                                       uint64_t first_clip) {
  __shared__ int s_start[2 * SPECAUG_MAX_MASKS], s_width[2 * SPECAUG_MAX_MASKS];  // frequency masks first, then time masks
  const int tid = threadIdx.x;
  const int b = blockIdx.x / n_mels, bin = blockIdx.x - b * n_mels;
  const int nf = pol.freq_masks, nt = pol.time_masks;
  if (tid < nf + nt) {
    const uint64_t h = draw_clip_hash(seed, first_clip + (uint64_t)b);
    int start, width;
    if (tid < nf)
      specaug_interval(h, DRAW_FREQ_MASK, tid, pol.freq_width, n_mels, &start, &width);
    else
      specaug_interval(h, DRAW_TIME_MASK, tid - nf, pol.time_width, T, &start, &width);
    s_start[tid] = start, s_width[tid] = width;
  }
  __syncthreads();
  float* row = mel + (size_t)blockIdx.x * (size_t)T;
  bool whole = false;
  for (int i = 0; i < nf; ++i) whole |= bin >= s_start[i] && bin < s_start[i] + s_width[i];
  if (whole) {  // (uniform: every thread read the same LDS words)
    specaug_fill(row, T, pol.fill, tid);
    return;
  }
  for (int i = nf; i < nf + nt; ++i) specaug_fill(row + s_start[i], s_width[i], pol.fill, tid);  // start + width <= T (specaug_interval)
}

int launch_spec_augment(float* mel, int B, int n_mels, int T, const oasr_specaug* p, uint64_t seed, uint64_t first_clip, hipStream_t st) {
  OASR_REQUIRE(mel && p, "oasr_spec_augment: null mel or policy");
  OASR_REQUIRE(((uintptr_t)mel & 3) == 0, "oasr_spec_augment: mel is not 4-byte aligned");
  OASR_REQUIRE(B >= 1 && n_mels >= 1 && T >= 1, "oasr_spec_augment: B = %d, n_mels = %d, T = %d must all be >= 1", B, n_mels, T);
  OASR_REQUIRE((long)B * n_mels <= 0x7fffffffL, "oasr_spec_augment: B * n_mels = %ld rows exceed one grid", (long)B * n_mels);
  const char* why = specaug_policy_error(p->freq_masks, p->freq_width, p->time_masks, p->time_width);
  OASR_REQUIRE(!why, "oasr_spec_augment: %s (freq %d x <= %d, time %d x <= %d)", why, p->freq_masks, p->freq_width, p->time_masks, p->time_width);
  if (p->freq_masks + p->time_masks == 0) return OASR_OK;  // a policy without masks writes nothing
  hipLaunchKernelGGL(spec_augment_kernel, dim3(B * n_mels), dim3(SPECAUG_THREADS), 0, st, mel, n_mels, T, *p, seed, first_clip);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}
