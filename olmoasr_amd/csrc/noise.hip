// Noise mixing of int16 PCM (include/oasr.h at oasr_noise_mix; the rule: noise_core.h): a bank row added at a drawn offset and SNR, in two
// launches -- exact energies, then gain and mix -- with no host round trip, no memset and no atomics.
//
// A tile is NOISE_TILE = 2048 consecutive samples of one clip on the 16-byte grid of the output row (pcm_tile.h), thread t of 256 holding
// samples 8 t .. 8 t + 7 of it.  The bank row sits at an offset from that grid that depends on the drawn offset o, so its eight samples come
// like the clip's, by one 16-byte load that is only 2-byte aligned; samples go one by one only at a row's ends and where the bank row wraps.
// Every workgroup evaluates the clip's plan itself from (seed, clip) -- four hashes of scalar work (draw_core.h) -- so nothing comes back to
// the host.
//   energy   one workgroup per tile that holds samples below n_valid of a drawn clip: the exact sums of x^2 and v^2 over its samples go to
//            workspace[clip][tile] as two u64.  Other workgroups return at once and write nothing.
//   mix      one workgroup per NOISE_MIX_TILES = 4 tiles.  It sums the clip's partials (only the tiles the energy launch wrote), computes the
//            gain -- one 64-bit division and a 32-step integer square root, some 500 instructions per wave, which is why a workgroup takes
//            four tiles and not one -- and writes its tiles: mixed below n_valid, copied above; a clip that is not mixed is copied, or left
//            alone in place.  The first workgroup of a clip writes the reports.
// Integer sums are associative: the result does not depend on the tiling, hence not on where a row starts.
#include "common.h"
#include "kernels.h"
#include "../../include/oasr.h"
#include "noise_core.h"
#include "pcm_tile.h"

static_assert(OASR_NOISE_NONE == NOISE_NONE, "include/oasr.h and noise_core.h disagree");

#define NOISE_THREADS 256
#define NOISE_PER_THREAD 8
#define NOISE_TILE (NOISE_THREADS * NOISE_PER_THREAD)
#define NOISE_MIX_TILES 4
#define NOISE_WAVES (NOISE_THREADS / 64)

static inline long noise_tiles(int N) { return ((long)N + 7 + NOISE_TILE - 1) / NOISE_TILE; }  // a row's tiles, whatever its address
size_t noise_workspace_bytes(int B, int N) { return (size_t)B * (size_t)noise_tiles(N) * 2 * sizeof(uint64_t); }

// the noise under samples [n0, n0 + 8) of a clip: brow[(o + n) % L] where 0 <= n < hi, zero elsewhere; n0 >= -7, o < L
__device__ __forceinline__ s16x8_t noise_bank8(const int16_t* __restrict__ brow, int o, int L, int n0, int hi) {
  s16x8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
  const int first = n0 > 0 ? n0 : 0;
  if (first >= hi) return v;
  int p = (int)((unsigned)(o + first) % (unsigned)L);  // (o + first < 2^27)
  if (n0 >= 0 && n0 + 8 <= hi && p + 8 <= L) {
    __builtin_memcpy(&v, brow + p, sizeof(v));
    return v;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (n0 + e >= first && n0 + e < hi) {
      v[e] = brow[p];
      if (++p == L) p = 0;
    }
  return v;
}

// the workgroup's sums of (ex, ev), in every thread; s_part: NOISE_WAVES x 2 words of LDS (all threads of the workgroup call this)
__device__ __forceinline__ void noise_block_sum(uint64_t& ex, uint64_t& ev, uint64_t (*s_part)[2]) {
  for (int o = 32; o > 0; o >>= 1) {
    ex += __shfl_xor((unsigned long long)ex, o, 64);
    ev += __shfl_xor((unsigned long long)ev, o, 64);
  }
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6][0] = ex, s_part[threadIdx.x >> 6][1] = ev;
  __syncthreads();
  ex = ev = 0;
#pragma unroll
  for (int w = 0; w < NOISE_WAVES; ++w) ex += s_part[w][0], ev += s_part[w][1];
}

__global__ __launch_bounds__(NOISE_THREADS) void noise_energy_kernel(oasr_noise_args a, long tiles) {
  __shared__ uint64_t s_part[NOISE_WAVES][2];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int nv = a.n_valid[b];
  if (nv < 1 || nv > a.N) return;
  const NoisePlan pl = noise_plan(a.seed, a.first_clip + (uint64_t)b, a.policy.prob_q16, a.policy.snr_lo_db, a.policy.snr_hi_db, a.M, a.L);
  if (!pl.drawn) return;
  const int16_t* x = a.pcm_in + (size_t)b * (size_t)a.ld_in;
  const int16_t* y = a.pcm_out + (size_t)b * (size_t)a.ld_out;
  const int16_t* brow = a.bank + (size_t)pl.m * (size_t)a.ld_bank;
  const int lead = pcm_lead(y);
  const long n_lo = (long)blockIdx.x * NOISE_TILE - lead;  // the tile covers [n_lo, n_lo + TILE) of the row
  if (n_lo >= nv) return;
  const int n0 = (int)n_lo + NOISE_PER_THREAD * tid;
  const s16x8_t x8 = pcm_load8(x, n0, nv), v8 = noise_bank8(brow, pl.o, a.L, n0, nv);
  uint64_t ex = 0, ev = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    ex += (uint32_t)((int)x8[e] * (int)x8[e]);  // (a square is at most 2^30)
    ev += (uint32_t)((int)v8[e] * (int)v8[e]);
  }
  noise_block_sum(ex, ev, s_part);
  if (tid == 0) {
    uint64_t* part = (uint64_t*)a.workspace + ((size_t)b * (size_t)tiles + blockIdx.x) * 2;
    part[0] = ex, part[1] = ev;
  }
}

__global__ __launch_bounds__(NOISE_THREADS) void noise_mix_kernel(oasr_noise_args a, long tiles) {
  __shared__ uint64_t s_part[NOISE_WAVES][2];
  const int tid = threadIdx.x, b = blockIdx.y, N = a.N;
  const int nv = a.n_valid[b];
  const NoisePlan pl = noise_plan(a.seed, a.first_clip + (uint64_t)b, a.policy.prob_q16, a.policy.snr_lo_db, a.policy.snr_hi_db, a.M, a.L);
  const int16_t* x = a.pcm_in + (size_t)b * (size_t)a.ld_in;  // (x may be y: no __restrict__)
  int16_t* y = a.pcm_out + (size_t)b * (size_t)a.ld_out;
  const int lead = pcm_lead(y);
  int64_t g = 0;
  bool mixed = false;
  if (pl.drawn && nv >= 1 && nv <= N) {  // (the same for every thread of the workgroup)
    const int n_live = (nv + lead + NOISE_TILE - 1) / NOISE_TILE;  // the tiles the energy launch wrote: those with n_lo < n_valid
    const uint64_t* part = (const uint64_t*)a.workspace + (size_t)b * (size_t)tiles * 2;
    uint64_t ex = 0, ev = 0;
    for (int t = tid; t < n_live; t += NOISE_THREADS) ex += part[2 * t], ev += part[2 * t + 1];
    noise_block_sum(ex, ev, s_part);
    mixed = noise_gain(ex, ev, pl.s, &g);
  }
  if (blockIdx.x == 0 && tid == 0) {
    if (a.row_out) a.row_out[b] = mixed ? pl.m : -1;
    if (a.snr_out) a.snr_out[b] = mixed ? pl.s : NOISE_NONE;
    if (a.gain_out) a.gain_out[b] = g;
  }
  if (!mixed && x == y) return;  // in place, the row stays as it is
  const int hi_v = mixed ? nv : 0;
  const int16_t* brow = a.bank + (size_t)pl.m * (size_t)a.ld_bank;
#pragma unroll 1
  for (int k = 0; k < NOISE_MIX_TILES; ++k) {
    const long n_lo = ((long)blockIdx.x * NOISE_MIX_TILES + k) * NOISE_TILE - lead;
    if (n_lo >= N) return;
    const int n0 = (int)n_lo + NOISE_PER_THREAD * tid;
    s16x8_t y8 = pcm_load8(x, n0, N);
    if (n0 < hi_v) {
      const s16x8_t v8 = noise_bank8(brow, pl.o, a.L, n0, hi_v);
#pragma unroll
      for (int e = 0; e < 8; ++e) y8[e] = noise_sample(y8[e], v8[e], g);
    }
    pcm_store8(y, n0, N, y8);
  }
}

int launch_noise_mix(const oasr_noise_args* a, hipStream_t st) {
  const char* why = noise_args_error(a);
  OASR_REQUIRE(!why, "oasr_noise_mix: %s", why);
  OASR_REQUIRE_WORKSPACE(a, 8, noise_workspace_bytes(a->B, a->N), "oasr_noise_mix", "oasr_noise_workspace_bytes");
  const long tiles = noise_tiles(a->N);
  hipLaunchKernelGGL(noise_energy_kernel, dim3((unsigned)tiles, (unsigned)a->B), dim3(NOISE_THREADS), 0, st, *a, tiles);
  OASR_LAUNCH_CHECK();
  hipLaunchKernelGGL(noise_mix_kernel, dim3((unsigned)cdiv(tiles, NOISE_MIX_TILES), (unsigned)a->B), dim3(NOISE_THREADS), 0, st, *a, tiles);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}
