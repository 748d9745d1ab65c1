// The telephone channel on int16 PCM (include/oasr.h at oasr_telephone; the rule: telephone_core.h): band-pass and decimation to 8 kHz, a
// drawn G.711 codec, interpolation back to 16 kHz -- out of place, one launch.
//
// One 256-thread workgroup owns TEL_TILE = 2048 consecutive output samples of one clip, laid on the 16-byte grid of the output row
// (pcm_tile.h), so each thread's 8 samples leave as one aligned 16-byte store.  Every workgroup evaluates the clip's plan itself from
// (seed, clip, n_valid) -- three hashes of scalar work (draw_core.h) -- so nothing comes back to the host.
//   copied row, tile at or past n_valid    a vector copy, nothing is staged
//   otherwise   with m_lo = floor(n_lo / 2): the tile's outputs read the 8 kHz samples c[m_lo - 15 .. m_lo + 1024 + 16] (TEL_NC = 1056 of
//               them: the tile's own 1024 or 1025 and the interpolator's 15 + 16), and those read x[2 (m_lo - 15) - 64 ..] (2 TEL_NXP = 2240
//               staged: the tile and a halo of 64 + 2 * 15 or 16 on either side).
//     stage     x, zero outside [0, n_valid), by 16-byte loads that are only 2-byte aligned, into LDS split by phase, int16 still:
//               s_xe[i] = x[x0 + 2 i], s_xo[i] = x[x0 + 2 i + 1].  The split turns the decimating filter into two stride-1 filters,
//               z[r] = sum_j he[j] xe[r + j] + sum_j ho[j] xo[r + j] (65 and 64 taps).
//     decimate  a thread takes 4 consecutive r.  Its window of 68 samples per phase comes as 17 ds_read_b64 at 8-byte aligned addresses
//               (lane stride 8 bytes: no bank conflict; never the 2-byte aligned wide reads that speed.hip measured as replays), two
//               samples to a register.  Taps travel two to a word as kernel arguments, hence in scalar registers, and a pair of products
//               is one v_dot2_i32_i16: outputs r and r + 2 meet the window's own words, r + 1 and r + 3 the words in between, made by
//               one funnel shift each -- 4 x 129 multiply-adds in 260 dot products and 68 shifts.  1056 = 264 groups of 4: the first
//               eight threads take a second group.  The companded values go back to LDS as int16.
//     output    thread t holds outputs 8 t .. 8 t + 7: four even ones are c itself, four odd ones the same 4-wide filter over c (32 taps).
// Exactness: every product is below 2^15 * 2^15, and the sums run in 32-bit PARTIAL accumulators -- the band-pass's even and odd taps apart,
// the interpolator's two halves apart -- joined in 64 bits before the rounding shift.  A partial sum stays below 65535 * 2^15 < 2^31
// because its group's sum of |tap| stays below 65536, and a tap fits the dot product's int16 operand: tel_tables_bounded
// (telephone_core.h) checks both where the tables are built, and the launcher refuses tables that miss it.  (One 32-bit accumulator per
// filter would wrap: the whole sums reach 2.52e9 and 2.67e9.)
#include "common.h"
#include "kernels.h"
#include "../../include/oasr.h"
#include "telephone_core.h"
#include "pcm_tile.h"

static_assert(OASR_TELEPHONE_MAX_CODECS == TEL_MAX_CODECS, "include/oasr.h and telephone_core.h disagree");

#define TEL_THREADS 256
#define TEL_PER_THREAD 8
#define TEL_TILE (TEL_THREADS * TEL_PER_THREAD)
#define TEL_NC (TEL_TILE / 2 + TEL_UP_TAPS)           // 1056 decimated samples per tile
#define TEL_NXP (TEL_NC + TEL_BP_HALF)                // 1120 staged samples per phase
#define TEL_EVEN_TAPS (TEL_BP_HALF + 1)               // 65: h[k] at even k
#define TEL_ODD_TAPS TEL_BP_HALF                      // 64: h[k] at odd k
#define TEL_WIN_WORDS ((4 + TEL_BP_HALF) / 2)          // 34 words = 68 samples: what 4 outputs of a 64- or 65-tap phase read
#define TEL_UP_WORDS ((4 + TEL_UP_TAPS) / 2)          // 18 words = 36 samples: what 4 odd outputs read
static_assert(TEL_NC % 4 == 0 && TEL_NXP % 4 == 0 && TEL_WIN_WORDS % 2 == 0 && TEL_UP_WORDS % 2 == 0, "windows are read as 8-byte words");
static_assert(TEL_NC - 4 + 2 * TEL_WIN_WORDS <= TEL_NXP, "the last group's window stays inside the staged phase");
static_assert(4 * (TEL_THREADS - 1) + 2 * TEL_UP_WORDS <= TEL_NC, "the last thread's window stays inside c");
static_assert(4 + TEL_EVEN_TAPS - 1 <= 2 * TEL_WIN_WORDS && (TEL_EVEN_TAPS + 1) / 2 + 1 <= TEL_WIN_WORDS,
              "65 even taps: the window holds every sample, and one padding word follows it in registers");
static_assert(TEL_UP_TAPS / 4 + TEL_UP_TAPS / 4 + 2 <= TEL_UP_WORDS, "the second half's window ends inside the 18 words");

typedef __attribute__((ext_vector_type(2))) short s16x2_t;

struct TelTaps {  // the tables as the kernel walks them, two int16 taps to a word (kernel arguments: scalar loads)
  uint32_t he[(TEL_EVEN_TAPS + 1) / 2];  // (he[2 i], he[2 i + 1]), he[j] = h[64 - 2 j], he[65] = 0
  uint32_t ho[TEL_ODD_TAPS / 2];         // (ho[2 i], ho[2 i + 1]), ho[j] = h[63 - 2 j]
  uint32_t u[TEL_UP_TAPS / 2];           // (u[2 i], u[2 i + 1])
};

__device__ __forceinline__ uint32_t tel_pack(int lo, int hi) { return ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16); }
__device__ __forceinline__ int32_t tel_dot2(uint32_t a, uint32_t b, int32_t c) {  // a.lo * b.lo + a.hi * b.hi + c, signed halves, no clamp
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2_t, a), __builtin_bit_cast(s16x2_t, b), c, false);
}

// words[0 .. WORDS) = the int16 samples s[0 .. 2 WORDS), two to a word; s is 8-byte aligned LDS, WORDS even
template <int WORDS>
__device__ __forceinline__ void tel_window(const int16_t* s, uint32_t* words) {
#pragma unroll
  for (int q = 0; q < WORDS / 2; ++q) {
    const u32x2_t v = *(const u32x2_t*)(s + 4 * q);
    words[2 * q] = v[0], words[2 * q + 1] = v[1];
  }
}

// acc[r] = sum_{j < 2 NP} tap[j] * s[r + j], r = 0 .. 3, over the window D = (s[0], s[1]), (s[2], s[3]), ..., of which D[0 .. NP + 1] are read;
// taps: NP words of two.  Outputs 0 and 2 meet the window's own words, outputs 1 and 3 the words in between (one funnel shift each); every
// product pair goes through one v_dot2_i32_i16.  The sums fit 32 bits (the header)
template <int NP>
__device__ __forceinline__ void tel_fir4(const uint32_t* D, const uint32_t* taps, int32_t acc[4]) {
  acc[0] = acc[1] = acc[2] = acc[3] = 0;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const uint32_t t = taps[i];
    acc[0] = tel_dot2(D[i], t, acc[0]);
    acc[1] = tel_dot2(__builtin_amdgcn_alignbit(D[i + 1], D[i], 16), t, acc[1]);
    acc[2] = tel_dot2(D[i + 1], t, acc[2]);
    acc[3] = tel_dot2(__builtin_amdgcn_alignbit(D[i + 2], D[i + 1], 16), t, acc[3]);
  }
}

__global__ __launch_bounds__(TEL_THREADS) void telephone_kernel(oasr_telephone_args a, TelTaps taps) {
  __shared__ __attribute__((aligned(16))) int16_t s_xe[TEL_NXP];
  __shared__ __attribute__((aligned(16))) int16_t s_xo[TEL_NXP];
  __shared__ __attribute__((aligned(16))) int16_t s_c[TEL_NC];
  const int tid = threadIdx.x, b = blockIdx.y, N = a.N;
  const int nv = a.n_valid[b];
  const int codec = tel_row_codec(a.seed, a.first_clip + (uint64_t)b, a.policy.prob_q16, a.policy.n_codecs, a.policy.codecs, nv, N);
  const int16_t* __restrict__ x = a.pcm_in + (size_t)b * (size_t)a.ld_in;
  int16_t* __restrict__ y = a.pcm_out + (size_t)b * (size_t)a.ld_out;
  if (blockIdx.x == 0 && tid == 0 && a.codec_out) a.codec_out[b] = codec;
  const int n_lo = (int)blockIdx.x * TEL_TILE - pcm_lead(y);  // the tile covers [n_lo, n_lo + TILE) of the row; y + n_lo is 16-byte aligned
  if (n_lo >= N) return;
  const int n0 = n_lo + TEL_PER_THREAD * tid;  // this thread's eight samples of the store
  if (codec < 0 || n_lo >= nv) {               // a copied row, or a tile behind the audio (codec >= 0 means 1 <= nv <= N)
    pcm_store8(y, n0, N, pcm_load8(x, n0, N));
    return;
  }
  const int m_lo = n_lo >> 1, odd_first = n_lo & 1;  // (n_lo >= -7: the shift floors)
  const int c0 = m_lo - TEL_UP_LEFT;                 // s_c[r] = c[c0 + r]
  const int x0 = 2 * c0 - TEL_BP_HALF;               // s_xe[i] = x[x0 + 2 i], s_xo[i] = x[x0 + 2 i + 1]
  const int M = (nv + 1) >> 1;

  for (int v = tid; v < TEL_NXP / 4; v += TEL_THREADS) {
    const s16x8_t w = pcm_load8(x, x0 + 8 * v, nv);
    const u32x2_t e = {tel_pack(w[0], w[2]), tel_pack(w[4], w[6])}, o = {tel_pack(w[1], w[3]), tel_pack(w[5], w[7])};
    *(u32x2_t*)(s_xe + 4 * v) = e;
    *(u32x2_t*)(s_xo + 4 * v) = o;
  }
  __syncthreads();

#pragma unroll 1
  for (int g = tid; g < TEL_NC / 4; g += TEL_THREADS) {
    const int r0 = 4 * g, m0 = c0 + r0;
    int32_t c[4] = {0, 0, 0, 0};
    if (m0 + 3 >= 0 && m0 < M) {  // (else: all four lie outside [0, M))
      int32_t z[4];
      if (a.policy.bandpass) {
        uint32_t D[TEL_WIN_WORDS + 1];
        int32_t ze[4], zo[4];
        tel_window<TEL_WIN_WORDS>(s_xe + r0, D);
        D[TEL_WIN_WORDS] = 0;  // (under the zero that pads the 65 even taps to 33 words)
        tel_fir4<(TEL_EVEN_TAPS + 1) / 2>(D, taps.he, ze);
        tel_window<TEL_WIN_WORDS>(s_xo + r0, D);
        tel_fir4<TEL_ODD_TAPS / 2>(D, taps.ho, zo);
#pragma unroll
        for (int i = 0; i < 4; ++i) z[i] = pcm_round_q15((int64_t)ze[i] + (int64_t)zo[i]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) z[i] = s_xe[r0 + TEL_BP_HALF / 2 + i];  // x[2 m]
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) c[i] = (m0 + i >= 0 && m0 + i < M) ? (int)tel_quantize(z[i], codec) : 0;
    }
    const u32x2_t packed = {tel_pack(c[0], c[1]), tel_pack(c[2], c[3])};
    *(u32x2_t*)(s_c + r0) = packed;
  }
  __syncthreads();

  if (n0 >= N) return;
  s16x8_t out;
  if (n0 < nv) {
    // the odd samples 2 m + 1, m = m_lo + 4 tid + i: sum_j u[j] c[m + j - 15] = sum_j u[j] s_c[4 tid + i + j], in two halves of 16 taps
    uint32_t D[TEL_UP_WORDS];
    int32_t lo[4], hi[4];
    tel_window<TEL_UP_WORDS>(s_c + 4 * tid, D);
    tel_fir4<TEL_UP_TAPS / 4>(D, taps.u, lo);
    tel_fir4<TEL_UP_TAPS / 4>(D + TEL_UP_TAPS / 4, taps.u + TEL_UP_TAPS / 4, hi);
    // the even samples 2 m: m = m_lo + 4 tid + i where the tile starts on an even sample, one further where it starts on an odd one
    const int16_t* ce = s_c + TEL_UP_LEFT + odd_first + 4 * tid;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int16_t even = ce[i], odd = pcm_round_q15((int64_t)lo[i] + (int64_t)hi[i]);
      out[2 * i] = odd_first ? odd : even;
      out[2 * i + 1] = odd_first ? even : odd;
    }
    if (n0 + TEL_PER_THREAD > nv) {  // the clip ends inside these eight: the rest is copied
      const s16x8_t x8 = pcm_load8(x, n0, N);
#pragma unroll
      for (int e = 0; e < TEL_PER_THREAD; ++e)
        if (n0 + e >= nv) out[e] = x8[e];
    }
  } else {
    out = pcm_load8(x, n0, N);
  }
  pcm_store8(y, n0, N, out);
}

int launch_telephone(const oasr_telephone_args* a, hipStream_t st) {
  const char* why = tel_args_error(a);
  OASR_REQUIRE(!why, "oasr_telephone: %s", why);
  const TelTables* t = tel_tables_cached();
  OASR_REQUIRE(t, "oasr_telephone: the tap tables miss the bound of the 32-bit partial sums (a group's sum of |tap| above 65535)");
  auto pack = [](int lo, int hi) { return ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16); };
  auto he = [t](int j) { return j < TEL_EVEN_TAPS ? t->h[2 * TEL_BP_HALF - 2 * j] : 0; };
  auto ho = [t](int j) { return t->h[2 * TEL_BP_HALF - 1 - 2 * j]; };
  TelTaps taps;
  for (int i = 0; i < (TEL_EVEN_TAPS + 1) / 2; ++i) taps.he[i] = pack(he(2 * i), he(2 * i + 1));
  for (int i = 0; i < TEL_ODD_TAPS / 2; ++i) taps.ho[i] = pack(ho(2 * i), ho(2 * i + 1));
  for (int i = 0; i < TEL_UP_TAPS / 2; ++i) taps.u[i] = pack(t->u[2 * i], t->u[2 * i + 1]);
  const dim3 grid((unsigned)cdiv((long)a->N + 7, TEL_TILE), (unsigned)a->B);
  hipLaunchKernelGGL(telephone_kernel, grid, dim3(TEL_THREADS), 0, st, *a, taps);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}
