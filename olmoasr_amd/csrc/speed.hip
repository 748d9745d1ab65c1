// Speed perturbation of int16 PCM (include/oasr.h at oasr_speed_perturb; the rule: speed_core.h): seeded integer polyphase resampling, out
// of place, with the transcript's timestamp tokens moved along -- one launch.
//
// One 256-thread workgroup owns SPEED_TILE = 2048 consecutive output samples of one clip.  Every workgroup evaluates the clip's plan itself
// from (seed, clip, n_valid) -- three hashes and one 64-bit remainder of scalar work (draw_core.h) -- so nothing comes back to the host.
// Tiles are laid on the 16-byte grid of the output row (pcm_tile.h), so each thread's 8 samples leave as one aligned 16-byte store.  The two
// staging loads below stay explicit ALIGNED loads on the input row's own grid rather than pcm_load8: that choice was measured.
//   identity row   a vector copy of the whole row
//   tile >= n_out  zeros are stored, nothing is read
//   otherwise      the ratio's Q x 2H table (row stride 2H + 1 words: the 32 lanes of a ds_read_b32 group hold consecutive n, hence
//                  different phases r, and an odd stride puts different rows on different banks; equal r broadcast) and the input window
//                  [m_first - H + 1, m_last + H] (aligned 16-byte loads of int16, zero outside [0, n_valid)) go to LDS.  The window is kept
//                  there as sign-extended 32-bit words: a tap loop over int16 LDS is merged into ds_read_b64 at addresses that are only
//                  2-byte aligned, which CDNA4 replays at 64 cycles each (measured here: 5.9 us per clip at 11/10 that way); over 32-bit
//                  words the same loop reads with ds_read2_b32, which needs no more than its 4-byte alignment.  Thread t computes
//                  outputs t, t + 256, ... of the tile -- neighbouring lanes read neighbouring input samples -- with an exact 64-bit sum
//                  (v_mad_i64_i32), leaves them in LDS, and after a barrier stores samples 8t .. 8t + 7.
// The workgroup of a clip's first tile also rewrites the clip's timestamp tokens and reports n_out / factor.
#include <map>
#include <mutex>
#include <tuple>

#include "common.h"
#include "kernels.h"
#include "../../include/oasr.h"
#include "speed_core.h"
#include "pcm_tile.h"

static_assert(OASR_SPEED_MAX_FACTORS == SPEED_MAX_FACTORS, "include/oasr.h and speed_core.h disagree");

#define SPEED_THREADS 256
#define SPEED_PER_THREAD 8
#define SPEED_TILE (SPEED_THREADS * SPEED_PER_THREAD)
#define SPEED_TSTRIDE_MAX (2 * SPEED_MAX_H + 1)
// input window of a tile: at most 2 (TILE - 1) + 1 + 2H samples, + 7 in front and + 7 behind for the 16-byte grid of the loads
#define SPEED_XBUF (2 * SPEED_TILE + 2 * SPEED_MAX_H + 28)
static_assert(SPEED_XBUF % 8 == 0 && SPEED_XBUF >= 2 * (SPEED_TILE - 1) + 1 + 2 * SPEED_MAX_H + 14, "the staged window does not fit");

typedef __attribute__((ext_vector_type(4))) int i32x4_t;

struct SpeedTables {  // device copies of the policy's tables (nullptr / 0 for an identity factor)
  const int32_t* tab[SPEED_MAX_FACTORS];
  int32_t H[SPEED_MAX_FACTORS];
};

__global__ __launch_bounds__(SPEED_THREADS) void speed_perturb_kernel(oasr_speed_args a, SpeedTables tabs) {
  __shared__ __attribute__((aligned(16))) int32_t s_x[SPEED_XBUF];
  __shared__ __attribute__((aligned(16))) int16_t s_y[SPEED_TILE];
  __shared__ int32_t s_T[SPEED_MAX_PQ * SPEED_TSTRIDE_MAX];
  const int tid = threadIdx.x, b = blockIdx.y, N = a.N;
  const int nv = a.n_valid[b];
  const int choice = speed_choice(a.seed, a.first_clip + (uint64_t)b, a.policy.n_factors);
  int P = 1, Q = 1, H = 0;
  const int32_t* tab = nullptr;
#pragma unroll
  for (int i = 0; i < SPEED_MAX_FACTORS; ++i)  // (a select per slot: no indexed copy of the policy in scratch)
    if (i == choice) P = a.policy.P[i], Q = a.policy.Q[i], H = tabs.H[i], tab = tabs.tab[i];
  const SpeedPlan pl = speed_plan_of(choice, P, Q, nv, N);
  P = pl.P, Q = pl.Q;
  const int16_t* __restrict__ x = a.pcm_in + (size_t)b * (size_t)a.ld_in;
  int16_t* __restrict__ y = a.pcm_out + (size_t)b * (size_t)a.ld_out;
  const int lead = pcm_lead(y);
  const int n_lo = (int)blockIdx.x * SPEED_TILE - lead;  // the tile covers [n_lo, n_lo + TILE) of the row; y + n_lo is 16-byte aligned
  if (n_lo >= N) return;
  const int n_hi = n_lo + SPEED_TILE < N ? n_lo + SPEED_TILE : N;
  const int n0 = n_lo + SPEED_PER_THREAD * tid;          // this thread's eight samples of the store

  if (blockIdx.x == 0) {
    if (tid == 0) {
      if (a.n_out) a.n_out[b] = pl.n_out;
      if (a.factor_out) a.factor_out[b] = pl.factor;
    }
    if (P != Q) {  // (an identity maps every token to itself; a row outside the contract has P = Q = 1)
      int64_t* ta = a.tokens_a ? a.tokens_a + (size_t)b * (size_t)a.ld_tokens_a : nullptr;
      int64_t* tb = a.tokens_b ? a.tokens_b + (size_t)b * (size_t)a.ld_tokens_b : nullptr;
      for (int s = tid; s < a.S; s += SPEED_THREADS) {
        if (ta) ta[s] = speed_token(ta[s], a.ts_begin, a.ts_max, P, Q);
        if (tb) tb[s] = speed_token(tb[s], a.ts_begin, a.ts_max, P, Q);
      }
    }
  }

  if (P == Q) {  // a copy of the row
    s16x8_t v;
    if (n0 >= 0 && n0 + 8 <= N && (((uintptr_t)(x + n0)) & 15) == 0) {
      v = *(const s16x8_t*)(x + n0);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (n0 + e >= 0 && n0 + e < N) ? x[n0 + e] : (int16_t)0;
    }
    pcm_store8(y, n0, N, v);
    return;
  }

  const int n_beg = n_lo > 0 ? n_lo : 0;
  const int n_end = n_hi < pl.n_out ? n_hi : pl.n_out;  // samples [n_beg, n_end) of the tile carry audio
  if (n_beg >= n_end) {                                 // at or past n_out: zeros, and nothing is read
    const s16x8_t z = {0, 0, 0, 0, 0, 0, 0, 0};
    pcm_store8(y, n0, N, z);
    return;
  }

  const int taps = 2 * H, tstride = taps + 1;
  for (int i = tid; i < Q * taps; i += SPEED_THREADS) {
    const int r = i / taps;
    s_T[r * tstride + (i - r * taps)] = tab[i];
  }
  // the window [w0, w1] of the input that the tile's samples read, staged from the 16-byte boundary g0 at or before w0
  const int m_first = (int)(((int64_t)n_beg * P) / Q), m_last = (int)(((int64_t)(n_end - 1) * P) / Q);
  const int w0 = m_first - H + 1, w1 = m_last + H;
  const int in_lead = pcm_lead(x);
  const int g0 = w0 - ((w0 + in_lead) & 7);
  const int n_vec = (w1 - g0 + 8) >> 3;  // <= SPEED_XBUF / 8 (the static_assert above)
  for (int v = tid; v < n_vec; v += SPEED_THREADS) {
    const int i0 = g0 + 8 * v;
    s16x8_t w;
    if (i0 >= 0 && i0 + 8 <= nv) {
      w = *(const s16x8_t*)(x + i0);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) w[e] = (i0 + e >= 0 && i0 + e < nv) ? x[i0 + e] : (int16_t)0;
    }
    const i32x4_t lo = {w[0], w[1], w[2], w[3]}, hi = {w[4], w[5], w[6], w[7]};
    *(i32x4_t*)(s_x + 8 * v) = lo;
    *(i32x4_t*)(s_x + 8 * v + 4) = hi;
  }
  __syncthreads();

  // outputs n_lo + tid + 256 i: (m, r) advance by a constant, so the division by Q runs once per thread
  const int64_t np = (int64_t)(n_lo + tid) * P;  // (n_lo + tid may be negative in a row's first tile: those samples are not computed)
  int m = (int)(np >= 0 ? np / Q : -((-np + Q - 1) / Q));
  int r = (int)(np - (int64_t)m * Q);
  const int dm = (SPEED_THREADS * P) / Q, dr = (SPEED_THREADS * P) % Q;
#pragma unroll 1
  for (int i = 0; i < SPEED_PER_THREAD; ++i) {
    const int v = tid + SPEED_THREADS * i, n = n_lo + v;
    int16_t out = 0;
    if (n >= n_beg && n < n_end) {
      const int32_t* xs = s_x + (m - H + 1 - g0);  // >= s_x + (w0 - g0), and xs + taps - 1 <= s_x + (w1 - g0)
      const int32_t* ts = s_T + r * tstride;
      int64_t acc = 0;
      for (int j = 0; j < taps; ++j) acc += (int64_t)xs[j] * ts[j];
      out = pcm_round_q15(acc);
    }
    s_y[v] = out;
    m += dm, r += dr;
    if (r >= Q) r -= Q, ++m;
  }
  __syncthreads();
  pcm_store8(y, n0, N, *(const s16x8_t*)(s_y + SPEED_PER_THREAD * tid));
}

// the device copy of a ratio's table on the current device: uploaded on first use (like the log-mel tables), kept for the process
static int speed_device_table(int P, int Q, const int32_t** tab, int* H) {
  static std::mutex mu;
  static std::map<std::tuple<int, int, int>, int32_t*> tables;
  int dev = 0;
  OASR_CHECK_HIP(hipGetDevice(&dev));
  const int32_t* host = speed_table_cached(P, Q, H);
  std::lock_guard<std::mutex> lock(mu);
  int32_t*& d = tables[std::make_tuple(dev, P, Q)];
  if (!d) {
    const size_t bytes = sizeof(int32_t) * (size_t)Q * 2 * (size_t)*H;
    int32_t* p = nullptr;
    OASR_CHECK_HIP(hipMalloc((void**)&p, bytes));
    if (hipMemcpy(p, host, bytes, hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(p);
      oasr_set_error("oasr_speed_perturb: uploading the %d / %d table failed", P, Q);
      return OASR_EHIP;
    }
    d = p;
  }
  *tab = d;
  return OASR_OK;
}

int launch_speed_perturb(const oasr_speed_args* a, hipStream_t st) {
  const char* why = speed_args_error(a);
  OASR_REQUIRE(!why, "oasr_speed_perturb: %s", why);
  SpeedTables tabs;
  memset(&tabs, 0, sizeof(tabs));
  for (int i = 0; i < a->policy.n_factors; ++i) {
    if (a->policy.P[i] == a->policy.Q[i]) continue;
    int H = 0;
    const int rc = speed_device_table(a->policy.P[i], a->policy.Q[i], &tabs.tab[i], &H);
    if (rc) return rc;
    OASR_REQUIRE(H >= 1 && H <= SPEED_MAX_H, "oasr_speed_perturb: H = %d of %d / %d outside [1, %d]", H, a->policy.P[i], a->policy.Q[i], SPEED_MAX_H);
    tabs.H[i] = H;
  }
  const dim3 grid((unsigned)cdiv((long)a->N + 7, SPEED_TILE), (unsigned)a->B);
  hipLaunchKernelGGL(speed_perturb_kernel, grid, dim3(SPEED_THREADS), 0, st, *a, tabs);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}
