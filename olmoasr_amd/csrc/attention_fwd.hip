// Flash attention forward (attention.hip has the overview): the tiled kernel, and the one-row kernel of the KV-cached decode step.
#include "attention_common.h"

namespace {

// Lazy rescale (log2 domain): the running reference maximum is only raised -- and O / l only rescaled -- when some row of
// the wave grows past it by more than this; until then P = exp2(s - m_ref) <= 2^8, harmless in fp32 / bf16.
constexpr float RESCALE_THR = 8.0f;

// ------------------------------------------------------------------------------------------------------------
// ROWS: the query side (and, when a.k_rows is set, the key side) lives in chunked token rows (kernels.h) -- the decoder of a
// span-limited training step.  ROWS == false is the plain strided layout and compiles to exactly the code it always was.
template <bool CAUSAL, bool ROWS>
__global__ __launch_bounds__(256, 3) void attn_fwd_kernel(AttnArgs a) {
  // K/V tiles move global -> LDS by DMA, two tiles ahead through a 3-stage ring (3 x 16 KiB per workgroup, three workgroups per CU): no staging
  // registers, no commit stores, and a tile has a whole iteration to land before anybody waits for it.  The ONE barrier of an iteration sits
  // between the softmax and the O^T MFMAs: it releases tile t+1, whose first four K fragments are then read under the O^T MFMAs of tile t, so the
  // next iteration's S^T MFMAs start without an LDS round trip.  (In-kernel cycle stamps of the register-staged form it replaces,
  // profiles/r04_attention_forward_stamps.txt: of a wave's 3400 cycles per tile 600 went into waiting for the next tile's global loads and
  // writing them to LDS, 870 into the K fragment round trip + S^T issue.  Results are bit-identical to that form: scripts/attn_crc.py.)
  __shared__ __attribute__((aligned(1024))) char smem[3 * 2 * TILE];  // stage s: K at 2s*TILE, V at (2s+1)*TILE
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> 5;
  // 1-D grid, XCD-aware: all query blocks of one (batch, head) run on the same XCD so K/V are filled into that XCD's
  // L2 once and re-used by the other query blocks (round-robin dispatch would fetch them through all 8 L2s).
  const int nqb = (a.Tq + 127) >> 7;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const BlockId id = block_id<ROWS>(a.qblk128, bid, nqb, a.H);
  const int b = id.b, h = id.h, qblk = id.blk;
  const int q0 = qblk * 128;
  const int myq = q0 + wave * 32 + (lane & 31);
  const int myq_c = myq < a.Tq ? myq : a.Tq - 1;
  const bool krows = ROWS && a.k_rows != nullptr;  // (block-uniform)
  // span-limited FORWARD (opt-in of the span step): query positions >= q_span[b] are not computed at all -- no output row written
  const int q_lim = (ROWS && a.q_span) ? min(a.q_span[b], a.Tq) : a.Tq;
  if (ROWS && q0 >= q_lim) return;  // (block-uniform, before any barrier)
  const bool w_act = !ROWS || q0 + wave * 32 < q_lim;  // (wave-uniform) an inactive wave computes on whatever its rows hold and stores nothing

  const bf16_t* qp = row_at(a.q, ROWS, a.q_rows, b, myq_c, a.ldq, a.bsq, h);
  bf16x8_t qf[4];
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) qf[ds] = ld_frag_global(qp + ds * 16 + hh * 8);

  const int kv_len = clamped_kv_len(a, b);
  int kv_end = kv_len;
  if (CAUSAL) kv_end = kv_end < q0 + 128 ? kv_end : q0 + 128;
  const int ntiles = kv_end > 0 ? (kv_end + 63) >> 6 : 1;  // >= 1: a fully masked tile yields l = 0 -> O = 0

  // first row of key tile t (64 keys = one chunk)
  auto krow0 = [&](int t) { return krows ? __builtin_amdgcn_readfirstlane(a.k_rows[b * OASR_ROWTAB + t]) : t * 64; };
  const PipeSrc1 ksrc = krows ? pipe_src1(a.k + h * 64, a.ldk, a.B * a.Tk, wave, lane) : pipe_src1(a.k + (long)b * a.bsk + h * 64, a.ldk, a.Tk, wave, lane);
  const PipeSrc1 vsrc = krows ? pipe_src1(a.v + h * 64, a.ldv, a.B * a.Tk, wave, lane) : pipe_src1(a.v + (long)b * a.bsv + h * 64, a.ldv, a.Tk, wave, lane);
  const unsigned smem_a = (unsigned)(size_t)smem;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);  // (the DMA's LDS base travels in m0: a scalar)
  const unsigned krb = (unsigned)(a.ldk * 2), vrb = (unsigned)(a.ldv * 2);
  // this wave's four 1 KiB pieces of key tile t2 (rows 8w.. and 32+8w.. of K and of V); tiles past the last one read as zeros (offset out of range)
  auto dma_tile = [&](int t2, int stage) {
    unsigned ko = 0x7fffff00u, vo = 0x7fffff00u;
    if (t2 < ntiles) {
      const unsigned r0 = (unsigned)krow0(t2);
      ko = ksrc.voff + r0 * krb;
      vo = vsrc.voff + r0 * vrb;
    }
    const unsigned dst = smem_a + stage * 2 * TILE + wave_u * 1024;
    glds16_asm(ksrc.rs, dst, ko);
    glds16_asm(ksrc.rs, dst + 4096, ko + 32 * krb);
    glds16_asm(vsrc.rs, dst + TILE, vo);
    glds16_asm(vsrc.rs, dst + TILE + 4096, vo + 32 * vrb);
  };

  f32x16_t oT[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) oT[i][r] = 0.f;
  float m_run = NEG;
  f32x2_t l_run2 = {0.f, 0.f};

  // Ring protocol (every wave issues 4 pieces per tile; vmcnt counts them in order):
  //   prologue      : tiles 0, 1 in flight; wait for tile 0 (vmcnt(4)) + barrier; K fragments (first 32 keys) of tile 0
  //   iteration t   : S^T MFMAs on tile t | softmax | vmcnt(0) + barrier: tile t+1 has landed for everybody and everybody is past its reads of
  //                   tile t-1 | DMA of tile t+2 into tile t-1's stage | K fragments of tile t+1 | O^T MFMAs on tile t
  asm volatile("" ::"v"(qf[0]), "v"(qf[1]), "v"(qf[2]), "v"(qf[3]));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the Q fragments; from here on the loop counts its own DMA pieces)
  dma_tile(0, 0);
  dma_tile(1, 1);
  int stg = 0;
  asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  ATTN_BARRIER();
  bf16x8_t kf0[4];
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) kf0[ds] = frag_rows(smem, 0, ds, lane);
  for (int t = 0; t < ntiles; ++t) {
    const char* kb = smem + stg * 2 * TILE;
    const char* vb = kb + TILE;
    stg = stg == 2 ? 0 : stg + 1;
    f32x16_t sT[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sT[kt][r] = 0.f;
#pragma unroll
      for (int ds = 0; ds < 4; ++ds) sT[kt] = MFMA(kt == 0 ? kf0[ds] : frag_rows(kb, 32, ds, lane), qf[ds], sT[kt]);
    }
    // Only boundary tiles need the per-element mask (wave-uniform test): last partial tile of kv_len, and for the
    // causal case the tiles that cross this wave's diagonal.  Scores stay raw; the softmax scale rides in the fma.
    constexpr float C = SCALE * LOG2E;
    const int q_lo = q0 + wave * 32;  // smallest query row of this wave
    const bool full = (t * 64 + 64 <= kv_len) && (!CAUSAL || (t * 64 + 63 <= q_lo));
    float m_tile = NEG;
    if (full) {
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) m_tile = fmaxf(m_tile, sT[kt][r]);
    } else {
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = t * 64 + kt * 32 + acc_row(r, hh);
          const bool ok = (key < kv_len) && (!CAUSAL || key <= myq);
          const float sv = ok ? sT[kt][r] : NEG;
          sT[kt][r] = sv;
          m_tile = fmaxf(m_tile, sv);
        }
    }
    m_tile = fmaxf(m_tile, __shfl_xor(m_tile, 32, 64));
    const float m_cand = m_tile * C;  // NEG * C stays hugely negative
    if (__any(m_cand > m_run + RESCALE_THR)) {  // wave-uniform; rare after the first tiles
      const float m_new = fmaxf(m_run, m_cand);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      const f32x2_t a2 = {alpha, alpha};
      l_run2 *= a2;
      m_run = m_new;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          f32x2_t o2 = {oT[dt][r], oT[dt][r + 1]};
          o2 *= a2;
          oT[dt][r] = o2[0];
          oT[dt][r + 1] = o2[1];
        }
    }
    {
      const float nm = -m_run;
      float ps0 = 0.f, ps1 = 0.f;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          const float p0 = __builtin_amdgcn_exp2f(fmaf(sT[kt][r], C, nm));
          const float p1 = __builtin_amdgcn_exp2f(fmaf(sT[kt][r + 1], C, nm));
          sT[kt][r] = p0;
          sT[kt][r + 1] = p1;
          ps0 += p0;
          ps1 += p1;
        }
      l_run2[0] += ps0;
      l_run2[1] += ps1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of tile t+1 have landed
    ATTN_BARRIER();                                    // ... and everybody's; everybody is past the O^T reads of tile t-1: its stage is free
    dma_tile(t + 2, stg == 2 ? 0 : stg + 1);           // (stg already names tile t+1's stage)
    if (t + 1 < ntiles) {
#pragma unroll
      for (int ds = 0; ds < 4; ++ds) kf0[ds] = frag_rows(smem + stg * 2 * TILE, 0, ds, lane);
    }
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const bf16x8_t pf = pack_half(sT[kt], u);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) oT[dt] = MFMA(frag_cols(vb, kt * 32 + 16 * u, dt * 32, lane), pf, oT[dt]);
      }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the tail pieces (zeros) must not land on the staging tiles below
  __syncthreads();

  const float l_run = l_run2[0] + l_run2[1];
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
  {
    // (the loop ended on a barrier: the K/V stages are free; 4 KiB of staging per wave)
    char* stg = smem + wave * 4096;
    const int rows_valid = w_act ? a.Tq - (q0 + wave * 32) : 0;  // may be <= 0 or > 32
    // (a wave's 32 rows lie inside one chunk; past Tq the table entry is a sentinel and rows_valid <= 0 keeps it unused)
    const long row0 = row_at(0L, ROWS, a.q_rows, b, q0 + wave * 32, a.ldo, a.bso, h);
    store_rows_bf16(stg, oT, inv, a.o + row0, a.ldo, rows_valid, lane);
    // rounding residual of O for the backward's delta term (bf16 O alone loses it when mean(V) dominates V's variation;
    // O + residual is fp32-grade at 4 bytes per element instead of 2 + 4)
    if (a.o_lo) {
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float v = oT[dt][r] * inv;
          oT[dt][r] = v - bf_round(v);
        }
      store_rows_bf16(stg, oT, 1.0f, a.o_lo + row0, a.ldo, rows_valid, lane);
    }
    if (myq < a.Tq && hh == 0 && a.lse && w_act) a.lse[((long)b * a.H + h) * a.Tq + myq] = (m_run + __builtin_amdgcn_logf(l_tot)) * LN2;
  }
}

// ------------------------------------------------------------------------------------------------------------
// One query row per (batch, head): the KV-cached decode step (Tq == 1).  The 128-row flash tile above spends a whole
// workgroup's prologue/epilogue on one row (measured 16 us per call, 27 % of a decode step); here a workgroup streams
// the K rows once (8 lanes x 16 bytes per key, 32 keys per pass), keeps the scores in LDS, and streams V once.
// Numerics as the tiled kernel: fp32 scores and normaliser, P rounded to bf16 before it multiplies V.
// Keys are taken in segments of <= dec::SEG_KEYS with their own maximum, merged in order (decode_shared.h): the arithmetic the
// one-launch step engine (decode_xcd.hip) spreads over workgroups -- the two are bit-identical; one segment (every self-attention)
// is the plain two-pass softmax.
__global__ __launch_bounds__(256) void attn_decode_kernel(AttnArgs a) {
  __shared__ float sc[dec::SEG_KEYS];
  __shared__ float red[32][64];
  __shared__ float lsum[32];
  __shared__ float wmax[4];
  const int tid = threadIdx.x, l8 = tid & 7, grp = tid >> 3, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.x / a.H, h = blockIdx.x - b * a.H;
  const int Tk = clamped_kv_len(a, b);
  float qv[8];
  dec::load_q8(*(const u32x4_t*)(a.q + (long)b * a.bsq + h * 64 + l8 * 8), qv);
  const bf16_t* kp = a.k + (long)b * a.bsk + h * 64 + l8 * 8;
  const bf16_t* vp = a.v + (long)b * a.bsv + h * 64 + l8 * 8;
  const int ns = dec::n_segments(a.Tk);  // (the segmentation follows the cache extent, not kv_len: a row's result does not depend on its neighbours)
  float m_s[dec::MAX_SEG] = {NEG, NEG}, l_s[dec::MAX_SEG] = {0.f, 0.f}, o_s[dec::MAX_SEG] = {0.f, 0.f};
#pragma unroll
  for (int sg = 0; sg < dec::MAX_SEG; ++sg) {
    if (sg >= ns) break;
    const int k0 = sg * dec::SEG_KEYS;
    int n = Tk - k0;  // keys of this segment
    n = n < 0 ? 0 : (n > dec::SEG_KEYS ? dec::SEG_KEYS : n);
    float mx = NEG;
    for (int t0 = grp; t0 < n; t0 += 32 * 8) {  // 8 independent 16-byte loads in flight per lane
      u32x4_t k4[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int t = t0 + 32 * u;
        k4[u] = *(const u32x4_t*)(kp + (long)(k0 + (t < n ? t : n - 1)) * a.ldk);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int t = t0 + 32 * u;
        const float s2 = dec::score8(qv, k4[u]);
        if (t < n) {
          if (l8 == 0) sc[t] = s2;
          mx = fmaxf(mx, s2);
        }
      }
    }
    mx = wave_max(mx);
    if (lane == 0) wmax[wave] = mx;
    __syncthreads();
    const float m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    float l = 0.f, o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = 0.f;
    for (int t0 = grp; t0 < n; t0 += 32 * 8) {
      u32x4_t v4[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int t = t0 + 32 * u;
        v4[u] = *(const u32x4_t*)(vp + (long)(k0 + (t < n ? t : n - 1)) * a.ldv);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int t = t0 + 32 * u;
        dec::accum_pv(t < n ? __builtin_amdgcn_exp2f(sc[t] - m) : 0.f, v4[u], l, o);
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) red[grp][l8 * 8 + j] = o[j];
    if (l8 == 0) lsum[grp] = l;
    __syncthreads();
    if (tid < 64) {
      dec::reduce_groups(red, lsum, tid, o_s[sg], l_s[sg]);
      m_s[sg] = m;
    }
    __syncthreads();  // sc / red / lsum / wmax are reused by the next segment
  }
  if (tid < 64) {
    float m, lt;
    const float val = dec::merge_segments(m_s, l_s, o_s, ns, m, lt);
    const float nb = __shfl_xor(val, 1, 64);
    if ((tid & 1) == 0) *(uint32_t*)(a.o + (long)b * a.bso + h * 64 + tid) = pack_bf2(val, nb);
    if (tid == 0 && a.lse) a.lse[(long)b * a.H + h] = lt > 0.f ? (m + __builtin_amdgcn_logf(lt)) * LN2 : NEG;
  }
}

}  // namespace

void attn_launch_fwd(const AttnArgs& a, dim3 grid, hipStream_t s) {
  static void (*const kern[2][2])(AttnArgs) = {{attn_fwd_kernel<false, false>, attn_fwd_kernel<false, true>},  // [causal][chunked rows]
                                               {attn_fwd_kernel<true, false>, attn_fwd_kernel<true, true>}};
  hipLaunchKernelGGL(kern[a.causal != 0][a.q_rows != nullptr], grid, dim3(256), 0, s, a);
}

void attn_launch_decode(const AttnArgs& a, hipStream_t s) { hipLaunchKernelGGL(attn_decode_kernel, dim3(a.B * a.H), dim3(256), 0, s, a); }
