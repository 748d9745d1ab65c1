// Flash attention backward, dK/dV side (attention.hip has the overview): the general kernel and the ping-pong kernel of the unmasked case.
// Both read the delta rows and the d_o tile flags that the dQ kernel of the same backward call has written.
#include "attention_common.h"

namespace {

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}

// ------------------------------------------------------------------------------------------------------------
// dK[k][:] = scale * sum_q dS[q][k] Q[q][:],  dV[k][:] = sum_q P[q][k] dO[q][:]
// index of the last 64-query tile whose d_o the dQ kernel found non-zero (-1: none); every wave computes it for itself
__device__ __forceinline__ int last_nonzero_qtile(const int32_t* flags, int n, int lane) {
  int last = -1;
  for (int i = lane; i < n; i += 64)
    if (flags[i] != 0) last = i;
  return __builtin_amdgcn_readfirstlane(wave_max_i(last));
}

template <bool CAUSAL, bool ROWS>
__global__ __launch_bounds__(256, 2) void attn_bwd_dkdv_kernel(AttnArgs a) {
  // stage s: Q tile, dO tile, then lse[64] | delta[64] floats
  constexpr int STAGE = 2 * TILE + 512;
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> 5;
  const int nkb = (a.Tk + 127) >> 7;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  // (a block table here is the query-block table of a self-attention over chunked key rows: the key blocks past the span are the empty ones)
  const BlockId id = block_id<ROWS>(a.qblk128, bid, nkb, a.H);
  const int b = id.b, h = id.h, kblk = id.blk;
  const int k0 = kblk * 128;
  const int mykey = k0 + wave * 32 + (lane & 31);
  const bool krows = ROWS && a.k_rows != nullptr;  // (block-uniform) chunked key rows: decoder self-attention
  // span-limited backward: query positions >= q_span[b] hold no gradient (their d_o rows are never read); with chunked key rows the
  // same positions are keys no supervised query sees -- their dk / dv rows lie outside the active rows and are not written
  const int q_lim = (ROWS && a.q_span) ? min(a.q_span[b], a.Tq) : a.Tq;
  const long dv_scratch_off0 = (long)a.B * ((a.Tq + 127) >> 7) * a.H * 64;
  if (krows && a.q_span && k0 >= q_lim) {
    if (a.dv_colsum && tid < 64) a.colsum_scratch[dv_scratch_off0 + ((long)(b * nkb + kblk) * a.H + h) * 64 + tid] = 0.f;
    return;
  }
  const bool w_store = !(krows && a.q_span) || k0 + wave * 32 < q_lim;  // (wave-uniform)
  const int mykey_c = !w_store ? k0 + (lane & 31) : (mykey < a.Tk ? mykey : a.Tk - 1);

  const int kv_len = clamped_kv_len(a, b);

  const bf16_t* kp = row_at(a.k, krows, a.k_rows, b, mykey_c, a.ldk, a.bsk, h);
  const bf16_t* vp = row_at(a.v, krows, a.k_rows, b, mykey_c, a.ldv, a.bsv, h);
  bf16x8_t kf[4], vf[4];
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) {
    kf[ds] = ld_frag_global(kp + ds * 16 + hh * 8);
    vf[ds] = ld_frag_global(vp + ds * 16 + hh * 8);
  }
  f32x16_t dkT[2], dvT[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      dkT[i][r] = 0.f;
      dvT[i][r] = 0.f;
    }

  const TileSrc qsrc = ROWS ? tile_src(a.q + h * 64, a.ldq, a.B * a.Tq, tid) : tile_src(a.q + (long)b * a.bsq + h * 64, a.ldq, a.Tq, tid);
  const TileSrc dosrc = ROWS ? tile_src(a.d_o + h * 64, a.ldo, a.B * a.Tq, tid) : tile_src(a.d_o + (long)b * a.bso + h * 64, a.ldo, a.Tq, tid);
  const float* lse_b = a.lse + ((long)b * a.H + h) * a.Tq;
  const float* delta_b = a.delta + ((long)b * a.H + h) * a.Tq;

  int nqt = (a.Tq + 63) >> 6;
  if (a.qtile_flags) nqt = last_nonzero_qtile(a.qtile_flags + ((long)b * a.H + h) * nqt, nqt, lane) + 1;  // d_o is zero past it
  if (ROWS && (q_lim >> 6) < nqt) nqt = q_lim >> 6;
  const int t_begin = (CAUSAL && k0 < kv_len) ? (k0 >> 6) : 0;
  const bool any = k0 < kv_len && t_begin < nqt;  // otherwise every P (or every d_o row) is zero: fall through and write zeros

  u32x4_t rq[2], rd[2];
  float rstat = 0.f;
  auto issue = [&](int t) {
    const int qr0 = ROWS ? __builtin_amdgcn_readfirstlane(a.q_rows[b * OASR_ROWTAB + t]) : t * 64;
    tile_issue(qsrc, qr0, rq);
    tile_issue(dosrc, qr0, rd);
    if (tid < 128) {
      int qi = t * 64 + (tid & 63);
      qi = qi < a.Tq ? qi : a.Tq - 1;
      rstat = tid < 64 ? lse_b[qi] * LOG2E : delta_b[qi];
    }
  };
  auto commit = [&](char* st) {
    tile_commit(st, tid, rq);
    tile_commit(st + TILE, tid, rd);
    if (tid < 128) ((float*)(st + 2 * TILE))[tid] = rstat;
  };
  // dv partial rows live behind the dq ones: [B * ceil(Tq/128)][H*64] then [B * ceil(Tk/128)][H*64]
  const long dv_scratch_off = dv_scratch_off0;
  if (!any) {  // every key of this block is padding: dK = dV = 0 (uniform early exit, before any load is issued)
    if (a.dv_colsum && tid < 64) a.colsum_scratch[dv_scratch_off + ((long)(b * nkb + kblk) * a.H + h) * 64 + tid] = 0.f;
    if (mykey < a.Tk && w_store) {
      bf16_t* dkp0 = row_at(a.dk, krows, a.k_rows, b, mykey, a.ldk, a.bsk, h);
      bf16_t* dvp0 = row_at(a.dv, krows, a.k_rows, b, mykey, a.ldv, a.bsv, h);
      const u32x4_t z = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        *(u32x4_t*)(dkp0 + hh * 32 + i * 8) = z;
        *(u32x4_t*)(dvp0 + hh * 32 + i * 8) = z;
      }
    }
    return;
  }
  // unconditional prologue: see attn_bwd_dq_kernel, attention_bwd_dq.hip (a guarded one makes hipcc re-wait the prefetch at the loop top)
  issue(t_begin);
  commit(smem);
  __syncthreads();
  for (int t = t_begin; t < nqt; ++t) {
    const int cur = (t - t_begin) & 1;
    const char* st = smem + cur * STAGE;
    const char* qb = st;
    const char* dob = st + TILE;
    const float* stat = (const float*)(st + 2 * TILE);
    const bool more = t + 1 < nqt;
    if (more) issue(t + 1);
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      f32x16_t s, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[r] = 0.f;
        dp[r] = 0.f;
      }
#pragma unroll
      for (int ds = 0; ds < 4; ++ds) {
        s = MFMA(frag_rows(qb, qt * 32, ds, lane), kf[ds], s);
        dp = MFMA(frag_rows(dob, qt * 32, ds, lane), vf[ds], dp);
      }
      const int key_hi = k0 + wave * 32 + 31;  // largest key of this wave
      const bool full = (t * 64 + qt * 32 + 32 <= a.Tq) && (key_hi < kv_len) && (!CAUSAL || key_hi <= t * 64 + qt * 32);
      if (full) {  // wave-uniform: no masks, pairs of queries per packed instruction
        const f32x2_t c2 = {SCALE * LOG2E, SCALE * LOG2E};
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int ql = qt * 32 + 8 * g4 + 4 * hh;
          const f32x4_t l4 = *(const f32x4_t*)(stat + ql);
          const f32x4_t d4 = *(const f32x4_t*)(stat + 64 + ql);
#pragma unroll
          for (int i = 0; i < 4; i += 2) {
            const int r = 4 * g4 + i;
            const f32x2_t s2 = {s[r], s[r + 1]}, dp2 = {dp[r], dp[r + 1]}, nl2 = {-l4[i], -l4[i + 1]}, nd2 = {-d4[i], -d4[i + 1]};
            const f32x2_t p2 = pk_exp2(pk_fma(s2, c2, nl2));
            const f32x2_t ds2 = p2 * (dp2 + nd2);
            s[r] = p2[0];
            s[r + 1] = p2[1];
            dp[r] = ds2[0];
            dp[r + 1] = ds2[1];
          }
        }
      } else {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int ql = qt * 32 + 8 * g4 + 4 * hh;
          const f32x4_t l4 = *(const f32x4_t*)(stat + ql);
          const f32x4_t d4 = *(const f32x4_t*)(stat + 64 + ql);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int r = 4 * g4 + i;
            const int qg = t * 64 + ql + i;
            const bool ok = (qg < a.Tq) && (mykey < kv_len) && (!CAUSAL || mykey <= qg);
            const float p = ok ? __builtin_amdgcn_exp2f(fmaf(s[r], SCALE * LOG2E, -l4[i])) : 0.f;
            s[r] = p;
            dp[r] = p * (dp[r] - d4[i]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const bf16x8_t pf = pack_half(s, u);
        const bf16x8_t dsf = pack_half(dp, u);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          dvT[dt] = MFMA(frag_cols(dob, qt * 32 + 16 * u, dt * 32, lane), pf, dvT[dt]);
          dkT[dt] = MFMA(frag_cols(qb, qt * 32 + 16 * u, dt * 32, lane), dsf, dkT[dt]);
        }
      }
    }
    if (more) commit(smem + (cur ^ 1) * STAGE);
    __syncthreads();
  }
  {
    char* stg = smem + wave * 4096;  // the loop ended on a barrier: both stages are free
    const int rows_valid = w_store ? a.Tk - (k0 + wave * 32) : 0;
    // (the conditional is spelled out here: row_at changed the instruction stream of the chunked-row instantiations)
    const long krow0 = krows ? (long)chunk_row(a.k_rows, b, k0 + wave * 32) : 0;
    store_rows_bf16(stg, dkT, SCALE, krows ? a.dk + krow0 * a.ldk + h * 64 : a.dk + (long)b * a.bsk + (long)(k0 + wave * 32) * a.ldk + h * 64,
                    a.ldk, rows_valid, lane);
    float* wsum = (float*)(smem + 16384);
    store_rows_bf16(stg, dvT, 1.0f, krows ? a.dv + krow0 * a.ldv + h * 64 : a.dv + (long)b * a.bsv + (long)(k0 + wave * 32) * a.ldv + h * 64,
                    a.ldv, rows_valid, lane, a.dv_colsum ? wsum + wave * 64 : nullptr);
    if (a.dv_colsum) {
      __syncthreads();
      if (tid < 64)
        a.colsum_scratch[dv_scratch_off + ((long)(b * nkb + kblk) * a.H + h) * 64 + tid] =
            (wsum[tid] + wsum[64 + tid]) + (wsum[128 + tid] + wsum[192 + tid]);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------
// Ping-pong dK/dV kernel for the unmasked case: 8 waves x 32 keys, Q / dO tiles (64 queries) + their lse / delta rows stream
// through the ring.  The key operands are held as K' = -K/8 and V' = -V (exact in bf16) and the first-stage accumulators START at
// lse[q] / delta[q] (read from LDS straight into the accumulator registers by the LOAD segment), so that
//   S_acc = lse - scale * S      -> P = exp2(-log2e * S_acc)          (one multiply + one exponential per score)
//   dP_acc = delta - dP          -> -dS = P * dP_acc                  (one multiply; the sign rides in dK's store scale)
// with no per-row statistics in registers.
constexpr int KSTAT = 2048;            // LDS: [4 stages x (lse[64] | delta[64])] then the 4 tile stages
constexpr int KLDS = KSTAT + PNS * PSTG;

__device__ __forceinline__ void glds4_asm(const u32x4_t rs, unsigned lds_addr, unsigned voff) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dword %1, %2, 0 offen lds" ::"s"(lds_addr), "v"(voff), "s"(rs) : "memory");
}

// ROWS: the query side (q, d_o) lives in chunked token rows and is limited to q_span (kernels.h)
template <bool ROWS>
__global__ __launch_bounds__(512, 1) void attn_bwd_dkdv_pp_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), hh = lane >> 5;
  const int grp = wave >> 2;
  const unsigned smem_a = (unsigned)(size_t)smem;
  const int nkb = (a.Tk + 255) >> 8;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = bid / nkb;
  const int b = bh / a.H, h = bh - b * a.H;
  const int k0 = (bid - bh * nkb) * 256;
  const int mykey = k0 + wave * 32 + (lane & 31);
  const int mykey_c = mykey < a.Tk ? mykey : a.Tk - 1;

  const bf16_t* kp = a.k + (long)b * a.bsk + (long)mykey_c * a.ldk + h * 64;
  const bf16_t* vp = a.v + (long)b * a.bsv + (long)mykey_c * a.ldv + h * 64;
  bf16x8_t kf[4], vf[4];
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) {
    const u32x4_t k4 = *(const u32x4_t*)(kp + ds * 16 + hh * 8);
    const u32x4_t v4 = *(const u32x4_t*)(vp + ds * 16 + hh * 8);
    u32x4_t kn, vn;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      kn[i] = pack_bf2(bf_lo(k4[i]) * -0.125f, bf_hi(k4[i]) * -0.125f);  // exact: a power of two
      vn[i] = v4[i] ^ 0x80008000u;
    }
    kf[ds] = __builtin_bit_cast(bf16x8_t, kn);
    vf[ds] = __builtin_bit_cast(bf16x8_t, vn);
  }
  asm volatile("" ::"v"(kf[3]), "v"(vf[3]));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the loop counts its own DMA pieces

  int ntiles = (a.Tq + 63) >> 6;
  if (a.qtile_flags) ntiles = last_nonzero_qtile(a.qtile_flags + ((long)b * a.H + h) * ntiles, ntiles, lane) + 1;  // d_o is zero past it
  if (ROWS && a.q_span) ntiles = min(ntiles, min(a.q_span[b], a.Tq) >> 6);  // d_o rows past the span are not even written
  const int ngroups = (ntiles + PNS - 1) / PNS;
  const PipeSrc1 qsrc = ROWS ? pipe_src1(a.q + h * 64, a.ldq, a.B * a.Tq, wave, lane) : pipe_src1(a.q + (long)b * a.bsq + h * 64, a.ldq, a.Tq, wave, lane);
  const PipeSrc1 dosrc = ROWS ? pipe_src1(a.d_o + h * 64, a.ldo, a.B * a.Tq, wave, lane) : pipe_src1(a.d_o + (long)b * a.bso + h * 64, a.ldo, a.Tq, wave, lane);
  // ROWS: the first token row of every 64-query tile, tiles at or past ntiles mapped far outside the tensors (the DMA then writes
  // zeros, exactly what the plain layout gets from its range check for the tail steps of the last group of four)
  int qrow[8];
  if (ROWS) {
#pragma unroll
    for (int i = 0; i < 8; ++i) qrow[i] = i < ntiles ? __builtin_amdgcn_readfirstlane(a.q_rows[b * OASR_ROWTAB + i]) : 0x3fffffff;
  }
  auto qrow_of = [&](int tile) {  // (scalar select chain: `tile` is wave-uniform, no register indexing)
    int r = 0x3fffffff;
#pragma unroll
    for (int i = 0; i < 8; ++i) r = tile == i ? qrow[i] : r;
    return r;
  };
  // lse / delta rows of a tile: 2 x 256 bytes; even waves bring lse, odd waves delta (four identical copies each: one DMA per
  // wave keeps every wave's vmcnt arithmetic the same)
  u32x4_t srs;
  {
    const unsigned long addr = (unsigned long)(((wave & 1) ? a.delta : a.lse) + ((long)b * a.H + h) * a.Tq);
    srs[0] = (unsigned)addr;
    srs[1] = (unsigned)(addr >> 32) & 0xffffu;
    srs[2] = (unsigned)(a.Tq * 4);
    srs[3] = 0x00020000u;
  }
  auto dma_tile = [&](int tile, int stage) {
    const unsigned dst = smem_a + KSTAT + stage * PSTG + wave * 1024;
    if (ROWS) {
      // a sentinel row times the row pitch wraps in 32 bits: clamp the byte offset to "past the end" instead
      const int r0 = qrow_of(tile);
      const unsigned qo = r0 == 0x3fffffff ? 0x7fffff00u : (unsigned)r0 * (unsigned)(a.ldq * 2);
      const unsigned oo = r0 == 0x3fffffff ? 0x7fffff00u : (unsigned)r0 * (unsigned)(a.ldo * 2);
      glds16_asm(qsrc.rs, dst, r0 == 0x3fffffff ? qo : qsrc.voff + qo);
      glds16_asm(dosrc.rs, dst + TILE, r0 == 0x3fffffff ? oo : dosrc.voff + oo);
      glds4_asm(srs, smem_a + stage * 512 + (wave & 1) * 256, r0 == 0x3fffffff ? 0x7fffff00u : (unsigned)(lane * 4 + tile * 256));
    } else {
      glds16_asm(qsrc.rs, dst, qsrc.voff + (unsigned)tile * qsrc.tile_bytes);
      glds16_asm(dosrc.rs, dst + TILE, dosrc.voff + (unsigned)tile * dosrc.tile_bytes);
      glds4_asm(srs, smem_a + stage * 512 + (wave & 1) * 256, (unsigned)(lane * 4 + tile * 256));
    }
  };

  // (own copy of the fragment addresses and readers, as in attn_bwd_dq_pp_kernel: a shared form changed the instruction streams of both)
  int ar[4], ac[2][2];
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) ar[ds] = KSTAT + tile_addr(lane & 31, ds * 2 + hh);
  {
    const int G = lane >> 4, i = lane & 15;
    const int row = 4 * (G >> 1) + (i >> 2);
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      const int col = dt * 32 + (G & 1) * 16 + (i & 3) * 4;
      ac[dt][0] = KSTAT + tile_addr(row, col >> 3) + (col & 7) * 2;
      ac[dt][1] = KSTAT + tile_addr(row + 8, col >> 3) + (col & 7) * 2;
    }
  }
  auto rd_rows = [&](int off, int ds) { return *(const bf16x8_t*)(smem + ar[ds] + off); };
  auto rd_tr = [&](int off, int dt, int half) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(smem + ac[dt][half] + off));
  };
  const int astat = hh * 16;  // byte offset of this lane's first row group in a 32-query statistics row

  bf16x8_t Aq[4], Ado[4];
  s16x4_t cq[2][2][2], cdo[2][2][2];  // [u][dt][half]
  f32x16_t dkT[2], dvT[2], S[2], dP[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      dkT[i][r] = 0.f;
      dvT[i][r] = 0.f;
    }

  // LOAD(j), j = 2t + kt, stage st = t & 3: Q / dO fragments + accumulator seeds of step j+1, transposed fragments of step j.
  // (The second stage runs in the SAME segment as its softmax here -- one pipeline stage less than the dQ kernel: a third stage
  // would keep a second set of bf16 P / dS tiles alive, and 96 accumulator + key registers already leave no room for it.)
  auto load_seg = [&](int t, int st, int kt) {
    if (kt == 0) dma_tile(t + 3, (st + 3) & 3);
    const int a_st = kt ? ((st + 1) & 3) : st;
    const int a_off = a_st * PSTG + (kt ^ 1) * 32 * 128;
    const int c_off = st * PSTG + kt * 32 * 128;
    const int s_off = a_st * 512 + (kt ^ 1) * 128 + astat;
    const int n = kt ^ 1;
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) {
      Aq[ds] = rd_rows(a_off, ds);
      Ado[ds] = rd_rows(a_off + TILE, ds);
    }
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const f32x4_t l4 = *(const f32x4_t*)(smem + s_off + g4 * 32);
      const f32x4_t d4 = *(const f32x4_t*)(smem + s_off + 256 + g4 * 32);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        S[n][4 * g4 + i] = l4[i];
        dP[n][4 * g4 + i] = d4[i];
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          cq[u][dt][hf] = rd_tr(c_off + u * 16 * 128, dt, hf);
          cdo[u][dt][hf] = rd_tr(c_off + TILE + u * 16 * 128, dt, hf);
        }
    if (kt == 0) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");  // this wave's pieces of tile t+1 have landed
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  };
  // COMPUTE(j): S / dP MFMAs of step j+1 (onto their seeds) with the softmax VALU of step j in their shadow, then the dV / dK
  // MFMAs of step j (the u = 0 half of P / dS is packed first, so its four MFMAs cover the rest of the VALU)
  auto compute_seg = [&](int kt) {
    const int n = kt ^ 1;
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) {
      S[n] = MFMA(Aq[ds], kf[ds], S[n]);
      dP[n] = MFMA(Ado[ds], vf[ds], dP[n]);
    }
    u32x4_t pf[2], dsf[2];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float p0 = __builtin_amdgcn_exp2f(S[kt][2 * j] * -LOG2E);
      const float p1 = __builtin_amdgcn_exp2f(S[kt][2 * j + 1] * -LOG2E);
      pf[j >> 2][j & 3] = pack_bf2(p0, p1);
      dsf[j >> 2][j & 3] = pack_bf2(p0 * dP[kt][2 * j], p1 * dP[kt][2 * j + 1]);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const s16x8_t c1 = __builtin_shufflevector(cdo[u][dt][0], cdo[u][dt][1], 0, 1, 2, 3, 4, 5, 6, 7);
        const s16x8_t c2 = __builtin_shufflevector(cq[u][dt][0], cq[u][dt][1], 0, 1, 2, 3, 4, 5, 6, 7);
        dvT[dt] = MFMA(__builtin_bit_cast(bf16x8_t, c1), __builtin_bit_cast(bf16x8_t, pf[u]), dvT[dt]);
        dkT[dt] = MFMA(__builtin_bit_cast(bf16x8_t, c2), __builtin_bit_cast(bf16x8_t, dsf[u]), dkT[dt]);
      }
    // 64 VALU: 6 beside each of the 8 first-stage MFMAs (all of u = 0 and half of u = 1), the rest beside the u = 0 second-stage MFMAs
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x402, 6, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x402, 4, 0);
    }
    __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
  };

  if (ntiles > 0) {  // (workgroup-uniform)
  // prologue: tiles 0..2 in flight; seeds + S / dP of step 0; LOAD(0)
  dma_tile(0, 0);
  dma_tile(1, 1);
  dma_tile(2, 2);
  asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  ATTN_BARRIER();
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) {
    Aq[ds] = rd_rows(0, ds);
    Ado[ds] = rd_rows(TILE, ds);
  }
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    const f32x4_t l4 = *(const f32x4_t*)(smem + astat + g4 * 32);
    const f32x4_t d4 = *(const f32x4_t*)(smem + astat + 256 + g4 * 32);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      S[0][4 * g4 + i] = l4[i];
      dP[0][4 * g4 + i] = d4[i];
    }
  }
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) {
    S[0] = MFMA(Aq[ds], kf[ds], S[0]);
    dP[0] = MFMA(Ado[ds], vf[ds], dP[0]);
  }
  ATTN_FENCE();
  load_seg(0, 0, 0);
  ATTN_BARRIER();
  if (grp == 1) ATTN_BARRIER();  // the upper half trails by one barrier from here on

  for (int g = 0; g < ngroups; ++g) {
#pragma unroll
    for (int st = 0; st < PNS; ++st) {
      const int t = g * PNS + st;
      compute_seg(0);
      ATTN_BARRIER();
      load_seg(t, st, 1);
      ATTN_BARRIER();
      compute_seg(1);
      ATTN_BARRIER();
      load_seg(t + 1, (st + 1) & 3, 0);
      ATTN_BARRIER();
    }
  }
  if (grp == 0) ATTN_BARRIER();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // tail DMA pieces (zeros) must not land on the staging tiles below
  }
  __syncthreads();
  {
    char* stg = smem + wave * 4096;
    const int rows_valid = a.Tk - (k0 + wave * 32);
    store_rows_bf16(stg, dkT, -SCALE, a.dk + (long)b * a.bsk + (long)(k0 + wave * 32) * a.ldk + h * 64, a.ldk, rows_valid, lane);
    float* wsum = (float*)(smem + 32768);
    store_rows_bf16(stg, dvT, 1.0f, a.dv + (long)b * a.bsv + (long)(k0 + wave * 32) * a.ldv + h * 64, a.ldv, rows_valid, lane,
                    a.dv_colsum ? wsum + wave * 64 : nullptr);
    // (own copy, as in attn_bwd_dq_pp_kernel: a shared helper added an instruction to both)
    if (a.dv_colsum) {  // two partial rows per workgroup, in the 128-key row numbering of the colsum scratch
      __syncthreads();
      if (tid < 128) {
        const int half = tid >> 6, c = tid & 63;
        const int nkb128 = (a.Tk + 127) >> 7;
        const int blk128 = (bid - bh * nkb) * 2 + half;
        const long dv_scratch_off = (long)a.B * ((a.Tq + 127) >> 7) * a.H * 64;
        if (blk128 < nkb128)
          a.colsum_scratch[dv_scratch_off + ((long)(b * nkb128 + blk128) * a.H + h) * 64 + c] =
              (wsum[half * 256 + c] + wsum[half * 256 + 64 + c]) + (wsum[half * 256 + 128 + c] + wsum[half * 256 + 192 + c]);
      }
    }
  }
}

}  // namespace

void attn_launch_bwd_dkdv(const AttnArgs& a, dim3 grid, hipStream_t s) {
  static void (*const kern[2][2])(AttnArgs) = {{attn_bwd_dkdv_kernel<false, false>, attn_bwd_dkdv_kernel<false, true>},  // [causal][chunked rows]
                                               {attn_bwd_dkdv_kernel<true, false>, attn_bwd_dkdv_kernel<true, true>}};
  hipLaunchKernelGGL(kern[a.causal != 0][a.q_rows != nullptr], grid, dim3(256), 0, s, a);
}

int attn_launch_bwd_dkdv_pp(const AttnArgs& a, dim3 grid, hipStream_t s) {
  static void (*const kern[2])(AttnArgs) = {attn_bwd_dkdv_pp_kernel<false>, attn_bwd_dkdv_pp_kernel<true>};  // [chunked rows]
  static LdsAttrOnce attr[2];
  const int rows = a.q_rows != nullptr;
  const int rc = ensure_dynamic_lds(attr[rows], (const void*)kern[rows], KLDS);
  if (rc) return rc;
  hipLaunchKernelGGL(kern[rows], grid, dim3(512), KLDS, s, a);
  return OASR_OK;
}
