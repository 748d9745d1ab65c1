// Flash attention backward, dQ side (attention.hip has the overview): the general kernel and the ping-pong kernel of the unmasked case.
// Both also produce delta = rowsum(dO * O) and the "which 64-query tiles of d_o are non-zero" flags for the dK/dV kernels.
#include "attention_common.h"

namespace {

// ------------------------------------------------------------------------------------------------------------
// dQ[q][:] = scale * sum_k dS[q][k] K[k][:],  dS = P o (dP - delta),  P = exp(scale*S - lse),  dP = dO V^T
template <bool CAUSAL, bool ROWS>
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_kernel(AttnArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> 5;
  // 1-D grid, XCD-aware: all query blocks of one (batch, head) run on the same XCD so K/V are filled into that XCD's
  // L2 once and re-used by the other query blocks (round-robin dispatch would fetch them through all 8 L2s).
  const int nqb = (a.Tq + 127) >> 7;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const BlockId id = block_id<ROWS>(a.qblk128, bid, nqb, a.H);
  const int b = id.b, h = id.h, qblk = id.blk;
  const int q0 = qblk * 128;
  const int myq = q0 + wave * 32 + (lane & 31);
  const bool krows = ROWS && a.k_rows != nullptr;  // (block-uniform)
  // span-limited backward: query positions >= q_span[b] hold no gradient -- their d_o / o rows are not read, dq is not written
  const int q_lim = (ROWS && a.q_span) ? min(a.q_span[b], a.Tq) : a.Tq;
  if (ROWS && q0 >= q_lim) {  // (block-uniform) nothing to do, but the partial bias-gradient row of this block must read as zeros
    if (a.dq_colsum && tid < 64) a.colsum_scratch[((long)(b * nqb + qblk) * a.H + h) * 64 + tid] = 0.f;
    return;
  }
  const bool w_act = !ROWS || q0 + wave * 32 < q_lim;        // (wave-uniform; spans are multiples of 64)
  const int myq_c = !w_act ? q0 + (lane & 31) : (myq < a.Tq ? myq : a.Tq - 1);  // an inactive wave re-reads rows of the block's first chunk

  bf16x8_t qf[4], dof[4];
  float delta, lse2;
  dq_row_setup<ROWS>(a, b, h, myq, myq_c, w_act, hh, qf, dof, delta, lse2);

  const int kv_len = clamped_kv_len(a, b);
  int kv_end = kv_len;
  if (CAUSAL) kv_end = kv_end < q0 + 128 ? kv_end : q0 + 128;
  int ntiles = kv_end > 0 ? (kv_end + 63) >> 6 : 1;  // >= 1: a fully masked tile yields l = 0 -> O = 0
  if (a.qtile_flags) {  // which 64-query tiles of d_o hold anything: recorded for the dK/dV kernel; a block of zeros has dQ = 0
    // (own copy, as in attn_bwd_dq_pp_kernel: taking even the per-lane test from a shared helper changed this kernel's instruction stream)
    __shared__ int nzs[4];
    bool nz = false;
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) {
      const u32x4_t d4 = __builtin_bit_cast(u32x4_t, dof[ds]);
      nz = nz || ((d4[0] | d4[1] | d4[2] | d4[3]) & 0x7fff7fffu) != 0u;
    }
    const bool wnz = __any(nz);
    if (lane == 0) nzs[wave] = wnz ? 1 : 0;
    __syncthreads();
    const int t0nz = nzs[0] | nzs[1], t1nz = nzs[2] | nzs[3];
    if (tid == 0) {
      const int ntq = (a.Tq + 63) >> 6, tq = q0 >> 6;
      int32_t* f = a.qtile_flags + ((long)b * a.H + h) * ntq;
      if (tq < ntq) f[tq] = t0nz;
      if (tq + 1 < ntq) f[tq + 1] = t1nz;
    }
    if (!(t0nz | t1nz)) ntiles = 0;
  }
  const TileSrc ksrc = krows ? tile_src(a.k + h * 64, a.ldk, a.B * a.Tk, tid) : tile_src(a.k + (long)b * a.bsk + h * 64, a.ldk, a.Tk, tid);
  const TileSrc vsrc = krows ? tile_src(a.v + h * 64, a.ldv, a.B * a.Tk, tid) : tile_src(a.v + (long)b * a.bsv + h * 64, a.ldv, a.Tk, tid);
  auto krow0 = [&](int t) { return krows ? __builtin_amdgcn_readfirstlane(a.k_rows[b * OASR_ROWTAB + t]) : t * 64; };

  f32x16_t dqT[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) dqT[i][r] = 0.f;

  // Unconditional prologue (ntiles >= 1 by construction): a guarded one leaves "Q/dO fragment loads may be pending" in
  // the compiler's wait-count state at the loop header, and hipcc then re-waits vmcnt(3..0) in front of the first MFMAs
  // of EVERY iteration -- i.e. for the K/V prefetch it has just issued -- serialising the load latency into the loop.
  u32x4_t rk[2], rv[2];
  tile_issue(ksrc, krow0(0), rk);
  tile_issue(vsrc, krow0(0), rv);
  tile_commit(smem, tid, rk);
  tile_commit(smem + TILE, tid, rv);
  __syncthreads();
  for (int t = 0; t < ntiles; ++t) {
    const char* kb = smem + (t & 1) * 2 * TILE;
    const char* vb = kb + TILE;
    const bool more = t + 1 < ntiles;
    if (more) {
      const int r0 = krow0(t + 1);
      tile_issue(ksrc, r0, rk);
      tile_issue(vsrc, r0, rv);
    }
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      f32x16_t sT, dpT;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sT[r] = 0.f;
        dpT[r] = 0.f;
      }
#pragma unroll
      for (int ds = 0; ds < 4; ++ds) {
        sT = MFMA(frag_rows(kb, kt * 32, ds, lane), qf[ds], sT);
        dpT = MFMA(frag_rows(vb, kt * 32, ds, lane), dof[ds], dpT);
      }
      const bool full = (t * 64 + kt * 32 + 32 <= kv_len) && (!CAUSAL || (t * 64 + kt * 32 + 31 <= q0 + wave * 32));
      if (full) {
        const f32x2_t c2 = {SCALE * LOG2E, SCALE * LOG2E}, nl2 = {-lse2, -lse2}, nd2 = {-delta, -delta};
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          const f32x2_t s2 = {sT[r], sT[r + 1]}, dp2 = {dpT[r], dpT[r + 1]};
          const f32x2_t ds2 = pk_exp2(pk_fma(s2, c2, nl2)) * (dp2 + nd2);
          sT[r] = ds2[0];
          sT[r + 1] = ds2[1];
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = t * 64 + kt * 32 + acc_row(r, hh);
          const bool ok = (key < kv_len) && (!CAUSAL || key <= myq);
          const float p = ok ? __builtin_amdgcn_exp2f(fmaf(sT[r], SCALE * LOG2E, -lse2)) : 0.f;
          sT[r] = p * (dpT[r] - delta);
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const bf16x8_t dsf = pack_half(sT, u);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) dqT[dt] = MFMA(frag_cols(kb, kt * 32 + 16 * u, dt * 32, lane), dsf, dqT[dt]);
      }
    }
    if (more) {
      char* nb = smem + ((t + 1) & 1) * 2 * TILE;
      tile_commit(nb, tid, rk);
      tile_commit(nb + TILE, tid, rv);
    }
    __syncthreads();
  }
  // (the loop ended on a barrier: the K/V stages are free for the per-wave staging tiles)
  float* wsum = (float*)(smem + 16384);  // [4 waves][64], behind the staging tiles
  {
    const long drow0 = row_at(0L, ROWS, a.q_rows, b, q0 + wave * 32, a.ldq, a.bsq, h);
    store_rows_bf16(smem + wave * 4096, dqT, SCALE, a.dq + drow0, a.ldq, w_act ? a.Tq - (q0 + wave * 32) : 0, lane,
                    a.dq_colsum ? wsum + wave * 64 : nullptr);
  }
  if (a.dq_colsum) {  // one partial row per workgroup: colsum_scratch[(b, query block)][h*64 + c], reduced by the launcher
    __syncthreads();
    if (tid < 64)
      a.colsum_scratch[((long)(b * nqb + qblk) * a.H + h) * 64 + tid] =
          (wsum[tid] + wsum[64 + tid]) + (wsum[128 + tid] + wsum[192 + tid]);
  }
}

// ------------------------------------------------------------------------------------------------------------
// Ping-pong kernels for the UNMASKED case (no causal mask, no per-sequence key length: encoder self-attention and
// cross-attention, 98 % of the attention time of a training step).
//
// What the measurements on the kernels above say (scripts/attn_kernel_times.py under rocprofv3, in-kernel s_memtime stamps;
// profiles/r03_attention_pingpong.txt):
//  * they issue the way they are written -- fragment reads -> wait -> S/dP MFMAs -> softmax VALU -> second-stage MFMAs -- and with
//    two waves per SIMD the matrix pipe idles through every LDS round trip and VALU block (MFMA-busy 0.33);
//  * interleaving everything in ONE wave's stream (reads of step i+2, MFMAs of step i+1, VALU of step i) does not fix it: an MFMA
//    whose operand comes from a ds_read issued even a full step earlier in the same wave still stalls (S/dP MFMAs alone 151 us,
//    with dependent fragment reads 277 us, with the same reads and nothing depending on them 168 us);
//  * v_pk_mul_f32 / v_pk_add_f32 beside MFMAs cost ~16 cycles each where two scalar ops cost ~0 (the compiler SLP-packs
//    adjacent fp32 multiplies: this file is built with -fno-slp-vectorize).
// So: 8 waves, two per SIMD, alternating roles between workgroup barriers -- one COMPUTEs (12 MFMAs with the softmax VALU in
// their shadow, every operand already in registers, nothing inside the segment depends on anything else inside it) while its
// partner LOADs (fragment reads for its next segment ending in lgkmcnt(0), DMA issue).  Waves 4-7 run one barrier behind
// waves 0-3.  K/V tiles move global -> LDS by DMA (buffer_load ... lds: no staging registers, no commit stores) two tiles ahead
// through a 4-stage ring; rows past the end read as zeros (buffer range check), which also makes the tail steps (the loop runs
// in groups of four tiles) contribute nothing.  No masks, no branches in the loop.
//   LOAD(j)   : operand fragments of step j+1, transposed fragments of step j-1; on even j the DMA of tile j/2+2 and the wait for
//               this wave's pieces of tile j/2+1
//   COMPUTE(j): first-stage MFMAs of step j+1, softmax VALU of step j, second-stage MFMAs of step j-1
// ROWS: the query side lives in chunked token rows and is limited to q_span (kernels.h): the cross-attention of a span-limited step
template <bool ROWS>
__global__ __launch_bounds__(512, 1) void attn_bwd_dq_pp_kernel(AttnArgs a) {
  __shared__ __attribute__((aligned(1024))) char smem[PNS * PSTG];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), hh = lane >> 5;
  const int grp = wave >> 2;
  const unsigned smem_a = (unsigned)(size_t)smem;
  const int nqb = (a.Tq + 255) >> 8;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const BlockId id = block_id<ROWS>(a.qblk256, bid, nqb, a.H);
  const int b = id.b, h = id.h, qblk = id.blk;
  const int q0 = qblk * 256;
  const int myq = q0 + wave * 32 + (lane & 31);
  const int q_lim = (ROWS && a.q_span) ? min(a.q_span[b], a.Tq) : a.Tq;
  if (ROWS && q0 >= q_lim) {  // (block-uniform) no gradient in this block: only its two partial bias-gradient rows must read as zeros
    if (a.dq_colsum && tid < 128) {
      const int nqb128 = (a.Tq + 127) >> 7, blk128 = qblk * 2 + (tid >> 6);
      if (blk128 < nqb128) a.colsum_scratch[((long)(b * nqb128 + blk128) * a.H + h) * 64 + (tid & 63)] = 0.f;
    }
    return;
  }
  const bool w_act = !ROWS || q0 + wave * 32 < q_lim;  // (wave-uniform)
  const int myq_c = !w_act ? q0 + (lane & 31) : (myq < a.Tq ? myq : a.Tq - 1);  // an inactive wave re-reads rows of the first chunk

  bf16x8_t qf[4], dof[4];
  float delta, lse2;
  dq_row_setup<ROWS>(a, b, h, myq, myq_c, w_act, hh, qf, dof, delta, lse2);
  asm volatile("" ::"v"(lse2), "v"(delta), "v"(qf[3]), "v"(dof[3]));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the loop counts its own DMA pieces
  bool blk_nz = true;
  if (a.qtile_flags) {  // which 64-query tiles of d_o hold anything: recorded for the dK/dV kernel; a block of zeros has dQ = 0
    int* nzs = (int*)smem;  // (the ring is not in use yet; a barrier below releases these bytes before the first DMA piece)
    bool nz = false;
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) {
      const u32x4_t d4 = __builtin_bit_cast(u32x4_t, dof[ds]);
      nz = nz || ((d4[0] | d4[1] | d4[2] | d4[3]) & 0x7fff7fffu) != 0u;
    }
    const bool wnz = __any(nz);
    if (lane == 0) nzs[wave] = wnz ? 1 : 0;
    __syncthreads();
    if (tid < 4) {
      const int ntq = (a.Tq + 63) >> 6, tq = (q0 >> 6) + tid;
      if (tq < ntq) a.qtile_flags[((long)b * a.H + h) * ntq + tq] = nzs[2 * tid] | nzs[2 * tid + 1];
    }
    blk_nz = (nzs[0] | nzs[1] | nzs[2] | nzs[3] | nzs[4] | nzs[5] | nzs[6] | nzs[7]) != 0;
    __syncthreads();
  }

  const int ntiles = (a.Tk + 63) >> 6;
  const int ngroups = (ntiles + PNS - 1) / PNS;
  const PipeSrc1 ksrc = pipe_src1(a.k + (long)b * a.bsk + h * 64, a.ldk, a.Tk, wave, lane);
  const PipeSrc1 vsrc = pipe_src1(a.v + (long)b * a.bsv + h * 64, a.ldv, a.Tk, wave, lane);
  auto dma_tile = [&](int tile, int stage) {
    const unsigned dst = smem_a + stage * PSTG + wave * 1024;
    glds16_asm(ksrc.rs, dst, ksrc.voff + (unsigned)tile * ksrc.tile_bytes);
    glds16_asm(vsrc.rs, dst + TILE, vsrc.voff + (unsigned)tile * vsrc.tile_bytes);
  };

  // (own copy of the fragment addresses and readers, as in attn_bwd_dkdv_pp_kernel: a shared form changed the instruction streams of both)
  int ar[4], ac[2][2];
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) ar[ds] = tile_addr(lane & 31, ds * 2 + hh);
  {
    const int G = lane >> 4, i = lane & 15;
    const int row = 4 * (G >> 1) + (i >> 2);
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      const int col = dt * 32 + (G & 1) * 16 + (i & 3) * 4;
      ac[dt][0] = tile_addr(row, col >> 3) + (col & 7) * 2;
      ac[dt][1] = tile_addr(row + 8, col >> 3) + (col & 7) * 2;
    }
  }
  auto rd_rows = [&](int off, int ds) { return *(const bf16x8_t*)(smem + ar[ds] + off); };
  auto rd_tr = [&](int off, int dt, int half) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(smem + ac[dt][half] + off));
  };

  bf16x8_t Ak[4], Av[4];
  s16x4_t kc[2][2][2];  // [u][dt][half]
  f32x16_t dqT[2], S[2], dP[2], ND;
  u32x4_t w[2][2];  // [step parity][u]: bf16 dS^T, the B operand of the dQ MFMAs one segment later
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      dqT[i][r] = 0.f;
      S[i][r] = 0.f;
    }
#pragma unroll
  for (int r = 0; r < 16; ++r) ND[r] = -delta;  // dP accumulators start at -delta (a lane's 16 rows all belong to its query)
  dP[0] = ND;
  dP[1] = ND;
  const float c1 = SCALE * LOG2E, nl1 = -lse2;

  // LOAD(j), j = 2t + kt, stage st = t & 3: K/V fragments of step j+1, transposed-K fragments of step j-1
  auto load_seg = [&](int t, int st, int kt) {
    if (kt == 0) dma_tile(t + 2, (st + 2) & 3);
    const int a_st = kt ? ((st + 1) & 3) : st;                    // step j+1 lives in the next tile when kt == 1
    const int c_st = kt ? st : ((st + 3) & 3);                    // step j-1 lives in the previous tile when kt == 0
    const int a_off = a_st * PSTG + (kt ^ 1) * 32 * 128;
    const int c_off = c_st * PSTG + (kt ^ 1) * 32 * 128;
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) {
      Ak[ds] = rd_rows(a_off, ds);
      Av[ds] = rd_rows(a_off + TILE, ds);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        kc[u][dt][0] = rd_tr(c_off + u * 16 * 128, dt, 0);
        kc[u][dt][1] = rd_tr(c_off + u * 16 * 128, dt, 1);
      }
    if (kt == 0) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");  // this wave's pieces of tile t+1 have landed
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  };
  // COMPUTE(j): S/dP MFMAs of step j+1, softmax VALU of step j, dQ MFMAs of step j-1 -- nothing here depends on anything else here
  auto compute_seg = [&](int kt) {
    const int n = kt ^ 1;
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) {
      if (ds == 0) {
        f32x16_t z;
#pragma unroll
        for (int r = 0; r < 16; ++r) z[r] = 0.f;
        S[n] = MFMA(Ak[0], qf[0], z);
        dP[n] = MFMA(Av[0], dof[0], ND);
      } else {
        S[n] = MFMA(Ak[ds], qf[ds], S[n]);
        dP[n] = MFMA(Av[ds], dof[ds], dP[n]);
      }
      if (ds < 2) {
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const s16x8_t kv8 = __builtin_shufflevector(kc[ds][dt][0], kc[ds][dt][1], 0, 1, 2, 3, 4, 5, 6, 7);
          dqT[dt] = MFMA(__builtin_bit_cast(bf16x8_t, kv8), __builtin_bit_cast(bf16x8_t, w[n][ds]), dqT[dt]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float p0 = __builtin_amdgcn_exp2f(fmaf(S[kt][2 * j], c1, nl1));
      const float p1 = __builtin_amdgcn_exp2f(fmaf(S[kt][2 * j + 1], c1, nl1));
      w[kt][j >> 2][j & 3] = pack_bf2(p0 * dP[kt][2 * j], p1 * dP[kt][2 * j + 1]);
    }
    // schedule request for this barrier-to-barrier region: 12 MFMA slots, the 56 VALU spread over them
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x400, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x400, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x400, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);
    }
  };

  if (blk_nz) {  // (workgroup-uniform)
  // prologue: tiles 0, 1 in flight; S/dP of step 0; LOAD(0) with nothing for the dQ MFMAs of "step -1" to add
  dma_tile(0, 0);
  dma_tile(1, 1);
  asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  ATTN_BARRIER();
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) {
    Ak[ds] = rd_rows(0, ds);
    Av[ds] = rd_rows(TILE, ds);
  }
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) {
    S[0] = MFMA(Ak[ds], qf[ds], S[0]);
    dP[0] = MFMA(Av[ds], dof[ds], dP[0]);
  }
  ATTN_FENCE();
  load_seg(0, 0, 0);  // (its transposed-K reads hit stage 3, which nothing has written: overwritten with zeros below)
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    w[1][u] = u32x4_t{0u, 0u, 0u, 0u};
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      kc[u][dt][0] = s16x4_t{0, 0, 0, 0};
      kc[u][dt][1] = s16x4_t{0, 0, 0, 0};
    }
  }
  ATTN_BARRIER();
  if (grp == 1) ATTN_BARRIER();  // the upper half trails by one barrier from here on

  for (int g = 0; g < ngroups; ++g) {
#pragma unroll
    for (int st = 0; st < PNS; ++st) {
      const int t = g * PNS + st;
      if (w_act) compute_seg(0);  // (a wave whose 32 queries lie past the span has nothing to compute: it keeps its DMA / barrier duties only)
      ATTN_BARRIER();
      load_seg(t, st, 1);
      ATTN_BARRIER();
      if (w_act) compute_seg(1);
      ATTN_BARRIER();
      load_seg(t + 1, (st + 1) & 3, 0);
      ATTN_BARRIER();
    }
  }
  // the dQ MFMAs of the last step (its transposed-K fragments came with the last LOAD)
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      const s16x8_t kv8 = __builtin_shufflevector(kc[u][dt][0], kc[u][dt][1], 0, 1, 2, 3, 4, 5, 6, 7);
      dqT[dt] = MFMA(__builtin_bit_cast(bf16x8_t, kv8), __builtin_bit_cast(bf16x8_t, w[1][u]), dqT[dt]);
    }
  if (grp == 0) ATTN_BARRIER();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // tail DMA pieces (zeros) must not land on the staging tiles below
  }
  __syncthreads();
  float* wsum = (float*)(smem + 32768);  // [8 waves][64], behind the staging tiles
  {
    const long drow0 = row_at(0L, ROWS, a.q_rows, b, q0 + wave * 32, a.ldq, a.bsq, h);
    store_rows_bf16(smem + wave * 4096, dqT, SCALE, a.dq + drow0, a.ldq, w_act ? a.Tq - (q0 + wave * 32) : 0, lane,
                    a.dq_colsum ? wsum + wave * 64 : nullptr);
  }
  // (own copy, as in attn_bwd_dkdv_pp_kernel: a shared helper added an instruction to both)
  if (a.dq_colsum) {  // two partial rows per workgroup, in the 128-query row numbering of the colsum scratch
    __syncthreads();
    if (tid < 128) {
      const int half = tid >> 6, c = tid & 63;
      const int nqb128 = (a.Tq + 127) >> 7;
      const int blk128 = qblk * 2 + half;
      if (blk128 < nqb128)
        a.colsum_scratch[((long)(b * nqb128 + blk128) * a.H + h) * 64 + c] =
            (wsum[half * 256 + c] + wsum[half * 256 + 64 + c]) + (wsum[half * 256 + 128 + c] + wsum[half * 256 + 192 + c]);
    }
  }
}

}  // namespace

void attn_launch_bwd_dq(const AttnArgs& a, dim3 grid, hipStream_t s) {
  static void (*const kern[2][2])(AttnArgs) = {{attn_bwd_dq_kernel<false, false>, attn_bwd_dq_kernel<false, true>},  // [causal][chunked rows]
                                               {attn_bwd_dq_kernel<true, false>, attn_bwd_dq_kernel<true, true>}};
  hipLaunchKernelGGL(kern[a.causal != 0][a.q_rows != nullptr], grid, dim3(256), 0, s, a);
}

void attn_launch_bwd_dq_pp(const AttnArgs& a, dim3 grid, hipStream_t s) {
  static void (*const kern[2])(AttnArgs) = {attn_bwd_dq_pp_kernel<false>, attn_bwd_dq_pp_kernel<true>};  // [chunked rows]
  hipLaunchKernelGGL(kern[a.q_rows != nullptr], grid, dim3(512), 0, s, a);
}
