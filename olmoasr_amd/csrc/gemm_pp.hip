// oasr_gemm_pp_kernel, the 256 x 256 x 64 "ping-pong" GEMM (the kernel families and what they share: gemm.hip).
//
// 8 waves (2 along M x 4 along N, 128 x 64 outputs each), one workgroup per CU, 128 KiB of LDS = two K-tile buffers of
// four 16 KiB half-tile images (A rows 0-127 / 128-255, B columns 0-127 / 128-255; each image is laid out exactly like
// a 128-row operand tile of oasr_gemm_fast_kernel, so the fragment readers are shared).
//
// The waves of the upper M half run one barrier behind the lower half, so on every SIMD one wave is in its MFMA section
// while the other issues LDS reads and DMA: the matrix pipe never waits for a barrier-drained staging step (the
// 1-workgroup-per-CU failure mode of oasr_gemm_fast_kernel).   The DMA queue is never drained inside the loop: one counted
// wait per K-tile leaves the newest pieces (tile t+2's B) in flight across the barriers.  Every MFMA section is pinned
// between its two barriers by empty asm statements on its accumulators: without them hipcc sinks most of a section's
// MFMAs below the closing s_barrier (the asm-volatile barrier orders memory, not register-only instructions; round 1's
// ISA had 1 + 7 MFMAs around the first barrier pair instead of 8 inside it).
//
// Two schedules of a K-tile exist (VAR, part of the kernel symbol):
//   VAR = 7, two sections of 16 MFMAs (4 barriers per K-tile), four of a wave's eight DMA pieces issued between the MFMAs.
//            Every layout without the fused column sum.  Against the four-phase schedule: +8 % on the NT forward shapes
//            at K = 1024, +16..19 % on the NN dgrads whose B fragments come through ds_read_b64_tr_b16
//            (profiles/r02_gemm_variants_ab.txt, r02_step_gemm_variants_same_box.txt).  NT at K = 4096 is 2 % faster on
//            four phases; not worth a shape-dependent choice between the two.
//   VAR = 2, four phases of 8 MFMAs (8 barriers per K-tile), one 64 x 32 output quadrant each, all DMA pieces issued in
//            the fragment-read sections.  The fused-colsum dgrad (CSUM), for which it won the whole-step A/B:
//     phase  LDS -> VGPR          MFMA        direct-to-LDS staging issued (2 x 1 KiB pieces per wave)
//       0    B0 (4), A0 (8)       A0 x B0     A rows   0-127 of tile t+1 -> other buffer
//       1    B1 (4)               A0 x B1     A rows 128-255 of tile t+1 -> other buffer
//       2    A1 (8)               A1 x B1     B cols   0-127 of tile t+2 -> THIS buffer (its B images are dead)
//       3    -                    A1 x B0     B cols 128-255 of tile t+2 -> THIS buffer;  s_waitcnt vmcnt(4)
//            Every phase is  { ds_reads; staging; s_barrier; MFMAs; s_barrier }.
// Hazards (DMA writes are ordered with LDS reads only by the issuing wave's vmcnt wait followed by a barrier; "phase"
// reads "section" in the two-section schedule, whose staging plan is written above its loop):
//   RAW  tile t+1 is complete after the counted wait of tile t + the barriers up to the first read in phase 0 of t+1
//        (two barrier events later even for the trailing wave group);
//   WAR  an image is re-staged >= 2 phases after its last ds_read, or in the next phase when the reading phase
//        retired its reads (lgkmcnt(0)) before its first barrier (B1 in phase 1 -> B restaged in phase 2).
#include "gemm_common.h"

#define OASR_PP_BARRIER() asm volatile("s_barrier" ::: "memory")

template <bool TA, bool TB, bool SWAP, bool CSUM, int VAR>
__global__ __launch_bounds__(512, 2) void oasr_gemm_pp_kernel(GemmArgs p) {
  static_assert(VAR == 2 || VAR == 7, "ping-pong schedules: 2 = four phases, 7 = two sections");
  constexpr bool TWO_SECTION = VAR == 7;
  constexpr int HALF = 128 * 64 * 2, BUF = 4 * HALF;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int tiles_m = (p.M + 255) / 256, tiles_n = (p.N + 255) / 256;
  const int kt_total = p.K / BK;
  const int per = (kt_total + p.split_k - 1) / p.split_k;
  const long stepA = TA ? (long)BK * p.A.ld : BK, stepB = TB ? (long)BK * p.B.ld : BK;
  // PERSISTENT launches (p.vgrid > gridDim.x, one workgroup per CU): workgroup w walks the virtual blocks w, w + gridDim.x, ...
  // of the grid a plain launch would have used -- gridDim.x is a multiple of 8, so the XCD a virtual block lands on, and with it
  // the rasterisation below, is exactly that of the plain launch.
  const int vgrid = p.vgrid > 0 ? p.vgrid : (int)gridDim.x;
  int m0, n0, nt;
  unsigned off[4][2];  // staging offsets: image i (0,1 = A halves; 2,3 = B halves), 2 pieces per wave
  const bf16_t *baseA, *baseB;
#define OASR_PP_TILE(V)                                                                                      \
  do {                                                                                                       \
    int tm_, tn_, ksplit_;                                                                                   \
    const int ntile_ = tiles_m * tiles_n;                                                                    \
    if (!SWAP && (p.split_k & 7) == 0 && gridDim.y == 1) { /* split-K range tied to the XCD (gemm_fast.hip) */        \
      const int xcd_ = (V) & 7, j_ = (V) >> 3;                                                               \
      const int s8_ = p.split_k >> 3;                                                                        \
      const int t_ = j_ % ntile_;                                                                            \
      ksplit_ = xcd_ * s8_ + j_ / ntile_;                                                                    \
      tm_ = t_ / tiles_n;                                                                                    \
      tn_ = t_ - tm_ * tiles_n;                                                                              \
    } else {                                                                                                 \
      const int bid_ = xcd_remap((V), vgrid);                                                                \
      /* groups of 8 tile rows, walked rows-first: the 32 tiles an XCD runs at once are 8 row panels x 4 column panels */ \
      /* (12 operand panels through its L2 instead of 2 x 16 = 18: -6 % on the N = 4096 layers, scripts/gemm_ab.py) */ \
      int gm_ = p.raster_gm > 0 ? p.raster_gm : 8;                                                           \
      gm_ = gm_ < 1 ? 1 : (gm_ > 16 ? 16 : gm_);                                                             \
      const int per_group_ = gm_ * tiles_n;                                                                  \
      const int group_ = bid_ / per_group_, in_group_ = bid_ - group_ * per_group_;                          \
      const int first_m_ = group_ * gm_;                                                                     \
      const int gsz_ = min(gm_, tiles_m - first_m_);                                                         \
      tm_ = first_m_ + in_group_ % gsz_;                                                                     \
      tn_ = in_group_ / gsz_;                                                                                \
      ksplit_ = blockIdx.y;                                                                                  \
    }                                                                                                        \
    m0 = tm_ * 256;                                                                                          \
    n0 = tn_ * 256;                                                                                          \
    const int kt0_ = ksplit_ * per;                                                                          \
    nt = min(kt_total, kt0_ + per) - kt0_; /* K-tiles of this output tile */                                 \
    fast_offsets<TA, 128, 2, 8>(p.A, p.M, m0, lane, wave, off[0], m0);                                       \
    fast_offsets<TA, 128, 2, 8>(p.A, p.M, m0 + 128, lane, wave, off[1], m0);                                 \
    fast_offsets<TB, 128, 2, 8>(p.B, p.N, n0, lane, wave, off[2], n0);                                       \
    fast_offsets<TB, 128, 2, 8>(p.B, p.N, n0 + 128, lane, wave, off[3], n0);                                 \
    baseA = (TA ? p.A.ptr + m0 : p.A.ptr + (long)m0 * p.A.ld) + (long)kt0_ * stepA;                         \
    baseB = (TB ? p.B.ptr + n0 : p.B.ptr + (long)n0 * p.B.ld) + (long)kt0_ * stepB;                         \
  } while (0)
  int v = blockIdx.x;
  OASR_PP_TILE(v);
  if (nt <= 0) return;  // (uneven split-K; the host never launches those persistent)
  // Phase stagger of the first wave of workgroups (one per CU): with equal-length tiles every CU reaches its epilogue at
  // the same moment and the 256 x 128 KiB of output must drain to HBM in one burst while the matrix cores idle; delaying
  // the CUs of each XCD by k/phases of a tile period spreads the stores under the other CUs' main loops.
  if (p.stagger > 0 && p.stagger_phases > 1 && blockIdx.x < 256 && blockIdx.y == 0) {
    const int ph = (blockIdx.x >> 3) % p.stagger_phases;
    for (int i = 0; i < ph * p.stagger; ++i) __builtin_amdgcn_s_sleep(127);
  }

#define OASR_PP_STAGE(IMG, T, BUFP)                                                                          \
  do {                                                                                                       \
    const __amdgpu_buffer_rsrc_t rs_ = make_rsrc((IMG) < 2 ? baseA + (T) * stepA : baseB + (T) * stepB);     \
    char* d_ = (BUFP) + (IMG) * HALF + wave * 1024;                                                          \
    glds16(rs_, d_, off[IMG][0]);                                                                            \
    glds16(rs_, d_ + 8192, off[IMG][1]);                                                                     \
  } while (0)

  // prologue of an output tile: all of K-tile 0 into buffer P0, the B images of K-tile 1 into the other buffer
#define OASR_PP_PROLOGUE(P0, P1)      \
  do {                                \
    OASR_PP_STAGE(0, 0, P0);          \
    OASR_PP_STAGE(1, 0, P0);          \
    OASR_PP_STAGE(2, 0, P0);          \
    OASR_PP_STAGE(3, 0, P0);          \
    if (nt > 1) {                     \
      OASR_PP_STAGE(2, 1, P1);        \
      OASR_PP_STAGE(3, 1, P1);        \
    }                                 \
  } while (0)
  f32x16_t acc[4][2];
  int parity = 0;     // buffer that holds K-tile 0 of the current output tile
  bool first = true;  // first output tile of this workgroup (its prologue was not issued from an epilogue)
  OASR_PP_PROLOGUE(smem, smem + BUF);
for (;;) {  // output tiles of this workgroup (one iteration unless the launch is persistent)
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  if (first && nt > 1) {
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  } else {  // later tiles: the prologue pieces are older than the previous epilogue's stores, so the count is drained
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  }
  OASR_PP_BARRIER();
  if (wm == 1) OASR_PP_BARRIER();  // the upper half trails by one barrier from here on

  const int aoff = wm * HALF, boff = (2 + (wn >> 1)) * HALF, bsub = (wn & 1) * 64;
  bf16x8_t fa[2][4], fb0[4], fb1[4];
#define OASR_PP_MFMA1(MT0, NT, FB, KS, T)                                                                     \
  do {                                                                                                       \
    if (SWAP)                                                                                                \
      acc[MT0 + T][NT] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(FB[KS], fa[T][KS], acc[MT0 + T][NT], 0, 0, 0); \
    else                                                                                                     \
      acc[MT0 + T][NT] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[T][KS], FB[KS], acc[MT0 + T][NT], 0, 0, 0); \
  } while (0)
  // one phase of the four-phase schedule: 8 MFMAs at priority 1, pinned between the barriers around them
#define OASR_PP_MMA(MT0, NT, FB)                                                                             \
  do {                                                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                                       \
    __builtin_amdgcn_s_setprio(1);                                                                           \
    asm volatile("" : "+v"(acc[MT0][NT]), "+v"(acc[MT0 + 1][NT]));                                           \
    OASR_PP_MFMA1(MT0, NT, FB, 0, 0);                                                                        \
    OASR_PP_MFMA1(MT0, NT, FB, 0, 1);                                                                        \
    OASR_PP_MFMA1(MT0, NT, FB, 1, 0);                                                                        \
    OASR_PP_MFMA1(MT0, NT, FB, 1, 1);                                                                        \
    OASR_PP_MFMA1(MT0, NT, FB, 2, 0);                                                                        \
    OASR_PP_MFMA1(MT0, NT, FB, 2, 1);                                                                        \
    OASR_PP_MFMA1(MT0, NT, FB, 3, 0);                                                                        \
    OASR_PP_MFMA1(MT0, NT, FB, 3, 1);                                                                        \
    asm volatile("" : "+v"(acc[MT0][NT]), "+v"(acc[MT0 + 1][NT]));                                           \
    __builtin_amdgcn_s_setprio(0);                                                                           \
    __builtin_amdgcn_sched_barrier(0);                                                                       \
  } while (0)

  if (TWO_SECTION) {
    // Two sections of 16 MFMAs per K-tile (4 barriers instead of 8): S0 = rows 0-63 of this wave's 128 x 64 block against
    // both column halves, S1 = rows 64-127.  Staging (hazards as in the header, with "phase" = section):
    //   S0 read : A image 0 of tile t+1 -> oth (its last reader, the leading group, is past its own S1 MFMAs);
    //             lgkmcnt(0) BEFORE the barrier, so the B images of `cur` are dead once both groups passed it
    //   S0 MFMA : A image 1 of tile t+1 -> oth, between the MFMAs (the trailing group finished reading it one barrier ago)
    //   S1 read : B image 0 of tile t+2 -> cur; vmcnt(2): everything of tile t+1 has landed, only those 2 pieces are in flight
    //   S1 MFMA : B image 1 of tile t+2 -> cur, between the MFMAs
    // A piece issued between bare MFMAs costs ~60 cycles of issue, which the section's matrix-pipe time covers, against
    // 100-185 cycles in a read section already carrying 8-12 ds_read_b128 (MI355X_MICROARCH.md, "LDS-DMA piece issue cost")
    // -- there it made the read section longer than the partner's MFMAs.
    for (int t = 0; t < nt; ++t) {
      char* cur = smem + ((t & 1) ^ parity) * BUF;
      char* oth = smem + ((t & 1) ^ parity ^ 1) * BUF;
      const bool next1 = t + 1 < nt, next2 = t + 2 < nt;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        fb0[ks] = fast_frag<TB, 256>(cur + boff, bsub, ks, lane);
        fb1[ks] = fast_frag<TB, 256>(cur + boff, bsub + 32, ks, lane);
      }
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int i = 0; i < 2; ++i) fa[i][ks] = fast_frag<TA, 256>(cur + aoff, i * 32, ks, lane);
      if (next1) OASR_PP_STAGE(0, t + 1, oth);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      OASR_PP_BARRIER();
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
      asm volatile("" : "+v"(acc[0][0]), "+v"(acc[1][0]), "+v"(acc[0][1]), "+v"(acc[1][1]));
      OASR_PP_MFMA1(0, 0, fb0, 0, 0);
      OASR_PP_MFMA1(0, 0, fb0, 0, 1);
      OASR_PP_MFMA1(0, 1, fb1, 0, 0);
      OASR_PP_MFMA1(0, 1, fb1, 0, 1);
      if (next1) {
        __builtin_amdgcn_sched_barrier(0);
        const __amdgpu_buffer_rsrc_t rs_ = make_rsrc(baseA + (t + 1) * stepA);
        glds16(rs_, oth + 1 * HALF + wave * 1024, off[1][0]);
        __builtin_amdgcn_sched_barrier(0);
      }
      OASR_PP_MFMA1(0, 0, fb0, 1, 0);
      OASR_PP_MFMA1(0, 0, fb0, 1, 1);
      OASR_PP_MFMA1(0, 1, fb1, 1, 0);
      OASR_PP_MFMA1(0, 1, fb1, 1, 1);
      if (next1) {
        __builtin_amdgcn_sched_barrier(0);
        const __amdgpu_buffer_rsrc_t rs_ = make_rsrc(baseA + (t + 1) * stepA);
        glds16(rs_, oth + 1 * HALF + wave * 1024 + 8192, off[1][1]);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int ks = 2; ks < 4; ++ks) {
        OASR_PP_MFMA1(0, 0, fb0, ks, 0);
        OASR_PP_MFMA1(0, 0, fb0, ks, 1);
        OASR_PP_MFMA1(0, 1, fb1, ks, 0);
        OASR_PP_MFMA1(0, 1, fb1, ks, 1);
      }
      asm volatile("" : "+v"(acc[0][0]), "+v"(acc[1][0]), "+v"(acc[0][1]), "+v"(acc[1][1]));
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
      OASR_PP_BARRIER();
      // ---- S1
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int i = 0; i < 2; ++i) fa[i][ks] = fast_frag<TA, 256>(cur + aoff, 64 + i * 32, ks, lane);
      if (next2) {
        OASR_PP_STAGE(2, t + 2, cur);
        asm volatile("s_waitcnt vmcnt(2)" ::: "memory");  // B image 1 goes out between this section's MFMAs: only these 2 pieces are newer
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      OASR_PP_BARRIER();
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
      asm volatile("" : "+v"(acc[2][0]), "+v"(acc[3][0]), "+v"(acc[2][1]), "+v"(acc[3][1]));
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        OASR_PP_MFMA1(2, 0, fb0, ks, 0);
        OASR_PP_MFMA1(2, 0, fb0, ks, 1);
        OASR_PP_MFMA1(2, 1, fb1, ks, 0);
        OASR_PP_MFMA1(2, 1, fb1, ks, 1);
        if (next2 && ks < 2) {
          __builtin_amdgcn_sched_barrier(0);
          const __amdgpu_buffer_rsrc_t rs_ = make_rsrc(baseB + (t + 2) * stepB);
          glds16(rs_, cur + 3 * HALF + wave * 1024 + ks * 8192, off[3][ks]);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      asm volatile("" : "+v"(acc[2][0]), "+v"(acc[3][0]), "+v"(acc[2][1]), "+v"(acc[3][1]));
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
      OASR_PP_BARRIER();
    }
  } else
  for (int t = 0; t < nt; ++t) {
    char* cur = smem + ((t & 1) ^ parity) * BUF;
    char* oth = smem + ((t & 1) ^ parity ^ 1) * BUF;
    const bool next1 = t + 1 < nt, next2 = t + 2 < nt;
    // ---- phase 0
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) fb0[ks] = fast_frag<TB, 256>(cur + boff, bsub, ks, lane);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i][ks] = fast_frag<TA, 256>(cur + aoff, i * 32, ks, lane);
    if (next1) OASR_PP_STAGE(0, t + 1, oth);
    OASR_PP_BARRIER();
    OASR_PP_MMA(0, 0, fb0);
    OASR_PP_BARRIER();
    // ---- phase 1
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) fb1[ks] = fast_frag<TB, 256>(cur + boff, bsub + 32, ks, lane);
    if (next1) OASR_PP_STAGE(1, t + 1, oth);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // B images of `cur` are dead before this phase's barrier
    OASR_PP_BARRIER();
    OASR_PP_MMA(0, 1, fb1);
    OASR_PP_BARRIER();
    // ---- phase 2
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i][ks] = fast_frag<TA, 256>(cur + aoff, 64 + i * 32, ks, lane);
    if (next2) OASR_PP_STAGE(2, t + 2, cur);
    OASR_PP_BARRIER();
    OASR_PP_MMA(2, 1, fb1);
    OASR_PP_BARRIER();
    // ---- phase 3: everything of tile t+1 (this wave's pieces) must have landed before the barrier that ends the tile
    if (next2) {
      OASR_PP_STAGE(3, t + 2, cur);
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");  // everything but tile t+2's B has landed (this wave's pieces)
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    OASR_PP_BARRIER();
    OASR_PP_MMA(2, 0, fb0);
    OASR_PP_BARRIER();
  }
  if (wm == 0) OASR_PP_BARRIER();  // re-join: the trailing half has finished its LDS reads after this
  // Persistent launch: the NEXT output tile's prologue is issued before this tile's epilogue, into the buffer the epilogue does
  // not stage through (K-tile 0 -> buffer parity ^ 1, K-tile 1's B images -> the upper half of buffer `parity`; the epilogue's
  // wave-private staging tiles live in the lower half of buffer `parity`, the bias rows behind both buffers).  The operand fetch
  // latency, the workgroup relaunch and the drain of this tile's stores then overlap instead of adding up per tile.
  const int em0 = m0, en0 = n0;
  char* const stg = smem + parity * BUF + wave * 4096;
  const int vn = v + (int)gridDim.x;
  const bool has_next = vn < vgrid;
  if (has_next) {
    OASR_PP_TILE(vn);
    parity ^= 1;
    OASR_PP_PROLOGUE(smem + parity * BUF, smem + (parity ^ 1) * BUF);
  }
  fast_epilogue<SWAP, CSUM>(p, acc, stg, (float*)(smem + 2 * BUF + wave * 256), em0, en0, wm, wn, lane);
  if (!has_next) break;
  v = vn;
  asm volatile("" : "+s"(v));  // re-derive the tile's offsets here instead of keeping 8 VGPRs live across the epilogue
  OASR_PP_TILE(v);
  first = false;
}
#undef OASR_PP_STAGE
#undef OASR_PP_PROLOGUE
#undef OASR_PP_TILE
#undef OASR_PP_MMA
#undef OASR_PP_MFMA1
}

#undef OASR_PP_BARRIER

namespace {

template <bool TA, bool TB, bool SWAP, bool CSUM, int VAR>
GemmKernel* pp_kernel() {
  static GemmKernel k{(const void*)oasr_gemm_pp_kernel<TA, TB, SWAP, CSUM, VAR>, std::string("oasr_gemm_pp_kernel<") + gemm_tf(TA) + ", " + gemm_tf(TB) + ", " +
                                                                                     gemm_tf(SWAP) + ", " + gemm_tf(CSUM) + ", " + std::to_string(VAR) + ">"};
  return &k;
}
template <bool TA, bool TB, bool SWAP, bool CSUM>
GemmKernel* pp_schedule_of(int var) {
  return var == 2 ? pp_kernel<TA, TB, SWAP, CSUM, 2>() : var == 7 ? pp_kernel<TA, TB, SWAP, CSUM, 7>() : nullptr;
}
// The instantiations that exist: both operand orders x both schedules per layout, and the fused column sums for the NN dgrad.
template <bool TA, bool TB>
GemmKernel* pp_kernel_of(const GemmRoute& r) {
  if (r.csum) {
    if constexpr (!TA && TB) {
      if (r.swap) return pp_schedule_of<false, true, true, true>(r.pp_var);
    }
    return nullptr;
  }
  return r.swap ? pp_schedule_of<TA, TB, true, false>(r.pp_var) : pp_schedule_of<TA, TB, false, false>(r.pp_var);
}

}  // namespace

GemmKernel* gemm_pp_kernel_of(bool ta, bool tb, const GemmRoute& r) {
  if (!ta && !tb) return pp_kernel_of<false, false>(r);
  if (!ta && tb) return pp_kernel_of<false, true>(r);
  if (ta && !tb) return pp_kernel_of<true, false>(r);
  return pp_kernel_of<true, true>(r);
}

int gemm_launch_pp(const GemmArgs& a, const GemmRoute& r, int want_persistent, hipStream_t stream) {
  GemmKernel* k = gemm_pp_kernel_of(a.ta, a.tb, r);
  OASR_REQUIRE(k, "gemm: no ping-pong kernel with schedule %d, swap %d, column sums %d for layout ta %d tb %d", r.pp_var, (int)r.swap, (int)r.csum, a.ta,
               a.tb);
  const int lds = 2 * 4 * 128 * 64 * 2 + 8 * 256;  // two K-tile buffers + the epilogue's per-wave bias rows
  const int tiles = cdiv(a.M, 256) * cdiv(a.N, 256);
  dim3 grid(tiles, a.split_k);
  if (!r.swap && (a.split_k & 7) == 0) grid = dim3(tiles * a.split_k, 1);
  // Persistent launch (one workgroup per CU walking the same virtual grid, next tile's prologue issued ahead of the epilogue):
  // opt-in (OASR_PP_PERSISTENT=1 or oasr_gemm_set_variant() bits 4-5).  Measured level with plain launches on every layer shape
  // (profiles/r02_gemm_tile_cost_model.txt): the chip is at its power budget in these kernels (effective clock 1.53 GHz of 2.4,
  // profiles/r02_gemm_effective_clock.txt), so cycles saved between tiles come back as a lower clock, and plain launches keep the
  // hardware's dynamic tile dispatch (robust when RCCL kernels hold CUs).  Launching only the GELU-epilogue shapes persistent was
  // level too (profiles/r05_gelu_gemm_persistent_ab.txt).
  static const int n_cu = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 256;
    n &= ~7;  // (the virtual-block -> XCD correspondence needs a multiple of 8)
    return n >= 8 ? n : 8;
  }();
  static const int env_persist = [] {
    const char* e = oasr_experiment_env("OASR_PP_PERSISTENT");
    return e ? atoi(e) : -1;
  }();
  GemmArgs pa = a;
  pa.vgrid = (int)grid.x;
  const int want = want_persistent >= 0 ? want_persistent : env_persist;
  const bool persistent = want == 1 && grid.y == 1 && (int)grid.x > n_cu && ((a.K / BK) % a.split_k) == 0;
  if (persistent) grid = dim3(n_cu, 1);
  return gemm_timed_launch(*k, GemmLaunch{grid, dim3(512), lds, gemm_flops(a), persistent}, pa, stream);
}
