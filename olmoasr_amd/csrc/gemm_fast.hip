// oasr_gemm_fast_kernel, the direct-to-LDS GEMM with one stage drained per barrier (the kernel families and what they share: gemm.hip).
//
// Fast path (plain operands, K % 64 == 0): operand tiles go L2/HBM -> LDS directly with buffer_load_dwordx4 ... lds
// (no VGPR staging, no ds_write).  The LDS image is lane-linear per wave instruction, so the bank-conflict swizzle is
// applied to the per-lane SOURCE address and undone by the same XOR on the fragment read.  Every wave owns a
// 128x64 sub-tile = 4x2 MFMA 32x32x16 blocks (128 accumulator VGPRs).  Two geometries:
//   * 256x256x64, 8 waves (2x4), two LDS stages (128 KiB): the next K-tile streams in while this one is multiplied;
//     one barrier per K-tile, one workgroup per CU, two waves per SIMD.                       (large problems)
//   * 256x128x64, 4 waves (2x2), one LDS stage (48 KiB): 2-3 workgroups per CU hide each other's load latency.
// M/N tails are handled by clamping source rows (garbage only reaches output rows/cols that are never stored).
// SWAP: MFMA issued as D'[n][m] (lane owns one output row, 4 consecutive columns -> vector stores); !SWAP: D[m][n]
// (lane owns one output column -> a wave's fp32 atomics hit 2 x 128 contiguous bytes): used for split-K wgrad.
#include "gemm_common.h"

// Issue this wave's share of one K-tile: NIA + NIB direct-to-LDS 1 KiB pieces (A image first, B image behind it).
#define OASR_STAGE_TILE(KT, DST)                                                                                          \
  do {                                                                                                                    \
    const __amdgpu_buffer_rsrc_t ra_ = make_rsrc(baseA + (KT) * stepA);                                                   \
    const __amdgpu_buffer_rsrc_t rb_ = make_rsrc(baseB + (KT) * stepB);                                                   \
    char* dst_ = (DST);                                                                                                   \
    _Pragma("unroll") for (int j_ = 0; j_ < NIA; ++j_)                                                                    \
        glds16(ra_, dst_ + (j_ * NW + wave) * 1024, offA[j_]);                                               \
    _Pragma("unroll") for (int j_ = 0; j_ < NIB; ++j_)                                                                    \
        glds16(rb_, dst_ + A_BYTES + (j_ * NW + wave) * 1024, offB[j_]);                                     \
  } while (0)

// (external linkage: hipcc 7.2 drops the host-side handle of this instantiation set when it has internal linkage)
template <bool TA, bool TB, int FBN, int NWN, int NSTAGE, bool SWAP, bool CSUM>
// (3 workgroups per CU only for the split-K / atomic variant: its epilogue needs no registers beyond the accumulators)
__global__ __launch_bounds__(128 * NWN, (NWN == 2 && !SWAP) ? 3 : 2) void oasr_gemm_fast_kernel(GemmArgs p) {
  constexpr int NW = 2 * NWN;                     // waves per workgroup
  constexpr int A_BYTES = FBM * 64 * 2, B_BYTES = FBN * 64 * 2, STAGE = A_BYTES + B_BYTES;
  constexpr int NIA = (A_BYTES / 1024) / NW, NIB = (B_BYTES / 1024) / NW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / NWN, wn = wave % NWN;
  const int tiles_m = (p.M + FBM - 1) / FBM, tiles_n = (p.N + FBN - 1) / FBN;
  // Rasterisation (speed only; any mapping is correct).  Block b runs on XCD b % 8, each XCD has a private 4 MiB L2.
  //  * split-K (SWAP == false, wgrad): the K-range index is tied to the XCD -- XCD x owns splits [x*S/8, (x+1)*S/8) for
  //    every output tile, walking all tiles of one split before the next.  The token slab a split streams is then
  //    fetched from HBM by exactly one L2 and shared by all concurrently running tiles (instead of once per XCD).
  //  * otherwise: XCD-contiguous chunks of the tile list, grouped GM rows of tiles x all column tiles with GM chosen so
  //    one group is resident on the XCD at once: the group's A panels stream through L2 once while every column tile
  //    consumes them, weights (small) are re-read from L2/MALL.
  int tm, tn, ksplit;
  {
    const int ntile = tiles_m * tiles_n;
    if (!SWAP && (p.split_k & 7) == 0 && gridDim.y == 1) {
      const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;  // j-th block dispatched to this XCD
      const int s8 = p.split_k >> 3;
      const int t = j % ntile;
      ksplit = xcd * s8 + j / ntile;
      tm = t / tiles_n;
      tn = t - tm * tiles_n;
    } else {
      const int bid = xcd_remap(blockIdx.x, gridDim.x);
      constexpr int RESIDENT = 32 * (NWN == 2 ? (SWAP ? 2 : 3) : 1);  // workgroups resident per XCD
      int gm = p.raster_gm > 0 ? p.raster_gm : RESIDENT / tiles_n;
      gm = gm < 1 ? 1 : (gm > 16 ? 16 : gm);
      const int per_group = gm * tiles_n;
      const int group = bid / per_group, in_group = bid - group * per_group;
      const int first_m = group * gm;
      const int gsz = min(gm, tiles_m - first_m);
      tm = first_m + in_group % gsz;
      tn = in_group / gsz;
      ksplit = blockIdx.y;
    }
  }
  const int m0 = tm * FBM, n0 = tn * FBN;

  const int kt_total = p.K / BK;
  const int per = (kt_total + p.split_k - 1) / p.split_k;
  const int kt0 = ksplit * per;
  const int kt1 = min(kt_total, kt0 + per);
  if (kt0 >= kt1) return;

  unsigned offA[NIA], offB[NIB];
  fast_offsets<TA, FBM, NIA, NW>(p.A, p.M, m0, lane, wave, offA);
  fast_offsets<TB, FBN, NIB, NW>(p.B, p.N, n0, lane, wave, offB);
  const bf16_t* baseA = TA ? p.A.ptr + m0 : p.A.ptr + (long)m0 * p.A.ld;
  const bf16_t* baseB = TB ? p.B.ptr + n0 : p.B.ptr + (long)n0 * p.B.ld;
  const long stepA = TA ? (long)BK * p.A.ld : BK, stepB = TB ? (long)BK * p.B.ld : BK;

  f32x16_t acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  if (NSTAGE == 2) {
    OASR_STAGE_TILE(kt0, smem);
    __syncthreads();
  }
  for (int kt = kt0; kt < kt1; ++kt) {
    const char* cur;
    if (NSTAGE == 2) {
      cur = smem + ((kt - kt0) & 1) * STAGE;
      if (kt + 1 < kt1)
        OASR_STAGE_TILE(kt + 1, smem + (((kt - kt0) & 1) ^ 1) * STAGE);
    } else {
      cur = smem;
      OASR_STAGE_TILE(kt, smem);
      __syncthreads();  // hipcc drains vmcnt(0) for the LDS-DMA before the barrier
    }
    const char* sA = cur;
    const char* sB = cur + A_BYTES;
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {
      bf16x8_t af[4], bfr[2];
#pragma unroll
      for (int t = 0; t < 4; ++t) af[t] = fast_frag<TA, FBM * 2>(sA, wm * 128 + t * 32, ks, lane);
#pragma unroll
      for (int t = 0; t < 2; ++t) bfr[t] = fast_frag<TB, FBN * 2>(sB, wn * 64 + t * 32, ks, lane);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          if (SWAP)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bfr[nt], af[mt], acc[mt][nt], 0, 0, 0);
          else
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[mt], bfr[nt], acc[mt][nt], 0, 0, 0);
        }
    }
    __syncthreads();  // stage fully consumed (and, with two stages, the prefetched tile has landed)
  }

  fast_epilogue<SWAP, CSUM, true>(p, acc, smem + wave * 8192, (float*)(smem + wave * 8192 + 4096), m0, n0, wm, wn, lane);
}

#undef OASR_STAGE_TILE

namespace {

template <bool TA, bool TB, int FBN, int NWN, int NSTAGE, bool SWAP, bool CSUM = false>
GemmKernel* fast_kernel() {
  static GemmKernel k{(const void*)oasr_gemm_fast_kernel<TA, TB, FBN, NWN, NSTAGE, SWAP, CSUM>,
                      std::string("oasr_gemm_fast_kernel<") + gemm_tf(TA) + ", " + gemm_tf(TB) + ", " + std::to_string(FBN) + ", " + std::to_string(NWN) +
                          ", " + std::to_string(NSTAGE) + ", " + gemm_tf(SWAP) + ", " + gemm_tf(CSUM) + ">"};
  return &k;
}

// The instantiations that exist: both geometries x both operand orders per layout, and the fused column sums for the NN dgrad on 256 x 128 tiles.
template <bool TA, bool TB>
GemmKernel* fast_kernel_of(const GemmRoute& r) {
  const bool big = r.fbn == 256 && r.nwn == 4 && r.nstage == 2;
  if (!big && !(r.fbn == 128 && r.nwn == 2 && r.nstage == 1)) return nullptr;
  if (r.csum) {
    if constexpr (!TA && TB) {
      if (!big && r.swap) return fast_kernel<false, true, 128, 2, 1, true, true>();
    }
    return nullptr;
  }
  if (big) return r.swap ? fast_kernel<TA, TB, 256, 4, 2, true>() : fast_kernel<TA, TB, 256, 4, 2, false>();
  return r.swap ? fast_kernel<TA, TB, 128, 2, 1, true>() : fast_kernel<TA, TB, 128, 2, 1, false>();
}

}  // namespace

GemmKernel* gemm_fast_kernel_of(bool ta, bool tb, const GemmRoute& r) {
  if (!ta && !tb) return fast_kernel_of<false, false>(r);
  if (!ta && tb) return fast_kernel_of<false, true>(r);
  if (ta && !tb) return fast_kernel_of<true, false>(r);
  return fast_kernel_of<true, true>(r);
}

int gemm_launch_fast(const GemmArgs& a, const GemmRoute& r, hipStream_t stream) {
  GemmKernel* k = gemm_fast_kernel_of(a.ta, a.tb, r);
  OASR_REQUIRE(k, "gemm: no direct-to-LDS kernel %d x %d x %d stages, swap %d, column sums %d for layout ta %d tb %d", r.fbn, r.nwn, r.nstage, (int)r.swap,
               (int)r.csum, a.ta, a.tb);
  const int lds = r.nstage * (FBM * 64 * 2 + r.fbn * 64 * 2);
  const int tiles = cdiv(a.M, FBM) * cdiv(a.N, r.fbn);
  dim3 grid(tiles, a.split_k);
  if (!r.swap && (a.split_k & 7) == 0) grid = dim3(tiles * a.split_k, 1);  // split index tied to the XCD (see kernel)
  return gemm_timed_launch(*k, GemmLaunch{grid, dim3(128 * r.nwn), lds, gemm_flops(a), false}, a, stream);
}
