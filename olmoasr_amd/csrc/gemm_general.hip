// The register-staged GEMM kernels (the kernel families and what they share: gemm.hip):
//  * gemm_kernel<TA, TB>     128x128x64 with bounds-checked buffer loads: conv window views, K not a multiple of 64, fp32 /
//    positional-embedding / odd-stride outputs;
//  * gemm_skinny_kernel<MT>  M <= 64 rows (decode steps), weights streamed straight into MFMA operands.
// Both leave through the 8-byte-store epilogue of gemm_common.h (epilogue_store).  (The kernels keep their anonymous namespace.)
#include "gemm_common.h"

namespace {

// Issue the 4 x 16-byte loads this thread contributes to one 128x64 (or 64x128) operand tile.
//   !TRANS: tile rows = output rows [row0, row0+128), cols = reduction [k0, k0+64)
//    TRANS: tile rows = reduction  [k0, k0+64),       cols = output rows [row0, row0+128)
template <bool TRANS>
__device__ __forceinline__ void issue_loads(const OperandView& v, int R, int K, int row0, int k0, int tid,
                                            u32x4_t (&regs)[4]) {
  if (!TRANS) {
    long base_el;
    if (v.rpb) {
      const int b0 = row0 / v.rpb, t0 = row0 - b0 * v.rpb;
      base_el = (long)b0 * v.bstride + (long)t0 * v.ld - v.lead + k0;
    } else {
      base_el = (long)row0 * v.ld + k0;
    }
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(v.ptr + base_el);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int id = tid + 256 * i;
      const int rl = id >> 3, c16 = id & 7;
      const int r = row0 + rl, k = k0 + c16 * 8;
      bool ok = (r < R) && (k < K);
      long off_el;
      if (v.rpb) {
        const int b = r / v.rpb, t = r - b * v.rpb;
        off_el = (long)b * v.bstride + (long)t * v.ld - v.lead + k - base_el;
        ok = ok && (k < v.kvalid) && !(t == 0 && k < v.lead) && !(t == v.rpb - 1 && k >= v.trail_from);
      } else {
        off_el = (long)rl * v.ld + c16 * 8;
      }
      const unsigned voff = ok ? (unsigned)(off_el * 2) : OOB;
      regs[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, 0, 0);
    }
  } else {
    long base_el;
    if (v.rpb) {
      const int b0 = k0 / v.rpb, t0 = k0 - b0 * v.rpb;
      base_el = (long)b0 * v.bstride + (long)t0 * v.ld - v.lead + row0;
    } else {
      base_el = (long)k0 * v.ld + row0;
    }
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(v.ptr + base_el);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int id = tid + 256 * i;
      const int kl = id >> 4, c16 = id & 15;
      const int kk = k0 + kl, col = row0 + c16 * 8;
      bool ok = (kk < K) && (col < R);
      long off_el;
      if (v.rpb) {
        const int b = kk / v.rpb, t = kk - b * v.rpb;
        off_el = (long)b * v.bstride + (long)t * v.ld - v.lead + col - base_el;
        ok = ok && (col < v.kvalid) && !(t == 0 && col < v.lead) && !(t == v.rpb - 1 && col >= v.trail_from);
      } else {
        off_el = (long)kl * v.ld + c16 * 8;
      }
      const unsigned voff = ok ? (unsigned)(off_el * 2) : OOB;
      regs[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, 0, 0);
    }
  }
}

template <bool TRANS>
__device__ __forceinline__ void store_tile(char* lds, int tid, const u32x4_t (&regs)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int id = tid + 256 * i;
    int addr;
    if (!TRANS) {
      const int rl = id >> 3, c16 = id & 7;
      addr = rl * 128 + ((c16 ^ ((rl >> 1) & 7)) << 4);
    } else {
      const int kl = id >> 4, c16 = id & 15;
      addr = kl * 256 + (((((c16 >> 2) ^ (kl & 3)) << 2) | (c16 & 3)) << 4);
    }
    *(u32x4_t*)(lds + addr) = regs[i];
  }
}

// MFMA 32x32x16 operand fragment for rows [sub, sub+32) of the tile, k-step ks (16 wide):
// lane l holds row (l & 31), k = ks*16 + (l >> 5)*8 + 0..7.
template <bool TRANS>
__device__ __forceinline__ bf16x8_t read_frag(const char* lds, int sub, int ks, int lane) {
  if (!TRANS) {
    const int row = sub + (lane & 31);
    const int c16 = ks * 2 + (lane >> 5);
    const int addr = row * 128 + ((c16 ^ ((row >> 1) & 7)) << 4);
    return *(const bf16x8_t*)(lds + addr);
  } else {
    const int G = lane >> 4, i = lane & 15;
    const int krow = ks * 16 + (G >> 1) * 8 + (i >> 2);
    const int col = sub + (G & 1) * 16 + (i & 3) * 4;
    const int c16 = col >> 3;
    const int addr = krow * 256 + (((((c16 >> 2) ^ (krow & 3)) << 2) | (c16 & 3)) << 4) + (col & 7) * 2;
    const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(lds + addr));
    const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(lds + addr + 4 * 256));
    const s16x8_t v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8_t, v);
  }
}

template <bool TA, bool TB>
__global__ __launch_bounds__(256, 2) void gemm_kernel(GemmArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tiles_n = (p.N + BN - 1) / BN;
  const int ntile = gridDim.x;
  const int bid = xcd_remap(blockIdx.x, ntile);
  const int tm = bid / tiles_n, tn = bid - tm * tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;

  const int kt_total = (p.K + BK - 1) / BK;
  const int per = (kt_total + p.split_k - 1) / p.split_k;
  const int kt0 = blockIdx.y * per;
  const int kt1 = min(kt_total, kt0 + per);
  if (kt0 >= kt1) return;

  // stage s: A tile at smem + s*2*TILE_BYTES, B tile right behind it

  f32x16_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  u32x4_t ra[4], rb[4];
  issue_loads<TA>(p.A, p.M, p.K, m0, kt0 * BK, tid, ra);
  issue_loads<TB>(p.B, p.N, p.K, n0, kt0 * BK, tid, rb);
  store_tile<TA>(smem, tid, ra);
  store_tile<TB>(smem + TILE_BYTES, tid, rb);
  __syncthreads();

  for (int kt = kt0; kt < kt1; ++kt) {
    const int cur = (kt - kt0) & 1;
    const bool more = (kt + 1 < kt1);
    const char* cA = smem + cur * 2 * TILE_BYTES;
    const char* cB = cA + TILE_BYTES;
    char* nA = smem + (cur ^ 1) * 2 * TILE_BYTES;
    if (more) {
      issue_loads<TA>(p.A, p.M, p.K, m0, (kt + 1) * BK, tid, ra);
      issue_loads<TB>(p.B, p.N, p.K, n0, (kt + 1) * BK, tid, rb);
    }
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {
      bf16x8_t af[2], bfr[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        af[t] = read_frag<TA>(cA, wm * 64 + t * 32, ks, lane);
        bfr[t] = read_frag<TB>(cB, wn * 64 + t * 32, ks, lane);
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bfr[nt], af[mt], acc[mt][nt], 0, 0, 0);
    }
    if (more) {
      store_tile<TA>(nA, tid, ra);
      store_tile<TB>(nA + TILE_BYTES, tid, rb);
    }
    __syncthreads();
  }

  // ---- epilogue: lane holds, for row m, columns n = nbase + 8q + 4h + (0..3) --------------------------------
  const int h = lane >> 5;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int m = m0 + wm * 64 + mt * 32 + (lane & 31);
    if (m >= p.M) continue;
    const int pos_row = p.pos ? (m % p.pos_period) : 0;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = n0 + wn * 64 + nt * 32 + 8 * q + 4 * h;
        if (n >= p.N) continue;
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = acc[mt][nt][q * 4 + i];
        epilogue_store(p, m, n, pos_row, v);
      }
    }
  }
}

// ---- skinny GEMM for the decode path: out[M <= 64][N] = x[M][K] . W[N][K]^T, NT layout --------------------------------
// A decoder step multiplies a handful of token rows with every weight matrix; the 256-wide tiles above would run 3-24
// workgroups that each walk K serially (measured 25-32 us per GEMM, 40x the time the weight bytes need).  Here one
// workgroup owns 32 output columns, its 4 waves split K four ways and stream the weight rows straight from L2/HBM
// into MFMA operands (16 bytes per lane, no LDS staging: every weight byte is used exactly once), x comes through
// L1/L2.  Partial accumulators meet in LDS; the epilogue is the general kernel's.
template <int MT>
__global__ __launch_bounds__(256) void gemm_skinny_kernel(GemmArgs p) {
  __shared__ float red[4][MT][16][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5;
  const int n0 = blockIdx.x * 32;
  int col = n0 + (lane & 31);
  col = col < p.N ? col : p.N - 1;
  const bf16_t* wp = p.B.ptr + (long)col * p.B.ld + h * 8;
  const bf16_t* xp[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    int row = mt * 32 + (lane & 31);
    row = row < p.M ? row : p.M - 1;
    xp[mt] = p.A.ptr + (long)row * p.A.ld + h * 8;
  }
  f32x16_t acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
  const int kq = p.K / 4;  // K % 64 == 0 (host): every wave gets a multiple of 16
  const int k_begin = wave * kq, k_end = k_begin + kq;
  int k = k_begin;
  for (; k + 64 <= k_end; k += 64) {  // 4 k-steps per trip: 4 (+ 4 MT) independent 16-byte loads in flight per lane
    u32x4_t wq[4], xq[MT][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      wq[j] = *(const u32x4_t*)(wp + k + 16 * j);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) xq[mt][j] = *(const u32x4_t*)(xp[mt] + k + 16 * j);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)  // D'[n][m]: lane owns output row m
        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, wq[j]), __builtin_bit_cast(bf16x8_t, xq[mt][j]),
                                                          acc[mt], 0, 0, 0);
  }
  for (; k < k_end; k += 16) {
    const bf16x8_t wf = __builtin_bit_cast(bf16x8_t, *(const u32x4_t*)(wp + k));
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const bf16x8_t xf = __builtin_bit_cast(bf16x8_t, *(const u32x4_t*)(xp[mt] + k));
      acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, xf, acc[mt], 0, 0, 0);
    }
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave][mt][r][lane] = acc[mt][r];
  __syncthreads();
  // wave w finishes register group q = w: columns n0 + 8w + 4h .. +3 of output row (lane & 31)
  const int n = n0 + 8 * wave + 4 * h;
  if (n < p.N) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int m = mt * 32 + (lane & 31);
      if (m < p.M) {
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          v[i] = red[0][mt][wave * 4 + i][lane] + red[1][mt][wave * 4 + i][lane] + red[2][mt][wave * 4 + i][lane] +
                 red[3][mt][wave * 4 + i][lane];
        epilogue_store(p, m, n, p.pos ? (m % p.pos_period) : 0, v);
      }
    }
  }
}

template <bool TA, bool TB>
GemmKernel* general_kernel() {
  static GemmKernel k{(const void*)gemm_kernel<TA, TB>, std::string("gemm_kernel<") + gemm_tf(TA) + ", " + gemm_tf(TB) + ">"};
  return &k;
}

}  // namespace

GemmKernel* gemm_general_kernel(bool ta, bool tb) {
  if (!ta && !tb) return general_kernel<false, false>();
  if (!ta && tb) return general_kernel<false, true>();
  if (ta && !tb) return general_kernel<true, false>();
  return general_kernel<true, true>();
}

GemmKernel* gemm_skinny_kernel_of(int M) {
  static GemmKernel k1{(const void*)gemm_skinny_kernel<1>, "gemm_skinny_kernel<1>"}, k2{(const void*)gemm_skinny_kernel<2>, "gemm_skinny_kernel<2>"};
  return M <= 32 ? &k1 : &k2;
}

int gemm_launch_general(const GemmArgs& a, hipStream_t stream) {
  const int tiles = cdiv(a.M, BM) * cdiv(a.N, BN);
  // algorithmic flops: conv windows count their real kernel width, not the zero padding
  const double kk = a.A.rpb ? (double)(a.ta ? a.K : a.A.kvalid) : (double)a.K;
  const double nn = (a.B.rpb && a.tb) ? (double)a.B.kvalid : (double)a.N;
  return gemm_timed_launch(*gemm_general_kernel(a.ta, a.tb), GemmLaunch{dim3(tiles, a.split_k), dim3(256), 4 * TILE_BYTES, 2.0 * (double)a.M * nn * kk, false},
                           a, stream);
}

int gemm_launch_skinny(const GemmArgs& a, hipStream_t stream) {
  return gemm_timed_launch(*gemm_skinny_kernel_of(a.M), GemmLaunch{dim3(cdiv(a.N, 32)), dim3(256), 0, gemm_flops(a), false}, a, stream);
}
