// What more than one of the GEMM kernel files shares (gemm.hip describes the kernels): the tile constants, the operand addressing and fragment
// readers of the direct-to-LDS kernels, the fused epilogue in its two forms (8-byte stores: general and skinny kernels; staged 16-byte rows:
// direct-to-LDS kernels), and the interface between gemm.hip -- which checks the arguments, chooses the kernel (gemm_route) and owns the
// profile state -- and the family files gemm_general.hip, gemm_fast.hip, gemm_pp.hip, which own the kernels and their launch geometry.
#pragma once
#include <string>

#include "kernels.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 64;  // the general kernel's tile; BK is every kernel's K-tile
constexpr int TILE_BYTES = 128 * 64 * 2;
constexpr unsigned OOB = 0x80000000u;  // > num_records of every descriptor below -> hardware returns 0

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7fffffff, 0x00020000);
}

typedef __attribute__((address_space(3))) s16x4_t* lds_s16x4_ptr;

// Fused epilogue math for 4 consecutive columns n..n+3 of output row m (see GemmArgs in kernels.h for the order of
// ops): returns the pre-activation and the final value packed to bf16; v[] holds the final fp32 values on return.
__device__ __forceinline__ void epilogue_math(const GemmArgs& p, int m, int n, int pos_row, float (&v)[4], u32x2_t& pre, u32x2_t& fin) {
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] *= p.alpha;
  if (p.bias) {
    const f32x4_t b4 = *(const f32x4_t*)(p.bias + n);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] += b4[i];
  }
  pre[0] = pack_bf2(v[0], v[1]);
  pre[1] = pack_bf2(v[2], v[3]);
  if (p.act == 1) {
    v[0] = gelu_f(bf_lo(pre[0]));
    v[1] = gelu_f(bf_hi(pre[0]));
    v[2] = gelu_f(bf_lo(pre[1]));
    v[3] = gelu_f(bf_hi(pre[1]));
  } else if (p.act == 2) {
    float d[4];
    gelu_and_deriv(bf_lo(pre[0]), v[0], d[0]);
    gelu_and_deriv(bf_hi(pre[0]), v[1], d[1]);
    gelu_and_deriv(bf_lo(pre[1]), v[2], d[2]);
    gelu_and_deriv(bf_hi(pre[1]), v[3], d[3]);
    pre[0] = pack_bf2(d[0], d[1]);
    pre[1] = pack_bf2(d[2], d[3]);
  }
  if (p.pos) {
    const f32x4_t p4 = *(const f32x4_t*)(p.pos + (long)pos_row * p.N + n);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = bf_round(v[i]) + p4[i];
  }
  if (p.dgelu_u) {
    const u32x2_t u = *(const u32x2_t*)(p.dgelu_u + (long)m * p.ldu + n);
    v[0] = bf_round(v[0]) * (p.dgelu_deriv ? bf_lo(u[0]) : dgelu_f(bf_lo(u[0])));
    v[1] = bf_round(v[1]) * (p.dgelu_deriv ? bf_hi(u[0]) : dgelu_f(bf_hi(u[0])));
    v[2] = bf_round(v[2]) * (p.dgelu_deriv ? bf_lo(u[1]) : dgelu_f(bf_lo(u[1])));
    v[3] = bf_round(v[3]) * (p.dgelu_deriv ? bf_hi(u[1]) : dgelu_f(bf_hi(u[1])));
  }
  if (p.resid) {
    const u32x2_t r = *(const u32x2_t*)(p.resid + (long)m * p.ldr + n);
    v[0] = bf_round(v[0]) + bf_lo(r[0]);
    v[1] = bf_round(v[1]) + bf_hi(r[0]);
    v[2] = bf_round(v[2]) + bf_lo(r[1]);
    v[3] = bf_round(v[3]) + bf_hi(r[1]);
  }
  fin[0] = pack_bf2(v[0], v[1]);
  fin[1] = pack_bf2(v[2], v[3]);
}

__device__ __forceinline__ void epilogue_f32(const GemmArgs& p, int m, int n, const float (&v)[4]) {
  float* dst = p.out_f32 + (long)m * p.ldc32 + n;
  if (p.atomic) {
#pragma unroll
    for (int i = 0; i < 4; ++i) unsafeAtomicAdd(dst + i, v[i]);
  } else {
    f32x4_t c4;
    if (p.beta != 0.f) {
      c4 = *(const f32x4_t*)dst;
#pragma unroll
      for (int i = 0; i < 4; ++i) c4[i] = p.beta * c4[i] + v[i];
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) c4[i] = v[i];
    }
    *(f32x4_t*)dst = c4;
  }
}

// direct (8-byte) stores: general kernel
__device__ __forceinline__ void epilogue_store(const GemmArgs& p, int m, int n, int pos_row, float (&v)[4]) {
  u32x2_t pre, fin;
  epilogue_math(p, m, n, pos_row, v, pre, fin);
  if (p.out_pre) *(u32x2_t*)(p.out_pre + (long)m * p.ldc + n) = pre;
  if (p.out) *(u32x2_t*)(p.out + (long)m * p.ldc + n) = fin;
  if (p.out_f32) epilogue_f32(p, m, n, v);
}

// ---- the direct-to-LDS kernels (gemm_fast.hip, gemm_pp.hip): 256-row tiles, operand images of 1 KiB chunks, 128 x 64 outputs per wave --------
constexpr int FBM = 256;

typedef __attribute__((address_space(3))) void* lds_void_ptr;
typedef __attribute__((address_space(3))) u32x2_t* lds_u32x2_ptr;
typedef __attribute__((address_space(3))) u32x4_t* lds_u32x4_ptr;

// Byte offsets (from the tile's base row/column `rel0`, default row0) of this lane's 16-byte pieces of the operand
// image that starts at row/column row0.
template <bool TRANS, int ROWS, int NI, int NW>
__device__ __forceinline__ void fast_offsets(const OperandView& v, int R, int row0, int lane, int wave, unsigned (&off)[NI],
                                             int rel0 = -1) {
  rel0 = rel0 < 0 ? row0 : rel0;
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int q = j * NW + wave;  // 1 KiB chunk index inside the tile image
    if (!TRANS) {
      const int row = q * 8 + (lane >> 3), phys = lane & 7;
      const int c16 = phys ^ ((row >> 1) & 7);
      int gr = row0 + row;
      gr = gr < R ? gr : R - 1;
      off[j] = (unsigned)(((long)(gr - rel0) * v.ld + c16 * 8) * 2);
    } else {
      constexpr int CPR = ROWS / 8;  // 16-byte pieces per k-row
      constexpr int KPC = 64 / CPR;  // k-rows per 1 KiB chunk
      const int krow = q * KPC + lane / CPR, phys = lane % CPR;
      const int c16 = phys ^ ((krow & 3) << 2);
      int col = row0 + c16 * 8;
      col = col + 8 <= R ? col : R - 8;
      off[j] = (unsigned)(((long)krow * v.ld + (col - rel0)) * 2);
    }
  }
}

template <bool TRANS, int RB /*row bytes of a transposed tile*/>
__device__ __forceinline__ bf16x8_t fast_frag(const char* lds, int sub, int ks, int lane) {
  if (!TRANS) {
    const int row = sub + (lane & 31);
    const int c16 = ks * 2 + (lane >> 5);
    return *(const bf16x8_t*)(lds + row * 128 + ((c16 ^ ((row >> 1) & 7)) << 4));
  } else {
    const int G = lane >> 4, i = lane & 15;
    const int krow = ks * 16 + (G >> 1) * 8 + (i >> 2);
    const int col = sub + (G & 1) * 16 + (i & 3) * 4;
    const int addr = krow * RB + ((((col >> 3)) ^ ((krow & 3) << 2)) << 4) + (col & 7) * 2;
    const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(lds + addr));
    const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(lds + addr + 4 * RB));
    const s16x8_t v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8_t, v);
  }
}

// 16 bytes per lane straight into LDS at (wave-uniform) dst + lane*16.  Kept in a non-template __device__ function:
// hipcc 7.2 silently drops the host-side kernel handle when this builtin appears in a template-dependent expression.
__device__ __forceinline__ void glds16(const __amdgpu_buffer_rsrc_t rs, char* dst, unsigned voff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_ptr)dst, 16, voff, 0, 0, 0);
}

// The common bf16-output epilogues (everything but fp32 / positional-embedding / odd-stride outputs), organised so that
// every runtime option is one wave-uniform branch per 32-row block and all global traffic is 16 bytes per lane:
//   pass A  acc * alpha (+ bias) -> bf16 (the autocast rounding point of the Linear) -> wave-private LDS tile
//           ([32 rows][128 B], 16-byte chunks XOR-swizzled by row);
//   pass B  each lane takes 8 consecutive columns of one row back out of LDS and applies what follows the rounding
//           point in GemmArgs order (GELU, x dGELU(u), + residual; u and the residual are read with the same
//           coalesced 16-byte accesses as the stores and are prefetched before pass A), accumulates the fused
//           bias-gradient column sums, and stores out_pre / out.
// Bit-identical to epilogue_math(): every later op starts from the bf16-rounded pre-activation.
__host__ __device__ __forceinline__ bool fast_rows_ok(const GemmArgs& p) {
  const unsigned long al = (unsigned long)p.out | (unsigned long)p.out_pre | (unsigned long)p.resid | (unsigned long)p.dgelu_u;
  return !p.out_f32 && (!p.pos || (!p.resid && !p.dgelu_u)) && (p.N % 8) == 0 && (p.ldc % 8) == 0 && (al & 15) == 0 &&
         (!p.resid || (p.ldr % 8) == 0) && (!p.dgelu_u || (p.ldu % 8) == 0) && !(p.resid && p.dgelu_u);
}

// 16-byte global accesses of the epilogue, optionally non-temporal (streaming: the output / side-input bytes are touched once
// and should not displace the operand panels the main loops re-read from L2)
__device__ __forceinline__ void store16(bf16_t* ptr, const u32x4_t& v, bool nt) {
  if (nt) __builtin_nontemporal_store(v, (u32x4_t*)ptr);
  else *(u32x4_t*)ptr = v;
}
__device__ __forceinline__ u32x4_t load16(const bf16_t* ptr, bool nt) {
  return nt ? __builtin_nontemporal_load((const u32x4_t*)ptr) : *(const u32x4_t*)ptr;
}
// The runtime options of the epilogue, as a bit set.  The body below is written once over these flags; for the combinations the
// training step actually launches (EPI_MODES) it is instantiated with the flags as compile-time constants, so that the ~12 wave-uniform
// branches per 8-column chunk, the per-row bounds predicates and the dead arithmetic disappear from the instruction stream -- the
// epilogue is instruction-bound (profiles/r03_gemm_tile_stamps.txt).  Anything else runs the generic instantiation (MODE < 0).
enum : unsigned {
  EPI_BIAS = 1, EPI_RESID = 2, EPI_U = 4, EPI_UDERIV = 8, EPI_PRE = 16, EPI_OUT = 32, EPI_GELU = 64, EPI_DERIV = 128, EPI_POS = 256,
  EPI_SCALE = 512, EPI_NT_ST = 1024, EPI_NT_LD = 2048, EPI_PARTIAL = 4096
};
__host__ __device__ __forceinline__ unsigned epi_flags_of(const GemmArgs& p, bool partial) {
  return (p.bias ? EPI_BIAS : 0) | (p.resid ? EPI_RESID : 0) | (p.dgelu_u ? EPI_U : 0) | (p.dgelu_deriv ? EPI_UDERIV : 0) |
         (p.out_pre ? EPI_PRE : 0) | (p.out ? EPI_OUT : 0) | (p.act != 0 ? EPI_GELU : 0) | (p.act == 2 ? EPI_DERIV : 0) |
         (p.pos ? EPI_POS : 0) | (p.alpha != 1.0f ? EPI_SCALE : 0) | ((p.epi_flags & 1) ? EPI_NT_ST : 0) |
         ((p.epi_flags & 2) ? EPI_NT_LD : 0) | (partial ? EPI_PARTIAL : 0);
}
constexpr unsigned EPI_MODES[] = {
    EPI_BIAS | EPI_OUT,                                   // Linear with bias (q|k|v, cross q / k|v)
    EPI_BIAS | EPI_OUT | EPI_RESID,                       // attention / MLP output projection + residual
    EPI_BIAS | EPI_OUT | EPI_PRE | EPI_GELU | EPI_DERIV,  // mlp.0 in training: GELU out, GELU' saved
    EPI_BIAS | EPI_OUT | EPI_GELU,                        // mlp.0 in inference
    EPI_OUT,                                              // dgrad
    EPI_OUT | EPI_RESID,                                  // dgrad accumulating into an existing gradient
    EPI_OUT | EPI_U | EPI_UDERIV,                         // dgrad through GELU (saved derivative)
};
constexpr int EPI_NMODES = (int)(sizeof(EPI_MODES) / sizeof(EPI_MODES[0]));

// stg: this wave's staging tile, 8-row groups of 1 KiB placed GS bytes apart; bias_lds: 64 floats of wave-private LDS.
template <bool CSUM, int GS, bool PF, int MODE>
__device__ __forceinline__ void fast_epilogue_rows_impl(const GemmArgs& p, f32x16_t (&acc)[4][2], char* stg, float* bias_lds,
                                                        int mrow0, int ncol0, int lane, unsigned rt_flags) {
  const unsigned F = MODE >= 0 ? EPI_MODES[MODE >= 0 ? MODE : 0] : rt_flags;  // compile-time constant when MODE >= 0
  const int h = lane >> 5, row = lane & 31;
  const bool has_bias = (F & EPI_BIAS) != 0, has_side = (F & (EPI_RESID | EPI_U)) != 0, has_u = (F & EPI_U) != 0;
  const bool has_pre = (F & EPI_PRE) != 0, has_out = (F & EPI_OUT) != 0, gelu = (F & EPI_GELU) != 0, has_pos = (F & EPI_POS) != 0;
  const bool save_deriv = (F & EPI_DERIV) != 0, u_is_deriv = (F & EPI_UDERIV) != 0;
  const bool nt_st = (F & EPI_NT_ST) != 0, nt_ld = (F & EPI_NT_LD) != 0;
  const bool partial = (F & EPI_PARTIAL) != 0;  // false: this wave's 128 x 64 block lies inside the matrix, no bounds predicates
  const bf16_t* side = has_u ? p.dgelu_u : p.resid;  // at most one of the two (fast_rows_ok)
  const long lds_ = has_u ? p.ldu : p.ldr;
  const int ch = lane & 7, nn = ncol0 + ch * 8;
  const bool n_ok = !partial || nn < p.N;
  if (has_bias) bias_lds[lane] = (!partial || ncol0 + lane < p.N) ? p.bias[ncol0 + lane] : 0.f;
  float cs[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) cs[e] = 0.f;
  u32x4_t sd[4];
  if (has_side && PF) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int mm = mrow0 + i * 8 + (lane >> 3);
      if (n_ok && (!partial || mm < p.M)) sd[i] = load16(side + (long)mm * lds_ + nn, nt_ld);
    }
  }
  __builtin_amdgcn_wave_barrier();
  // The epilogue is instruction-bound, not memory-bound (in-kernel cycle stamps, profiles/r03_gemm_tile_stamps.txt: 9.0 k cycles per
  // tile with bias only, 17 k with a side input -- with every global load and store REMOVED), so the per-value work is kept minimal:
  // the bias vectors of this wave's 64 columns are fetched once (not per 32-row block), alpha == 1 costs nothing, and values that
  // are already bf16 (unpacked from the staged pre-activation, no GELU / positional term applied) are not rounded again.
  const bool scale = (F & EPI_SCALE) != 0;
  const bool exact = !(gelu || has_pos);  // pass B's x[] are bf16 values exactly as unpacked
  // (hoisted only where 32 more registers are free: not beside side-input or GELU' temporaries, not in the generic instantiation)
  constexpr bool HOIST = MODE >= 0 && (EPI_MODES[MODE >= 0 ? MODE : 0] & (EPI_RESID | EPI_U | EPI_DERIV)) == 0;
  f32x4_t bv[2][4];
  if (HOIST) {
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int q = 0; q < 4; ++q) bv[nt][q] = has_bias ? *(const f32x4_t*)(bias_lds + nt * 32 + 8 * q + 4 * h) : f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  // staging addresses: the swizzle XOR only touches bits 4-6, so every chunk address is (lane base) ^ (chunk << 4)
  unsigned wbase = (unsigned)(size_t)stg + (row >> 3) * GS + (row & 7) * 128 + h * 8 + ((row & 7) << 4);
  unsigned rbase = (unsigned)(size_t)stg + (lane >> 3) * 128 + (((lane & 7) ^ ((lane >> 3) & 7)) << 4);
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    // (opaque re-definition per block: otherwise hipcc keeps all derived addresses of all four blocks live and spills)
    asm volatile("" : "+v"(wbase), "+v"(rbase));
    // pass A
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float v[4];
        const f32x4_t b4 = HOIST ? bv[nt][q] : has_bias ? *(const f32x4_t*)(bias_lds + nt * 32 + 8 * q + 4 * h) : f32x4_t{0.f, 0.f, 0.f, 0.f};
        if (scale) {
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = acc[mt][nt][q * 4 + i] * p.alpha + b4[i];
        } else if (has_bias) {
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = acc[mt][nt][q * 4 + i] + b4[i];
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = acc[mt][nt][q * 4 + i];
        }
        u32x2_t pk;
        pk[0] = pack_bf2(v[0], v[1]);
        pk[1] = pack_bf2(v[2], v[3]);
        *(lds_u32x2_ptr)(size_t)(wbase ^ ((nt * 4 + q) << 4)) = pk;
      }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_sched_barrier(0);  // keep the blocks apart: hipcc otherwise hoists work across them and spills
    // (PF == false, register-capped kernels: this block's own side inputs, right after its accumulators died)
    // side inputs of the next 32-row block (its accumulators' predecessors are dead now)
    u32x4_t sn[4];
    if (has_side && (mt < 3 || !PF)) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int mm = mrow0 + (mt + (PF ? 1 : 0)) * 32 + i * 8 + (lane >> 3);
        if (n_ok && (!partial || mm < p.M)) sn[i] = load16(side + (long)mm * lds_ + nn, nt_ld);
      }
    }
    // pass B
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r2 = i * 8 + (lane >> 3);
      const int mm = mrow0 + mt * 32 + r2;
      const bool ok = n_ok && (!partial || mm < p.M);
      const u32x4_t pre = *(lds_u32x4_ptr)(size_t)(rbase + i * GS);  // rows r2 = i*8 + (lane >> 3): (r2 & 7) == lane >> 3
      if (has_pre && !save_deriv && ok) store16(p.out_pre + (long)mm * p.ldc + nn, pre, nt_st);
      u32x4_t fin = pre;
      if (gelu || has_side || has_pos) {
        float x[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          x[2 * e] = bf_lo(pre[e]);
          x[2 * e + 1] = bf_hi(pre[e]);
        }
        if (save_deriv) {  // GELU and GELU' share the erf polynomial and the exponential
          float dv[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) gelu_and_deriv(x[e], x[e], dv[e]);
          if (has_pre && ok) {
            u32x4_t dpk;
#pragma unroll
            for (int e = 0; e < 4; ++e) dpk[e] = pack_bf2(dv[2 * e], dv[2 * e + 1]);
            store16(p.out_pre + (long)mm * p.ldc + nn, dpk, nt_st);
          }
        } else if (gelu) {
#pragma unroll
          for (int e = 0; e < 8; ++e) x[e] = gelu_f(x[e]);
        }
        if (has_pos && ok) {  // positional embedding row (m mod period), fp32 (conv2 + sinusoids)
          const float* pp = p.pos + (long)(mm % p.pos_period) * p.N + nn;
          const f32x4_t p0 = *(const f32x4_t*)pp, p1 = *(const f32x4_t*)(pp + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            x[e] = bf_round(x[e]) + p0[e];
            x[4 + e] = bf_round(x[4 + e]) + p1[e];
          }
        }
        if (has_side) {
          const u32x4_t sv = PF ? sd[i] : sn[i];
          if (has_u && u_is_deriv) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              x[2 * e] = (exact ? x[2 * e] : bf_round(x[2 * e])) * bf_lo(sv[e]);
              x[2 * e + 1] = (exact ? x[2 * e + 1] : bf_round(x[2 * e + 1])) * bf_hi(sv[e]);
            }
          } else if (has_u) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              x[2 * e] = (exact ? x[2 * e] : bf_round(x[2 * e])) * dgelu_f(bf_lo(sv[e]));
              x[2 * e + 1] = (exact ? x[2 * e + 1] : bf_round(x[2 * e + 1])) * dgelu_f(bf_hi(sv[e]));
            }
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              x[2 * e] = (exact ? x[2 * e] : bf_round(x[2 * e])) + bf_lo(sv[e]);
              x[2 * e + 1] = (exact ? x[2 * e + 1] : bf_round(x[2 * e + 1])) + bf_hi(sv[e]);
            }
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) fin[e] = pack_bf2(x[2 * e], x[2 * e + 1]);
      }
      if (CSUM && ok) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          cs[2 * e] += bf_lo(fin[e]);
          cs[2 * e + 1] += bf_hi(fin[e]);
        }
      }
      if (has_out && ok) store16(p.out + (long)mm * p.ldc + nn, fin, nt_st);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (PF) {
#pragma unroll
      for (int i = 0; i < 4; ++i) sd[i] = sn[i];
    }
  }
  if (CSUM) {  // lanes sharing (lane & 7) hold partial sums of the same 8 columns
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float t = cs[e];
      t += __shfl_xor(t, 8);
      t += __shfl_xor(t, 16);
      t += __shfl_xor(t, 32);
      cs[e] = t;
    }
    if (lane < 8 && n_ok) {
      if (p.colsum_scratch) {  // one partial row per 128-row wave block, written exactly once: no atomics
        float* dst = p.colsum_scratch + (long)(mrow0 >> 7) * p.N + nn;
        *(f32x4_t*)dst = f32x4_t{cs[0], cs[1], cs[2], cs[3]};
        *(f32x4_t*)(dst + 4) = f32x4_t{cs[4], cs[5], cs[6], cs[7]};
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) unsafeAtomicAdd(p.colsum + nn + e, cs[e]);
      }
    }
  }
}

template <bool CSUM, int GS, bool PF, int MODE>
__device__ __forceinline__ bool fast_epilogue_rows_try(const GemmArgs& p, f32x16_t (&acc)[4][2], char* stg, float* bias_lds, int mrow0,
                                                       int ncol0, int lane, unsigned flags) {
  if constexpr (MODE >= EPI_NMODES) {
    return false;
  } else {
    if (flags == EPI_MODES[MODE]) {
      fast_epilogue_rows_impl<CSUM, GS, PF, MODE>(p, acc, stg, bias_lds, mrow0, ncol0, lane, flags);
      return true;
    }
    return fast_epilogue_rows_try<CSUM, GS, PF, MODE + 1>(p, acc, stg, bias_lds, mrow0, ncol0, lane, flags);
  }
}
template <bool CSUM, int GS = 1024, bool PF = true>
__device__ __forceinline__ void fast_epilogue_rows(const GemmArgs& p, f32x16_t (&acc)[4][2], char* stg, float* bias_lds,
                                                   int mrow0, int ncol0, int lane) {
  const bool partial = mrow0 + 128 > p.M || ncol0 + 64 > p.N;  // wave-uniform
  const unsigned flags = epi_flags_of(p, partial);
  if (!fast_epilogue_rows_try<CSUM, GS, PF, 0>(p, acc, stg, bias_lds, mrow0, ncol0, lane, flags))
    fast_epilogue_rows_impl<CSUM, GS, PF, -1>(p, acc, stg, bias_lds, mrow0, ncol0, lane, flags);
}

// Epilogue shared by the direct-to-LDS kernels: each wave owns a 128 x 64 block of the output tile as acc[4][2]
// 32x32 MFMA blocks (rows m0 + wm*128 + mt*32, columns n0 + wn*64 + nt*32).  All waves of the workgroup must be past
// their last main-loop LDS read (the staging tiles alias the operand images).
// stg: this wave's 4 KiB staging tile, bias_lds: this wave's 64 floats.
template <bool SWAP, bool CSUM, bool PF = true>
__device__ __forceinline__ void fast_epilogue(const GemmArgs& p, f32x16_t (&acc)[4][2], char* stg, float* bias_lds, int m0, int n0,
                                              int wm, int wn, int lane) {
  if (SWAP) {  // bf16 outputs (the host routes anything fast_rows_ok() rejects to the general kernel)
    fast_epilogue_rows<CSUM, 1024, PF>(p, acc, stg, bias_lds, m0 + wm * 128, n0 + wn * 64, lane);
    return;
  }
  const int h = lane >> 5;
  {
    // D[m][n]: lane owns column n = .. + (lane & 31), rows (r & 3) + 8*(r >> 2) + 4*h.  fp32 atomic accumulate only.
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int n = n0 + wn * 64 + nt * 32 + (lane & 31);
      if (n >= p.N) continue;
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + wm * 128 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
          if (m < p.M) unsafeAtomicAdd(p.out_f32 + (long)m * p.ldc32 + n, p.alpha * acc[mt][nt][r]);
        }
      }
    }
  }
}

}  // namespace

// ---- between gemm.hip and the family files -----------------------------------------------------------------------------------------
// What gemm_route (gemm.hip) decides for one call: the kernel family, the instantiation inside it (what were template parameters of the
// dispatch), and the one step that follows the kernel.
enum class GemmFamily { General = 0, Skinny, Fast, PingPong };
enum class GemmPost { None = 0, ColsumFromOut = 1, ColsumFromScratch = 2 };  // reduce the column sums afterwards: of `out`, or of the scratch rows
struct GemmRoute {
  GemmFamily family = GemmFamily::General;
  int fbn = 0, nwn = 0, nstage = 0;  // Fast: 128, 2, 1 (256 x 128 tiles, one stage) or 256, 4, 2 (256 x 256, two stages)
  bool swap = false, csum = false;   // Fast / PingPong: MFMA operand order (bf16 outputs: swapped), fused column sums
  int pp_var = 0;                    // PingPong: K-tile schedule, 2 or 7
  GemmPost post = GemmPost::None;
};

// One compiled instantiation as its family file keeps it (a function-local static, built once): the host handle, the symbol as rocprofv3
// prints it (template arguments included), and the per-device state of its dynamic-LDS attribute.
struct GemmKernel {
  const void* handle;
  std::string symbol;
  LdsAttrOnce lds_attr;
};
struct GemmLaunch {
  dim3 grid, block;
  int lds;       // dynamic LDS bytes (0: none, the attribute is left alone)
  double flops;  // algorithmic flops of the call, for the profile record
  bool persistent;
};
static inline double gemm_flops(const GemmArgs& a) { return 2.0 * (double)a.M * (double)a.N * (double)a.K; }
static inline const char* gemm_tf(bool b) { return b ? "true" : "false"; }  // template arguments in a kernel symbol, as rocprofv3 prints them

#define GEMM_INTERNAL __attribute__((visibility("hidden")))
// gemm.hip: the one launch path.  Sets the kernel's dynamic-LDS attribute (once per device) and launches it on `stream` with `a` as its
// argument.  With profiling on (gemm_profile_enable) the launch's record is pushed and the launch runs between a pair of pooled events; with
// it off this makes no HIP call beyond the launch and its check.  The profile state itself is not visible outside gemm.hip.
GEMM_INTERNAL int gemm_timed_launch(GemmKernel& k, const GemmLaunch& l, const GemmArgs& a, hipStream_t stream);
// The family files: the instantiation a route names (null: not compiled), and its launch.
GEMM_INTERNAL GemmKernel* gemm_general_kernel(bool ta, bool tb);      // gemm_general.hip: gemm_kernel<ta, tb>
GEMM_INTERNAL GemmKernel* gemm_skinny_kernel_of(int M);               //                   gemm_skinny_kernel<1 | 2>
GEMM_INTERNAL GemmKernel* gemm_fast_kernel_of(bool ta, bool tb, const GemmRoute& r);  // gemm_fast.hip
GEMM_INTERNAL GemmKernel* gemm_pp_kernel_of(bool ta, bool tb, const GemmRoute& r);    // gemm_pp.hip
GEMM_INTERNAL int gemm_launch_general(const GemmArgs& a, hipStream_t stream);
GEMM_INTERNAL int gemm_launch_skinny(const GemmArgs& a, hipStream_t stream);
GEMM_INTERNAL int gemm_launch_fast(const GemmArgs& a, const GemmRoute& r, hipStream_t stream);
// want_persistent: oasr_gemm_set_variant's launch rule (-1 = default: the OASR_PP_PERSISTENT experiment env, else plain)
GEMM_INTERNAL int gemm_launch_pp(const GemmArgs& a, const GemmRoute& r, int want_persistent, hipStream_t stream);
