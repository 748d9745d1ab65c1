// What more than one of the flash-attention kernel files shares (attention.hip describes the kernels and their register layout):
// the swizzled 64x64 LDS tile and its fragment readers, the row-coalesced store epilogue, the block / row addressing of the chunked
// and the compact-grid launches, the LDS-DMA ring pieces, the key-length clamp, the row addressing and the row setup of the two dQ kernels.
// A shared piece is one whose extraction left every kernel's instruction stream as it was (scripts/isa_compare.py,
// profiles/attention_split_isa.txt); where it did not, the kernels keep their copies and say so.
#pragma once
#include "decode_shared.h"

namespace {

using dec::LN2;
using dec::LOG2E;
using dec::NEG;
using dec::SCALE;  // 1/sqrt(64)
constexpr int TILE = 64 * 64 * 2;  // one 64x64 bf16 tile

typedef __attribute__((address_space(3))) s16x4_t* lds_s16x4_ptr;

// Bank-conflict swizzle of a [64 rows][128 B] tile: chunk c16 of row r lives at chunk c16 ^ f((r >> 1) & 7), f(x) = x ^ ((x & 1) << 2).
//  * ds_read_b128 (frag_rows) is served in 16-lane groups whose rows cover every value of (r >> 1) & 7 exactly twice (once per
//    row parity = bank half): any bijection of that value keeps the 16 x 4 banks distinct;
//  * ds_read_b64_tr_b16 (frag_cols) is served in 32-lane groups = 4 consecutive rows x 4 consecutive chunks: rows r and r + 2 share
//    the bank half, so their chunk sets must be disjoint, i.e. f must differ in bit 2 between (r >> 1) and (r >> 1) + 1.  The plain
//    XOR with (r >> 1) & 7 did not (measured: 20-25 % of the LDS cycles of the three kernels were conflicts).
__device__ __forceinline__ int tile_addr(int row, int c16) {
  const int x = (row >> 1) & 7;
  return row * 128 + ((c16 ^ x ^ ((x & 1) << 2)) << 4);
}

// cooperative 64x64 tile: each of 256 threads moves 2 x 16 bytes.  Bounds-checked buffer loads: the descriptor covers
// rows [0, rmax) of this (batch, head) slice, so rows past the end read as zeros (their scores are masked, and zero V
// rows keep 0 * V finite); the per-thread offsets are loop invariants and the tile advance is a scalar offset, so the
// loop carries no vector address arithmetic.
struct TileSrc {
  __amdgpu_buffer_rsrc_t rs;
  unsigned voff[2];
  unsigned row_bytes;
};
__device__ __forceinline__ TileSrc tile_src(const bf16_t* base, long ld, int rmax, int tid) {
  TileSrc t;
  // last valid byte: row (rmax-1), 64 columns
  t.rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(base), 0, (int)(((long)(rmax - 1) * ld + 64) * 2), 0x00020000);
  t.row_bytes = (unsigned)(ld * 2);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int id = tid + 256 * i;
    t.voff[i] = (unsigned)((id >> 3) * ld * 2 + (id & 7) * 16);
  }
  return t;
}
__device__ __forceinline__ void tile_issue(const TileSrc& t, int row0, u32x4_t (&r)[2]) {
  const unsigned soff = (unsigned)row0 * t.row_bytes;
#pragma unroll
  // the tile offset goes into the VGPR offset: on gfx9-class raw buffers the range check does not cover soffset
  for (int i = 0; i < 2; ++i) r[i] = __builtin_amdgcn_raw_buffer_load_b128(t.rs, t.voff[i] + soff, 0, 0);
}
__device__ __forceinline__ void tile_commit(char* lds, int tid, const u32x4_t (&r)[2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int id = tid + 256 * i;
    *(u32x4_t*)(lds + tile_addr(id >> 3, id & 7)) = r[i];
  }
}
// MFMA operand: lane holds tile row (sub + (l & 31)), 8 contiguous columns ds*16 + (l >> 5)*8 ..
__device__ __forceinline__ bf16x8_t frag_rows(const char* lds, int sub, int ds, int lane) {
  return *(const bf16x8_t*)(lds + tile_addr(sub + (lane & 31), ds * 2 + (lane >> 5)));
}
// MFMA operand from the TRANSPOSE of the tile: lane holds column (csub + (l & 31)) and the 8 rows
// rbase + 8*(j >> 2) + 4*(l >> 5) + (j & 3), j = 0..7 -- exactly the rows a 32x32 accumulator's registers
// 8u..8u+7 cover, so a packed accumulator half is the matching other operand.
__device__ __forceinline__ bf16x8_t frag_cols(const char* lds, int rbase, int csub, int lane) {
  const int G = lane >> 4, i = lane & 15;
  const int row = rbase + 4 * (G >> 1) + (i >> 2);
  const int col = csub + (G & 1) * 16 + (i & 3) * 4;
  const int a0 = tile_addr(row, col >> 3) + (col & 7) * 2;
  const int a1 = tile_addr(row + 8, col >> 3) + (col & 7) * 2;
  const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(lds + a0));
  const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(lds + a1));
  const s16x8_t v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8_t, v);
}
__device__ __forceinline__ bf16x8_t pack_half(const f32x16_t& p, int u) {
  u32x4_t o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = pack_bf2(p[8 * u + 2 * i], p[8 * u + 2 * i + 1]);
  return __builtin_bit_cast(bf16x8_t, o);
}
__device__ __forceinline__ bf16x8_t ld_frag_global(const bf16_t* p) { return __builtin_bit_cast(bf16x8_t, *(const u32x4_t*)p); }
__device__ __forceinline__ int acc_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }
// ---- row-coalesced output stores --------------------------------------------------------------------------------------
// The kernels hold their results transposed, T[dt][r] = out[row = lane & 31][col = dt*32 + acc_row(r, lane >> 5)]: a lane owns
// one output row but only 4 consecutive columns per register group, so direct stores are 8-byte pieces scattered over
// 32 rows per instruction (measured: the forward kernel spends 14 % of its time issuing them).  Instead each wave
// transposes through a private LDS tile and every lane stores 16 contiguous bytes, 8 lanes covering one 128-byte row
// segment.  `stg`: wave-private, 4 KiB; all waves must be done with the operand tiles.
// `wave_sums` (optional, 64 floats of LDS owned by this wave): receives the column sums of the bf16 values stored for
// the valid rows (the caller combines the waves and writes ONE partial row per workgroup -- fp32 atomics from every wave
// onto the same d addresses were measured to cost more than the kernel itself).
__device__ __forceinline__ void store_rows_bf16(char* stg, const f32x16_t (&T)[2], float scale, bf16_t* gbase, long ld, int rows_valid,
                                                int lane, float* wave_sums = nullptr) {
  const int row = lane & 31, hh = lane >> 5;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      u32x2_t o;
      o[0] = pack_bf2(T[dt][4 * g4] * scale, T[dt][4 * g4 + 1] * scale);
      o[1] = pack_bf2(T[dt][4 * g4 + 2] * scale, T[dt][4 * g4 + 3] * scale);
      *(u32x2_t*)(stg + row * 128 + (((dt * 4 + g4) ^ (row & 7)) << 4) + hh * 8) = o;
    }
  __builtin_amdgcn_wave_barrier();
  float cs[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) cs[e] = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r2 = i * 8 + (lane >> 3), ch = lane & 7;
    const u32x4_t v = *(const u32x4_t*)(stg + r2 * 128 + ((ch ^ (r2 & 7)) << 4));
    if (r2 < rows_valid) {
      *(u32x4_t*)(gbase + (long)r2 * ld + ch * 8) = v;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        cs[2 * e] += bf_lo(v[e]);
        cs[2 * e + 1] += bf_hi(v[e]);
      }
    }
  }
  if (wave_sums) {  // (wave-uniform) lanes sharing (lane & 7) hold partial sums of the same 8 columns
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float t = cs[e];
      t += __shfl_xor(t, 8, 64);
      t += __shfl_xor(t, 16, 64);
      t += __shfl_xor(t, 32, 64);
      cs[e] = t;
    }
    if (lane < 8) {
#pragma unroll
      for (int e = 0; e < 8; ++e) wave_sums[lane * 8 + e] = cs[e];  // zeros when this wave has no valid row
    }
  }
  __builtin_amdgcn_wave_barrier();
}

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)

// Chunked token rows (AttnArgs.q_rows / k_rows, kernels.h): first row of the 64-position chunk that holds position t of sample b.
// Wave-uniform when t is (scalar load); entries past the last chunk hold a row far outside every tensor.
__device__ __forceinline__ int chunk_row(const int32_t* rows, int b, int t) { return rows[b * OASR_ROWTAB + (t >> 6)] + (t & 63); }

// Which (sample, head, query / key block) a workgroup works on.  Full grid: `bid` counts (b, h, block) with `nblk` blocks per (b, h).
// Compact grid of a span-limited launch (ROWS only; kernels.h: AttnArgs.qblk128 / qblk256): `bid` indexes the table of the blocks that
// lie inside the spans, in the same (b, h, block) order -- one scalar load, and no workgroup exists for a block past the span.
struct BlockId {
  int b, h, blk;
};
template <bool ROWS>
__device__ __forceinline__ BlockId block_id(const int32_t* tab, int bid, int nblk, int H) {
  BlockId r;
  if (ROWS && tab) {  // (block-uniform)
    const int e = tab[bid];
    r.b = e >> 16;
    r.h = (e >> 4) & 0xfff;
    r.blk = e & 15;
  } else {
    const int bh = bid / nblk;
    r.b = bh / H;
    r.h = bh - r.b * H;
    r.blk = bid - bh * nblk;
  }
  return r;
}

// Softmax arithmetic on pairs: gfx950's v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 process two fp32 values per lane per
// issue slot.  With head_dim 64 these kernels are VALU-issue bound (16 MFMAs against ~145 scalar VALU per 64-key tile and
// wave in the forward), so halving the fma / add / mul counts is what moves them; the exponential stays one v_exp_f32 each.
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2_t pk_fma(f32x2_t a, f32x2_t b, f32x2_t c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x2_t pk_exp2(f32x2_t a) {
  f32x2_t r;
  r[0] = __builtin_amdgcn_exp2f(a[0]);
  r[1] = __builtin_amdgcn_exp2f(a[1]);
  return r;
}

// ---- LDS-DMA ring helpers (used by the forward, attention_fwd.hip, and by the ping-pong backward kernels, where the scheme is described:
// attention_bwd_dq.hip) ----
#define ATTN_FENCE() __builtin_amdgcn_sched_barrier(0)
constexpr int PNS = 4;          // ring stages
constexpr int PSTG = 2 * TILE;  // two 64-row tiles per stage

// The DMA is issued from inline assembly on purpose: hipcc orders every later ds_read behind a compiler-visible LDS-DMA with
// s_waitcnt vmcnt(0) (it cannot tell the ring stages apart), which would drain the tiles in flight at every step.  The loops
// count their own pieces (s_waitcnt vmcnt(n) + s_barrier before a stage is read); in-order return makes any compiler-placed
// vmcnt for its own loads merely conservative.  (m0 is reserved: the compiler-generated code of these kernels has no other user.)
__device__ __forceinline__ void glds16_asm(const u32x4_t rs, unsigned lds_addr, unsigned voff) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(lds_addr), "v"(voff), "s"(rs) : "memory");
}
struct PipeSrc1 {
  u32x4_t rs;  // raw buffer descriptor over rows [0, rmax) of this (batch, head) slice, 64 columns
  unsigned voff;
  unsigned tile_bytes;
};
// Piece p (1 KiB = 8 rows) of a 64-row tile lands at LDS bytes [p * 1024, +1024) of the tile; lane l writes chunk c' = l & 7 of row
// 8p + (l >> 3), which under tile_addr's swizzle holds source chunk c' ^ g(row).  Wave w of 8 moves piece w of each tile.
__device__ __forceinline__ PipeSrc1 pipe_src1(const bf16_t* base, long ld, int rmax, int wave, int lane) {
  PipeSrc1 t;
  const unsigned long addr = (unsigned long)base;
  t.rs[0] = (unsigned)addr;
  t.rs[1] = (unsigned)(addr >> 32) & 0xffffu;  // stride 0: raw buffer
  t.rs[2] = (unsigned)(((long)(rmax - 1) * ld + 64) * 2);
  t.rs[3] = 0x00020000u;
  t.tile_bytes = (unsigned)(64 * ld * 2);
  const int row = wave * 8 + (lane >> 3);
  const int x = (row >> 1) & 7;
  const int c = (lane & 7) ^ x ^ ((x & 1) << 2);
  t.voff = (unsigned)(row * ld * 2 + c * 16);  // the tile offset is added here too: the range check does not cover soffset
  return t;
}
#define ATTN_BARRIER()                          \
  do {                                          \
    ATTN_FENCE();                               \
    asm volatile("s_barrier" ::: "memory");     \
    ATTN_FENCE();                               \
  } while (0)

// ---- pieces that stood in several kernels -----------------------------------------------------------------------------------------
// Keys of sample b that are visible at all: kv_len[b] (when given), at most Tk.
__device__ __forceinline__ int clamped_kv_len(const AttnArgs& a, int b) {
  const int kv_len = a.kv_len ? a.kv_len[b] : a.Tk;
  return kv_len < a.Tk ? kv_len : a.Tk;
}

// Row of (sample b, position t, head h) in a [.., H * 64] tensor with token stride ld: in chunked token rows (`rows`: q_rows / k_rows, batch
// stride unused) or in the plain strided layout (batch stride bs).  `base` is the tensor's pointer (-> the row's address) or 0L (-> its
// element offset, for several tensors of the same strides); the sum keeps the order the kernels wrote it in, which their address
// arithmetic was compiled from.
template <typename P>
__device__ __forceinline__ P row_at(P base, bool chunked, const int32_t* rows, int b, int t, long ld, long bs, int h) {
  return chunked ? base + (long)chunk_row(rows, b, t) * ld + h * 64 : base + (long)b * bs + (long)t * ld + h * 64;
}

// Row setup of the dQ kernels for the lane's query row myq_c (myq clamped into the block; an inactive wave, !w_act, re-reads rows of the
// block's first chunk and takes d_o as zeros): the Q and dO fragments, delta = rowsum(dO . (O + O_lo)) -- stored for the dK/dV kernel --
// and lse in the log2 domain.
template <bool ROWS>
__device__ __forceinline__ void dq_row_setup(const AttnArgs& a, int b, int h, int myq, int myq_c, bool w_act, int hh, bf16x8_t (&qf)[4],
                                             bf16x8_t (&dof)[4], float& delta, float& lse2) {
  const bf16_t* qp = row_at(a.q, ROWS, a.q_rows, b, myq_c, a.ldq, a.bsq, h);
  const long orow_off = row_at(0L, ROWS, a.q_rows, b, myq_c, a.ldo, a.bso, h);
  const bf16_t* dop = a.d_o + orow_off;
  const bf16_t* op = a.o + orow_off;
  const bf16_t* olop = a.o_lo ? a.o_lo + orow_off : nullptr;
  float dpart = 0.f;
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) {
    qf[ds] = ld_frag_global(qp + ds * 16 + hh * 8);
    u32x4_t d4 = *(const u32x4_t*)(dop + ds * 16 + hh * 8);
    if (ROWS && !w_act) d4 = u32x4_t{0u, 0u, 0u, 0u};
    dof[ds] = __builtin_bit_cast(bf16x8_t, d4);
    const u32x4_t o4 = *(const u32x4_t*)(op + ds * 16 + hh * 8);
    if (olop) {  // O = bf16 O + bf16 rounding residual (an fp32-grade O in 4 bytes per element, like the forward wrote it)
      const u32x4_t r4 = *(const u32x4_t*)(olop + ds * 16 + hh * 8);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        dpart += bf_lo(d4[i]) * (bf_lo(o4[i]) + bf_lo(r4[i])) + bf_hi(d4[i]) * (bf_hi(o4[i]) + bf_hi(r4[i]));
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) dpart += bf_lo(d4[i]) * bf_lo(o4[i]) + bf_hi(d4[i]) * bf_hi(o4[i]);
    }
  }
  delta = dpart + __shfl_xor(dpart, 32, 64);
  const long stat_idx = ((long)b * a.H + h) * a.Tq + myq_c;
  if (hh == 0 && myq < a.Tq && w_act) a.delta[stat_idx] = delta;  // (test order as the kernels had it: profiles/attention_split_isa.txt [3])
  lse2 = a.lse[stat_idx] * LOG2E;
}

}  // namespace

// One host function per kernel: picks the instantiation from a.causal / a.q_rows and launches it over `grid` (attention.hip decides which
// kernel runs, over which grid and with which arguments).  Internal to the library: kept out of its dynamic symbol table.
#define ATTN_INTERNAL __attribute__((visibility("hidden")))
ATTN_INTERNAL void attn_launch_fwd(const AttnArgs& a, dim3 grid, hipStream_t s);
ATTN_INTERNAL void attn_launch_decode(const AttnArgs& a, hipStream_t s);
ATTN_INTERNAL void attn_launch_bwd_dq(const AttnArgs& a, dim3 grid, hipStream_t s);
ATTN_INTERNAL void attn_launch_bwd_dq_pp(const AttnArgs& a, dim3 grid, hipStream_t s);
ATTN_INTERNAL void attn_launch_bwd_dkdv(const AttnArgs& a, dim3 grid, hipStream_t s);
ATTN_INTERNAL int attn_launch_bwd_dkdv_pp(const AttnArgs& a, dim3 grid, hipStream_t s);  // (sets the kernel's dynamic LDS size first: may fail)
