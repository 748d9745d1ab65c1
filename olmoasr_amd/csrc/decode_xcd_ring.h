// Device-only parts of the one-XCD step engine (decode_xcd.hip) that are not a phase: the kernel's arguments, the per-wave producer of ring blocks
// (unit table, LDS-DMA issue, counted waits), the fast run over a steady-state ring, and the team barrier.  The block SEQUENCE the producer
// follows is decode_xcd_plan.h's (shared with the host); decode_xcd.hip holds the phases, the kernel and the launcher.
#pragma once
#include "decode_shared.h"
#include "decode_xcd_plan.h"

namespace {

constexpr int XR = 6;        // ring slots per streaming wave
constexpr int SLOT = 4096;   // bytes per slot: 4 DMA instructions of 64 lanes x 16 B
constexpr unsigned SPIN_LIMIT = 1u << 21;
constexpr unsigned XL_RING = 0;  // the rings open the kernel's dynamic LDS block: 4 waves x XR slots (the rest of the layout: decode_xcd.hip)

struct XArgs : DecodeStepBufs {  // (rows exchanged through agent-scope accesses; part: [M * H * ns][66])
  int d, H, Te, S_max, L, M, pos, team, stride;
  int flags;             // experiments (decode_step_core.h: StepFlags)
  unsigned long long* stamps;  // optional [8 phases][8] s_memtime stamps of workgroup 0 in layer 1 (null: off)
  DecLayerOffsets l0;    // decoder layer 0; layer l = dec::layer_at(l0, l, lstride, astride): the blocks are laid out back to back (host-checked)
  long lstride, astride;
};

// (experiment switch: plain stores -- they stay in this XCD's L2, which is all a team on ONE XCD needs; not valid for a spread team)
__device__ __forceinline__ void st4_x(void* p, unsigned v, int flags) {
  if (flags & dec::XF_PLAIN_STORES) *(volatile unsigned*)p = v;
  else st4_agent(p, v);
}

// ---- LDS-DMA of one ring block (4 x 1 KiB), issued from inline assembly (hipcc would otherwise order every later ds_read behind it with
// s_waitcnt vmcnt(0) and drain the ring) ----------------------------------------------------------------------------------------------
__device__ __forceinline__ void dma16_s(const u32x4_t rs_in, unsigned lds_addr, unsigned voff, unsigned soff) {
  u32x4_t rs;  // (re-pinned: a descriptor that travelled through a loop-carried struct comes back as VGPRs)
  rs[0] = __builtin_amdgcn_readfirstlane(rs_in[0]), rs[1] = __builtin_amdgcn_readfirstlane(rs_in[1]);
  rs[2] = 0x7fffffffu, rs[3] = 0x00020000u;
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(__builtin_amdgcn_readfirstlane(lds_addr)), "v"(voff), "s"(rs),
               "s"(__builtin_amdgcn_readfirstlane(soff))
               : "memory");
}
__device__ __forceinline__ u32x4_t rsrc_of(const void* base) {
  const unsigned long addr = (unsigned long)base;
  u32x4_t rs;  // (readfirstlane: the descriptor must sit in SGPRs; the inline-asm "s" constraint does not move it there by itself)
  rs[0] = __builtin_amdgcn_readfirstlane((unsigned)addr);
  rs[1] = __builtin_amdgcn_readfirstlane((unsigned)(addr >> 32) & 0xffffu);  // stride 0: raw buffer
  rs[2] = 0x7fffffffu;
  rs[3] = 0x00020000u;
  return rs;
}
#define XWAIT_VM(N) asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory")
#define XBAR() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// ---- the producer: a table of UNITS per wave ------------------------------------------------------------------------------------------
// A unit = a run of ring blocks that share one descriptor and one set of per-lane offsets: all tiles of one projection segment that belong
// to this workgroup (consecutive tiles lie a constant distance apart), the full blocks of one item's K (or V) stream, or the one clamped
// block that ends a stream.  The units of decoder layer 0 are listed ONCE per launch by walking the cursor (the CPU-tested sequence) and
// kept in a wave-private LDS table; layer l adds l x (layer stride) to the soffset.  Issuing a block is then: 4 DMA instructions, three
// scalar updates, and -- at a unit's end -- one 16-byte LDS read.  (Versions 1-5 advanced the cursor per block: ~2 k cycles of single-wave
// instruction issue at every unit boundary, profiles/r05_decode_xcd_stamps_v5.txt.)
constexpr int XTABN = 32;  // units per layer and wave (6 projection segments + 4 per cross-attention item, <= 5 items)
struct XStream {  // per streaming wave (all fields wave-uniform, SGPR-resident)
  bool more;      // the producer has blocks left
  int issued, consumed;
  int islot, cslot;  // issued % XR, consumed % XR, kept incrementally
  int u, nunits, layer;  // current unit, units per layer, layer of the block to issue next
  unsigned soff, jump;   // soffset of the next block; step from a tile's last block to this workgroup's next tile (weights)
  int left, kind;        // blocks left in the unit; lane-offset set: 0 weights K = d, 1 weights K = 4d, 2 cross K/V, 3 cross K/V last (clamped) block
  int tleft, tnkb;       // blocks left in the tile being issued (incl. the next one), blocks per tile
};
// per-lane byte offsets that do not depend on the block (computed once per wave): the DMA source offsets of a weight block for K = d / K = 4d,
// of a K/V block, of the clamped last K/V block of the partial key segment, and the LDS fragment offsets of the 4 k16 steps of a weight block
struct XLane {
  unsigned w_d[4], w_4d[4], kv[4], kvc[4], frag[4];
};
__device__ __forceinline__ XLane make_lane(int d, int Te, int wave, int lane) {
  XLane v;
  const int r8 = lane >> 3, l8 = lane & 7, row = lane & 31, kc = lane >> 5;
  const int n_p = Te - (Te > dec::SEG_KEYS ? dec::SEG_KEYS : 0);  // keys of the last (possibly partial) segment
  const int last = n_p - 1 - 128 * ((n_p - 1) >> 7);              // last valid key of its last block, relative to that block
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c16 = l8 ^ ((q * 4 + (r8 >> 1)) & 7);
    v.w_d[q] = (unsigned)(((q * 8 + r8) * d + c16 * 8) * 2);
    v.w_4d[q] = (unsigned)(((q * 8 + r8) * 4 * d + c16 * 8) * 2);
    const int t = 32 * q + 8 * wave + r8;
    v.kv[q] = (unsigned)((t * 2 * d + l8 * 8) * 2);
    v.kvc[q] = (unsigned)(((t < last ? t : last) * 2 * d + l8 * 8) * 2);  // keys past the segment's end re-read its last key (never used)
    v.frag[q] = (unsigned)(row * 128 + (((2 * q + kc) ^ ((row >> 1) & 7)) << 4));
  }
  return v;
}

// List the units of decoder layer 0 for this wave into its LDS table (4 words each: soffset, blocks, kind | blocks per tile << 8, tile jump);
// returns their number.  Runs once per launch; walks the same cursor functions the CPU test pins.
struct XBuild {  // what the unit walk needs, BY VALUE (a reference to the kernel arguments would pull them out of SGPRs into scratch memory)
  int d, H, Te, M, L, team, wg;
  long w[6];  // layer 0 weight offsets by streamed segment: qkv, attn.out, cross q, (3 unused), cross out, mlp.0, mlp.2 -> indices 0,1,2,3,4,5
};
__device__ __attribute__((noinline)) int build_units(XBuild p, int wave, int lane, unsigned* tab) {
  const XGeom g = make_geom(p.d, p.H, p.Te, p.M, p.L, p.team, p.wg);
  XCur c{0, 0, 0, 0};
  bool more = cur_normalise(g, c);
  int n = 0;
  while (more && c.layer == 0 && n < XTABN) {
    unsigned soff, jump = 0;
    int nblk, kind, tnkb = 0x400000;
    if (c.seg == 3) {
      const XItem it = item_of(g, c.idx);
      const bool is_v = c.sub >= it.kvb;
      const int j = is_v ? c.sub - it.kvb : c.sub;
      soff = (unsigned)((((long)it.b * p.Te + (long)it.sg * dec::SEG_KEYS + 128 * j) * 2 * p.d + it.h * 64 + (is_v ? p.d : 0)) * 2);
      const int nfull = it.n >> 7;
      if (nfull > j) nblk = nfull - j, kind = 2;
      else nblk = 1, kind = 3;
      c.sub += nblk;
      more = cur_advance_from(g, c);
    } else {
      const long woff = p.w[c.seg < 3 ? c.seg : c.seg - 1];
      const int K = c.seg == 6 ? 4 * p.d : p.d, nkb = c.seg == 6 ? g.nkb_4d : g.nkb_d;
      const int tile = g.wg + g.team * c.idx;
      soff = (unsigned)((unsigned long)((woff + ((long)tile * 32) * K + (long)wave * (K >> 2)) * 2));  // relative to the arena's bf16 shadow
      nblk = (seg_cnt(g, c.seg) - c.idx) * nkb, kind = c.seg == 6 ? 1 : 0, tnkb = nkb;
      jump = (unsigned)((long)g.team * 32 * K * 2 - (long)(nkb - 1) * 128);
      c.idx = seg_cnt(g, c.seg), c.sub = 0;
      more = cur_normalise(g, c);
    }
    if (lane == 0) {
      tab[4 * n] = soff, tab[4 * n + 1] = (unsigned)nblk, tab[4 * n + 2] = (unsigned)kind | ((unsigned)tnkb << 8), tab[4 * n + 3] = jump;
    }
    ++n;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (read back by this wave only)
  return n;
}
// load unit st.u of layer st.layer into the producer state
__device__ __forceinline__ void unit_load(const XArgs& a, XStream& st, const unsigned* tab) {
  const u32x4_t e = *(const u32x4_t*)(tab + 4 * st.u);
  const int kind = XU(e[2] & 0xffu);
  const long stride = kind >= 2 ? a.cache_lstride : a.lstride;
  st.soff = XU(e[0] + (unsigned)((long)st.layer * stride * 2));
  st.left = XU(e[1]);
  st.kind = kind;
  st.tnkb = XU(e[2] >> 8);
  st.tleft = st.tnkb;
  st.jump = XU(e[3]);
}
// after a block has been issued: next block of the unit, next tile, or next unit / layer
__device__ __forceinline__ void unit_advance(const XArgs& a, XStream& st, const unsigned* tab) {
  st.left = XU(st.left - 1);
  if (st.left == 0) {
    st.u = XU(st.u + 1);
    if (st.u == st.nunits) st.u = 0, st.layer = XU(st.layer + 1);
    if (st.layer == a.L) st.more = false;
    else unit_load(a, st, tab);
  } else if (st.tleft == 1) {
    st.soff = XU(st.soff + st.jump), st.tleft = st.tnkb;  // the tile's last block: on to this workgroup's next tile of the segment
  } else {
    st.soff = XU(st.soff + (st.kind >= 2 ? (unsigned)(128 * 2 * a.d * 2) : 128u)), st.tleft = XU(st.tleft - 1);
  }
}
// the four DMA instructions of one block
__device__ __forceinline__ void issue_block(const XStream& st, const XLane& lv, const u32x4_t rs_w, const u32x4_t rs_kv, unsigned dst) {
  const int kind = XU(st.kind);
  const unsigned soff = XU(st.soff);
  if (kind == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) dma16_s(rs_w, dst + q * 1024, lv.w_d[q], soff);
  } else if (kind == 1) {
#pragma unroll
    for (int q = 0; q < 4; ++q) dma16_s(rs_w, dst + q * 1024, lv.w_4d[q], soff);
  } else if (kind == 2) {
#pragma unroll
    for (int q = 0; q < 4; ++q) dma16_s(rs_kv, dst + q * 1024, lv.kv[q], soff);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) dma16_s(rs_kv, dst + q * 1024, lv.kvc[q], soff);
  }
}
struct XProd {  // launch constants of the producer
  u32x4_t rs_w, rs_kv;  // descriptors: the bf16 shadow of the parameter arena; layer 0's cross K/V
  const unsigned* tab;  // this wave's unit table (LDS)
  unsigned ring_lds;    // LDS byte address of this wave's ring
};
// the ring slot behind `slot`
__device__ __forceinline__ int ring_next(int slot) { return XU(slot + 1 == XR ? 0 : slot + 1); }
// issue the next block into ring slot islot and advance
__device__ __forceinline__ void ring_issue(const XArgs& a, XStream& st, const XLane& lv, const XProd& pr) {
  if (!st.more) return;
  issue_block(st, lv, pr.rs_w, pr.rs_kv, pr.ring_lds + (unsigned)st.islot * SLOT);
  st.issued = XU(st.issued + 1);
  st.islot = ring_next(st.islot);
  unit_advance(a, st, pr.tab);
}
// the consumer is through with block `consumed` (its reads of the slot have retired before the slot is re-staged): the next block goes out
__device__ __forceinline__ void ring_consumed(const XArgs& a, XStream& st, const XLane& lv, const XProd& pr) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  st.consumed = XU(st.consumed + 1);
  st.cslot = ring_next(st.cslot);
  ring_issue(a, st, lv, pr);
}
// block `consumed` has landed: at most (issued - consumed - 1) younger blocks may still be in flight (loads return in order)
__device__ __forceinline__ void ring_wait(const XStream& st) {
  const int younger = XU(st.issued - st.consumed - 1);
  if (younger >= 5) XWAIT_VM(20);
  else if (younger == 4) XWAIT_VM(16);
  else if (younger == 3) XWAIT_VM(12);
  else if (younger == 2) XWAIT_VM(8);
  else if (younger == 1) XWAIT_VM(4);
  else XWAIT_VM(0);
}

// ---- team barrier (helper wave) ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void team_arrive(unsigned* ctrl) {
  XWAIT_VM(0);  // this workgroup's stores of the phase have been acknowledged
  if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(ctrl + dec::KV_TEAM_COUNTER, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void team_wait(unsigned* ctrl, unsigned target, int flags = 0) {
  if ((threadIdx.x & 63) == 0) {  // one lane polls; the wave reconverges behind it
    unsigned spins = 0;
    while ((int)(__hip_atomic_load(ctrl + dec::KV_TEAM_COUNTER, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) < 0) {
      if (!(flags & dec::XF_NO_SLEEP)) __builtin_amdgcn_s_sleep(1);
      if (++spins > SPIN_LIMIT || ((spins & 63) == 0 && __hip_atomic_load(ctrl + dec::KV_ERROR, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
        __hip_atomic_fetch_or(ctrl + dec::KV_ERROR, dec::KV_ERR_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // a team member never arrived: poison, do not hang
        break;
      }
    }
  }
}

// ---- fast run: `run` consecutive ring blocks during which nothing special happens on either side -- the consumer's blocks are full, the
// producer stays inside its current unit (st.left full blocks with one descriptor / lane-offset set) and the ring is in its steady state
// (XR blocks in flight: the block consumed and the block issued share a slot).  Per block: one counted wait, the consumer's body on the
// slot, four DMA instructions, a handful of scalar updates -- no cursor arithmetic (the general path costs ~1.7 k cycles of
// instruction issue per block, profiles/r05_decode_xcd_stamps_v3_instruction_bound.txt).
__device__ __forceinline__ int fast_run_len(const XStream& st, int consumer_full_left) {
  return (consumer_full_left > 0 && st.more && st.issued - st.consumed == XR) ? consumer_full_left : 0;
}
template <typename F>
__device__ __forceinline__ void fast_run(const XArgs& a, XStream& st, const XLane& lv, const XProd& pr, char* smem, int wave, int run, F&& body) {
  int i = 0;
  for (; i < run && st.more; ++i) {
    XWAIT_VM(20);  // 4 * (XR - 1): the oldest block in flight has landed
    body(smem + XL_RING + (wave * XR + st.cslot) * SLOT, i);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the body's reads of the slot have retired: it may be re-staged
    issue_block(st, lv, pr.rs_w, pr.rs_kv, pr.ring_lds + (unsigned)st.cslot * SLOT);  // (steady state: islot == cslot)
    st.cslot = ring_next(st.cslot);
    unit_advance(a, st, pr.tab);
  }
  st.islot = st.cslot;
  st.issued = XU(st.issued + i), st.consumed = XU(st.consumed + i);
  // the producer ran dry inside the run (the step's last blocks): the rest of the run is consumed without issuing
  for (; i < run; ++i) {
    ring_wait(st);
    body(smem + XL_RING + (wave * XR + st.cslot) * SLOT, i);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    st.consumed = XU(st.consumed + 1);
    st.cslot = ring_next(st.cslot);
  }
}

}  // namespace
