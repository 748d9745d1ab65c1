// One-launch KV-cached decoder step for a handful of sequences (B <= 4) on ONE XCD, gfx950 (round 5; since round 6 the default for one sequence is
// the chip-wide engine of decode_wide.hip, and this team engine runs where it is forced -- oasr_decode_set_ln_fold(2..4) -- or where that one does not apply)
// -- TextDecoder.forward for one new token per sequence, olmoasr/model.py:786-817 with the kv_cache hooks of :925-964
// (inference twin: olmoasr/inf_model.py:150-196, 320-362).
//
// Why: the multi-launch step (engine_decode.hip::oasr_decode_step_impl) is ~8 dependent launches per layer, each a 4.7 us dispatch floor plus a
// chain of dependent memory round trips (weights that must first miss to HBM, a reduction, a store): 2.4 ms per token at medium = 0.05
// of the HBM roof (profiles/r02_decode_step.txt, r03_decode_xcd.txt).  What those measurements asked for is built here:
//   * ONE persistent launch; the `team` workgroups (one per CU, by default the 32 CUs of ONE XCD: blockIdx % 8 == 0) walk the 8 phases
//     of every layer and meet at a team barrier (relaxed agent-scope counter, 1.2 us inside an XCD against 4.7 us per launch and 12 us for
//     a device-wide release/acquire barrier);
//   * everything that does NOT depend on the token -- the weight tiles and the cross-attention K/V a workgroup will consume -- is a STATIC
//     per-wave stream that runs AHEAD of the phases through a wave-private LDS ring (buffer_load ... lds issued from inline assembly, one
//     counted vmcnt per block, never drained): while a workgroup waits at a barrier its next XR blocks are already landing, so a phase
//     costs one round trip on the activations instead of five;
//   * a fifth "helper" wave per workgroup owns everything that is NOT streaming: the barrier, the activation rows (LayerNorm folded into the
//     operand exactly like decode_proj.hip), the K-split reduction + epilogue and the stores -- the four streaming waves issue no other
//     vector-memory instruction, so their vmcnt counts ring blocks only.
// Data crosses workgroups ONLY through agent-scope (sc1) atomic loads / stores, so results do not depend on where the team's workgroups
// land; the XCD placement is a speed matter (recorded in the control word KV_XCC_MASK).  Arithmetic is decode_shared.h's: bit-identical to the multi-launch step.
#include "decode_xcd_ring.h"

namespace {

constexpr int XHG = 8;        // heads merged per batch of partial loads

// dynamic LDS block, byte offsets (compile-time: d <= XMAXD fixes the operand row stride)
constexpr unsigned XL_XS = 4 * XMAXD * 2 + 16;  // row stride of the activation operand: K_max = 4d, + 16 so the rows sit on different banks
constexpr unsigned XL_XBUF = XL_RING + 4 * XR * SLOT;
constexpr unsigned XL_RED = XL_XBUF + XMAXM * XL_XS;
constexpr unsigned XL_SC = XL_RED + 4 * 4 * 16 * XMAXM * 2 * 4;  // NRED reduction buffers
constexpr unsigned XL_ARED = XL_SC + dec::SEG_KEYS * 4;  // (sc | ared contiguous: the cross-attention merge stages the partials there)
constexpr unsigned XL_LSUM = XL_ARED + 32 * 64 * 4;
constexpr unsigned XL_WMAX = XL_LSUM + 32 * 4;
constexpr unsigned XL_AOUT = XL_WMAX + 4 * 4;
constexpr unsigned XL_TAB = (XL_AOUT + 66 * 4 + 8 + 15) & ~15u;  // 4 waves x XTABN units x 16 bytes
constexpr unsigned XL_TOTAL = XL_TAB + 4 * XTABN * 16;
static_assert(XL_TOTAL <= 160 * 1024, "one-launch decode step: LDS budget");

struct XGemv {  // one projection phase
  int seg;
  const bf16_t* xin;    // activation rows [M][K] (global)
  int K, N;
  const float *ln_g, *ln_b;  // LayerNorm folded into the operand, or null
  bool merge_attn;      // the operand is the merged cross-attention output (a.part), not xin
  const float* bias;
  bool gelu;
  const bf16_t* resid;  // [M][d] or null
  bf16_t* out;
  long ldc;
};

// helper wave: activation rows of a projection phase -> LDS operand rows (bf16).  Every global load of a row is issued before the first
// one is used: ONE round trip per row, not one per chunk.
constexpr int XCH = 4;  // 16-byte chunks per lane and batch of a plain operand row (register budget: the kernel sits at 254 of 256 VGPRs)
__device__ __forceinline__ void helper_operand(const XArgs& a, const XGeom& g, const XGemv& ph, char* smem, int lane) {
  if (ph.merge_attn) {  // rows = merge of the cross-attention segments' partials (decode_shared.h), dimension `lane` of every head
    // ONE round trip per row: lane j < H * ns fetches (m, l) of pair j, every lane its dimension of every pair's o; the (m, l) of a pair
    // reach all lanes by a wave shuffle
    const int npair = a.H * g.ns;  // <= 40 (decode_xcd_supports)
    for (int b = 0; b < a.M; ++b) {
      const float* src = a.part + (long)b * npair * 66;
      const int jl = lane < npair ? lane : npair - 1;
      const float m_l = ldf_agent(src + jl * 66), l_l = ldf_agent(src + jl * 66 + 1);
      for (int h0 = 0; h0 < a.H; h0 += XHG) {  // XHG heads per batch of loads (register budget)
        float o[XHG * dec::MAX_SEG];
#pragma unroll
        for (int j = 0; j < XHG * dec::MAX_SEG; ++j) {
          const int pj = h0 * g.ns + j;
          o[j] = ldf_agent(src + (pj < npair ? pj : npair - 1) * 66 + 2 + lane);  // (unconditional: one batch of loads)
        }
#pragma unroll
        for (int hh = 0; hh < XHG; ++hh) {
          const int h = h0 + hh;
          if (h < a.H) {
            float m_s[dec::MAX_SEG] = {dec::NEG, dec::NEG}, l_s[dec::MAX_SEG] = {0.f, 0.f}, o_s[dec::MAX_SEG] = {0.f, 0.f};
            // (m, l) of a pair sit in lane `pair` of m_l / l_l: v_readlane (a scalar broadcast), not a ds_bpermute round trip
            if (g.ns == 2) {
              m_s[0] = rdlane(m_l, 2 * h), m_s[1] = rdlane(m_l, 2 * h + 1);
              l_s[0] = rdlane(l_l, 2 * h), l_s[1] = rdlane(l_l, 2 * h + 1);
              o_s[0] = o[2 * hh], o_s[1] = o[2 * hh + 1];
            } else {
              m_s[0] = rdlane(m_l, h), l_s[0] = rdlane(l_l, h), o_s[0] = o[hh];
            }
            float m, lt;
            const float val = dec::merge_segments(m_s, l_s, o_s, g.ns, m, lt);
            const float nb = dec::xor_lane<1>(val);
            if ((lane & 1) == 0) *(uint32_t*)(smem + XL_XBUF + b * XL_XS + (h * 64 + lane) * 2) = pack_bf2(val, nb);
          }
        }
      }
    }
    return;
  }
  const int nchunk = ph.K >> 3;
  for (int b = 0; b < a.M; ++b) {
    if (ph.ln_g) {  // K == d <= 2048: the row fits MAXC chunks per lane
      u32x4_t raw[dec::MAXC];
#pragma unroll
      for (int c = 0; c < dec::MAXC; ++c) {
        const int ch = lane + 64 * c;
        if (ch < nchunk) raw[c] = ld16_agent(ph.xin + (long)b * ph.K + ch * 8);
      }
      float mean, rstd;
      dec::row_stats(raw, lane, nchunk, ph.K, mean, rstd);
#pragma unroll
      for (int c = 0; c < dec::MAXC; ++c) {
        const int ch = lane + 64 * c;
        if (ch < nchunk) *(u32x4_t*)(smem + XL_XBUF + b * XL_XS + ch * 16) = dec::ln_apply8(raw[c], mean, rstd, ph.ln_g, ph.ln_b, ch * 8);
      }
    } else {
      for (int c0 = 0; c0 * 64 < nchunk; c0 += XCH) {  // (K = 4096: two batches)
        u32x4_t raw[XCH];
#pragma unroll
        for (int c = 0; c < XCH; ++c)
          if (lane + 64 * (c0 + c) < nchunk) raw[c] = ld16_agent(ph.xin + (long)b * ph.K + (lane + 64 * (c0 + c)) * 8);
#pragma unroll
        for (int c = 0; c < XCH; ++c)
          if (lane + 64 * (c0 + c) < nchunk) *(u32x4_t*)(smem + XL_XBUF + b * XL_XS + (lane + 64 * (c0 + c)) * 16) = raw[c];
      }
    }
  }
}
// helper wave: query rows of an attention phase -> LDS
__device__ __forceinline__ void helper_query_rows(const XArgs& a, const bf16_t* src, long row_stride, char* smem, int lane) {
  const int nchunk = a.d >> 3;
  for (int b = 0; b < a.M; ++b) {
    u32x4_t raw[dec::MAXC];
#pragma unroll
    for (int c = 0; c < dec::MAXC; ++c)
      if (lane + 64 * c < nchunk) raw[c] = ld16_agent(src + (long)b * row_stride + (lane + 64 * c) * 8);
#pragma unroll
    for (int c = 0; c < dec::MAXC; ++c)
      if (lane + 64 * c < nchunk) *(u32x4_t*)(smem + XL_XBUF + b * XL_XS + (lane + 64 * c) * 16) = raw[c];
  }
}

// helper wave: K-split reduction + epilogue + store of one 32-column tile (lane: row m = lane >> 4, columns 2 (lane & 15), + 1).
// The residual pair and the two biases do not depend on the tile's accumulators: they are requested BEFORE the workgroup barrier that
// releases the accumulators (helper_epilogue_inputs), so the epilogue itself is LDS reads + one store.
struct XEpiIn {
  unsigned rz;
  float b0, b1;
};
__device__ __forceinline__ XEpiIn helper_epilogue_inputs(const XArgs& a, const XGemv& ph, int n0, int lane) {
  const int m = lane >> 4, cp = lane & 15;
  XEpiIn in{0u, 0.f, 0.f};
  if (m >= a.M) return in;
  if (ph.resid) in.rz = __hip_atomic_load((const unsigned*)(ph.resid + (long)m * a.d + n0 + 2 * cp), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (ph.bias) in.b0 = ph.bias[n0 + 2 * cp], in.b1 = ph.bias[n0 + 2 * cp + 1];
  return in;
}
__device__ __forceinline__ void helper_epilogue(const XArgs& a, const XGemv& ph, const XEpiIn& in, const char* smem, int buf, int n0,
                                                int lane) {
  const int m = lane >> 4, cp = lane & 15;
  if (m >= a.M) return;
  const float* red = (const float*)(smem + XL_RED) + buf * (4 * 16 * XMAXM * 2);
  float y[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int c = 2 * cp + e;
    const int r = (c >> 3) * 4 + (c & 3), h = (c >> 2) & 1;
    const int idx = (r * XMAXM + m) * 2 + h;
    const float acc = red[0 * 16 * XMAXM * 2 + idx] + red[1 * 16 * XMAXM * 2 + idx] + red[2 * 16 * XMAXM * 2 + idx] + red[3 * 16 * XMAXM * 2 + idx];
    y[e] = dec::epi_value(acc, e ? in.b1 : in.b0, ph.gelu, ph.resid != nullptr, e ? bf_hi(in.rz) : bf_lo(in.rz));
  }
  st4_x(ph.out + (long)m * ph.ldc + n0 + 2 * cp, pack_bf2(y[0], y[1]), a.flags);
}

// streaming waves: the tiles of one projection phase, back to back.  A tile = this wave's K quarter of 32 weight rows against the operand
// rows, through the ring; its 16 accumulators go to one of NRED reduction buffers.  The helper wave is met once per GROUP of NRED tiles
// (every phase of every model up to d = 1024 is one group), not once per tile.
constexpr int NRED = 4;
template <bool DBG>
__device__ __forceinline__ void stream_phase(const XArgs& a, const XGeom& g, XStream& st, XCur& cc, const XLane& lv, const XProd& pr, const XGemv& ph,
                                             char* smem, int wave, int lane, int ntile) {
  const int nst = ph.seg == 6 ? g.nst_4d : g.nst_d, nkb = ph.seg == 6 ? g.nkb_4d : g.nkb_d;
  const bool allfull = (nst & 3) == 0;
  const int row = lane & 31, kc = lane >> 5;
  const int kq0 = wave * (ph.K >> 2);
  const char* xrow = smem + XL_XBUF + (row & (XMAXM - 1)) * XL_XS + (kq0 + kc * 8) * 2;
  f32x16_t acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  int tile = 0, kb = 0;
  auto tile_done = [&]() {  // accumulators -> reduction buffer (tile & (NRED - 1)); next tile
    if (row < XMAXM) {
      float* red = (float*)(smem + XL_RED) + (tile & (NRED - 1)) * (4 * 16 * XMAXM * 2) + wave * (16 * XMAXM * 2);
#pragma unroll
      for (int r = 0; r < 16; ++r) red[(r * XMAXM + row) * 2 + kc] = acc[r];
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    kb = 0;
    ++tile;
  };
  while (tile < ntile) {
    int gend = (tile & ~(NRED - 1)) + NRED;  // end of this group of tiles
    gend = gend < ntile ? gend : ntile;
    const int cfull = allfull ? (gend - tile) * nkb - kb : (nst >> 2) - kb;  // full blocks ahead of the consumer before anything special
    const int run = DBG ? 0 : fast_run_len(st, cfull);
    if (run > 0) {
      fast_run(a, st, lv, pr, smem, wave, run, [&](const char* slot, int) {
        bf16x8_t wf[4], xf[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          wf[q] = *(const bf16x8_t*)(slot + lv.frag[q]);
          xf[q] = *(const bf16x8_t*)(xrow + kb * 128 + q * 32);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[q], xf[q], acc, 0, 0, 0);
        if (++kb == nkb) tile_done();
      });
    } else {
      if (DBG) {
        if (cc.seg != ph.seg || cc.idx != tile || cc.sub != kb) __hip_atomic_fetch_or(a.ctrl + dec::KV_ERROR, dec::KV_ERR_STREAM | (unsigned)ph.seg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        cur_advance(g, cc);
      }
      ring_wait(st);
      const char* slot = smem + XL_RING + (wave * XR + st.cslot) * SLOT;
      int steps = nst - kb * 4;
      steps = steps > 4 ? 4 : steps;
      for (int q = 0; q < steps; ++q) {
        const bf16x8_t wf = *(const bf16x8_t*)(slot + row * 128 + (((2 * q + kc) ^ ((row >> 1) & 7)) << 4));
        const bf16x8_t xf = *(const bf16x8_t*)(xrow + (kb * 4 + q) * 32);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, xf, acc, 0, 0, 0);
      }
      ring_consumed(a, st, lv, pr);
      if (++kb == nkb) tile_done();
    }
    if (kb == 0 && (tile == ntile || (tile & (NRED - 1)) == 0)) {  // a group is complete: hand its accumulators to the helper wave
      XBAR();
      if (tile < ntile) XBAR();  // ... and wait until it has read them before the next group overwrites the buffers
    }
  }
}

__device__ __forceinline__ XGemv gemv_of(const XArgs& a, int layer, int ph) {
  const DecLayerOffsets ly = dec::layer_at(a.l0, layer, a.lstride, a.astride);
  bf16_t* self = a.cache + (long)layer * a.cache_lstride;
  XGemv p;
  p.merge_attn = false, p.gelu = false, p.ln_g = p.ln_b = nullptr, p.resid = nullptr, p.K = a.d, p.N = a.d, p.ldc = a.d;
  switch (ph) {
    case 0:  // attn_ln -> q | k | v of position pos, straight into the cache row
      p.seg = 0, p.xin = a.x, p.N = 3 * a.d, p.ln_g = a.params + ly.ln1g, p.ln_b = a.params + ly.ln1b, p.bias = a.aux + ly.bqkv_aux;
      p.out = self + (long)a.pos * 3 * a.d, p.ldc = (long)a.S_max * 3 * a.d;
      break;
    case 2:  // self-attention output projection + residual
      p.seg = 1, p.xin = a.o, p.bias = a.params + ly.bo, p.resid = a.x, p.out = a.x2;
      break;
    case 3:  // cross_attn_ln -> cross query
      p.seg = 2, p.xin = a.x2, p.ln_g = a.params + ly.lncg, p.ln_b = a.params + ly.lncb, p.bias = a.params + ly.bcq, p.out = a.q;
      break;
    case 5:  // cross-attention output projection + residual (operand = merged segment partials)
      p.seg = 4, p.xin = nullptr, p.merge_attn = true, p.bias = a.params + ly.bco, p.resid = a.x2, p.out = a.x3;
      break;
    case 6:  // mlp_ln -> mlp.0 + GELU
      p.seg = 5, p.xin = a.x3, p.N = 4 * a.d, p.ln_g = a.params + ly.ln2g, p.ln_b = a.params + ly.ln2b, p.bias = a.params + ly.b1, p.gelu = true;
      p.out = a.hg, p.ldc = 4 * a.d;
      break;
    default:  // 7: mlp.2 + residual
      p.seg = 6, p.xin = a.hg, p.K = 4 * a.d, p.bias = a.params + ly.b2, p.resid = a.x3, p.out = a.x;
      break;
  }
  return p;
}
// measurement: s_memtime of workgroup 0's helper wave (slots 0-4: phase start, barrier passed, operand / query rows in LDS, last tile stored,
// arrived) and of its streaming wave 0 (5, 6: released, last tile handed over) in decoder layer 1
#define XSTAMP(K)                                                                                          \
  do {                                                                                                     \
    if (a.stamps && wg == 0 && layer == 1 && lane == 0) a.stamps[ph * 8 + (K)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
template <bool DBG>  // DBG: the consumer checks every block against a mirror of the producer's cursor (tests; costs scalar work per block)
__global__ __launch_bounds__(320) void decode_xcd_kernel(XArgs a) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  if (a.stride == 8 && (blockIdx.x & 7) != 0) return;
  const int wg = a.stride == 8 ? (int)(blockIdx.x >> 3) : (int)blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool helper = wave == 4;
  XGeom g = make_geom(a.d, a.H, a.Te, a.M, a.L, a.team, wg);
  g.cnt_qkv = __builtin_amdgcn_readfirstlane(g.cnt_qkv), g.cnt_d = __builtin_amdgcn_readfirstlane(g.cnt_d);
  g.cnt_4d = __builtin_amdgcn_readfirstlane(g.cnt_4d), g.cnt_it = __builtin_amdgcn_readfirstlane(g.cnt_it);
  const unsigned base = a.ctrl[dec::KV_TEAM_EPOCH];  // epoch: the counter is never reset, every launch adds (phases x team) to it
  const unsigned ring_lds = (unsigned)(size_t)(smem + XL_RING) + (unsigned)wave * XR * SLOT;
  unsigned gphase = 0;  // phases completed by the whole team before the current one
  const XLane lv = make_lane(a.d, a.Te, wave, lane);

  XStream st;
  XCur cc;  // consumer's mirror of the block sequence (checked instantiation: a desynchronised producer is reported, not silently consumed)
  st.issued = st.consumed = 0, st.islot = st.cslot = 0;
  st.u = 0, st.nunits = 0, st.layer = 0, st.soff = 0, st.jump = 0, st.left = 0, st.kind = 0, st.tleft = st.tnkb = 0x400000;
  cc = XCur{0, 0, 0, 0};
  XProd pr;
  pr.tab = (const unsigned*)(smem + XL_TAB) + (wave & 3) * (XTABN * 4);
  pr.ring_lds = ring_lds;
  pr.rs_w = rsrc_of(a.wflat);
  pr.rs_kv = rsrc_of(a.cache + (long)3 * a.M * a.S_max * a.d);
  if (!helper) {
    {
      XBuild bp;
      bp.d = a.d, bp.H = a.H, bp.Te = a.Te, bp.M = a.M, bp.L = a.L, bp.team = a.team, bp.wg = wg;
      bp.w[0] = a.l0.wqkv, bp.w[1] = a.l0.wo, bp.w[2] = a.l0.wcq, bp.w[3] = a.l0.wco, bp.w[4] = a.l0.w1, bp.w[5] = a.l0.w2;
      st.nunits = XU(build_units(bp, wave, lane, (unsigned*)(smem + XL_TAB) + wave * (XTABN * 4)));
    }
    st.more = st.nunits > 0 && st.nunits < XTABN;  // (a full table means the walk was cut short: never the case for a supported shape)
    if (st.nunits >= XTABN && lane == 0) __hip_atomic_fetch_or(a.ctrl + dec::KV_ERROR, dec::KV_ERR_TABLE_FULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (st.more) unit_load(a, st, pr.tab);
    cur_normalise(g, cc);
    for (int i = 0; i < XR; ++i) ring_issue(a, st, lv, pr);
  } else {
    st.more = false;
    if (lane == 0) {
      unsigned xcc;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
      __hip_atomic_fetch_or(a.ctrl + dec::KV_XCC_MASK, 1u << (xcc & 15), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (int i = lane; i < (int)(XMAXM * XL_XS / 4); i += 64) ((unsigned*)(smem + XL_XBUF))[i] = 0u;  // operand rows >= M read as zeros
  }

#pragma unroll 1
  for (int layer = 0; layer < a.L; ++layer) {
#pragma unroll 1
    for (int ph = 0; ph < 8; ++ph, ++gphase) {
      const unsigned target = base + gphase * (unsigned)a.team;
      if (ph == 1 || ph == 4) {
        // ---------------- attention: items (b, h[, key segment]) of this workgroup ----------------
        const bool cross = ph == 4;
        const int nitem = cross ? g.cnt_it : cnt_of(a.M * a.H, wg, a.team);
        const bf16_t* self = a.cache + (long)layer * a.cache_lstride;
        if (helper) {
          XSTAMP(0);
          team_wait(a.ctrl, target, a.flags);
          XSTAMP(1);
          // query rows -> LDS (self: the q third of cache row pos; cross: the cross query)
          if (cross) helper_query_rows(a, a.q, a.d, smem, lane);
          else helper_query_rows(a, self + (long)a.pos * 3 * a.d, (long)a.S_max * 3 * a.d, smem, lane);
          XSTAMP(2);
          XBAR();  // A
          for (int j = 0; j < nitem; ++j) {
            XBAR();  // 1
            XBAR();  // 2
            XBAR();  // 3: the item's result is in XL_AOUT
            const float* ao = (const float*)(smem + XL_AOUT);
            if (cross) {
              const XItem it = item_of(g, j);
              float* dst = a.part + ((long)(it.b * a.H + it.h) * g.ns + it.sg) * 66;
              st4_x(dst + 2 + lane, __float_as_uint(ao[2 + lane]), a.flags);
              if (lane < 2) st4_x(dst + lane, __float_as_uint(ao[lane]), a.flags);
            } else {
              const int id = wg + a.team * j, b = (id >= a.H ? 1 : 0) + (id >= 2 * a.H ? 1 : 0) + (id >= 3 * a.H ? 1 : 0), h = id - b * a.H;
              const float val = ao[2 + lane], nb = dec::xor_lane<1>(val);
              if ((lane & 1) == 0) st4_x(a.o + (long)b * a.d + h * 64 + lane, pack_bf2(val, nb), a.flags);
            }
          }
          XSTAMP(3);
          team_arrive(a.ctrl);
          XSTAMP(4);
        } else {
          XBAR();  // A
          float* sc = (float*)(smem + XL_SC);
          float(*ared)[64] = (float(*)[64])(smem + XL_ARED);
          float* lsum = (float*)(smem + XL_LSUM);
          float* wmax = (float*)(smem + XL_WMAX);
          float* ao = (float*)(smem + XL_AOUT);
          const int l8 = tid & 7, grp = tid >> 3;
          for (int j = 0; j < nitem; ++j) {
            int b, h, n;
            XItem it;
            if (cross) {
              it = item_of(g, j);
              b = it.b, h = it.h, n = it.n;
            } else {
              const int id = wg + a.team * j;
              b = (id >= a.H ? 1 : 0) + (id >= 2 * a.H ? 1 : 0) + (id >= 3 * a.H ? 1 : 0), h = id - b * a.H, n = a.pos + 1;
            }
            float qv[8];
            dec::load_q8(*(const u32x4_t*)(smem + XL_XBUF + b * XL_XS + (h * 64 + l8 * 8) * 2), qv);
            float mx = dec::NEG, l = 0.f, o[8];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) o[jj] = 0.f;
            if (cross) {
              // K blocks, then V blocks, of this wave's keys (t == 8 wave + (lane >> 3) mod 32) through the ring
              for (int kb = 0; kb < it.kvb;) {
                const int run = DBG ? 0 : fast_run_len(st, (n >> 7) - kb);  // blocks whose 128 keys all lie inside the segment
                if (run > 0) {
                  fast_run(a, st, lv, pr, smem, wave, run, [&](const char* slot, int i) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                      const int t = 32 * ((kb + i) * 4 + q) + grp;
                      const float s2 = dec::score8(qv, *(const u32x4_t*)(slot + q * 1024 + lane * 16));
                      if (l8 == 0) sc[t] = s2;
                      mx = fmaxf(mx, s2);
                    }
                  });
                  kb += run;
                  continue;
                }
                if (DBG) {
                  if (cc.seg != 3 || cc.idx != j || cc.sub != kb) __hip_atomic_fetch_or(a.ctrl + dec::KV_ERROR, dec::KV_ERR_STREAM_K, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                  cur_advance(g, cc);
                }
                ring_wait(st);
                const char* slot = smem + XL_RING + (wave * XR + st.cslot) * SLOT;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                  const int t = 32 * (kb * 4 + q) + grp;
                  const float s2 = dec::score8(qv, *(const u32x4_t*)(slot + q * 1024 + lane * 16));
                  if (t < n) {
                    if (l8 == 0) sc[t] = s2;
                    mx = fmaxf(mx, s2);
                  }
                }
                ring_consumed(a, st, lv, pr);
                ++kb;
              }
            } else {
              // self-attention: <= S_max cached keys, q | k | v rows of this sequence (agent-scope: row pos was written in this launch)
              const bf16_t* kp = self + (long)b * a.S_max * 3 * a.d + a.d + h * 64 + l8 * 8;
              for (int t0 = grp; t0 < n; t0 += 32 * 8) {
                u32x4_t k4[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                  const int t = t0 + 32 * u;
                  k4[u] = ld16_agent(kp + (long)(t < n ? t : n - 1) * 3 * a.d);
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
            }
            mx = wave_max(mx);
            if (lane == 0) wmax[wave] = mx;
            XBAR();  // 1
            const float m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
            if (cross) {
              for (int kb = 0; kb < it.kvb;) {
                const int run = DBG ? 0 : fast_run_len(st, (n >> 7) - kb);
                if (run > 0) {
                  fast_run(a, st, lv, pr, smem, wave, run, [&](const char* slot, int i) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                      const int t = 32 * ((kb + i) * 4 + q) + grp;
                      dec::accum_pv(__builtin_amdgcn_exp2f(sc[t] - m), *(const u32x4_t*)(slot + q * 1024 + lane * 16), l, o);
                    }
                  });
                  kb += run;
                  continue;
                }
                if (DBG) {
                  if (cc.seg != 3 || cc.idx != j || cc.sub != it.kvb + kb) __hip_atomic_fetch_or(a.ctrl + dec::KV_ERROR, dec::KV_ERR_STREAM_V, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                  cur_advance(g, cc);
                }
                ring_wait(st);
                const char* slot = smem + XL_RING + (wave * XR + st.cslot) * SLOT;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                  const int t = 32 * (kb * 4 + q) + grp;
                  dec::accum_pv(t < n ? __builtin_amdgcn_exp2f(sc[t] - m) : 0.f, *(const u32x4_t*)(slot + q * 1024 + lane * 16), l, o);
                }
                ring_consumed(a, st, lv, pr);
                ++kb;
              }
            } else {
              const bf16_t* vp = self + (long)b * a.S_max * 3 * a.d + 2 * a.d + h * 64 + l8 * 8;
              for (int t0 = grp; t0 < n; t0 += 32 * 8) {
                u32x4_t v4[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                  const int t = t0 + 32 * u;
                  v4[u] = ld16_agent(vp + (long)(t < n ? t : n - 1) * 3 * a.d);
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                  const int t = t0 + 32 * u;
                  dec::accum_pv(t < n ? __builtin_amdgcn_exp2f(sc[t] - m) : 0.f, v4[u], l, o);
                }
              }
            }
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) ared[grp][l8 * 8 + jj] = o[jj];
            if (l8 == 0) lsum[grp] = l;
            XBAR();  // 2
            if (tid < 64) {
              float acc, lt;
              dec::reduce_groups(ared, lsum, tid, acc, lt);
              if (cross) {  // the segment's partial, merged by the consumer phase
                ao[2 + tid] = acc;
                if (tid == 0) ao[0] = m, ao[1] = lt;
              } else {
                float m_s[dec::MAX_SEG] = {m, dec::NEG}, l_s[dec::MAX_SEG] = {lt, 0.f}, o_s[dec::MAX_SEG] = {acc, 0.f};
                float mo, lo;
                ao[2 + tid] = dec::merge_segments(m_s, l_s, o_s, 1, mo, lo);
              }
            }
            XBAR();  // 3
          }
        }
      } else {
        // ---------------- projection: tiles t = wg, wg + team, ... ----------------
        const XGemv p = gemv_of(a, layer, ph);
        const int ntile = seg_cnt(g, p.seg);
        if (helper) {
          XSTAMP(0);
          team_wait(a.ctrl, target, a.flags);
          XSTAMP(1);
          if (ntile > 0) helper_operand(a, g, p, smem, lane);
          XSTAMP(2);
          XBAR();  // A: operand rows ready
          for (int i0 = 0; i0 < ntile; i0 += NRED) {  // groups of NRED tiles (stream_phase)
            const int i1 = i0 + NRED < ntile ? i0 + NRED : ntile;
            XEpiIn in[NRED];
#pragma unroll
            for (int k = 0; k < NRED; ++k)
              if (i0 + k < i1) in[k] = helper_epilogue_inputs(a, p, (wg + a.team * (i0 + k)) * 32, lane);
            XBAR();  // B: the group's accumulators are in the reduction buffers
#pragma unroll
            for (int k = 0; k < NRED; ++k)
              if (i0 + k < i1) helper_epilogue(a, p, in[k], smem, k, (wg + a.team * (i0 + k)) * 32, lane);
            if (i1 < ntile) XBAR();  // buffers free again
          }
          XSTAMP(3);
          team_arrive(a.ctrl);
          XSTAMP(4);
        } else {
          XBAR();  // A
          if (wave == 0) XSTAMP(5);
          stream_phase<DBG>(a, g, st, cc, lv, pr, p, smem, wave, lane, ntile);
          if (wave == 0) XSTAMP(6);
        }
      }
    }
  }
  if (helper) {
    if (wg == 0) {  // everybody has read the epoch base long ago; publish the next launch's once the whole team is through
      team_wait(a.ctrl, base + gphase * (unsigned)a.team);
      if (lane == 0) a.ctrl[dec::KV_TEAM_EPOCH] = base + gphase * (unsigned)a.team;
    }
  }
}

}  // namespace

// (which shapes and layouts the engine takes: decode_plan_host.cpp)
int launch_decode_xcd(const DecodeStepArgs& h, hipStream_t s) {
  OASR_REQUIRE(decode_xcd_supports(h.d, h.H, h.Te, h.S_max, h.L, h.M), "decode_xcd: unsupported shape (d=%d H=%d Te=%d S=%d L=%d M=%d)", h.d, h.H,
               h.Te, h.S_max, h.L, h.M);
  OASR_REQUIRE(h.team >= 1 && h.team <= 256 && (h.stride == 1 || h.stride == 8) && h.pos >= 0 && h.pos < h.S_max, "decode_xcd: bad launch shape");
  OASR_REQUIRE(decode_xcd_offsets_ok(h.l0, h.lstride, h.cache_lstride, h.d, h.Te, h.L, h.M),
               "decode_xcd: a weight / cross K/V byte offset reaches 2 GiB (32-bit buffer offsets); use the multi-launch step");
  XArgs a;
  static_cast<DecodeStepBufs&>(a) = h;
  a.d = h.d, a.H = h.H, a.Te = h.Te, a.S_max = h.S_max, a.L = h.L, a.M = h.M, a.pos = h.pos, a.team = h.team, a.stride = h.stride;
  a.flags = h.flags, a.stamps = (unsigned long long*)h.stamps;
  a.l0 = h.l0, a.lstride = h.lstride, a.astride = h.astride;
  const unsigned lds = XL_TOTAL;
  static LdsAttrOnce attr;
  static LdsAttrOnce attr_dbg;
  if (h.flags & dec::XF_CHECKED) {  // checked instantiation (tests)
    { const int rc_ = ensure_dynamic_lds(attr_dbg, (const void*)decode_xcd_kernel<true>, (int)lds); if (rc_) return rc_; }
    hipLaunchKernelGGL(decode_xcd_kernel<true>, dim3(h.team * h.stride), dim3(320), lds, s, a);
  } else {
    { const int rc_ = ensure_dynamic_lds(attr, (const void*)decode_xcd_kernel<false>, (int)lds); if (rc_) return rc_; }
    hipLaunchKernelGGL(decode_xcd_kernel<false>, dim3(h.team * h.stride), dim3(320), lds, s, a);
  }
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}
