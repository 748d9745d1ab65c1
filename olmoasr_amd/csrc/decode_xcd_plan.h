// The one-XCD step engine's plan (decode_xcd.hip): the static block sequence every streaming wave prefetches, as integer arithmetic the kernel
// and the host share -- the kernel walks these cursors, decode_plan_host.cpp exposes the same walk to the CPU suite (oasr_xcd_plan_debug) -- and
// the host's predicates for the shapes and layouts the engine takes.  Plain C++: no HIP header is needed to include this file.
#pragma once
#include "decode_step_core.h"

constexpr int XMAXM = 4;      // sequences this engine takes
constexpr int XMAXL = 32;     // decoder layers
constexpr int XMAXD = 1280;   // (fixes the operand row stride of the kernel's LDS block)
constexpr int NSEG = 7;       // streamed segments per layer (the self-attention phase streams nothing)
constexpr int XMAXPAIR = 40;  // (head, key segment) pairs of one sequence: H * ns <= 40 (d <= 1280)

// ---- the static block sequence of one workgroup (identical for its four streaming waves) ---------------------------------------------
struct XGeom {
  int d, H, Te, M, team, wg, L, ns;
  int nst_d, nst_4d;  // k16 steps per wave and tile for K = d / 4d
  int nkb_d, nkb_4d;  // ring blocks per wave and tile
  int cnt_qkv, cnt_d, cnt_4d, cnt_it;  // tiles of this workgroup in a phase of 3d/32, d/32, 4d/32 tiles; cross-attention items
};
OASR_HD int cnt_of(int n, int wg, int team) {  // tiles t = wg, wg + team, ... < n (a short loop instead of a division)
  int c = 0;
  for (int t = wg; t < n; t += team) ++c;
  return c;
}
OASR_HD XGeom make_geom(int d, int H, int Te, int M, int L, int team, int wg) {
  XGeom g;
  g.d = d, g.H = H, g.Te = Te, g.M = M, g.team = team, g.wg = wg, g.L = L;
  g.ns = Te > dec::SEG_KEYS ? 2 : 1;
  g.nst_d = d >> 6, g.nst_4d = d >> 4;
  g.nkb_d = (g.nst_d + 3) >> 2, g.nkb_4d = (g.nst_4d + 3) >> 2;
  g.cnt_qkv = cnt_of((3 * d) >> 5, wg, team);
  g.cnt_d = cnt_of(d >> 5, wg, team);
  g.cnt_it = cnt_of(M * H * g.ns, wg, team);
  g.cnt_4d = cnt_of((4 * d) >> 5, wg, team);
  return g;
}
// tiles (items for segment 3) of this workgroup in streamed segment `seg` (selects, not a table: the cursors live in SGPRs)
OASR_HD int seg_cnt(const XGeom& g, int seg) { return seg == 0 ? g.cnt_qkv : seg == 3 ? g.cnt_it : seg == 5 ? g.cnt_4d : g.cnt_d; }
struct XItem {
  int b, h, sg, n, kvb;  // sequence, head, key segment, keys in it, ring blocks per K (or V) stream
};
// (no integer division anywhere near the cursors: hipcc expands a 32-bit division through VALU float reciprocals, whose result -- and
// everything computed from it, i.e. the whole block bookkeeping -- then lives in VGPRs under exec-mask branches instead of SGPRs)
OASR_HD XItem item_of(const XGeom& g, int idx) {
  const int id = g.wg + g.team * idx;
  const int hn = g.H * g.ns;
  XItem it;
  it.b = (id >= hn ? 1 : 0) + (id >= 2 * hn ? 1 : 0) + (id >= 3 * hn ? 1 : 0);  // M <= 4 sequences
  const int rem = id - it.b * hn;
  it.h = g.ns == 2 ? rem >> 1 : rem;  // ns <= MAX_SEG = 2
  it.sg = g.ns == 2 ? rem & 1 : 0;
  int n = g.Te - it.sg * dec::SEG_KEYS;
  it.n = n > dec::SEG_KEYS ? dec::SEG_KEYS : n;
  it.kvb = (((it.n + 31) >> 5) + 3) >> 2;
  return it;
}
struct XCur {
  int layer, seg, idx, sub;
};
#if defined(__HIP_DEVICE_COMPILE__)
#define XU(x) __builtin_amdgcn_readfirstlane(x)  // pin a wave-uniform value to an SGPR (hipcc's uniformity analysis gives up on the cursors)
#else
#define XU(x) (x)
#endif
OASR_HD int nsub_of(const XGeom& g, int seg, int idx) {
  if (seg == 3) return 2 * item_of(g, idx).kvb;
  return seg == 6 ? g.nkb_4d : g.nkb_d;
}
// skip empty segments; returns false past the last layer
OASR_HD bool cur_normalise(const XGeom& g, XCur& c) {
  while (c.layer < g.L && c.idx >= seg_cnt(g, c.seg)) {
    c.idx = 0;
    if (++c.seg == NSEG) c.seg = 0, ++c.layer;
  }
  return c.layer < g.L;
}
// the cursor's sub already points one past the unit's last full block: roll over into the next tile / item / segment if the unit ends there
OASR_HD bool cur_advance_from(const XGeom& g, XCur& c) {
  if (c.sub >= nsub_of(g, c.seg, c.idx)) c.sub = 0, ++c.idx;
  const bool more = cur_normalise(g, c);
  c.layer = XU(c.layer), c.seg = XU(c.seg), c.idx = XU(c.idx), c.sub = XU(c.sub);
  return more;
}
OASR_HD bool cur_advance(const XGeom& g, XCur& c) {
  if (++c.sub >= nsub_of(g, c.seg, c.idx)) c.sub = 0, ++c.idx;
  const bool more = cur_normalise(g, c);
  c.layer = XU(c.layer), c.seg = XU(c.seg), c.idx = XU(c.idx), c.sub = XU(c.sub);
  return more;
}

// ---- host side (decode_plan_host.cpp) -------------------------------------------------------------------------------------------------
bool decode_xcd_supports(int d, int H, int Te, int S_max, int L, int M);
// every 32-bit buffer offset of the launch stays below 2 GiB (else: the multi-launch step)
bool decode_xcd_offsets_ok(const DecLayerOffsets& l0, long lstride, long cache_lstride, int d, int Te, int L, int M);
size_t decode_xcd_part_floats(int M, int H, int Te);  // cross-attention partials [M * H * ns][66]: m, l, o[64]
