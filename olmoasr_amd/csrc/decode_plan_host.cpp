// The host half of the one-launch decoder step engines: which shapes and layouts each engine takes (engine_decode.hip::pick_step_engine, the
// launchers' guards), and the oasr_*_debug entries (include/oasr_testing.h) through which the CPU suite walks the very plan code the kernels
// run (decode_xcd_plan.h, decode_wide_plan.h).  Plain C++ (no HIP, no GPU call): this file's build rule is what keeps those headers plain C++.
#include "../../include/oasr_testing.h"
#include "decode_wide_plan.h"
#include "decode_xcd_plan.h"

static_assert(OASR_KV_TAIL_BYTES == dec::KV_TAIL_BYTES, "include/oasr.h and decode_step_core.h disagree: the control tail's areas end where the tail ends");

// ---- the one-XCD team engine (decode_xcd.hip) ---------------------------------------------------------------------------------------------
size_t decode_xcd_part_floats(int M, int H, int Te) { return (size_t)M * H * dec::n_segments(Te) * 66; }

bool decode_xcd_supports(int d, int H, int Te, int S_max, int L, int M) {
  // (d % 256: a wave's K quarter is whole 64-element ring blocks)
  return M >= 1 && M <= XMAXM && L >= 1 && L <= XMAXL && d % 256 == 0 && d == H * 64 && d <= XMAXD && S_max <= dec::SEG_KEYS &&
         Te <= dec::MAX_SEG * dec::SEG_KEYS && Te >= 1 && H * dec::n_segments(Te) <= XMAXPAIR;
}

// The ring DMA addresses everything through raw buffer descriptors with 32-bit byte offsets from the start of the bf16 weight shadow and
// from layer 0's cross K/V rows (decode_xcd_ring.h: rsrc_of / dma16_s, num_records 0x7fffffff): an offset at or past 2 GiB would read zeros
// without any error.  True when the furthest byte any block of this launch can address stays below that (weights: OLMoASR-large ends at
// ~1.7 GB because the decoder sits at the start of the arena); the engine takes the multi-launch step otherwise.
bool decode_xcd_offsets_ok(const DecLayerOffsets& l0, long lstride, long cache_lstride, int d, int Te, int L, int M) {
  const long kLimit = (1L << 31) - (1L << 20);  // 1 MiB of slack for the per-lane part of an address
  const long woff[6] = {l0.wqkv, l0.wo, l0.wcq, l0.wco, l0.w1, l0.w2};
  const long wsize[6] = {3L * d * d, (long)d * d, (long)d * d, (long)d * d, 4L * d * d, 4L * d * d};
  // layer l = layer 0 + l * lstride; the arena keeps the decoder blocks in gradient-completion order (last block first), so the stride
  // is NEGATIVE in the product's layout: both ends of the walk are checked
  const long span = (long)(L - 1) * lstride;
  for (int k = 0; k < 6; ++k) {
    const long first = woff[k] + (span < 0 ? span : 0), last = woff[k] + (span > 0 ? span : 0) + wsize[k];
    if (first < 0 || last * 2 >= kLimit) return false;
  }
  const long kv_end = (long)(L - 1) * cache_lstride + (long)M * Te * 2 * d;  // from layer 0's cross K/V rows
  return cache_lstride >= 0 && kv_end * 2 < kLimit;
}

extern "C" int oasr_xcd_offsets_ok_debug(const int64_t* layer0, long long lstride, long long cache_lstride, int d, int Te, int L, int M) {
  DecLayerOffsets l0;
  for (int k = 0; k < DecLayerOffsets::FIELDS; ++k) l0.fields()[k] = (long)layer0[k];
  return decode_xcd_offsets_ok(l0, (long)lstride, (long)cache_lstride, d, Te, L, M) ? 1 : 0;
}

// Debug / CPU test: the block sequence (seg, idx, sub) of workgroup `wg` as the kernel's cursors generate it
extern "C" int oasr_xcd_plan_debug(int d, int H, int Te, int M, int L, int team, int wg, int* out, int max_blocks) {
  const XGeom g = make_geom(d, H, Te, M, L, team, wg);
  XCur c{0, 0, 0, 0};
  int n = 0;
  bool more = cur_normalise(g, c);
  while (more) {
    if (n < max_blocks) out[4 * n] = c.layer, out[4 * n + 1] = c.seg, out[4 * n + 2] = c.idx, out[4 * n + 3] = c.sub;
    ++n;
    more = cur_advance(g, c);
  }
  return n;
}

// ---- the chip-wide engine (decode_wide.hip) --------------------------------------------------------------------------------------------------
size_t decode_wide_part_floats(int H) { return (size_t)H * WNS * 66; }

// wmu<rd, ph>() for a run-time (rows per workgroup of an N = d projection, projection phase): the bound the kernel's instantiation unrolls
static int wmu_of(int rd, int ph) {
  return rd == 2 ? (ph == 0 ? wmu<2, 0>() : ph == 2 ? wmu<2, 2>() : wmu<2, 6>()) : rd == 4 ? (ph == 0 ? wmu<4, 0>() : ph == 2 ? wmu<4, 2>() : wmu<4, 6>())
                                                                                           : (ph == 0 ? wmu<6, 0>() : ph == 2 ? wmu<6, 2>() : wmu<6, 6>());
}

// V: the rows of the tied logits projection as the last phase deals them out (the token embedding's rows, unpadded: logits_phase's RW)
bool decode_wide_supports(int d, int H, int Te, int S_max, int L, int M, int nwg, int V) {
  if (!(M == 1 && L >= 1 && L <= WMAXL && d % 64 == 0 && d == H * 64 && d <= WMAXD && H <= 32 && S_max >= 1 && S_max <= WNG * WSK && Te >= 1 &&
        (Te + WNS - 1) / WNS <= WNG * WCK && nwg >= 64 && nwg <= WMAXWG && nwg % 4 == 0 && H * WNS <= nwg))
    return false;
  const int rd = wide_rows(d, nwg);
  if (rd > WPKR) return false;  // an N = d projection's rows per workgroup fill one packet
  if (V < 1 || (V + nwg - 1) / nwg > 64 * WC) return false;  // the logits phase parks a wave's rows of the workgroup's run in its 64 lanes
  {
    const int R0 = wide_rows(3 * d, nwg), NP0 = (R0 + 5) / 6;  // the q | k | v row: <= 3 packets per workgroup, <= 16 packets per head and range
    if (NP0 > 3 || ((63 + R0 - 1) / R0 + 1) * NP0 > 16 || H * 11 > WPKS) return false;
  }
  // units per wave: rows R x spans J dealt to 8 waves, within what the instantiation for this R_d unrolls (wmu)
  {
    auto upw = [&](int N, int K) { return (wide_rows(N, nwg) * ((K / 8 + 63) / 64) + WC - 1) / WC; };
    if (upw(3 * d, d) > wmu_of(rd, 0) || upw(d, d) > wmu_of(rd, 2) || upw(4 * d, d) > wmu_of(rd, 6) || upw(d, 4 * d) > wmu_of(rd, 6)) return false;
  }
  const int Ns[3] = {3 * d, d, 4 * d}, Ks[3] = {d, 4 * d, d};
  for (int i = 0; i < 3; ++i) {
    const int R = wide_rows(Ns[i], nwg), J = (Ks[i] / 8 + 63) / 64;
    if (R * J > 64 || R > 64) return false;
  }
  return true;
}

// Test hooks (include/oasr_testing.h): whether a shape runs on this engine, and the units of one compute wave (-1 past the unrolled bound, wmu)
extern "C" int oasr_wide_supports_debug(int d, int H, int Te, int S_max, int L, int M, int nwg, int V) {
  return decode_wide_supports(d, H, Te, S_max, L, M, nwg, V) ? 1 : 0;
}
extern "C" int oasr_wide_plan_debug(int d, int nwg, int N, int K, int wg, int wave, int* out, int max_units) {
  if (wave < 1 || wave > WC || wg < 0 || wg >= nwg) return -1;
  const int R = wide_rows(N, nwg);
  const WUnits q = units_of(K, N, R, wg, wave);
  const int cnt = q.U - q.u0 < q.upw ? q.U - q.u0 : q.upw;
  const int ph = N == 3 * d ? 0 : (N == 4 * d ? 6 : (K == 4 * d ? 7 : 2));
  if (cnt > wmu_of(wide_rows(d, nwg), ph)) return -1;
  int n = 0, j = q.j0, r = q.r0;
  for (int i = 0; i < cnt && n < max_units; ++i, ++n) {
    out[2 * n] = wg * R + r, out[2 * n + 1] = j;
    if (++j == q.J) j = 0, ++r;
  }
  return n;
}
