// The chip-wide step engine's plan (decode_wide.hip): its geometry constants, the split of a projection's (row, 512-element K span) units over
// the workgroups' compute waves, and the host's predicate for the shapes the engine takes.  The kernel and decode_plan_host.cpp
// (oasr_wide_plan_debug / oasr_wide_supports_debug, the CPU suite) share this text.  Plain C++: no HIP header is needed to include this file.
#pragma once
#include "decode_step_core.h"

constexpr int WT = 576;  // threads per workgroup
constexpr int WW = WT / 64;
constexpr int WC = WW - 1;  // compute waves 1 .. WW-1; wave 0 is the helper: poll, operand row, epilogue, stores, flag -- it requests no weights, so nothing slow sits in front of its polls
constexpr int WNG = WT / 8;  // 8-lane groups (attention: one key per group and step)
constexpr int WMAXU = (64 + WC - 1) / WC;  // units per compute wave and phase (64 units per workgroup at most)
constexpr int WNS_LOG = 3;
constexpr int WNS = 1 << WNS_LOG;  // cross-attention key segments per head (one workgroup each)
constexpr int WSK = (448 + WNG - 1) / WNG;  // self-attention keys per 8-lane group: S_max <= 448
constexpr int WCK = (1536 / WNS + WNG - 1) / WNG;  // cross-attention keys per group and segment: Te <= 1536
constexpr int WMAXD = 1280;
constexpr int WMAXL = 32;
constexpr int WMAXWG = 256;
// the exchange areas of the cache's control tail (decode_step_core.h), under the names the kernel uses
constexpr int WREP = dec::KV_REPLICAS;     // flag / packet replicas: one per XCC, 4 KB apart
constexpr int WFS = dec::KV_FLAG_STRIDE;   // dwords between flag replicas
// Rows that every workgroup consumes in the very next phase travel as PACKETS: the producing workgroup's (<= 6) bf16 values and the phase's epoch
// number in ONE 16-byte store per replica; a consumer polls the packets themselves.  No acknowledgement wait before a flag, no separate
// flag-then-row round trip.  Vectors: the block output x (mlp.2 -> the next attn_ln, or the final LayerNorm), x2 (attention output projection ->
// cross_attn_ln), x3 (cross output projection -> mlp_ln), q (cross query -> cross-attention).
constexpr int WPKV = dec::KV_PACKET_VECTORS, WV_X = 0, WV_X2 = 1, WV_X3 = 2, WV_Q = 3, WV_O = 4;  // (O: the self-attention output, 11 packets per head, slot h 11 + j)
constexpr int WQKS = dec::KV_QKV_SLOTS;    // slots per replica of the q | k | v row of the new position: <= 3 packets per workgroup (R <= 18), slot wg 3 + j
constexpr int WPKS = dec::KV_PACKET_SLOTS;  // packet slots per replica: one per workgroup
constexpr int WPKR = 6;      // values per packet at most: R <= 6 for an N = d projection (the kernel is instantiated per R: 2, 4, 6)
static_assert(WV_O == WPKV - 1 && WMAXWG <= WPKS && 3 * WMAXWG <= WQKS && WMAXWG <= WFS, "decode_wide: a slot per workgroup in every exchange area");

// units per compute wave and phase at most, at 256 workgroups (decode_wide_supports checks the shape against it): keeps the unrolled unit loops -- and the
// kernel under the 64 KB of instruction cache two CUs share -- as short as the instantiation allows
template <int RD, int PH>
constexpr int wmu() {  // ceil(units of the workgroup at most / compute waves); units: RD = 2: 6 / 2 / 8 / 8 (q|k|v, N = d, mlp.0, mlp.2), 4: 24 / 8 / 32 / 32, 6 (d <= 1280): 48 / 18 / 60 / 60
  constexpr int u = RD == 2 ? (PH == 0 ? 6 : (PH == 6 || PH == 7) ? 8 : 2) : RD == 4 ? (PH == 0 ? 24 : (PH == 6 || PH == 7) ? 32 : 8) : (PH == 0 ? 48 : (PH == 6 || PH == 7) ? 60 : 18);
  return (u + WC - 1) / WC;
}

// Work split: a projection's N output rows are dealt out in contiguous runs of R = wide_rows(N, nwg) rows per workgroup
OASR_HD int wide_rows(int N, int nwg) { return 2 * ((N + 2 * nwg - 1) / (2 * nwg)); }
// Units (row r of the workgroup's run, 512-element K span j), numbered u = r J + j, are dealt to the compute waves in contiguous runs of
// upw = ceil(U / WC): one division per wave and phase, then (r, j) by stepping.
struct WUnits {
  int U, upw, u0, r0, j0, J, KC;
};
OASR_HD WUnits units_of(int K, int N, int R, int wg, int wave) {  // an [N x K] projection, R rows per workgroup
  WUnits q;
  q.KC = K >> 3, q.J = (q.KC + 63) >> 6;
  int rows = N - wg * R;
  rows = rows < 0 ? 0 : (rows > R ? R : rows);
  q.U = rows * q.J;
  q.upw = (q.U + WC - 1) / WC;  // (WC is a compile-time constant)
  q.u0 = (wave - 1) * q.upw;
  q.r0 = q.u0 / q.J, q.j0 = q.u0 - q.r0 * q.J;
  return q;
}

// ---- host side (decode_plan_host.cpp) -------------------------------------------------------------------------------------------------
// (V: the rows the logits phase deals out -- the token embedding's rows, unpadded; else: the team or the multi-launch step)
bool decode_wide_supports(int d, int H, int Te, int S_max, int L, int M, int nwg, int V);
size_t decode_wide_part_floats(int H);  // cross-attention partials [H * WNS][66]: m, l, o[64]
