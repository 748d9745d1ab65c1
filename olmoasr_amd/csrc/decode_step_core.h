// What the KV-cached decoder step's engines and the host code that drives them agree on, declared ONCE: the offsets of a decoder layer, the
// layout of the cache's control tail, the key segments, the engines' numbers and the experiment flags.  Plain C++ (under hipcc: include it after
// the HIP runtime header).  olmoasr_amd/_native.py mirrors the KV_* constants and tests/test_native_abi.py parses them out of this file to hold
// the mirrors to them, so they stay `NAME = integer expression of earlier names`.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "core_hd.h"

// ---- element offsets of one decoder layer: w* into the bf16 shadow, bqkv_aux into the aux region, the rest into the fp32 parameter arena -----
// The one-launch kernels take layer 0's by value in their arguments (the field order is kernel-argument layout) and derive layer l from two
// strides, so the decoder blocks must lie back to back: engine.hip checks that when it builds the context.
struct DecLayerOffsets {
  long ln1g, ln1b, wqkv, bqkv_aux, wo, bo, lncg, lncb, wcq, bcq, wco, bco, ln2g, ln2b, w1, b1, w2, b2;
  static constexpr int FIELDS = 18;
  // the one view as an array, in declaration order (the regularity check of engine.hip; oasr_xcd_offsets_ok_debug's int64_t[18])
  long* fields() { return &ln1g; }
  const long* fields() const { return &ln1g; }
};
static_assert(sizeof(DecLayerOffsets) == DecLayerOffsets::FIELDS * sizeof(long), "DecLayerOffsets: 18 longs, no padding");
static_assert(sizeof(long) == sizeof(int64_t), "DecLayerOffsets holds arena offsets (int64_t)");

namespace dec {

// layer l = layer 0 + l * lstride; bqkv_aux, the one field that lives in the aux region, strides by astride
OASR_HD DecLayerOffsets layer_at(const DecLayerOffsets& l0, int l, long lstride, long astride) {
  DecLayerOffsets y = l0;
  const long s = (long)l * lstride;
  y.ln1g += s, y.ln1b += s, y.wqkv += s, y.wo += s, y.bo += s, y.lncg += s, y.lncb += s, y.wcq += s, y.bcq += s, y.wco += s, y.bco += s;
  y.ln2g += s, y.ln2b += s, y.w1 += s, y.b1 += s, y.w2 += s, y.b2 += s;
  y.bqkv_aux += (long)l * astride;
  return y;
}

// ---- cached keys are processed in segments of <= SEG_KEYS (decode_shared.h: the scores of a segment live in LDS) ------------------------------
constexpr int SEG_KEYS = 768;
constexpr int MAX_SEG = 2;  // Tk <= 1536
OASR_HD int n_segments(int Tk) { return (Tk + SEG_KEYS - 1) / SEG_KEYS; }

// ---- the KV cache's control tail (the last OASR_KV_TAIL_BYTES of the cache, zeroed by oasr_decode_begin), in 32-bit words -----------------------
enum KvCtrl : int {
  KV_TEAM_COUNTER = 0,  // decode_xcd: team barrier counter (never reset: every launch adds phases x team)
  KV_ERROR = 1,         // both one-launch engines: KvError bits, 0 = fine (read by oasr_decode_check)
  KV_TEAM_EPOCH = 2,    // decode_xcd: the counter's value at the start of the next launch
  KV_XCC_MASK = 3,      // both: bit i = a workgroup ran on XCC i (placement is a speed matter only)
  KV_WIDE_EPOCH = 4,    // decode_wide: phases completed by earlier launches
  KV_CTRL_WORDS = 5,
};
enum KvError : unsigned {
  KV_ERR_TIMEOUT = 1u,         // a workgroup never reached a barrier / a flag or packet never came: the launch is poisoned, not hung
  KV_ERR_STREAM = 0x100u,      // decode_xcd, checked instantiation: | streamed segment whose consumer and producer cursors disagree ...
  KV_ERR_STREAM_K = 0x103u,    // ... the cross-attention K blocks (KV_ERR_STREAM | segment 3)
  KV_ERR_STREAM_V = 0x113u,    // ... the cross-attention V blocks
  KV_ERR_TABLE_FULL = 0x200u,  // decode_xcd: the unit table of a wave overflowed (never for a supported shape)
};
// decode_wide's exchange areas behind the control words: per-workgroup phase flags, row packets {bf16 x 6, epoch} of the five vectors every
// workgroup consumes in the very next phase, and the packets of the new position's q | k | v row -- each replicated once per XCC
constexpr int KV_REPLICAS = 8;          // 256 workgroups polling the same cache lines serialise on one memory channel: a replica per XCC
constexpr int KV_FLAG_STRIDE = 1024;    // words between flag replicas (4 KB); one flag per workgroup, <= 256 used
constexpr int KV_PACKET_VECTORS = 5;    // x, x2, x3, q, o
constexpr int KV_PACKET_SLOTS = 256;    // packets per vector and replica: one per workgroup
constexpr int KV_QKV_SLOTS = 3 * 256;   // packets per replica of the q | k | v row: <= 3 per workgroup
constexpr int KV_PACKET_WORDS = 4;      // 16 bytes
constexpr int KV_FLAGS_WORD = KV_FLAG_STRIDE;  // replica r at KV_FLAGS_WORD + r * KV_FLAG_STRIDE (the first 4 KB hold the control words)
constexpr int KV_PACKETS_WORD = 16 * KV_FLAG_STRIDE;  // 64 KB in: [KV_PACKET_VECTORS][KV_REPLICAS][KV_PACKET_SLOTS] packets = 160 KB
constexpr int KV_QKV_PACKETS_WORD = KV_PACKETS_WORD + KV_PACKET_VECTORS * KV_REPLICAS * KV_PACKET_SLOTS * KV_PACKET_WORDS;  // [KV_REPLICAS][KV_QKV_SLOTS] = 96 KB
constexpr int KV_TAIL_WORDS = KV_QKV_PACKETS_WORD + KV_REPLICAS * KV_QKV_SLOTS * KV_PACKET_WORDS;
static_assert(KV_CTRL_WORDS <= KV_FLAGS_WORD && KV_FLAGS_WORD + KV_REPLICAS * KV_FLAG_STRIDE <= KV_PACKETS_WORD, "control words | flag replicas | packets overlap");
constexpr int KV_TAIL_BYTES = 4 * KV_TAIL_WORDS;  // == OASR_KV_TAIL_BYTES of include/oasr.h (320 KB; asserted by decode_plan_host.cpp, which sees both)

// ---- which engine a step runs on (oasr_decode_set_ln_fold: the name is historical) ---------------------------------------------------------------
enum StepMode : int {
  STEP_DEFAULT = -1,        // one sequence: the chip-wide engine, else the one-XCD team; 2-4 sequences: folded; more: separate kernels
  STEP_SEPARATE_LN = 0,     // multi-launch, separate LayerNorm kernels
  STEP_FOLDED_LN = 1,       // multi-launch, LayerNorm folded into the projections' operand loads, for every B <= 32
  STEP_TEAM_XCD = 2,        // decode_xcd.hip: 32 workgroups on the CUs of one XCD (B <= 4)
  STEP_TEAM_SPREAD32 = 3,   // ... the same team spread over the chip
  STEP_TEAM_SPREAD64 = 4,   // ... 64 workgroups spread over the chip
  STEP_WIDE = 5,            // decode_wide.hip: every CU (one sequence; more: as STEP_TEAM_XCD)
};
// experiment flags of the one-launch engines (OASR_XCD_FLAGS, scripts/decode_xcd_probe.py; 0 in production)
enum StepFlags : int {
  XF_PLAIN_STORES = 1,     // decode_xcd: plain (not agent-scope) activation stores
  XF_NO_SLEEP = 4,         // no s_sleep in the barrier / flag polls
  XF_CHECKED = 8,          // decode_xcd: the checked instantiation (the consumer mirrors the producer's cursor)
  XF_STAMPS = 0x100,       // in-kernel s_memtime stamps into the workspace tail
  XF_STAMP_WG_SHIFT = 9,   // bits 9-16: the workgroup whose stamps the chip-wide engine takes
};

}  // namespace dec
