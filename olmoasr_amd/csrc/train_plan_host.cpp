// The host decisions of the training engine (train_plan.h) and the oasr_train_*_debug entries (include/oasr_testing.h) through which the CPU
// suite asks them.  Plain C++ (no HIP, no GPU call); tools/train_plan_host_check.cpp runs the same text under the sanitizers.
#include "train_plan.h"

#include <math.h>

#include "../../include/oasr_testing.h"

static long cdiv_l(long a, long b) { return (a + b - 1) / b; }

WgradPlan train_wgrad_plan(long M, int N, int K, bool view) {
  const long tiles = cdiv_l(N, 256) * cdiv_l(K, 128);
  const long kt = cdiv_l(M, 64);
  // Split-K choice (scripts/wgrad_sweep.py): 768 workgroups are resident at once (3 per CU); what matters is how the
  // tiles x split grid quantises onto them (1.33 waves is the worst case), the (16 + split) K-tiles' worth of atomic epilogue
  // every workgroup adds, and that multiples of 8 let every XCD own whole K-ranges (gemm_fast.hip).
  long split = 1;
  double best = 1e30;
  static const int cand[] = {1, 2, 4, 8, 16, 24, 32};
  for (int s_ : cand) {
    if (s_ > 1 && (kt / s_ < 8 || tiles >= 768)) break;
    const double w = (double)tiles * s_, per = (double)kt / s_ + 16.0 + s_;  // atomics get slower the more splits collide
    const double waves = w <= 768.0 ? 0.7 + 0.3 * w / 768.0 : ceil(w / 768.0);
    const double score = per * waves;
    if (score < 0.97 * best) {
      best = score;
      split = s_;
    }
  }
  WgradPlan p{(int)split, 0};
  // With its MFMA sections pinned the 256x256 ping-pong loop beats the 256x128 kernel on the square and the 4:1 weight shapes
  // (scripts/wgrad_sweep.py, profiles/r02_wgrad_sweep.txt; TF/s pp vs 256x128): 192k tokens [1024x1024] 1071 vs 972 (split 16),
  // [4096x1024] 1157 vs 1117 (8), [1024x4096] 1158 vs 1064 (4); 57k tokens [4096x1024] 1032 vs 956 (4), [1024x4096] 1131 vs 996
  // (4); [3072x1024] and the 57k-token square stay on the 256x128 kernel.  One workgroup per CU: splits give 256-512 workgroups.
  if (M >= 40000 && !view && (N % 256) == 0 && (K % 256) == 0) {
    const long t256 = (long)(N / 256) * (K / 256);
    const bool long_tokens = M >= 150000;
    int pp_split = 0;
    if (t256 == 16 && long_tokens) pp_split = 16;
    else if (t256 == 64) pp_split = (long_tokens && N > K) ? 8 : 4;
    // round 4 (profiles/r04_wgrad_sweep.txt): the cross-attention key|value gradient [2048 x 1024] over the 192k encoder tokens, never swept
    // before: ping-pong split 8 = 0.687 ms (1173 TFLOP/s) vs 0.754 ms (1068) for the best 256x128 split; [3072 x 1024] stays (1.055 vs 1.081)
    else if (t256 == 32 && long_tokens) pp_split = 8;
    if (pp_split) {
      p.atomic_on_pp = 1;
      p.split_k = pp_split;
    }
  }
  return p;
}

BlockNeeds train_block_needs(const BlockAsk& a) {
  BlockNeeds n;
  n.sa = a.need_dx_in || a.sa;
  n.ca = a.cross && (n.sa || a.need_xa || a.ca);
  n.mlp = (a.cross ? n.ca : n.sa) || a.mlp;
  n.ca_kv = n.ca && (a.kv || a.need_xa);
  n.ca_tail = n.ca && (n.sa || a.cln);
  n.sa_tail = n.sa && (a.need_dx_in || a.attn_ln);
  return n;
}

bool span_chunkable(int S_max, int B) { return (S_max % 64) == 0 && S_max <= 64 * OASR_ROWTAB && B <= 512; }

extern "C" int oasr_train_wgrad_plan_debug(long long M, int N, int K, int view, int* split_k, int* atomic_on_pp) {
  if (M < 1 || N < 1 || K < 1 || !split_k || !atomic_on_pp) return OASR_EINVAL;
  const WgradPlan p = train_wgrad_plan((long)M, N, K, view != 0);
  *split_k = p.split_k;
  *atomic_on_pp = p.atomic_on_pp;
  return OASR_OK;
}

extern "C" int oasr_train_block_needs_debug(int asks) {
  if (asks < 0 || asks >= 1 << 9) return -1;
  auto bit = [&](int i) { return ((asks >> i) & 1) != 0; };
  const BlockNeeds n = train_block_needs(BlockAsk{bit(0), bit(1), bit(2), bit(3), bit(4), bit(5), bit(6), bit(7), bit(8)});
  return (n.mlp ? 1 : 0) | (n.ca ? 2 : 0) | (n.sa ? 4 : 0) | (n.ca_kv ? 8 : 0) | (n.ca_tail ? 16 : 0) | (n.sa_tail ? 32 : 0);
}
