// Stand-alone host check of the training engine's host decisions (train_plan.h, train_plan_host.cpp); built with
// -fsanitize=address,undefined by `make train_plan-host-check`.  The weight-gradient plan is held to recorded answers at the production
// shapes and to its legality rules over a sweep of shapes that reaches every candidate and both thresholds; the block-needs function is
// compared, over all 512 inputs, with the backward written as it used to be -- one pass with seven exits -- which records how far it got;
// the debug entries are called through exactly-sized heap words (the sanitizer guards their ends) and must refuse bad arguments before
// writing.  Exit status 0 = everything agreed.
#include <stdio.h>

#include <memory>

#include "../../../include/oasr_testing.h"
#include "../train_plan.h"

static int check_wgrad() {
  static const long rows[][6] = {{192000, 1024, 1024, 0, 16, 1}, {192000, 4096, 1024, 0, 8, 1}, {192000, 2048, 1024, 0, 8, 1}, {192000, 3072, 1024, 0, 8, 0},
                                 {57344, 1024, 1024, 0, 16, 0},  {57344, 1024, 4096, 0, 4, 1},  {57344, 1, 1024, 0, 24, 0},    {149999, 1024, 1024, 0, 24, 0},
                                 {39999, 4096, 1024, 0, 4, 0},   {192000, 1024, 4096, 1, 16, 0}, {384000, 1024, 256, 0, 32, 0}, {896, 384, 384, 0, 1, 0}};
  int bad = 0;
  for (auto& r : rows) {
    const WgradPlan w = train_wgrad_plan(r[0], (int)r[1], (int)r[2], r[3] != 0);
    if (w.split_k != r[4] || w.atomic_on_pp != r[5]) {
      fprintf(stderr, "wgrad plan (%ld, %ld, %ld, view %ld): got (%d, %d), want (%ld, %ld)\n", r[0], r[1], r[2], r[3], w.split_k, w.atomic_on_pp, r[4], r[5]);
      ++bad;
    }
  }
  // legality over a sweep: a split launch_gemm takes, never more K ranges than the rule allows, ping-pong only where its tiles are whole
  static const long Ms[] = {1, 63, 64, 511, 512, 513, 3000, 18688, 39999, 40000, 57344, 149999, 150000, 192000, 1L << 22};
  static const int NKs[] = {1, 8, 80, 256, 384, 1024, 1152, 2048, 3072, 4096, 51864};
  std::unique_ptr<int> split(new int(-7)), pp(new int(-7));
  for (long M : Ms)
    for (int N : NKs)
      for (int K : NKs)
        for (int view = 0; view < 2; ++view) {
          const WgradPlan w = train_wgrad_plan(M, N, K, view != 0);
          const bool cand = w.split_k == 1 || w.split_k == 2 || w.split_k == 4 || w.split_k == 8 || w.split_k == 16 || w.split_k == 24 || w.split_k == 32;
          const bool pp_ok = w.atomic_on_pp == 0 || (w.atomic_on_pp == 1 && !view && N % 256 == 0 && K % 256 == 0 && M >= 40000);
          const bool deep = w.split_k == 1 || (M + 63) / 64 / w.split_k >= 8;
          const int rc = oasr_train_wgrad_plan_debug(M, N, K, view, split.get(), pp.get());
          if (!cand || !pp_ok || !deep || rc != OASR_OK || *split != w.split_k || *pp != w.atomic_on_pp) {
            fprintf(stderr, "wgrad plan (%ld, %d, %d, view %d): (%d, %d), entry rc %d (%d, %d)\n", M, N, K, view, w.split_k, w.atomic_on_pp, rc, *split, *pp);
            ++bad;
          }
        }
  *split = *pp = -7;
  bad += oasr_train_wgrad_plan_debug(0, 8, 8, 0, split.get(), pp.get()) == OASR_OK;
  bad += oasr_train_wgrad_plan_debug(8, 0, 8, 0, split.get(), pp.get()) == OASR_OK;
  bad += oasr_train_wgrad_plan_debug(8, 8, -1, 0, split.get(), pp.get()) == OASR_OK;
  bad += oasr_train_wgrad_plan_debug(8, 8, 8, 0, nullptr, pp.get()) == OASR_OK;
  bad += oasr_train_wgrad_plan_debug(8, 8, 8, 0, split.get(), nullptr) == OASR_OK;
  bad += *split != -7 || *pp != -7;
  return bad;
}

// the block's backward as one pass with an exit wherever nothing further was needed; returns the answer bits of oasr_train_block_needs_debug
static int walk(const BlockAsk& a) {
  const bool sa_need = a.need_dx_in || a.sa;
  const bool ca_need = a.cross && (sa_need || a.need_xa || a.ca);
  const bool mlp_need = (a.cross ? ca_need : sa_need) || a.mlp;
  int got = 0;
  if (!mlp_need) return got;
  got |= 1;
  if (a.cross) {
    if (!ca_need) return got;
    got |= 2;
    if (a.kv || a.need_xa) got |= 8;
    if (!sa_need && !a.cln) return got;
    got |= 16;
  }
  if (!sa_need) return got;
  got |= 4;
  if (!a.need_dx_in && !a.attn_ln) return got;
  return got | 32;
}

static int check_needs() {
  int bad = 0;
  for (int asks = 0; asks < 512; ++asks) {
    auto bit = [&](int i) { return ((asks >> i) & 1) != 0; };
    const BlockAsk a = {bit(0), bit(1), bit(2), bit(3), bit(4), bit(5), bit(6), bit(7), bit(8)};
    const int want = walk(a), got = oasr_train_block_needs_debug(asks);
    const BlockNeeds n = train_block_needs(a);
    const bool nested = (!n.sa || !a.cross || n.ca) && (!n.ca || n.mlp) && (!n.sa || n.mlp) && (!n.ca || a.cross) && (!n.ca_kv || n.ca) &&
                        (!n.ca_tail || n.ca) && (!n.sa_tail || n.sa);
    if (got != want || !nested) {
      fprintf(stderr, "block needs, asks 0x%03x: got 0x%02x, want 0x%02x, nested %d\n", asks, got, want, (int)nested);
      ++bad;
    }
  }
  bad += oasr_train_block_needs_debug(-1) != -1;
  bad += oasr_train_block_needs_debug(512) != -1;
  return bad;
}

static int check_chunkable() {
  int bad = 0;
  bad += !span_chunkable(448, 1) + !span_chunkable(64, 512) + !span_chunkable(64 * OASR_ROWTAB, 8);
  bad += span_chunkable(447, 1) + span_chunkable(64 * OASR_ROWTAB + 64, 1) + span_chunkable(448, 513) + span_chunkable(32, 1);
  return bad;
}

int main() {
  const int w = check_wgrad(), n = check_needs(), s = check_chunkable();
  printf("train_plan_host_check: weight-gradient plan %d mismatches, block needs %d mismatches in 512 rows, span_chunkable %d\n", w, n, s);
  return w || n || s ? 1 : 0;
}
