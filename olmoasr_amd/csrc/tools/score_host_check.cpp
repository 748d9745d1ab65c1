// Stand-alone host check of the score-reduce rule the device kernel shares with the CPU (score_core.h, score_host.cpp); built with
// -fsanitize=address,undefined by `make score-host-check`.  It compares oasr_score_reduce_host with the rule of include/oasr.h written out
// again here -- a plain loop with its own validity test -- over seeded batches at the row counts where a kernel would change partition, in
// buffers of exactly the size the call may touch (the sanitizer guards their ends), plants a row pair whose fp32 and double sums differ, and
// checks that bad arguments are refused before anything is written.  Exit status 0 = everything agreed.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../../include/oasr.h"

void oasr_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t mod) {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_rng >> 33) % mod;
}

struct Want {
  float sum, mx;
  int32_t n_tok, n_hit;
};
// the rule of include/oasr.h, written from its text
static Want expect(const float* nll, const int32_t* pred, const int64_t* tgt, int span, int S, int V, int64_t ignore) {
  double sum = 0.0;
  float mx = 0.f;
  int n = 0, hit = 0;
  for (int s = 0; s < S && s < span; ++s) {
    const int64_t t = tgt[s];
    if (t == ignore || t < 0 || t >= V) continue;
    sum += (double)nll[s];
    if (n == 0 || nll[s] > mx) mx = nll[s];
    ++n;
    hit += (int64_t)pred[s] == t;
  }
  return Want{(float)sum, n ? mx : 0.f, n, hit};
}
static bool same(float a, float b) { return memcmp(&a, &b, 4) == 0; }

static int g_samples = 0;

static int check_batch(int B, int S, int V, int64_t ignore, bool plant) {
  std::vector<float> nll((size_t)B * S), sum(B, -7.f), mx(B, -7.f);
  std::vector<int32_t> pred((size_t)B * S), span(B), n_tok(B, -7), n_hit(B, -7);
  std::vector<int64_t> tgt((size_t)B * S);
  for (size_t i = 0; i < nll.size(); ++i) {
    nll[i] = ldexpf((float)rnd(1 << 20), -17 + (int)rnd(12));  // magnitudes spread over 12 binades: an fp32 running sum would round
    const uint32_t kind = rnd(8);
    tgt[i] = kind == 0 ? ignore : kind == 1 ? (int64_t)V + rnd(3) : kind == 2 ? -1 - (int64_t)rnd(2) : (int64_t)rnd(V);
    pred[i] = rnd(2) ? (int32_t)tgt[i] : (int32_t)rnd(V);
  }
  for (int b = 0; b < B; ++b) span[b] = b == 0 ? 0 : b == 1 ? S : b == 2 ? S + 5 : b == 3 ? -3 : (int32_t)rnd(S + 1);
  if (plant && B > 1 && S >= 3) {  // 2^24 + 1 + 1: the fp32 running sum stays at 2^24, the double sum rounds to 2^24 + 2
    nll[S + 0] = 16777216.f, nll[S + 1] = 1.f, nll[S + 2] = 1.f;
    for (int s = 0; s < S; ++s) tgt[S + s] = s < 3 ? 1 % V : ignore;
  }
  int bad = oasr_score_reduce_host(nll.data(), pred.data(), tgt.data(), span.data(), B, S, V, ignore, sum.data(), mx.data(), n_tok.data(),
                                   n_hit.data()) != 0;
  for (int b = 0; b < B; ++b) {
    const Want w = expect(&nll[(size_t)b * S], &pred[(size_t)b * S], &tgt[(size_t)b * S], span[b], S, V, ignore);
    const int wrong = !same(sum[b], w.sum) || !same(mx[b], w.mx) || n_tok[b] != w.n_tok || n_hit[b] != w.n_hit;
    if (wrong) fprintf(stderr, "B=%d S=%d V=%d sample %d: got (%g, %g, %d, %d), want (%g, %g, %d, %d)\n", B, S, V, b, sum[b], mx[b], n_tok[b],
                       n_hit[b], w.sum, w.mx, w.n_tok, w.n_hit);
    bad += wrong;
    ++g_samples;
  }
  if (plant && B > 1 && S >= 3 && V > 1 && sum[1] != 16777218.f) {
    fprintf(stderr, "planted pair: nll_sum = %.1f, want 16777218 (a double sum rounded once)\n", sum[1]);
    ++bad;
  }
  return bad;
}

int main() {
  int bad = 0;
  static const int Ss[] = {1, 2, 3, 63, 64, 65, 448, 511, 512, 513, 1100};
  static const int Vs[] = {1, 2, 9, 51865};
  for (int S : Ss)
    for (int V : Vs)
      for (int B : {1, 5}) bad += check_batch(B, S, V, V == 51865 ? 51864 : -100, true);
  // refusals, before anything is written
  int accepted = 0;
  {
    float nll[2] = {1.f, 2.f}, sum = -7.f, mx = -7.f;
    int32_t pred[2] = {0, 0}, span = 2, n_tok = -7, n_hit = -7;
    int64_t tgt[2] = {0, 0};
    accepted += oasr_score_reduce_host(nullptr, pred, tgt, &span, 1, 2, 5, -100, &sum, &mx, &n_tok, &n_hit) == 0;
    accepted += oasr_score_reduce_host(nll, nullptr, tgt, &span, 1, 2, 5, -100, &sum, &mx, &n_tok, &n_hit) == 0;
    accepted += oasr_score_reduce_host(nll, pred, nullptr, &span, 1, 2, 5, -100, &sum, &mx, &n_tok, &n_hit) == 0;
    accepted += oasr_score_reduce_host(nll, pred, tgt, nullptr, 1, 2, 5, -100, &sum, &mx, &n_tok, &n_hit) == 0;
    accepted += oasr_score_reduce_host(nll, pred, tgt, &span, 1, 2, 5, -100, nullptr, &mx, &n_tok, &n_hit) == 0;
    accepted += oasr_score_reduce_host(nll, pred, tgt, &span, 1, 2, 5, -100, &sum, &mx, &n_tok, nullptr) == 0;
    accepted += oasr_score_reduce_host(nll, pred, tgt, &span, 0, 2, 5, -100, &sum, &mx, &n_tok, &n_hit) == 0;
    accepted += oasr_score_reduce_host(nll, pred, tgt, &span, 1, 0, 5, -100, &sum, &mx, &n_tok, &n_hit) == 0;
    accepted += oasr_score_reduce_host(nll, pred, tgt, &span, 1, 2, 0, -100, &sum, &mx, &n_tok, &n_hit) == 0;
    accepted += sum != -7.f || mx != -7.f || n_tok != -7 || n_hit != -7;
    if (accepted) fprintf(stderr, "bad arguments: %d accepted or written through\n", accepted);
  }
  printf("score_host_check: %d samples, %d mismatches; bad arguments accepted: %d; sizeof(oasr_score_args) = %zu\n", g_samples, bad, accepted,
         oasr_sizeof_score_args());
  return bad || accepted ? 1 : 0;
}
