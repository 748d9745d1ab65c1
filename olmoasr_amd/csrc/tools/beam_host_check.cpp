// Stand-alone host check of the beam-search rule the device kernel shares with the CPU (beam_core.h, beam_host.cpp); built with
// -fsanitize=address,undefined by `make beam-host-check`.  It compares oasr_beam_update_host, step by step and output by output, with the
// host decoder's rule written out again here -- an insertion-ordered table of (sequence, score, origin) and a stable sort, no shared code --
// on the planted situations (identical prefixes, few survivors, eot inside and behind the beam, a pool cap reached in mid-step, equal
// scores, scores equal in fp32 only, windows completing at different steps and the latch behind them, a short step) and on seeded random
// runs for B in {1, 2, 5, 15}, in buffers of exactly the size the call may touch (the sanitizer guards their ends); then the host reorder
// against a gather through a copy, and the refusals.  Exit status 0 = everything agreed.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../../include/oasr.h"

void oasr_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
}

typedef std::vector<int64_t> Seq;
static const int64_t EOT = 7;

struct Entry {
  Seq seq;
  double score;
  int origin;
};

// the host decoder's state and rule, written from the text of include/oasr.h
struct Ref {
  int n_audio, B, C;
  std::vector<Seq> tokens;
  std::vector<float> sums;
  std::vector<int32_t> sources;
  std::vector<int64_t> last;
  std::vector<std::vector<Entry>> pool;
  std::vector<int> is_short;
  bool completed() const {
    for (const auto& p : pool)
      if ((int)p.size() < C) return false;
    return true;
  }
  void step(const std::vector<float>& lp, const std::vector<int64_t>& tk) {
    const int K = B + 1;
    if (completed()) {
      for (int r = 0; r < n_audio * B; ++r)
        if (!is_short[r / B]) sources[r] = r;
      return;
    }
    const std::vector<Seq> tok0 = tokens;
    const std::vector<float> sum0 = sums;
    for (int a = 0; a < n_audio; ++a) {
      if (is_short[a]) continue;
      std::vector<Entry> table;  // insertion ordered; a repeated key keeps its place and takes the new score and origin
      for (int j = 0; j < B; ++j)
        for (int k = 0; k < K; ++k) {
          const int idx = a * B + j;
          Seq s = tok0[idx];
          s.push_back(tk[idx * K + k]);
          const double sc = (double)sum0[idx] + (double)lp[idx * K + k];
          auto it = std::find_if(table.begin(), table.end(), [&](const Entry& e) { return e.seq == s; });
          if (it == table.end()) table.push_back(Entry{s, sc, idx});
          else it->score = sc, it->origin = idx;
        }
      std::stable_sort(table.begin(), table.end(), [](const Entry& x, const Entry& y) { return x.score > y.score; });
      std::vector<Entry> cont, newly;
      for (const auto& e : table) {
        if (e.seq.back() == EOT) newly.push_back(e);
        else {
          cont.push_back(e);
          if ((int)cont.size() == B) break;
        }
      }
      if ((int)cont.size() < B) {
        is_short[a] = 1;
        continue;
      }
      for (const auto& e : newly)
        if ((int)pool[a].size() < C) pool[a].push_back(e);
      for (int m = 0; m < B; ++m) {
        const int r = a * B + m;
        tokens[r] = cont[m].seq, sums[r] = (float)cont[m].score, sources[r] = cont[m].origin, last[r] = cont[m].seq.back();
      }
    }
  }
};

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t mod) {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_rng >> 33) % mod;
}

struct Step {
  std::vector<float> lp;
  std::vector<int64_t> tk;
};

static int g_steps = 0;

// one case through the twin and the restatement; the twin's buffers are exactly as large as the contract says
static int run(const char* name, int n_audio, int B, int C, int n_ctx, const std::vector<Seq>& init, const std::vector<float>& init_sums,
               const std::vector<Step>& steps, int expect_short = 0, int expect_completed_at = -1) {
  const int n = n_audio * B, K = B + 1;
  const int64_t FILL = -7;
  Ref ref{n_audio, B, C, init, init_sums, std::vector<int32_t>(n), std::vector<int64_t>(n, init[0].back()), std::vector<std::vector<Entry>>(n_audio),
          std::vector<int>(n_audio, 0)};
  for (int r = 0; r < n; ++r) ref.sources[r] = r;
  std::vector<int64_t> buf[2] = {std::vector<int64_t>((size_t)n * n_ctx, FILL), std::vector<int64_t>((size_t)n * n_ctx, FILL)};
  for (int r = 0; r < n; ++r) std::copy(init[r].begin(), init[r].end(), buf[0].begin() + (size_t)r * n_ctx);
  std::vector<float> sums = init_sums;
  std::vector<int32_t> sources = ref.sources, pool_len((size_t)n_audio * C, 0), count(n_audio, 0), full(n_audio, OASR_BEAM_NOT_FULL), shrt(n_audio, 0);
  std::vector<int64_t> last = ref.last, pool_tok((size_t)n_audio * C * n_ctx, FILL);
  std::vector<double> pool_score((size_t)n_audio * C, -7.0);
  int len = (int)init[0].size(), cur = 0, bad = 0, completed_at = -1;
  for (size_t i = 0; i < steps.size(); ++i, ++g_steps) {
    oasr_beam_args a = {};
    a.top_logprob = steps[i].lp.data(), a.top_token = steps[i].tk.data(), a.tokens_in = buf[cur].data(), a.tokens_out = buf[1 - cur].data();
    a.sums = sums.data(), a.sources = sources.data(), a.last_token = last.data(), a.pool_tokens = pool_tok.data(), a.pool_len = pool_len.data();
    a.pool_score = pool_score.data(), a.pool_count = count.data(), a.pool_full_len = full.data(), a.short_step = shrt.data();
    a.n_audio = n_audio, a.beam = B, a.max_candidates = C, a.n_ctx = n_ctx, a.len = len, a.eot = EOT;
    if ((int)steps[i].lp.size() != n * K || oasr_beam_update_host(&a) != 0) return 1;
    ref.step(steps[i].lp, steps[i].tk);
    cur = 1 - cur, ++len;
    int w = 0;
    for (int r = 0; r < n; ++r) {
      const int64_t* row = buf[cur].data() + (size_t)r * n_ctx;
      if (!ref.is_short[r / B]) {
        const Seq& want = ref.tokens[r];
        for (int t = 0; t < n_ctx; ++t) w |= row[t] != (t < (int)want.size() ? want[t] : FILL);
      }
      w |= !(sums[r] == ref.sums[r]) || sources[r] != ref.sources[r] || last[r] != ref.last[r];
    }
    for (int a2 = 0; a2 < n_audio; ++a2) {
      w |= count[a2] != (int)ref.pool[a2].size() || shrt[a2] != ref.is_short[a2];
      for (int k = 0; k < C; ++k) {
        const int64_t* row = pool_tok.data() + ((size_t)a2 * C + k) * n_ctx;
        const Seq none;
        const Seq& want = k < count[a2] && k < (int)ref.pool[a2].size() ? ref.pool[a2][k].seq : none;
        for (int t = 0; t < n_ctx; ++t) w |= row[t] != (t < (int)want.size() ? want[t] : FILL);
        if (!want.empty()) w |= pool_len[a2 * C + k] != (int)want.size() || !(pool_score[a2 * C + k] == ref.pool[a2][k].score);
      }
    }
    bool done = true;
    for (int a2 = 0; a2 < n_audio; ++a2) done &= full[a2] != OASR_BEAM_NOT_FULL;
    w |= done != ref.completed();
    if (done && completed_at < 0) completed_at = (int)i;
    if (w) fprintf(stderr, "%s: step %zu differs from the restatement\n", name, i);
    bad += w;
  }
  int any_short = 0;
  for (int s : shrt) any_short |= s;
  if (any_short != expect_short) fprintf(stderr, "%s: short = %d, expected %d\n", name, any_short, expect_short), ++bad;
  if (expect_completed_at >= 0 && completed_at != expect_completed_at)
    fprintf(stderr, "%s: completed at step %d, expected %d\n", name, completed_at, expect_completed_at), ++bad;
  return bad;
}

// rows of (logprob, token) lists -> one step, padded with (-inf, 0) to K entries
typedef std::vector<std::pair<float, int64_t>> Row;
static Step step_of(const std::vector<Row>& rows, int K) {
  Step s;
  for (const auto& r : rows)
    for (int k = 0; k < K; ++k) {
      s.lp.push_back(k < (int)r.size() ? r[k].first : -INFINITY);
      s.tk.push_back(k < (int)r.size() ? r[k].second : 0);
    }
  return s;
}
static std::vector<Row> split(int B) {  // B distinct prefixes out of one
  Row r;
  for (int k = 0; k < B; ++k) r.push_back({-0.1f * (k + 1), k + 1});
  return std::vector<Row>(B, r);
}
static std::vector<Row> cat(std::vector<Row> x, const std::vector<Row>& y) {
  x.insert(x.end(), y.begin(), y.end());
  return x;
}

static std::vector<Step> random_steps(int n, int B, int n_steps) {
  std::vector<Step> steps;
  for (int i = 0; i < n_steps; ++i) {
    std::vector<Row> rows;
    for (int r = 0; r < n; ++r) {
      std::vector<int64_t> vocab;
      for (int t = 0; t < 8; ++t)
        if (t != EOT || rnd(10) < 3) vocab.push_back(t);
      for (size_t k = vocab.size(); k > 1; --k) std::swap(vocab[k - 1], vocab[rnd((uint32_t)k)]);
      const size_t take = std::min<size_t>(B + 1, vocab.size() - rnd(3));
      std::vector<float> lps;
      for (size_t k = 0; k < take; ++k) lps.push_back(-(float)rnd(4000) / 1000.f);
      std::sort(lps.begin(), lps.end(), [](float x, float y) { return x > y; });
      Row row;
      for (size_t k = 0; k < take; ++k) row.push_back({lps[k], vocab[k]});
      rows.push_back(row);
    }
    steps.push_back(step_of(rows, B + 1));
  }
  return steps;
}

int main() {
  int bad = 0;
  const Seq INIT = {100, 101};
  auto same = [&](int n) { return std::vector<Seq>(n, INIT); };
  auto zeros = [](int n) { return std::vector<float>(n, 0.f); };
  // identical prefixes: the candidates of three rows collapse
  bad += run("identical prefixes", 1, 3, 3, 8, same(3), zeros(3),
             {step_of({{{-0.1f, 1}, {-0.5f, 2}, {-1.0f, 3}, {-2.0f, 4}}, {{-0.2f, 1}, {-0.4f, 2}, {-1.1f, 3}, {-2.5f, 5}}, {{-0.3f, 1}, {-0.6f, 2}, {-0.9f, 3}, {-3.0f, EOT}}}, 4),
              step_of(std::vector<Row>(3, Row{{-0.1f, 4}, {-0.2f, 5}, {-0.3f, 6}, {-0.4f, 1}}), 4)});
  // few survivors: (-inf, 0) more than once in a row
  bad += run("few survivors", 1, 3, 3, 8, same(3), zeros(3),
             {step_of(split(3), 4), step_of({{{-0.1f, 1}, {-0.2f, 2}}, {{-0.3f, 3}, {-0.4f, 4}, {-0.5f, 5}, {-0.6f, 6}}, {{-0.2f, 1}, {-0.9f, 2}}}, 4),
              step_of({{{-0.1f, 1}, {-0.2f, 2}}, {{-0.1f, 1}}, {{-0.5f, 5}, {-0.6f, 6}, {-0.7f, 2}, {-0.8f, 3}}}, 4)});
  // eot inside the beam is pooled, eot behind the B-th continuation is dropped
  bad += run("eot ranking", 1, 2, 2, 8, same(2), zeros(2),
             {step_of(split(2), 3), step_of({{{-0.1f, 1}, {-0.2f, EOT}, {-3.0f, 2}}, {{-0.5f, 3}, {-4.0f, 4}, {-5.0f, EOT}}}, 3)});
  {  // the pool cap (2 of 3) in mid-step; a second window that never finishes keeps the first from latching
    std::vector<Row> eots, plain(3, Row{{-0.3f, 1}, {-0.4f, 2}, {-0.5f, 3}, {-0.6f, 4}});
    for (int j = 0; j < 3; ++j) eots.push_back(Row{{-0.1f * (j + 1), EOT}, {-1.0f, 1}, {-1.1f, 2}, {-1.2f, 3}});
    bad += run("pool cap", 2, 3, 2, 8, same(6), zeros(6),
               {step_of(cat(split(3), split(3)), 4), step_of(cat(eots, plain), 4), step_of(cat(eots, plain), 4), step_of(cat(plain, plain), 4)});
    // a short step in window 0; window 1 goes on
    bad += run("short step", 2, 3, 3, 8, same(6), zeros(6),
               {step_of(cat(std::vector<Row>(3, Row{{-0.1f, EOT}}), split(3)), 4), step_of(cat(plain, plain), 4), step_of(cat(plain, plain), 4)}, 1);
  }
  bad += run("equal scores", 1, 2, 2, 8, same(2), zeros(2),
             {step_of(std::vector<Row>(2, Row{{-0.5f, 1}, {-0.5f, 2}, {-9.0f, 3}}), 3),
              step_of({{{-1.0f, 3}, {-1.0f, 4}, {-3.0f, 5}}, {{-1.0f, 4}, {-2.0f, 3}, {-3.0f, 5}}}, 3)});
  bad += run("fp32 versus double", 1, 2, 2, 8, same(2), {-16777216.f, -16777216.f},
             {step_of({{{-1.0f, 1}, {-2.0f, 3}, {-3.0f, 4}}, {{-0.5f, 2}, {-2.5f, 5}, {-3.5f, 6}}}, 3)});
  {  // three windows complete at steps 1, 2 and 4; two latched updates behind them
    std::vector<Step> steps;
    const int at[3] = {1, 2, 4};
    for (int i = 0; i < 7; ++i) {
      std::vector<Row> rows;
      for (int a = 0; a < 3; ++a)
        for (int j = 0; j < 2; ++j) {
          if (i == 0) rows.push_back(Row{{-0.1f, 1}, {-0.2f, 2}, {-9.0f, 3}});
          else if (i == at[a]) rows.push_back(Row{{-0.1f, EOT}, {-0.5f - 0.1f * j, 3}, {-0.9f, 4}});
          else rows.push_back(Row{{-0.2f - 0.1f * j, 1 + (i + j) % 5}, {-0.6f, 6}, {-2.0f + 0.5f * j, 2 - j}});
        }
      steps.push_back(step_of(rows, 3));
    }
    bad += run("latch", 3, 2, 2, 10, same(6), zeros(6), steps, 0, 4);
  }
  // patience: C = 2 < B = 4, C = 2 B
  bad += run("patience 0.5", 2, 4, 2, 16, same(8), zeros(8), random_steps(8, 4, 12));
  bad += run("patience 2.0", 2, 3, 6, 16, same(6), zeros(6), random_steps(6, 3, 12));
  // seeded random runs; 15 rows start from distinct prefixes (15 rows of one prefix over 8 tokens are short at once)
  static const int beams[] = {1, 2, 5, 15};
  for (int B : beams)
    for (int seed = 0; seed < 3; ++seed) {
      std::vector<Seq> init = same(2 * B);
      if (B > 5)
        for (int r = 0; r < 2 * B; ++r) init[r][0] = 100 + r;
      bad += run("random", 2, B, B, 14, init, zeros(2 * B), random_steps(2 * B, B, 12));
    }
  // the host reorder against a gather through a copy, 2- and 4-byte elements, in a buffer of exactly L layers
  int reorder_bad = 0;
  for (int esz : {2, 4}) {
    const int L = 2, B = 6, n_ctx = 5, d = 4, group = 3, pos = 3;
    const size_t row = (size_t)3 * d * esz, layer = (size_t)B * n_ctx * row;
    std::vector<unsigned char> buf(L * layer), want;
    for (auto& x : buf) x = (unsigned char)rnd(256);
    want = buf;
    const int32_t src[B] = {0, 0, 1, 5, 3, 3};
    for (int l = 0; l < L; ++l)
      for (int j = 0; j < B; ++j)
        for (int p = 0; p < pos; ++p)
          for (size_t b = (size_t)d * esz; b < row; ++b) want[l * layer + ((size_t)j * n_ctx + p) * row + b] = buf[l * layer + ((size_t)src[j] * n_ctx + p) * row + b];
    reorder_bad += oasr_decode_reorder_host(buf.data(), (int64_t)layer, L, B, n_ctx, d, esz, pos, group, src) != 0 || buf != want;
    const int32_t foreign[B] = {0, 0, 3, 5, 3, 3};
    reorder_bad += oasr_decode_reorder_host(buf.data(), (int64_t)layer, L, B, n_ctx, d, esz, pos, group, foreign) == 0 || buf != want;
    reorder_bad += oasr_decode_reorder_host(buf.data(), (int64_t)layer, L, B, n_ctx, d, esz, pos, 4, src) == 0;
    reorder_bad += oasr_decode_reorder_host(buf.data(), (int64_t)layer, L, B, n_ctx, d, esz, n_ctx + 1, group, src) == 0 || buf != want;
  }
  if (reorder_bad) fprintf(stderr, "host reorder: %d wrong results or accepted bad arguments\n", reorder_bad);
  // refusals, before anything is written
  int accepted = 0;
  {
    std::vector<int64_t> tin(2 * 8, 1), tout(2 * 8, -7), tk(2 * 3, 1), last(2, -7), ptok(2 * 8, -7);
    std::vector<float> lp(2 * 3, -1.f), sums(2, 0.f);
    std::vector<int32_t> src(2, -7), plen(2, -7), cnt(1, 0), full(1, OASR_BEAM_NOT_FULL), shrt(1, 0);
    std::vector<double> psc(2, -7.0);
    oasr_beam_args a = {};
    a.top_logprob = lp.data(), a.top_token = tk.data(), a.tokens_in = tin.data(), a.tokens_out = tout.data(), a.sums = sums.data();
    a.sources = src.data(), a.last_token = last.data(), a.pool_tokens = ptok.data(), a.pool_len = plen.data(), a.pool_score = psc.data();
    a.pool_count = cnt.data(), a.pool_full_len = full.data(), a.short_step = shrt.data();
    a.n_audio = 1, a.beam = 2, a.max_candidates = 2, a.n_ctx = 8, a.len = 2, a.eot = EOT;
    oasr_beam_args z = a;
    z.beam = 16, accepted += oasr_beam_update_host(&z) == 0;
    z = a, z.beam = 0, accepted += oasr_beam_update_host(&z) == 0;
    z = a, z.n_audio = 0, accepted += oasr_beam_update_host(&z) == 0;
    z = a, z.max_candidates = 0, accepted += oasr_beam_update_host(&z) == 0;
    z = a, z.len = 8, accepted += oasr_beam_update_host(&z) == 0;
    z = a, z.len = 0, accepted += oasr_beam_update_host(&z) == 0;
    z = a, z.tokens_out = tin.data(), accepted += oasr_beam_update_host(&z) == 0;
    z = a, z.top_token = nullptr, accepted += oasr_beam_update_host(&z) == 0;
    z = a, z.short_step = nullptr, accepted += oasr_beam_update_host(&z) == 0;
    accepted += oasr_beam_update_host(nullptr) == 0;
    for (auto x : tout) accepted += x != -7;
    for (auto x : src) accepted += x != -7;
    accepted += oasr_beam_update_host(&a) != 0;  // (and the block itself is fine)
    if (accepted) fprintf(stderr, "bad arguments: %d accepted or written through\n", accepted);
  }
  printf("beam_host_check: %d steps, %d mismatches; host reorder: %d wrong; bad arguments accepted: %d; sizeof(oasr_beam_args) = %zu\n", g_steps, bad,
         reorder_bad, accepted, oasr_sizeof_beam_args());
  return bad || reorder_bad || accepted ? 1 : 0;
}
