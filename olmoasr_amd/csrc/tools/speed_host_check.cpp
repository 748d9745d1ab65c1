// Stand-alone host check of the speed-perturbation rule the device kernel shares with the CPU (speed_core.h, speed_host.cpp); built with
// -fsanitize=address,undefined by `make speed-host-check`.  It compares oasr_speed_table, oasr_speed_plan and oasr_speed_perturb_host with
// the rule of include/oasr.h written out again here and with known answers, over a sweep of ratios, lengths, seeds and stream ids, on
// buffers of exactly the size the calls may touch (the sanitizer guards their ends), and checks that bad arguments are refused before
// anything is written.  Exit status 0 = everything agreed.
#include <math.h>
#include <string.h>

#include <vector>

#include "../../../include/oasr.h"
#include "host_check.h"

static uint64_t lcg(uint64_t& s) { return s = s * 6364136223846793005ull + 1442695040888963407ull; }

// ---- the table, from the text of include/oasr.h ---------------------------------------------------------------------------------------
static int check_table(int P, int Q, int want_H) {
  const double pi = 3.14159265358979323846;
  const double fc = 0.95 * (Q < P ? (double)Q / P : 1.0), Wd = 16.0 / fc;
  const int H = (int)floor(Wd) + 1;
  int got_H = -1;
  if (oasr_speed_table(P, Q, nullptr, &got_H) != 0 || got_H != H || H != want_H) return 1;
  std::vector<int32_t> T((size_t)Q * 2 * H);
  if (oasr_speed_table(P, Q, T.data(), &got_H) != 0) return 1;
  int bad = 0;
  for (int r = 0; r < Q; ++r) {
    long sum = 0;
    for (int j = 0; j < 2 * H; ++j) {
      const double u = (double)(j - H + 1) - (double)r / Q;
      double c = 0;
      if (fabs(u) < Wd) c = fc * (u == 0 ? 1.0 : sin(pi * fc * u) / (pi * fc * u)) * (0.5 + 0.5 * cos(pi * u / Wd));
      const long q = (long)floor(c * 32768.0 + 0.5), t = T[(size_t)r * 2 * H + j];
      sum += t;
      // (the tap that took the phase's correction may sit further off: it is the largest one, near the centre)
      if (labs(t - q) > 1 && !(j == H - 1 || j == H)) ++bad;
    }
    bad += sum != 32768;
  }
  return bad;
}

// ---- one batch through the twin, against the rule written out again -------------------------------------------------------------------
static int check_batch(const oasr_speed& pol, int B, int N, int pad, uint64_t seed, uint64_t first, const std::vector<int32_t>& nv, bool tokens) {
  const int S = 9;
  const int64_t ld = N + pad;
  uint64_t s = seed * 77 + first + N;
  std::vector<int16_t> x((size_t)(B - 1) * ld + N), y((size_t)(B - 1) * ld + N, 0x5a5a);
  for (auto& v : x) v = (int16_t)(lcg(s) >> 48);
  for (int b = 0; b < B; ++b)  // full-scale runs so that the clamp is met
    for (int n = 0; n < N && n < 64; ++n) x[(size_t)b * ld + n] = (b & 1) ? 32767 : -32768;
  std::vector<int64_t> ta((size_t)B * S), tb((size_t)B * S);
  static const int64_t ids[S] = {50257, 50363, 50364, 50374, 50363 + 750, 50363 + 1499, 50363 + 1500, 51864, 50256};
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < S; ++i) ta[(size_t)b * S + i] = ids[i], tb[(size_t)b * S + i] = ids[(i + 1) % S];
  std::vector<int32_t> n_out(B, -7), fac(B, -7);
  oasr_speed_args a;
  memset(&a, 0, sizeof(a));
  a.pcm_in = x.data(), a.pcm_out = y.data(), a.n_valid = nv.data(), a.n_out = n_out.data(), a.factor_out = fac.data();
  a.ld_in = a.ld_out = ld, a.seed = seed, a.first_clip = first, a.B = B, a.N = N, a.policy = pol;
  if (tokens) a.tokens_a = ta.data(), a.tokens_b = tb.data(), a.ld_tokens_a = a.ld_tokens_b = S, a.S = S, a.ts_begin = 50363, a.ts_max = 1500;
  if (oasr_speed_perturb_host(&a) != 0) return 1;
  int bad = 0;
  for (int b = 0; b < B; ++b) {
    const uint64_t h = mix(mix(seed) ^ (first + (uint64_t)b));
    int i = (int)(mix(h ^ (3ull << 16)) % (uint64_t)pol.n_factors);
    int P = pol.P[i], Q = pol.Q[i];
    long no = ((long)nv[b] * Q) / P;
    if (no > N) P = Q = 1, no = nv[b], i = -1;
    int pP = 0, pQ = 0, pn = 0, pf = 0;
    bad += oasr_speed_plan(&pol, seed, first + (uint64_t)b, nv[b], N, &pP, &pQ, &pn, &pf) != 0 || pP != P || pQ != Q || pn != no || pf != i;
    bad += n_out[b] != no || fac[b] != i;
    const int16_t* xr = &x[(size_t)b * ld];
    const int16_t* yr = &y[(size_t)b * ld];
    if (P == Q) {
      bad += memcmp(xr, yr, sizeof(int16_t) * N) != 0;
    } else {
      int H = 0;
      oasr_speed_table(P, Q, nullptr, &H);
      std::vector<int32_t> T((size_t)Q * 2 * H);
      oasr_speed_table(P, Q, T.data(), &H);
      for (int n = 0; n < N; ++n) {
        int64_t want = 0;
        if (n < no) {
          const long m = ((long)n * P) / Q, r = ((long)n * P) % Q;
          int64_t acc = 0;
          for (int j = 0; j < 2 * H; ++j) {
            const long k = m + j - H + 1;
            if (k >= 0 && k < nv[b]) acc += (int64_t)xr[k] * T[(size_t)r * 2 * H + j];
          }
          want = (acc + 16384) >> 15;
          want = want < -32768 ? -32768 : want > 32767 ? 32767 : want;
        }
        bad += yr[n] != want;
      }
    }
    if (b + 1 < B)
      for (int n = N; n < ld; ++n) bad += yr[n] != 0x5a5a;  // the gap between rows is not written
    for (int t = 0; t < S && tokens; ++t)
      for (int which = 0; which < 2; ++which) {
        const int64_t id = which ? ids[(t + 1) % S] : ids[t];
        int64_t want = id;
        if (id >= 50363 && id <= 50363 + 1500) {
          const int64_t k = (2 * (id - 50363) * Q + P) / (2 * P);
          want = 50363 + (k < 1500 ? k : 1500);
        }
        bad += (which ? tb : ta)[(size_t)b * S + t] != want;
      }
  }
  return bad;
}

int main() {
  int bad_tables = 0;
  static const int tables[][3] = {{11, 10, 19}, {9, 10, 17}, {3, 2, 26}, {2, 3, 17}, {32, 31, 18}, {1, 2, 17}, {2, 1, 34}, {31, 32, 17}, {17, 9, 32}};
  for (const auto& t : tables) {
    const int r = check_table(t[0], t[1], t[2]);
    if (r) fprintf(stderr, "table %d / %d: %d mismatches\n", t[0], t[1], r);
    bad_tables += r;
  }

  static const oasr_speed policies[] = {{3, {9, 1, 11}, {10, 1, 10}}, {1, {11}, {10}},  {1, {9}, {10}},           {2, {2, 1}, {1, 2}},
                                        {1, {1}, {1}},                {2, {32, 31}, {31, 32}}, {8, {9, 1, 11, 3, 2, 5, 4, 17}, {10, 1, 10, 2, 3, 4, 5, 9}}};
  static const int lengths[] = {1, 37, 300, 1031};
  static const uint64_t seeds[] = {0, 42, (1ull << 63) + 5, ~0ull};
  static const uint64_t firsts[] = {0, (1ull << 32) - 2, ~0ull - 1};
  int bad = 0, n = 0;
  for (const auto& p : policies)
    for (int N : lengths)
      for (uint64_t s : seeds)
        for (uint64_t f : firsts) {
          const std::vector<int32_t> nv = {0, 1, N / 2, N - 1 < 0 ? 0 : N - 1, N};
          const int r = check_batch(p, (int)nv.size(), N, (n % 3) * 5, s, f, nv, n % 2 == 0);
          if (r) fprintf(stderr, "batch mismatch: %d factors, N = %d, seed %llu, first %llu: %d\n", p.n_factors, N, (unsigned long long)s, (unsigned long long)f, r);
          bad += r, ++n;
        }

  // known answers: a constant row stays the constant away from its ends (every phase sums to 2^15), and the token map
  int wrong = 0;
  for (int which = 0; which < 2; ++which) {
    const oasr_speed p = {1, {which ? 9 : 11}, {10}};
    const int N = 4096, nv = 3000, H = which ? 17 : 19;
    std::vector<int16_t> x(N, 0), y(N, 1);
    for (int i = 0; i < nv; ++i) x[i] = 12345;
    int32_t n_valid = nv, n_out = -1, fac = -9;
    int64_t tok[6] = {50363, 50364, 50363 + 11, 50363 + 1500, 50363 + 9, 50362};
    oasr_speed_args a;
    memset(&a, 0, sizeof(a));
    a.pcm_in = x.data(), a.pcm_out = y.data(), a.n_valid = &n_valid, a.n_out = &n_out, a.factor_out = &fac;
    a.ld_in = a.ld_out = N, a.B = 1, a.N = N, a.policy = p, a.tokens_a = tok, a.ld_tokens_a = 6, a.S = 6, a.ts_begin = 50363, a.ts_max = 1500;
    int w = oasr_speed_perturb_host(&a) != 0 || n_out != (nv * 10) / p.P[0] || fac != 0;
    for (int i = 2 * H; i < n_out - 2 * H; ++i) w |= y[i] != 12345;
    for (int i = n_out; i < N; ++i) w |= y[i] != 0;
    static const int64_t want[2][6] = {{50363, 50364, 50363 + 10, 50363 + 1364, 50363 + 8, 50362}, {50363, 50364, 50363 + 12, 50363 + 1500, 50363 + 10, 50362}};
    for (int i = 0; i < 6; ++i) w |= tok[i] != want[which][i];
    wrong += w;
  }
  {  // a slow-down that does not fit: the copy, factor -1
    const oasr_speed p = {1, {9}, {10}};
    std::vector<int16_t> x(100), y(100, 7);
    for (int i = 0; i < 100; ++i) x[i] = (int16_t)(i * 321 - 9000);
    int32_t n_valid = 95, n_out = -1, fac = -9;
    oasr_speed_args a;
    memset(&a, 0, sizeof(a));
    a.pcm_in = x.data(), a.pcm_out = y.data(), a.n_valid = &n_valid, a.n_out = &n_out, a.factor_out = &fac, a.ld_in = a.ld_out = 100, a.B = 1, a.N = 100, a.policy = p;
    wrong += oasr_speed_perturb_host(&a) != 0 || n_out != 95 || fac != -1 || memcmp(x.data(), y.data(), 200) != 0;
  }
  if (wrong) fprintf(stderr, "known answers: %d wrong\n", wrong);

  // refusals, before anything is written
  int accepted = 0;
  {
    std::vector<int16_t> x(64, 3), y(64, 5);
    int32_t n_valid = 64, bad_len = 65;
    int64_t tok[4] = {50363, 50364, 50365, 50366};
    oasr_speed_args ok;
    memset(&ok, 0, sizeof(ok));
    ok.pcm_in = x.data(), ok.pcm_out = y.data(), ok.n_valid = &n_valid, ok.ld_in = ok.ld_out = 64, ok.B = 1, ok.N = 64, ok.policy = {1, {11}, {10}};
    static const oasr_speed refused[] = {{1, {4}, {6}}, {1, {0}, {1}}, {1, {1}, {0}}, {1, {33}, {32}}, {1, {32}, {33}}, {1, {3}, {1}}, {1, {1}, {3}},
                                         {0, {1}, {1}}, {9, {1, 1, 1, 1, 1, 1, 1, 1}, {1, 1, 1, 1, 1, 1, 1, 1}}, {2, {1, 6}, {1, 4}}};
    for (const auto& p : refused) {
      oasr_speed_args a = ok;
      a.policy = p;
      accepted += oasr_speed_perturb_host(&a) == 0;
      int P, Q, no, f;
      accepted += oasr_speed_plan(&p, 0, 0, 10, 64, &P, &Q, &no, &f) == 0;
    }
    oasr_speed_args a = ok;
    a.pcm_out = x.data() + 16;  // overlapping in and out
    a.N = 32, a.ld_in = a.ld_out = 32, n_valid = 32;
    accepted += oasr_speed_perturb_host(&a) == 0;
    n_valid = 64;
    a = ok, a.pcm_in = nullptr, accepted += oasr_speed_perturb_host(&a) == 0;
    a = ok, a.pcm_out = nullptr, accepted += oasr_speed_perturb_host(&a) == 0;
    a = ok, a.n_valid = nullptr, accepted += oasr_speed_perturb_host(&a) == 0;
    a = ok, a.n_valid = &bad_len, accepted += oasr_speed_perturb_host(&a) == 0;
    a = ok, a.B = 0, accepted += oasr_speed_perturb_host(&a) == 0;
    a = ok, a.N = 0, accepted += oasr_speed_perturb_host(&a) == 0;
    a = ok, a.ld_out = 63, accepted += oasr_speed_perturb_host(&a) == 0;
    a = ok, a.tokens_a = tok, a.S = 0, a.ld_tokens_a = 4, accepted += oasr_speed_perturb_host(&a) == 0;
    a = ok, a.tokens_a = tok, a.S = 4, a.ld_tokens_a = 3, accepted += oasr_speed_perturb_host(&a) == 0;
    a = ok, a.tokens_a = tok, a.S = 4, a.ld_tokens_a = 4, a.ts_max = -1, accepted += oasr_speed_perturb_host(&a) == 0;
    accepted += oasr_speed_perturb_host(nullptr) == 0;
    int H = 0;
    accepted += oasr_speed_table(1, 1, nullptr, &H) == 0;
    accepted += oasr_speed_table(4, 6, nullptr, &H) == 0;
    accepted += oasr_speed_table(11, 10, nullptr, nullptr) == 0;
    for (int16_t v : y) accepted += v != 5;
    for (int64_t t : tok) accepted += t < 50363 || t > 50366;
  }
  if (accepted) fprintf(stderr, "bad arguments: %d accepted or written through\n", accepted);
  printf("speed_host_check: tables: %d mismatches; %d batches, %d mismatches; known answers: %d wrong; bad arguments accepted: %d\n", bad_tables, n,
         bad, wrong, accepted);
  return bad_tables || bad || wrong || accepted ? 1 : 0;
}
