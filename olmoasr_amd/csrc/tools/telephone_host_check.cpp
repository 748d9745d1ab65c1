// Stand-alone host check of the telephone channel's rule the device kernel shares with the CPU (telephone_core.h, telephone_host.cpp); built
// with -fsanitize=address,undefined by `make telephone-host-check`.  It compares oasr_telephone_host and oasr_telephone_plan with the rule
// of include/oasr.h written out again here (quantisers by searching the segment, roundings by division, no shifts), over a sweep of shapes,
// lengths, policies, seeds and stream ids, in heap buffers of exactly the size the call may touch (the sanitizer guards their ends); holds
// the two tables to their formulas and to the sums the header states; walks both quantisers over all 65536 inputs; plants the two rows on
// which a 32-bit accumulator wraps; and checks that bad arguments are refused before anything is written.  Exit status 0 = everything agreed.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <vector>

#include "../../../include/oasr.h"
#include "host_check.h"
#include "../telephone_core.h"

static int32_t H[129], U[32];

static int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
static int64_t round_q15(int64_t S) {
  const int64_t v = floor_div(S + 16384, 32768);
  return v < -32768 ? -32768 : v > 32767 ? 32767 : v;
}

// the quantisers again: the segment is searched for, not computed from the leading bit
static int mulaw_again(int x) {
  const bool s = x < 0;
  int a = s ? -x : x;
  if (a > 32635) a = 32635;
  a += 132;
  int e = 0;
  while ((256 << e) <= a) ++e;  // 2^(e + 7) <= a < 2^(e + 8)
  const int m = (a / (8 << e)) % 16;
  const int y = (m * 8 + 132) * (1 << e) - 132;
  return s ? -y : y;
}
static int alaw_again(int x) {
  const bool s = x < 0;
  const int a = s ? -x - 1 : x, v = a / 8;
  int g = 0;
  while ((32 << g) <= v) ++g;  // g = 0 below 32, else 2^(g + 4) <= v < 2^(g + 5)
  const int m = g < 2 ? (v / 2) % 16 : (v / (1 << g)) % 16;
  const int y = g == 0 ? m * 16 + 8 : (m * 16 + 264) * (1 << (g - 1));
  return s ? -y : y;
}
static int quant_again(int x, int codec) { return codec == 1 ? mulaw_again(x) : codec == 2 ? alaw_again(x) : x; }

struct Case {
  int B, N, ld_in, ld_out;
  struct oasr_telephone pol;
  uint64_t seed, first;
};

// the rule on one row, from the header's text; returns the codec (-1: copied)
static int row_again(const Case& c, int b, const int16_t* x, int nv, std::vector<int64_t>& y) {
  const uint64_t h = mix(mix(c.seed) ^ (c.first + (uint64_t)b)), t = 6ull << 16;
  const bool drawn = mix(h ^ t) % 65536 < (uint64_t)c.pol.prob_q16;
  const int codec = c.pol.codecs[mix(h ^ (t | 1)) % (uint64_t)c.pol.n_codecs];
  y.assign(x, x + c.N);
  if (!drawn || nv < 1 || nv > c.N) return -1;
  auto xs = [&](int64_t i) -> int64_t { return i >= 0 && i < nv ? x[i] : 0; };
  const int M = (nv + 1) / 2;
  std::vector<int64_t> cc(M);
  for (int m = 0; m < M; ++m) {
    int64_t z = xs(2 * m);
    if (c.pol.bandpass) {
      int64_t S = 0;
      for (int k = -64; k <= 64; ++k) S += (int64_t)H[k + 64] * xs(2 * (int64_t)m - k);
      z = round_q15(S);
    }
    cc[m] = quant_again((int)z, codec);
  }
  for (int m = 0; m < M; ++m) {
    y[2 * m] = cc[m];
    if (2 * m + 1 < nv) {
      int64_t S = 0;
      for (int j = 0; j < 32; ++j) {
        const int i = m + j - 15;
        if (i >= 0 && i < M) S += (int64_t)U[j] * cc[i];
      }
      y[2 * m + 1] = round_q15(S);
    }
  }
  return codec;
}

static int run(const Case& c, const std::vector<int32_t>& nv, int amp, int* drawn_rows) {
  std::vector<int16_t> x((size_t)(c.B - 1) * c.ld_in + c.N), y((size_t)(c.B - 1) * c.ld_out + c.N, (int16_t)0x5EA7);
  for (auto& s : x) s = rnd16(amp);
  if (c.B > 1)
    for (int n = 0; n < c.N; ++n) x[(size_t)c.ld_in + n] = (n & 64) ? 32767 : -32768;  // a saturating row
  std::vector<int32_t> codec(c.B, 99);
  oasr_telephone_args a;
  memset(&a, 0, sizeof(a));
  a.pcm_in = x.data(), a.pcm_out = y.data(), a.n_valid = nv.data(), a.codec_out = codec.data();
  a.ld_in = c.ld_in, a.ld_out = c.ld_out, a.seed = c.seed, a.first_clip = c.first, a.B = c.B, a.N = c.N, a.policy = c.pol;
  if (oasr_telephone_host(&a) != 0) return c.B;
  int bad = 0;
  std::vector<int64_t> want;
  for (int b = 0; b < c.B; ++b) {
    const int cd = row_again(c, b, x.data() + (size_t)b * c.ld_in, nv[b], want);
    int pd = 0, pc = 0;
    int wrong = oasr_telephone_plan(&c.pol, c.seed, c.first + (uint64_t)b, &pd, &pc) != 0 || codec[b] != cd;
    if (cd >= 0) wrong |= !pd || pc != cd;
    for (int n = 0; n < c.N; ++n) wrong |= y[(size_t)b * c.ld_out + n] != want[n];
    for (int n = c.N; n < c.ld_out && b + 1 < c.B; ++n) wrong |= y[(size_t)b * c.ld_out + n] != (int16_t)0x5EA7;  // between the rows
    bad += wrong, *drawn_rows += cd >= 0;
  }
  return bad;
}

// one row of N samples through the channel: the sample at `at`
static int planted(std::vector<int16_t> x, struct oasr_telephone pol, int at) {
  const int N = (int)x.size();
  std::vector<int16_t> y(N);
  const int32_t nv[1] = {N};
  int32_t cd[1] = {99};
  oasr_telephone_args a;
  memset(&a, 0, sizeof(a));
  a.pcm_in = x.data(), a.pcm_out = y.data(), a.n_valid = nv, a.codec_out = cd, a.ld_in = a.ld_out = N, a.B = 1, a.N = N, a.policy = pol;
  if (oasr_telephone_host(&a) != 0 || cd[0] != 0) return -99999;
  return y[at];
}

int main() {
  rng_state = 424242;
  if (oasr_telephone_tables(H, U) != 0) return 1;

  // the tables against their formulas, and what the header states of them
  int table_wrong = 0;
  {
    const double pi = acos(-1.0);
    auto sinc = [pi](double t) { return t == 0.0 ? 1.0 : sin(pi * t) / (pi * t); };
    int64_t sum_h = 0, sum_u = 0, abs_u = 0, u_first[32], su = 0;
    for (int k = -64; k <= 64; ++k) {
      const double lp_hi = (2.0 * 3400.0 / 16000.0) * sinc(2.0 * 3400.0 * k / 16000.0), lp_lo = (2.0 * 300.0 / 16000.0) * sinc(2.0 * 300.0 * k / 16000.0);
      table_wrong += H[k + 64] != (int32_t)floor((lp_hi - lp_lo) * (0.5 + 0.5 * cos(pi * k / 65.0)) * 32768.0 + 0.5);
      table_wrong += H[k + 64] != H[64 - k];
      sum_h += H[k + 64] < 0 ? -H[k + 64] : H[k + 64];
    }
    int best = 0;
    for (int j = 0; j < 32; ++j) {
      const double t = (j - 15) - 0.5;
      u_first[j] = (int64_t)floor(sinc(t) * (0.5 + 0.5 * cos(pi * t / 16.0)) * 32768.0 + 0.5);
      su += u_first[j];
      if (u_first[j] > u_first[best]) best = j;
    }
    u_first[best] += 32768 - su;
    for (int j = 0; j < 32; ++j) table_wrong += U[j] != u_first[j], sum_u += U[j], abs_u += U[j] < 0 ? -U[j] : U[j];
    table_wrong += sum_h != 76960 || sum_u != 32768 || abs_u != 81604 || !tel_tables_bounded(H, U);
    int32_t h2[129], u2[32];
    memcpy(h2, H, sizeof(H)), memcpy(u2, U, sizeof(U));
    h2[64] += 40000;  // the even taps' sum of |tap| goes above 65535
    table_wrong += tel_tables_bounded(h2, U);
    u2[3] -= 30000;
    table_wrong += tel_tables_bounded(H, u2);
    table_wrong += oasr_telephone_tables(nullptr, nullptr) != 0;  // (each output is optional)
  }
  if (table_wrong) fprintf(stderr, "tables: %d wrong\n", table_wrong);

  // both quantisers over all 65536 inputs
  int quant_wrong = 0;
  for (int codec = 0; codec <= 2; ++codec) {
    std::vector<int16_t> in(65536), out(65536), twice(65536);
    for (int i = 0; i < 65536; ++i) in[i] = (int16_t)(i - 32768);
    quant_wrong += oasr_telephone_quantize_host(in.data(), out.data(), 65536, codec) != 0;
    quant_wrong += oasr_telephone_quantize_host(out.data(), twice.data(), 65536, codec) != 0;
    std::set<int> levels;
    int lo = 0, hi = 0, err = 0;
    for (int i = 0; i < 65536; ++i) {
      const int x = i - 32768, q = out[i];
      quant_wrong += q != quant_again(x, codec) || twice[i] != q || (i && out[i] < out[i - 1]);
      levels.insert(q), lo = q < lo ? q : lo, hi = q > hi ? q : hi, err = abs(q - x) > err ? abs(q - x) : err;
    }
    static const int want[3][6] = {{65536, -32768, 32767, 0, 0, -1}, {255, -32124, 32124, 644, 0, 0}, {256, -32256, 32256, 512, 8, -8}};
    quant_wrong += (int)levels.size() != want[codec][0] || lo != want[codec][1] || hi != want[codec][2] || err != want[codec][3] ||
                   out[32768] != want[codec][4] || out[32767] != want[codec][5];
  }
  int16_t one = 5;
  quant_wrong += oasr_telephone_quantize_host(&one, &one, 1, 3) == 0 || oasr_telephone_quantize_host(&one, &one, -1, 0) == 0 ||
                 oasr_telephone_quantize_host(nullptr, &one, 1, 0) == 0 || oasr_telephone_quantize_host(nullptr, nullptr, 0, 0) != 0 || one != 5;
  if (quant_wrong) fprintf(stderr, "quantisers: %d wrong\n", quant_wrong);

  // the operator against the restated rule
  int bad = 0, rows = 0, drawn = 0, k = 0;
  static const int Ns[] = {1, 2, 37, 300, 700};
  static const struct oasr_telephone pols[] = {{65536, 3, {1, 2, 0}, 1}, {32768, 3, {1, 2, 0}, 1}, {65536, 1, {0}, 1}, {65536, 1, {1}, 0},
                                               {65536, 8, {2, 2, 2, 1, 0, 2, 1, 2}, 0}, {0, 1, {2}, 1}, {65536, 1, {2}, 1}};
  static const uint64_t seeds[][2] = {{0, 0}, {7, 3}, {(1ull << 63) + 5, 1ull << 40}, {~0ull, ~0ull - 2}};
  for (int N : Ns)
    for (const auto& p : pols)
      for (const auto& sf : seeds) {
        const int B = 7;
        const Case c = {B, N, N + (k % 3), N + (k % 2) * 5, p, sf[0], sf[1]};
        const std::vector<int32_t> nv = {N, k % 2 ? 0 : N / 2, N - 1, k % 3 ? 1 : -1, k % 7 ? N : N + 1, N < 3 ? N : 3, N < 2 ? N : 2};
        static const int amps[] = {32767, 3000, 40, 1};
        bad += run(c, nv, amps[k % 4], &drawn), rows += B, ++k;
      }
  if (bad) fprintf(stderr, "operator mismatch: %d rows\n", bad);

  // the rows on which one 32-bit accumulator would wrap: the rule gives +32767, a wrapped sum a negative sample
  int wrap_wrong = 0;
  {
    const int N = 400, p = 200;
    std::vector<int16_t> x(N, 0);
    for (int k2 = -64; k2 <= 64; ++k2) x[p - k2] = H[k2 + 64] >= 0 ? 32767 : -32768;
    wrap_wrong += planted(x, {65536, 1, {0}, 1}, p) != 32767;
    std::vector<int16_t> e(N, 0);
    for (int j = 0; j < 32; ++j) e[2 * (100 + j - 15)] = U[j] >= 0 ? 32767 : -32768;  // c[m + j - 15], m = 100, on the even samples
    wrap_wrong += planted(e, {65536, 1, {0}, 0}, 2 * 100 + 1) != 32767;
  }
  if (wrap_wrong) fprintf(stderr, "planted wrap rows: %d wrong\n", wrap_wrong);

  // refusals, before anything is written
  std::vector<int16_t> x(2 * 64, 3), y(2 * 64, 5);
  std::vector<int32_t> nv = {64, 10}, cd(2, 99);
  oasr_telephone_args ok;
  memset(&ok, 0, sizeof(ok));
  ok.pcm_in = x.data(), ok.pcm_out = y.data(), ok.n_valid = nv.data(), ok.codec_out = cd.data();
  ok.ld_in = ok.ld_out = 64, ok.B = 2, ok.N = 64, ok.policy = {65536, 2, {1, 2}, 1};
  int accepted = 0;
  auto refused = [&](oasr_telephone_args a) { accepted += oasr_telephone_host(&a) == 0; };
  oasr_telephone_args a;
  a = ok, a.pcm_in = nullptr, refused(a);
  a = ok, a.pcm_out = nullptr, refused(a);
  a = ok, a.n_valid = nullptr, refused(a);
  a = ok, a.B = 0, refused(a);
  a = ok, a.B = 65536, refused(a);
  a = ok, a.N = 0, refused(a);
  a = ok, a.N = (1 << 26) + 1, a.ld_in = a.ld_out = a.N, refused(a);
  a = ok, a.ld_in = 63, refused(a);
  a = ok, a.ld_out = 63, refused(a);
  a = ok, a.pcm_in = (const int16_t*)((const char*)x.data() + 1), refused(a);
  a = ok, a.pcm_out = (int16_t*)((char*)y.data() + 1), refused(a);
  a = ok, a.codec_out = (int32_t*)((char*)cd.data() + 2), refused(a);
  a = ok, a.n_valid = (const int32_t*)((const char*)nv.data() + 2), refused(a);
  a = ok, a.pcm_in = y.data(), refused(a);                 // in place is not offered
  a = ok, a.pcm_in = y.data() + 1, a.N = 63, refused(a);   // partial overlap
  a = ok, a.policy.prob_q16 = -1, refused(a);
  a = ok, a.policy.prob_q16 = 65537, refused(a);
  a = ok, a.policy.n_codecs = 0, refused(a);
  a = ok, a.policy.n_codecs = 9, refused(a);
  a = ok, a.policy.codecs[1] = 3, refused(a);
  a = ok, a.policy.codecs[0] = -1, refused(a);
  a = ok, a.policy.bandpass = 2, refused(a);
  accepted += oasr_telephone_host(nullptr) == 0;
  int pd = 9;
  const struct oasr_telephone bad_pol = {65537, 1, {0}, 1};
  accepted += oasr_telephone_plan(&bad_pol, 0, 0, &pd, &pd) == 0;
  accepted += oasr_telephone_plan(nullptr, 0, 0, &pd, &pd) == 0;
  accepted += pd != 9;
  accepted += oasr_telephone_plan(&ok.policy, 0, 0, nullptr, nullptr) != 0;  // (every output is optional)
  for (auto s : y) accepted += s != 5;
  for (int b = 0; b < 2; ++b) accepted += cd[b] != 99;
  if (accepted) fprintf(stderr, "bad arguments: %d accepted or written through\n", accepted);
  accepted += oasr_telephone_host(&ok) != 0;  // ... and the block they were derived from is fine
  a = ok, a.codec_out = nullptr;
  accepted += oasr_telephone_host(&a) != 0;   // ... and so is one without the report
  printf("telephone_host_check: %d rows (%d through the channel), %d mismatches; tables wrong: %d; quantisers wrong: %d; planted wrap rows wrong: %d; "
         "bad arguments accepted: %d\n", rows, drawn, bad, table_wrong, quant_wrong, wrap_wrong, accepted);
  return bad || table_wrong || quant_wrong || wrap_wrong || accepted || drawn == 0 || drawn == rows ? 1 : 0;
}
