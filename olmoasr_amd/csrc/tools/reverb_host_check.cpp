// Stand-alone host check of the reverberation rule the device kernels share with the CPU (reverb_core.h, reverb_host.cpp); built with
// -fsanitize=address,undefined by `make reverb-host-check`.  It compares oasr_reverb_host and oasr_reverb_plan with the rule of include/oasr.h
// written out again here (the sum over every k with the zero extension spelled out, the floor without a shift), over a sweep of shapes,
// lengths, tap counts, delays, policies, seeds and stream ids, in heap buffers of exactly the size the call may touch (the sanitizer guards
// their ends); holds the byte-digit identity the device computes by to the plain product for every tap value against the digit boundaries of
// x; checks known answers and both sides of the clamp, and that bad arguments are refused before anything is written.  Exit status 0 =
// everything agreed.
#include <string.h>

#include <vector>

#include "../../../include/oasr.h"
#include "host_check.h"
#include "../reverb_core.h"

struct Case {
  int B, N, R, K, ld_in, ld_out, ld_rir, prob_q16;
  uint64_t seed, first;
};

// one call of the twin against the restated rule; returns the number of mismatching rows and counts reverberated rows
static int run(const Case& c, const std::vector<int32_t>& nv, int amp_x, int amp_h, int* wet_rows) {
  std::vector<int16_t> x((size_t)(c.B - 1) * c.ld_in + c.N), rir((size_t)(c.R - 1) * c.ld_rir + c.K);
  for (auto& s : x) s = rnd16(amp_x);
  for (auto& s : rir) s = rnd16(amp_h);  // (32767: taps beyond +-32639 meet the clamp)
  if (c.B > 1)
    for (int n = 0; n < c.N; ++n) x[(size_t)c.ld_in + n] = (n & 64) ? 32767 : -32768;  // a saturating row
  std::vector<int32_t> delay(c.R);
  for (int r = 0; r < c.R; ++r) delay[r] = r == 0 ? 0 : r == 1 ? c.K - 1 : r == 2 ? -5 : r == 3 ? c.K + 5 : (int)(mix(++rng_state) % (uint64_t)c.K);
  std::vector<int16_t> y((size_t)(c.B - 1) * c.ld_out + c.N, (int16_t)0x5EA7);
  std::vector<int32_t> row(c.B, 99);
  oasr_reverb_args a;
  memset(&a, 0, sizeof(a));
  a.pcm_in = x.data(), a.pcm_out = y.data(), a.n_valid = nv.data(), a.rir = rir.data(), a.delay = delay.data(), a.row_out = row.data();
  a.ld_in = c.ld_in, a.ld_out = c.ld_out, a.ld_rir = c.ld_rir, a.seed = c.seed, a.first_clip = c.first;
  a.B = c.B, a.N = c.N, a.R = c.R, a.K = c.K, a.policy.prob_q16 = c.prob_q16;
  if (oasr_reverb_host(&a) != 0) return c.B;
  int bad = 0;
  for (int b = 0; b < c.B; ++b) {
    const uint64_t h = mix(mix(c.seed) ^ (c.first + (uint64_t)b)), t = 5ull << 16;
    const bool drawn = mix(h ^ t) % 65536 < (uint64_t)c.prob_q16;
    const int r = (int)(mix(h ^ (t | 1)) % (uint64_t)c.R);
    const struct oasr_reverb pol = {c.prob_q16};
    int pd = 0, pr = 0;
    int wrong = oasr_reverb_plan(&pol, c.seed, c.first + (uint64_t)b, c.R, &pd, &pr) != 0;
    wrong |= pd != (int)drawn || pr != r;
    const bool wet = drawn && nv[b] >= 1 && nv[b] <= c.N;
    wrong |= row[b] != (wet ? r : -1);
    const int16_t* xr = x.data() + (size_t)b * c.ld_in;
    const int16_t* hr = rir.data() + (size_t)r * c.ld_rir;
    const int d = delay[r] < 0 ? 0 : delay[r] > c.K - 1 ? c.K - 1 : delay[r];
    for (int n = 0; n < c.N; ++n) {
      int64_t want = xr[n];
      if (wet && n < nv[b]) {
        int64_t S = 0;
        for (int k = 0; k < c.K; ++k) {
          const int64_t i = (int64_t)n + d - k, tap = hr[k] < -32639 ? -32639 : hr[k] > 32639 ? 32639 : hr[k];
          S += tap * (i >= 0 && i < nv[b] ? xr[i] : 0);
        }
        S += 16384;
        want = S >= 0 ? S / 32768 : -((-S + 32767) / 32768);  // the floor, without a shift
        want = want < -32768 ? -32768 : want > 32767 ? 32767 : want;
      }
      wrong |= y[(size_t)b * c.ld_out + n] != want;
    }
    for (int n = c.N; n < c.ld_out && b + 1 < c.B; ++n) wrong |= y[(size_t)b * c.ld_out + n] != (int16_t)0x5EA7;  // between the rows
    bad += wrong, *wet_rows += wet;
  }
  return bad;
}

int main() {
  rng_state = 4321;
  int bad = 0, rows = 0, wet = 0;
  static const int Ns[] = {1, 37, 600, 1031}, Ks[] = {1, 15, 16, 17, 81, 300};
  static const int probs[] = {65536, 32768, 0};
  static const uint64_t seeds[][2] = {{0, 0}, {7, 3}, {(1ull << 63) + 5, 1ull << 40}, {~0ull, ~0ull - 2}};
  int k = 0;
  for (int N : Ns)
    for (int K : Ks)
      for (int p : probs)
        for (const auto& sf : seeds) {
          const int B = 5, R = 6;
          const Case c = {B, N, R, K, N + (k % 3), N + (k % 2) * 5, K + (k % 4), p, sf[0], sf[1]};
          const std::vector<int32_t> nv = {N, k % 2 ? 0 : N / 2, N - 1, k % 3 ? 1 : -1, k % 7 ? N : N + 1};
          static const int amps[] = {32767, 3000, 40, 1};
          bad += run(c, nv, amps[k % 4], amps[(k / 4) % 4], &wet), rows += B, ++k;
        }
  if (bad) fprintf(stderr, "reverb mismatch: %d rows\n", bad);

  // the byte digits: every tap against the digit boundaries of x, one product at a time through reverb_combine
  int digits_wrong = 0;
  static const int xs[] = {-32768, -32767, -257, -256, -255, -129, -128, -127, -1, 0, 1, 127, 128, 129, 255, 256, 257, 32766, 32767};
  for (int tap = -REVERB_TAP_MAX; tap <= REVERB_TAP_MAX; ++tap) {
    const int th = reverb_tap_hi(tap), tl = reverb_tap_lo(tap);
    digits_wrong += th < -128 || th > 127 || tl < -128 || tl > 127 || 256 * th + tl != tap;
    for (int x : xs) {
      const int xh = reverb_x_hi(x), xl = reverb_x_lo(x);
      digits_wrong += xh < -128 || xh > 127 || xl < -128 || xl > 127 || 256 * xh + xl + 128 != x;
      digits_wrong += reverb_combine(th * xh, tl * xh + th * xl, tl * xl, tap) != (int64_t)tap * x;
    }
  }
  digits_wrong += reverb_x_hi(0) != 0 || reverb_x_lo(0) != -128;  // a zero outside [0, n_valid) is encoded like any sample
  if (digits_wrong) fprintf(stderr, "byte digits: %d wrong\n", digits_wrong);

  // known answers: the clamps and the rounding
  int wrong = 0;
  wrong += reverb_tap(32767) != 32639 || reverb_tap(-32768) != -32639 || reverb_tap(32639) != 32639 || reverb_tap(-5) != -5;
  wrong += reverb_delay(-5, 100) != 0 || reverb_delay(105, 100) != 99 || reverb_delay(42, 100) != 42 || reverb_delay(3, 1) != 0;
  wrong += pcm_round_q15(0) != 0 || pcm_round_q15(16383) != 0 || pcm_round_q15(16384) != 1 || pcm_round_q15(-16384) != 0 || pcm_round_q15(-16385) != -1;
  wrong += pcm_round_q15((int64_t)8192 * 32639 * 32767) != 32767 || pcm_round_q15(-(int64_t)8192 * 32639 * 32768) != -32768;
  wrong += pcm_round_q15((int64_t)32767 << 15) != 32767 || pcm_round_q15(-((int64_t)32768 << 15)) != -32768;
  {
    const int16_t x[4] = {100, -200, 300, -400}, taps[3] = {16384, 32767, -16384};  // 0.5, (clamped) 32639 / 32768, -0.5
    // d = 1: S[n] = taps[0] x[n + 1] + taps[1] x[n] + taps[2] x[n - 1]
    wrong += reverb_sum(x, 4, taps, 3, 1, 0) != (int64_t)16384 * -200 + (int64_t)32639 * 100;
    wrong += reverb_sum(x, 4, taps, 3, 1, 3) != (int64_t)32639 * -400 - (int64_t)16384 * 300;
    wrong += reverb_sum(x, 2, taps, 3, 1, 1) != (int64_t)32639 * -200 - (int64_t)16384 * 100;  // x[2] lies behind n_valid
  }
  if (wrong) fprintf(stderr, "known answers: %d wrong\n", wrong);

  // refusals, before anything is written
  std::vector<int16_t> x(2 * 64, 3), y(2 * 64, 5), rir(2 * 32, 7);
  std::vector<int32_t> nv = {64, 10}, delay = {0, 3}, row(2, 99);
  oasr_reverb_args ok;
  memset(&ok, 0, sizeof(ok));
  ok.pcm_in = x.data(), ok.pcm_out = y.data(), ok.n_valid = nv.data(), ok.rir = rir.data(), ok.delay = delay.data(), ok.row_out = row.data();
  ok.ld_in = ok.ld_out = 64, ok.ld_rir = 32, ok.B = 2, ok.N = 64, ok.R = 2, ok.K = 32, ok.policy.prob_q16 = 65536;
  int accepted = 0;
  auto refused = [&](oasr_reverb_args a) { accepted += oasr_reverb_host(&a) == 0; };
  oasr_reverb_args a;
  a = ok, a.pcm_in = nullptr, refused(a);
  a = ok, a.pcm_out = nullptr, refused(a);
  a = ok, a.n_valid = nullptr, refused(a);
  a = ok, a.rir = nullptr, refused(a);
  a = ok, a.delay = nullptr, refused(a);
  a = ok, a.B = 0, refused(a);
  a = ok, a.B = 65536, refused(a);
  a = ok, a.N = 0, refused(a);
  a = ok, a.N = (1 << 26) + 1, a.ld_in = a.ld_out = a.N, refused(a);
  a = ok, a.R = 0, refused(a);
  a = ok, a.R = 65536, refused(a);
  a = ok, a.K = 0, refused(a);
  a = ok, a.K = 8193, a.ld_rir = 8193, refused(a);
  a = ok, a.ld_in = 63, refused(a);
  a = ok, a.ld_out = 63, refused(a);
  a = ok, a.ld_rir = 31, refused(a);
  a = ok, a.pcm_in = (const int16_t*)((const char*)x.data() + 1), refused(a);
  a = ok, a.pcm_out = (int16_t*)((char*)y.data() + 1), refused(a);
  a = ok, a.rir = (const int16_t*)((const char*)rir.data() + 1), refused(a);
  a = ok, a.row_out = (int32_t*)((char*)row.data() + 2), refused(a);
  a = ok, a.delay = (const int32_t*)((const char*)delay.data() + 2), refused(a);
  a = ok, a.pcm_in = y.data(), refused(a);                // in place is not offered
  a = ok, a.pcm_in = y.data() + 1, a.N = 63, refused(a);  // partial overlap
  a = ok, a.rir = y.data(), refused(a);                   // the bank under the output
  a = ok, a.policy.prob_q16 = -1, refused(a);
  a = ok, a.policy.prob_q16 = 65537, refused(a);
  accepted += oasr_reverb_host(nullptr) == 0;
  int pd = 9;
  const struct oasr_reverb bad_pol = {65537};
  accepted += oasr_reverb_plan(&bad_pol, 0, 0, 1, &pd, &pd) == 0;
  accepted += oasr_reverb_plan(nullptr, 0, 0, 1, &pd, &pd) == 0;
  accepted += oasr_reverb_plan(&ok.policy, 0, 0, 0, &pd, &pd) == 0;
  accepted += oasr_reverb_plan(&ok.policy, 0, 0, 65536, &pd, &pd) == 0;
  accepted += pd != 9;
  accepted += oasr_reverb_plan(&ok.policy, 0, 0, 1, nullptr, nullptr) != 0;  // (every output is optional)
  for (auto s : y) accepted += s != 5;
  for (int b = 0; b < 2; ++b) accepted += row[b] != 99;
  if (accepted) fprintf(stderr, "bad arguments: %d accepted or written through\n", accepted);
  accepted += oasr_reverb_host(&ok) != 0;  // ... and the block they were derived from is fine
  a = ok, a.row_out = nullptr;
  accepted += oasr_reverb_host(&a) != 0;   // (the report is optional)
  printf("reverb_host_check: %d rows (%d reverberated), %d mismatches; byte digits wrong: %d; known answers wrong: %d; bad arguments accepted: %d\n",
         rows, wet, bad, digits_wrong, wrong, accepted);
  return bad || digits_wrong || wrong || accepted || wet == 0 || wet == rows ? 1 : 0;
}
