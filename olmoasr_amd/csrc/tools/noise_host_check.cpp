// Stand-alone host check of the noise-mixing rule the device kernels share with the CPU (noise_core.h, noise_host.cpp); built with
// -fsanitize=address,undefined by `make noise-host-check`.  It compares oasr_noise_mix_host and oasr_noise_plan with the rule of
// include/oasr.h written out again here (another square root, indices by %), over a sweep of shapes, lengths, policies, seeds and stream ids,
// in heap buffers of exactly the size the call may touch (the sanitizer guards their ends), out of place and in place, holds the 61
// amplitudes to their defining inequality in integers, checks known answers and the extremes of the gain, and checks that bad arguments
// are refused before anything is written.  Exit status 0 = everything agreed.
#include <string.h>

#include <vector>

#include "../../../include/oasr.h"
#include "host_check.h"
#include "../noise_core.h"

static uint64_t newton_isqrt(uint64_t v) {  // floor(sqrt(v)) for v < 2^63, by Newton's iteration from above
  if (v < 2) return v;
  uint64_t r = 1ull << 32, q;
  while ((q = (r + v / r) / 2) < r) r = q;
  return r;
}

struct Case {
  int B, N, M, L, ld_in, ld_out, ld_bank;
  oasr_noise pol;
  uint64_t seed, first;
  bool in_place;
};

// one call of the twin against the restated rule; returns the number of mismatching rows and counts mixed rows
static int run(const Case& c, const std::vector<int32_t>& nv, int amp_x, int amp_v, int* mixed_rows) {
  const int ld_in = c.in_place ? c.ld_out : c.ld_in;
  std::vector<int16_t> x((size_t)(c.B - 1) * ld_in + c.N), bank((size_t)(c.M - 1) * c.ld_bank + c.L);
  for (auto& s : x) s = rnd16(amp_x);
  for (auto& s : bank) s = rnd16(amp_v);
  if (c.B > 1) {  // a saturating row and a silent one
    for (int n = 0; n < c.N; ++n) x[(size_t)ld_in + n] = (n & 64) ? 32767 : -32768;
    for (int n = 0; n < c.N; ++n) x[n] = 0;
  }
  std::vector<int16_t> y((size_t)(c.B - 1) * c.ld_out + c.N, (int16_t)0x5EA7), x0 = x;
  std::vector<int32_t> row(c.B, 99), snr(c.B, 99);
  std::vector<int64_t> gain(c.B, 99);
  oasr_noise_args a;
  memset(&a, 0, sizeof(a));
  a.pcm_in = x.data(), a.pcm_out = c.in_place ? x.data() : y.data(), a.n_valid = nv.data(), a.bank = bank.data();
  a.row_out = row.data(), a.snr_out = snr.data(), a.gain_out = gain.data();
  a.ld_in = ld_in, a.ld_out = c.ld_out, a.ld_bank = c.ld_bank, a.seed = c.seed, a.first_clip = c.first;
  a.B = c.B, a.N = c.N, a.M = c.M, a.L = c.L, a.policy = c.pol;
  if (oasr_noise_mix_host(&a) != 0) return c.B;
  const int16_t* out = c.in_place ? x.data() : y.data();
  int bad = 0;
  for (int b = 0; b < c.B; ++b) {
    const uint64_t h = mix(mix(c.seed) ^ (c.first + (uint64_t)b)), t = 4ull << 16;
    const bool drawn = mix(h ^ t) % 65536 < (uint64_t)c.pol.prob_q16;
    const int m = (int)(mix(h ^ (t | 1)) % (uint64_t)c.M), o = (int)(mix(h ^ (t | 2)) % (uint64_t)c.L);
    const int s = c.pol.snr_lo_db + (int)(mix(h ^ (t | 3)) % (uint64_t)(c.pol.snr_hi_db - c.pol.snr_lo_db + 1));
    int pd = 0, pm = 0, po = 0, ps = 0;
    int wrong = oasr_noise_plan(&c.pol, c.seed, c.first + (uint64_t)b, c.M, c.L, &pd, &pm, &po, &ps) != 0;
    wrong |= pd != (int)drawn || pm != m || po != o || ps != s;
    const int16_t* xr = x0.data() + (size_t)b * ld_in;
    const int16_t* vr = bank.data() + (size_t)m * c.ld_bank;
    int64_t g = 0;
    bool mixed = false;
    if (drawn && nv[b] >= 1 && nv[b] <= c.N) {
      uint64_t Ex = 0, Ev = 0;
      for (int n = 0; n < nv[b]; ++n) {
        const int64_t xs = xr[n], vs = vr[((int64_t)o + n) % c.L];
        Ex += (uint64_t)(xs * xs), Ev += (uint64_t)(vs * vs);
      }
      int sh = 0;
      while (((Ex | Ev) >> sh) >> 31) ++sh;
      const uint64_t ex = Ex >> sh, ev = Ev >> sh;
      if (ex && ev) {
        mixed = true;
        g = (int64_t)((newton_isqrt((ex << 32) / ev) * (uint64_t)noise_amplitude(s) + 16384) >> 15);
      }
    }
    wrong |= row[b] != (mixed ? m : -1) || snr[b] != (mixed ? s : OASR_NOISE_NONE) || gain[b] != g;
    for (int n = 0; n < c.N; ++n) {
      int64_t want = xr[n];
      if (mixed && n < nv[b]) {
        const int64_t add = (int64_t)vr[((int64_t)o + n) % c.L] * g + 32768;
        want += add >= 0 ? add / 65536 : -((-add + 65535) / 65536);  // the floor, without a shift
        want = want < -32768 ? -32768 : want > 32767 ? 32767 : want;
      }
      wrong |= out[(size_t)b * c.ld_out + n] != want;
    }
    if (!c.in_place)
      for (int n = c.N; n < c.ld_out && b + 1 < c.B; ++n) wrong |= y[(size_t)b * c.ld_out + n] != (int16_t)0x5EA7;  // between the rows
    bad += wrong, *mixed_rows += mixed;
  }
  return bad;
}

int main() {
  rng_state = 12345;
  int bad = 0, rows = 0, mixed = 0;
  static const int Ns[] = {1, 37, 4096, 4099}, Ls[] = {1, 7, 1000, 4099, 9000};
  static const oasr_noise pols[] = {{65536, -10, 50}, {32768, 5, 20}, {0, 0, 0}, {65536, 0, 0}, {65536, 50, 50}, {65536, -10, -10}};
  static const uint64_t seeds[][2] = {{0, 0}, {7, 3}, {(1ull << 63) + 5, 1ull << 40}, {~0ull, ~0ull - 2}};
  int k = 0;
  for (int N : Ns)
    for (int L : Ls)
      for (const auto& p : pols)
        for (const auto& sf : seeds) {
          const int B = 5, M = 3;
          const Case c = {B, N, M, L, N + (k % 3), N + (k % 2) * 5, L + (k % 4), p, sf[0], sf[1], (k % 5) == 4};
          const std::vector<int32_t> nv = {N, k % 2 ? 0 : N / 2, N - 1, k % 3 ? 1 : -1, k % 7 ? N : N + 1};
          static const int amps[] = {32767, 3000, 40, 1};
          bad += run(c, nv, amps[k % 4], amps[(k / 4) % 4], &mixed), rows += B, ++k;
        }
  if (bad) fprintf(stderr, "mix mismatch: %d rows\n", bad);

  // the table: A = round(10^(-s / 20) 2^15)  <=>  (2 A - 1)^20 <= 2^320 10^(-s) < (2 A + 1)^20, compared in base 2^32 digits
  int table_wrong = 0;
  for (int s = NOISE_SNR_MIN; s <= NOISE_SNR_MAX; ++s) {
    auto power = [](uint64_t base, int e, int shift10, int pow2) {  // base^e * 10^shift10 * 2^pow2 as little-endian 32-bit digits
      std::vector<uint32_t> d(64, 0);
      d[pow2 / 32] = 1u << (pow2 % 32);
      auto mul = [&d](uint64_t f) {
        uint64_t carry = 0;
        for (auto& w : d) {
          const uint64_t t = (uint64_t)w * f + carry;
          w = (uint32_t)t, carry = t >> 32;
        }
      };
      for (int i = 0; i < e; ++i) mul(base);
      for (int i = 0; i < shift10; ++i) mul(10);
      return d;
    };
    auto less_eq = [](const std::vector<uint32_t>& p, const std::vector<uint32_t>& q) {
      for (int i = 63; i >= 0; --i)
        if (p[i] != q[i]) return p[i] < q[i];
      return true;
    };
    const uint64_t A = (uint64_t)noise_amplitude(s);
    // (2 A -+ 1)^20 10^max(s, 0)  against  2^320 10^max(-s, 0)
    const auto lo = power(2 * A - 1, 20, s > 0 ? s : 0, 0), hi = power(2 * A + 1, 20, s > 0 ? s : 0, 0), mid = power(1, 0, s < 0 ? -s : 0, 320);
    table_wrong += !less_eq(lo, mid) || less_eq(hi, mid);
  }
  table_wrong += noise_amplitude(-10) != 103622 || noise_amplitude(0) != 32768 || noise_amplitude(50) != 104;
  if (table_wrong) fprintf(stderr, "amplitude table: %d entries wrong\n", table_wrong);

  // known answers and extremes of the gain
  int wrong = 0;
  int64_t g = -1;
  wrong += !noise_gain(1000, 1000, 0, &g) || g != 65536;                                   // x = v at 0 dB
  wrong += noise_gain(0, 1000, 0, &g) || g != 0;                                           // a silent clip
  wrong += noise_gain(1000, 0, 0, &g) || g != 0;                                           // a silent bank row
  wrong += noise_gain((1ull << 56) - 1, 1, -10, &g) || g != 0;                             // ev vanishes at the common scale
  wrong += noise_gain(1, (1ull << 56) - 1, 50, &g) || g != 0;                              // ex does
  wrong += !noise_gain((1ull << 56), (1ull << 26), -10, &g) || g != (int64_t)((32768ull * 65536 * 103622 + 16384) >> 15);  // v = +-1 under full scale
  wrong += g >= (1ll << 34);
  wrong += noise_isqrt(0) != 0 || noise_isqrt(1) != 1 || noise_isqrt(3) != 1 || noise_isqrt(4) != 2 ||
           noise_isqrt((1ull << 63) - 1) != 3037000499ull || noise_isqrt(~0ull) != 0xffffffffull;
  wrong += noise_bitlength(0) != 0 || noise_bitlength(1) != 1 || noise_bitlength(1ull << 31) != 32 || noise_bitlength(~0ull) != 64;
  wrong += noise_sample(32767, 32767, (1ll << 34) - 1) != 32767 || noise_sample(-32768, 32767, (1ll << 34) - 1) != 32767 ||
           noise_sample(0, -32768, (1ll << 34) - 1) != -32768 || noise_sample(5, -1, 32768) != 5 || noise_sample(5, -1, 32769) != 4 ||
           noise_sample(5, 1, 32768) != 6;
  if (wrong) fprintf(stderr, "known answers: %d wrong\n", wrong);

  // refusals, before anything is written
  std::vector<int16_t> x(2 * 64, 3), y(2 * 64, 5), bank(2 * 32, 7);
  std::vector<int32_t> nv = {64, 10}, row(2, 99), snr(2, 99);
  std::vector<int64_t> gain(2, 99);
  oasr_noise_args ok;
  memset(&ok, 0, sizeof(ok));
  ok.pcm_in = x.data(), ok.pcm_out = y.data(), ok.n_valid = nv.data(), ok.bank = bank.data(), ok.row_out = row.data(), ok.snr_out = snr.data();
  ok.gain_out = gain.data(), ok.ld_in = ok.ld_out = 64, ok.ld_bank = 32, ok.B = 2, ok.N = 64, ok.M = 2, ok.L = 32, ok.policy = {65536, 5, 20};
  int accepted = 0;
  auto refused = [&](oasr_noise_args a) { accepted += oasr_noise_mix_host(&a) == 0; };
  oasr_noise_args a;
  a = ok, a.pcm_in = nullptr, refused(a);
  a = ok, a.pcm_out = nullptr, refused(a);
  a = ok, a.n_valid = nullptr, refused(a);
  a = ok, a.bank = nullptr, refused(a);
  a = ok, a.B = 0, refused(a);
  a = ok, a.B = 65536, refused(a);
  a = ok, a.N = 0, refused(a);
  a = ok, a.N = (1 << 26) + 1, a.ld_in = a.ld_out = a.N, refused(a);
  a = ok, a.M = 0, refused(a);
  a = ok, a.M = 65536, refused(a);
  a = ok, a.L = 0, refused(a);
  a = ok, a.L = (1 << 26) + 1, a.ld_bank = a.L, refused(a);
  a = ok, a.ld_in = 63, refused(a);
  a = ok, a.ld_out = 63, refused(a);
  a = ok, a.ld_bank = 31, refused(a);
  a = ok, a.pcm_in = (const int16_t*)((const char*)x.data() + 1), refused(a);
  a = ok, a.pcm_out = (int16_t*)((char*)y.data() + 1), refused(a);
  a = ok, a.bank = (const int16_t*)((const char*)bank.data() + 1), refused(a);
  a = ok, a.row_out = (int32_t*)((char*)row.data() + 2), refused(a);
  a = ok, a.gain_out = (int64_t*)((char*)gain.data() + 4), refused(a);
  a = ok, a.pcm_in = y.data() + 1, a.N = 63, refused(a);                 // partial overlap
  a = ok, a.pcm_in = y.data(), a.ld_in = 64, a.ld_out = 65, a.B = 1, refused(a);  // the same buffer, another stride
  a = ok, a.bank = y.data(), refused(a);                                  // the bank under the output
  a = ok, a.policy.prob_q16 = -1, refused(a);
  a = ok, a.policy.prob_q16 = 65537, refused(a);
  a = ok, a.policy.snr_lo_db = -11, refused(a);
  a = ok, a.policy.snr_hi_db = 51, refused(a);
  a = ok, a.policy.snr_lo_db = 21, refused(a);
  accepted += oasr_noise_mix_host(nullptr) == 0;
  int pd = 9;
  const oasr_noise bad_pol = {65537, 5, 20};
  accepted += oasr_noise_plan(&bad_pol, 0, 0, 1, 1, &pd, &pd, &pd, &pd) == 0;
  accepted += oasr_noise_plan(nullptr, 0, 0, 1, 1, &pd, &pd, &pd, &pd) == 0;
  accepted += oasr_noise_plan(&ok.policy, 0, 0, 0, 1, &pd, &pd, &pd, &pd) == 0;
  accepted += oasr_noise_plan(&ok.policy, 0, 0, 1, 0, &pd, &pd, &pd, &pd) == 0;
  accepted += oasr_noise_plan(&ok.policy, 0, 0, 65536, 1, &pd, &pd, &pd, &pd) == 0;
  accepted += oasr_noise_plan(&ok.policy, 0, 0, 1, (1 << 26) + 1, &pd, &pd, &pd, &pd) == 0;
  accepted += pd != 9;
  accepted += oasr_noise_plan(&ok.policy, 0, 0, 1, 1, nullptr, nullptr, nullptr, nullptr) != 0;  // (every output is optional)
  for (auto s : y) accepted += s != 5;
  for (int b = 0; b < 2; ++b) accepted += row[b] != 99 || snr[b] != 99 || gain[b] != 99;
  if (accepted) fprintf(stderr, "bad arguments: %d accepted or written through\n", accepted);
  accepted += oasr_noise_mix_host(&ok) != 0;  // ... and the block they were derived from is fine
  printf("noise_host_check: %d rows (%d mixed), %d mismatches; table entries wrong: %d; known answers wrong: %d; bad arguments accepted: %d\n", rows,
         mixed, bad, table_wrong, wrong, accepted);
  return bad || table_wrong || wrong || accepted || mixed == 0 || mixed == rows ? 1 : 0;
}
