// Stand-alone host check of the SpecAugment rule the device kernel shares with the CPU (specaug_core.h, specaug_host.cpp); built with
// -fsanitize=address,undefined by `make specaug-host-check`.  It compares oasr_spec_augment_plan with the rule written out again here and
// with known answers, over a sweep of shapes, policies, seeds and stream ids, into interval lists of exactly the size the call may write
// (the sanitizer guards their ends), and checks that bad arguments are refused.  Exit status 0 = everything agreed.
#include <memory>

#include "../../../include/oasr.h"
#include "host_check.h"

// the rule of include/oasr.h for one kind, written from its text
static void expect(uint64_t h, uint64_t kind, int n, int64_t W, int64_t L, int32_t* iv) {
  if (W > L) W = L;
  for (int i = 0; i < n; ++i) {
    const uint64_t width = mix(h ^ ((kind << 16) | ((uint64_t)i << 1))) % (uint64_t)(W + 1);
    const uint64_t start = mix(h ^ ((kind << 16) | ((uint64_t)i << 1) | 1)) % ((uint64_t)L - width + 1);
    iv[2 * i] = (int32_t)start, iv[2 * i + 1] = (int32_t)width;
  }
}

static int check(const oasr_specaug& p, uint64_t seed, uint64_t clip, int n_mels, int T) {
  std::unique_ptr<int32_t[]> f(new int32_t[2 * p.freq_masks]), t(new int32_t[2 * p.time_masks]);
  std::unique_ptr<int32_t[]> wf(new int32_t[2 * p.freq_masks]), wt(new int32_t[2 * p.time_masks]);
  if (oasr_spec_augment_plan(&p, seed, clip, n_mels, T, f.get(), t.get()) != 0) return 1;
  const uint64_t h = mix(mix(seed) ^ clip);
  expect(h, 1, p.freq_masks, p.freq_width, n_mels, wf.get());
  expect(h, 2, p.time_masks, p.time_width, T, wt.get());
  int bad = 0;
  for (int i = 0; i < p.freq_masks; ++i) {
    const int s = f[2 * i], w = f[2 * i + 1];
    bad += s != wf[2 * i] || w != wf[2 * i + 1] || s < 0 || w < 0 || s + w > n_mels || w > p.freq_width;
  }
  for (int i = 0; i < p.time_masks; ++i) {
    const int s = t[2 * i], w = t[2 * i + 1];
    bad += s != wt[2 * i] || w != wt[2 * i + 1] || s < 0 || w < 0 || s + w > T || w > p.time_width;
  }
  return bad != 0;
}

struct Known {
  uint64_t seed, clip;
  int time_width, n_mels, T;
  int32_t freq[4], time[4];
};

int main() {
  static const oasr_specaug policies[] = {{2, 27, 2, 100, 0.f}, {1, 27, 1, 100, 0.f},        {0, 27, 0, 100, 0.f},       {2, 0, 2, 0, 0.f},
                                          {8, 27, 8, 100, 0.f}, {3, 1000, 5, 100000, -1.5f}, {8, 0x7fffffff, 8, 0x7fffffff, 0.f}, {0, 0, 8, 3, 0.f}};
  static const int mels[] = {1, 2, 5, 80, 128}, frames[] = {1, 2, 37, 257, 1000, 3000, 0x7fffffff};
  static const uint64_t seeds[] = {0, 1, 42, 1234, (1ull << 63) + 5, ~0ull};
  static const uint64_t clips[] = {0, 7, (1ull << 32) - 2, (1ull << 32) - 1, 1ull << 32, (1ull << 40) + 3, 1ull << 63, ~0ull};
  int bad = 0, n = 0;
  for (const auto& p : policies)
    for (int m : mels)
      for (int T : frames)
        for (uint64_t s : seeds)
          for (uint64_t c : clips) {
            const int r = check(p, s, c, m, T);
            if (r) fprintf(stderr, "plan mismatch: policy %d/%d/%d/%d n_mels=%d T=%d seed=%llu clip=%llu\n", p.freq_masks, p.freq_width,
                           p.time_masks, p.time_width, m, T, (unsigned long long)s, (unsigned long long)c);
            bad += r, ++n;
          }
  // known answers (LD; the last row with the time width capped at 3)
  static const Known known[] = {{0, 0, 100, 80, 3000, {0, 11, 65, 4}, {2666, 25, 2253, 54}},
                                {1234, 7, 100, 80, 3000, {52, 19, 11, 22}, {2549, 28, 1021, 78}},
                                {(1ull << 63) + 5, (1ull << 40) + 3, 100, 80, 3000, {44, 22, 40, 14}, {300, 67, 2392, 62}},
                                {0, 0, 3, 80, 37, {0, 11, 65, 4}, {2, 2, 7, 1}}};
  int wrong = 0;
  for (const auto& k : known) {
    const oasr_specaug p = {2, 27, 2, k.time_width, 0.f};
    int32_t f[4], t[4];
    int w = oasr_spec_augment_plan(&p, k.seed, k.clip, k.n_mels, k.T, f, t) != 0;
    for (int e = 0; e < 4; ++e) w |= f[e] != k.freq[e] || t[e] != k.time[e];
    wrong += w;
  }
  if (wrong) fprintf(stderr, "known answers: %d of 4 rows wrong\n", wrong);
  // refusals, before anything is written
  int32_t iv[16] = {0};
  const oasr_specaug ok = {2, 27, 2, 100, 0.f};
  static const oasr_specaug refused[] = {{-1, 27, 2, 100, 0.f}, {2, -1, 2, 100, 0.f}, {2, 27, -1, 100, 0.f}, {2, 27, 2, -1, 0.f},
                                         {9, 27, 2, 100, 0.f},  {2, 27, 9, 100, 0.f}};
  int accepted = 0;
  for (const auto& p : refused) accepted += oasr_spec_augment_plan(&p, 0, 0, 80, 3000, iv, iv) == 0;
  accepted += oasr_spec_augment_plan(nullptr, 0, 0, 80, 3000, iv, iv) == 0;
  accepted += oasr_spec_augment_plan(&ok, 0, 0, 80, 3000, nullptr, iv) == 0;
  accepted += oasr_spec_augment_plan(&ok, 0, 0, 80, 3000, iv, nullptr) == 0;
  accepted += oasr_spec_augment_plan(&ok, 0, 0, 0, 3000, iv, iv) == 0;
  accepted += oasr_spec_augment_plan(&ok, 0, 0, 80, 0, iv, iv) == 0;
  for (int e = 0; e < 16; ++e) accepted += iv[e] != 0;
  if (accepted) fprintf(stderr, "bad arguments: %d accepted or written through\n", accepted);
  printf("specaug_host_check: %d plans, %d mismatches; known answers: %d of 4 wrong; bad arguments accepted: %d\n", n, bad, wrong, accepted);
  return bad || wrong || accepted ? 1 : 0;
}
