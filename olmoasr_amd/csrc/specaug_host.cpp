// oasr_spec_augment_plan (include/oasr.h): the host twin of specaug.hip -- the (start, width) intervals the kernel derives for one clip,
// from the same text (specaug_core.h).  Plain C++ (no HIP, no GPU call), so it serves where there is no device and builds alone under a
// host sanitizer (tools/specaug_host_check.cpp).
#include "../../include/oasr.h"
#include "specaug_core.h"

void oasr_set_error(const char* fmt, ...);

static_assert(OASR_SPECAUG_MAX_MASKS == SPECAUG_MAX_MASKS, "include/oasr.h and specaug_core.h disagree");

extern "C" int oasr_spec_augment_plan(const oasr_specaug* p, uint64_t seed, uint64_t clip, int n_mels, int T, int32_t* freq_iv,
                                      int32_t* time_iv) {
  if (!p || !freq_iv || !time_iv) {
    oasr_set_error("oasr_spec_augment_plan: null policy or interval list");
    return OASR_EINVAL;
  }
  const char* why = specaug_policy_error(p->freq_masks, p->freq_width, p->time_masks, p->time_width);
  if (why) {
    oasr_set_error("oasr_spec_augment_plan: %s (freq %d x <= %d, time %d x <= %d)", why, p->freq_masks, p->freq_width, p->time_masks,
                   p->time_width);
    return OASR_EINVAL;
  }
  if (n_mels < 1 || T < 1) {
    oasr_set_error("oasr_spec_augment_plan: n_mels = %d and T = %d must be >= 1", n_mels, T);
    return OASR_EINVAL;
  }
  const uint64_t h = draw_clip_hash(seed, clip);
  for (int i = 0; i < p->freq_masks; ++i) {
    int start, width;
    specaug_interval(h, DRAW_FREQ_MASK, i, p->freq_width, n_mels, &start, &width);
    freq_iv[2 * i] = start, freq_iv[2 * i + 1] = width;
  }
  for (int i = 0; i < p->time_masks; ++i) {
    int start, width;
    specaug_interval(h, DRAW_TIME_MASK, i, p->time_width, T, &start, &width);
    time_iv[2 * i] = start, time_iv[2 * i + 1] = width;
  }
  return OASR_OK;
}
