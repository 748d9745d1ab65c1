// What the stand-alone host checks of the augmentation operators (tools/{specaug,speed,noise,reverb}_host_check.cpp) have in common: the
// library's error sink, the stream's mixing function restated, and a small generator of test samples.  The restatement of mix is separate
// text from draw_core.h on purpose: the checks hold the library's draws to it.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

void oasr_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
}

static uint64_t mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// a sample in [-amp, amp]; rng_state: the check's own seed
static uint64_t rng_state;
static inline int16_t rnd16(int amp) { return (int16_t)((int64_t)(mix(++rng_state) % (uint64_t)(2 * amp + 1)) - amp); }
