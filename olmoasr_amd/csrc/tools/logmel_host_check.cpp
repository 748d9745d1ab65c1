// Stand-alone host check of the log-mel tables (logmel_tables.h, logmel_host.cpp); built with -fsanitize=address,undefined by
// `make logmel-host-check`.  It builds the tables and checks what otherwise only a first GPU call could notice: the zero rows and columns of
// the folded basis, that the sparse filter rows of the LDS FFT kernel are the dense filterbank bit for bit and fit their LDS slot, that every
// per-lane mel weight of the quad kernel sits at the slot and lane logmel_quad_tables.h gives it and is zero elsewhere, and that the window
// and twiddle tables are their formulas, evaluated again here.  Exit status 0 = everything agreed.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "../../../include/oasr.h"
#include "../logmel_tables.h"

void oasr_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
}

static bool same(float a, float b) { return memcmp(&a, &b, sizeof(float)) == 0; }

int main() {
  const double PI = 3.14159265358979323846;
  LogmelHostTables t;
  if (logmel_build_tables(t) != OASR_OK) return 1;
  std::vector<float> fb((size_t)NMEL * NFREQ);
  oasr_mel_filterbank(fb.data());
  int sizes = t.basis.size() != (size_t)BASIS_ROWS * BASIS_COLS || t.melfilt.size() != (size_t)MELFILT_ROWS * NMEL ||
              t.fft_tab.size() != (size_t)XTAB || t.quad_tab.size() != (size_t)QTAB;
  if (sizes) {
    fprintf(stderr, "table sizes wrong\n");
    return 1;
  }
  int nonzero = 0, edge = 0;
  for (int m = 0; m < NMEL; ++m)
    for (int f = 0; f < NFREQ; ++f) nonzero += fb[m * NFREQ + f] != 0.f, edge += (f == 0 || f == NFREQ - 1) && fb[m * NFREQ + f] != 0.f;

  // ---- the folded basis: rows past n = 200 and the sine of the two samples that are their own mirror carry nothing
  int basis_bad = 0;
  for (int j = NFFT / 2 + 1; j < BASIS_ROWS; ++j)
    for (int c = 0; c < BASIS_COLS; ++c) basis_bad += t.basis[(size_t)j * BASIS_COLS + c] != 0.f;
  for (int j : {0, NFFT / 2})
    for (int c = BASIS_COLS / 2; c < BASIS_COLS; ++c) basis_bad += t.basis[(size_t)j * BASIS_COLS + c] != 0.f;
  for (int f = 0; f < MELFILT_ROWS; ++f)
    for (int m = 0; m < NMEL; ++m) basis_bad += !same(t.melfilt[(size_t)f * NMEL + m], f < NFREQ ? fb[m * NFREQ + f] : 0.f);
  if (basis_bad) fprintf(stderr, "folded basis / dense filters: %d words wrong\n", basis_bad);

  // ---- the sparse rows of logmel_fft, read the way the kernel reads them: (first bin, first weight) of filter m, taps up to filter m + 1's
  int sparse_bad = 0, covered = 0, span = 0;
  {
    int idx[2 * (NMEL + 1)];
    memcpy(idx, &t.fft_tab[XTAB_OFF_M], sizeof(idx));
    const float* val = &t.fft_tab[XTAB_OFF_M + 2 * (NMEL + 1)];
    std::vector<float> dense((size_t)NMEL * NFREQ, 0.f);
    for (int m = 0; m < NMEL; ++m) {
      const int lo = idx[2 * m], p0 = idx[2 * m + 1], cnt = idx[2 * m + 3] - p0;
      if (lo < 0 || cnt < 1 || lo + cnt > NFREQ || p0 < 0 || 2 * (NMEL + 1) + p0 + cnt > t.mel_words) {
        ++sparse_bad;
        continue;
      }
      span = cnt > span ? cnt : span;
      for (int i = 0; i < cnt; ++i) dense[(size_t)m * NFREQ + lo + i] = val[p0 + i], covered += val[p0 + i] != 0.f;
    }
    sparse_bad += memcmp(dense.data(), fb.data(), sizeof(float) * dense.size()) != 0;
    sparse_bad += covered != nonzero || nonzero != 391 || span != t.mel_span;  // (391: the generator's own filterbank, scripts/gen_logmel_quad_tables.py, has as many)
    sparse_bad += t.mel_words > XTAB_M_MAX || t.mel_words != 2 * (NMEL + 1) + idx[2 * NMEL + 1];
    if (sparse_bad) fprintf(stderr, "sparse filter rows: %d checks failed (covered %d of %d non-zeros, %d words)\n", sparse_bad, covered, nonzero, t.mel_words);
  }

  // ---- the per-lane mel weights of logmel_quad: slot QMEL_OFF[m] + sl, lane l holds bin k = K1[l] + 4 (QMEL_K2LO[m] + sl) of filter m
  int quad_bad = 0, quad_nonzero = 0;
  {
    const int K1[4] = {0, 2, 1, 3};
    int next = 0;
    for (int m = 0; m < NMEL; ++m) {
      quad_bad += QMEL_OFF[m] != next || QMEL_NSLOT[m] < 1 || QMEL_K2LO[m] + QMEL_NSLOT[m] > 50;
      next += QMEL_NSLOT[m];
      for (int sl = 0; sl < QMEL_NSLOT[m]; ++sl)
        for (int l = 0; l < 4; ++l) {
          const int k = K1[l] + 4 * (QMEL_K2LO[m] + sl);
          const float got = t.quad_tab[(size_t)QTAB_MEL + 4 * (QMEL_OFF[m] + sl) + l];
          const float w = k <= 199 ? fb[m * NFREQ + k] : 0.f;
          quad_bad += !same(got, ldexpf(0.25f * w, QLOG_SHIFT)) || ((k > 199 || w == 0.f) && got != 0.f);
          quad_nonzero += got != 0.f;
        }
    }
    quad_bad += next != QMEL_SLOTS || quad_nonzero != nonzero || edge != 0;  // (every non-zero weight has a slot; bins 0 and 200 have none)
    if (quad_bad) fprintf(stderr, "quad mel weights: %d checks failed (%d non-zero of %d)\n", quad_bad, quad_nonzero, nonzero);
  }

  // ---- window and twiddles, from their formulas
  int tw_bad = 0;
  for (int j = 0; j < 200; ++j) {
    tw_bad += !same(t.fft_tab[2 * j], (float)cos(2.0 * PI * j / 200.0)) || !same(t.fft_tab[2 * j + 1], (float)(-sin(2.0 * PI * j / 200.0)));
  }
  for (int j = 0; j <= 200; ++j) tw_bad += !same(t.fft_tab[400 + j], (float)(0.5 - 0.5 * cos(2.0 * PI * j / NFFT)));
  for (int k = 0; k <= 200; ++k) {
    tw_bad += !same(t.fft_tab[XTAB_OFF_P + 2 * k], (float)cos(2.0 * PI * k / 400.0));
    tw_bad += !same(t.fft_tab[XTAB_OFF_P + 2 * k + 1], (float)(-sin(2.0 * PI * k / 400.0)));
  }
  for (int s = 0; s < NFFT; ++s) tw_bad += !same(t.quad_tab[QTAB_WIN + s], (float)(0.5 - 0.5 * cos(2.0 * PI * s / NFFT)));
  for (int m = 0; m < 50; ++m)
    for (int l = 0; l < 4; ++l) {
      const int k1 = ((l & 1) << 1) | (l >> 1);              // bit-reversed lane
      const double sgn = ((l >> 1) ^ (l & 1)) ? -1.0 : 1.0;  // sg1 sg2 of the lane
      const int e200 = (m * k1) % 200, e400 = k1 + 4 * m;
      const float* w2 = &t.quad_tab[QTAB_TW200 + 2 * (4 * m + l)];
      const float* w4 = &t.quad_tab[QTAB_TW400 + 2 * (4 * m + l)];
      tw_bad += !same(w2[0], (float)(sgn * cos(2.0 * PI * e200 / 200.0))) || !same(w2[1], (float)(-sgn * sin(2.0 * PI * e200 / 200.0)));
      tw_bad += !same(w4[0], (float)cos(2.0 * PI * e400 / 400.0)) || !same(w4[1], (float)(-sin(2.0 * PI * e400 / 400.0)));
    }
  if (tw_bad) fprintf(stderr, "window / twiddle tables: %d words wrong\n", tw_bad);

  printf("logmel_host_check: %d filter non-zeros, %d mel words (slot %d), span %d, %d quad slots; basis words wrong: %d; sparse row checks failed: %d; "
         "quad weight checks failed: %d; window / twiddle words wrong: %d\n",
         nonzero, t.mel_words, XTAB_M_MAX, t.mel_span, QMEL_SLOTS, basis_bad, sparse_bad, quad_bad, tw_bad);
  return basis_bad || sparse_bad || quad_bad || tw_bad ? 1 : 0;
}
