// The constant tables of the log-mel kernels: the sizes and layouts the kernels and the host builder (logmel_host.cpp) share, and the host
// image of the four tables.  Plain C++: no HIP header is needed to include this file (tools/logmel_host_check.cpp builds it alone).
#pragma once
#include <vector>

#include "logmel_quad_tables.h"

constexpr int NFFT = 400, HOP = 160, NFREQ = 201, NMEL = 80;

// logmel_main (logmel_dft.hip): folded basis [208][416] = w[n] cos | w[n] sin, rows 201..207 zero; mel filters transposed [208][80]
constexpr int BASIS_ROWS = 208, BASIS_COLS = 416, MELFILT_ROWS = 208;

// logmel_fft (logmel_fft.hip), resident in LDS: W200 (200 complex) | hann[0..200] (+3 pad) | W400 (201 complex) | mel: (first bin, first weight) x 81 | weights
// (the power spectrum overwrites the Z rows in place -- each thread holds its 26 values across a barrier -- so samples + Z + tables
// fit 80 KiB: two workgroups per CU)
constexpr int XTAB_A = 400 + 204, XTAB_P = 402, XTAB_M_MAX = 604;
constexpr int XTAB_OFF_P = XTAB_A, XTAB_OFF_M = XTAB_A + XTAB_P, XTAB = XTAB_A + XTAB_P + XTAB_M_MAX;

// logmel_quad (logmel_quad.hip): window | W200 per lane | W400 per lane | mel weights per lane [slot][4 lanes] (floats)
constexpr int QLOG_SHIFT = 16;  // the mel weights carry 2^16: see the logarithm at the end of the kernel's mel phase
constexpr int QTAB_WIN = 0, QTAB_TW200 = 400, QTAB_TW400 = 800, QTAB_MEL = 1200, QTAB = 1200 + 4 * QMEL_SLOTS;

struct LogmelHostTables {
  std::vector<float> basis;     // [BASIS_ROWS][BASIS_COLS]
  std::vector<float> melfilt;   // [MELFILT_ROWS][NMEL]
  std::vector<float> fft_tab;   // [XTAB]
  std::vector<float> quad_tab;  // [QTAB]
  int mel_words = 0;            // used words of fft_tab's mel part (162 + non-zeros)
  int mel_span = 0;             // taps of the widest filter
};
// Fills every table in double precision, rounded once to f32.  OASR_OK, or OASR_ESTATE (error text set) when the filterbank does not fit the
// LDS slot of logmel_fft or is not the one logmel_quad_tables.h was generated from.
int logmel_build_tables(LogmelHostTables& t);
