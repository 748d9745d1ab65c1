// The host half of the log-mel front end: the slaney filterbank (oasr_mel_filterbank) and the constant tables of the three kernels
// (logmel_tables.h), built in double precision and rounded once to f32.  Plain C++ (no HIP, no GPU call): it loads where there is no
// device and builds alone under a host sanitizer (tools/logmel_host_check.cpp).
#include <math.h>
#include <string.h>

#include "../../include/oasr.h"
#include "logmel_tables.h"

void oasr_set_error(const char* fmt, ...);

static double hz_to_mel(double f) {
  const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
  return f >= min_log_hz ? min_log_mel + log(f / min_log_hz) / logstep : f / f_sp;
}
static double mel_to_hz(double m) {
  const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
  return m >= min_log_mel ? min_log_hz * exp(logstep * (m - min_log_mel)) : f_sp * m;
}

// Slaney-scale / slaney-normalised filterbank == librosa.filters.mel(sr=16000, n_fft=400, n_mels=80),
// the content of whisper's assets/mel_filters.npz.  Exported so the host mirror can hand it to tests.
extern "C" int oasr_mel_filterbank(float* out /*[80][201]*/) {
  const int sr = 16000;
  double pts[NMEL + 2];
  const double m0 = hz_to_mel(0.0), m1 = hz_to_mel(sr / 2.0);
  for (int i = 0; i < NMEL + 2; ++i) pts[i] = mel_to_hz(m0 + (m1 - m0) * i / (NMEL + 1));
  for (int m = 0; m < NMEL; ++m) {
    const double enorm = 2.0 / (pts[m + 2] - pts[m]);
    for (int f = 0; f < NFREQ; ++f) {
      const double hz = (sr / 2.0) * f / (NFREQ - 1);
      const double lower = (hz - pts[m]) / (pts[m + 1] - pts[m]);
      const double upper = (pts[m + 2] - hz) / (pts[m + 2] - pts[m + 1]);
      double w = lower < upper ? lower : upper;
      if (w < 0) w = 0;
      out[m * NFREQ + f] = (float)(w * enorm);
    }
  }
  return OASR_OK;
}

int logmel_build_tables(LogmelHostTables& t) {
  const double PI = 3.14159265358979323846;
  std::vector<float> fb((size_t)NMEL * NFREQ);
  oasr_mel_filterbank(fb.data());
  int lo[NMEL], hi[NMEL];  // first and last non-zero bin of every filter (hi < lo: none)
  for (int m = 0; m < NMEL; ++m) {
    lo[m] = NFREQ, hi[m] = -1;
    for (int f = 0; f < NFREQ; ++f)
      if (fb[m * NFREQ + f] != 0.f) {
        lo[m] = f < lo[m] ? f : lo[m];
        hi[m] = f;
      }
  }

  // ---- logmel_main: folded basis (rows 201..207 stay zero) and the transposed dense filterbank
  t.basis.assign((size_t)BASIS_ROWS * BASIS_COLS, 0.f);
  for (int j = 0; j <= NFFT / 2; ++j) {
    const double w = 0.5 - 0.5 * cos(2.0 * PI * j / NFFT);  // torch.hann_window(400), periodic: w[400 - j] == w[j]
    for (int f = 0; f < NFREQ; ++f) {
      const int ph = (int)(((long)j * f) % NFFT);  // exact argument reduction
      const double ang = 2.0 * PI * ph / NFFT;
      t.basis[(size_t)j * BASIS_COLS + f] = (float)(w * cos(ang));
      if (j >= 1 && j < NFFT / 2) t.basis[(size_t)j * BASIS_COLS + BASIS_COLS / 2 + f] = (float)(w * sin(ang));
    }
  }
  t.melfilt.assign((size_t)MELFILT_ROWS * NMEL, 0.f);
  for (int m = 0; m < NMEL; ++m)
    for (int f = 0; f < NFREQ; ++f) t.melfilt[(size_t)f * NMEL + m] = fb[m * NFREQ + f];

  // ---- logmel_fft: W200, hann[0..200], W400, the filters as sparse rows
  t.fft_tab.assign((size_t)XTAB, 0.f);
  for (int j = 0; j < 200; ++j) {
    t.fft_tab[(size_t)2 * j] = (float)cos(2.0 * PI * j / 200.0);
    t.fft_tab[(size_t)2 * j + 1] = (float)(-sin(2.0 * PI * j / 200.0));
  }
  for (int j = 0; j <= 200; ++j) t.fft_tab[(size_t)400 + j] = (float)(0.5 - 0.5 * cos(2.0 * PI * j / NFFT));
  for (int k = 0; k <= 200; ++k) {
    t.fft_tab[(size_t)XTAB_OFF_P + 2 * k] = (float)cos(2.0 * PI * k / 400.0);
    t.fft_tab[(size_t)XTAB_OFF_P + 2 * k + 1] = (float)(-sin(2.0 * PI * k / 400.0));
  }
  std::vector<int> idx((size_t)2 * (NMEL + 1), 0);  // (first bin, first weight) per filter; row 80 carries the total
  std::vector<float> val;
  t.mel_span = 0;
  for (int m = 0; m < NMEL; ++m) {
    const int l = hi[m] < lo[m] ? 0 : lo[m], h = hi[m] < lo[m] ? 0 : hi[m];
    idx[(size_t)2 * m] = l;
    idx[(size_t)2 * m + 1] = (int)val.size();
    t.mel_span = h - l + 1 > t.mel_span ? h - l + 1 : t.mel_span;
    for (int f = l; f <= h; ++f) val.push_back(fb[m * NFREQ + f]);
  }
  idx[(size_t)2 * NMEL + 1] = (int)val.size();
  if (idx.size() + val.size() > (size_t)XTAB_M_MAX) {
    oasr_set_error("log-mel: sparse filterbank (%zu words) exceeds its LDS slot", idx.size() + val.size());
    return OASR_ESTATE;
  }
  memcpy(&t.fft_tab[(size_t)XTAB_OFF_M], idx.data(), idx.size() * sizeof(int));
  memcpy(&t.fft_tab[(size_t)XTAB_OFF_M + idx.size()], val.data(), val.size() * sizeof(float));
  t.mel_words = (int)(idx.size() + val.size());

  // ---- logmel_quad: lane l of a quad holds k1 = {0, 2, 1, 3}[l] (bit-reversed) after the cross-lane radix-4
  const int K1[4] = {0, 2, 1, 3};
  t.quad_tab.assign((size_t)QTAB, 0.f);
  for (int s = 0; s < NFFT; ++s) t.quad_tab[(size_t)QTAB_WIN + s] = (float)(0.5 - 0.5 * cos(2.0 * PI * s / NFFT));
  for (int m = 0; m < 50; ++m)
    for (int l = 0; l < 4; ++l) {
      const int e200 = (m * K1[l]) % 200, e400 = K1[l] + 4 * m;  // W200^(m k1); W400^(k1 + 4 k2) with k2 = m
      const double sgn = (l == 1 || l == 2) ? -1.0 : 1.0;       // sg1 sg2 of lane l: the sign its one-instruction butterflies leave (logmel_quad.hip)
      t.quad_tab[(size_t)QTAB_TW200 + 2 * (4 * m + l)] = (float)(sgn * cos(2.0 * PI * e200 / 200.0));
      t.quad_tab[(size_t)QTAB_TW200 + 2 * (4 * m + l) + 1] = (float)(-sgn * sin(2.0 * PI * e200 / 200.0));
      t.quad_tab[(size_t)QTAB_TW400 + 2 * (4 * m + l)] = (float)cos(2.0 * PI * e400 / 400.0);
      t.quad_tab[(size_t)QTAB_TW400 + 2 * (4 * m + l) + 1] = (float)(-sin(2.0 * PI * e400 / 400.0));
    }
  for (int m = 0; m < NMEL; ++m) {
    // the compile-time slot structure (logmel_quad_tables.h, generated from the same formulas) must describe THIS filterbank
    if (hi[m] < lo[m] || lo[m] / 4 != QMEL_K2LO[m] || hi[m] / 4 - lo[m] / 4 + 1 != QMEL_NSLOT[m] || hi[m] > 199) {
      oasr_set_error("log-mel: filter %d spans bins %d..%d, logmel_quad_tables.h says k2 %d + %d: regenerate (scripts/gen_logmel_quad_tables.py)",
                     m, lo[m], hi[m], QMEL_K2LO[m], QMEL_NSLOT[m]);
      return OASR_ESTATE;
    }
    for (int sl = 0; sl < QMEL_NSLOT[m]; ++sl)
      for (int l = 0; l < 4; ++l) {
        const int k = K1[l] + 4 * (QMEL_K2LO[m] + sl);
        t.quad_tab[(size_t)QTAB_MEL + 4 * (QMEL_OFF[m] + sl) + l] = k <= 199 ? (float)(1 << QLOG_SHIFT) * 0.25f * fb[m * NFREQ + k] : 0.f;  // (P holds 4 |X|^2; 2^QLOG_SHIFT: logmel_quad.hip)
      }
  }
  return OASR_OK;
}
