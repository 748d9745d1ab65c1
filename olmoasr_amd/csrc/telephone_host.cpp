// The host half of the telephone channel (include/oasr.h at oasr_telephone): the library's two tap tables (built once, read by the kernel's
// launcher and by the twin alike), oasr_telephone_tables, oasr_telephone_plan, oasr_telephone_quantize_host and oasr_telephone_host -- the
// twin of telephone.hip from the same text (telephone_core.h).  Plain C++ (no HIP, no GPU call), so it serves where there is no device and
// builds alone under a host sanitizer (tools/telephone_host_check.cpp).
#include <string.h>

#include <vector>

#include "../../include/oasr.h"
#include "telephone_core.h"

void oasr_set_error(const char* fmt, ...);

static_assert(OASR_TELEPHONE_MAX_CODECS == TEL_MAX_CODECS, "include/oasr.h and telephone_core.h disagree");
static_assert(OASR_TELEPHONE_LINEAR == TEL_LINEAR && OASR_TELEPHONE_MULAW == TEL_MULAW && OASR_TELEPHONE_ALAW == TEL_ALAW,
              "include/oasr.h and telephone_core.h disagree");

const TelTables* tel_tables_cached() {
  struct Built {
    TelTables t;
    bool ok;
    Built() {
      tel_build_tables(t.h, t.u);
      ok = tel_tables_bounded(t.h, t.u);
    }
  };
  static const Built built;  // (initialised once, under the language's own lock)
  return built.ok ? &built.t : nullptr;
}

static const TelTables* tables_or_error(const char* who) {
  const TelTables* t = tel_tables_cached();
  if (!t) oasr_set_error("%s: the tap tables miss the bound of the 32-bit partial sums (a group's sum of |tap| above 65535)", who);
  return t;
}

extern "C" int oasr_telephone_tables(int32_t* h, int32_t* u) {
  const TelTables* t = tables_or_error("oasr_telephone_tables");
  if (!t) return OASR_EINVAL;
  if (h) memcpy(h, t->h, sizeof(t->h));
  if (u) memcpy(u, t->u, sizeof(t->u));
  return OASR_OK;
}

extern "C" int oasr_telephone_plan(const struct oasr_telephone* p, uint64_t seed, uint64_t clip, int* drawn, int* codec) {
  const char* why = p ? tel_policy_error(p->prob_q16, p->n_codecs, p->codecs, p->bandpass) : "null policy";
  if (why) {
    oasr_set_error("oasr_telephone_plan: %s", why);
    return OASR_EINVAL;
  }
  const TelPlan pl = tel_plan(seed, clip, p->prob_q16, p->n_codecs);
  if (drawn) *drawn = pl.drawn ? 1 : 0;
  if (codec) *codec = tel_codec_at(p->codecs, pl.choice);
  return OASR_OK;
}

extern "C" int oasr_telephone_quantize_host(const int16_t* in, int16_t* out, int64_t n, int codec) {
  if (n < 0 || (n > 0 && (!in || !out)) || codec < TEL_LINEAR || codec > TEL_ALAW) {
    oasr_set_error("oasr_telephone_quantize_host: n = %lld below 0, a null buffer, or codec = %d outside {0, 1, 2}", (long long)n, codec);
    return OASR_EINVAL;
  }
  for (int64_t i = 0; i < n; ++i) out[i] = tel_quantize(in[i], codec);
  return OASR_OK;
}

extern "C" int oasr_telephone_host(const oasr_telephone_args* a) {
  const char* why = tel_args_error(a);
  if (why) {
    oasr_set_error("oasr_telephone_host: %s", why);
    return OASR_EINVAL;
  }
  const TelTables* t = tables_or_error("oasr_telephone_host");
  if (!t) return OASR_EINVAL;
  std::vector<int16_t> c;
  for (int b = 0; b < a->B; ++b) {
    const int nv = a->n_valid[b];
    const int codec = tel_row_codec(a->seed, a->first_clip + (uint64_t)b, a->policy.prob_q16, a->policy.n_codecs, a->policy.codecs, nv, a->N);
    const int16_t* x = a->pcm_in + (size_t)b * (size_t)a->ld_in;
    int16_t* y = a->pcm_out + (size_t)b * (size_t)a->ld_out;
    if (a->codec_out) a->codec_out[b] = codec;
    if (codec < 0) {
      pcm_copy_row(y, x, 0, a->N);
      continue;
    }
    const int M = (nv + 1) / 2;
    c.resize((size_t)M);
    for (int m = 0; m < M; ++m) c[m] = tel_quantize(tel_decimated(x, nv, t->h, a->policy.bandpass, m), codec);
    for (int m = 0; m < M; ++m) {
      y[2 * m] = c[m];
      if (2 * m + 1 < nv) y[2 * m + 1] = tel_interpolated(c.data(), M, t->u, m);
    }
    pcm_copy_row(y, x, nv, a->N);
  }
  return OASR_OK;
}
