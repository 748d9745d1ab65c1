// Stand-alone host check of the edit-distance rule the device kernel shares with the CPU (editdist_core.h, editdist_host.cpp); built with
// -fsanitize=address,undefined by `make editdist-host-check`.  It compares oasr_edit_counts_host with a plain full-matrix DP written out
// again here -- explicit (S, D, I) triples, no packing -- and with the known answers of include/oasr.h, over exhaustive binary pairs, seeded
// random pairs and the longest lengths, in buffers of exactly the size the call may touch (the sanitizer guards their ends), and checks
// that bad arguments are refused before anything is written.  Exit status 0 = everything agreed.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../../include/oasr.h"

void oasr_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
}

struct Sdi {
  int s, d, i;
  int cost() const { return s + d + i; }
};

// the rule of include/oasr.h, written from its text: the whole (n + 1) x (m + 1) table
static void expect(const std::vector<int32_t>& h, const std::vector<int32_t>& r, int32_t* out) {
  const int n = (int)h.size(), m = (int)r.size();
  std::vector<Sdi> t((size_t)(n + 1) * (m + 1));
  auto at = [&](int i, int j) -> Sdi& { return t[(size_t)i * (m + 1) + j]; };
  for (int j = 0; j <= m; ++j) at(0, j) = Sdi{0, j, 0};
  for (int i = 0; i <= n; ++i) at(i, 0) = Sdi{0, 0, i};
  for (int i = 1; i <= n; ++i)
    for (int j = 1; j <= m; ++j) {
      const int sub = h[i - 1] != r[j - 1];
      const int cd = at(i - 1, j - 1).cost() + sub, cl = at(i, j - 1).cost() + 1, cu = at(i - 1, j).cost() + 1;
      Sdi c;
      if (cd <= cl && cd <= cu) c = at(i - 1, j - 1), c.s += sub;
      else if (cl <= cu) c = at(i, j - 1), c.d += 1;
      else c = at(i - 1, j), c.i += 1;
      at(i, j) = c;
    }
  const Sdi e = at(n, m);
  out[0] = e.s, out[1] = e.d, out[2] = e.i, out[3] = m - e.s - e.d;
}

static int g_pairs = 0;

// one pair through the twin, in vectors of exactly hyp_len / ref_len tokens
static int check(const std::vector<int32_t>& h, const std::vector<int32_t>& r) {
  const int32_t n = (int32_t)h.size(), m = (int32_t)r.size();
  int32_t got[4] = {-7, -7, -7, -7}, want[4];
  oasr_edit_args a = {};
  a.hyp = h.data(), a.ref = r.data(), a.hyp_len = &n, a.ref_len = &m, a.out = got;
  a.ld_hyp = n, a.ld_ref = m, a.B = 1, a.Lh = n, a.Lr = m;
  ++g_pairs;
  if (oasr_edit_counts_host(&a) != 0) return 1;
  expect(h, r, want);
  int bad = 0;
  for (int e = 0; e < 4; ++e) bad |= got[e] != want[e] || got[e] < 0;
  bad |= got[0] + got[1] + got[3] != m || got[0] + got[2] + got[3] != n;
  if (bad) fprintf(stderr, "mismatch at lengths %d / %d: got (%d, %d, %d, %d), want (%d, %d, %d, %d)\n", n, m, got[0], got[1], got[2], got[3], want[0],
                   want[1], want[2], want[3]);
  return bad;
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t mod) {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_rng >> 33) % mod;
}
static std::vector<int32_t> rand_seq(int len, int alphabet) {
  std::vector<int32_t> v(len);
  for (auto& x : v) x = (int32_t)rnd(alphabet);
  return v;
}

struct Known {
  std::vector<int32_t> hyp, ref;
  int32_t sdih[4];
};

int main() {
  int bad = 0;
  // every pair of binary sequences of length 0 .. 5
  std::vector<std::vector<int32_t>> bin;
  for (int len = 0; len <= 5; ++len)
    for (int bits = 0; bits < (1 << len); ++bits) {
      std::vector<int32_t> v(len);
      for (int k = 0; k < len; ++k) v[k] = (bits >> k) & 1;
      bin.push_back(v);
    }
  for (const auto& h : bin)
    for (const auto& r : bin) bad += check(h, r);
  // seeded random pairs
  static const int alphabets[] = {2, 3, 50};
  for (int t = 0; t < 300; ++t) bad += check(rand_seq(rnd(41), alphabets[t % 3]), rand_seq(rnd(41), alphabets[t % 3]));
  // the lengths at which a kernel would change partition, on either side
  static const int lens[] = {0, 1, 63, 64, 65, 448, 1023};
  for (int n : lens)
    for (int m : lens) bad += check(rand_seq(n, 3), rand_seq(m, 3));
  // known answers
  static const Known known[] = {{{}, {1, 2, 3}, {0, 3, 0, 0}},           {{1, 2, 3}, {}, {0, 0, 3, 0}},      {{1, 9, 3}, {1, 2, 3}, {1, 0, 0, 2}},
                                {{1, 3}, {1, 2, 3}, {0, 1, 0, 2}},       {{1, 2, 2, 3}, {1, 2, 3}, {0, 0, 1, 3}}, {{2, 1}, {1, 2}, {2, 0, 0, 0}},
                                {{1, 1, 2}, {1, 2}, {0, 0, 1, 2}},       {{0, 1, 0, 1}, {1, 0, 1, 0}, {0, 1, 1, 3}}};
  int wrong = 0;
  for (const auto& k : known) {
    int32_t want[4];
    expect(k.hyp, k.ref, want);
    int w = check(k.hyp, k.ref);
    for (int e = 0; e < 4; ++e) w |= want[e] != k.sdih[e];
    wrong += w;
  }
  if (wrong) fprintf(stderr, "known answers: %d of 8 wrong\n", wrong);
  // a batch with row strides, trailing tokens past the lengths and one guard row of output
  {
    const int B = 3, Lh = 7, Lr = 5, ldh = 9, ldr = 6;
    std::vector<int32_t> h((B - 1) * ldh + Lh), r((B - 1) * ldr + Lr), out(4 * B + 4, -7);
    for (auto& x : h) x = (int32_t)rnd(3);
    for (auto& x : r) x = (int32_t)rnd(3);
    const int32_t hl[B] = {7, 0, 4}, rl[B] = {5, 3, 0};
    oasr_edit_args a = {};
    a.hyp = h.data(), a.ref = r.data(), a.hyp_len = hl, a.ref_len = rl, a.out = out.data();
    a.ld_hyp = ldh, a.ld_ref = ldr, a.B = B, a.Lh = Lh, a.Lr = Lr;
    int w = oasr_edit_counts_host(&a) != 0;
    for (int b = 0; b < B; ++b) {
      int32_t want[4];
      expect(std::vector<int32_t>(h.begin() + b * ldh, h.begin() + b * ldh + hl[b]), std::vector<int32_t>(r.begin() + b * ldr, r.begin() + b * ldr + rl[b]),
             want);
      for (int e = 0; e < 4; ++e) w |= out[4 * b + e] != want[e];
    }
    for (int e = 0; e < 4; ++e) w |= out[4 * B + e] != -7;
    if (w) fprintf(stderr, "strided batch: wrong rows or a written guard row\n");
    bad += w, ++g_pairs;
  }
  // refusals, before anything is written
  int accepted = 0;
  {
    std::vector<int32_t> tok(1024, 1);
    int32_t out[4] = {-7, -7, -7, -7};
    struct Case {
      int32_t n, m, Lh, Lr;
    };
    static const Case cases[] = {{1024, 1, 1024, 1}, {1, 1024, 1, 1024}, {5, 1, 4, 1}, {1, 5, 1, 4}, {-1, 1, 4, 4}, {1, -1, 4, 4}};
    for (const auto& c : cases) {
      oasr_edit_args a = {};
      a.hyp = tok.data(), a.ref = tok.data(), a.hyp_len = &c.n, a.ref_len = &c.m, a.out = out;
      a.ld_hyp = c.Lh, a.ld_ref = c.Lr, a.B = 1, a.Lh = c.Lh, a.Lr = c.Lr;
      accepted += oasr_edit_counts_host(&a) == 0;
    }
    const int32_t one = 1;
    oasr_edit_args a = {};
    a.hyp = tok.data(), a.ref = tok.data(), a.hyp_len = &one, a.ref_len = &one, a.out = out;
    a.ld_hyp = 1, a.ld_ref = 1, a.B = 1, a.Lh = 1, a.Lr = 1;
    oasr_edit_args z = a;
    z.B = 0, accepted += oasr_edit_counts_host(&z) == 0;
    z = a, z.out = nullptr, accepted += oasr_edit_counts_host(&z) == 0;
    z = a, z.hyp = nullptr, accepted += oasr_edit_counts_host(&z) == 0;
    z = a, z.ref_len = nullptr, accepted += oasr_edit_counts_host(&z) == 0;
    z = a, z.B = 2, z.Lh = 4, z.ld_hyp = 3, accepted += oasr_edit_counts_host(&z) == 0;
    accepted += oasr_edit_counts_host(nullptr) == 0;
    for (int e = 0; e < 4; ++e) accepted += out[e] != -7;
    if (accepted) fprintf(stderr, "bad arguments: %d accepted or written through\n", accepted);
  }
  printf("editdist_host_check: %d pairs, %d mismatches; known answers: %d of 8 wrong; bad arguments accepted: %d; sizeof(oasr_edit_args) = %zu\n",
         g_pairs, bad, wrong, accepted, oasr_sizeof_edit_args());
  return bad || wrong || accepted ? 1 : 0;
}
