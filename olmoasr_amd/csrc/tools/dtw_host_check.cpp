// Stand-alone host check of the DTW text the device kernel shares with the CPU (dtw_core.h, dtw_host.cpp) and of the median networks
// (median_core.h); built with -fsanitize=address,undefined by `make dtw-host-check`.  It compares oasr_test_dtw_host with a plain
// full-table DTW written here, over the shapes and value families of tests/test_gpu_alignment.py, through guarded buffers, and checks every
// median network on all 0/1 inputs.  Exit status 0 = everything agreed.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../dtw_core.h"
#include "../median_core.h"

extern "C" size_t oasr_dtw_workspace_bytes(int N, int M);
extern "C" int oasr_test_dtw_host(const float* cost, int64_t ld, int N, int M, int negate, int32_t* text_indices, int32_t* time_indices,
                                  int32_t* path_len, void* workspace);
void oasr_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
}

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_state >> 33);
}
static float gauss() {  // sum of uniforms: near enough to normal for a cost matrix
  float s = 0.f;
  for (int k = 0; k < 6; ++k) s += (float)(rnd() & 0xffff) / 65536.f;
  return (s - 3.f) * 1.4142135f;
}

static void reference(const std::vector<float>& x, int N, int M, std::vector<int>& ti, std::vector<int>& tj) {
  std::vector<float> cost((size_t)(N + 1) * (M + 1), INFINITY);
  std::vector<int8_t> trace((size_t)(N + 1) * (M + 1), -1);
  cost[0] = 0.f;
  for (int j = 1; j <= M; ++j)
    for (int i = 1; i <= N; ++i) {
      const float c0 = cost[(size_t)(i - 1) * (M + 1) + j - 1], c1 = cost[(size_t)(i - 1) * (M + 1) + j], c2 = cost[(size_t)i * (M + 1) + j - 1];
      float c;
      int t;
      if (c0 < c1 && c0 < c2) c = c0, t = 0;
      else if (c1 < c0 && c1 < c2) c = c1, t = 1;
      else c = c2, t = 2;
      cost[(size_t)i * (M + 1) + j] = x[(size_t)(i - 1) * M + j - 1] + c;
      trace[(size_t)i * (M + 1) + j] = (int8_t)t;
    }
  for (int j = 0; j <= M; ++j) trace[j] = 2;
  for (int i = 0; i <= N; ++i) trace[(size_t)i * (M + 1)] = 1;
  int i = N, j = M;
  ti.clear(), tj.clear();
  while (i > 0 || j > 0) {
    ti.push_back(i - 1), tj.push_back(j - 1);
    const int t = trace[(size_t)i * (M + 1) + j];
    if (t == 0) --i, --j;
    else if (t == 1) --i;
    else --j;
  }
  std::reverse(ti.begin(), ti.end());
  std::reverse(tj.begin(), tj.end());
}

static int check_dtw(int N, int M, int family, int negate) {
  std::vector<float> x((size_t)N * M);
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < M; ++j) {
      float v = 0.f;
      if (family == 0) v = gauss();
      if (family == 1) v = (float)(rnd() % 3);
      if (family == 3) v = gauss() - ((long)j * N / M == i ? 4.f : 0.f);
      x[(size_t)i * M + j] = v;
    }
  std::vector<float> xr(x);
  if (negate)
    for (float& v : xr) v = -v;
  std::vector<int> ti, tj;
  reference(xr, N, M, ti, tj);
  // the input as rows [2, 2 + N) of a wider, taller NaN matrix; exact-size output and workspace buffers (the sanitizer guards their ends)
  const int ld = M + 3;
  std::vector<float> big((size_t)(N + 3) * ld, NAN);
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < M; ++j) big[(size_t)(i + 2) * ld + j] = x[(size_t)i * M + j];
  const int P = N + M - 1;
  std::vector<int32_t> text(P, -77), time(P, -77);
  std::vector<uint8_t> ws(oasr_dtw_workspace_bytes(N, M), 0xA5);
  int32_t len = -1;
  if (oasr_test_dtw_host(big.data() + 2 * (size_t)ld, ld, N, M, negate, text.data(), time.data(), &len, ws.data()) != 0) return 1;
  if (len != (int)ti.size()) return 1;
  for (int e = 0; e < P; ++e) {
    if (e < len ? (text[e] != ti[e] || time[e] != tj[e]) : (text[e] != -77 || time[e] != -77)) return 1;
  }
  return 0;
}

template <int W>
static int check_median() {
  for (unsigned bits = 0; bits < (1u << W); ++bits) {
    float p[W];
    for (int k = 0; k < W; ++k) p[k] = (float)((bits >> k) & 1u);
    const float want = __builtin_popcount(bits) > W / 2 ? 1.f : 0.f;
    if (median_net<W>(p) != want) return 1;
  }
  return 0;
}

int main() {
  static const int shapes[][2] = {{1, 1}, {1, 9}, {7, 1}, {2, 2}, {5, 64}, {64, 5}, {65, 63}, {130, 129}, {448, 3}, {3, 1500}, {446, 1500}, {448, 1500}};
  int bad = 0, n = 0;
  for (const auto& s : shapes)
    for (int family = 0; family < 4; ++family)
      for (int negate = 0; negate < 2; ++negate) {
        const int r = check_dtw(s[0], s[1], family, negate);
        if (r) fprintf(stderr, "dtw mismatch: N=%d M=%d family=%d negate=%d\n", s[0], s[1], family, negate);
        bad += r, ++n;
      }
  if (oasr_dtw_workspace_bytes(0, 5) || oasr_dtw_workspace_bytes(449, 5) || oasr_dtw_workspace_bytes(5, 1501)) ++bad;
  int32_t dummy = 0;
  float one = 0.f;
  if (oasr_test_dtw_host(&one, 1, 449, 1, 0, &dummy, &dummy, &dummy, &dummy) == 0) ++bad;  // refused before anything is touched
  const int med = check_median<1>() + check_median<3>() + check_median<5>() + check_median<7>() + check_median<9>() + check_median<11>() +
                  check_median<13>() + check_median<15>();
  if (med) fprintf(stderr, "median network mismatch (%d widths)\n", med);
  printf("dtw_host_check: %d DTW cases, %d mismatches; median networks 1..15: %d wrong\n", n, bad, med);
  return bad || med ? 1 : 0;
}
