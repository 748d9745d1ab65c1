// oasr_test_dtw_host (include/oasr_testing.h): the DTW of align.hip run on the CPU.  Shared with the kernel through dtw_core.h: the cell
// update, the skewed one-byte trace index and the 64-cell backtrace step.  The forward loop below re-states the kernel's wavefront (one
// "thread" per token row, two cost rows) without its register prefetch and LDS double buffer, which only the GPU suite covers.  It exists so
// that the indexing the kernel relies on is tested where there is no GPU; it is not a fast host DTW.  Plain C++ (no HIP), so it also builds
// alone under a host sanitizer (tools/dtw_host_check.cpp).
#include <math.h>
#include <string.h>

#include <vector>

#include "dtw_core.h"

void oasr_set_error(const char* fmt, ...);

extern "C" size_t oasr_dtw_workspace_bytes(int N, int M) {
  if (N < 1 || N > DTW_MAX_N || M < 1 || M > DTW_MAX_M) return 0;
  return dtw_workspace_bytes(N, M);
}

extern "C" int oasr_test_dtw_host(const float* cost, int64_t ld, int N, int M, int negate, int32_t* text_indices, int32_t* time_indices,
                                  int32_t* path_len, void* workspace) {
  if (!cost || !text_indices || !time_indices || !path_len || !workspace || N < 1 || N > DTW_MAX_N || M < 1 || M > DTW_MAX_M || ld < M) {
    oasr_set_error("oasr_test_dtw_host: bad arguments (N=%d in [1, %d], M=%d in [1, %d], ld=%lld >= M, no null pointer)", N, DTW_MAX_N, M,
                   DTW_MAX_M, (long long)ld);
    return -1;
  }
  const int pitch = dtw_pitch(N), P = N + M - 1;
  uint8_t* trace = (uint8_t*)workspace;
  int32_t* rev_text = (int32_t*)((char*)workspace + dtw_align16(dtw_trace_bytes(N, M)));
  int32_t* rev_time = rev_text + P;
  const float inf = INFINITY;
  // forward: slot 0 of the two cost rows is the border row (always +inf); thread r owns row i = r + 1
  std::vector<float> cb(2 * (size_t)(pitch + 1), inf), diag(pitch, inf), left(pitch, inf);
  for (int d = 2; d <= N + M; ++d) {
    float* cur = cb.data() + (size_t)(d & 1) * (pitch + 1);
    const float* prev = cb.data() + (size_t)((d - 1) & 1) * (pitch + 1);
    for (int r = 0; r < pitch; ++r) {
      const int i = r + 1, j = d - i;
      if (i > N || j < 1 || j > M) continue;
      if (j == 1) diag[r] = i == 1 ? 0.f : inf, left[r] = inf;
      const float up = prev[i - 1];
      const float x = cost[(size_t)(i - 1) * (size_t)ld + (size_t)(j - 1)];
      int t;
      const float c = dtw_cell(diag[r], up, left[r], negate ? -x : x, &t);
      trace[dtw_trace_index(i, j, pitch)] = (uint8_t)t;
      cur[i] = c;
      left[r] = c;
      diag[r] = up;
    }
  }
  // backtrace: one "wave" of DTW_LANES lanes
  int i = N, j = M, n = 0;
  for (;;) {
    uint64_t stops = 0;
    int mv[DTW_LANES];
    for (int k = 0; k < DTW_LANES; ++k) {
      mv[k] = dtw_lane_move(trace, pitch, i, j, k);
      if (mv[k] != DTW_RIGHT) stops |= (uint64_t)1 << k;
    }
    bool leave;
    const int run = dtw_run(stops, &leave);
    for (int k = 0; k < run && n + k < P; ++k) rev_text[n + k] = i - 1, rev_time[n + k] = j - k - 1;
    n += run;
    if (n > P) n = P;
    if (!leave) {
      j -= DTW_LANES;
      continue;
    }
    const int c = j - (run - 1);
    if (i == 1 && c == 1) break;
    i -= 1;
    j = mv[run - 1] == DTW_DIAG ? c - 1 : c;
  }
  for (int e = 0; e < n; ++e) text_indices[e] = rev_text[n - 1 - e], time_indices[e] = rev_time[n - 1 - e];
  *path_len = n;
  return 0;
}
