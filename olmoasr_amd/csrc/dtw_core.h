// Dynamic time warping as olmoasr_amd/timing.py::dtw states it (whisper.timing.dtw): the pieces the device kernel (align.hip) and the host
// driver (dtw_host.cpp, oasr_test_dtw_host) share, so that the skewed trace layout, the cell update and the backtrace are ONE text that the
// CPU suite exercises without a GPU.  Plain C++: no HIP header is needed to include this file.
//
// Cells are 1-based, (i, j) in [1, N] x [1, M]; row 0 and column 0 are the +inf border with cost(0, 0) = 0.  Cell (i, j) lies on
// anti-diagonal d = i + j in [2, N + M].  The trace is stored skewed, one byte per cell:  trace[(d - 2) * pitch + (i - 1)],
// pitch = N rounded up to 64 -- the rows of one diagonal are neighbours in memory, so the wavefront's stores of a diagonal coalesce.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "core_hd.h"

#define DTW_MAX_N 448   // n_text_ctx
#define DTW_MAX_M 1500  // n_audio_ctx
#define DTW_LANES 64    // cells of one row the backtrace looks at per step

enum { DTW_DIAG = 0, DTW_DOWN = 1, DTW_RIGHT = 2 };  // where the path CAME from: (i-1, j-1), (i-1, j), (i, j-1)

OASR_HD int dtw_pitch(int N) { return (N + 63) & ~63; }
OASR_HD size_t dtw_trace_index(int i, int j, int pitch) { return (size_t)(i + j - 2) * (size_t)pitch + (size_t)(i - 1); }
OASR_HD size_t dtw_trace_bytes(int N, int M) { return (size_t)(N + M - 1) * (size_t)dtw_pitch(N); }
OASR_HD size_t dtw_align16(size_t n) { return (n + 15) & ~(size_t)15; }
// workspace: the skewed trace, then the path in walking order (end to start) as int32 text[P], time[P], P = N + M - 1
OASR_HD size_t dtw_workspace_bytes(int N, int M) { return dtw_align16(dtw_trace_bytes(N, M)) + 2 * sizeof(int32_t) * (size_t)(N + M - 1); }

// One cell: c0 = cost(i-1, j-1), c1 = cost(i-1, j), c2 = cost(i, j-1).  Diagonal only when strictly cheapest, else down only when
// strictly cheapest, else right; the new cost is one fp32 add.
OASR_HD float dtw_cell(float c0, float c1, float c2, float x, int* t) {
  int tt = DTW_RIGHT;
  float c = c2;
  if (c1 < c0 && c1 < c2) tt = DTW_DOWN, c = c1;
  if (c0 < c1 && c0 < c2) tt = DTW_DIAG, c = c0;
  *t = tt;
  return x + c;
}

// The move out of cell (i, j) as the backtrace takes it.  With finite costs the stored trace already says this (the borders are +inf);
// stating it keeps the walk inside the table whatever the input held: (1, 1) ends the path, row 1 only moves right, column 1 only down.
OASR_HD int dtw_move(int t, int i, int j) {
  if (i == 1 && j == 1) return DTW_DIAG;
  if (i == 1) return DTW_RIGHT;
  if (j == 1) return DTW_DOWN;
  return t;
}

// Backtrace, one step: lane k of DTW_LANES looks at cell (i, j - k) of the current row.  `stops` has bit k set where that cell's move is not
// DTW_RIGHT (which includes the lanes left of column 1).  Cells k = 0 .. run - 1 are on the path; `leave` says whether cell `run - 1` leaves the
// row (else all DTW_LANES cells moved right and the walk goes on at column j - DTW_LANES).
OASR_HD int dtw_lane_move(const uint8_t* trace, int pitch, int i, int j, int k) {  // the move out of cell (i, j - k); -1 left of column 1
  const int c = j - k;
  if (c < 1) return -1;
  return dtw_move(trace[dtw_trace_index(i, c, pitch)], i, c);
}
OASR_HD int dtw_run(uint64_t stops, bool* leave) {
  if (stops == 0) {
    *leave = false;
    return DTW_LANES;
  }
  *leave = true;
  return __builtin_ctzll(stops) + 1;
}
