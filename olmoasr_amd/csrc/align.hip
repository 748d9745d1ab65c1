// Word-timestamp alignment on the device (olmoasr_amd/timing.py::find_alignment, steps 2 and 3 of its docstring):
//
//   oasr_alignment_matrix   the cross-attention score planes of the alignment heads -> the [tokens, frames] matrix
//       out[i, j] = mean_h median_w( z_h[i, reflect(j - w/2 .. j + w/2)] ),   z_h = (p_h - mean_i p_h) / std_i p_h,   p_h = softmax_j(scale * qk_h)
//     in three plain kernels that read the planes IN PLACE (per-layer base pointer + bit mask of heads; nothing of the planes' size is
//     written): row statistics (max, sum) per (head, token), column statistics (mean, 1/std) per (head, frame), then per (token, 256-frame
//     tile) z recomputed into LDS with its reflected halo, the median by a compare-exchange network (median_core.h) and the heads summed
//     in ascending (layer, head) order -- the result does not depend on scheduling.
//
//   oasr_dtw                the monotonic alignment of timing.py::dtw, bit for bit, path included
//     ONE workgroup, one thread per token row, walks the N + M - 1 anti-diagonals: cost(i, j - 1) and cost(i - 1, j - 1) stay in the
//     thread's registers, cost(i - 1, j) comes from the neighbour through a double-buffered LDS row, one barrier per diagonal.  The trace is
//     stored skewed ([diagonal][row], dtw_core.h), so a diagonal's stores coalesce; it lives in global memory (it does not fit the LDS) and
//     stays in L2.  After the last barrier wave 0 walks back: per step its 64 lanes load the 64 cells left of the current one, ballot for the
//     first that leaves the row and jump there, about N + M / 64 dependent loads instead of N + M.  The path is written end-to-start into the
//     workspace and turned round by the whole workgroup.
#include <hip/hip_runtime.h>

#include "../../include/oasr.h"
#include "dtw_core.h"
#include "kernels.h"
#include "median_core.h"

namespace {

// ---- alignment matrix ---------------------------------------------------------------------------------------------------------------
struct AlignSel {
  const float* qk[OASR_ALIGN_MAX_LAYERS];
  uint32_t mask[OASR_ALIGN_MAX_LAYERS];
  int n_layers;
};

// plane of the s-th selected head in ascending (layer, head) order (s is uniform per wave: scalar code)
__device__ __forceinline__ const float* sel_plane(const AlignSel& a, int s, long plane) {
  for (int l = 0; l < a.n_layers; ++l) {
    uint32_t m = a.mask[l];
    const int c = __popc(m);
    if (s < c) {
      for (int t = 0; t < s; ++t) m &= m - 1;
      return a.qk[l] + (long)(__ffs(m) - 1) * plane;
    }
    s -= c;
  }
  return nullptr;
}

// (max, sum exp) of scale * qk over the first F frames: one wave per (selected head, token) row
__global__ __launch_bounds__(256) void align_row_stats_kernel(AlignSel sel, int nsel, int n_tok, int Tk, int F, float scale, float* __restrict__ ml) {
  const int lane = threadIdx.x & 63, R = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (R >= nsel * n_tok) return;
  const int s = R / n_tok, i = R - s * n_tok;
  const float* row = sel_plane(sel, s, (long)n_tok * Tk) + (long)i * Tk;
  float m = -__builtin_huge_valf();
  for (int j = lane; j < F; j += 64) m = fmaxf(m, __fmul_rn(row[j], scale));
  m = wave_max(m);
  float l = 0.f;
  for (int j = lane; j < F; j += 64) l += expf(__fmul_rn(row[j], scale) - m);
  l = wave_sum(l);
  if (lane == 0) ml[2 * (long)R] = m, ml[2 * (long)R + 1] = l;
}

// (mean, 1/std) of p over ALL n_tok rows per (selected head, frame): 64 frames x 4 token slices per workgroup, sums in double, the slices
// added in a fixed order
__global__ __launch_bounds__(256) void align_col_stats_kernel(AlignSel sel, int n_tok, int Tk, int F, float scale, const float* __restrict__ ml,
                                                              float* __restrict__ mean, float* __restrict__ rstd) {
  __shared__ double s1[4][64], s2[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, s = blockIdx.y, j = blockIdx.x * 64 + tx;
  const float* plane = sel_plane(sel, s, (long)n_tok * Tk);
  const float* st = ml + 2 * (long)s * n_tok;
  double a = 0., b = 0.;
  if (j < F)
    for (int i = ty; i < n_tok; i += 4) {
      const float p = expf(__fmul_rn(plane[(long)i * Tk + j], scale) - st[2 * i]) / st[2 * i + 1];
      a += (double)p;
      b += (double)p * (double)p;
    }
  s1[ty][tx] = a, s2[ty][tx] = b;
  __syncthreads();
  if (ty == 0 && j < F) {
    const double sum = ((s1[0][tx] + s1[1][tx]) + s1[2][tx]) + s1[3][tx], sq = ((s2[0][tx] + s2[1][tx]) + s2[2][tx]) + s2[3][tx];
    const double mu = sum / n_tok, var = fmax(sq / n_tok - mu * mu, 0.);
    mean[(long)s * F + j] = (float)mu;
    rstd[(long)s * F + j] = (float)(1. / sqrt(var));  // a column of zero variance is outside the contract (the torch path yields NaN there)
  }
}

// out[i, tile] = mean over the selected heads of the width-W median of z along the frames (W = 1: z itself)
template <int W>
__global__ __launch_bounds__(256) void align_out_kernel(AlignSel sel, int nsel, int n_tok, int Tk, int F, float scale, const float* __restrict__ ml,
                                                        const float* __restrict__ mean, const float* __restrict__ rstd, float* __restrict__ out,
                                                        long ldo) {
  constexpr int PAD = W / 2, TILE = 256, BUF = TILE + 2 * PAD;
  __shared__ float zb[2][BUF];
  const int tid = threadIdx.x, i = blockIdx.y, t0 = blockIdx.x * TILE, j = t0 + tid;
  float acc = 0.f;
  int s = 0;
  for (int l = 0; l < sel.n_layers; ++l) {
    for (uint32_t hm = sel.mask[l]; hm; hm &= hm - 1, ++s) {
      const float* row = sel.qk[l] + ((long)(__ffs(hm) - 1) * n_tok + i) * Tk;
      const float m = ml[2 * ((long)s * n_tok + i)], li = ml[2 * ((long)s * n_tok + i) + 1];
      const float* mu = mean + (long)s * F;
      const float* rs = rstd + (long)s * F;
      float* buf = zb[s & 1];
      for (int t = tid; t < BUF; t += TILE) {
        int fr = t0 - PAD + t;
        if (fr < F + PAD) {  // reflect: -k -> k, F - 1 + k -> F - 1 - k (PAD < F whenever W > 1)
          fr = fr < 0 ? -fr : (fr >= F ? 2 * (F - 1) - fr : fr);
          const float p = expf(__fmul_rn(row[fr], scale) - m) / li;
          buf[t] = (p - mu[fr]) * rs[fr];
        }
      }
      __syncthreads();  // (one barrier per head: the next head fills the other buffer)
      if (j < F) {
        float w[W];
#pragma unroll
        for (int k = 0; k < W; ++k) w[k] = buf[tid + k];
        acc += median_net<W>(w);
      }
    }
  }
  if (j < F) out[(long)i * ldo + j] = acc / (float)nsel;
}

template <int W>
void launch_align_out(const AlignSel& sel, int nsel, const oasr_align_args& a, const float* ml, const float* mean, const float* rstd, hipStream_t st) {
  hipLaunchKernelGGL(align_out_kernel<W>, dim3(cdiv(a.n_frames, 256), a.n_tok), dim3(256), 0, st, sel, nsel, a.n_tok, a.Tk, a.n_frames, a.qk_scale, ml,
                     mean, rstd, a.out, (long)a.ldo);
}

// ---- DTW ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void dtw_kernel(const float* __restrict__ cost, long ld, int N, int M, int negate, uint8_t* trace,
                                                  int32_t* rev_text, int32_t* rev_time, int32_t* __restrict__ text,
                                                  int32_t* __restrict__ time, int32_t* __restrict__ path_len) {
  constexpr int ROW = DTW_MAX_N + 64 + 1;  // slot 0: the +inf border row
  __shared__ float cb[2][ROW];
  __shared__ int s_len;
  const int tid = threadIdx.x, NT = blockDim.x, pitch = dtw_pitch(N), i = tid + 1, P = N + M - 1;
  const float inf = __builtin_huge_valf();
  for (int e = tid; e < 2 * ROW; e += NT) (&cb[0][0])[e] = inf;
  __syncthreads();
  const bool mine = i <= N;
  const float* xr = cost + (long)(mine ? i - 1 : 0) * ld;
  float diag = inf, left = inf;
  // the row's costs four columns at a time, one group ahead of the cell being computed
  float xc0 = 0.f, xc1 = 0.f, xc2 = 0.f, xc3 = 0.f, xn0 = 0.f, xn1 = 0.f, xn2 = 0.f, xn3 = 0.f;
  if (mine) {
    xn0 = xr[0];
    if (1 < M) xn1 = xr[1];
    if (2 < M) xn2 = xr[2];
    if (3 < M) xn3 = xr[3];
  }
  for (int d = 2; d <= N + M; ++d) {
    const int j = d - i;
    if (mine && j >= 1 && j <= M) {
      const int q = (j - 1) & 3;
      if (q == 0) {
        xc0 = xn0, xc1 = xn1, xc2 = xn2, xc3 = xn3;
        const int c = j - 1 + 4;
        if (c < M) xn0 = xr[c];
        if (c + 1 < M) xn1 = xr[c + 1];
        if (c + 2 < M) xn2 = xr[c + 2];
        if (c + 3 < M) xn3 = xr[c + 3];
      }
      if (j == 1) diag = i == 1 ? 0.f : inf, left = inf;
      const float up = cb[(d - 1) & 1][i - 1];
      const float xv = q == 0 ? xc0 : (q == 1 ? xc1 : (q == 2 ? xc2 : xc3));
      int t;
      const float c = dtw_cell(diag, up, left, negate ? -xv : xv, &t);
      trace[dtw_trace_index(i, j, pitch)] = (uint8_t)t;
      cb[d & 1][i] = c;
      left = c;
      diag = up;
    }
    __syncthreads();
  }
  __threadfence();  // the trace of every wave, before wave 0 reads it
  __syncthreads();
  if (tid < DTW_LANES) {
    int ci = N, cj = M, n = 0;
    for (;;) {
      const int mv = dtw_lane_move(trace, pitch, ci, cj, tid);
      bool leave;
      const int run = dtw_run(__ballot(mv != DTW_RIGHT), &leave);
      if (tid < run && n + tid < P) rev_text[n + tid] = ci - 1, rev_time[n + tid] = cj - tid - 1;
      n = min(n + run, P);
      if (!leave) {
        cj -= DTW_LANES;
        continue;
      }
      const int c = cj - (run - 1);
      if (ci == 1 && c == 1) break;
      const int out_mv = __shfl(mv, run - 1, 64);
      ci -= 1;
      cj = out_mv == DTW_DIAG ? c - 1 : c;
    }
    if (tid == 0) s_len = n, *path_len = n;
  }
  __threadfence();
  __syncthreads();
  const int n = s_len;
  for (int e = tid; e < n; e += NT) text[e] = rev_text[n - 1 - e], time[e] = rev_time[n - 1 - e];
}

}  // namespace

static int align_count_heads(const oasr_align_args* a) {
  int n = 0;
  for (int l = 0; l < a->n_layers; ++l) n += __builtin_popcount(a->head_mask[l]);
  return n;
}

extern "C" size_t oasr_alignment_workspace_bytes(int n_selected_heads, int n_tok, int n_frames) {
  if (n_selected_heads < 1 || n_tok < 1 || n_frames < 1) return 0;
  return sizeof(float) * 2 * (size_t)n_selected_heads * ((size_t)n_tok + (size_t)n_frames);
}

int launch_alignment_matrix(const oasr_align_args* a, void* workspace, size_t workspace_bytes, hipStream_t st) {
  OASR_REQUIRE(a && workspace, "oasr_alignment_matrix: null args");
  OASR_REQUIRE(a->n_layers >= 1 && a->n_layers <= OASR_ALIGN_MAX_LAYERS && a->H >= 1 && a->H <= 32,
               "oasr_alignment_matrix: n_layers = %d (1 .. %d), H = %d (1 .. 32)", a->n_layers, OASR_ALIGN_MAX_LAYERS, a->H);
  OASR_REQUIRE(a->n_tok >= 1 && a->n_tok <= 65535 && a->Tk >= 1 && a->n_frames >= 1 && a->n_frames <= a->Tk,
               "oasr_alignment_matrix: n_tok = %d (1 .. 65535), n_frames = %d (1 .. Tk = %d)", a->n_tok, a->n_frames, a->Tk);
  OASR_REQUIRE(a->medfilt_width >= 1 && a->medfilt_width <= 15 && (a->medfilt_width & 1),
               "oasr_alignment_matrix: medfilt_width = %d (odd, 1 .. 15)", a->medfilt_width);
  OASR_REQUIRE(a->out && a->ldo >= a->n_frames, "oasr_alignment_matrix: out is null or its row stride %lld < n_frames", (long long)a->ldo);
  AlignSel sel;
  memset(&sel, 0, sizeof(sel));
  sel.n_layers = a->n_layers;
  for (int l = 0; l < a->n_layers; ++l) {
    const uint32_t m = a->head_mask[l];
    OASR_REQUIRE(a->H == 32 || (m >> a->H) == 0, "oasr_alignment_matrix: head_mask[%d] = 0x%x names a head >= H = %d", l, m, a->H);
    OASR_REQUIRE(!m || a->qk[l], "oasr_alignment_matrix: layer %d has selected heads and a null score tensor", l);
    sel.qk[l] = a->qk[l];
    sel.mask[l] = m;
  }
  const int nsel = align_count_heads(a);
  OASR_REQUIRE(nsel >= 1, "oasr_alignment_matrix: no head selected");
  const size_t need = oasr_alignment_workspace_bytes(nsel, a->n_tok, a->n_frames);
  OASR_REQUIRE(workspace_bytes >= need, "oasr_alignment_matrix: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  const int F = a->n_frames;
  float* ml = (float*)workspace;
  float* mean = ml + 2 * (size_t)nsel * a->n_tok;
  float* rstd = mean + (size_t)nsel * F;
  hipLaunchKernelGGL(align_row_stats_kernel, dim3(cdiv((long)nsel * a->n_tok, 4)), dim3(256), 0, st, sel, nsel, a->n_tok, a->Tk, F, a->qk_scale, ml);
  OASR_LAUNCH_CHECK();
  hipLaunchKernelGGL(align_col_stats_kernel, dim3(cdiv(F, 64), nsel), dim3(256), 0, st, sel, a->n_tok, a->Tk, F, a->qk_scale, ml, mean, rstd);
  OASR_LAUNCH_CHECK();
  const int W = F <= a->medfilt_width / 2 ? 1 : a->medfilt_width;  // median_filter leaves a row no longer than the padding as it is
  switch (W) {
    case 1: launch_align_out<1>(sel, nsel, *a, ml, mean, rstd, st); break;
    case 3: launch_align_out<3>(sel, nsel, *a, ml, mean, rstd, st); break;
    case 5: launch_align_out<5>(sel, nsel, *a, ml, mean, rstd, st); break;
    case 7: launch_align_out<7>(sel, nsel, *a, ml, mean, rstd, st); break;
    case 9: launch_align_out<9>(sel, nsel, *a, ml, mean, rstd, st); break;
    case 11: launch_align_out<11>(sel, nsel, *a, ml, mean, rstd, st); break;
    case 13: launch_align_out<13>(sel, nsel, *a, ml, mean, rstd, st); break;
    default: launch_align_out<15>(sel, nsel, *a, ml, mean, rstd, st); break;
  }
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}

int launch_dtw(const float* cost, long ld, int N, int M, int negate, int32_t* text_indices, int32_t* time_indices, int32_t* path_len, void* workspace,
               size_t workspace_bytes, hipStream_t st) {
  OASR_REQUIRE(cost && text_indices && time_indices && path_len && workspace, "oasr_dtw: null args");
  OASR_REQUIRE(N >= 1 && N <= DTW_MAX_N && M >= 1 && M <= DTW_MAX_M && ld >= M, "oasr_dtw: N = %d (1 .. %d), M = %d (1 .. %d), ld = %lld (>= M)", N,
               DTW_MAX_N, M, DTW_MAX_M, (long long)ld);
  OASR_REQUIRE(workspace_bytes >= dtw_workspace_bytes(N, M), "oasr_dtw: workspace of %zu bytes, %zu needed", workspace_bytes, dtw_workspace_bytes(N, M));
  uint8_t* trace = (uint8_t*)workspace;
  int32_t* rev_text = (int32_t*)((char*)workspace + dtw_align16(dtw_trace_bytes(N, M)));
  hipLaunchKernelGGL(dtw_kernel, dim3(1), dim3(dtw_pitch(N)), 0, st, cost, ld, N, M, negate, trace, rev_text,
                     rev_text + (N + M - 1), text_indices, time_indices, path_len);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}
