// Batched edit distance with substitution / deletion / insertion / hit counts (include/oasr.h at oasr_edit_counts; the rule: editdist_core.h).
//
// ONE workgroup per (hyp, ref) pair, one thread per hyp token (row i = tid + 1), walking the hyp_len + ref_len - 1 anti-diagonals of the
// table like dtw_kernel (align.hip): cell (i, j - 1) and cell (i - 1, j - 1) stay in the thread's registers, cell (i - 1, j) comes from the
// neighbour through a double-buffered LDS row, one barrier per diagonal.  A cell is one packed 32-bit word, so the three live diagonals
// take 8 KB of LDS; the ref tokens are staged into LDS once (4 KB), the thread's own hyp token sits in a register.  The table never goes to
// global memory and nothing but out[b, 0:4] is written.  The workgroup is as wide as the hyp ROWS are (rounded up to a wave), because the
// lengths live on the device; threads past hyp_len only take part in the barriers.
//
// A wave-resident form (several rows per lane, cross-lane shifts instead of barriers) was not built: 256 pairs of 224 tokens take 0.11 ms
// here beside a logging step of more than a second (profiles/train_error_counts.txt).
#include <hip/hip_runtime.h>

#include "../../include/oasr.h"
#include "editdist_core.h"
#include "kernels.h"

static_assert(OASR_EDIT_MAX_LEN == ED_MAX_LEN, "include/oasr.h and editdist_core.h disagree");

namespace {

constexpr int ED_THREADS_MAX = 1024;  // >= ED_MAX_LEN rows

__global__ __launch_bounds__(ED_THREADS_MAX) void edit_counts_kernel(const int32_t* __restrict__ hyp, long ld_hyp, int Lh,
                                                                     const int32_t* __restrict__ ref, long ld_ref, int Lr,
                                                                     const int32_t* __restrict__ hyp_len, const int32_t* __restrict__ ref_len,
                                                                     int32_t* __restrict__ out) {
  __shared__ uint32_t cb[2][ED_THREADS_MAX + 1];  // cb[d & 1][i] = cell (i, d - i) of diagonal d
  __shared__ int32_t rtok[ED_THREADS_MAX];
  const int b = blockIdx.x, tid = threadIdx.x, i = tid + 1;
  const int n = hyp_len[b], m = ref_len[b];  // (uniform)
  int32_t* o = out + 4 * (long)b;
  if (!ed_len_ok(n, Lh) || !ed_len_ok(m, Lr)) {  // lengths outside the contract: the row says so, nothing is read
    if (tid < 4) o[tid] = -1;
    return;
  }
  if (n == 0 || m == 0) {  // a border cell
    if (tid == 0) ed_unpack(n == 0 ? ed_row0(m) : ed_col0(n), m, o);
    return;
  }
  const int32_t* rr = ref + (long)b * ld_ref;
  for (int j = tid; j < m; j += blockDim.x) rtok[j] = rr[j];
  const bool mine = i <= n;  // n <= blockDim.x (launcher: blockDim.x >= min(Lh, ED_MAX_LEN) >= n)
  const int32_t h = mine ? hyp[(long)b * ld_hyp + tid] : 0;
  uint32_t diag = ed_col0(i - 1), left = ed_col0(i);
  __syncthreads();
  for (int d = 2; d <= n + m; ++d) {
    const int j = d - i;
    if (mine && j >= 1 && j <= m) {
      const uint32_t up = i == 1 ? ed_row0(j) : cb[(d - 1) & 1][i - 1];
      const uint32_t c = ed_cell(diag, left, up, h != rtok[j - 1]);
      cb[d & 1][i] = c;
      left = c;
      diag = up;
    }
    __syncthreads();
  }
  if (i == n) ed_unpack(left, m, o);  // cell (n, m)
}

}  // namespace

int launch_edit_counts(const oasr_edit_args* a, hipStream_t st) {
  const char* why = ed_args_error(a);
  OASR_REQUIRE(!why, "oasr_edit_counts: %s", why);
  OASR_REQUIRE(a->B <= 0x7fffffff / 4, "oasr_edit_counts: B = %d", a->B);
  const int rows = a->Lh < ED_MAX_LEN ? a->Lh : ED_MAX_LEN;
  const int threads = rows < 64 ? 64 : (rows + 63) & ~63;  // <= 1024
  hipLaunchKernelGGL(edit_counts_kernel, dim3(a->B), dim3(threads), 0, st, a->hyp, (long)a->ld_hyp, a->Lh, a->ref, (long)a->ld_ref, a->Lr,
                     a->hyp_len, a->ref_len, a->out);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}
