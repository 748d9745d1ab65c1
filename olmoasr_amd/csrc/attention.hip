// Flash attention (head_dim 64) forward + backward for gfx950, bf16 in/out, fp32 softmax and accumulation.
//
// Replaces F.scaled_dot_product_attention as called by the reference MultiHeadAttention
// (olmoasr/model.py:317-340): encoder self-attention (no mask), decoder self-attention (causal + key padding
// mask, model.py:740-741, given here as kv_len[b] -- the [B,448,448] additive mask of
// train_timestamps.py:314-315 is column-only) and cross-attention (no mask, Tq=448, Tk=1500), SURVEY.md K6-K8, K14.
//
// Register layout trick: every score tile is computed TRANSPOSED, S^T[k][q] = K.Q^T, with
// v_mfma_f32_32x32x16_bf16.  In the 32x32 accumulator layout lane l owns column q = l & 31 and 16 rows (keys), so
// the online softmax (row max / exp / row sum / rescale) is lane-local except for one exchange between lanes
// l and l^32.  The exponentiated tile, packed to bf16, already IS the B operand of O^T[d][q] = V^T.P^T, and V^T is
// produced from the row-major V tile in LDS by ds_read_b64_tr_b16 -- P never touches LDS.  The same idea drives
// the backward: dK/dV kernel computes S[q][k] with the key lane-local, dQ kernel computes S^T with the query
// lane-local; P and dS feed the second-stage MFMAs straight from registers.
//
// forward : grid (ceil(Tq/128), B*H), 4 waves x 32 queries, KV tiles of 64 keys through a 3-stage LDS-DMA ring.
// backward: bwd_dq   grid (ceil(Tq/128), B*H)  -- also produces delta = rowsum(dO * O)
//           bwd_dkdv grid (ceil(Tk/128), B*H)  -- loops over 64-query tiles of Q / dO / lse / delta.
//
// One file per kernel family -- attention_fwd.hip (forward, decode step), attention_bwd_dq.hip, attention_bwd_dkdv.hip (each: the general
// kernel and the ping-pong kernel of the unmasked case) -- over attention_common.h; this file checks the arguments and decides which
// kernel runs over which grid.
#include "attention_common.h"

namespace {

int g_attn_pingpong = 1;  // tests / A-B (oasr_attention_set_pingpong): 0 routes the unmasked case through the general kernels
int g_attn_span_grid = 1;  // tests / A-B (oasr_attention_set_span_grid): 0 launches the full grid even when a block table is given

// A block table is used where the blocks it leaves out are the ones that exit at once: chunked query rows limited by q_span.
bool span_grid(const AttnArgs& a) { return g_attn_span_grid && a.q_rows && a.q_span && a.qblk128 && a.qblk256; }

int check_args(const AttnArgs& a, bool bwd) {
  OASR_REQUIRE(a.q && a.k && a.v && a.o, "attention: null pointer");
  OASR_REQUIRE(a.B > 0 && a.H > 0 && a.Tq > 0 && a.Tk > 0, "attention: bad shape");
  OASR_REQUIRE((a.ldq % 8) == 0 && (a.ldk % 8) == 0 && (a.ldv % 8) == 0 && (a.ldo % 8) == 0, "attention: strides must be multiples of 8");
  OASR_REQUIRE(!a.causal || a.Tq == a.Tk, "attention: causal needs Tq == Tk");
  if (bwd) OASR_REQUIRE(a.d_o && a.lse && a.delta && a.dq && a.dk && a.dv, "attention_bwd: null pointer");
  if (bwd) OASR_REQUIRE((!a.dq_colsum && !a.dv_colsum) || a.colsum_scratch, "attention_bwd: fused bias gradients need colsum_scratch");
  OASR_REQUIRE(!a.k_rows || a.q_rows, "attention: k_rows needs q_rows");
  OASR_REQUIRE(!a.q_span || a.q_rows, "attention: q_span needs q_rows");
  OASR_REQUIRE(!a.q_rows || ((a.Tq % 64) == 0 && a.Tq <= 64 * OASR_ROWTAB), "attention: chunked query rows need Tq %% 64 == 0 and Tq <= %d", 64 * OASR_ROWTAB);
  OASR_REQUIRE(!a.k_rows || ((a.Tk % 64) == 0 && a.Tk <= 64 * OASR_ROWTAB), "attention: chunked key rows need Tk %% 64 == 0 and Tk <= %d", 64 * OASR_ROWTAB);
  OASR_REQUIRE(!a.qblk128 == !a.qblk256, "attention: the 128- and the 256-query block tables come together");
  OASR_REQUIRE(!a.qblk128 || (a.n128 >= 0 && a.n128 <= a.B * cdiv(a.Tq, 128) && a.n256 >= 0 && a.n256 <= a.B * cdiv(a.Tq, 256) && a.n256 <= a.n128 &&
                              a.n128 <= 2 * a.n256),
               "attention: block counts n128 = %d, n256 = %d do not fit B = %d, Tq = %d", a.n128, a.n256, a.B, a.Tq);
  return OASR_OK;
}

}  // namespace

void attention_set_pingpong(int on) { g_attn_pingpong = on; }
void attention_set_span_grid(int on) { g_attn_span_grid = on; }

int launch_attention_fwd(const AttnArgs& a, hipStream_t s) {
  int rc = check_args(a, false);
  if (rc) return rc;
  if (a.Tq == 1 && a.Tk <= 1536 && !a.o_lo && !a.q_rows) {  // decode step (causality is implied: every cached key is visible)
    attn_launch_decode(a, s);
    OASR_LAUNCH_CHECK();
    return OASR_OK;
  }
  dim3 grid(cdiv(a.Tq, 128) * a.B * a.H);
  AttnArgs r = a;
  if (span_grid(a)) {  // (chunked query rows) only the query blocks inside the spans
    if (a.n128 == 0) return OASR_OK;
    grid = dim3(a.n128 * a.H);
  } else {
    r.qblk128 = r.qblk256 = nullptr;  // (the plain layout never reads the tables)
  }
  attn_launch_fwd(r, grid, s);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}

int launch_attention_bwd(const AttnArgs& a, hipStream_t s) {
  int rc = check_args(a, true);
  if (rc) return rc;
  dim3 gq(cdiv(a.Tq, 128) * a.B * a.H), gk(cdiv(a.Tk, 128) * a.B * a.H), gq256(cdiv(a.Tq, 256) * a.B * a.H);
  const bool rows = a.q_rows != nullptr;
  const int d = a.H * 64;
  const long rq = (long)a.B * cdiv(a.Tq, 128), rk = (long)a.B * cdiv(a.Tk, 128);
  // Compact grids (kernels.h: AttnArgs.qblk128 / qblk256).  aq: the arguments of the dQ kernel; ak: of the dK/dV kernel, which takes the
  // table only where its empty blocks are the same ones -- chunked KEY rows, i.e. the decoder's self-attention.
  AttnArgs aq = a, ak = a;
  const bool cq = rows && span_grid(a), ck = cq && a.k_rows != nullptr && a.Tk == a.Tq;
  if (!cq) aq.qblk128 = aq.qblk256 = nullptr;
  if (!ck) ak.qblk128 = ak.qblk256 = nullptr;
  if (cq) {
    if (a.n128 == 0) return OASR_OK;  // every span is 0: no gradient anywhere, nothing to add to the bias gradients
    gq = dim3(a.n128 * a.H);
    gq256 = dim3(a.n256 * a.H);
    if (ck) gk = gq;
    // The partial bias-gradient rows keep their [B * ceil(T / 128)] layout (the reduction below sums the same rows as with the full
    // grid); the rows of the blocks that are no longer launched are zeroed here instead of by their workgroups.
    const long zrows = (a.dq_colsum ? rq : 0) + (ck && a.dv_colsum ? rk : 0);
    float* z0 = a.dq_colsum ? a.colsum_scratch : a.colsum_scratch + rq * d;
    if (zrows) OASR_CHECK_HIP(hipMemsetAsync(z0, 0, (size_t)zrows * d * sizeof(float), s));
  }
  // the ping-pong kernels take the unmasked case; with chunked rows only the cross-attention form (plain key side, <= 8 query tiles)
  const bool pp = !a.causal && !a.kv_len && g_attn_pingpong && (!rows || (!a.k_rows && a.Tq <= 512));
  // The chunked-row case is the cross-attention backward of a span step: ~2 active 64-query tiles per sample.  Kernel choice per side measured with an
  // experiment build (bit 0 / bit 1 = dQ / dK-dV on the ping-pong kernels; (profiles/r04_cross_attention_kernel_choice.txt, whole step, same box): both 1363.5 /
  // 1367.1 ms, dQ ping-pong + dK/dV general 1358.8, dQ general + dK/dV ping-pong 1377.2, both general 1371.6.  The 0.3-0.6 % of "1" are
  // NOT taken: with the same kernels on both sides the span step reproduces the plain step's arithmetic row by row (gradients equal to
  // 1e-7, fp32 summation order only; tests/test_gpu_span.py), with a different dK/dV kernel only to bf16 rounding (2.6e-4).
  if (pp) {
    attn_launch_bwd_dq_pp(aq, gq256, s);
    rc = attn_launch_bwd_dkdv_pp(a, dim3(cdiv(a.Tk, 256) * a.B * a.H), s);  // (always the full grid: it does not take the block tables)
    if (rc) return rc;
  } else {
    attn_launch_bwd_dq(aq, gq, s);
    attn_launch_bwd_dkdv(ak, gk, s);
  }
  OASR_LAUNCH_CHECK();
  // fused query / value bias gradients: reduce the per-workgroup partial rows (a few MB) into the fp32 gradients
  if (a.dq_colsum) {
    int rc2 = launch_colsum_accum(a.colsum_scratch, d, rq, d, a.dq_colsum, s);
    if (rc2) return rc2;
  }
  if (a.dv_colsum) {
    int rc2 = launch_colsum_accum(a.colsum_scratch + rq * d, d, rk, d, a.dv_colsum, s);
    if (rc2) return rc2;
  }
  return OASR_OK;
}
