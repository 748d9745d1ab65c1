// C ABI plumbing: error string, unit-operator wrappers over the internal launchers, and a one-wave probe that
// dumps what ds_read_b64_tr_b16 returns (used by tests to pin the transpose-read lane mapping the GEMM and
// attention kernels rely on).
#include <stdarg.h>

#include "../../include/oasr.h"
#include "kernels.h"

static thread_local char g_err[512] = "";

void oasr_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* oasr_last_error(void) { return g_err; }
extern "C" int oasr_version(void) { return OASR_ABI_VERSION; }
extern "C" size_t oasr_sizeof_attn_args(void) { return sizeof(oasr_attn_args); }

static OperandView to_view(const oasr_operand& o) {
  return OperandView{(const bf16_t*)o.ptr, (long)o.ld, o.rpb, (long)o.bstride, o.lead, o.kvalid, o.trail_from};
}

static int to_gemm(const oasr_gemm_args* a, GemmArgs& g) {
  OASR_REQUIRE(a, "oasr_gemm: null args");
  g = gemm_defaults();
  g.A = to_view(a->A);
  g.B = to_view(a->B);
  g.M = a->M;
  g.N = a->N;
  g.K = a->K;
  g.ta = a->ta;
  g.tb = a->tb;
  g.alpha = a->alpha;
  g.bias = a->bias;
  g.act = a->act;
  g.pos = a->pos;
  g.pos_period = a->pos_period;
  g.dgelu_u = (const bf16_t*)a->dgelu_u;
  g.ldu = a->ldu;
  g.resid = (const bf16_t*)a->resid;
  g.ldr = a->ldr;
  g.out = (bf16_t*)a->out;
  g.out_pre = (bf16_t*)a->out_pre;
  g.ldc = a->ldc;
  g.out_f32 = a->out_f32;
  g.ldc32 = a->ldc32;
  g.beta = a->beta;
  g.colsum = a->colsum;
  g.atomic = a->atomic;
  g.split_k = a->split_k < 1 ? 1 : a->split_k;
  g.dgelu_deriv = a->dgelu_deriv;
  OASR_REQUIRE(a->act >= 0 && a->act <= 2, "oasr_gemm: act must be 0 (none), 1 (GELU) or 2 (GELU, out_pre = GELU')");
  return OASR_OK;
}

extern "C" int oasr_gemm(const oasr_gemm_args* a, void* stream) {
  GemmArgs g;
  const int rc = to_gemm(a, g);
  return rc ? rc : launch_gemm(g, (hipStream_t)stream);
}

// tests (include/oasr_testing.h): oasr_gemm plus the launch options only the engine sets
extern "C" int oasr_test_gemm(const oasr_gemm_args* a, float* colsum_scratch, int atomic_on_pp, int raster_gm, int stagger, int stagger_phases,
                              void* stream) {
  GemmArgs g;
  const int rc = to_gemm(a, g);
  if (rc) return rc;
  g.colsum_scratch = colsum_scratch;
  g.atomic_on_pp = atomic_on_pp;
  g.raster_gm = raster_gm;
  g.stagger = stagger;
  g.stagger_phases = stagger_phases;
  return launch_gemm(g, (hipStream_t)stream);
}

// The setters below change process-wide kernel-selection state: testing hooks, inert without the opt-in (common.h: OASR_HOOK_GATE).
extern "C" int oasr_profile_gemm(int enable) {
  gemm_profile_enable(enable);
  return OASR_OK;
}
extern "C" int oasr_gemm_set_variant(int v) {
  OASR_HOOK_GATE("oasr_gemm_set_variant");
  return gemm_set_variant(v);
}
extern "C" int oasr_gemm_set_stagger(int sleeps, int phases) {
  OASR_HOOK_GATE("oasr_gemm_set_stagger");
  gemm_set_stagger(sleeps, phases);
  return OASR_OK;
}
extern "C" int oasr_attention_set_pingpong(int on) {
  OASR_HOOK_GATE("oasr_attention_set_pingpong");
  attention_set_pingpong(on);
  return OASR_OK;
}
extern "C" int oasr_attention_set_span_grid(int on) {
  OASR_HOOK_GATE("oasr_attention_set_span_grid");
  attention_set_span_grid(on);
  return OASR_OK;
}
extern "C" int oasr_gemm_force_general(int on) {
  OASR_HOOK_GATE("oasr_gemm_force_general");
  gemm_force_general(on);
  return OASR_OK;
}
extern "C" int oasr_profile_gemm_records(char* buf, int cap) {
  const int n = gemm_profile_records(buf, cap);
  OASR_REQUIRE(n >= 0, "oasr_profile_gemm_records: %d bytes do not hold the launch records", cap);
  return n;
}
extern "C" int oasr_profile_gemm_collect(double* ms4, double* flops4, int64_t* count4, char* by_symbol, int cap) {
  OASR_REQUIRE(ms4 && flops4 && count4, "profile_collect: null");
  long c[4];
  int rc = gemm_profile_collect(ms4, flops4, c, by_symbol, cap);
  for (int i = 0; i < 4; ++i) count4[i] = c[i];
  return rc;
}

extern "C" int oasr_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int64_t rows,
                                  int d, void* stream) {
  return launch_layernorm_fwd((const bf16_t*)x, gamma, beta, (bf16_t*)y, mean, rstd, rows, d, (hipStream_t)stream);
}
extern "C" int oasr_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                                  const void* dres, void* dx, float* dgamma, float* dbeta, int64_t rows, int d, void* stream) {
  return launch_layernorm_bwd((const bf16_t*)dy, (const bf16_t*)x, gamma, mean, rstd, (const bf16_t*)dres, (bf16_t*)dx, dgamma, dbeta,
                              nullptr, rows, d, (hipStream_t)stream);
}

static AttnArgs to_attn(const oasr_attn_args* a) {
  AttnArgs r;
  memset(&r, 0, sizeof(r));
  r.q = (const bf16_t*)a->q;
  r.k = (const bf16_t*)a->k;
  r.v = (const bf16_t*)a->v;
  r.ldq = a->ldq;
  r.ldk = a->ldk;
  r.ldv = a->ldv;
  r.bsq = a->bsq;
  r.bsk = a->bsk;
  r.bsv = a->bsv;
  r.o = (bf16_t*)a->o;
  r.ldo = a->ldo;
  r.bso = a->bso;
  r.lse = a->lse;
  r.o_lo = (bf16_t*)a->o_lo;
  r.kv_len = a->kv_len;
  r.B = a->B;
  r.H = a->H;
  r.Tq = a->Tq;
  r.Tk = a->Tk;
  r.causal = a->causal;
  r.d_o = (const bf16_t*)a->d_o;
  r.delta = a->delta;
  r.dq = (bf16_t*)a->dq;
  r.dk = (bf16_t*)a->dk;
  r.dv = (bf16_t*)a->dv;
  r.dq_colsum = a->dq_colsum;
  r.dv_colsum = a->dv_colsum;
  r.colsum_scratch = a->colsum_scratch;
  r.qtile_flags = a->qtile_flags;
  r.q_rows = a->q_rows;
  r.k_rows = a->k_rows;
  r.q_span = a->q_span;
  r.qblk128 = a->qblk128;
  r.qblk256 = a->qblk256;
  r.n128 = a->n128;
  r.n256 = a->n256;
  return r;
}
extern "C" int oasr_attention_fwd(const oasr_attn_args* a, void* stream) {
  OASR_REQUIRE(a, "oasr_attention_fwd: null args");
  return launch_attention_fwd(to_attn(a), (hipStream_t)stream);
}
extern "C" int oasr_attention_bwd(const oasr_attn_args* a, void* stream) {
  OASR_REQUIRE(a, "oasr_attention_bwd: null args");
  return launch_attention_bwd(to_attn(a), (hipStream_t)stream);
}
extern "C" int oasr_attention_scores(const oasr_attn_args* a, int dtype, float* scores, void* stream) {
  OASR_REQUIRE(a && scores, "oasr_attention_scores: null args");
  OASR_REQUIRE(dtype == OASR_DTYPE_BF16 || dtype == OASR_DTYPE_F32, "oasr_attention_scores: dtype %d (0 = bf16 operands, 1 = fp32 operands)", dtype);
  if (dtype == OASR_DTYPE_BF16) return launch_attention_scores(to_attn(a), scores, (hipStream_t)stream);
  AttnArgsF f;
  memset(&f, 0, sizeof(f));
  f.q = (const float*)a->q, f.k = (const float*)a->k;
  f.ldq = a->ldq, f.ldk = a->ldk, f.bsq = a->bsq, f.bsk = a->bsk;
  f.kv_len = a->kv_len;
  f.B = a->B, f.H = a->H, f.Tq = a->Tq, f.Tk = a->Tk, f.causal = a->causal;
  f.q_rows = a->q_rows, f.k_rows = a->k_rows;
  return launch_attention_scores(f, scores, (hipStream_t)stream);
}

extern "C" size_t oasr_sizeof_align_args(void) { return sizeof(oasr_align_args); }
extern "C" int oasr_alignment_matrix(const oasr_align_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  return launch_alignment_matrix(a, workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" int oasr_dtw(const float* cost, int64_t ld, int N, int M, int negate, int32_t* text_indices, int32_t* time_indices, int32_t* path_len,
                        void* workspace, size_t workspace_bytes, void* stream) {
  return launch_dtw(cost, (long)ld, N, M, negate, text_indices, time_indices, path_len, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" size_t oasr_sizeof_specaug(void) { return sizeof(oasr_specaug); }
extern "C" int oasr_spec_augment(float* mel, int B, int n_mels, int T, const oasr_specaug* policy, uint64_t seed, uint64_t first_clip,
                                 void* stream) {
  return launch_spec_augment(mel, B, n_mels, T, policy, seed, first_clip, (hipStream_t)stream);
}

extern "C" int oasr_edit_counts(const oasr_edit_args* a, void* stream) { return launch_edit_counts(a, (hipStream_t)stream); }

extern "C" int oasr_score_rows(const void* logits, int dtype, int64_t ld, int V, const int64_t* targets, const int32_t* span, int B, int S,
                               int64_t ignore, float* row_nll, int32_t* pred, void* stream) {
  OASR_REQUIRE(dtype == OASR_DTYPE_BF16 || dtype == OASR_DTYPE_F32, "oasr_score_rows: dtype %d (0 = bf16, 1 = fp32 logits)", dtype);
  if (dtype == OASR_DTYPE_BF16)
    return launch_score_rows((const bf16_t*)logits, (long)ld, V, targets, span, B, S, (long)ignore, row_nll, pred, (hipStream_t)stream);
  return launch_score_rows((const float*)logits, (long)ld, V, targets, span, B, S, (long)ignore, row_nll, pred, (hipStream_t)stream);
}
extern "C" int oasr_score_reduce(const float* row_nll, const int32_t* pred, const int64_t* targets, const int32_t* span, int B, int S, int V,
                                 int64_t ignore, float* nll_sum, float* nll_max, int32_t* n_tok, int32_t* n_hit, void* stream) {
  return launch_score_reduce(row_nll, pred, targets, span, B, S, V, (long)ignore, nll_sum, nll_max, n_tok, n_hit, (hipStream_t)stream);
}

extern "C" int oasr_beam_update(const oasr_beam_args* a, void* stream) { return launch_beam_update(a, (hipStream_t)stream); }

extern "C" size_t oasr_sizeof_speed(void) { return sizeof(oasr_speed); }
extern "C" size_t oasr_sizeof_speed_args(void) { return sizeof(oasr_speed_args); }
extern "C" int oasr_speed_perturb(const oasr_speed_args* a, void* stream) { return launch_speed_perturb(a, (hipStream_t)stream); }

extern "C" size_t oasr_sizeof_noise(void) { return sizeof(oasr_noise); }
extern "C" size_t oasr_sizeof_noise_args(void) { return sizeof(oasr_noise_args); }
extern "C" size_t oasr_noise_workspace_bytes(int B, int N) { return (B < 1 || N < 1) ? 0 : noise_workspace_bytes(B, N); }
extern "C" int oasr_noise_mix(const oasr_noise_args* a, void* stream) { return launch_noise_mix(a, (hipStream_t)stream); }

extern "C" size_t oasr_sizeof_reverb(void) { return sizeof(struct oasr_reverb); }
extern "C" size_t oasr_sizeof_reverb_args(void) { return sizeof(oasr_reverb_args); }
extern "C" size_t oasr_reverb_workspace_bytes(int R, int K) {
  return (R < 1 || R > 65535 || K < 1 || K > 8192) ? 0 : reverb_workspace_bytes(R, K);
}
extern "C" int oasr_reverb(const oasr_reverb_args* a, void* stream) { return launch_reverb(a, (hipStream_t)stream); }

extern "C" size_t oasr_sizeof_telephone(void) { return sizeof(struct oasr_telephone); }
extern "C" size_t oasr_sizeof_telephone_args(void) { return sizeof(oasr_telephone_args); }
extern "C" int oasr_telephone(const oasr_telephone_args* a, void* stream) { return launch_telephone(a, (hipStream_t)stream); }

extern "C" int oasr_test_span_tables(const int32_t* span_host, int B, int S, const int64_t* targets, int32_t* rows_out, int32_t* span_out,
                                     int64_t* targets_rows_out, int64_t* active_rows_out, void* stream) {
  OASR_REQUIRE(active_rows_out, "oasr_test_span_tables: null");
  long act = 0;
  const int rc = launch_build_span_tables(span_host, B, S, targets, 51864, rows_out, span_out, targets_rows_out, &act, (hipStream_t)stream);
  *active_rows_out = act;
  return rc;
}

extern "C" int oasr_test_span_block_tables(const int32_t* span_host, int B, int S, int H, const int64_t* targets, int32_t* rows_out,
                                           int32_t* span_out, int64_t* targets_rows_out, int32_t* blk128_out, int32_t* blk256_out,
                                           int32_t* counts_out, void* stream) {
  OASR_REQUIRE(counts_out, "oasr_test_span_block_tables: null");
  long act = 0;
  SpanBlockTables blk{H, blk128_out, blk256_out, 0, 0};
  const int rc = launch_build_span_tables(span_host, B, S, targets, 51864, rows_out, span_out, targets_rows_out, &act, (hipStream_t)stream, &blk);
  counts_out[0] = blk.n128;
  counts_out[1] = blk.n256;
  return rc;
}

// ---- tests (include/oasr_testing.h): the glue launchers of kernels.h as unit operators.  Thin: the launchers check their own arguments;
// dtype selects the bf16 production kernel or the fp32 validation overload, as in oasr_attention_scores. --------------------------------
#define OASR_TEST_DTYPE(name) \
  OASR_REQUIRE(dtype == OASR_DTYPE_BF16 || dtype == OASR_DTYPE_F32, name ": dtype %d (0 = bf16, 1 = fp32 activations)", dtype)

extern "C" int oasr_test_embedding_fwd(const int64_t* tok, const float* E, const float* pos, void* x, int dtype, int B, int S, int d,
                                       int64_t n_embed, const int32_t* rows, void* stream) {
  OASR_TEST_DTYPE("oasr_test_embedding_fwd");
  if (dtype == OASR_DTYPE_BF16) return launch_embedding_fwd(tok, E, pos, (bf16_t*)x, B, S, d, (long)n_embed, (hipStream_t)stream, rows);
  return launch_embedding_fwd(tok, E, pos, (float*)x, B, S, d, (long)n_embed, (hipStream_t)stream, rows);
}
extern "C" int oasr_test_embedding_bwd(const int64_t* tok, const void* dx, int dtype, float* dE, float* dpos, int B, int S, int d, int64_t pad_id,
                                       int64_t n_embed, const int32_t* rows, const int32_t* span, void* stream) {
  OASR_TEST_DTYPE("oasr_test_embedding_bwd");
  OASR_REQUIRE(!span || rows, "oasr_test_embedding_bwd: span comes with a chunk-row table");
  if (dtype == OASR_DTYPE_BF16)
    return launch_embedding_bwd(tok, (const bf16_t*)dx, dE, dpos, B, S, d, (long)pad_id, (long)n_embed, (hipStream_t)stream, rows, span);
  return launch_embedding_bwd(tok, (const float*)dx, dE, dpos, B, S, d, (long)pad_id, (long)n_embed, (hipStream_t)stream, rows, span);
}
extern "C" int oasr_test_colsum(const void* x, int dtype, int64_t ld, int64_t M, int ncols, float* out, void* stream) {
  OASR_TEST_DTYPE("oasr_test_colsum");
  if (dtype == OASR_DTYPE_BF16) return launch_colsum_accum((const bf16_t*)x, (long)ld, (long)M, ncols, out, (hipStream_t)stream);
  return launch_colsum_accum((const float*)x, (long)ld, (long)M, ncols, out, (hipStream_t)stream);
}
extern "C" int oasr_test_conv2_col2im_dgelu(const void* dA, const void* u1, void* dpre1, int dtype, int B, int T1, int d, void* stream) {
  OASR_TEST_DTYPE("oasr_test_conv2_col2im_dgelu");
  OASR_REQUIRE(B > 0 && T1 > 0 && d > 0, "oasr_test_conv2_col2im_dgelu: bad shape (B=%d T1=%d d=%d)", B, T1, d);
  if (dtype == OASR_DTYPE_BF16) return launch_conv2_col2im_dgelu((const bf16_t*)dA, (const bf16_t*)u1, (bf16_t*)dpre1, B, T1, d, (hipStream_t)stream);
  return launch_conv2_col2im_dgelu((const float*)dA, (const float*)u1, (float*)dpre1, B, T1, d, (hipStream_t)stream);
}
extern "C" int oasr_test_conv1_col2im_mel(const void* dcol, int dtype, float* dmel, int B, int T1, int n_mels, void* stream) {
  OASR_TEST_DTYPE("oasr_test_conv1_col2im_mel");
  if (dtype == OASR_DTYPE_BF16) return launch_conv1_col2im_mel((const bf16_t*)dcol, dmel, B, T1, n_mels, (hipStream_t)stream);
  return launch_conv1_col2im_mel((const float*)dcol, dmel, B, T1, n_mels, (hipStream_t)stream);
}
extern "C" int oasr_test_mel_to_time_major(const float* mel, void* out, int dtype, int B, int n_mels, int T, const float* clip_max, void* stream) {
  OASR_TEST_DTYPE("oasr_test_mel_to_time_major");
  OASR_REQUIRE(B > 0 && n_mels > 0 && T > 0, "oasr_test_mel_to_time_major: bad shape (B=%d n_mels=%d T=%d)", B, n_mels, T);
  if (dtype == OASR_DTYPE_BF16) return launch_mel_to_time_major(mel, (bf16_t*)out, B, n_mels, T, (hipStream_t)stream, clip_max);
  return launch_mel_to_time_major(mel, (float*)out, B, n_mels, T, (hipStream_t)stream, clip_max);
}
extern "C" int oasr_test_pack_conv_weight(const float* w, void* dst, int dtype, int co, int ci, int ldk, void* stream) {
  OASR_TEST_DTYPE("oasr_test_pack_conv_weight");
  OASR_REQUIRE(co > 0 && ci > 0, "oasr_test_pack_conv_weight: bad shape (co=%d ci=%d)", co, ci);
  if (dtype == OASR_DTYPE_BF16) return launch_pack_conv_weight(w, (bf16_t*)dst, co, ci, ldk, (hipStream_t)stream);
  return launch_pack_conv_weight(w, (float*)dst, co, ci, ldk, (hipStream_t)stream);
}
extern "C" int oasr_test_unpack_conv_grad(const float* g, float* dw, int co, int ci, int ldk, void* stream) {
  OASR_REQUIRE(co > 0 && ci > 0, "oasr_test_unpack_conv_grad: bad shape (co=%d ci=%d)", co, ci);
  return launch_unpack_conv_grad(g, dw, co, ci, ldk, (hipStream_t)stream);
}
extern "C" int oasr_test_pack_embedding(const float* e, void* dst, int rows, int rows_pad, int d, void* stream) {
  OASR_REQUIRE(rows > 0 && d > 0, "oasr_test_pack_embedding: bad shape (rows=%d d=%d)", rows, d);
  return launch_pack_embedding(e, (bf16_t*)dst, rows, rows_pad, d, (hipStream_t)stream);
}
extern "C" int oasr_test_dgelu_mul(const void* dy, const void* u, void* out, int dtype, int64_t n, void* stream) {
  OASR_TEST_DTYPE("oasr_test_dgelu_mul");
  OASR_REQUIRE(n > 0, "oasr_test_dgelu_mul: n = %lld", (long long)n);
  if (dtype == OASR_DTYPE_BF16) return launch_dgelu_mul((const bf16_t*)dy, (const bf16_t*)u, (bf16_t*)out, (long)n, (hipStream_t)stream);
  return launch_dgelu_mul((const float*)dy, (const float*)u, (float*)out, (long)n, (hipStream_t)stream);
}
extern "C" int oasr_test_dlogits_from_f32(const float* src, int V, int64_t rows, int64_t ld, void* dst, int dtype, void* stream) {
  OASR_TEST_DTYPE("oasr_test_dlogits_from_f32");
  OASR_REQUIRE(rows > 0 && V > 0, "oasr_test_dlogits_from_f32: bad shape");
  if (dtype == OASR_DTYPE_BF16) return launch_dlogits_from_f32(src, V, (long)rows, (long)ld, (bf16_t*)dst, (hipStream_t)stream);
  return launch_dlogits_from_f32(src, V, (long)rows, (long)ld, (float*)dst, (hipStream_t)stream);
}
extern "C" int oasr_test_logits_to_f32(const void* logits, int dtype, int64_t ld, int64_t rows, int V, float* out, void* stream) {
  OASR_TEST_DTYPE("oasr_test_logits_to_f32");
  OASR_REQUIRE(logits && out && rows > 0 && V > 0 && V <= ld, "oasr_test_logits_to_f32: bad args");
  if (dtype == OASR_DTYPE_BF16) return launch_logits_to_f32((const bf16_t*)logits, (long)ld, (long)rows, V, out, (hipStream_t)stream);
  return launch_logits_to_f32((const float*)logits, (long)ld, (long)rows, V, out, (hipStream_t)stream);
}
extern "C" int oasr_test_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, const void* dres,
                                       void* dx, float* dgamma, float* dbeta, float* dsum, int dtype, int64_t rows, int d, void* stream) {
  OASR_TEST_DTYPE("oasr_test_layernorm_bwd");
  if (dtype == OASR_DTYPE_BF16)
    return launch_layernorm_bwd((const bf16_t*)dy, (const bf16_t*)x, gamma, mean, rstd, (const bf16_t*)dres, (bf16_t*)dx, dgamma, dbeta, dsum,
                                (long)rows, d, (hipStream_t)stream);
  return launch_layernorm_bwd((const float*)dy, (const float*)x, gamma, mean, rstd, (const float*)dres, (float*)dx, dgamma, dbeta, dsum, (long)rows, d,
                              (hipStream_t)stream);
}

extern "C" int oasr_test_argmax_rows(const void* logits, int dtype, int64_t ld, int V, int64_t n_rows, const int32_t* rows, const int32_t* span, int B,
                                     int S, int32_t* pred_out, void* stream) {
  OASR_TEST_DTYPE("oasr_test_argmax_rows");
  if (dtype == OASR_DTYPE_BF16)
    return launch_argmax_rows((const bf16_t*)logits, (long)ld, V, (long)n_rows, rows, span, B, S, pred_out, (hipStream_t)stream);
  return launch_argmax_rows((const float*)logits, (long)ld, V, (long)n_rows, rows, span, B, S, pred_out, (hipStream_t)stream);
}

// count_valid -> cross-entropy kernel of the logits' type -> loss_reduce: the body of oasr_cross_entropy_ex and of its test twin below
template <typename T>
static int cross_entropy_chain(const char* who, T* logits, int64_t ld, int V, const int64_t* targets, int64_t rows, int64_t ignore, float gscale,
                               int32_t* n_valid_dev, float* row_loss, float* loss_out, int write_grad, float label_smoothing, float z_loss,
                               float* row_parts, hipStream_t st) {
  int rc = check_ce_reg(who, label_smoothing, z_loss);
  if (rc) return rc;
  CeReg reg;
  reg.eps = label_smoothing;
  reg.z = z_loss;
  reg.parts = row_parts;
  reg.parts_stride = (long)rows;
  rc = launch_count_valid(targets, rows, ignore, V, n_valid_dev, st);
  if (rc) return rc;
  rc = launch_cross_entropy(logits, ld, V, targets, rows, ignore, gscale, n_valid_dev, row_loss, write_grad, st, reg);
  if (rc) return rc;
  if (loss_out) rc = launch_loss_reduce(row_loss, rows, n_valid_dev, 1.0f, loss_out, 0, st);
  return rc;
}
extern "C" int oasr_cross_entropy_ex(void* logits, int64_t ld, int V, const int64_t* targets, int64_t rows, int64_t ignore, float gscale,
                                     int32_t* n_valid_dev, float* row_loss, float* loss_out, int write_grad, float label_smoothing, float z_loss,
                                     float* row_parts, void* stream) {
  return cross_entropy_chain("oasr_cross_entropy_ex", (bf16_t*)logits, ld, V, targets, rows, ignore, gscale, n_valid_dev, row_loss, loss_out,
                             write_grad, label_smoothing, z_loss, row_parts, (hipStream_t)stream);
}
extern "C" int oasr_test_cross_entropy(void* logits, int dtype, int64_t ld, int V, const int64_t* targets, int64_t rows, int64_t ignore, float gscale,
                                       int32_t* n_valid_dev, float* row_loss, float* loss_out, int write_grad, float label_smoothing,
                                       float z_loss, float* row_parts, void* stream) {
  OASR_TEST_DTYPE("oasr_test_cross_entropy");
  if (dtype == OASR_DTYPE_BF16)
    return cross_entropy_chain("oasr_test_cross_entropy", (bf16_t*)logits, ld, V, targets, rows, ignore, gscale, n_valid_dev, row_loss, loss_out,
                               write_grad, label_smoothing, z_loss, row_parts, (hipStream_t)stream);
  return cross_entropy_chain("oasr_test_cross_entropy", (float*)logits, ld, V, targets, rows, ignore, gscale, n_valid_dev, row_loss, loss_out,
                             write_grad, label_smoothing, z_loss, row_parts, (hipStream_t)stream);
}
extern "C" int oasr_cross_entropy(void* logits, int64_t ld, int V, const int64_t* targets, int64_t rows, int64_t ignore, float gscale,
                                  int32_t* n_valid_dev, float* row_loss, float* loss_out, int write_grad, void* stream) {
  return oasr_cross_entropy_ex(logits, ld, V, targets, rows, ignore, gscale, n_valid_dev, row_loss, loss_out, write_grad, 0.f, 0.f, nullptr, stream);
}

extern "C" int oasr_pick_tokens(const float* logits, int64_t ld, int V, int64_t rows, const float* mask, const float* mask2, int64_t* tok,
                                float* logprob, void* stream) {
  SelectArgs a{logits, ld, V, rows, mask, mask2};
  a.tok = tok;
  a.logprob = logprob;
  return launch_pick_tokens(a, (hipStream_t)stream);
}
extern "C" int oasr_pick_tokens_ts(const float* logits, int64_t ld, int V, int64_t rows, const float* mask, const float* mask2,
                                   const int64_t* history, int64_t history_ld, int n_history, int timestamp_begin, int eot, int no_timestamps,
                                   int max_initial_index, int64_t* tok, float* logprob, void* stream) {
  return launch_pick_tokens_ts({logits, ld, V, rows, mask, mask2, history, history_ld, n_history, timestamp_begin, eot, no_timestamps,
                                max_initial_index, tok, logprob}, (hipStream_t)stream);
}
extern "C" int oasr_topk_tokens(const float* logits, int64_t ld, int V, int64_t rows, const float* mask, const float* mask2,
                                const int64_t* history, int64_t history_ld, int n_history, int timestamp_begin, int eot, int no_timestamps,
                                int max_initial_index, int K, int64_t* tok, float* logprob, void* stream) {
  return launch_topk_tokens_ts({logits, ld, V, rows, mask, mask2, history, history_ld, n_history, timestamp_begin, eot, no_timestamps,
                                max_initial_index, tok, logprob}, K, (hipStream_t)stream);
}
extern "C" int oasr_sample_tokens(const float* logits, int64_t ld, int V, int64_t rows, const float* mask, const float* mask2,
                                  const int64_t* history, int64_t history_ld, int n_history, int timestamp_begin, int eot, int no_timestamps,
                                  int max_initial_index, float temperature, const float* uniforms, int64_t* tok, float* logprob, void* stream) {
  return launch_sample_tokens_ts({logits, ld, V, rows, mask, mask2, history, history_ld, n_history, timestamp_begin, eot, no_timestamps,
                                  max_initial_index, tok, logprob}, temperature, uniforms, (hipStream_t)stream);
}

extern "C" int oasr_cast_f32_bf16(const float* src, void* dst, int64_t n, void* stream) {
  return launch_cast_f32_bf16(src, (bf16_t*)dst, n, (hipStream_t)stream);
}

// One wave: LDS image = src [16 rows][64 cols] bf16 (128-byte rows); lane l reads 8 bytes at
// row (l >> 4)*4 + ((l & 15) >> 2), col ((l & 15) & 3) * 4 through ds_read_b64_tr_b16 and stores its 4 results.
typedef __attribute__((address_space(3))) s16x4_t* lds_s16x4_ptr_t;
__global__ void probe_tr16_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst) {
  __shared__ __attribute__((aligned(16))) bf16_t tile[16 * 64];
  const int l = threadIdx.x;
  for (int i = l; i < 16 * 64; i += 64) tile[i] = src[i];
  __syncthreads();
  const int row = (l >> 4) * 4 + ((l & 15) >> 2), col = ((l & 15) & 3) * 4;
  const s16x4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr_t)(tile + row * 64 + col));
  for (int j = 0; j < 4; ++j) dst[l * 4 + j] = (bf16_t)v[j];
}
// One wave: LDS pre-filled with 0xAAAA; lanes < 32 issue an in-range 16-byte buffer_load..lds, lanes >= 32 an
// out-of-range one (offset beyond num_records).  dst[64*8] u16 shows what the hardware writes for OOB lanes.
typedef __attribute__((address_space(3))) void* lds_void_ptr_t;
__global__ void probe_lds_oob_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst) {
  __shared__ __attribute__((aligned(16))) bf16_t tile[64 * 8];
  const int l = threadIdx.x;
  for (int i = l; i < 64 * 8; i += 64) tile[i] = 0xAAAA;
  __syncthreads();
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(src), 0, 64 * 16, 0x00020000);
  const unsigned off = l < 32 ? l * 16 : 0x80000000u;
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_ptr_t)tile, 16, off, 0, 0, 0);
  __syncthreads();
  for (int i = l; i < 64 * 8; i += 64) dst[i] = tile[i];
}
extern "C" int oasr_probe_lds_oob(const void* src, void* dst, void* stream) {
  hipLaunchKernelGGL(probe_lds_oob_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const bf16_t*)src, (bf16_t*)dst);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}
extern "C" int oasr_probe_tr16(const void* src, void* dst, void* stream) {
  hipLaunchKernelGGL(probe_tr16_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const bf16_t*)src, (bf16_t*)dst);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}
