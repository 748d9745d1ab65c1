// Entry points of the inference forward and of every training step (plain, supervised-span, cut at the logits, staged at xa): argument checks,
// one Step<T> (engine_run.h) per call, and the order in which the Runner's halves are issued.
#include "engine_run.h"

// Runner::side_mode of the span step (engine_side.h: SideMode).  7 = the decoder backward's R-row weight gradients, the cross-attention key|value gradients AND the
// forward's key|value projections on the lowest-priority side streams: -1.4..-1.55 % of the step against no side streams, -0.7 % against mode 5
// (same-box A/Bs, profiles/r05_side_streams.txt; round 6 re-measured: profiles/r06_side_streams.txt).  The 48 forward projections share the
// dominant forward kernel's symbol; as filler their begin-to-end spans are queueing times, so the GEMM launch statistics carry the lane a
// launch ran on (gemm_profile_lane, set by SideStreams::OnStream) and bench.py's `roofline` / scripts/rocprof_summary.py price main-stream launches only.
constexpr int SIDE_STREAMS_DEFAULT = SIDE_WGRAD | SIDE_KV_FWD | SIDE_KV_BWD;

template <typename T>
static size_t plan_bytes(const oasr_ctx* c, int B, int S, bool train, int stage) {
  return Step<T>(c, nullptr, 0, nullptr, B, S, nullptr, train, stage).A.cur;
}
extern "C" size_t oasr_workspace_bytes(const oasr_ctx* c, int B, int S, int mode) {
  if (!c || B <= 0 || S <= 0 || mode < OASR_MODE_INFER || mode > OASR_MODE_TRAIN_DEC) return 0;
  const bool train = mode != OASR_MODE_INFER;
  const int stage = mode == OASR_MODE_TRAIN_ENC ? STAGE_ENC : mode == OASR_MODE_TRAIN_DEC ? STAGE_DEC : STAGE_ALL;
  return OASR_BY_DTYPE(c, plan_bytes, c, B, S, train, stage) + 4096;
}

template <typename T>
static int oasr_forward_impl(oasr_ctx* c, const float* mel, const int64_t* tokens, const int32_t* text_len, int B, int S,
                            float* logits_out, void* xa_out, void* workspace, size_t workspace_bytes, void* stream) {
  RC(check_bound(c, false));
  OASR_REQUIRE(mel && tokens && workspace && B > 0 && S > 0 && S <= c->S_max, "oasr_forward: bad args (B=%d S=%d)", B, S);
  OASR_REQUIRE(workspace_bytes >= oasr_workspace_bytes(c, B, S, OASR_MODE_INFER), "oasr_forward: workspace too small");
  Step<T> s(c, workspace, workspace_bytes, stream, B, S, text_len, false);
  RC(s.r.encoder_fwd(s.p, mel));
  RC(s.r.decoder_fwd(s.p, tokens));
  if (xa_out) RC(copy_xa<T>(c, xa_out, s.p.xa, B, s.r.st));
  if (logits_out) RC(launch_logits_to_f32(s.p.logits, c->Vp, (long)B * S, c->V, logits_out, s.r.st));
  return OASR_OK;
}
extern "C" int oasr_forward(oasr_ctx* c, const float* mel, const int64_t* tokens, const int32_t* text_len, int B, int S,
                            float* logits_out, void* xa_out, void* workspace, size_t workspace_bytes, void* stream) {
  OASR_REQUIRE(c, "oasr_forward: null context");
  return OASR_BY_DTYPE(c, oasr_forward_impl, c, mel, tokens, text_len, B, S, logits_out, xa_out, workspace, workspace_bytes, stream);
}

// ---- teacher-forced scoring (oasr_score; the contract: include/oasr.h at oasr_score_args): oasr_forward's forward, then score.hip's two
// launches on the logits in the compute dtype.  Every refusal, before anything is launched or dereferenced:
static int score_check(const oasr_ctx* c, const oasr_score_args* a, const void* workspace, size_t workspace_bytes) {
  RC(check_bound(c, false));
  OASR_REQUIRE(a, "oasr_score: null args");
  OASR_REQUIRE(!a->mel != !a->xa, "oasr_score: exactly one of mel and xa is required (mel: the whole forward; xa: the decoder alone on given features)");
  OASR_REQUIRE(a->tokens && a->targets && a->span && workspace, "oasr_score: bad args (tokens, targets, span and workspace are required)");
  OASR_REQUIRE(a->row_nll && a->pred && a->nll_sum && a->nll_max && a->n_tok && a->n_hit,
               "oasr_score: bad args (row_nll, pred [B, S] and nll_sum, nll_max, n_tok, n_hit [B] are required)");
  OASR_REQUIRE(a->B > 0 && a->S > 0 && a->S <= c->S_max, "oasr_score: B=%d must be positive and S=%d inside (0, n_text_ctx=%d]", a->B, a->S, c->S_max);
  OASR_REQUIRE(workspace_bytes >= oasr_workspace_bytes(c, a->B, a->S, OASR_MODE_INFER), "oasr_score: workspace too small");
  return OASR_OK;
}
template <typename T>
static int oasr_score_impl(oasr_ctx* c, const oasr_score_args& a, void* workspace, size_t workspace_bytes, void* stream) {
  Step<T> s(c, workspace, workspace_bytes, stream, a.B, a.S, a.text_len, false);
  if (a.xa) RC(copy_xa<T>(c, s.p.xa, a.xa, a.B, s.r.st));
  else RC(s.r.encoder_fwd(s.p, a.mel));
  RC(s.r.decoder_fwd(s.p, a.tokens));
  RC(launch_score_rows(s.p.logits, c->Vp, c->V, a.targets, a.span, a.B, a.S, PAD_ID, a.row_nll, a.pred, s.r.st));
  return launch_score_reduce(a.row_nll, a.pred, a.targets, a.span, a.B, a.S, c->V, PAD_ID, a.nll_sum, a.nll_max, a.n_tok, a.n_hit, s.r.st);
}
extern "C" int oasr_score(oasr_ctx* c, const oasr_score_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  RC(score_check(c, a, workspace, workspace_bytes));
  return OASR_BY_DTYPE(c, oasr_score_impl, c, *a, workspace, workspace_bytes, stream);
}

// AudioEncoder.forward (olmoasr/model.py:571-623): mel -> xa bf16 [B, n_audio_ctx, d]
template <typename T>
static int oasr_encode_impl(oasr_ctx* c, const float* mel, int B, void* xa_out, void* workspace, size_t workspace_bytes, void* stream) {
  RC(check_bound(c, false));
  OASR_REQUIRE(mel && xa_out && workspace && B > 0, "oasr_encode: bad args");
  OASR_REQUIRE(workspace_bytes >= oasr_workspace_bytes(c, B, 1, OASR_MODE_INFER), "oasr_encode: workspace too small");
  Step<T> s(c, workspace, workspace_bytes, stream, B, 1, nullptr, false);
  RC(s.r.encoder_fwd(s.p, mel));
  return copy_xa<T>(c, xa_out, s.p.xa, B, s.r.st);
}
extern "C" int oasr_encode(oasr_ctx* c, const float* mel, int B, void* xa_out, void* workspace, size_t workspace_bytes, void* stream) {
  OASR_REQUIRE(c, "oasr_encode: null context");
  return OASR_BY_DTYPE(c, oasr_encode_impl, c, mel, B, xa_out, workspace, workspace_bytes, stream);
}

// TextDecoder.forward without kv_cache (olmoasr/model.py:688-775) on given audio features: OLMoASR.logits(tokens, xa).
// last_only != 0: logits_out is f32 [B, rows] for position S-1 only (greedy decode step); else f32 [B, S, rows].
template <typename T>
static int oasr_decode_logits_impl(oasr_ctx* c, const int64_t* tokens, const void* xa, const int32_t* text_len, int B, int S,
                                  int last_only, float* logits_out, void* workspace, size_t workspace_bytes, void* stream) {
  RC(check_bound(c, false));
  OASR_REQUIRE(tokens && xa && logits_out && workspace && B > 0 && S > 0 && S <= c->S_max, "oasr_decode_logits: bad args");
  OASR_REQUIRE(workspace_bytes >= oasr_workspace_bytes(c, B, S, OASR_MODE_INFER), "oasr_decode_logits: workspace too small");
  Step<T> s(c, workspace, workspace_bytes, stream, B, S, text_len, false);
  RC(copy_xa<T>(c, s.p.xa, xa, B, s.r.st));
  RC(s.r.decoder_fwd(s.p, tokens, last_only != 0));
  return launch_logits_to_f32(s.p.logits, c->Vp, last_only ? (long)B : (long)B * S, c->V, logits_out, s.r.st);
}
extern "C" int oasr_decode_logits(oasr_ctx* c, const int64_t* tokens, const void* xa, const int32_t* text_len, int B, int S,
                                  int last_only, float* logits_out, void* workspace, size_t workspace_bytes, void* stream) {
  OASR_REQUIRE(c, "oasr_decode_logits: null context");
  return OASR_BY_DTYPE(c, oasr_decode_logits_impl, c, tokens, xa, text_len, B, S, last_only, logits_out, workspace, workspace_bytes, stream);
}

// Side streams of the supervised-span step (Runner::side_mode): the setter is a testing hook, OASR_SIDE_STREAMS an experiment switch
static int g_side_streams = -1;
static int span_side_streams() {
  if (g_side_streams >= 0) return g_side_streams;
  static const int env = [] {
    const char* e = oasr_experiment_env("OASR_SIDE_STREAMS");
    return e ? atoi(e) : -1;
  }();
  return env >= 0 ? (env & SIDE_ALL) : SIDE_STREAMS_DEFAULT;
}
extern "C" int oasr_span_side_streams(void) { return span_side_streams(); }
extern "C" int oasr_span_set_side_streams(int mode) {
  OASR_HOOK_GATE("oasr_span_set_side_streams");
  g_side_streams = mode < 0 ? -1 : (mode & SIDE_ALL);
  return OASR_OK;
}

// ---- the fused micro-step (oasr_train_step; the contract of every field: include/oasr.h at oasr_train_step_args) -----------------------
// S < n_text_ctx (text_ctx): with S >= max(text_len) rounded up, the loss, every gradient and therefore the optimizer step are those of
// the full padded context: positions past the last real token only ever see ignore_index targets, and no real query attends to them
// (causal mask), so the reference spends their share of the decoder on exact zeros (train_timestamps.py:318-329 pads every sample to 448).
// span_host, the supervised-span step: same forward (all n_text_ctx positions, as the reference pads them), same loss, same gradients; what
// changes is WHERE the decoder's token rows live and how much of the backward is executed.  span_host[b] (host memory, known to the
// data loader: train_timestamps.py:238-343 builds the token sequences on the host) bounds the positions of sample b that can carry
// gradient: every target at or past it is ignore_index (train_timestamps.py:1444) and it is >= text_len[b], the first masked key
// column (:314-315).  Rows of every decoder-side gradient past the span are exactly zero in the reference's computation -- the loss
// ignores them, no supervised query attends to them -- so:
//   * the decoder's activations are laid out in 64-position CHUNKS, every chunk with a position < span first (kernels.h:
//     AttnArgs.q_rows; only the embedding, the attention kernels and the target gather know about the permutation -- LayerNorm, the
//     GEMMs and their epilogues are row-wise and see plain matrices);
//   * the backward of the decoder (dgrad / wgrad GEMMs, LayerNorm, attention, cross-entropy gradient, embedding scatter) runs on the
//     leading R = sum_b ceil64(span[b]) rows only -- on the synthetic lengths 1/3 of the 448 * B.
// The results differ from the plain step's only by fp32 summation order (weight gradients sum over fewer, re-ordered token rows).
// A shape the row table cannot chunk takes the plain step (same results): span_chunkable, train_plan.h.

// Every refusal of oasr_train_step, before anything is launched or dereferenced: the arguments, then the workspace size, then the context's state.
static int train_step_check(const oasr_ctx* c, const oasr_train_step_args* a, const void* workspace, size_t workspace_bytes) {
  RC(check_bound(c, true));
  OASR_REQUIRE(a, "oasr_train_step: null args");
  OASR_REQUIRE(!a->mel != !a->xa, "oasr_train_step: exactly one of mel and xa is required (mel: the whole step; xa: the decoder alone on given features)");
  OASR_REQUIRE(a->tokens && a->targets && a->text_len && a->loss_out && workspace,
               "oasr_train_step: bad args (tokens, targets, text_len, loss_out and workspace are required)");
  OASR_REQUIRE(a->B > 0 && a->S > 0 && a->S <= c->S_max, "oasr_train_step: B=%d must be positive and S=%d inside (0, n_text_ctx=%d]", a->B, a->S, c->S_max);
  if (a->span_host) {
    OASR_REQUIRE(a->S == c->S_max, "oasr_train_step: a span step covers the whole context (S = %d, n_text_ctx = %d)", a->S, c->S_max);
    OASR_REQUIRE(a->span_forward == OASR_SPAN_FORWARD_ALL || a->span_forward == OASR_SPAN_FORWARD_ACTIVE, "oasr_train_step: span_forward");
    OASR_REQUIRE(!a->logits_out, "oasr_train_step: logits_out belongs to the plain step (the span step keeps no fp32 logits)");
  } else {
    OASR_REQUIRE(!a->pred_out, "oasr_train_step: pred_out comes with span_host (the predictions cover the span's rows)");
    OASR_REQUIRE(!a->mel_clip_max, "oasr_train_step: mel_clip_max comes with span_host (the un-finalized log-mel is consumed by the span step only)");
  }
  OASR_REQUIRE(!a->xa || (!a->mel_clip_max && !a->logits_out), "oasr_train_step: mel_clip_max / logits_out do not apply to the step from a given xa");
  // pred_out is indexed through the row table: no plain-step fall-back with it
  OASR_REQUIRE(!a->pred_out || span_chunkable(c->S_max, a->B),
               "pred_out needs the chunk-row table: n_text_ctx = %d must be a multiple of 64 (<= %d) and B = %d <= 512", c->S_max, 64 * OASR_ROWTAB, a->B);
  RC(check_ce_reg("oasr_train_step", a->label_smoothing, a->z_loss));
  OASR_REQUIRE(!a->loss_parts_out || a->loss_parts_rows, "oasr_train_step: loss_parts_out needs loss_parts_rows (f32 [2, B * S] of per-row scratch the caller owns)");
  OASR_REQUIRE(workspace_bytes >= oasr_workspace_bytes(c, a->B, a->S, a->xa ? OASR_MODE_TRAIN_DEC : OASR_MODE_TRAIN), "oasr_train_step: workspace too small");
  if (a->xa && c->pr.enc_any) {
    oasr_set_error("oasr_train_step: an encoder tensor is trainable -- the step from a given xa has no encoder backward (freeze the "
                   "encoder, or pass mel)");
    return OASR_ESTATE;
  }
  return OASR_OK;
}

// chunked: the supervised-span step over the chunk-row table; else the plain step over B * S rows (an unchunkable span call included)
template <typename T>
static int train_step_impl(oasr_ctx* c, const oasr_train_step_args& a, bool chunked, void* workspace, size_t workspace_bytes, void* stream) {
  const int B = a.B, S = a.S;
  const long Md = (long)B * S;
  Step<T> s(c, workspace, workspace_bytes, stream, B, S, a.text_len, true, a.xa ? STAGE_DEC : STAGE_ALL);  // (s.r.lane: the lane tag is put back on every path)
  auto& p = s.p;
  auto& r = s.r;
  hipStream_t st = r.st;
  r.mel_clip_max = a.mel_clip_max;  // un-finalized log-mel (oasr_log_mel_raw): the floor / scale lines ride in the encoder's transpose
  const int64_t* ce_targets = a.targets;  // cross-entropy over every row, or over the R active rows in row order
  long ce_rows = Md;
  if (chunked) {
    long R = 0;
    SpanBlockTables blk{c->H, p.blk128, p.blk256, 0, 0};
    RC(launch_build_span_tables(a.span_host, B, S, a.targets, PAD_ID, p.rows, p.span_dev, p.targets_phys, &R, st, p.blk128 ? &blk : nullptr));
    OASR_REQUIRE(R > 0, "oasr_train_step: no position of the micro-batch carries gradient (every span is 0)");
    r.dec_rows = p.rows;
    r.dec_span = p.span_dev;
    r.dec_blk128 = p.blk128;
    r.dec_blk256 = p.blk256;
    r.dec_n128 = blk.n128;
    r.dec_n256 = blk.n256;
    r.dec_rows_bwd = R;
    r.dec_rows_fwd = a.span_forward == OASR_SPAN_FORWARD_ACTIVE ? R : 0;
    if (const int mode = span_side_streams()) RC(r.side_begin(mode));
    ce_targets = p.targets_phys;
    ce_rows = R;
  }
  // ---------------- forward (every position, unless the caller of a span step opted out of the padded ones) ----------------
  if (a.xa) RC(copy_xa<T>(c, p.xa, a.xa, B, st));
  else RC(r.encoder_fwd(p, a.mel));
  RC(r.decoder_fwd(p, a.tokens));
  if (a.logits_out) RC(launch_logits_to_f32(p.logits, c->Vp, Md, c->V, a.logits_out, st));
  // predictions on request, while the logits are still logits (the cross-entropy below overwrites them with their gradient)
  if (a.pred_out) RC(launch_argmax_rows(p.logits, c->Vp, c->V, Md, p.rows, p.span_dev, B, S, a.pred_out, st));
  // loss (chunked: over the active rows; the other rows' targets are ignore_index: they add nothing to the sum and nothing to the count)
  RC(launch_count_valid(a.targets, Md, PAD_ID, c->V, p.n_valid, st));
  // label smoothing / z-loss (all zero: the plain kernel); the parts' per-row values go to the caller's scratch, never to the workspace
  CeReg reg;
  reg.eps = a.label_smoothing;
  reg.z = a.z_loss;
  reg.parts = a.loss_parts_out ? a.loss_parts_rows : nullptr;
  reg.parts_stride = Md;
  RC(launch_cross_entropy(p.logits, c->Vp, c->V, ce_targets, ce_rows, PAD_ID, a.loss_scale * a.inv_accum, p.n_valid, p.row_loss, 1, st, reg));
  RC(launch_loss_reduce(p.row_loss, ce_rows, p.n_valid, a.inv_accum, a.loss_out, a.accumulate_loss, st));
  if (reg.parts) {
    RC(launch_loss_reduce(reg.parts, ce_rows, p.n_valid, a.inv_accum, a.loss_parts_out, a.accumulate_loss, st));
    RC(launch_loss_reduce(reg.parts + Md, ce_rows, p.n_valid, a.inv_accum, a.loss_parts_out + 1, a.accumulate_loss, st));
  }
  return r.train_backward(p, a.tokens, a.seg_events);
}
extern "C" size_t oasr_sizeof_train_step_args(void) { return sizeof(oasr_train_step_args); }
extern "C" int oasr_train_step(oasr_ctx* c, const oasr_train_step_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  RC(train_step_check(c, a, workspace, workspace_bytes));
  return OASR_BY_DTYPE(c, train_step_impl, c, *a, a->span_host && span_chunkable(c->S_max, a->B), workspace, workspace_bytes, stream);
}

// ---- the same micro-step cut at the logits, for torch.autograd (OLMoASR.forward in training mode, olmoasr/model.py:856-887 followed
// by the caller's own loss, train_timestamps.py:1440-1454): oasr_train_fwd returns fp32 logits [B, S, rows] and leaves every saved
// activation in the workspace; oasr_train_bwd takes d(loss)/d(logits) (fp32, same shape; rounded to the engine's activation type
// exactly where autocast's backward would round it) and accumulates the parameter gradients into the bound arena.  The workspace
// must not be used for anything else in between; B, S, tokens and text_len must be the forward's.
template <typename T>
static int oasr_train_fwd_impl(oasr_ctx* c, const float* mel, const int64_t* tokens, const int32_t* text_len, int B, int S,
                               float* logits_out, void* workspace, size_t workspace_bytes, void* stream) {
  Step<T> s(c, workspace, workspace_bytes, stream, B, S, text_len, true);
  RC(s.r.encoder_fwd(s.p, mel));
  RC(s.r.decoder_fwd(s.p, tokens));
  return launch_logits_to_f32(s.p.logits, c->Vp, (long)B * S, c->V, logits_out, s.r.st);
}
template <typename T>
static int oasr_train_bwd_impl(oasr_ctx* c, const int64_t* tokens, const int32_t* text_len, const float* dlogits, int B, int S, void** ev,
                               void* workspace, size_t workspace_bytes, void* stream) {
  Step<T> s(c, workspace, workspace_bytes, stream, B, S, text_len, true);
  RC(launch_dlogits_from_f32(dlogits, c->V, (long)B * S, c->Vp, s.p.logits, s.r.st));
  return s.r.train_backward(s.p, tokens, ev);
}
extern "C" int oasr_train_fwd(oasr_ctx* c, const float* mel, const int64_t* tokens, const int32_t* text_len, int B, int S, float* logits_out,
                              void* workspace, size_t workspace_bytes, void* stream) {
  RC(check_bound(c, true));
  OASR_REQUIRE(S > 0 && S <= c->S_max, "oasr_train_fwd: S=%d outside (0, n_text_ctx=%d]", S, c->S_max);
  OASR_REQUIRE(mel && tokens && text_len && logits_out && workspace && B > 0, "oasr_train_fwd: bad args");
  OASR_REQUIRE(workspace_bytes >= oasr_workspace_bytes(c, B, S, OASR_MODE_TRAIN), "oasr_train_fwd: workspace too small");
  return OASR_BY_DTYPE(c, oasr_train_fwd_impl, c, mel, tokens, text_len, B, S, logits_out, workspace, workspace_bytes, stream);
}
extern "C" int oasr_train_bwd(oasr_ctx* c, const int64_t* tokens, const int32_t* text_len, const float* dlogits, int B, int S, void** ev,
                              void* workspace, size_t workspace_bytes, void* stream) {
  RC(check_bound(c, true));
  OASR_REQUIRE(S > 0 && S <= c->S_max, "oasr_train_bwd: S=%d outside (0, n_text_ctx=%d]", S, c->S_max);
  OASR_REQUIRE(tokens && text_len && dlogits && workspace && B > 0, "oasr_train_bwd: bad args");
  OASR_REQUIRE(workspace_bytes >= oasr_workspace_bytes(c, B, S, OASR_MODE_TRAIN), "oasr_train_bwd: workspace too small");
  return OASR_BY_DTYPE(c, oasr_train_bwd_impl, c, tokens, text_len, dlogits, B, S, ev, workspace, workspace_bytes, stream);
}

// ---- the training step in two stages, for torch.autograd through model.encoder / model.decoder -------------------
// Each stage has a workspace plan of its own (OASR_MODE_TRAIN_ENC / _DEC) that holds one forward's saved activations until its backward.
// The forwards are the fused training forward's (train = true: the MLP epilogue saves GELU'(u)), cut at xa: encode then decode runs the
// kernels of oasr_train_fwd on the same inputs, plus one copy of xa into the decoder's plan.  The backwards are the two halves of
// Runner::train_backward, started from the caller's d(logits) / d(xa); a requested input gradient (d(xa), d(mel)) is computed even where the mask
// would prune it, and an all-frozen mask is accepted when one is requested.
template <typename T>
static int oasr_train_encode_impl(oasr_ctx* c, const float* mel, int B, void* xa_out, void* workspace, size_t workspace_bytes, void* stream) {
  Step<T> s(c, workspace, workspace_bytes, stream, B, 1, nullptr, true, STAGE_ENC);
  RC(s.r.encoder_fwd(s.p, mel));
  return copy_xa<T>(c, xa_out, s.p.xa, B, s.r.st);
}
template <typename T>
static int oasr_train_encode_bwd_impl(oasr_ctx* c, const void* dxa, int B, float* dmel_out, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  RC(backward_check(c, dmel_out != nullptr));
  Step<T> s(c, workspace, workspace_bytes, stream, B, 1, nullptr, true, STAGE_ENC);
  RC(s.r.backward_begin(s.p));
  int seg = 0;
  RC(s.r.backward_encoder(s.p, (const T*)dxa, nullptr, seg, dmel_out));
  return s.r.backward_finish(s.p, nullptr, seg, STAGE_ENC);
}
template <typename T>
static int oasr_train_decode_impl(oasr_ctx* c, const int64_t* tokens, const void* xa, const int32_t* text_len, int B, int S, float* logits_out,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  Step<T> s(c, workspace, workspace_bytes, stream, B, S, text_len, true, STAGE_DEC);
  RC(copy_xa<T>(c, s.p.xa, xa, B, s.r.st));
  RC(s.r.decoder_fwd(s.p, tokens));
  return launch_logits_to_f32(s.p.logits, c->Vp, (long)B * S, c->V, logits_out, s.r.st);
}
template <typename T>
static int oasr_train_decode_bwd_impl(oasr_ctx* c, const int64_t* tokens, const int32_t* text_len, const float* dlogits, int B, int S,
                                      void* dxa_out, void* workspace, size_t workspace_bytes, void* stream) {
  RC(backward_check(c, dxa_out != nullptr));
  Step<T> s(c, workspace, workspace_bytes, stream, B, S, text_len, true, STAGE_DEC);
  RC(launch_dlogits_from_f32(dlogits, c->V, (long)B * S, c->Vp, s.p.logits, s.r.st));
  RC(s.r.backward_begin(s.p));
  int seg = 0;
  RC(s.r.backward_decoder(s.p, tokens, nullptr, seg, dxa_out != nullptr));
  // d(xa) in the compute dtype, summed over the decoder layers in block_bwd's order (top layer first)
  if (dxa_out) RC(copy_xa<T>(c, dxa_out, s.p.gxa, B, s.r.st));
  return s.r.backward_finish(s.p, nullptr, seg, STAGE_DEC);
}
extern "C" int oasr_train_encode(oasr_ctx* c, const float* mel, int B, void* xa_out, void* workspace, size_t workspace_bytes, void* stream) {
  RC(check_bound(c, true));
  OASR_REQUIRE(mel && xa_out && workspace && B > 0, "oasr_train_encode: bad args (mel, xa_out and workspace are required, B > 0)");
  OASR_REQUIRE(workspace_bytes >= oasr_workspace_bytes(c, B, 1, OASR_MODE_TRAIN_ENC), "oasr_train_encode: workspace too small");
  return OASR_BY_DTYPE(c, oasr_train_encode_impl, c, mel, B, xa_out, workspace, workspace_bytes, stream);
}
extern "C" int oasr_train_encode_bwd(oasr_ctx* c, const void* dxa, int B, float* dmel_out, void* workspace, size_t workspace_bytes, void* stream) {
  RC(check_bound(c, true));
  OASR_REQUIRE(dxa && workspace && B > 0, "oasr_train_encode_bwd: bad args (dxa and workspace are required, B > 0)");
  OASR_REQUIRE(workspace_bytes >= oasr_workspace_bytes(c, B, 1, OASR_MODE_TRAIN_ENC), "oasr_train_encode_bwd: workspace too small");
  return OASR_BY_DTYPE(c, oasr_train_encode_bwd_impl, c, dxa, B, dmel_out, workspace, workspace_bytes, stream);
}
extern "C" int oasr_train_decode(oasr_ctx* c, const int64_t* tokens, const void* xa, const int32_t* text_len, int B, int S, float* logits_out,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  RC(check_bound(c, true));
  OASR_REQUIRE(S > 0 && S <= c->S_max, "oasr_train_decode: S=%d outside (0, n_text_ctx=%d]", S, c->S_max);
  OASR_REQUIRE(tokens && xa && text_len && logits_out && workspace && B > 0,
               "oasr_train_decode: bad args (tokens, xa, text_len, logits_out and workspace are required, B > 0)");
  OASR_REQUIRE(workspace_bytes >= oasr_workspace_bytes(c, B, S, OASR_MODE_TRAIN_DEC), "oasr_train_decode: workspace too small");
  return OASR_BY_DTYPE(c, oasr_train_decode_impl, c, tokens, xa, text_len, B, S, logits_out, workspace, workspace_bytes, stream);
}
extern "C" int oasr_train_decode_bwd(oasr_ctx* c, const int64_t* tokens, const int32_t* text_len, const float* dlogits, int B, int S, void* dxa_out,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  RC(check_bound(c, true));
  OASR_REQUIRE(S > 0 && S <= c->S_max, "oasr_train_decode_bwd: S=%d outside (0, n_text_ctx=%d]", S, c->S_max);
  OASR_REQUIRE(tokens && text_len && dlogits && workspace && B > 0,
               "oasr_train_decode_bwd: bad args (tokens, text_len, dlogits and workspace are required, B > 0)");
  OASR_REQUIRE(workspace_bytes >= oasr_workspace_bytes(c, B, S, OASR_MODE_TRAIN_DEC), "oasr_train_decode_bwd: workspace too small");
  return OASR_BY_DTYPE(c, oasr_train_decode_bwd_impl, c, tokens, text_len, dlogits, B, S, dxa_out, workspace, workspace_bytes, stream);
}
