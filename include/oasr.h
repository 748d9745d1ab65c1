/* liboasr -- C ABI of the MI355X-native OLMoASR training hot path.
 *
 * The reference (allenai/OLMoASR) is pure Python: it has no FFI.  Its "boundary" for this path is the Python surface
 * of olmoasr/model.py + scripts/training/train_timestamps.py; every entry point below names the reference call site
 * it replaces.  olmoasr_amd/ (Python, ctypes) mirrors that surface on top of this ABI; INTEGRATION.md shows the stub a
 * reference maintainer would add.
 *
 * Conventions: all pointers are DEVICE pointers owned by the caller unless stated; every function is asynchronous on
 * `stream` (a hipStream_t passed as void*), never synchronises, returns 0 on success or a negative OASR_E* code and
 * leaves a message retrievable by oasr_last_error().  One host thread per process (rank) drives a context.
 * bf16 tensors are raw uint16 bit patterns.  No exceptions cross the ABI.
 */
#ifndef OASR_H
#define OASR_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define OASR_OK 0
#define OASR_EINVAL (-1)
#define OASR_EHIP (-2)
#define OASR_ESTATE (-3)
#define OASR_ERETRY (-4) /* oasr_decode_check: the window's steps must be enqueued again (the context changed engines; see there) */

typedef struct oasr_ctx oasr_ctx;

/* olmoasr/config/model_dims.py:4-25 (ModelDimensions) */
typedef struct oasr_dims {
  int n_mels, n_audio_ctx, n_audio_state, n_audio_head, n_audio_layer;
  int n_vocab, n_text_ctx, n_text_state, n_text_head, n_text_layer;
} oasr_dims;

const char* oasr_last_error(void);
/* ABI version: 100 * major + minor.  Structs passed by pointer (oasr_attn_args, oasr_gemm_args) only grow at the end and only with a
 * major bump; olmoasr_amd/_native.py refuses to drive a library whose version differs from OASR_ABI_VERSION. */
#define OASR_ABI_VERSION 216
int oasr_version(void);

/* ---- log-mel front end: whisper.audio.log_mel_spectrogram as called at train_timestamps.py:196,214 and
 *      olmoasr/transcribe.py:148 (re-exported olmoasr/__init__.py:21).  pcm_dtype 0 = f32 waveform, 1 = int16 PCM
 *      (scaled by 1/32768 like train_timestamps.py:196).  mel: f32 [B, 80, n_samples/160].  The dynamic-range floor
 *      (max - 8) is per clip.  workspace: oasr_log_mel_workspace_bytes(B) bytes. */
size_t oasr_log_mel_workspace_bytes(int B);
int oasr_log_mel(const void* pcm, int pcm_dtype, int B, int n_samples, float* mel, void* workspace, void* stream);
/* The same front end without its last pass over the tensor: mel_raw = log10(max(mel power, 1e-10)), clip_max f32 [B] = each clip's maximum
 * of it.  whisper.audio's last two lines -- max(x, x.max() - 8), (x + 4) / 4 -- are then applied by the consumer while it reads the
 * tensor anyway (oasr_train_step's mel_clip_max): half the HBM traffic of this front end, bit-identical encoder input. */
int oasr_log_mel_raw(const void* pcm, int pcm_dtype, int B, int n_samples, float* mel_raw, float* clip_max, void* workspace, void* stream);
/* HOST helper: the slaney 80 x 201 filterbank (whisper assets/mel_filters.npz) into a host buffer. */
int oasr_mel_filterbank(float* out_host);

/* ---- model context: olmoasr.model.OLMoASR(dims) (olmoasr/model.py:778-813) -------------------------------------------- */
oasr_ctx* oasr_create(const oasr_dims* dims); /* training model: n_vocab + 1 embedding rows (pad row, model.py:665-667) */
/* embed_rows = n_vocab selects olmoasr.inf_model.OLMoASR's layout (inf_model.py:302; scripts/eval/gen_inf_ckpt.py) */
oasr_ctx* oasr_create_ex(const oasr_dims* dims, int embed_rows);
/* compute_dtype selects the arithmetic of the whole context -- the reference's --precision flag
 * (scripts/training/train_timestamps.py:2128: "bfloat16" | "float32"; autocast + dtype policy :1414, :2220-2224):
 *   OASR_DTYPE_BF16  production: bf16 MFMA operands / activations, fp32 accumulation and master weights (= autocast(bfloat16))
 *   OASR_DTYPE_F32   validation: the same engine schedule on plain fp32 kernels (fp32 activations, operands, softmax,
 *                    residual stream; exact-erf GELU).  Every `void*` activation the ABI exchanges (xa, kv_cache) then holds
 *                    fp32 instead of bf16.  This is the mode the "logits within 1e-3" criterion is tested in. */
#define OASR_DTYPE_BF16 0
#define OASR_DTYPE_F32 1
oasr_ctx* oasr_create_ex2(const oasr_dims* dims, int embed_rows, int compute_dtype);
int oasr_compute_dtype(const oasr_ctx*);
/* ABI 213: LoRA adapters in weight space (peft's LoraConfig(r, lora_alpha, target_modules) on a frozen base).
 * targets: n_targets tensor indices (oasr_param_info order of the context WITHOUT adapters) of block Linear weights -- attn / cross_attn
 * query, key, value, out and mlp.0 / mlp.2 of any block; rank 1..OASR_LORA_MAX_RANK; scale = lora_alpha / rank.  Target j with weight
 * W0 [out, in] gains two tensors, "<module>.lora_A" [rank, in] and "<module>.lora_B" [out, rank], and computes with the effective weight
 *     W = W0 + scale * lora_B . lora_A
 * (= torch.nn.utils.parametrize / minLoRA).  The adapters sit in the parameter table in target order, between the conv stem and the token
 * embedding, and form the LAST gradient segment.  Every compute copy of an adapted tensor (the bf16 shadow slot; fp32 mode: a full fp32
 * copy of the arena that only adapter contexts have) holds W, re-derived by oasr_refresh_shadow and at the end of oasr_optim_step, so the
 * forward, the decode engines and the data gradients are unchanged.  The backward writes dL/dW of an adapted tensor into workspace scratch
 * (never into W0's gradient range) and projects it: d lora_B = scale * dW . lora_A^T, d lora_A = scale * lora_B^T . dW, accumulated into the
 * gradient arena before the last segment's event.  An adapted base weight can never be trainable (oasr_set_trainable refuses it), and an
 * adapter context has no default mask: the backward entries and oasr_optim_step return OASR_ESTATE until oasr_set_trainable has been
 * called.  ZeRO-1's range entries refuse adapter contexts.
 * n_targets == 0 gives exactly oasr_create_ex2's context. */
#define OASR_LORA_MAX_RANK 64
oasr_ctx* oasr_create_ex3(const oasr_dims* dims, int embed_rows, int compute_dtype, const int32_t* targets, int n_targets, int rank, float scale);
int oasr_lora_count(const oasr_ctx*); /* adapted tensors */
/* Fold the adapters into the master weights: W0 <- W0 + scale * lora_B . lora_A (the fp32 expression the compute copy is rounded from: a
 * model built from the merged masters has a bit-identical compute copy).  The adapters themselves are left as they are; the caller drops
 * them (a context without adapters over the merged base weights). */
int oasr_lora_merge(oasr_ctx*, void* stream);
void oasr_destroy(oasr_ctx*);

/* Parameter table: one flat fp32 arena in gradient-ready (reverse-backward) order; the Python modules expose
 * nn.Parameter views of it under the reference's state_dict names. */
int oasr_param_count(const oasr_ctx*);
int oasr_param_info(const oasr_ctx*, int idx, char* name, int name_cap, int64_t* offset, int64_t* numel, int* ndim,
                    int64_t shape[4]);
int64_t oasr_param_numel(const oasr_ctx*);
/* Gradient segments (arena ranges that become final together during backward), in the order they complete. */
int oasr_segment_count(const oasr_ctx*);
int oasr_segment_info(const oasr_ctx*, int idx, int64_t* offset, int64_t* numel);

/* Bind the flat arenas (params/grads/exp_avg/exp_avg_sq: fp32 [numel]) and the encoder's sinusoid buffer
 * (encoder.positional_embedding, fp32 [n_audio_ctx, d], olmoasr/model.py:199-230,565). */
int oasr_bind(oasr_ctx*, float* params, float* grads, float* exp_avg, float* exp_avg_sq, const float* enc_pos);
/* bf16 compute copies of the weights (+ packed conv kernels, fused qkv biases). */
size_t oasr_shadow_bytes(const oasr_ctx*);
int oasr_bind_shadow(oasr_ctx*, void* shadow);
int oasr_refresh_shadow(oasr_ctx*, void* stream); /* after params changed outside oasr_optim_step */

#define OASR_MODE_INFER 0
#define OASR_MODE_TRAIN 1
#define OASR_MODE_TRAIN_ENC 2 /* ABI 214: the workspace of the staged encoder entries (oasr_train_encode / _encode_bwd; S is not used) */
#define OASR_MODE_TRAIN_DEC 3 /* ABI 214: the workspace of the staged decoder entries (oasr_train_decode / _decode_bwd, and of oasr_train_step from a given xa) */
size_t oasr_workspace_bytes(const oasr_ctx*, int B, int S, int mode); /* 0 for an unknown mode */

/* OLMoASR.forward(mel, tokens, padding_mask) (olmoasr/model.py:856-887).  mel f32 [B,80,2*n_audio_ctx]; tokens i64 [B,S];
 * text_len i32 [B] = first padded key column of the reference's column-only padding mask (train_timestamps.py:314-315),
 * NULL = no padding mask (causal only).  logits_out f32 [B,S,n_vocab+1] (or NULL); xa_out bf16 [B,n_audio_ctx,d] (or NULL). */
int oasr_forward(oasr_ctx*, const float* mel, const int64_t* tokens, const int32_t* text_len, int B, int S, float* logits_out,
                 void* xa_out, void* workspace, size_t workspace_bytes, void* stream);

/* OLMoASR.embed_audio(mel) (model.py:815): xa_out bf16 [B, n_audio_ctx, d]. */
int oasr_encode(oasr_ctx*, const float* mel, int B, void* xa_out, void* workspace, size_t workspace_bytes, void* stream);
/* OLMoASR.logits(tokens, audio_features) (model.py:818-854): decoder on given xa.  last_only != 0 -> logits_out f32
 * [B, rows] of position S-1 only (the greedy step of whisper.decoding / notebooks/ow_decoding.py:50-72). */
int oasr_decode_logits(oasr_ctx*, const int64_t* tokens, const void* xa, const int32_t* text_len, int B, int S, int last_only,
                       float* logits_out, void* workspace, size_t workspace_bytes, void* stream);

/* Cached greedy decoding = the reference's install_kv_cache_hooks (model.py:925-964 / inf_model.py:422-453) + one
 * TextDecoder step per token.  kv_cache: oasr_kv_cache_bytes(B) bytes, caller owned, valid for one 30 s window batch.
 * decode_begin computes the cross-attention K/V of every layer from xa (bf16 [B, n_audio_ctx, d]); decode_step consumes
 * the token at position `pos` of each sequence (tokens_last i64 [B]) and returns f32 logits [B, rows] for position pos+1.
 * Engines (one arithmetic, csrc/decode_shared.h): ONE sequence on the bf16 engine -> one persistent launch for the whole decoder stack
 * on every CU of the device (csrc/decode_wide.hip: a few weight rows per workgroup, rows exchanged through per-workgroup phase flags;
 * agrees with the other engines to the fp32 rounding of a differently ordered K sum); where that engine does not apply, the one-XCD team
 * of csrc/decode_xcd.hip; 2-4 sequences -> LayerNorm folded into the projections' operand loads; more -> separate kernels (these three
 * are bit-identical).  The one-launch engines keep their control words and phase flags in the cache's last OASR_KV_TAIL_BYTES bytes
 * (zeroed by decode_begin; the cache is oasr_kv_cache_bytes(B) bytes INCLUDING that tail -- ABI 211; a caller that re-packs a cache,
 * e.g. the beam re-gather of whisper's rearrange_kv_cache, zeroes the tail of the new buffer).  A one-launch engine needs all of its
 * workgroups resident at once, i.e. the device to itself: a workgroup that never arrives (a second decoder on the device, a CU mask)
 * poisons a flag instead of hanging; oasr_decode_check then clears it, switches the CONTEXT to the multi-launch engine for good and
 * returns OASR_ERETRY: the caller decodes the window again. */
#define OASR_KV_TAIL_BYTES 327680
size_t oasr_kv_cache_bytes(const oasr_ctx*, int B);
size_t oasr_decode_step_workspace_bytes(const oasr_ctx*, int B);
int oasr_decode_begin(oasr_ctx*, const void* xa, int B, void* kv_cache, void* stream);
int oasr_decode_step(oasr_ctx*, const int64_t* tokens_last, int B, int pos, void* kv_cache, float* logits_out, void* workspace,
                     size_t workspace_bytes, void* stream);
/* Synchronises the stream and checks the one-launch engine's error flag: call once per decoded window, where the caller reads the
 * tokens back.  OASR_OK, or OASR_ERETRY (see above: enqueue the window's begin / steps again; at most once per context). */
int oasr_decode_check(oasr_ctx*, int B, void* kv_cache, void* stream);

/* ABI 216: one micro-step of train() (train_timestamps.py:1440-1454): forward, CE(ignore_index=pad)/accum, backward -- ONE entry for every
 * form of the fused step; the options are fields of oasr_train_step_args, NULL / 0 where not used, and a binding checks
 * oasr_sizeof_train_step_args like oasr_sizeof_attn_args.  Gradients of the loss scaled by loss_scale are ACCUMULATED into the bound grad
 * arena (zero it with oasr_zero_grad at the start of an accumulation window).  Every combination the fields' comments exclude is refused
 * (OASR_EINVAL; OASR_ESTATE for the context's state) before anything is launched or dereferenced.
 * Streams: asynchronous on `stream` like everything else.  With span_host, part of the decoder's backward (weight-gradient GEMMs) runs on two
 * lowest-priority streams the context owns (created on the first call, destroyed by oasr_destroy), forked from and joined back into `stream`
 * with events inside the call: when the call returns, everything it enqueued is ordered before whatever the caller enqueues on `stream`
 * next, and each seg_events[i] still means "every gradient of segment i is complete". */
#define OASR_SPAN_FORWARD_ALL 0    /* the reference's shape: the decoder's forward covers all n_text_ctx positions */
#define OASR_SPAN_FORWARD_ACTIVE 1 /* opt-in: the forward leaves the positions past the span out too -- their logits exist in the reference
                                    * (model.py:768-770 over the padded context) but nothing reads them: loss and gradients unchanged */
typedef struct oasr_train_step_args {
  /* Exactly one of mel and xa. */
  const float* mel; /* f32 [B, n_mels, 2*n_audio_ctx]: the whole step.  Workspace: OASR_MODE_TRAIN bytes. */
  /* compute dtype [B, n_audio_ctx, d]: the decoder alone, from a given encoder output -- a frozen encoder's features computed once and
   * reused.  Loss, events and gradients as from mel; every segment event is recorded, the encoder's at once.  OASR_ESTATE if an encoder
   * tensor (or an encoder adapter) is trainable.  Not with mel_clip_max or logits_out.  Workspace: OASR_MODE_TRAIN_DEC bytes. */
  const void* xa;
  const int64_t* tokens;   /* [B, S] */
  const int64_t* targets;  /* [B, S] */
  const int32_t* text_len; /* [B] */
  /* NULL: the plain step.  Or HOST int32 [B] (the data loader builds the token sequences on the host, train_timestamps.py:238-343): the
   * same micro-step with the decoder's BACKWARD limited to the supervised span -- exact, and the forward still covers all n_text_ctx
   * positions like the reference's (train_timestamps.py:318-329 pads every sample to 448; :1444 then ignores the padding).  Every target of
   * sample b at a position >= span_host[b] is ignore_index, and span_host[b] >= text_len[b].  Gradient rows past the span are exactly zero
   * in the reference's computation, so the decoder's token rows are stored in 64-position chunks with the chunks that can carry gradient
   * first and the decoder's backward GEMMs / LayerNorms / attention run over those rows only (olmoasr_amd/csrc/engine_step.hip).  Loss and
   * gradients equal the plain step's up to fp32 summation order.  Needs S = n_text_ctx and span_forward = OASR_SPAN_FORWARD_*; not with
   * logits_out.  Falls back to the plain step when n_text_ctx is not a multiple of 64 or B > 512. */
  const int32_t* span_host;
  /* NULL (mel is finished log-mel, as everywhere else), or device f32 [B] with mel = oasr_log_mel_raw's output.  With span_host and mel only. */
  const float* mel_clip_max;
  float* loss_out;   /* device f32: unscaled loss/accum, overwritten or (accumulate_loss != 0) accumulated */
  float* logits_out; /* NULL, or f32 [B, S, n_vocab+1] (parity mode; costs an extra pass).  Plain step from mel only. */
  /* The teacher-forced predictions on request (the reference's gen_pred argmax, train_timestamps.py:1077, without leaving the span step and
   * without an fp32 logits tensor).  NULL (then the step is the one without them, launch for launch), or device int32 [B, n_text_ctx]:
   *     pred_out[b, s] = argmax over c < n_vocab + 1 of logits[b, s, c]   for s < span_host[b] rounded up to 64 -- the rows every forward
   *                      mode computes; the lowest index wins among equal maxima, the padded columns of the tied head are never candidates
   *     pred_out[b, s] = -1                                               elsewhere
   * One extra kernel between the decoder forward and the cross-entropy (which overwrites the logits with their gradient): each active row is
   * read once in the compute dtype, 4 bytes are written; it addresses rows through the chunk-row table, so the output is in logical order.
   * Loss and gradients are unchanged.  With span_host only, and a shape the row table cannot chunk (n_text_ctx not a multiple of 64, or
   * B > 512) is then refused (OASR_EINVAL) before any launch instead of taking the plain step. */
  int32_t* pred_out;
  void** seg_events; /* NULL or oasr_segment_count() hipEvent_t handles; event i is recorded when segment i's gradient is final */
  int32_t B;
  /* decoder positions, 0 < S <= n_text_ctx.  For S >= max(text_len) the loss and all gradients equal the full-context ones (the trimmed
   * positions are pure padding: ignore_index targets, never attended to by a real query) -- an opt-in the reference does not have. */
  int32_t S;
  int32_t span_forward; /* OASR_SPAN_FORWARD_*; read with span_host only */
  int32_t accumulate_loss;
  float loss_scale, inv_accum; /* inv_accum = 1 / accumulation steps */
  /* Regularisers of the objective (added at the end without a new OASR_ABI_VERSION, like oasr_attn_args' compact-grid fields: a binding
   * compares oasr_sizeof_train_step_args before the first call).  All zero / NULL: exactly the step without them, launch for launch.  For a
   * valid row (target t in [0, V), t != ignore_index) with logits x over the V = n_vocab + 1 classes, lse = logsumexp(x), p = softmax(x):
   *     row_loss  = lse - (1 - eps) * x_t - (eps / V) * sum_{c < V} x_c + z * lse^2
   *     dlogits_c = g * [(1 + 2 * z * lse) * p_c - (1 - eps) * [c == t] - eps / V]        g = loss_scale * inv_accum / n_valid
   * = F.cross_entropy(ignore_index, label_smoothing = eps) + z * mean_valid(lse^2) (the PaLM / OLMo z-loss); ignored rows and the padded
   * columns of the tied head keep zero loss and exactly zero gradient; loss_out = mean_valid(row_loss) * inv_accum, the objective that is
   * differentiated.  One more workgroup reduction (sum x) inside the cross-entropy kernel, no extra pass over the logits.  Every form of the
   * step (plain, span_host in both forward modes, xa, logits_out, pred_out) and both compute dtypes take them.
   * label_smoothing in [0, 1), z_loss >= 0, both finite; else OASR_EINVAL. */
  float label_smoothing; /* eps */
  float z_loss;          /* z */
  /* The objective's parts on request: NULL, or device f32 [2] = { mean_valid(lse - x_t), mean_valid(lse^2) } * inv_accum, overwritten /
   * accumulated like loss_out (so loss_out = (1 - eps) * parts[0] + z * parts[1] + eps * mean_valid(lse - mean_c x) * inv_accum). */
  float* loss_parts_out;
  /* With loss_parts_out (OASR_EINVAL without): device f32 [2, B * S] per-row scratch the caller owns (the workspace plans do not grow). */
  float* loss_parts_rows;
} oasr_train_step_args;
size_t oasr_sizeof_train_step_args(void);
int oasr_train_step(oasr_ctx*, const oasr_train_step_args*, void* workspace, size_t workspace_bytes, void* stream);

/* The same micro-step cut at the logits, for torch.autograd: OLMoASR.forward in training mode (olmoasr/model.py:856-887) followed by
 * the CALLER's loss and .backward() (train_timestamps.py:1440-1454 unchanged).  train_fwd: fp32 logits [B, S, rows], every saved
 * activation stays in the workspace.  train_bwd: dlogits = d(loss)/d(logits), fp32, same shape -> parameter gradients ACCUMULATED into
 * the bound arena (seg_events as above).  Same B, S, tokens, text_len for the pair; the workspace must not be reused in between. */
int oasr_train_fwd(oasr_ctx*, const float* mel, const int64_t* tokens, const int32_t* text_len, int B, int S, float* logits_out,
                   void* workspace, size_t workspace_bytes, void* stream);
int oasr_train_bwd(oasr_ctx*, const int64_t* tokens, const int32_t* text_len, const float* dlogits, int B, int S, void** seg_events,
                   void* workspace, size_t workspace_bytes, void* stream);
int oasr_zero_grad(oasr_ctx*, void* stream);

/* ABI 214: the same training step in two stages, for torch.autograd through model.encoder(mel) and model.decoder(tokens, xa) (the reference's
 * AudioEncoder / TextDecoder as ordinary modules).  Each stage has a workspace of its own (OASR_MODE_TRAIN_ENC / _DEC bytes) that holds one
 * forward's saved activations until that stage's backward: the pair shares B (and S, tokens, text_len), and nothing else may use that
 * workspace in between.  The forwards are the fused training forward's (oasr_train_fwd: training-mode GELU epilogue), cut at xa, so
 * encode -> decode gives bit-identical logits to it.  The backwards are the two halves of its backward: parameter gradients are ACCUMULATED
 * into the bound arena under the trainability mask (a stage's backward writes its own stage's tensors and, with adapters, projects its own
 * stage's adapters only).  An input gradient that is asked for is computed even through frozen blocks, and then an all-zero mask is accepted
 * (saliency on a frozen model); otherwise a mask with no trainable tensor is refused (OASR_ESTATE).
 *   train_encode:     mel f32 [B, n_mels, 2*n_audio_ctx] -> xa_out [B, n_audio_ctx, d] in the compute dtype.
 *   train_encode_bwd: dxa (compute dtype, as xa) -> encoder gradients; dmel_out: NULL, or f32 [B, n_mels, 2*n_audio_ctx] = d(loss)/d(mel)
 *                     (the bf16 engine's cast of mel counts as the identity, as autocast's does).
 *   train_decode:     tokens i64 [B, S], xa (compute dtype, copied into the workspace), text_len i32 [B] -> logits_out f32 [B, S, rows].
 *   train_decode_bwd: dlogits f32 [B, S, rows] -> decoder gradients; dxa_out: NULL, or d(loss)/d(xa) [B, n_audio_ctx, d] in the compute
 *                     dtype, summed over the decoder layers from the top one down. */
int oasr_train_encode(oasr_ctx*, const float* mel, int B, void* xa_out, void* workspace, size_t workspace_bytes, void* stream);
int oasr_train_encode_bwd(oasr_ctx*, const void* dxa, int B, float* dmel_out, void* workspace, size_t workspace_bytes, void* stream);
int oasr_train_decode(oasr_ctx*, const int64_t* tokens, const void* xa, const int32_t* text_len, int B, int S, float* logits_out,
                      void* workspace, size_t workspace_bytes, void* stream);
int oasr_train_decode_bwd(oasr_ctx*, const int64_t* tokens, const int32_t* text_len, const float* dlogits, int B, int S, void* dxa_out,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Frozen parameters (torch's requires_grad == False): mask holds one byte per tensor in oasr_param_info order, nonzero = trainable;
 * the default is all ones.  From then on the backward entries (oasr_train_step, oasr_train_bwd) neither launch nor
 * write anything whose only purpose is a frozen tensor's gradient: frozen ranges of the gradient arena are left as they are.
 * oasr_optim_step updates, decays and clips over the trainable tensors only (frozen moments stay as they are).  With no trainable
 * tensor the backward entries return OASR_ESTATE.  The call is synchronous (it uploads the optimizer's table of trainable runs).
 * ABI 213: a mask that makes an adapted base weight trainable is refused (OASR_EINVAL, oasr_create_ex3). */
int oasr_set_trainable(oasr_ctx*, const uint8_t* mask, int n_params);

/* scaler.unscale_ + clip_grad_norm_(max_norm) + AdamW.step + bf16 shadow refresh (train_timestamps.py:1509-1512).
 * step is 1-based.  stats_out (device f32[2]): [0] = sum of squares of the SCALED grads, [1] = non-finite flag
 * (step skipped when nonzero, like GradScaler).  scratch: >= 8192 bytes device.
 * Overflow of the norm: the squares are formed in fp32 (their sum in double), so a FINITE scaled gradient above sqrt(FLT_MAX) = 1.8e19 makes
 * stats[0] +inf without raising the non-finite flag.  The clip coefficient is then max_norm / inf = 0: the step runs with every gradient taken
 * as zero -- moments decay, weight decay and the momentum term still apply -- where torch would run a clipped step.  Loss scaling keeps
 * healthy gradients twelve orders of magnitude below that; a caller that can see such values should treat stats[0] == inf as found_inf.
 * The range and run-table forms (oasr_grad_sumsq_range, frozen tensors) behave the same.  Pinned by tests/test_gpu_optimizer_planted.py. */
int oasr_optim_step(oasr_ctx*, float inv_loss_scale, float max_grad_norm, float lr, float beta1, float beta2, float eps,
                    float weight_decay, int64_t step, float* stats_out, void* scratch, void* stream);

/* ZeRO-1 (optimizer-state sharding; the reference's sharded variant is FSDP, scripts/training/train_fsdp_timestamps.py:2665-2719):
 * the same fused step over a contiguous range [off, off+numel) of the arenas (multiples of 4).  sumsq_range: stats_out[0] = sum of
 * squares of the scaled gradients in the range, [1] = non-finite flag.  step_range: `stats` = those two numbers summed over ALL
 * ranges (all-reduce them), exp_avg / exp_avg_sq are shard-local buffers of numel floats.  After every rank has stepped its range
 * and the parameters are all-gathered, call oasr_refresh_shadow.  Host side: olmoasr_amd/zero.py. */
int oasr_grad_sumsq_range(oasr_ctx*, int64_t off, int64_t numel, float* stats_out, void* scratch, void* stream);
int oasr_optim_step_range(oasr_ctx*, int64_t off, int64_t numel, float* exp_avg_shard, float* exp_avg_sq_shard, const float* stats,
                          float inv_loss_scale, float max_grad_norm, float lr, float beta1, float beta2, float eps, float weight_decay,
                          int64_t step, void* stream);

/* ---- unit operators (exposed for op-level parity tests; the engine calls the same launchers) ---------------------- */
typedef struct oasr_operand { /* bf16 matrix, optionally a conv-window view: see olmoasr_amd/csrc/kernels.h */
  const void* ptr; int64_t ld; int rpb; int64_t bstride; int lead; int kvalid; int trail_from;
} oasr_operand;
typedef struct oasr_gemm_args {
  oasr_operand A, B; int M, N, K; int ta, tb; float alpha;
  const float* bias; int act; const float* pos; int pos_period;
  const void* dgelu_u; int64_t ldu; const void* resid; int64_t ldr;
  void* out; void* out_pre; int64_t ldc; float* out_f32; int64_t ldc32; float beta; float* colsum; int atomic; int split_k;
  int dgelu_deriv; /* dgelu_u holds GELU'(u) itself (written by an act == 2 forward: out_pre = GELU'(pre)) */
} oasr_gemm_args;
int oasr_gemm(const oasr_gemm_args*, void* stream);
int oasr_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int64_t rows, int d, void* stream);
int oasr_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, const void* dres,
                       void* dx, float* dgamma, float* dbeta, int64_t rows, int d, void* stream);
typedef struct oasr_attn_args {
  const void *q, *k, *v; int64_t ldq, ldk, ldv, bsq, bsk, bsv; void* o; int64_t ldo, bso; float* lse; void* o_lo; const int32_t* kv_len;
  int B, H, Tq, Tk, causal; const void* d_o; float* delta; void *dq, *dk, *dv;
  float *dq_colsum, *dv_colsum; /* optional [H*64], accumulated: column sums of dq / dv = query / value bias gradients */
  float* colsum_scratch;        /* with either of them: B * (ceil(Tq/128) + ceil(Tk/128)) * H*64 floats of scratch */
  int32_t* qtile_flags;         /* optional [B, H, ceil(Tq/64)] workspace (backward): 64-query tiles of d_o that are all zero -- the padded
                                 * positions of a decoder batch -- are recorded by the dQ kernel and skipped by both; bit-identical */
  /* ABI 200: chunked token rows (the decoder of oasr_train_step with span_host).  q_rows / k_rows: optional int32 [B][OASR_ROWTAB]: first
   * token row -- relative to the base pointers, batch strides unused -- of every 64-position chunk of sample b (q_rows: q, o, o_lo,
   * d_o, dq; k_rows: k, v, dk, dv); q_span: optional int32 [B], multiples of 64 (backward): d_o is zero at query positions >=
   * q_span[b]; those rows are not read and their dq (self-attention: dk / dv too) not written. */
  const int32_t *q_rows, *k_rows, *q_span;
  /* Compact grids over the span (added at the end without a new OASR_ABI_VERSION: a binding compares oasr_sizeof_attn_args with its own
   * struct before the first call, which refuses a library built without these fields).  qblk128 / qblk256: optional int32 [n128 * H] / [n256 * H] tables of the 128- / 256-query blocks
   * that start inside their sample's span (n128 = sum_b ceil(q_span[b] / 128), n256 likewise), in (sample, head, block) order, entry =
   * sample << 16 | head << 4 | block -- as oasr_train_step builds them from span_host (tests: oasr_test_span_block_tables).  A launch
   * that carries q_rows and q_span then starts n * H workgroups instead of one per block of the padded context; both tables come
   * together; null = the full grid.  Results are bit-identical.  n128 == 0: nothing is launched. */
  const int32_t *qblk128, *qblk256;
  int n128, n256;
} oasr_attn_args;
#define OASR_ROWTAB 16
/* sizeof(oasr_attn_args) as the library was built: a binding compares it with its own before the first call */
size_t oasr_sizeof_attn_args(void);
int oasr_attention_fwd(const oasr_attn_args*, void* stream);
int oasr_attention_bwd(const oasr_attn_args*, void* stream);
/* The score matrix on request = `qk` of MultiHeadAttention.qkv_attention (olmoasr/model.py:347-442, returned by forward :327,:345 on the
 * manual path; inf_model.py:172-196): scores f32 [B, H, Tq, Tk] = (q * 64^-1/4) . (k * 64^-1/4), pre-softmax, with -inf where the
 * reference's additive mask puts it (causal: j > i; key padding: j >= kv_len[b]).  Reads q, k, their strides, kv_len, B, H, Tq, Tk, causal
 * of the argument block; dtype = OASR_DTYPE_BF16 / OASR_DTYPE_F32 of the operands.  The training and decoding kernels never form this
 * matrix; word-level timestamp alignment (whisper.timing.find_alignment, called from olmoasr/transcribe.py:410-419) reads it from the
 * cross-attention of the upper decoder layers. */
int oasr_attention_scores(const oasr_attn_args*, int dtype, float* scores, void* stream);
/* Word-timestamp alignment on the device (olmoasr_amd/timing.py::find_alignment = whisper.timing.find_alignment, the part after the
 * decoder passes; csrc/align.hip).  Both operators add entry points only: OASR_ABI_VERSION is unchanged, and a binding checks
 * oasr_sizeof_align_args like oasr_sizeof_attn_args.
 *
 * oasr_alignment_matrix: the per-layer score tensors qk[l] = f32 [H, n_tok, Tk], exactly as oasr_attention_scores wrote them (B = 1), are read
 * IN PLACE -- head h of layer l takes part when bit h of head_mask[l] is set; no stacked copy is made, and unselected heads and frames
 * >= n_frames are never read.  out f32 [n_tok, n_frames] (row stride ldo):
 *     out[i, j] = mean over the selected heads h of  median_w( z_h[i, reflect(j - w/2 .. j + w/2)] )
 *     z_h[i, j] = (p_h[i, j] - mean_i p_h[., j]) / std_i p_h[., j]        (population std over ALL n_tok rows)
 *     p_h[i, .] = softmax over j < n_frames of qk_scale * qk_h[i, j]
 * with w = medfilt_width (odd, 1 .. 15; 7 is whisper's), reflect padding -k -> k, F-1+k -> F-1-k, and NO filter when n_frames <= w / 2
 * (median_filter's own rule).  1 <= n_frames <= Tk, 1 <= n_layers <= OASR_ALIGN_MAX_LAYERS, H <= 32.  fp32 throughout (the column sums in
 * double), heads added in ascending (layer, head) order: deterministic.  A column of zero variance is outside the contract (NaN / inf).
 * workspace: oasr_alignment_workspace_bytes(number of selected heads, n_tok, n_frames) bytes of device memory, contents irrelevant. */
#define OASR_ALIGN_MAX_LAYERS 32
typedef struct oasr_align_args {
  const float* qk[OASR_ALIGN_MAX_LAYERS];
  uint32_t head_mask[OASR_ALIGN_MAX_LAYERS];
  int32_t n_layers, H, n_tok, Tk, n_frames, medfilt_width;
  float qk_scale;
  int32_t reserved;
  float* out;
  int64_t ldo;
} oasr_align_args;
size_t oasr_sizeof_align_args(void);
size_t oasr_alignment_workspace_bytes(int n_selected_heads, int n_tok, int n_frames);
int oasr_alignment_matrix(const oasr_align_args*, void* workspace, size_t workspace_bytes, void* stream);
/* oasr_dtw: the monotonic alignment of rows (tokens) to columns (frames) of cost f32 [N, M] (row stride ld, so a row slice of the matrix
 * above is passed as it is; negate != 0: of -cost), bit-identical to timing.py::dtw / whisper.timing.dtw: fp32 cost table with +inf borders,
 * each cell x + min-choice in ONE fp32 add; diagonal only when strictly cheapest, else down only when strictly cheapest, else right; the
 * path runs from (0, 0) to (N-1, M-1).  1 <= N <= 448 (n_text_ctx), 1 <= M <= 1500 (n_audio_ctx).  text_indices / time_indices: device
 * int32, N + M - 1 entries each, of which the first *path_len (device int32) are written; everything stays on the device.  One workgroup;
 * workspace: oasr_dtw_workspace_bytes(N, M) bytes of device memory, contents irrelevant (0 for N, M outside the range). */
size_t oasr_dtw_workspace_bytes(int N, int M);
int oasr_dtw(const float* cost, int64_t ld, int N, int M, int negate, int32_t* text_indices, int32_t* time_indices, int32_t* path_len,
             void* workspace, size_t workspace_bytes, void* stream);
/* SpecAugment (Park et al. 2019, without time warping) on the FINALIZED log-mel tensor, before the engine sees it (csrc/specaug.hip; the
 * rule itself: csrc/specaug_core.h).  Both entries add entry points only: OASR_ABI_VERSION is unchanged, and a binding checks
 * oasr_sizeof_specaug like oasr_sizeof_align_args.
 *
 * A clip's masks are a pure integer function of (seed, clip stream id, policy, shape), in unsigned 64-bit arithmetic with wrap-around:
 *     mix(z):  z += 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *              return z ^ (z >> 31)
 *     h = mix(mix(seed) ^ clip)                                    clip = first_clip + row index in the batch
 *     for (kind, n, W, L) in ((1, freq_masks, freq_width, n_mels), (2, time_masks, time_width, T)), mask i < n, W = min(W, L):
 *         width = mix(h ^ ((kind << 16) | (i << 1)    )) % (W + 1)
 *         start = mix(h ^ ((kind << 16) | (i << 1) | 1)) % (L - width + 1)
 * and the cells [start, start + width) along that axis, over the whole other axis, are set to `fill`.  Masks may overlap and may have
 * width 0.  time_width is taken as given: a cap relative to the clip length is the caller's (integer) business.
 *
 * oasr_spec_augment: mel f32 [B, n_mels, T], contiguous, in place, one launch on `stream`.  Masked cells are stored to; no other cell is
 * written and mel is never read.  B, n_mels, T >= 1; 0 <= counts <= OASR_SPECAUG_MAX_MASKS; widths >= 0; else OASR_EINVAL.
 * oasr_spec_augment_plan: HOST function (no GPU call, host pointers): the same intervals for ONE clip as (start, width) pairs,
 * freq_iv int32 [freq_masks][2], time_iv int32 [time_masks][2]; both lists must be non-null. */
#define OASR_SPECAUG_MAX_MASKS 8
typedef struct oasr_specaug {
  int32_t freq_masks, freq_width, time_masks, time_width;
  float fill;
} oasr_specaug;
size_t oasr_sizeof_specaug(void);
int oasr_spec_augment(float* mel, int B, int n_mels, int T, const oasr_specaug* policy, uint64_t seed, uint64_t first_clip, void* stream);
int oasr_spec_augment_plan(const oasr_specaug* policy, uint64_t seed, uint64_t clip, int n_mels, int T, int32_t* freq_iv, int32_t* time_iv);
/* Token error counts (csrc/editdist.hip; the rule itself: csrc/editdist_core.h): the batched edit distance between hypothesis and reference
 * token rows with its split into substitutions, deletions, insertions and hits -- what calc_pred_wer (train_timestamps.py:1125) reports at
 * word level.  Both entries add entry points only: OASR_ABI_VERSION is unchanged, and a binding checks oasr_sizeof_edit_args like
 * oasr_sizeof_specaug.
 *
 * hyp int32 [B, Lh] (row stride ld_hyp), ref int32 [B, Lr] (row stride ld_ref), unit column stride; hyp_len / ref_len int32 [B] with
 * 0 <= length <= min(OASR_EDIT_MAX_LEN, row width); tokens past a length are never read.  out int32 [B, 4], contiguous = (S, D, I, H).
 * Cell (i, j) covers hyp prefix i and ref prefix j and carries (S, D, I); its cost is S + D + I.
 *     borders    (0, j) = (0, j, 0)      (i, 0) = (0, 0, i)
 *     interior   cd = cost(i-1, j-1) + (hyp[i-1] != ref[j-1]),   cl = cost(i, j-1) + 1 (deletion: the ref token is missing from hyp),
 *                cu = cost(i-1, j) + 1 (insertion); the minimum wins, on a tie the diagonal, then the deletion, then the insertion; the
 *                cell inherits the chosen predecessor's counts and adds its own step
 * The answer is cell (hyp_len, ref_len) and H = ref_len - S - D.  S + D + I is the Levenshtein distance, which is unique; its split depends
 * on the tie rule, which is this library's own (a backtracing aligner such as jiwer's may split a tie differently).  Known answers:
 *     [] -> [1,2,3]: (0,3,0,0)   [1,2,3] -> []: (0,0,3,0)   [1,9,3] -> [1,2,3]: (1,0,0,2)   [1,3] -> [1,2,3]: (0,1,0,2)
 *     [1,2,2,3] -> [1,2,3]: (0,0,1,3)   [2,1] -> [1,2]: (2,0,0,0)   [1,1,2] -> [1,2]: (0,0,1,2)   [0,1,0,1] -> [1,0,1,0]: (0,1,1,3)
 *
 * oasr_edit_counts: device pointers, one launch on `stream`, one workgroup per pair; nothing but out[b, 0:4] is written.  The lengths live
 * on the device, so the host cannot refuse them: a pair whose length is outside the contract gets out[b] = (-1, -1, -1, -1) and none of its
 * tokens is read.  Everything else (null pointers, B < 1, a row stride below the row width) is OASR_EINVAL before the launch.
 * oasr_edit_counts_host: HOST function (no GPU call, host pointers), the same rule from the same text; a length outside the contract is
 * OASR_EINVAL before anything is written. */
#define OASR_EDIT_MAX_LEN 1023
typedef struct oasr_edit_args {
  const int32_t *hyp, *ref, *hyp_len, *ref_len;
  int32_t* out;
  int64_t ld_hyp, ld_ref;
  int32_t B, Lh, Lr, reserved;
} oasr_edit_args;
size_t oasr_sizeof_edit_args(void);
int oasr_edit_counts(const oasr_edit_args*, void* stream);
int oasr_edit_counts_host(const oasr_edit_args*);
/* Teacher-forced scoring, forward only (csrc/score.hip; the reduce rule itself: csrc/score_core.h): per position the negative log-likelihood
 * of the target and the argmax prediction, per sample their totals -- a held-out loss, a token accuracy, or a model-based quality score of
 * an (audio, transcript) pair, without fp32 logits, without a gradient write and without a host read.  Entry points only: OASR_ABI_VERSION
 * is unchanged, and a binding checks oasr_sizeof_score_args like oasr_sizeof_edit_args.
 *
 * oasr_score_rows: logits [B * S, ld] of `dtype` (OASR_DTYPE_BF16 / OASR_DTYPE_F32), row (b, s) at row b * S + s; V <= ld columns are valid;
 * targets i64 [B, S]; span i32 [B]; row_nll f32 [B, S]; pred i32 [B, S]; all on the device, contiguous.  Row (b, s):
 *     s >= span[b]   row_nll = 0, pred = -1, and the row is NOT READ (it may hold anything)
 *     s <  span[b]   pred = argmax over c < V, the lowest index among equal maxima (columns [V, ld) are never candidates; a row with no
 *                    column above -inf gives 0); for a valid target (0 <= t < V and t != ignore) row_nll = logsumexp(x[:V]) - x_t with
 *                    fp32 statistics, otherwise row_nll = 0 exactly.
 * Each active row is read once when rows are 16-byte aligned (ld a multiple of 8 bf16 / 4 fp32 columns) and V <= 57344; otherwise column by
 * column.  One launch; null pointers, B or S < 1, V < 1 or ld < V: OASR_EINVAL before it.
 *
 * oasr_score_reduce: row (b, s) is COUNTED when s < min(span[b], S) and its target is valid.  Per sample over its counted rows:
 *     nll_sum f32 [B]  row_nll added in ascending s into a double, rounded once      nll_max f32 [B]  the largest row_nll, 0 if none
 *     n_tok   i32 [B]  the number of counted rows                                     n_hit   i32 [B]  those with pred == target
 * One launch, one wave per sample.  oasr_score_reduce_host: HOST function (no GPU call, host pointers), the same rule from the same text;
 * the two agree bit for bit.  Null pointers or B, S, V < 1: OASR_EINVAL before anything is written.
 *
 * oasr_score: the inference forward exactly as oasr_forward runs it (from mel, or the decoder alone from given audio features xa in the
 * compute dtype, as oasr_decode_logits), then the two launches above on the engine's own logits in the compute dtype with V = n_vocab + 1
 * and ignore = 51864.  text_len may be NULL (no padding mask), as for oasr_forward; every other pointer is required, exactly one of mel and
 * xa.  Workspace: OASR_MODE_INFER bytes -- row_nll and pred are the caller's so that plan does not grow.  Reads the compute copies of the
 * weights only: no gradient, no saved activation, no optimizer state is touched, whatever the context is bound to.  Every refusal (null
 * pointers, both or neither of mel and xa, B < 1, S outside (0, n_text_ctx], a workspace that is too small: OASR_EINVAL; an unbound
 * context: OASR_ESTATE) comes before anything is launched or dereferenced. */
typedef struct oasr_score_args {
  const float* mel; /* f32 [B, n_mels, 2*n_audio_ctx] */
  const void* xa;   /* compute dtype [B, n_audio_ctx, n_audio_state]; exactly one of mel and xa */
  const int64_t* tokens;
  const int64_t* targets; /* i64 [B, S] each */
  const int32_t* text_len;
  const int32_t* span; /* i32 [B] each, device */
  float* row_nll;
  int32_t* pred; /* [B, S], caller owned, required */
  float* nll_sum;
  float* nll_max;
  int32_t* n_tok;
  int32_t* n_hit; /* [B] */
  int32_t B, S;
} oasr_score_args;
size_t oasr_sizeof_score_args(void);
int oasr_score(oasr_ctx*, const oasr_score_args*, void* workspace, size_t workspace_bytes, void* stream);
int oasr_score_rows(const void* logits, int dtype, int64_t ld, int V, const int64_t* targets, const int32_t* span, int B, int S, int64_t ignore,
                    float* row_nll, int32_t* pred, void* stream);
int oasr_score_reduce(const float* row_nll, const int32_t* pred, const int64_t* targets, const int32_t* span, int B, int S, int V, int64_t ignore,
                      float* nll_sum, float* nll_max, int32_t* n_tok, int32_t* n_hit, void* stream);
int oasr_score_reduce_host(const float* row_nll, const int32_t* pred, const int64_t* targets, const int32_t* span, int B, int S, int V,
                           int64_t ignore, float* nll_sum, float* nll_max, int32_t* n_tok, int32_t* n_hit);
/* Device-resident beam search (csrc/beam.hip; the rule itself: csrc/beam_core.h): whisper's BeamSearchDecoder.update for every audio window
 * of a batch in one launch, and rearrange_kv_cache as one in-place launch.  Entry points only: OASR_ABI_VERSION is unchanged, and a binding
 * checks oasr_sizeof_beam_args like oasr_sizeof_edit_args.
 *
 * One update.  n = n_audio * beam rows, K = beam + 1 candidates per row, `len` tokens per row so far (the sot sequence included).
 *   top_logprob f32 [n, K], top_token i64 [n, K]: oasr_topk_tokens' output.  tokens_in i64 [n, n_ctx]: the rows of this step; tokens_out i64
 *   [n, n_ctx]: the rows of the next one (another buffer: rows are gathered).  sums f32 [n], in place.  sources i32 [n]: row r of the next
 *   step continues row sources[r] (oasr_decode_reorder's index).  last_token i64 [n]: the token appended to row r (oasr_decode_step's input).
 *   Pool of finished sequences per window: pool_tokens i64 [n_audio, max_candidates, n_ctx], pool_len i32 and pool_score f64 [n_audio,
 *   max_candidates], pool_count i32 [n_audio].  Status: pool_full_len i32 [n_audio] = the `len` of the step that filled the window's pool
 *   (OASR_BEAM_NOT_FULL until then; the caller initialises it, pool_count = 0 and short_step = 0), short_step i32 [n_audio].
 * Per window: candidates in (row, k) order with key (row's prefix, token) and score (double)sum + (double)logprob; equal keys collapse to
 * the first position with the score and origin row of the last; entries are ordered by score descending, position ascending; walking them,
 * an eot entry is newly finished, any other becomes the next row of the window until `beam` rows exist, where the walk ends.  Row m of
 * the window then holds the origin's `len` tokens + the token, sums = (float)score.  Newly finished entries enter the pool in walk order
 * (tokens + eot, the double score) while it holds fewer than max_candidates.  Fewer than `beam` continuations: nothing of the window is
 * written, short_step = 1 and the window is skipped from then on.  Once EVERY window's pool_full_len is below the step's `len` (all pools
 * were full before this step) the step is latched: tokens_in's `len` tokens are copied to tokens_out unchanged, sources are the identity,
 * and sums, last tokens and pools stay as they are -- a caller may therefore poll the status every few steps without changing a result.
 * Nothing past token len of a row, and nothing outside the window's own rows and pool slots, is written.
 * oasr_beam_update: device pointers, one launch on `stream`, one workgroup per window.  oasr_beam_update_host: HOST function (no GPU call,
 * host pointers), the same rule from the same text.  Both refuse (OASR_EINVAL) null pointers, beam outside [1, OASR_BEAM_MAX],
 * max_candidates < 1 and len outside [1, n_ctx).
 *
 * oasr_decode_reorder: row j of the KV cache continues row sources[j] (device i32 [B]) -- per decoder layer the self-attention K | V
 * columns [d, 3d) of positions < pos move, in place; cross-attention K/V, the q slots, later positions and the control tail are not
 * touched.  Every source must lie in its destination's group of `group` rows (1 <= group <= OASR_BEAM_MAX, B % group == 0): a group whose
 * device index breaks that, or is the identity, is left as it is; sources_host (host i32 [B], may be NULL), when given, is the same index
 * readable by the host and is checked first (OASR_EINVAL).  oasr_decode_reorder_host: HOST function, the same gather over a host copy of
 * the self-attention rows (`rows`: L layers, `layer_stride` BYTES apart, each [B, n_ctx, 3d] elements of `elem_size` 2 or 4 bytes); a source
 * outside its group is OASR_EINVAL before anything moves. */
#define OASR_BEAM_MAX 15
#define OASR_BEAM_NOT_FULL 0x7fffffff
typedef struct oasr_beam_args {
  const float* top_logprob;
  const int64_t *top_token, *tokens_in;
  int64_t* tokens_out;
  float* sums;
  int32_t* sources;
  int64_t *last_token, *pool_tokens;
  int32_t* pool_len;
  double* pool_score;
  int32_t *pool_count, *pool_full_len, *short_step;
  int32_t n_audio, beam, max_candidates, n_ctx, len, reserved;
  int64_t eot;
} oasr_beam_args;
size_t oasr_sizeof_beam_args(void);
int oasr_beam_update(const oasr_beam_args*, void* stream);
int oasr_beam_update_host(const oasr_beam_args*);
int oasr_decode_reorder(oasr_ctx*, void* kv_cache, int B, int pos, int group, const int32_t* sources, const int32_t* sources_host, void* stream);
int oasr_decode_reorder_host(void* rows, int64_t layer_stride, int L, int B, int n_ctx, int d, int elem_size, int pos, int group,
                             const int32_t* sources);
/* Speed perturbation (Ko et al. 2015; Kaldi's 0.9 / 1.0 / 1.1) of int16 PCM AHEAD of oasr_log_mel, with the transcript's timestamp tokens
 * moved along (csrc/speed.hip; the rule itself: csrc/speed_core.h).  Entry points only: OASR_ABI_VERSION is unchanged, and a binding checks
 * oasr_sizeof_speed and oasr_sizeof_speed_args like oasr_sizeof_specaug.  The operator is an integer function: int16 in, Q15 integer taps,
 * an exact sum, int16 out; floating point enters only where the HOST builds a ratio's tap table, once.
 *
 * Policy: factor i plays a clip P[i] / Q[i] times FASTER -- output sample n sits at input position n P / Q.  1 <= n_factors <=
 * OASR_SPEED_MAX_FACTORS; 1 <= P, Q <= 32; gcd(P, Q) = 1; Q <= 2 P and P <= 2 Q; else OASR_EINVAL.
 *
 * Choice per clip, with mix() and h = mix(mix(seed) ^ clip), clip = first_clip + row, as at oasr_spec_augment (the SAME h; kind 3 keeps the
 * draw apart from the masks' kinds 1 and 2), n_valid the row's leading non-padding samples and N the row length:
 *     i = mix(h ^ (3 << 16)) % n_factors        (P, Q) = (P[i], Q[i])        n_out = (n_valid * Q) / P   (integer division)
 *     n_out > N (a slow-down would push audio the transcript covers past the end of the row): the identity, P = Q = 1, n_out = n_valid,
 *     reported as factor -1
 * Identity: P == Q is a copy of the whole row, bit for bit; it is not a filter.
 *
 * Table of a ratio P != Q (double precision, on the host):  fc = 0.95 min(1, Q / P),  Wd = 16 / fc,  H = floor(Wd) + 1,  2 H taps per phase;
 *     for phase r < Q, tap j < 2 H:   k = j - H + 1,   u = k - r / Q
 *         c = fc sinc(fc u) (0.5 + 0.5 cos(pi u / Wd))  where |u| < Wd, else 0         sinc(x) = sin(pi x) / (pi x), sinc(0) = 1
 *         T[r][j] = floor(c * 32768 + 0.5)
 *     then the phase's largest tap (the first of equal ones) takes + (32768 - sum_j T[r][j]): every phase sums to exactly 2^15.
 * oasr_speed_table writes T as int32 [Q][2 H] (at most 32 x 68 entries) and H; HOST function; P == Q or a pair outside the policy's bounds
 * is OASR_EINVAL.
 *
 * Sample n < n_out:   m = (n P) / Q,  r = (n P) % Q,   acc = sum_j x[m + j - H + 1] T[r][j]   with x = 0 outside [0, n_valid)
 *                     y[n] = clamp((acc + 16384) >> 15, -32768, 32767)        (arithmetic shift; acc exact: it needs more than 32 bits,
 *                     sum_j |T[r][j]| reaches 73920 at 9 / 10)
 * and y[n] = 0 for n_out <= n < N.
 *
 * Timestamp tokens (optional): a token t in [ts_begin, ts_begin + ts_max], k = t - ts_begin, becomes
 *     ts_begin + min(ts_max, (2 k Q + P) / (2 P))
 * (the nearest timestamp of k Q / P, halves up), every other token stays; the map is monotone and the number of tokens unchanged.
 *
 * oasr_speed_perturb: device pointers, ONE launch on `stream`, never synchronises (the first call that meets a ratio on a device uploads
 * its table, like the log-mel tables).  pcm_in / pcm_out int16 [B, N] with row strides ld_in / ld_out >= N (samples), out of place: the two
 * must not overlap.  n_valid int32 [B].  n_out, factor_out: int32 [B] or NULL.  tokens_a, tokens_b: int64 [B, S] (row strides ld_tokens_a /
 * ld_tokens_b >= S) rewritten in place, or NULL; S >= 1, ts_begin >= 0 and 0 <= ts_max <= 2^24 when either is given.  1 <= B <= 65535,
 * 1 <= N <= 2^26.  The plan is evaluated on the device; lengths live there, so the host cannot refuse them: a row whose n_valid is outside
 * [0, N] is copied unchanged, reports factor -1 and n_out = min(max(n_valid, 0), N), and its tokens are left alone.  Everything else that
 * is wrong is OASR_EINVAL before a launch.
 * oasr_speed_perturb_host: HOST function (no GPU call, host pointers), the same rule from the same text; an n_valid outside [0, N] is
 * OASR_EINVAL before anything is written.
 * oasr_speed_plan: HOST function: the (P, Q), n_out and factor of ONE clip (each output may be NULL); 0 <= n_valid <= N, else OASR_EINVAL. */
#define OASR_SPEED_MAX_FACTORS 8
typedef struct oasr_speed {
  int32_t n_factors;
  int32_t P[OASR_SPEED_MAX_FACTORS], Q[OASR_SPEED_MAX_FACTORS];
} oasr_speed;
typedef struct oasr_speed_args {
  const int16_t* pcm_in;
  int16_t* pcm_out;
  const int32_t* n_valid;
  int32_t *n_out, *factor_out;
  int64_t *tokens_a, *tokens_b;
  int64_t ld_in, ld_out, ld_tokens_a, ld_tokens_b;
  uint64_t seed, first_clip;
  int32_t B, N, S, ts_begin, ts_max;
  oasr_speed policy;
} oasr_speed_args;
size_t oasr_sizeof_speed(void);
size_t oasr_sizeof_speed_args(void);
int oasr_speed_perturb(const oasr_speed_args*, void* stream);
int oasr_speed_perturb_host(const oasr_speed_args*);
int oasr_speed_plan(const oasr_speed* policy, uint64_t seed, uint64_t clip, int n_valid, int N, int* P, int* Q, int* n_out, int* factor);
int oasr_speed_table(int P, int Q, int32_t* out, int* H);
/* Noise mixing: additive background noise from a bank of recordings at a drawn signal-to-noise ratio, on int16 PCM AHEAD of oasr_log_mel
 * and after oasr_speed_perturb (csrc/noise.hip; the rule itself: csrc/noise_core.h).  Entry points only: OASR_ABI_VERSION is unchanged, and
 * a binding checks oasr_sizeof_noise and oasr_sizeof_noise_args like oasr_sizeof_speed.  The operator is an integer function of its
 * operands: unsigned and signed 64-bit integers only, no floating point anywhere (the host included) and no 128-bit type.
 *
 * Operands: pcm_in / pcm_out int16 [B, N], row strides ld_in / ld_out >= N (samples), rows at any even address; the two either do not
 * overlap or are the same buffer with the same stride (in place).  n_valid int32 [B]: each row's leading non-padding samples.  bank int16
 * [M, L], row stride ld_bank >= L, every row fully valid and read cyclically; it must not overlap pcm_out.  1 <= B, M <= 65535,
 * 1 <= N, L <= 2^26.  Reports, each NULL or [B]: row_out int32, snr_out int32, gain_out int64.
 * Policy: prob_q16 in [0, 65536] (the chance of a clip to be drawn, in 1 / 65536), snr_lo_db <= snr_hi_db whole dB inside [-10, 50].
 *
 * Draws per clip, with mix() and h = mix(mix(seed) ^ clip), clip = first_clip + row, as at oasr_spec_augment (the SAME h; kind 4 keeps the
 * draws apart from the masks' kinds 1 and 2 and speed perturbation's 3), t = 4 << 16:
 *     drawn = mix(h ^ t) % 65536 < prob_q16        m = mix(h ^ (t | 1)) % M        o = mix(h ^ (t | 2)) % L
 *     s = snr_lo_db + mix(h ^ (t | 3)) % (snr_hi_db - snr_lo_db + 1)
 * Amplitudes: A[s + 10] = round(10^(-s / 20) * 2^15) for s = -10 .. 50, 61 integer constants (A[0] = 103622, A[10] = 32768, A[60] = 104).
 *
 * Gain of a drawn clip with 1 <= n_valid <= N:   v[n] = bank[m][(o + n) % L],   Ex = sum x[n]^2,  Ev = sum v[n]^2  over n < n_valid (exact,
 * <= 2^56);   sh = max(0, bitlength(Ex | Ev) - 31),  ex = Ex >> sh,  ev = Ev >> sh;   ex == 0 or ev == 0: the clip is not mixed; else
 *     g0 = isqrt((ex << 32) / ev)   (Q16, below 2^31.5)        g = (g0 * A[s + 10] + 2^14) >> 15   (Q16, below 2^34)
 * Sample:   y[n] = clamp(x[n] + ((v[n] * g + 2^15) >> 16), -32768, 32767) for n < n_valid (arithmetic shift),   y[n] = x[n] for n_valid <= n < N.
 * A clip that is not mixed -- not drawn, n_valid outside [1, N], ex == 0 or ev == 0 -- is copied bit for bit (in place: left alone) and
 * reports row_out = -1, snr_out = OASR_NOISE_NONE, gain_out = 0; a mixed clip reports m, s and g.
 *
 * oasr_noise_mix: device pointers, TWO launches on `stream` (exact per-tile energies into `workspace`, then gain and mix), never synchronises,
 * no memset, nothing comes back to the host.  workspace: device memory of at least oasr_noise_workspace_bytes(B, N) bytes, 8-byte aligned,
 * contents irrelevant.  The plan is evaluated on the device; lengths live there, so the host cannot refuse them.  Everything else that is
 * wrong is OASR_EINVAL before a launch.
 * oasr_noise_mix_host: HOST function (no GPU call, host pointers, workspace ignored), the same rule from the same text.
 * oasr_noise_plan: HOST function: (drawn, m, o, s) of ONE clip (each output may be NULL); it needs no audio. */
#define OASR_NOISE_NONE (-128)
typedef struct oasr_noise {
  int32_t prob_q16, snr_lo_db, snr_hi_db;
} oasr_noise;
typedef struct oasr_noise_args {
  const int16_t* pcm_in;
  int16_t* pcm_out;
  const int32_t* n_valid;
  const int16_t* bank;
  int32_t *row_out, *snr_out;
  int64_t* gain_out;
  void* workspace;
  size_t workspace_bytes;
  int64_t ld_in, ld_out, ld_bank;
  uint64_t seed, first_clip;
  int32_t B, N, M, L;
  oasr_noise policy;
  int32_t reserved;
} oasr_noise_args;
size_t oasr_sizeof_noise(void);
size_t oasr_sizeof_noise_args(void);
size_t oasr_noise_workspace_bytes(int B, int N);
int oasr_noise_mix(const oasr_noise_args*, void* stream);
int oasr_noise_mix_host(const oasr_noise_args*);
int oasr_noise_plan(const oasr_noise* policy, uint64_t seed, uint64_t clip, int M, int L, int* drawn, int* row, int* offset, int* snr_db);
/* Reverberation: each drawn clip convolved with a room impulse response from a bank, on int16 PCM AHEAD of oasr_log_mel, after
 * oasr_speed_perturb and before oasr_noise_mix (csrc/reverb.hip; the rule itself: csrc/reverb_core.h).  Entry points only: OASR_ABI_VERSION
 * is unchanged, and a binding checks oasr_sizeof_reverb and oasr_sizeof_reverb_args like oasr_sizeof_noise.  The operator is an integer
 * function of its operands: floating point enters only where the HOST builds the bank (Python: augment.rir_bank), once.
 *
 * Operands: pcm_in / pcm_out int16 [B, N], row strides ld_in / ld_out >= N (samples), rows at any even address; the two must not overlap (an
 * output sample reads up to K input samples around it: in place is not offered).  n_valid int32 [B]: each row's leading non-padding samples.
 * rir int16 [R, K]: Q15 taps, row stride ld_rir >= K; delay int32 [R]: the index of each row's direct-path tap; rir must not overlap
 * pcm_out.  1 <= B, R <= 65535, 1 <= N <= 2^26, 1 <= K <= 8192.  Report: row_out int32 [B], or NULL.
 * Policy: prob_q16 in [0, 65536] (the chance of a clip to be drawn, in 1 / 65536).
 *
 * Draws per clip, with mix() and h = mix(mix(seed) ^ clip), clip = first_clip + row, as at oasr_spec_augment (the SAME h; kind 5 keeps the
 * draws apart from the masks' kinds 1 and 2, speed perturbation's 3 and noise mixing's 4), t = 5 << 16:
 *     drawn = mix(h ^ t) % 65536 < prob_q16        r = mix(h ^ (t | 1)) % R
 * Sample of a drawn clip with 1 <= n_valid <= N:
 *     tap(k) = clamp(rir[r][k], -32639, 32639)     d = clamp(delay[r], 0, K - 1)     x(i) = pcm_in[row][i] for 0 <= i < n_valid, else 0
 *     S[n]   = sum_{k = 0}^{K - 1} tap(k) * x(n + d - k)                             (exact; |S| < 2^44)
 *     y[n]   = clamp((S[n] + 2^14) >> 15, -32768, 32767) for n < n_valid (arithmetic shift),     y[n] = pcm_in[row][n] for n_valid <= n < N
 * The output is shifted back by the direct-path delay and cut at n_valid, so lengths and timestamp tokens do not change.  Both clamps make
 * the rule total over whatever the bank's memory holds (the host cannot inspect it); 32639 = 127 * 256 + 127 is the largest magnitude whose
 * two byte digits both fit a signed byte, which is how the device computes S on the matrix cores.
 * A clip that is not drawn, or whose n_valid is outside [1, N], is copied bit for bit and reports row_out = -1; a reverberated clip reports r.
 *
 * oasr_reverb: device pointers, TWO launches on `stream` (the bank's rows expanded into `workspace` as matrix-core operands, then the
 * convolution), never synchronises, no memset, nothing comes back to the host.  workspace: device memory of at least
 * oasr_reverb_workspace_bytes(R, K) bytes, 16-byte aligned, contents irrelevant.  The plan is evaluated on the device; lengths, taps and
 * delays live there, so the host cannot refuse them.  Everything else that is wrong is OASR_EINVAL before a launch.
 * oasr_reverb_host: HOST function (no GPU call, host pointers, workspace ignored), the same rule from the same text.
 * oasr_reverb_plan: HOST function: (drawn, r) of ONE clip (each output may be NULL); it needs no audio. */
struct oasr_reverb { /* the policy; no typedef: in C and C++ alike the plain name oasr_reverb is the entry point below, the policy is `struct oasr_reverb` */
  int32_t prob_q16;
};
typedef struct oasr_reverb_args {
  const int16_t* pcm_in;
  int16_t* pcm_out;
  const int32_t* n_valid;
  const int16_t* rir;
  const int32_t* delay;
  int32_t* row_out;
  void* workspace;
  size_t workspace_bytes;
  int64_t ld_in, ld_out, ld_rir;
  uint64_t seed, first_clip;
  int32_t B, N, R, K;
  struct oasr_reverb policy;
  int32_t reserved;
} oasr_reverb_args;
size_t oasr_sizeof_reverb(void);
size_t oasr_sizeof_reverb_args(void);
size_t oasr_reverb_workspace_bytes(int R, int K);
int oasr_reverb(const oasr_reverb_args*, void* stream);
int oasr_reverb_host(const oasr_reverb_args*);
int oasr_reverb_plan(const struct oasr_reverb* policy, uint64_t seed, uint64_t clip, int R, int* drawn, int* row);
/* Telephone channel: each drawn clip band-limited to 300 - 3400 Hz at 8 kHz, passed through a drawn G.711 codec and brought back to 16 kHz,
 * on int16 PCM AHEAD of oasr_log_mel and after oasr_noise_mix -- the channel carries the noise too (csrc/telephone.hip; the rule itself:
 * csrc/telephone_core.h).  Entry points only: OASR_ABI_VERSION is unchanged, and a binding checks oasr_sizeof_telephone_args like
 * oasr_sizeof_reverb_args.  The operator is an integer function of its operands: floating point enters only where the HOST builds the two
 * tap tables (oasr_telephone_tables), once.
 *
 * Operands: pcm_in / pcm_out int16 [B, N], row strides ld_in / ld_out >= N (samples), rows at any even address; the two must not overlap (an
 * output sample reads up to 95 input samples on either side: in place is not offered).  n_valid int32 [B]: each row's leading non-padding
 * samples.  1 <= B <= 65535, 1 <= N <= 2^26.  Report: codec_out int32 [B], or NULL.
 * Policy: prob_q16 in [0, 65536] (the chance of a clip to be drawn, in 1 / 65536); n_codecs in [1, 8] entries of codecs, each one of
 * OASR_TELEPHONE_LINEAR (0), _MULAW (1), _ALAW (2) -- repeats act as weights; bandpass 1, or 0 for material that is narrow-band already.
 *
 * Draws per clip, with mix() and h = mix(mix(seed) ^ clip), clip = first_clip + row, as at oasr_spec_augment (the SAME h; kind 6 keeps the
 * draws apart from kinds 1 .. 5 of the masks, speed perturbation, noise mixing and reverberation), t = 6 << 16:
 *     drawn = mix(h ^ t) % 65536 < prob_q16        codec = codecs[mix(h ^ (t | 1)) % n_codecs]
 * Tables, built by the host in double precision, sinc(t) = sin(pi t) / (pi t), sinc(0) = 1:
 *     h[k] = floor(c * 32768 + 0.5),  k = -64 .. 64,   c = (lp(3400)[k] - lp(300)[k]) * (0.5 + 0.5 cos(pi k / 65)),
 *            lp(f)[k] = (2 f / 16000) * sinc(2 f k / 16000)                      (129 taps, symmetric, no sum fix-up; sum |h| = 76960)
 *     u[j] = floor(sinc(t) * (0.5 + 0.5 cos(pi t / 16)) * 32768 + 0.5),  j = 0 .. 31,  t = (j - 15) - 0.5;  then 32768 - sum u is added to
 *            the first largest tap, so that the phase sums to exactly 2^15                                      (sum |u| = 81604)
 * Samples of a drawn clip with 1 <= n_valid <= N:   x(i) = pcm_in[row][i] for 0 <= i < n_valid, else 0;   M = ceil(n_valid / 2);
 *     z[m]     = clamp((sum_{k = -64}^{64} h[k] * x(2 m - k) + 2^14) >> 15, -32768, 32767)  for 0 <= m < M        (exact sum, arithmetic shift)
 *                with bandpass = 0:  z[m] = x(2 m)
 *     c[m]     = q_codec(z[m])  for 0 <= m < M,  0 elsewhere
 *     y[2 m]   = c[m]
 *     y[2 m+1] = clamp((sum_{j = 0}^{31} u[j] * c[m + j - 15] + 2^14) >> 15, -32768, 32767)  where 2 m + 1 < n_valid
 *     y[n]     = pcm_in[row][n]  for n_valid <= n < N
 * Both sums exceed 32 bits (|sum| up to 76960 * 2^15 and 81604 * 2^15): they are exact all the same.  The filters are symmetric about the
 * sample they produce (zero phase), so lengths, n_valid and timestamp tokens do not change.
 * Codecs -- the G.711 quantisers as expand(compress(x)) on the 16-bit value, in closed form, s = x < 0, q = s ? -y : y:
 *     linear   q(x) = x
 *     mu-law   a = min(s ? -x : x, 32635) + 132;   e = floor(log2 a) - 7;   m = (a >> (e + 3)) & 15;   y = (((m << 3) + 132) << e) - 132
 *     A-law    a = s ? -x - 1 : x;   v = a >> 3;   g = v < 32 ? 0 : floor(log2 v) - 4;   m = g < 2 ? (v >> 1) & 15 : (v >> g) & 15;
 *              y = g == 0 ? (m << 4) + 8 : ((m << 4) + 264) << (g - 1)
 *     (mu-law: 255 levels inside +-32124, q(0) = q(-1) = 0, |q(x) - x| <= 644;  A-law: 256 levels inside +-32256, q(0) = 8, q(-1) = -8,
 *     |q(x) - x| <= 512;  both monotone and idempotent)
 * A clip that is not drawn, or whose n_valid is outside [1, N], is copied bit for bit and reports codec_out = -1; any other reports its codec.
 *
 * oasr_telephone: device pointers, ONE launch on `stream`, never synchronises, no workspace, nothing comes back to the host.  The plan is
 * evaluated on the device; lengths live there, so the host cannot refuse them.  Everything else that is wrong is OASR_EINVAL before a launch.
 * oasr_telephone_host: HOST function (no GPU call, host pointers), the same rule from the same text.
 * oasr_telephone_plan: HOST function: (drawn, codec) of ONE clip (each output may be NULL); it needs no audio.
 * oasr_telephone_tables: HOST function: the library's h (as h[k + 64]) and u (each may be NULL).
 * oasr_telephone_quantize_host: HOST function: out[i] = q_codec(in[i]) for i < n (n >= 0; in may be out). */
#define OASR_TELEPHONE_MAX_CODECS 8
#define OASR_TELEPHONE_LINEAR 0
#define OASR_TELEPHONE_MULAW 1
#define OASR_TELEPHONE_ALAW 2
struct oasr_telephone { /* the policy; no typedef, as with `struct oasr_reverb`: the plain name oasr_telephone is the entry point below */
  int32_t prob_q16, n_codecs;
  int32_t codecs[OASR_TELEPHONE_MAX_CODECS];
  int32_t bandpass;
};
typedef struct oasr_telephone_args {
  const int16_t* pcm_in;
  int16_t* pcm_out;
  const int32_t* n_valid;
  int32_t* codec_out;
  int64_t ld_in, ld_out;
  uint64_t seed, first_clip;
  int32_t B, N;
  struct oasr_telephone policy;
  int32_t reserved;
} oasr_telephone_args;
size_t oasr_sizeof_telephone(void);
size_t oasr_sizeof_telephone_args(void);
int oasr_telephone(const oasr_telephone_args*, void* stream);
int oasr_telephone_host(const oasr_telephone_args*);
int oasr_telephone_plan(const struct oasr_telephone* policy, uint64_t seed, uint64_t clip, int* drawn, int* codec);
int oasr_telephone_tables(int32_t h[129], int32_t u[32]);
int oasr_telephone_quantize_host(const int16_t* in, int16_t* out, int64_t n, int codec);
int oasr_cross_entropy(void* logits_bf16, int64_t ld, int V, const int64_t* targets, int64_t rows, int64_t ignore, float gscale,
                       int32_t* n_valid_dev, float* row_loss, float* loss_out, int write_grad, void* stream);
/* The same operator with the regularisers of oasr_train_step_args (label_smoothing, z_loss: the formula there; gscale takes the place of
 * loss_scale * inv_accum) -- an entry point only, OASR_ABI_VERSION is unchanged.  row_loss / loss_out hold the regularised objective.
 * row_parts: NULL, or device f32 [2, rows]: row_parts[0][r] = lse - x_t, row_parts[1][r] = lse^2 (0 for ignored rows).
 * label_smoothing = z_loss = 0 and row_parts = NULL: oasr_cross_entropy itself, which forwards here.  Values outside [0, 1) / below 0 / not
 * finite: OASR_EINVAL. */
int oasr_cross_entropy_ex(void* logits_bf16, int64_t ld, int V, const int64_t* targets, int64_t rows, int64_t ignore, float gscale,
                          int32_t* n_valid_dev, float* row_loss, float* loss_out, int write_grad, float label_smoothing, float z_loss,
                          float* row_parts, void* stream);
int oasr_cast_f32_bf16(const float* src, void* dst, int64_t n, void* stream);
/* The two LoRA kernels as unit operators (the engine calls the same launchers).  merge: out = w0 + scale * B . A (w0 [rows, cols] f32,
 * A [rank, cols], B [rows, rank]; out_dtype OASR_DTYPE_BF16 / OASR_DTYPE_F32; out may be w0 for f32).  grad: dA += scale * B^T . dW,
 * dB += scale * dW . A^T, scratch of oasr_lora_grad_scratch_bytes. */
int oasr_lora_merge_op(const float* w0, const float* A, const float* B, int rows, int cols, int rank, float scale, int out_dtype, void* out,
                       void* stream);
size_t oasr_lora_grad_scratch_bytes(int rows, int cols, int rank);
int oasr_lora_grad_op(const float* dW, const float* A, const float* B, int rows, int cols, int rank, float scale, float* dA, float* dB,
                      void* scratch, void* stream);
/* Per-row token pick over fp32 logits [rows, ld] (first V columns): tok = argmax(logits + mask + mask2) with the lowest index
 * among equal maxima, logprob = log_softmax(logits + masks)[tok] (NULL to skip).  masks: additive f32 [V] (0 / -inf) or NULL.
 * = the tail of whisper.decoding GreedyDecoder.update (argmax + log_softmax gather) after SuppressBlank / SuppressTokens,
 * and gen_pred's argmax over teacher-forced logits (scripts/training/train_timestamps.py:1096-1098). */
int oasr_pick_tokens(const float* logits, int64_t ld, int V, int64_t rows, const float* mask, const float* mask2, int64_t* tok,
                     float* logprob, void* stream);
/* The same pick in TIMESTAMP mode -- the reference's default for transcribe() (olmoasr/transcribe.py:212: DecodingOptions without
 * without_timestamps) -- with whisper.decoding.ApplyTimestampRules evaluated on the device from the sampled history
 * (history i64 [rows, history_ld], n_history tokens sampled so far per row; max_initial_index < 0: no limit on the first timestamp):
 * pairs must be closed, text must follow a pair, timestamps do not decrease, the first token is a timestamp <= max_initial, and a
 * timestamp is forced when the timestamp mass beats every text token.  Replaces ApplyTimestampRules.apply + GreedyDecoder.update. */
int oasr_pick_tokens_ts(const float* logits, int64_t ld, int V, int64_t rows, const float* mask, const float* mask2,
                        const int64_t* history, int64_t history_ld, int n_history, int timestamp_begin, int eot, int no_timestamps,
                        int max_initial_index, int64_t* tok, float* logprob, void* stream);
/* Beam search and sampling on the SAME filtered distribution (suppress masks; with n_history >= 0 also ApplyTimestampRules from the
 * device-resident history, as above; n_history < 0: masks only -- the without_timestamps mode).
 * topk: tok / logprob [rows, K] = the K (<= 16) largest log_softmax values and their tokens, descending, ties to the lower id --
 *       whisper.decoding.BeamSearchDecoder.update's logprobs.topk(beam_size + 1) (the reference's long-form eval is beam 5,
 *       scripts/eval/eval.py:2077-2084).
 * sample: one draw per row from softmax(filtered logits / temperature) by inverse CDF on uniforms[row] in [0, 1) (the caller's
 *       generator), logprob = the draw's log_softmax at temperature 1 -- GreedyDecoder.update at temperature > 0 (the fallback
 *       temperatures of olmoasr/transcribe.py:193-233). */
int oasr_topk_tokens(const float* logits, int64_t ld, int V, int64_t rows, const float* mask, const float* mask2, const int64_t* history,
                     int64_t history_ld, int n_history, int timestamp_begin, int eot, int no_timestamps, int max_initial_index, int K,
                     int64_t* tok, float* logprob, void* stream);
int oasr_sample_tokens(const float* logits, int64_t ld, int V, int64_t rows, const float* mask, const float* mask2, const int64_t* history,
                       int64_t history_ld, int n_history, int timestamp_begin, int eot, int no_timestamps, int max_initial_index,
                       float temperature, const float* uniforms, int64_t* tok, float* logprob, void* stream);
/* Measurement / test hooks (GEMM launch timing for bench.py, kernel-path forcing, hardware probes) are declared in
 * include/oasr_testing.h: they are exported by the same library but are not part of the product surface. */

#ifdef __cplusplus
}
#endif
#endif
