/* liboasr -- measurement and test hooks.  Exported by liboasr.so next to the product ABI of include/oasr.h, but NOT part of
 * the drop-in surface: nothing on the training / decoding path calls them.  Users: bench.py (live GEMM roofline), tests/
 * (kernel-path forcing, hardware-behaviour probes that pin what the kernels rely on), scripts/ (A/B experiments).
 * The setters that change process-wide kernel selection (oasr_gemm_set_variant / _set_stagger / _force_general,
 * oasr_attention_set_pingpong, oasr_attention_set_span_grid, oasr_decode_set_ln_fold, oasr_span_set_side_streams) are INERT unless the process opts in with OASR_TESTING_HOOKS=1 in its
 * environment: without it they return OASR_ESTATE and change nothing, so a production process cannot be steered through them. */
#ifndef OASR_TESTING_H
#define OASR_TESTING_H
#include "oasr.h"
#ifdef __cplusplus
extern "C" {
#endif

/* bench.py's live roofline measurement: when enabled every GEMM launch is bracketed by HIP events on ITS stream;
 * collect() synchronises and returns, per kernel variant (index 2*ta+tb: 0 = NT forward, 1 = NN dgrad, 3 = TN wgrad),
 * summed milliseconds, summed algorithmic flops (2*M*N*K, conv windows at their real width) and launch count; by_symbol
 * receives the same sums keyed by the kernel symbol rocprofv3 prints, so the two can be compared line by line. */
int oasr_profile_gemm(int enable);
/* tests / experiments on the 256x256 ping-pong kernel.  v < 0: defaults.  bits 0-3: K-tile schedule -- 2 = four phases of 8 MFMAs, 7 = two
 * sections of 16 MFMAs, 8 = the per-layout default (7; 2 for the dgrad with fused column sums); any other value returns OASR_EINVAL and changes
 * nothing.  bits 4-5: 1 = plain launches, 2 = persistent launches (next tile's prologue ahead of the epilogue); bit 6 / 7: non-temporal epilogue
 * stores / side loads */
int oasr_gemm_set_variant(int v);
/* tests / A-B: selects the ENGINE of the KV-cached step (the name is historical; csrc/decode_step_core.h: StepMode).  -1 = default (ONE sequence on the bf16 engine: the chip-wide one-launch engine of
 * csrc/decode_wide.hip; 2-4: LayerNorm folded into the projections; more: separate kernels), 0 = separate LayerNorm kernels, 1 = LayerNorm
 * folded into the projections' operand loads for every B <= 32, 2 = the one-launch TEAM engine of csrc/decode_xcd.hip on the 32 CUs of one
 * XCD (B <= 4), 3 / 4 = that team as 32 / 64 workgroups spread over the chip, 5 = the chip-wide engine (one sequence; more: as 2).
 * 0-4 are bit-identical; 5 agrees with them to the fp32 rounding of differently ordered K sums (tests/test_gpu_decode_step.py). */
int oasr_decode_set_ln_fold(int mode);
/* tests / A-B: side streams of the supervised-span step (oasr_train_step with span_host; csrc/engine_side.h: SideMode).  Bit 0: the decoder
 * backward's weight gradients over the R active rows, bit 2: the cross-attention key|value weight gradient and d(xa) -- run on lowest-priority
 * streams beside the data-gradient chain; bit 1: the key|value projections of the decoder forward likewise; bit 3: without segment events leave
 * the key|value gradients in flight across blocks.  -1 = the library default.  Gradients differ by fp32 atomic order only
 * (tests/test_gpu_span.py).  The getter returns the mode in effect. */
int oasr_span_set_side_streams(int mode);
int oasr_span_side_streams(void);
/* tests (CPU): the static block stream of workgroup `wg` of the one-launch step engine as its cursors generate it: out[4 i ..] = layer,
 * segment (0 qkv, 1 attn.out, 2 cross q, 3 cross K/V, 4 cross out, 5 mlp.0, 6 mlp.2), tile / item ordinal, block; returns the count. */
int oasr_xcd_plan_debug(int d, int H, int Te, int M, int L, int team, int wg, int* out, int max_blocks);
/* the chip-wide step engine (csrc/decode_wide.hip): does the shape run on it with `nwg` workgroups and a logits phase over the V rows of the token
 * embedding (unpadded, as the context holds them: n_vocab, + 1 with the training layout's pad row) -- 0: the engine takes the team or the multi-launch
 * step; the (row, 512-element K span) units of compute wave
 * `wave` (1 .. 8) of workgroup `wg` for an [N x K] projection of a width-d model: out[2 i] = row, out[2 i + 1] = span; returns the count (-1: bad arguments or
 * past the kernel's unrolled bound) */
int oasr_wide_supports_debug(int d, int H, int Te, int S_max, int L, int M, int nwg, int V);
int oasr_wide_plan_debug(int d, int nwg, int N, int K, int wg, int wave, int* out, int max_units);
/* tests (CPU): 1 when every 32-bit buffer offset of a one-launch step stays below 2 GiB (layer0 = the 18 element offsets of decoder layer 0
 * in the field order of csrc/decode_step_core.h::DecLayerOffsets, strides in elements), 0 when the engine must take the multi-launch step instead. */
int oasr_xcd_offsets_ok_debug(const int64_t* layer0, long long lstride, long long cache_lstride, int d, int Te, int L, int M);
/* tests / A-B: 1 (default) = the unmasked attention cases (encoder self-, cross-attention) run the 8-wave ping-pong kernels,
 * 0 = the general (maskable) kernels run everything.  Same results up to accumulation order (tests/test_gpu_ops.py). */
int oasr_attention_set_pingpong(int on);
/* tests / A-B: 1 (default) = an attention launch that carries block tables (oasr_attn_args.qblk128 / qblk256; the decoder attentions of
 * oasr_train_step with span_host) starts one workgroup per query block inside the spans, 0 = the full grid over the padded context, whose
 * blocks past the span exit at once.  Bit-identical results (tests/test_gpu_span_grid.py). */
int oasr_attention_set_span_grid(int on);
int oasr_gemm_set_stagger(int sleeps, int phases); /* experiments: first-wave phase stagger of the 256x256 kernel (0 = off) */
int oasr_gemm_force_general(int on); /* tests: route every GEMM through the register-staged general kernel */
/* tests: oasr_gemm with the launch options only the engine sets (csrc/kernels.h GemmArgs): colsum_scratch -- fp32 [2 * ceil(M/256)][N] partial
 * rows for the fused column sums instead of atomics; atomic_on_pp -- split-K / atomic output on the 256x256 ping-pong kernel (M, N % 256 == 0);
 * raster_gm -- tile rows per L2 group (0 = default); stagger, stagger_phases -- first-wave stagger of the ping-pong kernel (0 = the automatic rule). */
int oasr_test_gemm(const oasr_gemm_args* a, float* colsum_scratch, int atomic_on_pp, int raster_gm, int stagger, int stagger_phases, void* stream);
/* tests: which kernels ran.  One text line per GEMM launch since oasr_profile_gemm(1), in launch order (oasr_profile_gemm_collect clears them):
 * "symbol\tM\tN\tK\tta\ttb\tflags\tsplit_k\tatomic\tatomic_on_pp\tscratch\tstagger\tstagger_phases\tpersistent\tlane\n" -- flags: the epilogue flag word
 * of csrc/gemm_common.h (EPI_BIAS = 1, RESID 2, U 4, UDERIV 8, PRE 16, OUT 32, GELU 64, DERIV 128, POS 256, SCALE 512, NT_ST 1024, NT_LD 2048); scratch: a
 * colsum_scratch came with colsum (the fused kernels then write partial rows instead of atomics); stagger: as the launch carried it (automatic rule applied); persistent: ping-pong kernel launched with
 * one workgroup per CU.  Returns the number of records (< 0: `cap` bytes do not hold them).  Does not synchronise. */
int oasr_profile_gemm_records(char* buf, int cap);
/* tests (CPU, tests/test_gemm_route_cpu.py): the kernel choice of oasr_gemm (csrc/gemm.hip: gemm_route) for a call described by plain integers --
 * no device pointer, nothing launched, and the process-wide hooks above are NOT read: the forced path and the schedule override are parameters.
 * The call is taken to pass oasr_gemm's argument checks (N % 4 == 0, K % 8 == 0 for a k-contiguous operand, ...).
 *   M, N, K, ta, tb, split_k, atomic, atomic_on_pp: as in oasr_gemm_args / oasr_test_gemm; a_view, b_view: the operand is a conv-window view;
 *   outputs: bit 0 out, 1 out_pre, 2 out_f32;  sides: bit 0 bias, 1 resid, 2 dgelu_u, 3 pos;  ldc, ldr, ldu: their leading dimensions;
 *   misalign: the low four address bits of out / out_pre / resid / dgelu_u or-ed together (0 = all 16-byte aligned);
 *   colsum, colsum_scratch: given or not;  forced_path: the code of oasr_gemm_force_general (0 = automatic);  pp_schedule: 2, 7 or -1 = the
 *   per-layout default (oasr_gemm_set_variant bits 0-3);  geom_env: the OASR_GEMM_GEOM experiment value (0 = none).
 * symbol (cap bytes) receives the kernel symbol exactly as oasr_profile_gemm_records prints it, *post the step that follows the kernel:
 * 0 = none, 1 = column sums reduced from `out`, 2 = column sums reduced from the colsum_scratch rows. */
int oasr_gemm_route_debug(int M, int N, int K, int ta, int tb, int a_view, int b_view, int split_k, int atomic, int atomic_on_pp, int outputs,
                          int sides, long long ldc, long long ldr, long long ldu, int misalign, int colsum, int colsum_scratch, int forced_path,
                          int pp_schedule, int geom_env, char* symbol, int cap, int* post);
/* tests (CPU, tests/test_train_plan_cpu.py): the host decisions of the training engine (csrc/train_plan.h) on plain integers -- nothing launched.
 * wgrad_plan: how the engine launches the weight gradient dW[N, K] += dy[M, N]^T . x[M, K] over M token rows (view: x is a conv-window view):
 *   *split_k and *atomic_on_pp as oasr_test_gemm takes them.  OASR_EINVAL (nothing written) for a dimension < 1 or a null output.
 * block_needs: which parts of one transformer block's backward run.  asks, bit 0 need_dx_in (the block's input gradient is wanted), 1 need_xa
 *   (d(xa) is wanted), 2 the block has a cross-attention, then "a tensor of the group needs a gradient": 3 self-attention + attn_ln, 4 cross-attention
 *   + cross_attn_ln, 5 mlp.0 + mlp_ln, 6 cross_attn_ln, 7 attn_ln, 8 the cross key | value weights.  Returns, bit 0 the MLP section (everything past
 *   the mlp.2 weight gradient), 1 the cross-attention section, 2 the self-attention section, 3 the cross key|value side (its weight gradient / d(xa)),
 *   4 / 5 the data gradient through cross_attn_ln / attn_ln; -1 for asks outside [0, 512). */
int oasr_train_wgrad_plan_debug(long long M, int N, int K, int view, int* split_k, int* atomic_on_pp);
int oasr_train_block_needs_debug(int asks);
int oasr_profile_gemm_collect(double* ms4, double* flops4, int64_t* count4, char* by_symbol /* "symbol\tlaunches\tms\tflops\n"... or NULL */, int cap);
int oasr_probe_lds_oob(const void* src_u16 /*[512]*/, void* dst_u16 /*[512]*/, void* stream);
int oasr_probe_tr16(const void* src_bf16 /*[16][64]*/, void* dst_bf16 /*[64 lanes][4]*/, void* stream);
/* tests: the tables oasr_train_step builds from span_host for one micro-batch -- span_host: HOST int32 [B]; rows_out: device int32
 * [B][OASR_ROWTAB] chunk-row table; span_out: device int32 [B] spans rounded up to 64; targets_rows_out: device int64 [B*S] targets in
 * row order (active rows only); active_rows_out: HOST int64, the number of leading rows the decoder's backward runs over. */
int oasr_test_span_tables(const int32_t* span_host, int B, int S, const int64_t* targets, int32_t* rows_out, int32_t* span_out,
                          int64_t* targets_rows_out, int64_t* active_rows_out, void* stream);
/* tests: the same launch with the query-block tables of the attention kernels' compact grids for H heads (oasr_attn_args.qblk128 / qblk256):
 * blk128_out / blk256_out: device int32, B * ceil(S / 128) * H and B * ceil(S / 256) * H entries of room; counts_out: HOST int32 [2] =
 * n128, n256 (blocks inside the spans, per head). */
int oasr_test_span_block_tables(const int32_t* span_host, int B, int S, int H, const int64_t* targets, int32_t* rows_out, int32_t* span_out,
                                int64_t* targets_rows_out, int32_t* blk128_out, int32_t* blk256_out, int32_t* counts_out, void* stream);

/* tests (tests/test_gpu_glue_ops.py): the glue launchers of csrc/kernels.h as unit operators -- the kernels between the GEMMs and the attention
 * that the training step reaches only inside a whole-model run.  Contracts: csrc/kernels.h, argument for argument.  dtype = OASR_DTYPE_BF16 (the
 * production kernel) / OASR_DTYPE_F32 (the fp32 validation overload): the type of every `void*` activation; float* arguments are fp32 in both.
 * They change no process state, so they need no OASR_TESTING_HOOKS opt-in.
 *   embedding_fwd  x[row(b, s)] = E[tok[b, s]] + pos[s] (ids outside [0, n_embed): pos[s] alone); rows: optional chunk-row table [B][OASR_ROWTAB]
 *   embedding_bwd  dE[tok] += dx (not for pad_id / ids outside the table), dpos[s] += sum_b dx; dE or dpos may be null; span (with rows):
 *                  positions s >= span[b] are not read
 *   colsum         out[n] += sum_m x[m][n], x [M][ld], columns [0, ncols)
 *   conv2_col2im_dgelu  dpre1[b, t] = gelu'(u1[b, t]) * (the conv2 windows dA [B*T1/2][3][d] folded onto input row t)
 *   conv1_col2im_mel    dmel f32 [B][n_mels][T1] = the conv1 windows dcol [B*T1][256] folded onto the frames
 *   mel_to_time_major   mel f32 [B][n_mels][T] -> [B][T][n_mels]; clip_max (optional [B]): max(x, clip_max[b] - 8), (x + 4) / 4 on the way
 *   pack_conv_weight    w f32 [co][ci][3] -> [co][ldk], k = kk * ci + c, zero padded;  unpack_conv_grad: dw[co][ci][3] += g [co][ldk]
 *   pack_embedding      e f32 [rows][d] -> bf16 [rows_pad][d], rows past `rows` zero
 *   dgelu_mul           out = dy * gelu'(u) over n elements (bf16: n % 8 == 0)
 *   dlogits_from_f32    src f32 [rows][V] -> [rows][ld], columns >= V zero;  logits_to_f32: [rows][ld] -> f32 [rows][V]
 *   layernorm_bwd       oasr_layernorm_bwd with dsum (optional [d]: += column sums of the stored dx) and nullable dgamma / dbeta */
int oasr_test_embedding_fwd(const int64_t* tok, const float* E, const float* pos, void* x, int dtype, int B, int S, int d, int64_t n_embed,
                            const int32_t* rows, void* stream);
int oasr_test_embedding_bwd(const int64_t* tok, const void* dx, int dtype, float* dE, float* dpos, int B, int S, int d, int64_t pad_id,
                            int64_t n_embed, const int32_t* rows, const int32_t* span, void* stream);
int oasr_test_colsum(const void* x, int dtype, int64_t ld, int64_t M, int ncols, float* out, void* stream);
int oasr_test_conv2_col2im_dgelu(const void* dA, const void* u1, void* dpre1, int dtype, int B, int T1, int d, void* stream);
int oasr_test_conv1_col2im_mel(const void* dcol, int dtype, float* dmel, int B, int T1, int n_mels, void* stream);
int oasr_test_mel_to_time_major(const float* mel, void* out, int dtype, int B, int n_mels, int T, const float* clip_max, void* stream);
int oasr_test_pack_conv_weight(const float* w, void* dst, int dtype, int co, int ci, int ldk, void* stream);
int oasr_test_unpack_conv_grad(const float* g, float* dw, int co, int ci, int ldk, void* stream);
int oasr_test_pack_embedding(const float* e, void* dst, int rows, int rows_pad, int d, void* stream);
int oasr_test_dgelu_mul(const void* dy, const void* u, void* out, int dtype, int64_t n, void* stream);
int oasr_test_dlogits_from_f32(const float* src, int V, int64_t rows, int64_t ld, void* dst, int dtype, void* stream);
int oasr_test_logits_to_f32(const void* logits, int dtype, int64_t ld, int64_t rows, int V, float* out, void* stream);
int oasr_test_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, const void* dres, void* dx,
                            float* dgamma, float* dbeta, float* dsum, int dtype, int64_t rows, int d, void* stream);

/* tests (CPU, tests/test_alignment_cpu.py): oasr_dtw's algorithm run on the HOST.  Shared with the kernel through csrc/dtw_core.h: the cell
 * update, the skewed trace index and the 64-cell backtrace step.  The forward loop over anti-diagonals (one "thread" per row, two cost rows) is
 * re-stated in csrc/dtw_host.cpp; the kernel's register prefetch of the costs and its LDS double buffer are covered by the GPU suite only.
 * All pointers are host memory; workspace: oasr_dtw_workspace_bytes(N, M) bytes.  Touches no device. */
int oasr_test_dtw_host(const float* cost, int64_t ld, int N, int M, int negate, int32_t* text_indices, int32_t* time_indices, int32_t* path_len,
                       void* workspace);

/* tests (tests/test_gpu_train_pred.py): the prediction kernel of oasr_train_step's pred_out on a caller's matrix and tables, like the glue
 * operators above (no process state, no opt-in).  logits: [n_rows][ld] in `dtype`, ld >= V (16-byte aligned rows that hold V rounded up to a 16-byte piece are read in such pieces, others column by column);
 * rows: device int32 [B][OASR_ROWTAB] chunk-row table; span: device int32 [B], multiples of 64, <= S; pred_out: device int32 [B][S]:
 *     pred_out[b, s] = argmax over c < V of logits[rows[b][s >> 6] + (s & 63)][c] for s < span[b] (lowest index among equal maxima), else -1;
 * a table entry that points outside [0, n_rows) also gives -1 (the row is not read). */
int oasr_test_argmax_rows(const void* logits, int dtype, int64_t ld, int V, int64_t n_rows, const int32_t* rows, const int32_t* span, int B, int S,
                          int32_t* pred_out, void* stream);

/* tests (tests/test_gpu_vocab_planted.py): oasr_cross_entropy_ex -- count_valid, the cross-entropy kernel, loss_reduce -- on logits of either
 * type, argument for argument: dtype = OASR_DTYPE_BF16 runs the production kernel (what oasr_cross_entropy_ex runs), OASR_DTYPE_F32 the fp32
 * validation kernel of the fp32 engine (logits fp32 [rows][ld], any ld >= V), which has no entry of its own in the product ABI.  No process state,
 * no opt-in. */
int oasr_test_cross_entropy(void* logits, int dtype, int64_t ld, int V, const int64_t* targets, int64_t rows, int64_t ignore, float gscale,
                            int32_t* n_valid_dev, float* row_loss, float* loss_out, int write_grad, float label_smoothing, float z_loss,
                            float* row_parts, void* stream);

#ifdef __cplusplus
}
#endif
#endif
