// Internal launch interface between the kernel translation units and the engine (not part of the C ABI).
#pragma once
#include "common.h"
#include "decode_step_core.h"

// A row-major bf16 operand, optionally viewed as overlapping convolution windows:
//   plain   : element (r, k) at  r*ld + k
//   windows : rpb > 0.  r = b*rpb + t ; element (r,k) at  b*bstride + t*ld - lead + k, and it is an implicit
//             zero when k >= kvalid, or (t == 0 && k < lead), or (t == rpb-1 && k >= trail_from).
//             conv1 (k3,s1,p1) over time-major mel [B][3000][80]  : ld=80,  rpb=3000, lead=80, kvalid=240, trail_from=160
//             conv2 (k3,s2,p1) over time-major h1 [B][3000][d]    : ld=2d,  rpb=1500, lead=d,  kvalid=3d,  trail_from=3d
// T = bf16_t: the production kernels.  T = float: the fp32 VALIDATION kernels (fp32ref.hip) that run the same engine
// schedule with fp32 activations, fp32 operands and fp32 accumulation -- the reference's precision="float32" path
// (scripts/training/train_timestamps.py:2128,2220-2224), used to hold the engine to 1e-3 against the fp32 CPU oracle.
template <typename T>
struct OperandViewT {
  const T* ptr;
  long ld;
  int rpb;
  long bstride;
  int lead;
  int kvalid;
  int trail_from;
};
typedef OperandViewT<bf16_t> OperandView;
typedef OperandViewT<float> OperandViewF;
template <typename T>
static inline OperandViewT<T> plain_view(const T* p, long ld) {
  return OperandViewT<T>{p, ld, 0, 0, 0, 0, 0};
}

// C[M,N] = epilogue( alpha * sum_k A(m,k) * B(n,k) )
//   ta == 0 : A stored [M][K] (k contiguous);  ta == 1 : A stored [K][M] (m contiguous)
//   tb == 0 : B stored [N][K];                 tb == 1 : B stored [K][N]
// Epilogue, in this order, every pointer optional (fp32 math on the accumulator):
//   v = alpha*acc (+ bias[n]) ; out_pre <- bf16(v) ; if act: v = gelu(bf16(v)) ;
//   (act == 2: as act == 1, but out_pre <- bf16(gelu'(bf16(v))) -- the training forward of mlp.0 saves the derivative the
//    backward needs in the slot of the pre-activation, same bytes, so the dgrad epilogue is one multiply instead of ~25 VALU)
//   if pos: v = bf16(v) + pos[(m % pos_period)*N + n] ; if dgelu_u: v = bf16(v) * (dgelu_deriv ? u[m,n] : gelu'(u[m,n])) ;
//   if resid: v = bf16(v) + resid[m,n] ; out <- bf16(v) ; out_f32 <- (atomic ? += v : beta*out_f32 + v)
template <typename T>
struct GemmArgsT {
  OperandViewT<T> A, B;
  int M, N, K;
  int ta, tb;
  float alpha;
  const float* bias;
  int act;  // 0 none, 1 exact-erf GELU, 2 exact-erf GELU with out_pre = GELU'(pre-activation)
  const float* pos;
  int pos_period;
  const T* dgelu_u;
  long ldu;
  const T* resid;
  long ldr;
  T* out;
  T* out_pre;
  long ldc;
  float* out_f32;
  long ldc32;
  float beta;
  float* colsum;  // optional [N]: += column sums of the bf16 values stored to `out` (fused bias gradient)
  int atomic;   // out_f32 += v with hardware fp32 atomics (split-K safe)
  int split_k;  // >= 1; > 1 requires atomic out_f32 and no other output
  int raster_gm;  // fast path: tile rows per L2 group (0 = choose from residency)
  int dgelu_deriv;  // dgelu_u already holds GELU'(u) (written by an act == 2 forward)
  int stagger, stagger_phases;  // ping-pong kernel: first-wave phase stagger in units of s_sleep(127) (0 = off)
  int atomic_on_pp;             // split-K / atomic output on the 256x256 ping-pong kernel instead of the 256x128 one
  int vgrid;                    // set by the launcher: blocks of the virtual grid a persistent ping-pong launch walks
  int epi_flags;                // epilogue memory policy: bit 0 non-temporal output stores, bit 1 non-temporal side-input loads
  float* colsum_scratch;        // optional, with colsum on the direct-to-LDS kernels: fp32 [2 * ceil(M/256)][N] partial rows (one per
                                // 128-row wave block) that the launcher reduces into colsum -- instead of fp32 atomics from every wave
};
typedef GemmArgsT<bf16_t> GemmArgs;
typedef GemmArgsT<float> GemmArgsF;
int launch_gemm(const GemmArgs& a, hipStream_t stream);
int launch_gemm(const GemmArgsF& a, hipStream_t stream);  // fp32 validation kernel: any shape / view, split_k ignored
// bench-only: time every GEMM launch with HIP events on its stream; collect() sums per variant (2*ta+tb)
void gemm_profile_enable(int on);
int gemm_profile_lane(int lane);  // tag the following launches' profile records (0 = main stream, 1 = side stream); returns the old tag
void gemm_force_general(int on);  // tests: 0 = automatic choice, 1 = general kernel, 2 = 256x128, 3 = 256x256 two-stage, 4 = ping-pong
// tests / experiments on the ping-pong kernel: v < 0 = defaults; bits 0-3 = K-tile schedule (2, 7, or 8 = per-layout default), bits 4-5 = plain /
// persistent launch, bits 6-7 = non-temporal epilogue stores / side-input loads.  OASR_EINVAL, and no change, for a schedule that does not exist
int gemm_set_variant(int v);
void gemm_set_stagger(int sleeps, int phases);  // experiments: first-wave phase stagger of the ping-pong kernel
int gemm_profile_collect(double ms[4], double flops[4], long count[4], char* by_symbol, int cap);
int gemm_profile_records(char* buf, int cap);  // tests: one text line per recorded launch (kernel symbol, shape, layout, epilogue flags, launch options)
template <typename T>
static inline GemmArgsT<T> gemm_defaults_t() {
  GemmArgsT<T> g;
  memset(&g, 0, sizeof(g));
  g.alpha = 1.0f;
  g.split_k = 1;
  return g;
}
static inline GemmArgs gemm_defaults() { return gemm_defaults_t<bf16_t>(); }

// LayerNorm over the last dim (eps 1e-5, fp32 internals, bf16 in/out; reference model.py:39)
int launch_layernorm_fwd(const bf16_t* x, const float* gamma, const float* beta, bf16_t* y, float* mean, float* rstd,
                         long rows, int d, hipStream_t s);
// dx = LN'(dy) (+ dres) ; dgamma/dbeta are ACCUMULATED (atomic fp32) into the grad arena; dsum (optional) += column
// sums of the produced dx (= the bias gradient of the Linear whose output this residual-stream gradient belongs to)
int launch_layernorm_bwd(const bf16_t* dy, const bf16_t* x, const float* gamma, const float* mean, const float* rstd,
                         const bf16_t* dres, bf16_t* dx, float* dgamma, float* dbeta, float* dsum, long rows, int d, hipStream_t s);
int launch_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, long rows, int d,
                         hipStream_t s);
int launch_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, const float* dres,
                         float* dx, float* dgamma, float* dbeta, float* dsum, long rows, int d, hipStream_t s);

// Flash attention over head_dim 64.  Q/K/V are strided views [B, T, H, 64] (row strides in elements);
// key j visible to query i iff j < kv_len[b] (nullptr -> Tk) and (!causal || j <= i).  scale = 1/8.
template <typename T>
struct AttnArgsT {
  const T *q, *k, *v;
  long ldq, ldk, ldv;        // token strides
  long bsq, bsk, bsv;        // batch strides
  T* o;                      // [B, Tq, H*64]
  long ldo, bso;
  float* lse;                // [B, H, Tq] natural-log-sum-exp of scaled scores
  T* o_lo;                   // optional bf16 rounding residual of o (same strides): fwd writes it, bwd uses o + o_lo for delta = rowsum(dO*O)
  const int32_t* kv_len;     // [B] or null
  int B, H, Tq, Tk, causal;
  // backward only
  const T* d_o;              // [B, Tq, H*64], same strides as o
  float* delta;              // [B, H, Tq] workspace: rowsum(dO * O)
  T *dq, *dk, *dv;           // same strides as q/k/v
  // optional [H*64] fp32, ACCUMULATED: column sums over all (b, t) rows of the stored dq / dv = the gradients of the
  // query / value projection biases (key has none, olmoasr/model.py:259), fused into the backward kernels' store epilogues
  float *dq_colsum, *dv_colsum;
  float* colsum_scratch;     // required with either: fp32 [(B*ceil(Tq/128) + B*ceil(Tk/128)) * H*64] per-workgroup partial rows
  // optional int32 [B, H, ceil(Tq/64)] workspace: the dQ kernel records which 64-query tiles of d_o hold any non-zero value, the
  // dK/dV kernel stops at the last such tile (decoder side of a padded batch: the loss ignores the padded positions, their d_o rows
  // are exactly zero and contribute exactly nothing -- three quarters of the 448 positions on average).  Results are bit-identical.
  int32_t* qtile_flags;
  // ---- chunked token rows (the decoder side of a span-limited training step, engine_step.hip "supervised span") -----------------
  // q_rows / k_rows: optional int32 [B][OASR_ROWTAB]: entry c = first token row (relative to the tensor base pointers, batch
  // strides unused) of the 64-position chunk c of sample b; q_rows addresses q / o / o_lo / d_o / dq, k_rows k / v / dk / dv.
  // lse / delta / qtile_flags keep their logical [B, H, Tq] indexing.  Needs Tq (Tk) % 64 == 0 and <= 64 * OASR_ROWTAB.
  const int32_t *q_rows, *k_rows;
  // q_span: optional int32 [B], multiples of 64 (backward only): d_o of sample b is zero at every query position >= q_span[b];
  // those rows of d_o / o are not read, dq (and, for self-attention, dk / dv: their keys see no supervised query) not written.
  const int32_t* q_span;
  // ---- compact grids over the span (with q_rows and q_span) --------------------------------------------------------------------
  // qblk128 / qblk256: optional int32 [n128 * H] / [n256 * H] block tables written by launch_build_span_tables from the SAME spans as
  // q_span: entry v = attn_qblk_pack(b, h, query block) of the v-th 128- / 256-query block that lies inside its sample's span, in
  // (b, h, block) order; n128 = sum_b ceil(q_span[b] / 128), n256 likewise.  The chunked-row kernels are then launched over n * H
  // workgroups instead of ceil(Tq / 128 | 256) * B * H of which those past the span only exit.  Null = the full grid.  n128 == 0 (every
  // span 0): nothing is launched.  Results are bit-identical to the full grid's.
  const int32_t *qblk128, *qblk256;
  int n128, n256;
};
// block-table entry: sample << 16 | head << 4 | query block (B <= 512, <= 16 blocks)
__host__ __device__ static inline int32_t attn_qblk_pack(int b, int h, int blk) { return (int32_t)((b << 16) | (h << 4) | blk); }
#ifndef OASR_ROWTAB
#define OASR_ROWTAB 16  // (also defined by include/oasr.h)
#endif
static inline size_t attn_colsum_scratch_floats(int B, int H, int Tq, int Tk) {
  return (size_t)B * ((size_t)(Tq + 127) / 128 + (size_t)(Tk + 127) / 128) * H * 64;
}
typedef AttnArgsT<bf16_t> AttnArgs;
typedef AttnArgsT<float> AttnArgsF;
int launch_attention_fwd(const AttnArgs& a, hipStream_t s);
int launch_attention_bwd(const AttnArgs& a, hipStream_t s);
// qk of MultiHeadAttention.qkv_attention (model.py:347-442): fp32 pre-softmax scaled scores [B, H, Tq, Tk], masked entries -inf (scores.hip)
int launch_attention_scores(const AttnArgs& a, float* out, hipStream_t s);
void attention_set_pingpong(int on);  // testing hook: 0 = general kernels for the unmasked case too
void attention_set_span_grid(int on);  // testing hook: 0 = the full grid even when a block table (AttnArgs.qblk128 / qblk256) is given
int launch_attention_fwd(const AttnArgsF& a, hipStream_t s);  // fp32 validation kernels (o_lo unused: O is fp32)
int launch_attention_bwd(const AttnArgsF& a, hipStream_t s);
int launch_attention_scores(const AttnArgsF& a, float* out, hipStream_t s);

// ---- LayerNorm-folded decode projection (decode_proj.hip) ------------------------------------------------
int launch_decode_proj(const bf16_t* x, int M, int K, const bf16_t* W, int N, const float* ln_g, const float* ln_b, const float* bias,
                       int gelu, const bf16_t* resid, long ldr, bf16_t* out, long ldc, float* out_f32, long ldf, hipStream_t s);

// ---- one-launch decoder steps: the one-XCD team for <= 4 sequences (decode_xcd.hip), the chip-wide engine for one (decode_wide.hip) ----------
// Host-only: what either launcher takes.  Which shapes and layouts an engine accepts: decode_xcd_plan.h / decode_wide_plan.h.
struct DecodeStepBufs {  // the memory of a step: what the launchers hand on unchanged, so both kernels' arguments begin with it too
  const bf16_t* wflat;  // bf16 shadow of the flat parameter arena
  const float* params;  // fp32 parameter arena (LayerNorm parameters, biases)
  const float* aux;     // fused [q_bias | 0 | v_bias] rows
  bf16_t* cache;        // KV cache (per layer: self q|k|v [M, S_max, 3d], cross k|v [M, Te, 2d])
  long cache_lstride;   // elements per layer
  bf16_t *x, *x2, *x3, *q, *o, *hg;  // activation rows [M][d] ([M][4d] for hg): x holds the embedded token on entry and the last block's output on return
  float* part;          // cross-attention partials (m, l, o[64]): decode_xcd_part_floats() / decode_wide_part_floats() floats
  unsigned* ctrl;       // the cache's control tail (OASR_KV_TAIL_BYTES, laid out by decode_step_core.h), zeroed once per cache (oasr_decode_begin)
};
struct DecodeStepArgs : DecodeStepBufs {
  int d, H, Te, S_max, L, M, pos;
  int flags;            // experiments (decode_step_core.h: StepFlags), 0 in production
  void* stamps;         // optional 512-byte device buffer for in-kernel cycle stamps (measurement), or null
  int team, stride;     // `team` workgroups; stride 8 = one per CU of ONE XCD (grid 8 x team, blockIdx % 8 == 0), 1 = spread over the chip
  // chip-wide engine only: the final LayerNorm + tied logits projection as the launch's last phase (null logits_out: not done there)
  const bf16_t* w_logits = nullptr;  // bf16 token embedding [V][d]
  const float *lnf_g = nullptr, *lnf_b = nullptr;
  float* logits_out = nullptr;       // f32 [V]
  int V = 0;
  DecLayerOffsets l0;             // element offsets of decoder layer 0
  long lstride, astride;          // layer l = layer 0 + l * lstride (arena / shadow elements), + l * astride for the aux entry
};
int launch_decode_xcd(const DecodeStepArgs& a, hipStream_t s);
int launch_decode_wide(const DecodeStepArgs& a, hipStream_t s);  // `team` = workgroups (one per CU)

// ---- elementwise / reductions -------------------------------------------------------------------------
int launch_cast_f32_bf16(const float* src, bf16_t* dst, long n, hipStream_t s);
// conv weight [co][ci][3] f32 -> bf16 [co][ldk] with k = kk*ci_n + ci, zero padded to ldk
int launch_pack_conv_weight(const float* w, bf16_t* dst, int co, int ci, int ldk, hipStream_t s);
// grad [co][ldk] f32 (k = kk*ci_n+ci) accumulated into dw [co][ci][3]
int launch_unpack_conv_grad(const float* g, float* dw, int co, int ci, int ldk, hipStream_t s);
// token embedding rows f32 [rows][d] -> bf16 [rows_pad][d], rows >= rows zero
int launch_pack_embedding(const float* e, bf16_t* dst, int rows, int rows_pad, int d, hipStream_t s);
// mel f32 [B][80][T] -> bf16 time-major [B][T][80]
// clip_max (optional [B]): mel is the un-finalized log10 mel power of oasr_log_mel_raw; max(x, clip_max[b] - 8), (x + 4) / 4 on the fly
int launch_mel_to_time_major(const float* mel, bf16_t* out, int B, int n_mels, int T, hipStream_t s, const float* clip_max = nullptr);
// x[b,s,:] = bf16(E[tok[b,s]] + pos[s]);  rows (optional): chunk-row table [B][OASR_ROWTAB] -- x row of (b, s) =
// rows[b][s >> 6] + (s & 63) instead of b*S + s
int launch_embedding_fwd(const int64_t* tok, const float* E, const float* pos, bf16_t* x, int B, int S, int d, long n_embed,
                         hipStream_t s, const int32_t* rows = nullptr);
// dE[tok] += dx (skipping pad_id), dpos[s] += sum_b dx;  span (optional, with rows): positions s >= span[b] hold no gradient and are skipped
int launch_embedding_bwd(const int64_t* tok, const bf16_t* dx, float* dE, float* dpos, int B, int S, int d, long pad_id, long n_embed,
                         hipStream_t s, const int32_t* rows = nullptr, const int32_t* span = nullptr);
// Supervised-span tables of one decoder micro-batch (engine_step.hip): span_host[b] (host, <= S) -> on the device
//   rows [B][OASR_ROWTAB]: the chunk-row table -- the active chunks (64*c < span[b]) of all samples first, position-block-major,
//                          then the inactive ones; span_dev [B] = span rounded up to 64; targets_phys [B*S]: targets in row order
// Returns the number of active token rows through *active_rows (host).  S % 64 == 0, S <= 64 * OASR_ROWTAB, B <= 512.
// blocks (optional): the query-block tables of AttnArgs.qblk128 / qblk256 for H heads, written by the same launch; the counts come back
// on the host (they follow from span_host alone: no synchronisation).
struct SpanBlockTables {
  int H;
  int32_t *blk128, *blk256;  // device, span_block_entries(B, S, H, 128 | 256) entries
  int n128, n256;            // out (host): blocks inside the spans, per head
};
static inline size_t span_block_entries(int B, int S, int H, int gran) { return (size_t)B * ((S + gran - 1) / gran) * H; }
int launch_build_span_tables(const int32_t* span_host, int B, int S, const int64_t* targets, long ignore, int32_t* rows, int32_t* span_dev,
                             int64_t* targets_phys, long* active_rows, hipStream_t s, SpanBlockTables* blocks = nullptr);
// out[n] += sum_m x[m, n]   (x bf16 [M, ld], columns [0, ncols))
int launch_colsum_accum(const bf16_t* x, long ld, long M, int ncols, float* out, hipStream_t s);
// conv2 input-gradient fold + conv1 GELU backward: dpre1[b,t,c] = gelu'(u1) * sum of the dA windows covering t
int launch_conv2_col2im_dgelu(const bf16_t* dA /*[B*T2][3d]*/, const bf16_t* u1 /*[B*T1][d]*/, bf16_t* dpre1, int B, int T1,
                              int d, hipStream_t s);
// conv1 input gradient (conv_grad.hip): dcol [B*T1][256] = the conv1 data gradient as im2col columns (k*n_mels + c) -> fp32 channel-major
//   dmel[b][c][t] = sum_{k=0..2, 0 <= t+1-k < T1} dcol[b*T1 + t+1-k][k*n_mels + c]   (taps in the zero padding / the next sample dropped)
int launch_conv1_col2im_mel(const bf16_t* dcol, float* dmel, int B, int T1, int n_mels, hipStream_t s);
int launch_conv1_col2im_mel(const float* dcol, float* dmel, int B, int T1, int n_mels, hipStream_t s);
// dst(f32) += src(f32) over n  (grad of the fp32 sinusoid buffer is not needed; used for misc accumulations)
int launch_axpy_f32(const float* src, float* dst, long n, float a, hipStream_t s);
// fp32 validation overloads (fp32ref.hip): same contracts with fp32 activations
int launch_pack_conv_weight(const float* w, float* dst, int co, int ci, int ldk, hipStream_t s);
int launch_mel_to_time_major(const float* mel, float* out, int B, int n_mels, int T, hipStream_t s, const float* clip_max = nullptr);
int launch_embedding_fwd(const int64_t* tok, const float* E, const float* pos, float* x, int B, int S, int d, long n_embed, hipStream_t s,
                         const int32_t* rows = nullptr);
int launch_embedding_bwd(const int64_t* tok, const float* dx, float* dE, float* dpos, int B, int S, int d, long pad_id, long n_embed,
                         hipStream_t s, const int32_t* rows = nullptr, const int32_t* span = nullptr);
int launch_colsum_accum(const float* x, long ld, long M, int ncols, float* out, hipStream_t s);
int launch_conv2_col2im_dgelu(const float* dA, const float* u1, float* dpre1, int B, int T1, int d, hipStream_t s);
int launch_dgelu_mul(const bf16_t* dy, const bf16_t* u, bf16_t* out, long n, hipStream_t s);
int launch_dgelu_mul(const float* dy, const float* u, float* out, long n, hipStream_t s);
int launch_logits_to_f32(const bf16_t* logits, long ld, long rows, int V, float* out, hipStream_t s);
int launch_logits_to_f32(const float* logits, long ld, long rows, int V, float* out, hipStream_t s);
int launch_dlogits_from_f32(const float* src, int V, long rows, long ld, bf16_t* dst, hipStream_t s);  // fp32 [rows, V] -> padded [rows, ld]
int launch_dlogits_from_f32(const float* src, int V, long rows, long ld, float* dst, hipStream_t s);

// ---- loss -------------------------------------------------------------------------------------------------
// logits bf16 [rows][ld] (first V entries valid).  Writes, in place, dlogits = (softmax - onehot) * gscale / n_valid
// (zeros for ignored rows and pad columns), row_loss[r] = lse - logit[target] (0 for ignored rows).
// n_valid_dev: device int32 (count of targets != ignore inside [0, V): an id outside that range is an ignored row, not an error).
// loss_out += sum(row_loss)/n_valid * loss_mul.  Columns [V, ld) may hold anything on entry, NaN included; write_grad = 0 leaves the logits untouched.
int launch_count_valid(const int64_t* targets, long rows, long ignore, int V, int32_t* n_valid_dev, hipStream_t s);
// CeReg: the regularisers of the objective (include/oasr.h at oasr_train_step_args.label_smoothing); all zero = the plain kernel, launch for
// launch.  Otherwise row_loss[r] = lse - (1 - eps) x_t - eps / V sum_{c<V} x_c + z lse^2, dlogits = g [(1 + 2 z lse) softmax - (1 - eps) onehot
// - eps / V] on the first V columns (pad columns and ignored rows stay exactly zero); parts (optional): parts[r] = lse - x_t,
// parts[parts_stride + r] = lse^2.
struct CeReg {
  float eps = 0.f, z = 0.f;
  float* parts = nullptr;
  long parts_stride = 0;
  bool on() const { return eps != 0.f || z != 0.f || parts; }
};
int check_ce_reg(const char* who, float label_smoothing, float z_loss);  // OASR_EINVAL naming the field: eps outside [0, 1), z < 0, non-finite
int launch_cross_entropy(bf16_t* logits, long ld, int V, const int64_t* targets, long rows, long ignore, float gscale,
                         const int32_t* n_valid_dev, float* row_loss, int write_grad, hipStream_t s, const CeReg& reg = CeReg());
int launch_cross_entropy(float* logits, long ld, int V, const int64_t* targets, long rows, long ignore, float gscale,
                         const int32_t* n_valid_dev, float* row_loss, int write_grad, hipStream_t s, const CeReg& reg = CeReg());  // fp32 validation
int launch_loss_reduce(const float* row_loss, long rows, const int32_t* n_valid_dev, float mul, float* loss_out, int accumulate,
                       hipStream_t s);

// ---- token selection (select.hip) ---------------------------------------------------------------------------------------------------
// The argument block of the four launchers, in the order of the C ABI (include/oasr.h at oasr_pick_tokens_ts): logits fp32 [rows][ld], V
// columns valid; mask / mask2: optional additive fp32 [V] (0 / -inf); hist int64 [rows][hist_ld], n_hist tokens sampled so far, and the
// token ids whisper's ApplyTimestampRules needs (n_hist < 0: no timestamp rules, none of these is read); tok / logprob: the outputs.
struct SelectArgs {
  const float* logits;
  long ld;
  int V;
  long rows;
  const float *mask, *mask2;
  const int64_t* hist = nullptr;
  long hist_ld = 0;
  int n_hist = -1, ts_begin = 0, eot = 0, no_ts = 0, max_initial_index = -1;
  int64_t* tok = nullptr;
  float* logprob = nullptr;
};
// tok[r] = argmax_c (logits[r][c] + mask[c] + mask2[c]) (lowest index on ties), logprob[r] = log_softmax of that entry (optional)
// The empty row, for this launcher and the three below: a row in which no column survives (every entry -inf after the masks and the rules) gives
// token 0 and log-probability -inf -- never NaN -- and top-k entries past the last survivor are (0, -inf) likewise.  Columns [V, ld) are never read.
int launch_pick_tokens(const SelectArgs& a, hipStream_t s);  // (no rules: reads neither the history nor the ids)
// + whisper's ApplyTimestampRules evaluated from the device-resident sampled history (n_hist >= 0 required)
int launch_pick_tokens_ts(const SelectArgs& a, hipStream_t s);
// the K best (log_softmax, token) pairs per row over the same filtered distribution (n_hist < 0: masks only, no timestamp rules):
// tok / logprob [rows][K] -- BeamSearchDecoder.update's topk(beam_size + 1)
int launch_topk_tokens_ts(const SelectArgs& a, int K, hipStream_t s);
// one draw per row from softmax(filtered logits / temperature) by inverse CDF on u[row] in [0, 1); logprob at temperature 1
int launch_sample_tokens_ts(const SelectArgs& a, float temperature, const float* u, hipStream_t s);

// ---- word-timestamp alignment (align.hip; the argument block and the contracts: include/oasr.h) ---------------------------------
// score planes of the selected heads, read in place -> fp32 [n_tok, n_frames]; workspace of oasr_alignment_workspace_bytes
struct oasr_align_args;
int launch_alignment_matrix(const oasr_align_args* a, void* workspace, size_t workspace_bytes, hipStream_t s);
// timing.py::dtw bit for bit, one workgroup, path left on the device; workspace of oasr_dtw_workspace_bytes (dtw_core.h)
int launch_dtw(const float* cost, long ld, int N, int M, int negate, int32_t* text_indices, int32_t* time_indices, int32_t* path_len,
               void* workspace, size_t workspace_bytes, hipStream_t s);

// ---- token error counts (editdist.hip; the contract: include/oasr.h at oasr_edit_counts, the rule: editdist_core.h) ---------------------
struct oasr_edit_args;
int launch_edit_counts(const oasr_edit_args* a, hipStream_t s);

// ---- device-resident beam search (beam.hip; the contract: include/oasr.h at oasr_beam_update, the rule: beam_core.h) --------------------
struct oasr_beam_args;
int launch_beam_update(const oasr_beam_args* a, hipStream_t s);
// row j of the self-attention cache continues row sources[j] (device int32 [B]), in place: per layer (layer_stride BYTES apart) the rows are
// [B][n_ctx][3d] elements of elem_size bytes, and the columns [d, 3d) of positions < pos move; d * elem_size % 16 == 0
int launch_kv_reorder(void* rows, long layer_stride, int L, int B, int n_ctx, int d, int elem_size, int pos, int group, const int32_t* sources,
                      hipStream_t s);

// ---- teacher-forced predictions of the span step (argmax.hip) --------------------------------------------------------------------------
// pred[b, s] = argmax_c<V logits[rows[b][s >> 6] + (s & 63)][c] (lowest index among equal maxima) for s < span[b], else -1; logits
// [n_rows][ld], rows int32 [B][OASR_ROWTAB], span int32 [B] (multiples of 64), pred int32 [B][S].  Reads each active row once.
int launch_argmax_rows(const bf16_t* logits, long ld, int V, long n_rows, const int32_t* rows, const int32_t* span, int B, int S, int32_t* pred,
                       hipStream_t s);
int launch_argmax_rows(const float* logits, long ld, int V, long n_rows, const int32_t* rows, const int32_t* span, int B, int S, int32_t* pred,
                       hipStream_t s);

// ---- teacher-forced scoring (score.hip; the contract: include/oasr.h at oasr_score, the reduce rule: score_core.h) ----------------------
// row (b, s) of logits [B * S][ld]: s >= span[b]: (row_nll, pred) = (0, -1), row not read; else pred = argmax_c<V (lowest index among equal
// maxima) and row_nll = logsumexp(x[:V]) - x_t for a valid target (0 <= t < V, t != ignore), exactly 0 otherwise.  Reads each active row once.
int launch_score_rows(const bf16_t* logits, long ld, int V, const int64_t* targets, const int32_t* span, int B, int S, long ignore, float* row_nll,
                      int32_t* pred, hipStream_t s);
int launch_score_rows(const float* logits, long ld, int V, const int64_t* targets, const int32_t* span, int B, int S, long ignore, float* row_nll,
                      int32_t* pred, hipStream_t s);
// per sample: nll_sum (double sum in ascending s, rounded once), nll_max, n_tok, n_hit over the counted rows; one wave per sample
int launch_score_reduce(const float* row_nll, const int32_t* pred, const int64_t* targets, const int32_t* span, int B, int S, int V, long ignore,
                        float* nll_sum, float* nll_max, int32_t* n_tok, int32_t* n_hit, hipStream_t s);

// ---- SpecAugment (specaug.hip; the policy block and the rule: include/oasr.h, specaug_core.h) ------------------------------------
// mel fp32 [B, n_mels, T] in place: the seeded masks of clips first_clip .. first_clip + B - 1 set to policy->fill, nothing else written
struct oasr_specaug;
int launch_spec_augment(float* mel, int B, int n_mels, int T, const oasr_specaug* policy, uint64_t seed, uint64_t first_clip, hipStream_t s);

// ---- speed perturbation (speed.hip; the contract: include/oasr.h at oasr_speed_perturb, the rule: speed_core.h) ---------------------------
// pcm_out = each clip of pcm_in resampled by its seeded factor (or copied), timestamp tokens rescaled in place; one launch, plan on the device
struct oasr_speed_args;
int launch_speed_perturb(const oasr_speed_args* a, hipStream_t s);

// ---- noise mixing (noise.hip; the contract: include/oasr.h at oasr_noise_mix, the rule: noise_core.h) -------------------------------------
// pcm_out = each drawn clip of pcm_in plus its bank row at the drawn offset and SNR (else a copy); two launches (exact per-tile energies into
// a->workspace, then gain and mix), plan on the device
struct oasr_noise_args;
size_t noise_workspace_bytes(int B, int N);
int launch_noise_mix(const oasr_noise_args* a, hipStream_t s);

// ---- reverberation (reverb.hip; the contract: include/oasr.h at oasr_reverb, the rule: reverb_core.h) -------------------------------------
// pcm_out = each drawn clip of pcm_in convolved with its bank row on the int8 matrix cores (else a copy); two launches (the bank expanded into
// a->workspace as MFMA operands, then the convolution), plan on the device
struct oasr_reverb_args;
size_t reverb_workspace_bytes(int R, int K);
int launch_reverb(const oasr_reverb_args* a, hipStream_t s);

// ---- telephone channel (telephone.hip; the contract: include/oasr.h at oasr_telephone, the rule: telephone_core.h) ------------------------
// pcm_out = each drawn clip of pcm_in band-passed to 8 kHz, companded by its drawn G.711 codec and interpolated back (else a copy); one
// launch, plan on the device, tables from the host half (telephone_host.cpp) as kernel arguments
struct oasr_telephone_args;
int launch_telephone(const oasr_telephone_args* a, hipStream_t s);

// ---- LoRA adapters in weight space (lora.hip) -----------------------------------------------------------------
// out = W0 + scale * B . A  (W0 [rows][cols] fp32, A [r][cols], B [rows][r]; k sum in ascending order): exactly one of out32 (fp32, may be w0
// itself) / out16 (bf16, the rounding of launch_cast_f32_bf16)
int launch_lora_merge(const float* w0, const float* A, const float* B, int rows, int cols, int r, float scale, float* out32, bf16_t* out16,
                      hipStream_t s);
// dB += scale * dW . A^T, dA += scale * B^T . dW (dW [rows][cols] fp32 read once; deterministic two-pass reduction through `scratch`;
// a null dA or dB is skipped)
size_t lora_grad_scratch_floats(int rows, int cols, int r);
int launch_lora_grad(const float* dW, const float* A, const float* B, int rows, int cols, int r, float scale, float* dA, float* dB, float* scratch,
                     hipStream_t s);

// ---- optimizer (flat fp32 arenas) ---------------------------------------------------------------------------
// stats[0] = sum g^2 (of the *scaled* grads), stats[1] = found_inf flag (nonzero if any non-finite)
int launch_grad_stats(const float* g, long n, double* partial /*[1024]*/, float* stats /*[2]*/, hipStream_t s);
// Fused unscale + clip + AdamW (decoupled decay) + bf16 shadow emit.  Skips everything when stats[1] != 0.
int launch_adamw(float* p, const float* g, float* m, float* v, bf16_t* shadow, long n, const float* stats, float inv_scale,
                 float max_norm, float lr, float b1, float b2, float eps, float wd, float bc1, float bc2, hipStream_t s);
// the same two passes over a device table of (offset, numel) runs of the arena (the trainable tensors, oasr_set_trainable)
int launch_grad_stats_runs(const float* g, const int64_t* runs, int nruns, double* partial /*[1024]*/, float* stats /*[2]*/, hipStream_t s);
int launch_adamw_runs(float* p, const float* g, float* m, float* v, bf16_t* shadow, const int64_t* runs, int nruns, const float* stats,
                      float inv_scale, float max_norm, float lr, float b1, float b2, float eps, float wd, float bc1, float bc2, hipStream_t s);
