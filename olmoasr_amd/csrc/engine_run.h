// Host-side engine: workspace planning and the explicit forward / backward schedule of the OLMoASR training micro-step (the parameter
// layout it runs over is engine.hip's, its entry points are engine_step.hip / engine_decode.hip).  No autograd tape: every saved activation
// has a planned slot in the caller's workspace and the backward is written out by hand, layer by layer, in the order gradients become
// final (so per-segment events can release RCCL buckets while the rest of the backward is still running).
//
// Reference schedule being replaced: OLMoASR.forward (olmoasr/model.py:856-887) -> AudioEncoder.forward (:571-623)
// -> TextDecoder.forward (:688-775) -> F.cross_entropy(ignore_index=51864)/accum (train_timestamps.py:1444-1450)
// -> scaler.scale(loss).backward() (:1454) -> unscale_/clip_grad_norm_/AdamW (:1509-1512).
#pragma once
#include "engine_ctx.h"

namespace {

// The GEMM launch statistics' lane tag (gemm_profile_lane) is process-wide: a step that changes it puts it back to its value on entry
// when its scope ends, on every path -- an early error return must not leave every later launch of the process mislabelled.
struct LaneScope {
  const int entry = gemm_profile_lane(-1);
  ~LaneScope() { gemm_profile_lane(entry); }
};

// Everything below is written once for both compute dtypes: T = bf16_t (production) or float (validation).
template <typename T>
struct Engine {
  typedef OperandViewT<T> View;
  typedef GemmArgsT<T> Gemm;
  typedef AttnArgsT<T> Attn;

struct AttnSave {
  T *ln, *qkv, *o;  // self: qkv [M,3d];  cross: qkv = q [M,d]
  T* kv;            // cross only: [B*Te, 2d]
  float *mean, *rstd, *lse;
  T* o_lo;  // training only: bf16 rounding residual of the attention output (o + o_lo = fp32-grade O for the backward's delta)
};
struct BlockSave {
  T* x_in;  // residual stream entering the block (owned by the previous stage)
  AttnSave sa, ca;
  T *x_mid, *x_mid2, *ln2, *u, *hg, *x_out;
  float *mean2, *rstd2;
};

struct Plan {
  // encoder
  T *mel_tm, *u1, *h1, *u2, *x0, *xa;
  float *mean_p, *rstd_p;
  std::vector<BlockSave> enc, dec;
  // decoder
  T *dx0, *lnf, *logits;
  float *mean_f, *rstd_f, *row_loss;
  int32_t* n_valid;
  // backward temporaries
  T *ga, *gb, *gc, *gln, *gqkv, *go, *gu, *gxa, *gkv, *gq, *gA2;
  float *delta, *tmp_w1p, *tmp_w2p, *cs_scratch, *gemm_cs_scratch;
  int32_t* qtile_flags;  // attention backward of the decoder: which 64-position tiles of d_o are non-zero
  // supervised-span step (oasr_train_step with span_host): chunk-row table of the decoder's token rows, spans, targets in row order
  int32_t *rows, *span_dev;
  // query-block tables of the decoder attentions' compact grids (kernels.h: AttnArgs.qblk128 / qblk256).  They live in the slot of
  // qtile_flags: a span step does not use the flags (the span says where the all-zero tiles of d_o are), a plain step has no tables.
  // Null when the slot is too small for them (a 64-position context): the step then launches the full grids.
  int32_t *blk128, *blk256;
  int64_t* targets_phys;
  float *lora_dw, *lora_part;  // adapter contexts: the adapted weights' gradients (oasr_ctx::Lora::dw) and lora_grad's partial sums
};

static void plan_attn(Arena& A, AttnSave& s, long M, long Mkv, int d, int B, int H, long Tq, bool cross, bool train) {
  s.ln = A.template act<T>(M * d);
  s.qkv = A.template act<T>(M * (cross ? d : 3 * d));
  s.kv = cross ? A.template act<T>(Mkv * 2 * d) : nullptr;
  s.o = A.template act<T>(M * d);
  s.mean = A.f32(M);
  s.rstd = A.f32(M);
  s.lse = A.f32((long)B * H * Tq);
  s.o_lo = train ? A.template act<T>(M * d) : nullptr;
}

// In inference mode the per-layer buffers are shared between layers (allocated once); in training each layer
// gets its own slots because the backward needs them.
// stage (training plans only): STAGE_ALL = the fused step's plan (encoder + decoder, backward temporaries for the larger of the two);
// STAGE_ENC / STAGE_DEC = the plan of one stage of the staged autograd entries (oasr_train_encode* / oasr_train_decode*): the encoder's
// saved activations and encoder-sized backward temporaries (+ the d(mel) columns), or the decoder's own copy of xa, its saved activations
// and temporaries sized by the decoder rows (+ d(xa)).  A stage plan has no slot for the other stage (null pointers).
static void make_plan(const oasr_ctx* c, Arena& A, Plan& p, int B, int S, bool train, int stage = STAGE_ALL) {
  const int d = c->d;
  const long Me = (long)B * c->Te, M1 = (long)B * c->T1, Md = (long)B * S;
  const bool enc = stage != STAGE_DEC, dec = stage != STAGE_ENC;
  p = Plan();
  if (enc) {
    p.mel_tm = A.template act<T>(M1 * c->dims.n_mels + 2 * 256) + 256;  // zeroed guard rows on both sides (conv1 weight gradient windows)
    p.u1 = A.template act<T>(M1 * d);
    p.h1 = A.template act<T>(M1 * d + d) + d;  // one zeroed time row in front: the conv2 weight gradient reads h1 as overlapping windows from h1 - d
    p.u2 = A.template act<T>(Me * d);
    p.x0 = A.template act<T>(Me * d);
  }
  auto plan_block = [&](BlockSave& s, long M, long Tq, bool cross) {
    plan_attn(A, s.sa, M, 0, d, B, c->H, Tq, false, train);
    s.x_mid = A.template act<T>(M * d);
    if (cross) {
      plan_attn(A, s.ca, M, Me, d, B, c->H, Tq, true, train);
      s.x_mid2 = A.template act<T>(M * d);
    } else {
      s.x_mid2 = nullptr;
    }
    s.ln2 = A.template act<T>(M * d);
    s.u = A.template act<T>(M * 4 * d);
    s.hg = A.template act<T>(M * 4 * d);
    s.mean2 = A.f32(M);
    s.rstd2 = A.f32(M);
    s.x_out = A.template act<T>(M * d);
  };
  p.enc.resize(c->L_enc);
  p.dec.resize(c->L_dec);
  if (!enc) {
  } else if (train) {
    for (auto& s : p.enc) plan_block(s, Me, c->Te, false);
  } else {
    BlockSave s0, s1;
    plan_block(s0, Me, c->Te, false);
    s1 = s0;
    s1.x_out = A.template act<T>(Me * d);  // ping-pong the residual stream
    for (int i = 0; i < c->L_enc; ++i) p.enc[i] = (i & 1) ? s1 : s0;
  }
  p.xa = A.template act<T>(Me * d);  // (decoder stage: its own copy of the caller's xa)
  if (enc) {
    p.mean_p = A.f32(Me);
    p.rstd_p = A.f32(Me);
  }
  if (dec) {
    p.dx0 = A.template act<T>(Md * d);
    if (train) {
      for (auto& s : p.dec) plan_block(s, Md, S, true);
    } else {
      BlockSave s0, s1;
      plan_block(s0, Md, S, true);
      s1 = s0;
      s1.x_out = A.template act<T>(Md * d);
      for (int i = 0; i < c->L_dec; ++i) p.dec[i] = (i & 1) ? s1 : s0;
    }
    p.lnf = A.template act<T>(Md * d);
    p.mean_f = A.f32(Md);
    p.rstd_f = A.f32(Md);
    p.logits = A.template act<T>(Md * c->Vp);
    p.row_loss = A.f32(Md);
    p.n_valid = (int32_t*)A.raw(256);
  }
  if (train) {
    if (dec) {
      p.rows = (int32_t*)A.raw((size_t)B * OASR_ROWTAB * 4);
      p.span_dev = (int32_t*)A.raw((size_t)B * 4);
      p.targets_phys = (int64_t*)A.raw((size_t)Md * 8);
    }
    const long Mmax = stage == STAGE_ENC ? Me : stage == STAGE_DEC ? Md : (Me > Md ? Me : Md);
    p.ga = A.template act<T>(Mmax * d);
    p.gb = A.template act<T>(Mmax * d);
    p.gc = A.template act<T>(Mmax * d);
    p.gln = A.template act<T>(Mmax * d);
    p.gqkv = A.template act<T>(Mmax * 3 * d);
    p.go = A.template act<T>(Mmax * d);
    p.gu = A.template act<T>(enc && M1 * d > Mmax * 4 * d ? M1 * d : Mmax * 4 * d);  // also holds dpre1 [B*3000, d]
    if (dec) {
      p.gxa = A.template act<T>(Me * d);
      p.gkv = A.template act<T>(Me * 2 * d);
      p.gq = A.template act<T>(Md * d);
    }
    if (enc)  // (encoder stage: also the d(mel) columns [B*3000, 256] of the conv1 data gradient)
      p.gA2 = A.template act<T>(stage == STAGE_ENC && M1 * 256 > Me * 3 * d ? M1 * 256 : Me * 3 * d);
    p.delta = A.f32((long)B * c->H * (stage == STAGE_DEC ? S : c->Te));
    // (the largest of the three attention shapes)
    p.cs_scratch = A.f32(stage == STAGE_DEC ? attn_colsum_scratch_floats(B, c->H, S, S > c->Te ? S : c->Te)
                                            : attn_colsum_scratch_floats(B, c->H, c->Te, c->Te));
    if (dec) {
      const size_t n_flags = (size_t)B * c->H * ((S + 63) / 64) + 16, n128 = span_block_entries(B, S, c->H, 128);
      p.qtile_flags = (int32_t*)A.f32(n_flags);
      if (n128 + span_block_entries(B, S, c->H, 256) <= n_flags) {  // (every context of two or more 64-position chunks)
        p.blk128 = p.qtile_flags;
        p.blk256 = p.qtile_flags + n128;
      }
    }
    p.gemm_cs_scratch = A.f32((size_t)2 * cdiv(Mmax, 256) * 4 * d + 64);
    if (enc) {
      p.tmp_w1p = A.f32((long)d * 256);
      p.tmp_w2p = A.f32((long)d * 3 * d);
    }
    if (!c->lora.empty()) {
      p.lora_dw = A.f32(c->lora_dw_floats);
      p.lora_part = A.f32(c->lora_part_floats);
    }
    // the residual stream entering each block (block_fwd records the same pointers): a plan re-made for a backward-only call
    // (oasr_train_bwd) must be complete without having run the forward
    if (enc)
      for (int i = 0; i < c->L_enc; ++i) p.enc[i].x_in = i ? p.enc[i - 1].x_out : p.x0;
    if (dec)
      for (int i = 0; i < c->L_dec; ++i) p.dec[i].x_in = i ? p.dec[i - 1].x_out : p.dx0;
  }
}

struct Runner {
  const oasr_ctx* c;
  hipStream_t st;
  int B, S;
  const int32_t* text_len;
  bool train = false;  // the training forward saves GELU'(u) in place of u (GemmArgs.act == 2)
  float* cs_scratch = nullptr;  // partial rows of fused bias-gradient column sums (GemmArgs.colsum_scratch)
  // Supervised-span step: the decoder's token rows are CHUNKED (64 positions per chunk, kernels.h: AttnArgs.q_rows) with every
  // chunk that can carry gradient first, so the whole decoder backward runs on the first `dec_rows_bwd` rows as plain matrices.
  const int32_t* dec_rows = nullptr;  // chunk-row table [B][OASR_ROWTAB] (device) or null = plain [B, S] rows
  const int32_t* dec_span = nullptr;  // [B] spans rounded up to 64 (device); backward only
  long dec_rows_bwd = 0;              // active decoder rows (0 = all B*S)
  // the query blocks inside the spans, and how many there are per head: the span-limited decoder attentions are launched over these
  const int32_t *dec_blk128 = nullptr, *dec_blk256 = nullptr;
  int dec_n128 = 0, dec_n256 = 0;
  // opt-in (OASR_SPAN_FORWARD_ACTIVE): the decoder's FORWARD covers the active rows only as well.  The rows left out are the padded
  // positions whose logits the reference computes and nothing ever reads (no supervised query attends to them, the loss ignores them).
  long dec_rows_fwd = 0;
  const float* mel_clip_max = nullptr;  // [B] or null: `mel` is oasr_log_mel_raw's output, finalized in the time-major transpose
  float* lora_dw = nullptr;             // adapter contexts, backward: Plan::lora_dw
  // where the weight gradient of the tensor at `off` goes: its arena range, or -- an adapted base weight, frozen -- its workspace scratch
  float* Gw(int64_t off) const {
    const int j = c->lora_at(off);
    return j >= 0 ? lora_dw + c->lora[j].dw : c->G(off);
  }

  int linear(const T* x, long M, int K, const T* W, int N, const float* bias, int act, const T* resid, T* out,
             T* out_pre) {
    Gemm g = gemm_defaults_t<T>();
    g.A = plain_view(x, K);
    g.B = plain_view(W, K);
    g.M = (int)M;
    g.N = N;
    g.K = K;
    g.bias = bias;
    g.act = act;
    g.resid = resid;
    g.ldr = N;
    g.out = out;
    g.out_pre = out_pre;
    g.ldc = N;
    return launch_gemm(g, st);
  }
  // dx[M,K] = dy[M,N] . W[N,K]  (* gelu'(u))  (+ resid)
  int dgrad(const T* dy, long M, int N, const T* W, int K, const T* dgelu_u, const T* resid, T* dx,
            float* colsum = nullptr, bool u_is_deriv = false) {
    Gemm g = gemm_defaults_t<T>();
    g.A = plain_view(dy, N);
    g.B = plain_view(W, K);
    g.tb = 1;
    g.M = (int)M;
    g.N = K;
    g.K = N;
    g.dgelu_u = dgelu_u;
    g.dgelu_deriv = u_is_deriv ? 1 : 0;
    g.ldu = K;
    g.resid = resid;
    g.ldr = K;
    g.out = dx;
    g.ldc = K;
    g.colsum = colsum;
    g.colsum_scratch = colsum ? cs_scratch : nullptr;
    return launch_gemm(g, st);
  }
  // dW[N,K] += dy[M,N]^T . x[M,K]   (fp32 atomics, split over the token dimension)
  int wgrad(const T* dy, long ldy, long M, int N, const View& x, int K, float* dW, long ldw) {
    Gemm g = gemm_defaults_t<T>();
    g.A = plain_view(dy, ldy);
    g.ta = 1;
    g.B = x;
    g.tb = 1;
    g.M = N;
    g.N = K;
    g.K = (int)M;
    g.out_f32 = dW;
    g.ldc32 = ldw;
    g.atomic = 1;
    const long tiles = (long)cdiv(N, 256) * cdiv(K, 128);
    const long kt = cdiv(M, 64);
    // Split-K choice (scripts/wgrad_sweep.py): 768 workgroups are resident at once (3 per CU); what matters is how the
    // tiles x split grid quantises onto them (1.33 waves is the worst case), the (16 + split) K-tiles' worth of atomic epilogue
    // every workgroup adds, and that multiples of 8 let every XCD own whole K-ranges (gemm_fast.hip).
    long split = 1;
    double best = 1e30;
    static const int cand[] = {1, 2, 4, 8, 16, 24, 32};
    for (int s_ : cand) {
      if (s_ > 1 && (kt / s_ < 8 || tiles >= 768)) break;
      const double w = (double)tiles * s_, per = (double)kt / s_ + 16.0 + s_;  // atomics get slower the more splits collide
      const double waves = w <= 768.0 ? 0.7 + 0.3 * w / 768.0 : ceil(w / 768.0);
      const double score = per * waves;
      if (score < 0.97 * best) {
        best = score;
        split = s_;
      }
    }
    g.split_k = (int)split;
    // With its MFMA sections pinned the 256x256 ping-pong loop beats the 256x128 kernel on the square and the 4:1 weight shapes
    // (scripts/wgrad_sweep.py, profiles/r02_wgrad_sweep.txt; TF/s pp vs 256x128): 192k tokens [1024x1024] 1071 vs 972 (split 16),
    // [4096x1024] 1157 vs 1117 (8), [1024x4096] 1158 vs 1064 (4); 57k tokens [4096x1024] 1032 vs 956 (4), [1024x4096] 1131 vs 996
    // (4); [3072x1024] and the 57k-token square stay on the 256x128 kernel.  One workgroup per CU: splits give 256-512 workgroups.
    if (M >= 40000 && x.rpb == 0 && (N % 256) == 0 && (K % 256) == 0) {
      const long t256 = (long)(N / 256) * (K / 256);
      const bool long_tokens = M >= 150000;
      int pp_split = 0;
      if (t256 == 16 && long_tokens) pp_split = 16;
      else if (t256 == 64) pp_split = (long_tokens && N > K) ? 8 : 4;
      // round 4 (profiles/r04_wgrad_sweep.txt): the cross-attention key|value gradient [2048 x 1024] over the 192k encoder tokens, never swept
      // before: ping-pong split 8 = 0.687 ms (1173 TFLOP/s) vs 0.754 ms (1068) for the best 256x128 split; [3072 x 1024] stays (1.055 vs 1.081)
      else if (t256 == 32 && long_tokens) pp_split = 8;
      if (pp_split) {
        g.atomic_on_pp = 1;
        g.split_k = pp_split;
      }
    }
    return launch_gemm(g, st);
  }
  // ---- side stream (decoder backward of a span step) ----------------------------------------------------------------------------
  // The decoder-side GEMMs of a span step run over R ~ 18.7k rows: 292 tiles of 256 x 256 for an N = 1024 output = 1.14 rounds over the 256
  // CUs, the second round 14 % full.  A weight gradient and the data gradient launched after it are independent (both read dy), so the
  // weight gradients go to a second, lowest-priority stream whose workgroups take the CUs the main stream's tails leave idle; the main
  // stream waits for them (join_side) before the LayerNorm backward that ends each section of block_bwd -- the next kernel that may
  // overwrite something a weight gradient reads -- so the per-block events (DDP buckets) still mean "this block's gradients are complete".
  // The encoder-sized GEMMs of the cross-attention key|value side (the projection of xa in the forward -- it depends on the encoder output
  // only, so all L_dec of them are issued when the decoder starts; its weight gradient and d(xa) in the backward) run on a second side
  // stream the same way: short workgroups by the thousand, the filler for every tail of the decoder's own launches.
  struct OnStream {  // launches of this scope go to `to`
    hipStream_t& ref;
    hipStream_t keep;
    int lane;  // (bench.py's per-launch GEMM statistics keep side-stream spans -- queueing times -- apart from main-stream kernel times)
    OnStream(hipStream_t& r, hipStream_t to) : ref(r), keep(r), lane(gemm_profile_lane(to != r ? 1 : -1)) { ref = to; }
    ~OnStream() {
      ref = keep;
      gemm_profile_lane(lane);
    }
  };
  int side_mode = 0;  // bit 0: R-row weight gradients, bit 1: forward key|value projections, bit 2: backward key|value gradients
  bool side_pending = false, big_pending = false;
  LaneScope lane;  // (decoder_fwd tags the main stream "[shared]" while side-stream filler is in flight)
  // the side streams have drained: what follows has the chip to itself (the encoder's 192k-row GEMMs fill it on their own)
  void side_end() {
    side_mode = 0;
    gemm_profile_lane(lane.entry);
  }
  int side_begin(int mode) {
    oasr_ctx::Side& sd = c->side;
    if (!sd.stream) {
      // built into a local and published only when every call has succeeded: a failure half way must not leave a non-null stream
      // beside null events for the next step to trip over (whatever was created is destroyed again)
      oasr_ctx::Side nw;
      nw.kv_ready.assign((size_t)c->L_dec, nullptr);
      auto build = [&]() -> int {
        int least = 0, greatest = 0;
        OASR_CHECK_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        OASR_CHECK_HIP(hipStreamCreateWithPriority(&nw.stream, hipStreamNonBlocking, least));
        OASR_CHECK_HIP(hipStreamCreateWithPriority(&nw.big, hipStreamNonBlocking, least));
        for (hipEvent_t& e : nw.fork) OASR_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        for (hipEvent_t& e : nw.join) OASR_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        for (hipEvent_t& e : nw.kv_ready) OASR_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        return OASR_OK;
      };
      if (const int rc = build()) {
        for (hipEvent_t e : nw.fork) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : nw.join) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : nw.kv_ready) if (e) (void)hipEventDestroy(e);
        if (nw.stream) (void)hipStreamDestroy(nw.stream);
        if (nw.big) (void)hipStreamDestroy(nw.big);
        return rc;
      }
      sd = nw;
    }
    side_mode = mode;
    return OASR_OK;
  }
  // everything launched on `st` so far happens before whatever is launched on `to` next
  int fork_to(hipStream_t to) {
    oasr_ctx::Side& sd = c->side;
    hipEvent_t e = sd.fork[sd.nf++ & 3];
    OASR_CHECK_HIP(hipEventRecord(e, st));
    OASR_CHECK_HIP(hipStreamWaitEvent(to, e, 0));
    return OASR_OK;
  }
  int join_from(hipStream_t from) {
    oasr_ctx::Side& sd = c->side;
    hipEvent_t e = sd.join[sd.nj++ & 3];
    OASR_CHECK_HIP(hipEventRecord(e, from));
    OASR_CHECK_HIP(hipStreamWaitEvent(st, e, 0));
    return OASR_OK;
  }
  int wgrad_side(const T* dy, long ldy, long M, int N, const View& x, int K, float* dW, long ldw) {
    if (!(side_mode & 1)) return wgrad(dy, ldy, M, N, x, K, dW, ldw);
    RC(fork_to(c->side.stream));
    OnStream on(st, c->side.stream);
    side_pending = true;
    return wgrad(dy, ldy, M, N, x, K, dW, ldw);
  }
  int join_side() {
    if (!side_pending) return OASR_OK;
    side_pending = false;
    return join_from(c->side.stream);
  }
  int join_big() {
    if (!big_pending) return OASR_OK;
    big_pending = false;
    return join_from(c->side.big);
  }

  int attn_args(Attn& a, const AttnSave& s, bool cross, long Tq, long Tk, bool causal) {
    const int d = c->d;
    memset(&a, 0, sizeof(a));
    if (!cross) {
      a.q = s.qkv;
      a.k = s.qkv + d;
      a.v = s.qkv + 2 * d;
      a.ldq = a.ldk = a.ldv = 3 * d;
      a.bsq = a.bsk = a.bsv = Tq * 3 * d;
    } else {
      a.q = s.qkv;
      a.ldq = d;
      a.bsq = Tq * d;
      a.k = s.kv;
      a.v = s.kv + d;
      a.ldk = a.ldv = 2 * d;
      a.bsk = a.bsv = Tk * 2 * d;
    }
    a.o = s.o;
    a.ldo = d;
    a.bso = Tq * d;
    a.lse = s.lse;
    a.o_lo = s.o_lo;
    a.kv_len = causal ? text_len : nullptr;
    a.B = B;
    a.H = c->H;
    a.Tq = (int)Tq;
    a.Tk = (int)Tk;
    a.causal = causal ? 1 : 0;
    if (dec_rows && (causal || cross)) {  // a decoder attention of a span-limited step: chunked query rows (+ key rows for self-attention)
      a.q_rows = dec_rows;
      a.k_rows = cross ? nullptr : dec_rows;
      if (dec_rows_fwd) a.q_span = dec_span;  // (the backward sets it itself)
      a.qblk128 = dec_blk128;  // (used by the launches that carry q_span: the blocks past the span are the ones they do not compute)
      a.qblk256 = dec_blk256;
      a.n128 = dec_n128;
      a.n256 = dec_n256;
    }
    return OASR_OK;
  }

  int kv_proj(const BlockP& bp, BlockSave& s, const T* xa) {
    const int d = c->d;
    return linear(xa, (long)B * c->Te, d, c->template Wt<T>(bp.cattn.kw), 2 * d, c->aux(bp.cattn.fused_bias) + d, 0, nullptr, s.ca.kv, nullptr);
  }
  int block_fwd(const BlockP& bp, BlockSave& s, const T* x_in, long M, long Tq, const T* xa, bool causal, hipEvent_t kv_ready = nullptr) {
    const int d = c->d;
    s.x_in = const_cast<T*>(x_in);
    RC(launch_layernorm_fwd(x_in, c->P(bp.attn_ln_w), c->P(bp.attn_ln_b), s.sa.ln, s.sa.mean, s.sa.rstd, M, d, st));
    RC(linear(s.sa.ln, M, d, c->template Wt<T>(bp.attn.qw), 3 * d, c->aux(bp.attn.fused_bias), 0, nullptr, s.sa.qkv, nullptr));
    Attn a;
    attn_args(a, s.sa, false, Tq, Tq, causal);
    RC(launch_attention_fwd(a, st));
    RC(linear(s.sa.o, M, d, c->template Wt<T>(bp.attn.ow), d, c->P(bp.attn.ob), 0, x_in, s.x_mid, nullptr));
    const T* xm = s.x_mid;
    if (bp.cross) {
      RC(launch_layernorm_fwd(xm, c->P(bp.cln_w), c->P(bp.cln_b), s.ca.ln, s.ca.mean, s.ca.rstd, M, d, st));
      RC(linear(s.ca.ln, M, d, c->template Wt<T>(bp.cattn.qw), d, c->P(bp.cattn.qb), 0, nullptr, s.ca.qkv, nullptr));
      if (kv_ready)  // (decoder_fwd issued this layer's key|value projection on the side stream)
        OASR_CHECK_HIP(hipStreamWaitEvent(st, kv_ready, 0));
      else
        RC(kv_proj(bp, s, xa));
      attn_args(a, s.ca, true, Tq, c->Te, false);
      RC(launch_attention_fwd(a, st));
      RC(linear(s.ca.o, M, d, c->template Wt<T>(bp.cattn.ow), d, c->P(bp.cattn.ob), 0, xm, s.x_mid2, nullptr));
      xm = s.x_mid2;
    }
    RC(launch_layernorm_fwd(xm, c->P(bp.mlp_ln_w), c->P(bp.mlp_ln_b), s.ln2, s.mean2, s.rstd2, M, d, st));
    RC(linear(s.ln2, M, d, c->template Wt<T>(bp.w1), 4 * d, c->P(bp.b1), train ? 2 : 1, nullptr, s.hg, train ? s.u : nullptr));
    RC(linear(s.hg, M, 4 * d, c->template Wt<T>(bp.w2), d, c->P(bp.b2), 0, xm, s.x_out, nullptr));
    return OASR_OK;
  }

  View conv1_view(const T* mel_tm) const {
    const int nm = c->dims.n_mels;
    return View{mel_tm, nm, c->T1, (long)c->T1 * nm, nm, 3 * nm, 2 * nm};
  }
  View conv2_view(const T* h1) const {
    const int d = c->d;
    return View{h1, 2L * d, c->Te, (long)c->T1 * d, d, 3 * d, 3 * d};
  }

  int encoder_fwd(Plan& p, const float* mel) {
    const int d = c->d;
    const long M1 = (long)B * c->T1, Me = (long)B * c->Te;
    RC(launch_mel_to_time_major(mel, p.mel_tm, B, c->dims.n_mels, c->T1, st, mel_clip_max));
    // Both convolutions run on the direct-to-LDS kernels: the im2col matrix is the input itself read as a PLAIN matrix of
    // overlapping rows (row stride = conv stride * C) that starts one time row before the buffer.  That view is exact
    // except at sample boundaries -- window (b, 0) sees the previous sample's last row (or the zeroed guard row) where
    // the conv pads with zeros, and for conv1 window (b, T1-1) sees the next sample's first row -- so those 2B (conv1) /
    // B (conv2) output rows are recomputed afterwards by a small GEMM over one-row-per-sample window views whose
    // padding IS an out-of-range predicate (OperandView with rpb = 1).
    const int nm = c->dims.n_mels;
    OASR_CHECK_HIP(hipMemsetAsync(p.mel_tm - 256, 0, 256 * sizeof(T), st));
    OASR_CHECK_HIP(hipMemsetAsync(p.mel_tm + M1 * nm, 0, 256 * sizeof(T), st));
    OASR_CHECK_HIP(hipMemsetAsync(p.h1 - d, 0, (size_t)d * sizeof(T), st));
    for (int pass = 0; pass < 3; ++pass) {  // 0: all rows through the plain view; 1: rows (b, 0); 2: rows (b, T1-1)
      Gemm g = gemm_defaults_t<T>();
      long row_off = 0;
      if (pass == 0) {
        g.A = plain_view(p.mel_tm - nm, nm);
        g.M = (int)M1;
        g.ldc = d;
      } else {
        row_off = pass == 1 ? 0 : c->T1 - 1;
        g.A = pass == 1 ? View{p.mel_tm, nm, 1, (long)c->T1 * nm, nm, 3 * nm, 3 * nm}
                        : View{p.mel_tm + (long)(c->T1 - 2) * nm, nm, 1, (long)c->T1 * nm, 0, 3 * nm, 2 * nm};
        g.M = B;
        g.ldc = (long)c->T1 * d;
      }
      g.B = plain_view(c->template w1p<T>(), 256);
      g.N = d;
      g.K = 256;
      g.bias = c->P(c->conv1_b);
      g.act = 1;
      g.out = p.h1 + row_off * d;
      g.out_pre = p.u1 + row_off * d;
      RC(launch_gemm(g, st));
    }
    for (int pass = 0; pass < 2; ++pass) {  // 0: all rows; 1: rows (b, 0)
      Gemm g = gemm_defaults_t<T>();
      if (pass == 0) {
        g.A = plain_view(p.h1 - d, 2L * d);
        g.M = (int)Me;
        g.ldc = d;
        g.pos_period = c->Te;
      } else {
        g.A = View{p.h1, 2L * d, 1, (long)c->T1 * d, d, 3 * d, 3 * d};
        g.M = B;
        g.ldc = (long)c->Te * d;
        g.pos_period = 1;  // every recomputed row is position 0
      }
      g.B = plain_view(c->template w2p<T>(), 3 * d);
      g.N = d;
      g.K = 3 * d;
      g.bias = c->P(c->conv2_b);
      g.act = 1;
      g.pos = c->enc_pos;
      g.out = p.x0;
      g.out_pre = p.u2;
      RC(launch_gemm(g, st));
    }
    const T* x = p.x0;
    for (int i = 0; i < c->L_enc; ++i) {
      RC(block_fwd(c->enc[i], p.enc[i], x, Me, c->Te, nullptr, false));
      x = p.enc[i].x_out;
    }
    RC(launch_layernorm_fwd(x, c->P(c->enc_lnp_w), c->P(c->enc_lnp_b), p.xa, p.mean_p, p.rstd_p, Me, d, st));
    return OASR_OK;
  }

  int decoder_fwd(Plan& p, const int64_t* tokens, bool last_only = false) {
    const int d = c->d;
    const long Md = dec_rows_fwd ? dec_rows_fwd : (long)B * S;  // token rows the row-wise kernels run over
    RC(launch_embedding_fwd(tokens, c->P(c->tok_emb), c->P(c->dec_pos), p.dx0, B, S, d, c->V, st, dec_rows));
    const bool kv_side = (side_mode & 2) && train;  // (training plan: every layer has its own key|value buffer)
    // launch statistics: from here until the backward's last join (side_end) the main stream shares the chip with side-stream filler (lane 2, "[shared]")
    if (side_mode && train) gemm_profile_lane(2);
    if (kv_side) {
      RC(fork_to(c->side.big));  // p.xa is complete
      OnStream on(st, c->side.big);
      for (int i = 0; i < c->L_dec; ++i) {
        RC(kv_proj(c->dec[i], p.dec[i], p.xa));
        OASR_CHECK_HIP(hipEventRecord(c->side.kv_ready[i], st));
      }
    }
    const T* x = p.dx0;
    for (int i = 0; i < c->L_dec; ++i) {
      RC(block_fwd(c->dec[i], p.dec[i], x, Md, S, p.xa, true, kv_side ? c->side.kv_ready[i] : nullptr));
      x = p.dec[i].x_out;
    }
    RC(launch_layernorm_fwd(x, c->P(c->dec_ln_w), c->P(c->dec_ln_b), p.lnf, p.mean_f, p.rstd_f, Md, d, st));
    if (last_only) {  // greedy decoding only needs position S-1 of every sequence: M = B rows, row stride S*d
      Gemm g = gemm_defaults_t<T>();
      g.A = plain_view(p.lnf + (long)(S - 1) * d, (long)S * d);
      g.B = plain_view(c->template Wt<T>(c->tok_emb), d);
      g.M = B;
      g.N = c->Vp;
      g.K = d;
      g.out = p.logits;
      g.ldc = c->Vp;
      return launch_gemm(g, st);
    }
    RC(linear(p.lnf, Md, d, c->template Wt<T>(c->tok_emb), c->Vp, nullptr, 0, nullptr, p.logits, nullptr));
    return OASR_OK;
  }

  int record(void** ev, int idx) {
    if (ev && ev[idx]) OASR_CHECK_HIP(hipEventRecord((hipEvent_t)ev[idx], st));
    return OASR_OK;
  }

  // dx_out (grad of the block output) -> returns grad of the block input in *dx_in_out (ping-pong ga/gb)
  // Bias gradients of Linears that write into the residual stream (mlp.2, attn.out, cross_attn.out) are column sums of a
  // residual-stream gradient, and every such gradient is produced by a LayerNorm backward -> that kernel accumulates
  // them (its `dsum` output).  The caller's LN backward already filled this block's mlp.2.bias gradient from dx_out;
  // `dsum_next` is the bias gradient the produced dx_in belongs to (previous block's mlp.2.bias, or null).
  // Frozen parameters (oasr_ctx::Prune): every weight / bias / LayerNorm gradient of a frozen tensor is left out (null outputs, skipped
  // launches), and a section's data path runs only if something it feeds still needs a gradient -- `need_dx_in` (the block's input
  // gradient: a trainable tensor below it) or `need_xa` (d(xa): a trainable encoder tensor).  With every tensor trainable both are true
  // and every launch is the one of the plain step.
  // A weight gradient over consecutive [rows x K] tensors of the arena that one GEMM fills (q|k|v, cross k|v): one launch when all are
  // trainable, one per trainable tensor otherwise (columns j*rows.. of dy).
  // An adapted tensor's gradient goes to its scratch (Gw), so it always gets a launch of its own.
  int wgrad_parts(const T* dy, long ldy, long M, const View& x, int K, const int64_t* offs, int n, int rows) {
    int ntr = 0;
    for (int j = 0; j < n; ++j) ntr += (c->tr(offs[j]) && c->lora_at(offs[j]) < 0) ? 1 : 0;
    if (ntr == n) return wgrad_side(dy, ldy, M, n * rows, x, K, c->G(offs[0]), K);
    for (int j = 0; j < n; ++j)
      if (c->wn(offs[j])) RC(wgrad_side(dy + (long)j * rows, ldy, M, rows, x, K, Gw(offs[j]), K));
    return OASR_OK;
  }
  int block_bwd(const BlockP& bp, const BlockSave& s, Plan& p, const T* dx_out, T* scratch_a, T* scratch_b, long M,
                long Tq, bool causal, bool first_cross, float* dsum_next, const T** dx_in, bool need_dx_in = true, bool need_xa = true) {
    const int d = c->d;
    const T* xm = bp.cross ? s.x_mid2 : s.x_mid;
    auto any = [&](std::initializer_list<int64_t> offs) {  // (weights: adapted ones count -- their adapters need dW)
      for (int64_t o : offs)
        if (c->wn(o)) return true;
      return false;
    };
    const AttnP& sa_p = bp.attn;
    const bool sa_need = need_dx_in || any({sa_p.qw, sa_p.kw, sa_p.vw, sa_p.ow, sa_p.qb, sa_p.vb, sa_p.ob, bp.attn_ln_w, bp.attn_ln_b});
    const bool ca_need = bp.cross && (sa_need || need_xa || any({bp.cattn.qw, bp.cattn.kw, bp.cattn.vw, bp.cattn.ow, bp.cattn.qb, bp.cattn.vb,
                                                                  bp.cattn.ob, bp.cln_w, bp.cln_b}));
    const bool mlp_need = (bp.cross ? ca_need : sa_need) || any({bp.w1, bp.b1, bp.mlp_ln_w, bp.mlp_ln_b});
    *dx_in = nullptr;
    // ---- MLP -----------------------------------------------------------------------------------------------
    if (c->wn(bp.w2)) RC(wgrad_side(dx_out, d, M, d, plain_view(s.hg, 4 * d), 4 * d, Gw(bp.w2), 4 * d));
    if (!mlp_need) return join_side();
    RC(dgrad(dx_out, M, d, c->template Wt<T>(bp.w2), 4 * d, s.u, nullptr, p.gu, c->Gt(bp.b1), true));  // s.u = GELU'(u); + fused mlp.0.bias gradient
    if (c->wn(bp.w1)) RC(wgrad_side(p.gu, 4 * d, M, 4 * d, plain_view(s.ln2, d), d, Gw(bp.w1), d));
    RC(dgrad(p.gu, M, 4 * d, c->template Wt<T>(bp.w1), d, nullptr, nullptr, p.gln));
    RC(join_side());
    RC(launch_layernorm_bwd(p.gln, xm, c->P(bp.mlp_ln_w), s.mean2, s.rstd2, dx_out, scratch_a, c->Gt(bp.mlp_ln_w), c->Gt(bp.mlp_ln_b),
                            c->Gt(bp.cross ? bp.cattn.ob : bp.attn.ob), M, d, st));
    const T* dx = scratch_a;
    T* nxt = scratch_b;
    // ---- cross attention ---------------------------------------------------------------------------------------
    if (bp.cross) {
      const long Mkv = (long)B * c->Te;
      if (c->wn(bp.cattn.ow)) RC(wgrad_side(dx, d, M, d, plain_view(s.ca.o, d), d, Gw(bp.cattn.ow), d));
      if (!ca_need) return join_side();
      RC(dgrad(dx, M, d, c->template Wt<T>(bp.cattn.ow), d, nullptr, nullptr, p.go));
      Attn a;
      attn_args(a, s.ca, true, Tq, c->Te, false);
      a.d_o = p.go;
      a.delta = p.delta;
      a.dq = p.gq;
      a.dk = p.gkv;
      a.dv = p.gkv + d;
      a.dq_colsum = c->Gt(bp.cattn.qb);  // query / value bias gradients = column sums of dq / dv, fused into the store epilogues
      a.dv_colsum = c->Gt(bp.cattn.vb);
      a.colsum_scratch = p.cs_scratch;
      // decoder positions the loss ignores have d_o == 0 exactly (three quarters of the 448 on the synthetic lengths): the kernels
      // find those 64-position tiles themselves and skip them (span-limited step: the span says where they are, and the rows past
      // it are not even written)
      a.qtile_flags = dec_span ? nullptr : p.qtile_flags;
      a.q_span = dec_span;
      RC(join_big());  // (the previous layer's key|value gradients still read p.gkv)
      RC(launch_attention_bwd(a, st));
      if (c->wn(bp.cattn.qw)) RC(wgrad_side(p.gq, d, M, d, plain_view(s.ca.ln, d), d, Gw(bp.cattn.qw), d));
      const bool kv_tr = any({bp.cattn.kw, bp.cattn.vw});
      if (kv_tr || need_xa) {
        const bool big = (side_mode & 4) != 0;
        if (big) {
          RC(fork_to(c->side.big));
          big_pending = true;
        }
        OnStream on(st, big ? c->side.big : st);
        if (kv_tr) {
          if (c->tr(bp.cattn.kw) && c->tr(bp.cattn.vw) && c->lora_at(bp.cattn.kw) < 0 && c->lora_at(bp.cattn.vw) < 0) {
            RC(wgrad(p.gkv, 2 * d, Mkv, 2 * d, plain_view(p.xa, d), d, c->G(bp.cattn.kw), d));
          } else {
            const int64_t kv[2] = {bp.cattn.kw, bp.cattn.vw};
            for (int j = 0; j < 2; ++j)
              if (c->wn(kv[j])) RC(wgrad(p.gkv + (long)j * d, 2 * d, Mkv, d, plain_view(p.xa, d), d, Gw(kv[j]), d));
          }
        }
        // d(xa) accumulates over the decoder layers (bf16, like autograd's accumulation into xa.grad)
        if (need_xa) RC(dgrad(p.gkv, Mkv, 2 * d, c->template Wt<T>(bp.cattn.kw), d, nullptr, first_cross ? nullptr : p.gxa, p.gxa));
      }
      if (!sa_need && !any({bp.cln_w, bp.cln_b})) return join_side();
      RC(dgrad(p.gq, M, d, c->template Wt<T>(bp.cattn.qw), d, nullptr, nullptr, p.gln));
      RC(join_side());
      RC(launch_layernorm_bwd(p.gln, s.x_mid, c->P(bp.cln_w), s.ca.mean, s.ca.rstd, dx, nxt, c->Gt(bp.cln_w), c->Gt(bp.cln_b),
                              c->Gt(bp.attn.ob), M, d, st));
      const T* t = dx;
      dx = nxt;
      nxt = const_cast<T*>(t);
    }
    // ---- self attention ----------------------------------------------------------------------------------------
    if (!sa_need) return join_side();
    if (c->wn(bp.attn.ow)) RC(wgrad_side(dx, d, M, d, plain_view(s.sa.o, d), d, Gw(bp.attn.ow), d));
    RC(dgrad(dx, M, d, c->template Wt<T>(bp.attn.ow), d, nullptr, nullptr, p.go));
    Attn a;
    attn_args(a, s.sa, false, Tq, Tq, causal);
    a.d_o = p.go;
    a.delta = p.delta;
    a.dq = p.gqkv;
    a.dk = p.gqkv + d;
    a.dv = p.gqkv + 2 * d;
    a.dq_colsum = c->Gt(bp.attn.qb);
    a.dv_colsum = c->Gt(bp.attn.vb);
    a.colsum_scratch = p.cs_scratch;
    a.qtile_flags = (causal && !dec_span) ? p.qtile_flags : nullptr;  // (decoder blocks only: an encoder block's d_o has no zero rows)
    a.q_span = causal ? dec_span : nullptr;
    RC(launch_attention_bwd(a, st));
    {
      const int64_t qkv[3] = {sa_p.qw, sa_p.kw, sa_p.vw};
      RC(wgrad_parts(p.gqkv, 3 * d, M, plain_view(s.sa.ln, d), d, qkv, 3, d));
    }
    if (!need_dx_in && !any({bp.attn_ln_w, bp.attn_ln_b})) return join_side();
    RC(dgrad(p.gqkv, M, 3 * d, c->template Wt<T>(bp.attn.qw), d, nullptr, nullptr, p.gln));
    RC(join_side());
    RC(launch_layernorm_bwd(p.gln, s.x_in, c->P(bp.attn_ln_w), s.sa.mean, s.sa.rstd, dx, nxt, c->Gt(bp.attn_ln_w), c->Gt(bp.attn_ln_b),
                            dsum_next, M, d, st));
    *dx_in = nxt;
    return OASR_OK;
  }
};

};  // struct Engine

// One call's workspace plan and runner.  A training plan's runner saves GELU'(u), sums bias gradients through the plan's scratch and sends
// adapted weights' gradients to the plan's (Runner::train / cs_scratch / lora_dw).  A null workspace is a dry run: A.cur is the plan's size.
template <typename T>
struct Step {
  Arena A;
  typename Engine<T>::Plan p;
  typename Engine<T>::Runner r;
  Step(const oasr_ctx* c, void* workspace, size_t bytes, void* stream, int B, int S, const int32_t* text_len, bool train, int stage = STAGE_ALL)
      : A(workspace, bytes), r{c, (hipStream_t)stream, B, S, text_len} {
    Engine<T>::make_plan(c, A, p, B, S, train, stage);
    if (train) {
      r.train = true;
      r.cs_scratch = p.gemm_cs_scratch;
      r.lora_dw = p.lora_dw;
    }
  }
};

// xa [B, n_audio_ctx, d] in the compute dtype, into or out of a plan
template <typename T>
int copy_xa(const oasr_ctx* c, void* dst, const void* src, int B, hipStream_t st) {
  OASR_CHECK_HIP(hipMemcpyAsync(dst, src, (size_t)B * c->Te * c->d * sizeof(T), hipMemcpyDeviceToDevice, st));
  return OASR_OK;
}

}  // namespace

// the two stream-gradient buffers (of p.ga / gb / gc) that are not `cur`
template <typename T>
static void other_two(typename Engine<T>::Plan& p, const T* cur, T** a, T** b) {
  T* all[3] = {p.ga, p.gb, p.gc};
  int n = 0;
  T* o[2] = {nullptr, nullptr};
  for (int j = 0; j < 3; ++j)
    if (all[j] != cur && n < 2) o[n++] = all[j];
  *a = o[0];
  *b = o[1];
}

// The backward half of a training micro-step: p.logits holds d(loss)/d(logits) (bf16 engine: bf16 [Md, Vp]) on entry -- written in
// place by the fused cross-entropy (oasr_train_step) or converted from the caller's fp32 tensor (oasr_train_bwd, the
// torch.autograd path) -- and every saved activation of the forward is still in the workspace.  It runs in two halves (train_backward
// below calls both).  backward_decoder starts from p.logits and ends at the token / positional embeddings; with `xa_grad` it
// leaves d(xa) in p.gxa.  backward_encoder starts from d(xa) = `gxa` and ends at the conv stem; with `dmel` it also writes d(mel) (fp32
// [B, n_mels, T1]: the conv1 data gradient, which no parameter needs).  A requested input gradient forces the data gradient it needs through
// every block of its stage, whatever the trainability mask prunes (the staged autograd entries, oasr_train_encode_bwd / _decode_bwd); the
// fused step asks for d(xa) exactly when an encoder tensor needs a gradient, and never for d(mel).
template <typename T>
static int backward_decoder(oasr_ctx* c, typename Engine<T>::Runner& r, typename Engine<T>::Plan& p, const int64_t* tokens, int B, int S,
                            void** ev, int& seg, bool xa_grad) {
  const int d = c->d;
  // Md: the decoder's token rows the backward runs over -- all B*S, or (supervised-span step) the leading rows that hold every
  // position able to carry gradient; the rows behind them are never read or written by the backward
  const long Md = r.dec_rows_bwd ? r.dec_rows_bwd : (long)B * S;
  hipStream_t st = r.st;
  const oasr_ctx::Prune& pr = c->pr;
  // tied logits: dE += dlogits^T . lnf ; d(lnf) = dlogits . E
  // (V = n_vocab + 1 is odd: the direct-to-LDS kernel wants a multiple of 8 rows, so the pad class gets its own 1-row GEMM)
  if (c->tr(c->tok_emb)) {
    const int v8 = c->V & ~7;
    RC(r.wgrad(p.logits, c->Vp, Md, v8, plain_view(p.lnf, d), d, c->G(c->tok_emb), d));
    if (v8 < c->V) RC(r.wgrad(p.logits + v8, c->Vp, Md, c->V - v8, plain_view(p.lnf, d), d, c->G(c->tok_emb) + (long)v8 * d, d));
  }
  RC(r.dgrad(p.logits, Md, c->Vp, c->template Wt<T>(c->tok_emb), d, nullptr, nullptr, p.gln));
  const T* x_last = c->L_dec ? p.dec[c->L_dec - 1].x_out : p.dx0;
  RC(launch_layernorm_bwd(p.gln, x_last, c->P(c->dec_ln_w), p.mean_f, p.rstd_f, nullptr, p.ga, c->Gt(c->dec_ln_w), c->Gt(c->dec_ln_b),
                          c->L_dec ? c->Gt(c->dec[c->L_dec - 1].b2) : nullptr, Md, d, st));
  RC(r.record(ev, seg++));
  const T* dx = p.ga;
  for (int i = c->L_dec - 1; i >= 0; --i) {
    // the gradient of block i's input: for a trainable tensor below it, or for a lower block's d(xa)
    const bool need_in = pr.all || pr.dec_below[i] || (i > 0 && xa_grad);
    if (pr.all || pr.dec_blk[i] || need_in || xa_grad) {
      T *sa, *sb;
      other_two<T>(p, dx, &sa, &sb);
      const T* dx_in = nullptr;
      RC(r.block_bwd(c->dec[i], p.dec[i], p, dx, sa, sb, Md, S, true, i == c->L_dec - 1, i > 0 ? c->Gt(c->dec[i - 1].b2) : nullptr, &dx_in,
                     need_in, xa_grad));
      dx = dx_in;
    }
    // the block's event says "every gradient of this block is complete" (the DDP reducer sends the bucket on it): that includes the
    // key|value weight gradient on the side stream (bit 3, experiments without events: leave it in flight until the next block needs p.gkv)
    if (ev || !(r.side_mode & 8)) RC(r.join_big());
    RC(r.record(ev, seg++));
  }
  RC(r.join_side());
  RC(r.join_big());
  r.side_end();
  if (c->tr(c->tok_emb) || c->tr(c->dec_pos))
    RC(launch_embedding_bwd(tokens, dx, c->Gt(c->tok_emb), c->Gt(c->dec_pos), B, S, d, PAD_ID, c->V, st, r.dec_rows, r.dec_span));
  RC(r.record(ev, seg++));  // decoder.positional_embedding
  RC(r.record(ev, seg++));  // token embedding (arena tail)
  if (xa_grad && c->L_dec == 0) OASR_CHECK_HIP(hipMemsetAsync(p.gxa, 0, (size_t)B * c->Te * d * sizeof(T), st));
  return OASR_OK;
}

template <typename T>
static int backward_encoder(oasr_ctx* c, typename Engine<T>::Runner& r, typename Engine<T>::Plan& p, const T* gxa, int B, void** ev, int& seg,
                            float* dmel) {
  const int d = c->d;
  const long Me = (long)B * c->Te, M1 = (long)B * c->T1;
  hipStream_t st = r.st;
  const oasr_ctx::Prune& pr = c->pr;
  if (!pr.enc_any && !dmel) {  // nothing in the encoder is trainable and no d(mel): neither d(xa) (skipped in the decoder blocks) nor anything below it
    for (int i = 0; i < c->L_enc + 2; ++i) RC(r.record(ev, seg++));  // ln_post, the blocks, the conv stem
    return OASR_OK;
  }
  const T* xe_last = c->L_enc ? p.enc[c->L_enc - 1].x_out : p.x0;
  const bool enc_top_in = pr.all || pr.enc_in[c->L_enc] || dmel;
  if (enc_top_in || c->tr(c->enc_lnp_w) || c->tr(c->enc_lnp_b))
    RC(launch_layernorm_bwd(gxa, xe_last, c->P(c->enc_lnp_w), p.mean_p, p.rstd_p, nullptr, p.ga, c->Gt(c->enc_lnp_w), c->Gt(c->enc_lnp_b),
                            c->L_enc ? c->Gt(c->enc[c->L_enc - 1].b2) : nullptr, Me, d, st));
  RC(r.record(ev, seg++));
  const T* dx = p.ga;
  for (int i = c->L_enc - 1; i >= 0; --i) {
    if (pr.all || pr.enc_blk[i] || pr.enc_in[i] || dmel) {
      T *sa, *sb;
      other_two<T>(p, dx, &sa, &sb);
      const T* dx_in = nullptr;
      RC(r.block_bwd(c->enc[i], p.enc[i], p, dx, sa, sb, Me, c->Te, false, false, i > 0 ? c->Gt(c->enc[i - 1].b2) : nullptr, &dx_in,
                     pr.all || pr.enc_in[i] || dmel, false));
      dx = dx_in;
    }
    RC(r.record(ev, seg++));
  }
  // conv stem: x0 = gelu(u2) + pos ; u2 = conv2(h1) ; h1 = gelu(u1) ; u1 = conv1(mel)
  if (pr.all || c->tr(c->conv2_w) || c->tr(c->conv2_b) || pr.conv1 || dmel) {
    RC(launch_dgelu_mul(dx, p.u2, p.gln, Me * d, st));  // gln = d(u2)
    if (c->tr(c->conv2_w)) {
      OASR_CHECK_HIP(hipMemsetAsync(p.tmp_w2p, 0, (size_t)d * 3 * d * 4, st));
      // conv2 weight gradient on the direct-to-LDS kernel: the im2col matrix [B*1500][3d] is h1 itself read as overlapping
      // rows of 3d elements at stride 2d from h1 - d (per-sample stride 3000*d == 1500 rows * 2d, so the view is plain).
      // Only window (b, t = 0) is wrong in its first d elements (it sees the last row of sample b-1, or the zeroed guard row,
      // instead of the left zero padding); that rank-B term is subtracted by a second, tiny GEMM over the B first rows.
      RC(r.wgrad(p.gln, d, Me, d, plain_view(p.h1 - d, 2L * d), 3 * d, p.tmp_w2p, 3 * d));  // (guard row zeroed by the forward)
      {
        GemmArgsT<T> g = gemm_defaults_t<T>();
        g.A = plain_view(p.gln, (long)c->Te * d);          // dY rows (b, t = 0)
        g.ta = 1;
        g.B = plain_view(p.h1 - d, (long)c->T1 * d);       // what those windows wrongly saw as their first tap
        g.tb = 1;
        g.M = d;
        g.N = d;
        g.K = B;
        g.alpha = -1.0f;
        g.out_f32 = p.tmp_w2p;
        g.ldc32 = 3 * d;
        g.atomic = 1;
        RC(launch_gemm(g, st));
      }
      RC(launch_unpack_conv_grad(p.tmp_w2p, c->G(c->conv2_w), d, d, 3 * d, st));
    }
    if (c->tr(c->conv2_b)) RC(launch_colsum_accum(p.gln, d, Me, d, c->G(c->conv2_b), st));
  }
  if (pr.all || pr.conv1 || dmel) {  // the conv2 data gradient serves conv1 (and d(mel)) alone
    RC(r.dgrad(p.gln, Me, d, c->template w2p<T>(), 3 * d, nullptr, nullptr, p.gA2));
    RC(launch_conv2_col2im_dgelu(p.gA2, p.u1, p.gu, B, c->T1, d, st));  // gu = d(u1) [B*3000, d]
    if (c->tr(c->conv1_w)) {
      OASR_CHECK_HIP(hipMemsetAsync(p.tmp_w1p, 0, (size_t)d * 256 * 4, st));
      // conv1 weight gradient, same trick: windows of 3*n_mels (+ junk up to 256, whose gradient columns are never
      // unpacked) at stride n_mels from mel_tm - n_mels; the first tap of every (b, 0) and the last tap of every (b, T1-1)
      // see the neighbouring sample (or a zeroed guard row) instead of the zero padding -> two rank-B corrections.
      {
        const int nm = c->dims.n_mels;
        RC(r.wgrad(p.gu, d, M1, d, plain_view(p.mel_tm - nm, nm), 256, p.tmp_w1p, 256));  // (guard rows zeroed by the forward)
        for (int side = 0; side < 2; ++side) {
          GemmArgsT<T> g = gemm_defaults_t<T>();
          g.A = plain_view(p.gu + (side ? (long)(c->T1 - 1) * d : 0), (long)c->T1 * d);  // dU rows (b, 0) / (b, T1-1)
          g.ta = 1;
          g.B = plain_view(side ? p.mel_tm + (long)c->T1 * nm : p.mel_tm - nm, (long)c->T1 * nm);
          g.tb = 1;
          g.M = d;
          g.N = nm;
          g.K = B;
          g.alpha = -1.0f;
          g.out_f32 = p.tmp_w1p + (side ? 2 * nm : 0);
          g.ldc32 = 256;
          g.atomic = 1;
          RC(launch_gemm(g, st));
        }
      }
      RC(launch_unpack_conv_grad(p.tmp_w1p, c->G(c->conv1_w), d, c->dims.n_mels, 256, st));
    }
    if (c->tr(c->conv1_b)) RC(launch_colsum_accum(p.gu, d, M1, d, c->G(c->conv1_b), st));
    if (dmel) {
      // d(mel): the conv1 data gradient as columns dcol [B*T1, 256] = d(u1) . w1p (gA2 is free again), then folded back onto the mel
      // frames -- taps that fall into the zero padding or the neighbouring sample are dropped (conv_grad.hip).  The bf16 engine's cast of
      // mel to bf16 counts as the identity here, as autocast's cast does.
      RC(r.dgrad(p.gu, M1, d, c->template w1p<T>(), 256, nullptr, nullptr, p.gA2));
      RC(launch_conv1_col2im_mel(p.gA2, dmel, B, c->T1, c->dims.n_mels, st));
    }
  }
  RC(r.record(ev, seg++));
  return OASR_OK;
}

// adapter contexts: the adapted weights' gradients of THIS micro-batch go to workspace scratch (Runner::Gw; projected into the arena at the end)
template <typename T>
static int backward_begin(oasr_ctx* c, typename Engine<T>::Runner& r, typename Engine<T>::Plan& p) {
  if (!c->lora.empty()) OASR_CHECK_HIP(hipMemsetAsync(p.lora_dw, 0, (size_t)c->lora_dw_floats * 4, r.st));
  return OASR_OK;
}
// the last gradient segment of an adapter context: d lora_B = s * dW . lora_A^T, d lora_A = s * lora_B^T . dW (every dW is final here).
// A stage's backward projects the adapters of its own stage's weights only (the other stage's scratch was never written).
template <typename T>
static int backward_finish(oasr_ctx* c, typename Engine<T>::Runner& r, typename Engine<T>::Plan& p, void** ev, int seg, int stage) {
  if (!c->lora.empty()) {
    for (const oasr_ctx::Lora& L : c->lora) {
      const bool in_enc = L.w >= c->enc_lnp_w && L.w < c->stem_end;
      if ((stage == STAGE_ENC && !in_enc) || (stage == STAGE_DEC && in_enc)) continue;
      float *ga = c->Gt(L.a), *gb = c->Gt(L.b);
      if (ga || gb)
        RC(launch_lora_grad(p.lora_dw + L.dw, c->P(L.a), c->P(L.b), L.out, L.in, c->lora_r, c->lora_s, ga, gb, p.lora_part, r.st));
    }
    RC(r.record(ev, seg++));
  }
  if (stage == STAGE_ALL && seg != (int)c->segments.size()) {
    oasr_set_error("internal: segment count mismatch %d vs %zu", seg, c->segments.size());
    return OASR_ESTATE;
  }
  return OASR_OK;
}
// refusals shared by every backward entry.  The fused ones need a trainable tensor; a stage backward that returns an input gradient does not
// (saliency on a frozen model).
static int backward_check(const oasr_ctx* c, bool input_grad) {
  if (!c->lora.empty() && !c->mask_set) {
    oasr_set_error("oasr_train backward: a context with adapters needs oasr_set_trainable before the first backward");
    return OASR_ESTATE;
  }
  if (!c->pr.any && !input_grad) {
    oasr_set_error("oasr_train backward: no parameter is trainable (oasr_set_trainable mask is all zeros)");
    return OASR_ESTATE;
  }
  return OASR_OK;
}

template <typename T>
static int train_backward(oasr_ctx* c, typename Engine<T>::Runner& r, typename Engine<T>::Plan& p, const int64_t* tokens, int B, int S, void** ev) {
  // Frozen parameters (oasr_set_trainable, oasr_ctx::Prune): launches that only serve frozen tensors are left out, the data gradient
  // stops where nothing earlier in the forward is trainable.  Every segment event is still recorded (DDP buckets wait on them).
  RC(backward_check(c, false));
  RC(backward_begin<T>(c, r, p));
  int seg = 0;
  RC(backward_decoder<T>(c, r, p, tokens, B, S, ev, seg, c->pr.all || c->pr.enc_any));
  RC(backward_encoder<T>(c, r, p, p.gxa, B, ev, seg, nullptr));
  return backward_finish<T>(c, r, p, ev, seg, STAGE_ALL);
}

