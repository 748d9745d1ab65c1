// The forward schedule: one transformer block, the encoder (conv stem as GEMMs over overlapping-row views) and the decoder.
//
// Reference schedule being replaced: OLMoASR.forward (olmoasr/model.py:856-887) -> AudioEncoder.forward (:571-623)
// -> TextDecoder.forward (:688-775).
#pragma once
#include "engine_gemm.h"
#include "engine_plan.h"

namespace {

template <typename T>
struct Forward : GemmCalls<T> {
  typedef GemmCalls<T> G;
  typedef OperandViewT<T> View;
  typedef AttnArgsT<T> Attn;
  using G::c, G::st, G::side_mode, G::fork_to, G::linear, G::product;  // (names of a dependent base)
  int B, S;
  const int32_t* text_len;
  bool train = false;  // the training forward saves GELU'(u) in place of u (GemmArgs.act == 2)
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
  Forward(const oasr_ctx* c_, hipStream_t st_, int B_, int S_, const int32_t* text_len_) : G(c_, st_), B(B_), S(S_), text_len(text_len_) {}

  void attn_args(Attn& a, const AttnSave<T>& s, bool cross, long Tq, long Tk, bool causal) {
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
  }

  int kv_proj(const BlockP& bp, BlockSave<T>& s, const T* xa) {
    const int d = c->d;
    return linear(xa, (long)B * c->Te, d, c->template Wt<T>(bp.cattn.kw), 2 * d, c->aux(bp.cattn.fused_bias) + d, 0, nullptr, s.ca.kv, nullptr);
  }
  int block_fwd(const BlockP& bp, BlockSave<T>& s, const T* x_in, long M, long Tq, const T* xa, bool causal, hipEvent_t kv_ready = nullptr) {
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

  int encoder_fwd(Plan<T>& p, const float* mel) {
    const int d = c->d, nm = c->dims.n_mels, T1 = c->T1, Te = c->Te;
    const long M1 = (long)B * T1, Me = (long)B * Te;
    RC(launch_mel_to_time_major(mel, p.mel_tm, B, nm, T1, st, mel_clip_max));
    // Both convolutions run on the direct-to-LDS kernels: the im2col matrix is the input itself read as a PLAIN matrix of
    // overlapping rows (row stride = conv stride * C) that starts one time row before the buffer.  That view is exact
    // except at sample boundaries -- window (b, 0) sees the previous sample's last row (or the zeroed guard row) where
    // the conv pads with zeros, and for conv1 window (b, T1-1) sees the next sample's first row -- so those 2B (conv1) /
    // B (conv2) output rows are recomputed afterwards by a small GEMM over one-row-per-sample window views whose
    // padding IS an out-of-range predicate (OperandView with rpb = 1).
    OASR_CHECK_HIP(hipMemsetAsync(p.mel_tm - 256, 0, 256 * sizeof(T), st));
    OASR_CHECK_HIP(hipMemsetAsync(p.mel_tm + M1 * nm, 0, 256 * sizeof(T), st));
    OASR_CHECK_HIP(hipMemsetAsync(p.h1 - d, 0, (size_t)d * sizeof(T), st));
    // conv1 -- all rows through the plain view; rows (b, 0); rows (b, T1-1)
    const View mel_rows[3] = {plain_view(p.mel_tm - nm, nm), View{p.mel_tm, nm, 1, (long)T1 * nm, nm, 3 * nm, 3 * nm},
                              View{p.mel_tm + (long)(T1 - 2) * nm, nm, 1, (long)T1 * nm, 0, 3 * nm, 2 * nm}};
    for (int pass = 0; pass < 3; ++pass) {
      const long row_off = pass == 2 ? T1 - 1 : 0;
      RC(launch_gemm(product(mel_rows[pass], pass ? B : M1, 256, c->template w1p<T>(), d, c->P(c->conv1_b), 1, p.h1 + row_off * d,
                             p.u1 + row_off * d, pass ? (long)T1 * d : d),
                     st));
    }
    // conv2 + the sinusoids -- all rows; rows (b, 0), every one of them position 0
    const View h1_rows[2] = {plain_view(p.h1 - d, 2L * d), View{p.h1, 2L * d, 1, (long)T1 * d, d, 3 * d, 3 * d}};
    for (int pass = 0; pass < 2; ++pass) {
      auto g = product(h1_rows[pass], pass ? B : Me, 3 * d, c->template w2p<T>(), d, c->P(c->conv2_b), 1, p.x0, p.u2, pass ? (long)Te * d : d);
      g.pos = c->enc_pos;
      g.pos_period = pass ? 1 : Te;
      RC(launch_gemm(g, st));
    }
    const T* x = p.x0;
    for (int i = 0; i < c->L_enc; ++i) {
      RC(block_fwd(c->enc[i], p.enc[i], x, Me, Te, nullptr, false));
      x = p.enc[i].x_out;
    }
    RC(launch_layernorm_fwd(x, c->P(c->enc_lnp_w), c->P(c->enc_lnp_b), p.xa, p.mean_p, p.rstd_p, Me, d, st));
    return OASR_OK;
  }

  int decoder_fwd(Plan<T>& p, const int64_t* tokens, bool last_only = false) {
    const int d = c->d;
    const long Md = dec_rows_fwd ? dec_rows_fwd : (long)B * S;  // token rows the row-wise kernels run over
    RC(launch_embedding_fwd(tokens, c->P(c->tok_emb), c->P(c->dec_pos), p.dx0, B, S, d, c->V, st, dec_rows));
    const bool kv_side = (side_mode & SIDE_KV_FWD) && train;  // (training plan: every layer has its own key|value buffer)
    // launch statistics: from here until the backward's last join (side_end) the main stream shares the chip with side-stream filler (lane 2, "[shared]")
    if (side_mode && train) gemm_profile_lane(2);
    if (kv_side) {
      RC(fork_to(c->side.big));  // p.xa is complete
      SideStreams::OnStream on(st, c->side.big);
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
    const T* E = c->template Wt<T>(c->tok_emb);
    if (last_only)  // greedy decoding only needs position S-1 of every sequence: M = B rows, row stride S*d
      return launch_gemm(product(plain_view(p.lnf + (long)(S - 1) * d, (long)S * d), B, d, E, c->Vp, nullptr, 0, p.logits, nullptr, c->Vp), st);
    return linear(p.lnf, Md, d, E, c->Vp, nullptr, 0, nullptr, p.logits, nullptr);
  }
};

}  // namespace
