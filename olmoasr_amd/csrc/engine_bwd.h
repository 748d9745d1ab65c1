// The hand-written backward, layer by layer, in the order gradients become final (so per-segment events can release RCCL buckets while the
// rest of the backward is still running).
//
// Reference schedule being replaced: F.cross_entropy(ignore_index=51864)/accum (train_timestamps.py:1444-1450)
// -> scaler.scale(loss).backward() (:1454) -> unscale_/clip_grad_norm_/AdamW (:1509-1512).
#pragma once
#include <utility>

#include "engine_fwd.h"

namespace {

// refusals shared by every backward entry.  The fused ones need a trainable tensor; a stage backward that returns an input gradient does not
// (saliency on a frozen model).
int backward_check(const oasr_ctx* c, bool input_grad) {
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

// The three residual-gradient buffers of a backward (Plan::ga / gb / gc).  One is live: the gradient the next section consumes (null: nothing
// was handed down).  A block leaves the gradient it was given alone and alternates between the other two, so the LayerNorm backward that ends a
// section never writes what it reads.
template <typename T>
struct ResidGrad {
  T* buf[3];
  const T* live;
  T* spare[2];  // [0]: where the next section writes
  void enter_block() {
    int n = 0;
    for (T* b : buf)
      if (b != live && n < 2) spare[n++] = b;
  }
  void produced() {
    live = spare[0];
    std::swap(spare[0], spare[1]);
  }
};

template <typename T>
struct Runner : Forward<T> {
  typedef Forward<T> F;
  typedef AttnArgsT<T> Attn;
  using Forward<T>::Forward;
  using F::c, F::st, F::B, F::S, F::attn_args, F::dec_rows, F::dec_rows_bwd, F::dec_span;  // (names of a dependent base)
  using F::dgrad, F::wgrad, F::wgrad_side, F::wgrad_parts, F::wgrad_uncount, F::Gw;        // engine_gemm.h
  using F::side_mode, F::big_pending, F::fork_to, F::join_side, F::join_big, F::side_end;  // engine_side.h

  int record(void** ev, int idx) {
    if (ev && ev[idx]) OASR_CHECK_HIP(hipEventRecord((hipEvent_t)ev[idx], st));
    return OASR_OK;
  }

  // ---- one block.  dx_out (grad of the block output, g.live on entry) -> the grad of the block input (g.live on return).
  // Bias gradients of Linears that write into the residual stream (mlp.2, attn.out, cross_attn.out) are column sums of a
  // residual-stream gradient, and every such gradient is produced by a LayerNorm backward -> that kernel accumulates
  // them (its `dsum` output).  The caller's LN backward already filled this block's mlp.2.bias gradient from dx_out;
  // `dsum_next` is the bias gradient the produced dx_in belongs to (previous block's mlp.2.bias, or null).
  // Frozen parameters (oasr_ctx::Prune): every weight / bias / LayerNorm gradient of a frozen tensor is left out (null outputs, skipped
  // launches), and a section's data path runs only if something it feeds still needs a gradient (train_block_needs) -- `need_dx_in` (the
  // block's input gradient: a trainable tensor below it) or `need_xa` (d(xa): a trainable encoder tensor).  With every tensor trainable
  // both are true and every launch is the one of the plain step.

  // the end of a section: dx = LN'(gln) + (live gradient) into the spare buffer, once the section's side-stream weight gradients -- which read
  // what this may overwrite -- are done
  int ln_tail(Plan<T>& p, const T* x, int64_t w, int64_t b, const float* mean, const float* rstd, float* dsum, ResidGrad<T>& g, long M) {
    RC(join_side());
    RC(launch_layernorm_bwd(p.gln, x, c->P(w), mean, rstd, g.live, g.spare[0], c->Gt(w), c->Gt(b), dsum, M, c->d, st));
    g.produced();
    return OASR_OK;
  }
  // an attention backward from d_o = p.go: the forward's arguments, dq | dk | dv (self: p.gqkv; cross: p.gq, p.gkv), the query / value bias
  // gradients = column sums of dq / dv, fused into the store epilogues.
  // decoder positions the loss ignores have d_o == 0 exactly (three quarters of the 448 on the synthetic lengths): the kernels
  // find those 64-position tiles themselves and skip them (span-limited step: the span says where they are, and the rows past
  // it are not even written).  An encoder block's d_o has no zero rows.
  int attn_bwd(const AttnSave<T>& s, Plan<T>& p, const AttnP& ap, bool cross, long Tq, bool causal) {
    const int d = c->d;
    const bool dec = cross || causal;
    Attn a;
    attn_args(a, s, cross, Tq, cross ? c->Te : Tq, causal);
    a.d_o = p.go;
    a.delta = p.delta;
    a.dq = cross ? p.gq : p.gqkv;
    a.dk = cross ? p.gkv : p.gqkv + d;
    a.dv = a.dk + d;
    a.dq_colsum = c->Gt(ap.qb);
    a.dv_colsum = c->Gt(ap.vb);
    a.colsum_scratch = p.cs_scratch;
    a.qtile_flags = (dec && !dec_span) ? p.qtile_flags : nullptr;
    a.q_span = dec ? dec_span : nullptr;
    return launch_attention_bwd(a, st);
  }
  int mlp_bwd(const BlockP& bp, const BlockSave<T>& s, Plan<T>& p, ResidGrad<T>& g, long M) {
    const int d = c->d;
    RC(dgrad(g.live, M, d, c->template Wt<T>(bp.w2), 4 * d, s.u, nullptr, p.gu, c->Gt(bp.b1), true));  // s.u = GELU'(u); + fused mlp.0.bias gradient
    if (c->wn(bp.w1)) RC(wgrad_side(p.gu, 4 * d, M, 4 * d, plain_view(s.ln2, d), d, Gw(bp.w1), d));
    RC(dgrad(p.gu, M, 4 * d, c->template Wt<T>(bp.w1), d, nullptr, nullptr, p.gln));
    return ln_tail(p, bp.cross ? s.x_mid2 : s.x_mid, bp.mlp_ln_w, bp.mlp_ln_b, s.mean2, s.rstd2, c->Gt(bp.cross ? bp.cattn.ob : bp.attn.ob), g, M);
  }
  int cross_bwd(const BlockP& bp, const BlockSave<T>& s, Plan<T>& p, ResidGrad<T>& g, const BlockNeeds& n, long M, long Tq, bool first_cross,
                bool need_xa) {
    const int d = c->d;
    const long Mkv = (long)B * c->Te;
    if (c->wn(bp.cattn.ow)) RC(wgrad_side(g.live, d, M, d, plain_view(s.ca.o, d), d, Gw(bp.cattn.ow), d));
    RC(dgrad(g.live, M, d, c->template Wt<T>(bp.cattn.ow), d, nullptr, nullptr, p.go));
    RC(join_big());  // (the previous layer's key|value gradients still read p.gkv)
    RC(attn_bwd(s.ca, p, bp.cattn, true, Tq, false));
    if (c->wn(bp.cattn.qw)) RC(wgrad_side(p.gq, d, M, d, plain_view(s.ca.ln, d), d, Gw(bp.cattn.qw), d));
    if (n.ca_kv) {  // the encoder-sized key|value side: on its own side stream when the span step asks for it
      const bool big = (side_mode & SIDE_KV_BWD) != 0;
      if (big) {
        RC(fork_to(c->side.big));
        big_pending = true;
      }
      SideStreams::OnStream on(st, big ? c->side.big : st);
      const int64_t kv[2] = {bp.cattn.kw, bp.cattn.vw};
      RC(wgrad_parts(p.gkv, 2 * d, Mkv, plain_view(p.xa, d), d, kv, 2, d, true));
      // d(xa) accumulates over the decoder layers (bf16, like autograd's accumulation into xa.grad)
      if (need_xa) RC(dgrad(p.gkv, Mkv, 2 * d, c->template Wt<T>(bp.cattn.kw), d, nullptr, first_cross ? nullptr : p.gxa, p.gxa));
    }
    if (!n.ca_tail) return OASR_OK;
    RC(dgrad(p.gq, M, d, c->template Wt<T>(bp.cattn.qw), d, nullptr, nullptr, p.gln));
    return ln_tail(p, s.x_mid, bp.cln_w, bp.cln_b, s.ca.mean, s.ca.rstd, c->Gt(bp.attn.ob), g, M);
  }
  int self_bwd(const BlockP& bp, const BlockSave<T>& s, Plan<T>& p, ResidGrad<T>& g, const BlockNeeds& n, long M, long Tq, bool causal,
               float* dsum_next) {
    const int d = c->d;
    if (c->wn(bp.attn.ow)) RC(wgrad_side(g.live, d, M, d, plain_view(s.sa.o, d), d, Gw(bp.attn.ow), d));
    RC(dgrad(g.live, M, d, c->template Wt<T>(bp.attn.ow), d, nullptr, nullptr, p.go));
    RC(attn_bwd(s.sa, p, bp.attn, false, Tq, causal));
    const int64_t qkv[3] = {bp.attn.qw, bp.attn.kw, bp.attn.vw};
    RC(wgrad_parts(p.gqkv, 3 * d, M, plain_view(s.sa.ln, d), d, qkv, 3, d));
    if (!n.sa_tail) return OASR_OK;
    RC(dgrad(p.gqkv, M, 3 * d, c->template Wt<T>(bp.attn.qw), d, nullptr, nullptr, p.gln));
    return ln_tail(p, s.x_in, bp.attn_ln_w, bp.attn_ln_b, s.sa.mean, s.sa.rstd, dsum_next, g, M);
  }
  int block_bwd(const BlockP& bp, const BlockSave<T>& s, Plan<T>& p, ResidGrad<T>& g, long M, long Tq, bool causal, bool first_cross,
                float* dsum_next, bool need_dx_in, bool need_xa) {
    const int d = c->d;
    auto any = [&](std::initializer_list<int64_t> offs) {  // (weights: adapted ones count -- their adapters need dW)
      for (int64_t o : offs)
        if (c->wn(o)) return true;
      return false;
    };
    const AttnP &sa = bp.attn, &ca = bp.cattn;
    BlockAsk ask = {need_dx_in, need_xa, bp.cross};
    ask.sa = any({sa.qw, sa.kw, sa.vw, sa.ow, sa.qb, sa.vb, sa.ob, bp.attn_ln_w, bp.attn_ln_b});
    ask.ca = bp.cross && any({ca.qw, ca.kw, ca.vw, ca.ow, ca.qb, ca.vb, ca.ob, bp.cln_w, bp.cln_b});
    ask.mlp = any({bp.w1, bp.b1, bp.mlp_ln_w, bp.mlp_ln_b});
    ask.cln = bp.cross && any({bp.cln_w, bp.cln_b});
    ask.attn_ln = any({bp.attn_ln_w, bp.attn_ln_b});
    ask.kv = bp.cross && any({ca.kw, ca.vw});
    const BlockNeeds n = train_block_needs(ask);
    g.enter_block();
    if (c->wn(bp.w2)) RC(wgrad_side(g.live, d, M, d, plain_view(s.hg, 4 * d), 4 * d, Gw(bp.w2), 4 * d));
    if (n.mlp) RC(mlp_bwd(bp, s, p, g, M));
    if (n.ca) RC(cross_bwd(bp, s, p, g, n, M, Tq, first_cross, need_xa));
    if (n.sa) RC(self_bwd(bp, s, p, g, n, M, Tq, causal, dsum_next));
    if (!n.sa_tail) g.live = nullptr;  // (nothing below this block takes a gradient)
    return join_side();
  }

  // ---- the backward half of a training micro-step: p.logits holds d(loss)/d(logits) (bf16 engine: bf16 [Md, Vp]) on entry -- written in
  // place by the fused cross-entropy (oasr_train_step) or converted from the caller's fp32 tensor (oasr_train_bwd, the
  // torch.autograd path) -- and every saved activation of the forward is still in the workspace.  It runs in two halves (train_backward
  // below calls both).  backward_decoder starts from p.logits and ends at the token / positional embeddings; with `xa_grad` it
  // leaves d(xa) in p.gxa.  backward_encoder starts from d(xa) = `gxa` and ends at the conv stem; with `dmel` it also writes d(mel) (fp32
  // [B, n_mels, T1]: the conv1 data gradient, which no parameter needs).  A requested input gradient forces the data gradient it needs through
  // every block of its stage, whatever the trainability mask prunes (the staged autograd entries, oasr_train_encode_bwd / _decode_bwd); the
  // fused step asks for d(xa) exactly when an encoder tensor needs a gradient, and never for d(mel).
  int backward_decoder(Plan<T>& p, const int64_t* tokens, void** ev, int& seg, bool xa_grad) {
    const int d = c->d;
    // Md: the decoder's token rows the backward runs over -- all B*S, or (supervised-span step) the leading rows that hold every
    // position able to carry gradient; the rows behind them are never read or written by the backward
    const long Md = dec_rows_bwd ? dec_rows_bwd : (long)B * S;
    const oasr_ctx::Prune& pr = c->pr;
    // tied logits: dE += dlogits^T . lnf ; d(lnf) = dlogits . E
    // (V = n_vocab + 1 is odd: the direct-to-LDS kernel wants a multiple of 8 rows, so the pad class gets its own 1-row GEMM)
    if (c->tr(c->tok_emb)) {
      const int v8 = c->V & ~7;
      RC(wgrad(p.logits, c->Vp, Md, v8, plain_view(p.lnf, d), d, c->G(c->tok_emb), d));
      if (v8 < c->V) RC(wgrad(p.logits + v8, c->Vp, Md, c->V - v8, plain_view(p.lnf, d), d, c->G(c->tok_emb) + (long)v8 * d, d));
    }
    RC(dgrad(p.logits, Md, c->Vp, c->template Wt<T>(c->tok_emb), d, nullptr, nullptr, p.gln));
    const T* x_last = c->L_dec ? p.dec[c->L_dec - 1].x_out : p.dx0;
    RC(launch_layernorm_bwd(p.gln, x_last, c->P(c->dec_ln_w), p.mean_f, p.rstd_f, nullptr, p.ga, c->Gt(c->dec_ln_w), c->Gt(c->dec_ln_b),
                            c->L_dec ? c->Gt(c->dec[c->L_dec - 1].b2) : nullptr, Md, d, st));
    RC(record(ev, seg++));
    ResidGrad<T> g = {{p.ga, p.gb, p.gc}, p.ga};
    for (int i = c->L_dec - 1; i >= 0; --i) {
      // the gradient of block i's input: for a trainable tensor below it, or for a lower block's d(xa)
      const bool need_in = pr.all || pr.dec_below[i] || (i > 0 && xa_grad);
      if (pr.all || pr.dec_blk[i] || need_in || xa_grad)
        RC(block_bwd(c->dec[i], p.dec[i], p, g, Md, S, true, i == c->L_dec - 1, i > 0 ? c->Gt(c->dec[i - 1].b2) : nullptr, need_in, xa_grad));
      // the block's event says "every gradient of this block is complete" (the DDP reducer sends the bucket on it): that includes the
      // key|value weight gradient on the side stream (SIDE_KV_INFLIGHT, without events: it stays in flight until the next block needs p.gkv)
      if (ev || !(side_mode & SIDE_KV_INFLIGHT)) RC(join_big());
      RC(record(ev, seg++));
    }
    RC(join_side());
    RC(join_big());
    side_end();
    if (c->tr(c->tok_emb) || c->tr(c->dec_pos))
      RC(launch_embedding_bwd(tokens, g.live, c->Gt(c->tok_emb), c->Gt(c->dec_pos), B, S, d, PAD_ID, c->V, st, dec_rows, dec_span));
    RC(record(ev, seg++));  // decoder.positional_embedding
    RC(record(ev, seg++));  // token embedding (arena tail)
    if (xa_grad && c->L_dec == 0) OASR_CHECK_HIP(hipMemsetAsync(p.gxa, 0, (size_t)B * c->Te * d * sizeof(T), st));
    return OASR_OK;
  }

  int backward_encoder(Plan<T>& p, const T* gxa, void** ev, int& seg, float* dmel) {
    const int d = c->d, nm = c->dims.n_mels, T1 = c->T1, Te = c->Te;
    const long Me = (long)B * Te, M1 = (long)B * T1;
    const oasr_ctx::Prune& pr = c->pr;
    if (!pr.enc_any && !dmel) {  // nothing in the encoder is trainable and no d(mel): neither d(xa) (skipped in the decoder blocks) nor anything below it
      for (int i = 0; i < c->L_enc + 2; ++i) RC(record(ev, seg++));  // ln_post, the blocks, the conv stem
      return OASR_OK;
    }
    const T* xe_last = c->L_enc ? p.enc[c->L_enc - 1].x_out : p.x0;
    const bool enc_top_in = pr.all || pr.enc_in[c->L_enc] || dmel;
    if (enc_top_in || c->tr(c->enc_lnp_w) || c->tr(c->enc_lnp_b))
      RC(launch_layernorm_bwd(gxa, xe_last, c->P(c->enc_lnp_w), p.mean_p, p.rstd_p, nullptr, p.ga, c->Gt(c->enc_lnp_w), c->Gt(c->enc_lnp_b),
                              c->L_enc ? c->Gt(c->enc[c->L_enc - 1].b2) : nullptr, Me, d, st));
    RC(record(ev, seg++));
    ResidGrad<T> g = {{p.ga, p.gb, p.gc}, p.ga};
    for (int i = c->L_enc - 1; i >= 0; --i) {
      if (pr.all || pr.enc_blk[i] || pr.enc_in[i] || dmel)
        RC(block_bwd(c->enc[i], p.enc[i], p, g, Me, Te, false, false, i > 0 ? c->Gt(c->enc[i - 1].b2) : nullptr, pr.all || pr.enc_in[i] || dmel,
                     false));
      RC(record(ev, seg++));
    }
    // conv stem: x0 = gelu(u2) + pos ; u2 = conv2(h1) ; h1 = gelu(u1) ; u1 = conv1(mel)
    if (pr.all || c->tr(c->conv2_w) || c->tr(c->conv2_b) || pr.conv1 || dmel) {
      RC(launch_dgelu_mul(g.live, p.u2, p.gln, Me * d, st));  // gln = d(u2)
      if (c->tr(c->conv2_w)) {
        OASR_CHECK_HIP(hipMemsetAsync(p.tmp_w2p, 0, (size_t)d * 3 * d * 4, st));
        // conv2 weight gradient on the direct-to-LDS kernel: the im2col matrix [B*1500][3d] is h1 itself read as overlapping
        // rows of 3d elements at stride 2d from h1 - d (per-sample stride 3000*d == 1500 rows * 2d, so the view is plain).
        // Only window (b, t = 0) is wrong in its first d elements (it sees the last row of sample b-1, or the zeroed guard row,
        // instead of the left zero padding): dY rows (b, 0) times what those windows wrongly saw as their first tap comes out again.
        RC(wgrad(p.gln, d, Me, d, plain_view(p.h1 - d, 2L * d), 3 * d, p.tmp_w2p, 3 * d));  // (guard row zeroed by the forward)
        RC(wgrad_uncount(p.gln, (long)Te * d, B, d, p.h1 - d, (long)T1 * d, d, p.tmp_w2p, 3 * d));
        RC(launch_unpack_conv_grad(p.tmp_w2p, c->G(c->conv2_w), d, d, 3 * d, st));
      }
      if (c->tr(c->conv2_b)) RC(launch_colsum_accum(p.gln, d, Me, d, c->G(c->conv2_b), st));
    }
    if (pr.all || pr.conv1 || dmel) {  // the conv2 data gradient serves conv1 (and d(mel)) alone
      RC(dgrad(p.gln, Me, d, c->template w2p<T>(), 3 * d, nullptr, nullptr, p.gA2));
      RC(launch_conv2_col2im_dgelu(p.gA2, p.u1, p.gu, B, T1, d, st));  // gu = d(u1) [B*3000, d]
      if (c->tr(c->conv1_w)) {
        OASR_CHECK_HIP(hipMemsetAsync(p.tmp_w1p, 0, (size_t)d * 256 * 4, st));
        // conv1 weight gradient, same trick: windows of 3*n_mels (+ junk up to 256, whose gradient columns are never
        // unpacked) at stride n_mels from mel_tm - n_mels; the first tap of every (b, 0) and the last tap of every (b, T1-1)
        // see the neighbouring sample (or a zeroed guard row) instead of the zero padding -> dU rows (b, 0) / (b, T1-1) come out again.
        RC(wgrad(p.gu, d, M1, d, plain_view(p.mel_tm - nm, nm), 256, p.tmp_w1p, 256));  // (guard rows zeroed by the forward)
        RC(wgrad_uncount(p.gu, (long)T1 * d, B, d, p.mel_tm - nm, (long)T1 * nm, nm, p.tmp_w1p, 256));
        RC(wgrad_uncount(p.gu + (long)(T1 - 1) * d, (long)T1 * d, B, d, p.mel_tm + (long)T1 * nm, (long)T1 * nm, nm, p.tmp_w1p + 2 * nm, 256));
        RC(launch_unpack_conv_grad(p.tmp_w1p, c->G(c->conv1_w), d, nm, 256, st));
      }
      if (c->tr(c->conv1_b)) RC(launch_colsum_accum(p.gu, d, M1, d, c->G(c->conv1_b), st));
      if (dmel) {
        // d(mel): the conv1 data gradient as columns dcol [B*T1, 256] = d(u1) . w1p (gA2 is free again), then folded back onto the mel
        // frames -- taps that fall into the zero padding or the neighbouring sample are dropped (conv_grad.hip).  The bf16 engine's cast of
        // mel to bf16 counts as the identity here, as autocast's cast does.
        RC(dgrad(p.gu, M1, d, c->template w1p<T>(), 256, nullptr, nullptr, p.gA2));
        RC(launch_conv1_col2im_mel(p.gA2, dmel, B, T1, nm, st));
      }
    }
    RC(record(ev, seg++));
    return OASR_OK;
  }

  // adapter contexts: the adapted weights' gradients of THIS micro-batch go to workspace scratch (Gw; projected into the arena at the end)
  int backward_begin(Plan<T>& p) {
    if (!c->lora.empty()) OASR_CHECK_HIP(hipMemsetAsync(p.lora_dw, 0, (size_t)c->lora_dw_floats * 4, st));
    return OASR_OK;
  }
  // the last gradient segment of an adapter context: d lora_B = s * dW . lora_A^T, d lora_A = s * lora_B^T . dW (every dW is final here).
  // A stage's backward projects the adapters of its own stage's weights only (the other stage's scratch was never written).
  int backward_finish(Plan<T>& p, void** ev, int seg, int stage) {
    if (!c->lora.empty()) {
      for (const oasr_ctx::Lora& L : c->lora) {
        const bool in_enc = L.w >= c->enc_lnp_w && L.w < c->stem_end;
        if ((stage == STAGE_ENC && !in_enc) || (stage == STAGE_DEC && in_enc)) continue;
        float *ga = c->Gt(L.a), *gb = c->Gt(L.b);
        if (ga || gb) RC(launch_lora_grad(p.lora_dw + L.dw, c->P(L.a), c->P(L.b), L.out, L.in, c->lora_r, c->lora_s, ga, gb, p.lora_part, st));
      }
      RC(record(ev, seg++));
    }
    if (stage == STAGE_ALL && seg != (int)c->segments.size()) {
      oasr_set_error("internal: segment count mismatch %d vs %zu", seg, c->segments.size());
      return OASR_ESTATE;
    }
    return OASR_OK;
  }

  int train_backward(Plan<T>& p, const int64_t* tokens, void** ev) {
    // Frozen parameters (oasr_set_trainable, oasr_ctx::Prune): launches that only serve frozen tensors are left out, the data gradient
    // stops where nothing earlier in the forward is trainable.  Every segment event is still recorded (DDP buckets wait on them).
    RC(backward_check(c, false));
    RC(backward_begin(p));
    int seg = 0;
    RC(backward_decoder(p, tokens, ev, seg, c->pr.all || c->pr.enc_any));
    RC(backward_encoder(p, p.gxa, ev, seg, nullptr));
    return backward_finish(p, ev, seg, STAGE_ALL);
  }
};

}  // namespace
