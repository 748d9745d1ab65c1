// Workspace plan of the engine: every saved activation and every backward temporary of one call has a slot in the caller's workspace
// (no autograd tape).  Written once for both compute dtypes: T = bf16_t (production) or float (validation).
#pragma once
#include "engine_ctx.h"

namespace {

template <typename T>
struct AttnSave {
  T *ln, *qkv, *o;  // self: qkv [M,3d];  cross: qkv = q [M,d]
  T* kv;            // cross only: [B*Te, 2d]
  float *mean, *rstd, *lse;
  T* o_lo;  // training only: bf16 rounding residual of the attention output (o + o_lo = fp32-grade O for the backward's delta)
};
template <typename T>
struct BlockSave {
  T* x_in;  // residual stream entering the block (owned by the previous stage)
  AttnSave<T> sa, ca;
  T *x_mid, *x_mid2, *ln2, *u, *hg, *x_out;
  float *mean2, *rstd2;
};

template <typename T>
struct Plan {
  // encoder
  T *mel_tm, *u1, *h1, *u2, *x0, *xa;
  float *mean_p, *rstd_p;
  std::vector<BlockSave<T>> enc, dec;
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

template <typename T>
void plan_attn(Arena& A, AttnSave<T>& s, long M, long Mkv, int d, int B, int H, long Tq, bool cross, bool train) {
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
template <typename T>
void make_plan(const oasr_ctx* c, Arena& A, Plan<T>& p, int B, int S, bool train, int stage = STAGE_ALL) {
  const int d = c->d;
  const long Me = (long)B * c->Te, M1 = (long)B * c->T1, Md = (long)B * S;
  const bool enc = stage != STAGE_DEC, dec = stage != STAGE_ENC;
  p = Plan<T>();
  if (enc) {
    p.mel_tm = A.template act<T>(M1 * c->dims.n_mels + 2 * 256) + 256;  // zeroed guard rows on both sides (conv1 weight gradient windows)
    p.u1 = A.template act<T>(M1 * d);
    p.h1 = A.template act<T>(M1 * d + d) + d;  // one zeroed time row in front: the conv2 weight gradient reads h1 as overlapping windows from h1 - d
    p.u2 = A.template act<T>(Me * d);
    p.x0 = A.template act<T>(Me * d);
  }
  auto plan_block = [&](BlockSave<T>& s, long M, long Tq, bool cross) {
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
    BlockSave<T> s0, s1;
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
      BlockSave<T> s0, s1;
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

}  // namespace
