// The training engine's host decisions that are pure arithmetic on plain values (train_plan_host.cpp): how a weight gradient is split, which
// sections of a block's backward run under a trainability mask, and whether the span step's row table can chunk a shape.  Plain C++ (no HIP).
#pragma once

// Runner::wgrad: dW[N, K] += dy[M, N]^T . x[M, K] over M token rows; `view`: x is a conv-window view (OperandView::rpb != 0)
struct WgradPlan {
  int split_k, atomic_on_pp;
};
WgradPlan train_wgrad_plan(long M, int N, int K, bool view);

// Runner::block_bwd.  Asked: need_dx_in -- the gradient of the block's input (a trainable tensor below it); need_xa -- d(xa) (a trainable
// encoder tensor, or the caller's request); cross -- the block has a cross-attention; and, per group of the block's tensors, "one of them needs a
// gradient" (weights: oasr_ctx::wn, adapted ones count): sa = self-attention weights, biases and attn_ln; ca = the cross-attention's and
// cross_attn_ln; mlp = mlp.0 and mlp_ln (mlp.2 is asked on its own: its weight gradient comes first, before anything can stop); cln =
// cross_attn_ln alone; attn_ln alone; kv = the cross key | value weights.
struct BlockAsk {
  bool need_dx_in, need_xa, cross, sa, ca, mlp, cln, attn_ln, kv;
};
// Answered: the sections whose data path runs (mlp: everything past the mlp.2 weight gradient), and inside them the cross key|value side
// (its weight gradient and / or d(xa)) and the two LayerNorm tails that hand the gradient on (through cross_attn_ln, through attn_ln).
// sa implies ca in a cross block, and either implies mlp: a section never runs without the ones above it.
struct BlockNeeds {
  bool mlp, ca, sa, ca_kv, ca_tail, sa_tail;
};
BlockNeeds train_block_needs(const BlockAsk& a);

// the supervised-span step's chunk-row table (64-position chunks, kernels.h: launch_build_span_tables) covers this context and batch
bool span_chunkable(int S_max, int B);
