// Engine context shared by engine.hip / engine_step.hip / engine_decode.hip: the parameter table and bound memory (oasr_ctx), the workspace bump
// allocator, and the small helpers every engine entry point uses.  Host code only.
#pragma once
#include <string>
#include <vector>

#include "../../include/oasr.h"
#include <math.h>

#include "kernels.h"

namespace {

constexpr long PAD_ID = 51864;

struct Tensor {
  std::string name;
  int64_t off, numel;
  int ndim;
  int64_t shape[4];
};

struct AttnP {
  int64_t qw, kw, vw, ow, qb, vb, ob;  // arena offsets (elements); qw,kw,vw are contiguous -> fused [3d,d]
  int64_t fused_bias;                  // offset (floats) into the aux fp32 region: [qb | 0 | vb]
};
struct BlockP {
  int64_t attn_ln_w, attn_ln_b, cln_w, cln_b, mlp_ln_w, mlp_ln_b, w1, b1, w2, b2;
  AttnP attn, cattn;
  bool cross;
};
struct Segment {
  int64_t off, numel;
};

}  // namespace

struct oasr_ctx {
  oasr_dims dims;
  int d, H, L_enc, L_dec, Te, T1, S_max, V, Vp;  // V = n_vocab+1 rows (train model), Vp = padded to 128
  std::vector<Tensor> tensors;
  std::vector<Segment> segments;
  std::vector<BlockP> enc, dec;
  int64_t dec_ln_w, dec_ln_b, dec_pos, enc_lnp_w, enc_lnp_b, conv1_w, conv1_b, conv2_w, conv2_b, tok_emb;
  int64_t numel;
  // bound memory
  float *params = nullptr, *grads = nullptr, *m = nullptr, *v = nullptr;
  const float* enc_pos = nullptr;
  char* shadow = nullptr;
  // shadow layout (bytes)
  size_t sh_flat, sh_w1p, sh_w2p, sh_aux, sh_total;
  int64_t aux_floats;
  int f32 = 0;  // compute_dtype: 0 = bf16 production kernels, 1 = fp32 validation kernels (fp32ref.hip)
  DecLayerOffsets dec_l0 = {};       // decoder layer 0's tensor offsets (the one-launch step engines derive every layer's from them)
  int64_t dec_lstride = 0, dec_astride = 0;  // layer l = dec::layer_at(dec_l0, l, dec_lstride, dec_astride)
  bool dec_regular = false;          // ... holds for every decoder block (false: irregular layout, one-launch engines off)
  // Side streams of the span step (engine_side.h): created on first use, lowest priority, so its weight-gradient
  // workgroups fill the compute units the main stream's launches leave idle
  struct Side {
    hipStream_t stream = nullptr;  // the R-row weight gradients of the decoder backward
    hipStream_t big = nullptr;     // the encoder-sized GEMMs of the cross-attention key|value side (forward projection, its two gradients)
    hipEvent_t fork[4] = {nullptr, nullptr, nullptr, nullptr}, join[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<hipEvent_t> kv_ready;  // [L_dec]: layer i's key|value projection has been written (forward)
    unsigned nf = 0, nj = 0;
    void destroy() {  // whatever was created (a half-built one included: engine_side.h, SideStreams::side_begin)
      for (hipEvent_t e : fork)
        if (e) (void)hipEventDestroy(e);
      for (hipEvent_t e : join)
        if (e) (void)hipEventDestroy(e);
      for (hipEvent_t e : kv_ready)
        if (e) (void)hipEventDestroy(e);
      if (stream) (void)hipStreamDestroy(stream);
      if (big) (void)hipStreamDestroy(big);
    }
  };
  mutable Side side;
  // set by oasr_decode_check when the one-launch decoder step (decode_xcd.hip) reported a poisoned team barrier: its 32 workgroups must be
  // resident at once, which a shared / CU-masked device does not guarantee.  From then on this context decodes on the multi-launch engine.
  bool xcd_disabled = false;
  int n_cu = 0;  // compute units of the device (queried by the first decoder step)
  // ---- frozen parameters (oasr_set_trainable) ----
  // Derived once per mask change and kept: which tensors are trainable, and for every place the backward could stop, whether anything
  // before it in the forward still needs a gradient.  all == true is the untouched training step (every launch as before).
  struct Prune {
    bool all = true, any = true;
    std::vector<uint8_t> tr;                 // [tensors]
    std::vector<uint8_t> need;               // [tensors]: tr, or an adapted base weight one of whose adapters is trainable
    bool enc_any = true;                     // some encoder tensor (ln_post, blocks, conv stem): the encoder backward and d(xa) run
    std::vector<uint8_t> dec_blk, enc_blk;   // [L]: the block holds a trainable tensor
    std::vector<uint8_t> dec_in, enc_in;     // [L + 1]: the data gradient out of block i (into the residual stream below it) is needed
    std::vector<uint8_t> dec_below;          // [L + 1]: dec_in without d(xa): a tensor below block i (a lower block, the embeddings) is trainable
    bool conv1 = true;                       // conv1 weight or bias: the conv2 data gradient and the col2im run
  } pr;
  int64_t* runs_dev = nullptr;  // [2 * n_runs] (offset, numel) of the maximal trainable stretches of the arena (device)
  int n_runs = 0;
  bool mask_set = false;  // oasr_set_trainable has been called (an adapter context has no default mask)
  // ---- LoRA adapters (oasr_create_ex3) ----
  struct Lora {
    int64_t w, a, b;  // arena offsets: base weight [out, in], lora_A [r, in], lora_B [out, r]
    int out, in;
    int64_t dw;       // offset (floats) of the base weight's gradient in a training step's workspace scratch (Plan::lora_dw)
  };
  std::vector<Lora> lora;
  std::vector<int> lora_of;           // [tensors]: index into `lora` of an adapted base weight, -1 otherwise
  int lora_r = 0;
  float lora_s = 0.f;
  int64_t lora_dw_floats = 0, lora_part_floats = 0;  // training workspace: adapted weight gradients, lora_grad's partial sums
  int64_t stem_end = 0;  // arena end of the conv stem (= the token embedding's offset when there are no adapters)
  size_t sh_eff = 0;     // fp32 mode with adapters: the fp32 effective copy of the arena in the shadow (0 = none)
  size_t tidx(int64_t off) const {  // the tensor at arena offset `off`
    size_t lo = 0, hi = tensors.size();
    while (hi - lo > 1) {
      const size_t mid = (lo + hi) / 2;
      if (tensors[mid].off <= off) lo = mid;
      else hi = mid;
    }
    return lo;
  }
  // is the tensor at arena offset `off` trainable
  bool tr(int64_t off) const { return pr.all || pr.tr[tidx(off)] != 0; }
  // does the backward need the weight gradient of the tensor at `off`: trainable, or an adapted base weight with a trainable adapter
  bool wn(int64_t off) const { return pr.all || pr.need[tidx(off)] != 0; }
  int lora_at(int64_t off) const { return lora.empty() ? -1 : lora_of[tidx(off)]; }
  float* Gt(int64_t off) const { return tr(off) ? grads + off : nullptr; }  // gradient of a tensor, null when it is frozen
  ~oasr_ctx() {
    if (runs_dev) (void)hipFree(runs_dev);
    side.destroy();
  }
  // compute copy of the weight at arena offset `off`: the bf16 shadow, or -- fp32 validation -- the master weights themselves (with
  // adapters: their fp32 effective copy).  An adapted tensor's compute copy is its effective weight W0 + s * B . A.
  template <typename T>
  const T* Wt(int64_t off) const;
  template <typename T>
  const T* w1p() const { return (const T*)(shadow + sh_w1p); }  // packed conv1 kernel [d][256]
  template <typename T>
  const T* w2p() const { return (const T*)(shadow + sh_w2p); }  // packed conv2 kernel [d][3d]
  const float* P(int64_t off) const { return params + off; }
  float* G(int64_t off) const { return grads + off; }
  const float* aux(int64_t off) const { return (const float*)(shadow + sh_aux) + off; }
};

template <>
inline const bf16_t* oasr_ctx::Wt<bf16_t>(int64_t off) const { return (const bf16_t*)(shadow + sh_flat) + off; }
template <>
inline const float* oasr_ctx::Wt<float>(int64_t off) const { return sh_eff ? (const float*)(shadow + sh_eff) + off : params + off; }

// fn<T>(args...) for the context's compute dtype: T = bf16_t (production) or float (validation)
#define OASR_BY_DTYPE(c, fn, ...) ((c)->f32 ? fn<float>(__VA_ARGS__) : fn<bf16_t>(__VA_ARGS__))

namespace {

// ---- workspace bump allocator (dry-run when base == nullptr) --------------------------------------------------
struct Arena {
  char* base;
  size_t cur = 0, cap;
  Arena(void* b, size_t c) : base((char*)b), cap(c) {}
  void* raw(size_t bytes) {
    cur = (cur + 255) & ~(size_t)255;
    void* p = base ? base + cur : (void*)(uintptr_t)(cur + 256);  // non-null fake in dry-run
    cur += bytes;
    return p;
  }
  template <typename T>
  T* act(size_t n) { return (T*)raw((n + 32) * sizeof(T)); }  // +32 elements: conv windows / 16-byte tails may over-read
  float* f32(size_t n) { return (float*)raw(n * 4); }
};

#define RC(x)            \
  do {                   \
    int _rc = (x);       \
    if (_rc) return _rc; \
  } while (0)

// Plans of the training step (engine_plan.h: make_plan): the fused step's, or one stage's of the staged autograd entries
enum { STAGE_ALL = 0, STAGE_ENC = 1, STAGE_DEC = 2 };

int check_bound(const oasr_ctx* c, bool need_grads) {
  OASR_REQUIRE(c, "null context");
  if (!c->params || !c->shadow || !c->enc_pos || (need_grads && !c->grads)) {
    oasr_set_error("context not fully bound (oasr_bind / oasr_bind_shadow)");
    return OASR_ESTATE;
  }
  return OASR_OK;
}

}  // namespace
