// Context lifetime of the engine: parameter layout (Builder, oasr_create*), binding, the compute copies of the weights (shadow refresh, LoRA merge),
// the trainability mask and the optimizer entries.  The schedule itself is engine_fwd.h / engine_bwd.h (gathered by engine_run.h); its entry points are engine_step.hip / engine_decode.hip.
#include "engine_ctx.h"

namespace {

struct Builder {
  oasr_ctx* c;
  int64_t cur = 0;
  int64_t add(const std::string& name, std::initializer_list<int64_t> shape) {
    Tensor t;
    t.name = name;
    t.off = cur;
    t.ndim = (int)shape.size();
    t.numel = 1;
    int i = 0;
    for (auto s : shape) {
      t.shape[i++] = s;
      t.numel *= s;
    }
    for (; i < 4; ++i) t.shape[i] = 1;
    cur += t.numel;
    c->tensors.push_back(t);
    return t.off;
  }
  void attn(const std::string& p, AttnP& a, int d) {
    a.qw = add(p + ".query.weight", {d, d});
    a.kw = add(p + ".key.weight", {d, d});
    a.vw = add(p + ".value.weight", {d, d});
    a.ow = add(p + ".out.weight", {d, d});
    a.qb = add(p + ".query.bias", {d});
    a.vb = add(p + ".value.bias", {d});
    a.ob = add(p + ".out.bias", {d});
    a.fused_bias = c->aux_floats;
    c->aux_floats += 3 * d;
  }
  void block(const std::string& p, BlockP& b, int d, bool cross) {
    const int64_t start = cur;
    b.cross = cross;
    b.w2 = add(p + ".mlp.2.weight", {d, 4 * d});
    b.b2 = add(p + ".mlp.2.bias", {d});
    b.w1 = add(p + ".mlp.0.weight", {4 * d, d});
    b.b1 = add(p + ".mlp.0.bias", {4 * d});
    b.mlp_ln_w = add(p + ".mlp_ln.weight", {d});
    b.mlp_ln_b = add(p + ".mlp_ln.bias", {d});
    if (cross) {
      attn(p + ".cross_attn", b.cattn, d);
      b.cln_w = add(p + ".cross_attn_ln.weight", {d});
      b.cln_b = add(p + ".cross_attn_ln.bias", {d});
    }
    attn(p + ".attn", b.attn, d);
    b.attn_ln_w = add(p + ".attn_ln.weight", {d});
    b.attn_ln_b = add(p + ".attn_ln.bias", {d});
    c->segments.push_back({start, cur - start});
  }
};

}  // namespace

// ---- small kernels local to the engine -------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fused_bias_kernel(const float* __restrict__ qb, const float* __restrict__ vb, float* __restrict__ out,
                                                        int d) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < 3 * d; i += gridDim.x * 256)
    out[i] = i < d ? qb[i] : (i < 2 * d ? 0.f : vb[i - 2 * d]);
}

// ================================================ C ABI ============================================================
extern "C" oasr_ctx* oasr_create_ex2(const oasr_dims* dm, int embed_rows, int compute_dtype) {
  return oasr_create_ex3(dm, embed_rows, compute_dtype, nullptr, 0, 0, 0.f);
}
extern "C" oasr_ctx* oasr_create_ex(const oasr_dims* dm, int embed_rows) { return oasr_create_ex2(dm, embed_rows, OASR_DTYPE_BF16); }
extern "C" oasr_ctx* oasr_create(const oasr_dims* dm) { return oasr_create_ex2(dm, dm ? dm->n_vocab + 1 : 0, OASR_DTYPE_BF16); }

// embed_rows: rows of decoder.token_embedding -- n_vocab + 1 for the training model (pad row, olmoasr/model.py:665-667),
// n_vocab for the inference model (olmoasr/inf_model.py:302; checkpoints written by scripts/eval/gen_inf_ckpt.py)
// compute_dtype: OASR_DTYPE_BF16 = the production kernels; OASR_DTYPE_F32 = the fp32 validation kernels on the same
// schedule (reference: precision="float32", scripts/training/train_timestamps.py:2128,2220-2224)
// targets / rank / scale: LoRA adapters on block Linear weights (include/oasr.h, ABI 213; n_targets == 0: none)
extern "C" oasr_ctx* oasr_create_ex3(const oasr_dims* dm, int embed_rows, int compute_dtype, const int32_t* targets, int n_targets, int rank,
                                     float scale) {
  if (compute_dtype != OASR_DTYPE_BF16 && compute_dtype != OASR_DTYPE_F32) {
    oasr_set_error("oasr_create_ex2: compute_dtype must be OASR_DTYPE_BF16 or OASR_DTYPE_F32");
    return nullptr;
  }
  if (n_targets < 0 || (n_targets > 0 && (!targets || rank < 1 || rank > OASR_LORA_MAX_RANK || !(scale == scale)))) {
    oasr_set_error("oasr_create_ex3: adapters need a target list, rank 1..%d and a finite scale", OASR_LORA_MAX_RANK);
    return nullptr;
  }
  if (!dm) {
    oasr_set_error("oasr_create: null dims");
    return nullptr;
  }
  if (embed_rows != dm->n_vocab && embed_rows != dm->n_vocab + 1) {
    oasr_set_error("oasr_create_ex: embed_rows must be n_vocab or n_vocab + 1");
    return nullptr;
  }
  const int d = dm->n_audio_state;
  if (dm->n_text_state != d || dm->n_audio_head != dm->n_text_head || d != 64 * dm->n_audio_head || dm->n_mels != 80 ||
      (d % 64) != 0 || d > 2048 || dm->n_text_ctx > 448 || dm->n_text_ctx < 1) {
    oasr_set_error("oasr_create: unsupported dims (need n_audio_state == n_text_state == 64*heads <= 2048, n_mels == 80, n_text_ctx <= 448)");
    return nullptr;
  }
  oasr_ctx* c = new oasr_ctx();
  c->f32 = compute_dtype == OASR_DTYPE_F32;
  c->dims = *dm;
  c->d = d;
  c->H = dm->n_audio_head;
  c->L_enc = dm->n_audio_layer;
  c->L_dec = dm->n_text_layer;
  c->Te = dm->n_audio_ctx;
  c->T1 = 2 * dm->n_audio_ctx;
  c->S_max = dm->n_text_ctx;
  c->V = embed_rows;
  c->Vp = c->f32 ? c->V : (c->V + 127) / 128 * 128;  // (the fp32 kernels need no padded vocabulary)
  c->aux_floats = 0;
  Builder b{c};
  {  // decoder.ln
    const int64_t s0 = b.cur;
    c->dec_ln_w = b.add("decoder.ln.weight", {d});
    c->dec_ln_b = b.add("decoder.ln.bias", {d});
    c->segments.push_back({s0, b.cur - s0});
  }
  c->dec.resize(c->L_dec);
  for (int i = c->L_dec - 1; i >= 0; --i) b.block("decoder.blocks." + std::to_string(i), c->dec[i], d, true);
  {
    const int64_t s0 = b.cur;
    c->dec_pos = b.add("decoder.positional_embedding", {dm->n_text_ctx, d});
    c->segments.push_back({s0, b.cur - s0});
  }
  const size_t emb_seg = c->segments.size();
  c->segments.push_back({0, 0});  // token embedding: becomes final here in time, lives at the arena's end
  {
    const int64_t s0 = b.cur;
    c->enc_lnp_w = b.add("encoder.ln_post.weight", {d});
    c->enc_lnp_b = b.add("encoder.ln_post.bias", {d});
    c->segments.push_back({s0, b.cur - s0});
  }
  c->enc.resize(c->L_enc);
  for (int i = c->L_enc - 1; i >= 0; --i) b.block("encoder.blocks." + std::to_string(i), c->enc[i], d, false);
  {
    const int64_t s0 = b.cur;
    c->conv2_w = b.add("encoder.conv2.weight", {d, d, 3});
    c->conv2_b = b.add("encoder.conv2.bias", {d});
    c->conv1_w = b.add("encoder.conv1.weight", {d, dm->n_mels, 3});
    c->conv1_b = b.add("encoder.conv1.bias", {d});
    c->segments.push_back({s0, b.cur - s0});
  }
  c->stem_end = b.cur;
  if (n_targets > 0) {  // LoRA adapters: the last gradient segment, between the conv stem and the token embedding
    static const char* kinds[] = {".query.weight", ".key.weight", ".value.weight", ".out.weight", ".mlp.0.weight", ".mlp.2.weight"};
    const int n_base = (int)c->tensors.size();
    c->lora_of.assign((size_t)n_base + 2 * n_targets + 1, -1);
    c->lora_r = rank;
    c->lora_s = scale;
    for (int j = 0; j < n_targets; ++j) {
      const int ti = targets[j];
      bool ok = ti >= 0 && ti < n_base && c->lora_of[ti] < 0 && c->tensors[ti].name.find(".blocks.") != std::string::npos;
      if (ok) {
        const std::string& nm = c->tensors[ti].name;
        bool kind = false;
        for (const char* k : kinds) kind = kind || (nm.size() > strlen(k) && nm.compare(nm.size() - strlen(k), strlen(k), k) == 0);
        ok = kind && c->tensors[ti].ndim == 2;
      }
      if (!ok) {
        oasr_set_error("oasr_create_ex3: target %d (tensor %d%s%s) is not a block Linear weight (attn / cross_attn query|key|value|out, mlp.0, "
                       "mlp.2) or is listed twice", j, ti, ti >= 0 && ti < n_base ? ": " : "", ti >= 0 && ti < n_base ? c->tensors[ti].name.c_str() : "");
        delete c;
        return nullptr;
      }
      c->lora_of[ti] = j;
    }
    const int64_t s0 = b.cur;
    for (int j = 0; j < n_targets; ++j) {
      const Tensor w = c->tensors[targets[j]];
      const std::string mod = w.name.substr(0, w.name.size() - strlen(".weight"));
      oasr_ctx::Lora L;
      L.w = w.off;
      L.out = (int)w.shape[0];
      L.in = (int)w.shape[1];
      L.a = b.add(mod + ".lora_A", {rank, L.in});
      L.b = b.add(mod + ".lora_B", {L.out, rank});
      L.dw = c->lora_dw_floats;
      c->lora_dw_floats += (int64_t)L.out * L.in;
      const int64_t part = (int64_t)lora_grad_scratch_floats(L.out, L.in, rank);
      if (part > c->lora_part_floats) c->lora_part_floats = part;
      c->lora.push_back(L);
    }
    c->segments.push_back({s0, b.cur - s0});
    c->pr.all = c->pr.any = false;  // no default mask (include/oasr.h): nothing is trainable until oasr_set_trainable
  }
  c->tok_emb = b.add("decoder.token_embedding.weight", {c->V, d});
  c->segments[emb_seg] = {c->tok_emb, (int64_t)c->V * d};
  c->numel = b.cur;
  if (!c->lora.empty()) {
    c->lora_of.resize(c->tensors.size(), -1);
    c->pr.tr.assign(c->tensors.size(), 0);
    c->pr.need.assign(c->tensors.size(), 0);
  }
  {  // decoder layer 0's tensor offsets + the per-layer strides: the one-launch step engines derive every layer's addresses from them, so
     // the blocks must be laid out back to back with one stride -- checked here, engines off otherwise
    auto offs = [](const BlockP& bp) {
      DecLayerOffsets o;
      o.ln1g = bp.attn_ln_w, o.ln1b = bp.attn_ln_b, o.wqkv = bp.attn.qw, o.bqkv_aux = bp.attn.fused_bias, o.wo = bp.attn.ow, o.bo = bp.attn.ob;
      o.lncg = bp.cln_w, o.lncb = bp.cln_b, o.wcq = bp.cattn.qw, o.bcq = bp.cattn.qb, o.wco = bp.cattn.ow, o.bco = bp.cattn.ob;
      o.ln2g = bp.mlp_ln_w, o.ln2b = bp.mlp_ln_b, o.w1 = bp.w1, o.b1 = bp.b1, o.w2 = bp.w2, o.b2 = bp.b2;
      return o;
    };
    if (c->L_dec >= 1) {
      c->dec_l0 = offs(c->dec[0]);
      if (c->L_dec >= 2) {
        const DecLayerOffsets o1 = offs(c->dec[1]);
        c->dec_lstride = o1.ln1g - c->dec_l0.ln1g;
        c->dec_astride = o1.bqkv_aux - c->dec_l0.bqkv_aux;
      }
      c->dec_regular = true;
      for (int l = 0; l < c->L_dec; ++l) {
        const DecLayerOffsets ol = offs(c->dec[l]), want = dec::layer_at(c->dec_l0, l, c->dec_lstride, c->dec_astride);
        for (int k = 0; k < DecLayerOffsets::FIELDS; ++k) c->dec_regular = c->dec_regular && ol.fields()[k] == want.fields()[k];
      }
    }
  }
  // shadow: [bf16 flat arena + zero pad rows for the padded vocab] [W1p d x 256] [W2p d x 3d] [aux fp32]
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  c->sh_flat = 0;
  const size_t esz = c->f32 ? 4 : 2;  // fp32 validation: no shadow of the flat arena (the master weights are the operands)
  size_t off = c->f32 ? 256 : al(((size_t)c->numel + (size_t)(c->Vp - c->V) * d + 64) * 2);
  c->sh_w1p = off;
  off = al(off + (size_t)d * 256 * esz);
  c->sh_w2p = off;
  off = al(off + (size_t)d * 3 * d * esz);
  c->sh_aux = off;
  off = al(off + (size_t)c->aux_floats * 4);
  if (c->f32 && !c->lora.empty()) {  // fp32 effective copy of the whole arena (adapted slots = W0 + s * B . A)
    c->sh_eff = off;
    off = al(off + ((size_t)c->numel + 64) * 4);
  }
  c->sh_total = off;
  return c;
}
extern "C" void oasr_destroy(oasr_ctx* c) { delete c; }
extern "C" int oasr_compute_dtype(const oasr_ctx* c) { return c && c->f32 ? OASR_DTYPE_F32 : OASR_DTYPE_BF16; }
extern "C" int oasr_lora_count(const oasr_ctx* c) { return c ? (int)c->lora.size() : 0; }
extern "C" int oasr_param_count(const oasr_ctx* c) { return c ? (int)c->tensors.size() : 0; }
extern "C" int64_t oasr_param_numel(const oasr_ctx* c) { return c ? c->numel : 0; }
extern "C" int oasr_param_info(const oasr_ctx* c, int idx, char* name, int name_cap, int64_t* offset, int64_t* numel, int* ndim,
                               int64_t shape[4]) {
  OASR_REQUIRE(c && idx >= 0 && idx < (int)c->tensors.size(), "param_info: bad index");
  const Tensor& t = c->tensors[idx];
  if (name && name_cap > 0) snprintf(name, name_cap, "%s", t.name.c_str());
  if (offset) *offset = t.off;
  if (numel) *numel = t.numel;
  if (ndim) *ndim = t.ndim;
  if (shape)
    for (int i = 0; i < 4; ++i) shape[i] = t.shape[i];
  return OASR_OK;
}
extern "C" int oasr_segment_count(const oasr_ctx* c) { return c ? (int)c->segments.size() : 0; }
extern "C" int oasr_segment_info(const oasr_ctx* c, int idx, int64_t* offset, int64_t* numel) {
  OASR_REQUIRE(c && idx >= 0 && idx < (int)c->segments.size(), "segment_info: bad index");
  if (offset) *offset = c->segments[idx].off;
  if (numel) *numel = c->segments[idx].numel;
  return OASR_OK;
}
extern "C" int oasr_bind(oasr_ctx* c, float* params, float* grads, float* m, float* v, const float* enc_pos) {
  OASR_REQUIRE(c && params && enc_pos, "oasr_bind: params and enc_pos are required");
  c->params = params;
  c->grads = grads;
  c->m = m;
  c->v = v;
  c->enc_pos = enc_pos;
  return OASR_OK;
}
extern "C" size_t oasr_shadow_bytes(const oasr_ctx* c) { return c ? c->sh_total : 0; }
extern "C" int oasr_bind_shadow(oasr_ctx* c, void* shadow) {
  OASR_REQUIRE(c && shadow, "oasr_bind_shadow: null");
  c->shadow = (char*)shadow;
  return OASR_OK;
}

static int refresh_packed(oasr_ctx* c, hipStream_t st) {
  const int d = c->d;
  if (c->f32) {
    RC(launch_pack_conv_weight(c->P(c->conv1_w), (float*)(c->shadow + c->sh_w1p), d, c->dims.n_mels, 256, st));
    RC(launch_pack_conv_weight(c->P(c->conv2_w), (float*)(c->shadow + c->sh_w2p), d, d, 3 * d, st));
  } else {
    RC(launch_pack_conv_weight(c->P(c->conv1_w), (bf16_t*)(c->shadow + c->sh_w1p), d, c->dims.n_mels, 256, st));
    RC(launch_pack_conv_weight(c->P(c->conv2_w), (bf16_t*)(c->shadow + c->sh_w2p), d, d, 3 * d, st));
  }
  float* aux = (float*)(c->shadow + c->sh_aux);
  auto fb = [&](const AttnP& a) {
    hipLaunchKernelGGL(fused_bias_kernel, dim3(cdiv(3 * d, 256)), dim3(256), 0, st, c->P(a.qb), c->P(a.vb), aux + a.fused_bias, d);
  };
  for (auto& b : c->enc) fb(b.attn);
  for (auto& b : c->dec) {
    fb(b.attn);
    fb(b.cattn);
  }
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}

// Adapter contexts: the compute copies of the adapted tensors = their effective weights (lora_merge of the current masters and adapters).
// fp32 mode first copies the whole arena into the effective copy (validation mode: every tensor's operand comes from there).
static int refresh_lora(oasr_ctx* c, hipStream_t st) {
  if (c->lora.empty()) return OASR_OK;
  float* eff = c->f32 ? (float*)(c->shadow + c->sh_eff) : nullptr;
  bf16_t* flat = c->f32 ? nullptr : (bf16_t*)(c->shadow + c->sh_flat);
  if (eff) OASR_CHECK_HIP(hipMemcpyAsync(eff, c->params, (size_t)c->numel * 4, hipMemcpyDeviceToDevice, st));
  for (const oasr_ctx::Lora& L : c->lora)
    RC(launch_lora_merge(c->P(L.w), c->P(L.a), c->P(L.b), L.out, L.in, c->lora_r, c->lora_s, eff ? eff + L.w : nullptr, flat ? flat + L.w : nullptr, st));
  return OASR_OK;
}

extern "C" int oasr_refresh_shadow(oasr_ctx* c, void* stream) {
  RC(check_bound(c, false));
  hipStream_t st = (hipStream_t)stream;
  if (!c->f32) {
    bf16_t* flat = (bf16_t*)(c->shadow + c->sh_flat);
    RC(launch_cast_f32_bf16(c->params, flat, c->numel, st));
    OASR_CHECK_HIP(hipMemsetAsync(flat + c->numel, 0, ((size_t)(c->Vp - c->V) * c->d + 64) * 2, st));
  }
  RC(refresh_lora(c, st));
  return refresh_packed(c, st);
}

extern "C" int oasr_lora_merge(oasr_ctx* c, void* stream) {
  RC(check_bound(c, false));
  OASR_REQUIRE(!c->lora.empty(), "oasr_lora_merge: the context has no adapters");
  for (const oasr_ctx::Lora& L : c->lora)  // in place: every element is read and written by the same thread
    RC(launch_lora_merge(c->P(L.w), c->P(L.a), c->P(L.b), L.out, L.in, c->lora_r, c->lora_s, c->params + L.w, nullptr, (hipStream_t)stream));
  return OASR_OK;
}

extern "C" int oasr_zero_grad(oasr_ctx* c, void* stream) {
  RC(check_bound(c, true));
  OASR_CHECK_HIP(hipMemsetAsync(c->grads, 0, (size_t)c->numel * 4, (hipStream_t)stream));
  return OASR_OK;
}

// ---- frozen parameters ----------------------------------------------------------------------------------------------------------
// The plan of the pruned backward (oasr_ctx::Prune) and the optimizer's table of trainable runs, derived here once per mask change.
extern "C" int oasr_set_trainable(oasr_ctx* c, const uint8_t* mask, int n_params) {
  OASR_REQUIRE(c && mask && n_params == (int)c->tensors.size(), "oasr_set_trainable: need one byte per tensor (%d)", c ? (int)c->tensors.size() : 0);
  oasr_ctx::Prune pr;
  pr.tr.resize(c->tensors.size());
  pr.need.resize(c->tensors.size());
  bool all = true, any = false;
  for (int i = 0; i < n_params; ++i) {
    pr.tr[i] = mask[i] ? 1 : 0;
    all = all && pr.tr[i];
    any = any || pr.tr[i];
    OASR_REQUIRE(!(pr.tr[i] && !c->lora.empty() && c->lora_of[i] >= 0),
                 "oasr_set_trainable: %s carries a LoRA adapter and must stay frozen (merge the adapters first to train it)", c->tensors[i].name.c_str());
  }
  pr.any = any;
  for (int i = 0; i < n_params; ++i) {  // an adapted base weight needs its weight gradient while one of its adapters is trainable
    const int j = c->lora.empty() ? -1 : c->lora_of[i];
    pr.need[i] = pr.tr[i] || (j >= 0 && (mask[c->tidx(c->lora[j].a)] || mask[c->tidx(c->lora[j].b)]));
  }
  // maximal stretches of trainable tensors (the arena is the tensors back to back, in table order)
  std::vector<int64_t> runs;
  for (size_t i = 0; i < c->tensors.size(); ++i) {
    if (!pr.tr[i]) continue;
    const Tensor& t = c->tensors[i];
    if (!runs.empty() && runs[runs.size() - 2] + runs.back() == t.off) runs.back() += t.numel;
    else {
      runs.push_back(t.off);
      runs.push_back(t.numel);
    }
  }
  for (size_t k = 0; k < runs.size(); ++k)
    OASR_REQUIRE((runs[k] % 4) == 0, "oasr_set_trainable: trainable runs must start and end on multiples of 4 elements");
  auto any_in = [&](int64_t lo, int64_t hi) {  // a tensor inside arena range [lo, hi) that needs a gradient
    for (size_t i = 0; i < c->tensors.size(); ++i)
      if (pr.need[i] && c->tensors[i].off >= lo && c->tensors[i].off < hi) return true;
    return false;
  };
  auto blk_range = [&](const BlockP& b, int64_t* lo, int64_t* hi) {  // a block's tensors: mlp.2.weight first, attn_ln.bias last
    *lo = b.w2;
    *hi = b.attn_ln_b + c->d;
  };
  const int Ld = c->L_dec, Le = c->L_enc;
  pr.enc_any = any_in(c->enc_lnp_w, c->stem_end);
  pr.conv1 = any_in(c->conv1_w, c->conv1_w + 1) || any_in(c->conv1_b, c->conv1_b + 1);
  pr.dec_blk.assign(Ld, 0);
  pr.enc_blk.assign(Le, 0);
  pr.dec_in.assign(Ld + 1, 0);
  pr.enc_in.assign(Le + 1, 0);
  for (int i = 0; i < Ld; ++i) {
    int64_t lo, hi;
    blk_range(c->dec[i], &lo, &hi);
    pr.dec_blk[i] = any_in(lo, hi);
  }
  for (int i = 0; i < Le; ++i) {
    int64_t lo, hi;
    blk_range(c->enc[i], &lo, &hi);
    pr.enc_blk[i] = any_in(lo, hi);
  }
  // dec_in[i]: the gradient of block i's input is needed -- by the embeddings, a lower block, or (i > 0) a lower block's d(xa)
  bool below = any_in(c->tok_emb, c->tok_emb + 1) || any_in(c->dec_pos, c->dec_pos + 1);
  pr.dec_below.assign(Ld + 1, 0);
  for (int i = 0; i <= Ld; ++i) {
    pr.dec_below[i] = below;
    pr.dec_in[i] = below || (i > 0 && pr.enc_any);
    if (i < Ld) below = below || pr.dec_blk[i];
  }
  below = any_in(c->conv2_w, c->stem_end);  // the conv stem
  for (int i = 0; i <= Le; ++i) {
    pr.enc_in[i] = below;
    if (i < Le) below = below || pr.enc_blk[i];
  }
  pr.all = all;
  int64_t* dev = nullptr;
  if (!all && !runs.empty()) {
    OASR_CHECK_HIP(hipMalloc(&dev, runs.size() * sizeof(int64_t)));
    if (hipMemcpy(dev, runs.data(), runs.size() * sizeof(int64_t), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(dev);
      oasr_set_error("oasr_set_trainable: upload of the run table failed");
      return OASR_EHIP;
    }
  }
  // (the previous table may still be read by an optimizer step in flight on the caller's stream)
  if (c->runs_dev) OASR_CHECK_HIP(hipDeviceSynchronize());
  if (c->runs_dev) (void)hipFree(c->runs_dev);
  c->runs_dev = dev;
  c->n_runs = (int)(runs.size() / 2);
  c->pr = pr;
  c->mask_set = true;
  return OASR_OK;
}

extern "C" int oasr_optim_step(oasr_ctx* c, float inv_loss_scale, float max_grad_norm, float lr, float beta1, float beta2, float eps,
                               float weight_decay, int64_t step, float* stats_out, void* scratch, void* stream) {
  RC(check_bound(c, true));
  OASR_REQUIRE(c->m && c->v && stats_out && scratch && step >= 1, "oasr_optim_step: bad args");
  OASR_REQUIRE(c->pr.any, "oasr_optim_step: no parameter is trainable (oasr_set_trainable)");
  OASR_REQUIRE(c->lora.empty() || c->mask_set, "oasr_optim_step: a context with adapters needs oasr_set_trainable first");
  hipStream_t st = (hipStream_t)stream;
  const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
  const float bc2 = (float)(1.0 - pow((double)beta2, (double)step));
  bf16_t* sh = c->f32 ? nullptr : (bf16_t*)(c->shadow + c->sh_flat);
  if (c->pr.all) {
    RC(launch_grad_stats(c->grads, c->numel, (double*)scratch, stats_out, st));
    RC(launch_adamw(c->params, c->grads, c->m, c->v, sh, c->numel, stats_out, inv_loss_scale, max_grad_norm, lr, beta1, beta2, eps,
                    weight_decay, bc1, bc2, st));
  } else {  // trainable runs only: clip norm and found_inf over their gradients, frozen masters / moments / shadow untouched
    RC(launch_grad_stats_runs(c->grads, c->runs_dev, c->n_runs, (double*)scratch, stats_out, st));
    RC(launch_adamw_runs(c->params, c->grads, c->m, c->v, sh, c->runs_dev, c->n_runs, stats_out, inv_loss_scale, max_grad_norm, lr, beta1,
                         beta2, eps, weight_decay, bc1, bc2, st));
  }
  RC(refresh_lora(c, st));  // (adapters: the effective compute copies of the stepped masters and adapters)
  return refresh_packed(c, st);
}

// ---- ZeRO-1 building blocks: the optimizer over a contiguous RANGE of the flat arenas --------------------------------------
// The reference's sharded variant is FSDP (scripts/training/train_fsdp_timestamps.py:2665-2719).  Here optimizer-state
// sharding follows from the flat arena: rank r owns one contiguous range, keeps exp_avg / exp_avg_sq for that range only,
// and the step is  reduce-scatter(grads) -> partial sum of squares per rank -> all-reduce of 2 floats -> AdamW on the owned
// range -> all-gather(params)  (olmoasr_amd/zero.py).  Two entry points: the gradient statistics of a range and the step of a
// range given GLOBAL statistics.
extern "C" int oasr_grad_sumsq_range(oasr_ctx* c, int64_t off, int64_t numel, float* stats_out, void* scratch, void* stream) {
  RC(check_bound(c, true));
  OASR_REQUIRE(c->lora.empty(), "oasr_grad_sumsq_range: ZeRO-1 does not support LoRA adapters");
  OASR_REQUIRE(stats_out && scratch && off >= 0 && numel > 0 && off + numel <= c->numel && (off % 4) == 0 && (numel % 4) == 0,
               "oasr_grad_sumsq_range: bad range [%lld, +%lld) (multiples of 4 inside the arena)", (long long)off, (long long)numel);
  return launch_grad_stats(c->grads + off, numel, (double*)scratch, stats_out, (hipStream_t)stream);
}

// stats: device f32[2] = [sum of squares of the scaled gradients over the WHOLE arena, non-finite flag] (already reduced
// over ranks); m_shard / v_shard: this range's exp_avg / exp_avg_sq (numel floats each, shard-local buffers).
extern "C" int oasr_optim_step_range(oasr_ctx* c, int64_t off, int64_t numel, float* m_shard, float* v_shard, const float* stats,
                                     float inv_loss_scale, float max_grad_norm, float lr, float beta1, float beta2, float eps,
                                     float weight_decay, int64_t step, void* stream) {
  RC(check_bound(c, true));
  OASR_REQUIRE(c->lora.empty(), "oasr_optim_step_range: ZeRO-1 does not support LoRA adapters");
  OASR_REQUIRE(m_shard && v_shard && stats && step >= 1 && off >= 0 && numel > 0 && off + numel <= c->numel && (off % 4) == 0 &&
                   (numel % 4) == 0,
               "oasr_optim_step_range: bad args");
  const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
  const float bc2 = (float)(1.0 - pow((double)beta2, (double)step));
  return launch_adamw(c->params + off, c->grads + off, m_shard, v_shard, c->f32 ? nullptr : (bf16_t*)(c->shadow + c->sh_flat) + off, numel,
                      stats, inv_loss_scale, max_grad_norm, lr, beta1, beta2, eps, weight_decay, bc1, bc2, (hipStream_t)stream);
}
