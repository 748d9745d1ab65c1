// KV-cache greedy decoding: cache layout, the choice between the three step engines, and the multi-launch step itself.
#include "engine_run.h"
#include "decode_wide_plan.h"
#include "decode_xcd_plan.h"

// ---- cached greedy decoding (OLMoASR.install_kv_cache_hooks, olmoasr/model.py:925-964 / inf_model.py:422-453) -----------
// The reference caches every key/value Linear output in a dict via forward hooks (self-attention K/V grow by torch.cat per
// token, cross-attention K/V are computed once per window).  Here the cache is one caller-owned buffer:
//   per decoder layer: self Q|K|V [B, n_text_ctx, 3d] | cross KV [B, n_audio_ctx, 2d]   (bf16)
// oasr_decode_begin fills the cross K/V of all layers from xa; oasr_decode_step runs the decoder on ONE new token per
// sequence at position `pos`: ONE fused q|k|v projection writes straight into the cache row of that position (GEMM output
// row stride = one sequence's cache; the q slot is scratch that keeps the three projections in a single launch),
// attention reads q from that row and the first pos+1 cached keys/values through strides.
namespace {
// elements of one decoder layer's cache: self q|k|v [B, S_max, 3d] followed by cross k|v [B, Te, 2d]
size_t kv_layer_elems(const oasr_ctx* c, int B) { return (size_t)3 * B * c->S_max * c->d + (size_t)B * c->Te * 2 * c->d; }
template <typename T>
struct KvLayer {
  T *qkv, *ckv;  // self [B, S_max, 3d] (q | k | v per position), cross [B, Te, 2d]
};
template <typename T>
KvLayer<T> kv_layer(const oasr_ctx* c, void* cache, int B, int layer) {
  T* base = (T*)cache + kv_layer_elems(c, B) * layer;
  return KvLayer<T>{base, base + (size_t)3 * B * c->S_max * c->d};
}
unsigned* kv_ctrl(const oasr_ctx* c, void* cache, int B) {  // the control tail behind the last layer (oasr_kv_cache_bytes)
  return (unsigned*)((char*)cache + kv_layer_elems(c, B) * (c->f32 ? 4 : 2) * c->L_dec);
}

// A/B and test switch of the step engine (oasr_decode_set_ln_fold; decode_step_core.h: StepMode).  STEP_SEPARATE_LN .. STEP_TEAM_SPREAD64 are
// bit-identical, STEP_WIDE within fp32 summation-order rounding (tests/test_gpu_decode_step.py).
int g_step_mode = dec::STEP_DEFAULT;

// The engine one step runs on.  Neither `wide` nor `team`: the multi-launch step, with (`folded`) or without LayerNorm folded into the projections.
struct StepEngine {
  bool folded = false, team = false, wide = false;
  int nwg = 0, stride = 0;  // one-launch engines: workgroups, and 8 = one per CU of ONE XCD / 1 = spread over the chip (DecodeStepArgs::team, stride)
};
int pick_step_engine(oasr_ctx* c, int B, StepEngine& e) {
  e = StepEngine();
  if (c->f32) return OASR_OK;  // (fp32 validation: separate kernels only)
  const int d = c->d, S_max = c->S_max, mode = g_step_mode;
  // a few sequences on the bf16 engine: every LayerNorm rides in the operand load of the projection that consumes it and the
  // logits leave as fp32 (8 launches per layer instead of 11; bit-identical to the separate kernels).  Measured
  // (profiles/r02_decode_step.txt): -5 % per step at B = 1, but every workgroup recomputes the B row statistics, which loses
  // from B = 16 on (+20 %) -- so only small batches take it (oasr_decode_set_ln_fold forces either side for the A/B and the
  // bit-identity test).
  e.folded = d % 64 == 0 && d <= 2048 && mode != dec::STEP_SEPARATE_LN && (B <= 4 || (mode == dec::STEP_FOLDED_LN && B <= 32));
  // one launch for the whole decoder stack (decode_xcd.hip): the default for a handful of sequences
  // (default: ONE sequence -- the timestamp-mode transcribe loop -- on the chip-wide one-launch engine, decode_wide.hip: 0.74 ms per token at medium
  // against 1.76 for the one-XCD team of decode_xcd.hip and 2.44 multi-launch, profiles/r06_decode_wide.txt; at small B = 4 the multi-launch
  // kernels, which spread over the whole chip, win: profiles/r05_decode_xcd_probe_v8.txt.  STEP_WIDE forces the chip-wide engine, the STEP_TEAM_*
  // modes the team engine up to B = 4.)
  if (c->n_cu == 0) {
    int dev = 0, n = 0;
    OASR_CHECK_HIP(hipGetDevice(&dev));
    OASR_CHECK_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
    c->n_cu = n > 0 ? n : -1;
  }
  const int nwg = c->n_cu >= 256 ? 256 : (c->n_cu > 0 ? c->n_cu & ~3 : 0);
  const bool one_launch = !c->xcd_disabled && c->dec_regular;
  const bool spread = mode == dec::STEP_TEAM_SPREAD32 || mode == dec::STEP_TEAM_SPREAD64;
  e.wide = (mode == dec::STEP_DEFAULT || mode == dec::STEP_WIDE) && B == 1 && one_launch && decode_wide_supports(d, c->H, c->Te, S_max, c->L_dec, B, nwg, c->V);
  e.team = !e.wide && ((mode == dec::STEP_DEFAULT && B == 1) || mode >= dec::STEP_TEAM_XCD) && one_launch && decode_xcd_supports(d, c->H, c->Te, S_max, c->L_dec, B) &&
           decode_xcd_offsets_ok(c->dec_l0, c->dec_lstride, (long)kv_layer_elems(c, B), d, c->Te, c->L_dec, B);
  e.nwg = e.wide ? nwg : (mode == dec::STEP_TEAM_SPREAD64 ? 64 : 32);
  e.stride = (e.wide || spread) ? 1 : 8;
  return OASR_OK;
}
}  // namespace

extern "C" size_t oasr_kv_cache_bytes(const oasr_ctx* c, int B) {
  if (!c || B <= 0) return 0;
  return kv_layer_elems(c, B) * (c->f32 ? 4 : 2) * c->L_dec + OASR_KV_TAIL_BYTES;
}
extern "C" int oasr_decode_set_ln_fold(int mode) {
  OASR_HOOK_GATE("oasr_decode_set_ln_fold");
  g_step_mode = mode < 0 ? dec::STEP_DEFAULT : (mode > dec::STEP_WIDE ? dec::STEP_FOLDED_LN : mode);  // (the clamping is part of the hook's contract)
  return OASR_OK;
}

extern "C" size_t oasr_decode_step_workspace_bytes(const oasr_ctx* c, int B) {
  if (!c || B <= 0) return 0;
  // x, ln, q, o, x2 (5 * B*d) + u, hg (2 * B*4d) + logits (B*Vp) bf16 + stats
  return ((size_t)B * c->d * 6 + (size_t)B * 8 * c->d + (size_t)B * c->Vp + 9 * 32) * (c->f32 ? 4 : 2) + (size_t)B * c->H * 8 + (size_t)B * 16 + 8192 +
         (B <= 4 ? (decode_xcd_part_floats(B, c->H, c->Te) + decode_wide_part_floats(c->H)) * 4 + 256 + 512 : 0);
}

template <typename T>
static int oasr_decode_begin_impl(oasr_ctx* c, const void* xa, int B, void* kv_cache, void* stream) {
  RC(check_bound(c, false));
  OASR_REQUIRE(xa && kv_cache && B > 0, "oasr_decode_begin: bad args");
  Runner<T> r{c, (hipStream_t)stream, B, 1, nullptr};
  const int d = c->d;
  // the one-launch step engines' control words, flags and packets live in the cache's tail (decode_step_core.h: KvCtrl)
  OASR_CHECK_HIP(hipMemsetAsync(kv_ctrl(c, kv_cache, B), 0, OASR_KV_TAIL_BYTES, (hipStream_t)stream));
  for (int i = 0; i < c->L_dec; ++i) {
    const BlockP& bp = c->dec[i];
    KvLayer<T> kl = kv_layer<T>(c, kv_cache, B, i);
    RC(r.linear((const T*)xa, (long)B * c->Te, d, c->template Wt<T>(bp.cattn.kw), 2 * d, c->aux(bp.cattn.fused_bias) + d, 0, nullptr, kl.ckv, nullptr));
  }
  return OASR_OK;
}
extern "C" int oasr_decode_begin(oasr_ctx* c, const void* xa, int B, void* kv_cache, void* stream) {
  OASR_REQUIRE(c, "oasr_decode_begin: null context");
  return OASR_BY_DTYPE(c, oasr_decode_begin_impl, c, xa, B, kv_cache, stream);
}

namespace {
// one step's activation rows and statistics in the caller's workspace
template <typename T>
struct StepWs {
  Arena A;
  T *x, *ln, *q, *o, *x2, *x3, *u, *hg, *logits;
  float *lse, *mean, *rstd;
  StepWs(const oasr_ctx* c, int B, void* workspace, size_t bytes) : A(workspace, bytes) {
    const size_t Bd = (size_t)B * c->d;
    x = A.template act<T>(Bd);
    ln = A.template act<T>(Bd);
    q = A.template act<T>(Bd);
    o = A.template act<T>(Bd);
    x2 = A.template act<T>(Bd);
    x3 = A.template act<T>(Bd);
    u = A.template act<T>(4 * Bd);
    hg = A.template act<T>(4 * Bd);
    logits = A.template act<T>((size_t)B * c->Vp);
    lse = A.f32((size_t)B * c->H);
    mean = A.f32(B);
    rstd = A.f32(B);
  }
};

// final LayerNorm + tied logits projection, folded: fp32 logits [B, rows] straight from the residual stream
int folded_logits(const oasr_ctx* c, const bf16_t* x, int B, float* logits_out, hipStream_t st) {
  return launch_decode_proj(x, B, c->d, c->Wt<bf16_t>(c->tok_emb), c->V, c->P(c->dec_ln_w), c->P(c->dec_ln_b), nullptr, 0, nullptr, 0, nullptr, 0,
                            logits_out, c->V, st);
}

// the whole decoder stack of one token in ONE launch (w.x: the embedded token): the chip-wide engine, which also projects the logits, or the
// team engine followed by the folded logits projection
int launch_one_launch_step(const oasr_ctx* c, const StepEngine& e, StepWs<bf16_t>& w, int B, int pos, void* kv_cache, float* logits_out, hipStream_t st) {
  DecodeStepArgs xa;
  xa.wflat = c->Wt<bf16_t>(0);
  xa.params = c->params;
  xa.aux = c->aux(0);
  xa.cache = (bf16_t*)kv_cache;
  xa.cache_lstride = (long)kv_layer_elems(c, B);
  xa.x = w.x, xa.x2 = w.x2, xa.x3 = w.x3, xa.q = w.q, xa.o = w.o, xa.hg = w.hg;
  xa.part = w.A.f32(decode_xcd_part_floats(B, c->H, c->Te));
  xa.ctrl = kv_ctrl(c, kv_cache, B);
  xa.d = c->d, xa.H = c->H, xa.Te = c->Te, xa.S_max = c->S_max, xa.L = c->L_dec, xa.M = B, xa.pos = pos;
  xa.team = e.nwg, xa.stride = e.stride;
  if (e.wide) xa.part = w.A.f32(decode_wide_part_floats(c->H));
  {  // measurement hooks (scripts/decode_xcd_probe.py; inert without OASR_TESTING_HOOKS=1): experiment flags, in-kernel stamps in the workspace tail
    static const int xflags = [] {
      const char* e = oasr_experiment_env("OASR_XCD_FLAGS");
      return e ? atoi(e) : 0;
    }();
    xa.flags = (xflags & 0xff) | (((xflags >> dec::XF_STAMP_WG_SHIFT) & 0xff) << 8);  // (bits 9-16: the workgroup whose stamps the chip-wide engine takes)
    xa.stamps = (xflags & dec::XF_STAMPS) ? (void*)(w.A.base + w.A.cap - 512) : nullptr;
  }
  xa.l0 = c->dec_l0, xa.lstride = c->dec_lstride, xa.astride = c->dec_astride;
  if (e.wide) {  // ... and the final LayerNorm + logits projection as its last phase: one launch per token behind the embedding
    xa.w_logits = c->Wt<bf16_t>(c->tok_emb), xa.lnf_g = c->P(c->dec_ln_w), xa.lnf_b = c->P(c->dec_ln_b), xa.logits_out = logits_out, xa.V = c->V;
    return launch_decode_wide(xa, st);
  }
  RC(launch_decode_xcd(xa, st));
  return folded_logits(c, w.x, B, logits_out, st);
}
}  // namespace

// tokens_last i64 [B]: the token at position pos of every sequence.  logits_out f32 [B, rows] for the NEXT position.
template <typename T>
static int oasr_decode_step_impl(oasr_ctx* c, const int64_t* tokens_last, int B, int pos, void* kv_cache, float* logits_out,
                                void* workspace, size_t workspace_bytes, void* stream) {
  RC(check_bound(c, false));
  OASR_REQUIRE(tokens_last && kv_cache && logits_out && workspace && B > 0 && pos >= 0 && pos < c->S_max, "oasr_decode_step: bad args");
  OASR_REQUIRE(workspace_bytes >= oasr_decode_step_workspace_bytes(c, B), "oasr_decode_step: workspace too small");
  constexpr bool bf16 = std::is_same<T, bf16_t>::value;
  const int d = c->d, S_max = c->S_max;
  hipStream_t st = (hipStream_t)stream;
  Runner<T> r{c, st, B, 1, nullptr};
  StepWs<T> w(c, B, workspace, workspace_bytes);
  // token + positional embedding of position pos: S = 1 per sequence, positional row offset by pos
  RC(launch_embedding_fwd(tokens_last, c->P(c->tok_emb), c->P(c->dec_pos) + (size_t)pos * d, w.x, B, 1, d, c->V, st));
  StepEngine e;
  RC(pick_step_engine(c, B, e));
  if constexpr (bf16) {
    if (e.wide || e.team) return launch_one_launch_step(c, e, w, B, pos, kv_cache, logits_out, st);
  }
  // out[B, N] (row stride ldc) = act(LayerNorm(x) . W^T + bias): folded into one projection kernel, or the LayerNorm kernel and a GEMM
  auto ln_linear = [&](const T* x, int64_t ln_w, int64_t ln_b, int64_t W, int N, const float* bias, int act, T* out, long ldc, T* out_pre) -> int {
    if constexpr (bf16) {
      if (e.folded)
        return launch_decode_proj(x, B, d, c->template Wt<T>(W), N, c->P(ln_w), c->P(ln_b), bias, act, nullptr, 0, out, ldc, nullptr, 0, st);
    }
    RC(launch_layernorm_fwd(x, c->P(ln_w), c->P(ln_b), w.ln, w.mean, w.rstd, B, d, st));
    GemmArgsT<T> g = gemm_defaults_t<T>();
    g.A = plain_view(w.ln, d);
    g.B = plain_view(c->template Wt<T>(W), d);
    g.M = B;
    g.N = N;
    g.K = d;
    g.bias = bias;
    g.act = act;
    g.out = out;
    g.out_pre = out_pre;
    g.ldc = ldc;
    return launch_gemm(g, st);
  };
  T *cur = w.x, *x2 = w.x2, *x3 = w.x3;
  for (int i = 0; i < c->L_dec; ++i) {
    const BlockP& bp = c->dec[i];
    KvLayer<T> kl = kv_layer<T>(c, kv_cache, B, i);
    // q | k | v of this position in one launch, straight into the cache: output row b lands at [b, pos, 0:3d]
    // (query | key | value weights are adjacent in the arena; bias = [q_bias | 0 | v_bias])
    RC(ln_linear(cur, bp.attn_ln_w, bp.attn_ln_b, bp.attn.qw, 3 * d, c->aux(bp.attn.fused_bias), 0, kl.qkv + (size_t)pos * 3 * d, (long)S_max * 3 * d,
                 nullptr));
    AttnArgsT<T> a;
    memset(&a, 0, sizeof(a));
    a.q = kl.qkv + (size_t)pos * 3 * d;
    a.ldq = 3 * d;
    a.bsq = (long)S_max * 3 * d;
    a.k = kl.qkv + d;
    a.v = kl.qkv + 2 * d;
    a.ldk = a.ldv = 3 * d;
    a.bsk = a.bsv = (long)S_max * 3 * d;
    a.o = w.o;
    a.ldo = d;
    a.bso = d;
    a.lse = w.lse;
    a.B = B;
    a.H = c->H;
    a.Tq = 1;
    a.Tk = pos + 1;
    RC(launch_attention_fwd(a, st));
    RC(r.linear(w.o, B, d, c->template Wt<T>(bp.attn.ow), d, c->P(bp.attn.ob), 0, cur, x2, nullptr));
    RC(ln_linear(x2, bp.cln_w, bp.cln_b, bp.cattn.qw, d, c->P(bp.cattn.qb), 0, w.q, d, nullptr));
    a.q = w.q;
    a.ldq = d;
    a.bsq = d;
    a.k = kl.ckv;
    a.v = kl.ckv + d;
    a.ldk = a.ldv = 2 * d;
    a.bsk = a.bsv = (long)c->Te * 2 * d;
    a.Tk = c->Te;
    RC(launch_attention_fwd(a, st));
    RC(r.linear(w.o, B, d, c->template Wt<T>(bp.cattn.ow), d, c->P(bp.cattn.ob), 0, x2, x3, nullptr));
    RC(ln_linear(x3, bp.mlp_ln_w, bp.mlp_ln_b, bp.w1, 4 * d, c->P(bp.b1), 1, w.hg, 4 * d, w.u));
    RC(r.linear(w.hg, B, 4 * d, c->template Wt<T>(bp.w2), d, c->P(bp.b2), 0, x3, cur == w.x ? x2 : w.x, nullptr));
    cur = (cur == w.x) ? x2 : w.x;
  }
  if constexpr (bf16) {
    if (e.folded) return folded_logits(c, cur, B, logits_out, st);
  }
  RC(ln_linear(cur, c->dec_ln_w, c->dec_ln_b, c->tok_emb, c->Vp, nullptr, 0, w.logits, c->Vp, nullptr));
  return launch_logits_to_f32(w.logits, c->Vp, B, c->V, logits_out, st);
}
extern "C" int oasr_decode_step(oasr_ctx* c, const int64_t* tokens_last, int B, int pos, void* kv_cache, float* logits_out,
                                void* workspace, size_t workspace_bytes, void* stream) {
  OASR_REQUIRE(c, "oasr_decode_step: null context");
  return OASR_BY_DTYPE(c, oasr_decode_step_impl, c, tokens_last, B, pos, kv_cache, logits_out, workspace, workspace_bytes, stream);
}

// whisper's rearrange_kv_cache on the engine-owned cache, in place and in one launch (beam.hip: kv_reorder_kernel): row j continues row
// sources[j] (device int32 [B]).  Only the self-attention k | v columns of positions < pos move; sources_host, when given, is the same index
// where the host can read it, and an index that leaves its group of `group` rows is refused there before the launch.
extern "C" int oasr_decode_reorder(oasr_ctx* c, void* kv_cache, int B, int pos, int group, const int32_t* sources, const int32_t* sources_host,
                                   void* stream) {
  OASR_REQUIRE(c && kv_cache && sources && B > 0, "oasr_decode_reorder: bad args");
  OASR_REQUIRE(group >= 1 && group <= OASR_BEAM_MAX && B % group == 0, "oasr_decode_reorder: 1 <= group <= %d must divide B = %d", OASR_BEAM_MAX, B);
  OASR_REQUIRE(pos >= 0 && pos <= c->S_max, "oasr_decode_reorder: pos = %d outside [0, %d]", pos, c->S_max);
  if (sources_host)
    for (int j = 0; j < B; ++j) {
      const int lo = j / group * group;
      OASR_REQUIRE(sources_host[j] >= lo && sources_host[j] < lo + group,
                   "oasr_decode_reorder: row %d continues row %d, outside its group of %d rows (beams never cross windows)", j, sources_host[j], group);
    }
  const int esz = c->f32 ? 4 : 2;
  return launch_kv_reorder(kv_cache, (long)(kv_layer_elems(c, B) * esz), c->L_dec, B, c->S_max, c->d, esz, pos, group, sources, (hipStream_t)stream);
}

// Synchronises the stream before the caller reads a window's tokens back (the step engines themselves cannot fail once enqueued).
extern "C" int oasr_decode_check(oasr_ctx* c, int B, void* kv_cache, void* stream) {
  OASR_REQUIRE(c && kv_cache && B > 0, "oasr_decode_check: bad args");
  OASR_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  unsigned ctrl[dec::KV_CTRL_WORDS] = {};  // the one-launch step engines' control words: a poisoned team barrier / a desynchronised stream is an error
  OASR_CHECK_HIP(hipMemcpy(ctrl, kv_ctrl(c, kv_cache, B), sizeof(ctrl), hipMemcpyDeviceToHost));
  if (ctrl[dec::KV_ERROR] != 0) {
    // The one-launch engine needs its whole team (32 workgroups x ~160 KB of LDS on one XCD) resident at once; a second decoder on the same
    // device, or a CU-masked / partitioned device, can leave part of a team queued behind the rest, and the bounded spin then poisons the
    // barrier instead of hanging.  Nothing is wrong with the cache's K/V rows written before that step, but the window's tokens are: the
    // context falls back to the multi-launch engine for good, the control words are cleared, and the caller re-decodes the window
    // (olmoasr_amd.decoding.decode does; OASR_ERETRY says "same call again").
    c->xcd_disabled = true;
    OASR_CHECK_HIP(hipMemset(kv_ctrl(c, kv_cache, B), 0, OASR_KV_TAIL_BYTES));
    oasr_set_error("oasr_decode_check: the one-launch decoder step reported 0x%x (1 = a team member never reached a barrier -- is the device "
                   "shared or CU-masked? --, 0x1xx = block stream out of step); XCC mask 0x%x.  The one-launch engine is now disabled for this "
                   "context; decode the window again (it will run on the multi-launch engine)", ctrl[dec::KV_ERROR], ctrl[dec::KV_XCC_MASK]);
    return OASR_ERETRY;
  }
  return OASR_OK;
}

