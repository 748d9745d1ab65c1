// bf16 MFMA GEMM for gfx950 with fp32 accumulation and a fused epilogue.
//
// Implements every Linear / Conv1d / tied-logits contraction of the reference (olmoasr/model.py:97-101 Linear,
// :104-195 Conv1d as window GEMMs, :768-770 logits) and their autograd backward (dgrad, wgrad), SURVEY.md §2.3
// K2,K3,K5,K9,K12,K14.
//
// Four kernel families, one file each over gemm_common.h (what they share: operand views, LDS images and fragment readers of the
// direct-to-LDS kernels, the fused epilogue); this file checks the arguments, chooses the kernel (gemm_route) and owns the test hooks and
// the per-launch profile records:
//  * oasr_gemm_pp_kernel   (gemm_pp.hip) 256x256x64 "ping-pong": 8 waves, one workgroup per CU, direct-to-LDS (buffer_load ... lds)
//    staging that is never drained inside the K loop (one counted vmcnt per K-tile), two wave groups one barrier
//    apart so one of them is always inside an MFMA section.  Default for every bf16-output GEMM with more than half
//    a wave of tiles (all Linear forward / dgrad GEMMs of the training step).
//  * oasr_gemm_fast_kernel (gemm_fast.hip) 256x128x64 (4 waves; 3 workgroups per CU for the split-K / atomic wgrad variant, 2 for
//    bf16 outputs) and 256x256x64 (8 waves, 2 stages): direct-to-LDS staging, one stage drained per barrier;
//    co-resident workgroups hide each other's drains.  wgrad (fp32 atomics, XCD-owned K ranges) and small problems.
//  * gemm_kernel           (gemm_general.hip) 128x128x64, register-staged with bounds-checked buffer loads: conv window views (rpb != 0),
//    K not a multiple of 64, fp32 / positional-embedding / odd-stride outputs.
//  * gemm_skinny_kernel    (gemm_general.hip) M <= 64 rows (decode steps): 32 columns per workgroup, K split over the 4 waves, weights streamed
//    from L2/HBM straight into MFMA operands.
// Operands whose reduction index is NOT contiguous in memory (dgrad's W[N][K], wgrad's dY[M][N] and X[M][K]) are kept
// in their natural layout and transposed on the way into the matrix core with ds_read_b64_tr_b16, so no transposed
// copies of weights or activations exist in HBM.  LDS images are XOR-swizzled so both ds_read_b128 (k-contiguous
// tiles) and the transpose reads are bank-conflict free.  For bf16 outputs the MFMA is issued with swapped operands
// (D'[n][m]) so each lane holds 4 consecutive columns of one output row; results leave through a wave-private LDS
// tile so that every global access of the epilogue (stores, residual / dGELU-input reads) is 16 bytes per lane.
#include <math.h>
#include <stdlib.h>

#include <map>
#include <string>
#include <vector>

#include "gemm_common.h"

namespace {

// ---- optional per-launch timing (bench.py's live roofline measurement): HIP events on the launch stream --------
struct GemmProfile {
  bool on = false;
  std::vector<hipEvent_t> events;  // pairs (start, stop)
  struct Rec {
    int kind;
    double flops;
    const char* name;  // kernel symbol as rocprofv3 prints it (template arguments included)
    int M = 0, N = 0, K = 0, epi = 0;  // shape + epilogue summary (bit 0 bias, 1 residual, 2 GELU, 3 GELU' input, 4 colsum, 5 atomic/split-K)
    int lane = 0;                      // 0 = the caller's stream with the chip to itself, 1 = a lowest-priority side stream of the span step,
                                       // 2 = the caller's stream while side-stream filler is in flight (gemm_profile_lane)
    // what the launch was, for tests that must know which kernel ran and how (gemm_profile_records)
    int ta = 0, tb = 0, flags = 0, split_k = 1, atomic = 0, atomic_on_pp = 0, scratch = 0, stagger = 0, stagger_phases = 0, persistent = 0;
  };
  std::vector<Rec> recs;
  int lane = 0;
  // A side-stream launch is low-priority filler: its begin-to-end span (HIP events and rocprofv3 alike) includes the time it waits for
  // compute units behind the main stream's workgroups, so it is a queueing time, not a kernel time.  Records carry the lane they were
  // launched on and gemm_profile_collect() reports the lanes apart ("symbol [side]"; "symbol [shared]" = main-stream launches of the decoder
  // phases, which give up compute units to that filler and run longer for it): the roofline of a symbol is that of the launches that have
  // the chip to themselves (profiles/r05_side_streams.txt: mixing them turned 0.40 into 0.33 while the step got faster).
  void push(Rec r) {
    r.lane = lane;
    recs.push_back(r);
  }
};
GemmProfile g_prof;

// Process-wide kernel selection set through include/oasr_testing.h (tests and A/B scripts); the defaults are what production runs.
enum class ForcedPath { Auto = 0, General, Fast256x128, Fast256x256Stage2, PingPong };  // the codes of oasr_gemm_force_general
struct GemmHooks {
  ForcedPath path = ForcedPath::Auto;   // oasr_gemm_force_general
  int stagger = 0, stagger_phases = 2;  // oasr_gemm_set_stagger: 0 = the automatic rule, > 0 = forced on every call, < 0 = off everywhere
  // oasr_gemm_set_variant; -1 = default everywhere
  int pp_schedule = -1;    // ping-pong K-tile schedule (2 or 7) instead of the per-layout choice
  int pp_persistent = -1;  // ping-pong kernel launched persistent: 0 never, 1 whenever possible
  int epi_flags = -1;      // epilogue memory policy (GemmArgs::epi_flags) instead of the caller's
};
GemmHooks g_hooks;

// profile record of one launch: kind = layout index 2*ta + tb, the epilogue summary bench.py's by-shape lines print, and the launch facts
GemmProfile::Rec gemm_rec(const GemmArgs& a, double flops, const char* name, bool persistent = false) {
  GemmProfile::Rec r{(a.ta ? 2 : 0) + (a.tb ? 1 : 0), flops, name, a.M, a.N, a.K,
                     (a.bias ? 1 : 0) | (a.resid ? 2 : 0) | (a.act ? 4 : 0) | (a.dgelu_u ? 8 : 0) | (a.colsum ? 16 : 0) | (a.atomic ? 32 : 0)};
  r.ta = a.ta ? 1 : 0;
  r.tb = a.tb ? 1 : 0;
  r.flags = (int)epi_flags_of(a, false);
  r.split_k = a.split_k;
  r.atomic = a.atomic;
  r.atomic_on_pp = a.atomic_on_pp;
  r.scratch = (a.colsum && a.colsum_scratch) ? 1 : 0;
  r.stagger = a.stagger;
  r.stagger_phases = a.stagger_phases;
  r.persistent = persistent ? 1 : 0;
  return r;
}

// Geometry choice for bf16-output GEMMs, from interleaved A/B runs on the OLMoASR-medium shapes (scripts/gemm_ab.py,
// encoder M = 96000 and decoder M = 28672 tokens): the ping-pong kernel is faster on every layer shape (+4..20 % on
// the encoder, +4..43 % on the decoder where 256 x 128 tiles quantise badly) except the dGELU-epilogue dgrad (-3 %).
// Below ~half a wave of 256 x 256 tiles the 256 x 128 geometry keeps more CUs busy.
bool prefer_pingpong(const GemmArgs& a) {
  return a.K >= 2 * BK && (long)cdiv(a.M, 256) * cdiv(a.N, 256) > 128;
}

// The whole kernel choice of one call, in one place: `a` is the call with the hooks and launch rules applied, `geom_env` the OASR_GEMM_GEOM
// experiment value (0 = none).  Host-only and free of side effects: no HIP call, no allocation, nothing process-wide is read.
GemmRoute gemm_route(const GemmArgs& a, const GemmHooks& hooks, int geom_env) {
  GemmRoute r;
  const bool plain = !a.A.rpb && !a.B.rpb && (a.K % BK) == 0;
  // decode-sized problems: a few token rows against a whole weight matrix
  if (a.M <= 64 && !a.ta && !a.tb && plain && a.split_k == 1 && !a.atomic && !a.colsum && hooks.path == ForcedPath::Auto) {
    r.family = GemmFamily::Skinny;
    return r;
  }
  const bool atomic_only = a.atomic && a.out_f32 && !a.out && !a.out_pre;
  const bool fast = plain && (!a.ta || (a.M % 8) == 0) && (!a.tb || (a.N % 8) == 0) && a.M >= 8 && a.N >= 8 && hooks.path != ForcedPath::General &&
                    (atomic_only || fast_rows_ok(a));
  if (!fast) {
    r.family = GemmFamily::General;
    r.post = a.colsum ? GemmPost::ColsumFromOut : GemmPost::None;  // unfused fallback
    return r;
  }
  // Geometry (measured: scripts/gemm_ab.py, scripts/wgrad_sweep.py): bf16 outputs -> the ping-pong kernel unless the
  // problem has under half a wave of 256x256 tiles; split-K / atomic outputs (wgrad) -> 256x128 with 3 workgroups per
  // CU, whose co-resident workgroups hide the atomic epilogues.  OASR_GEMM_GEOM=1|2|3 overrides (experiments).
  // 1 = 256x128, 2 = 256x256 / 2 stages, 3 = ping-pong (ForcedPath::General never gets here)
  const int geom = hooks.path != ForcedPath::Auto ? (int)hooks.path - 1 : geom_env;
  const bool pp = geom == 3 || (geom == 0 && !atomic_only && prefer_pingpong(a)) ||
                  (geom == 0 && atomic_only && a.atomic_on_pp && (a.M % 256) == 0 && (a.N % 256) == 0);
  const bool big = geom == 2;  // (the 256x256 / 2-stage geometry lost to 256x128 on every measured shape incl. small split-K outputs: scripts/wgrad_sweep.py)
  r.family = pp ? GemmFamily::PingPong : GemmFamily::Fast;
  r.swap = !atomic_only;                                  // bf16 outputs: D'[n][m]; fp32 atomics: D[m][n]
  r.csum = r.swap && a.colsum && !a.ta && a.tb && !big;  // dgrad + fused bias gradient
  if (pp) {
    r.pp_var = hooks.pp_schedule >= 0 ? hooks.pp_schedule : (r.csum ? 2 : 7);  // which schedule a layout gets, and why: gemm_pp.hip
  } else {
    r.fbn = big ? 256 : 128;
    r.nwn = big ? 4 : 2;
    r.nstage = big ? 2 : 1;
  }
  // column sums: fused kernels leave partial rows in the scratch (without scratch they used atomics: nothing left to do), the others sum `out`
  if (a.colsum) r.post = !r.csum ? GemmPost::ColsumFromOut : a.colsum_scratch ? GemmPost::ColsumFromScratch : GemmPost::None;
  return r;
}

GemmKernel* route_kernel(const GemmArgs& a, const GemmRoute& r) {
  switch (r.family) {
    case GemmFamily::Skinny: return gemm_skinny_kernel_of(a.M);
    case GemmFamily::Fast: return gemm_fast_kernel_of(a.ta, a.tb, r);
    case GemmFamily::PingPong: return gemm_pp_kernel_of(a.ta, a.tb, r);
    default: return gemm_general_kernel(a.ta, a.tb);
  }
}

}  // namespace

int gemm_timed_launch(GemmKernel& k, const GemmLaunch& l, const GemmArgs& a, hipStream_t stream) {
  if (l.lds > 0) {
    const int rc = ensure_dynamic_lds(k.lds_attr, k.handle, l.lds);
    if (rc) return rc;
  }
  hipEvent_t e1 = nullptr;
  if (g_prof.on) {
    const size_t idx = g_prof.recs.size();
    while (g_prof.events.size() < 2 * (idx + 1)) {
      hipEvent_t e;
      OASR_CHECK_HIP(hipEventCreate(&e));
      g_prof.events.push_back(e);
    }
    e1 = g_prof.events[2 * idx + 1];
    g_prof.push(gemm_rec(a, l.flops, k.symbol.c_str(), l.persistent));
    OASR_CHECK_HIP(hipEventRecord(g_prof.events[2 * idx], stream));
  }
  void* params[] = {const_cast<GemmArgs*>(&a)};
  (void)hipLaunchKernel(k.handle, l.grid, l.block, params, (size_t)l.lds, stream);
  OASR_LAUNCH_CHECK();
  if (e1) OASR_CHECK_HIP(hipEventRecord(e1, stream));
  return OASR_OK;
}

// v < 0: defaults.  bits 0-3: ping-pong schedule, 2 or 7 (the VAR of oasr_gemm_pp_kernel) or 8 = the per-layout default; bits 4-5:
// 0 = default launch rule, 1 = never persistent, 2 = persistent whenever possible; bit 6: non-temporal output stores, bit 7:
// non-temporal side-input loads.  (24 = default kernels, plain launches; 40 = default kernels, persistent)
int gemm_set_variant(int v) {
  const int sched = v & 15, launch = (v >> 4) & 3;
  OASR_REQUIRE(v < 0 || sched == 2 || sched == 7 || sched == 8,
               "gemm_set_variant: schedule %d (bits 0-3 of %d) does not exist: 2, 7 or 8 = per-layout default", sched, v);
  g_hooks.pp_schedule = (v < 0 || sched == 8) ? -1 : sched;
  g_hooks.pp_persistent = v < 0 ? -1 : launch - 1;
  g_hooks.epi_flags = v < 0 ? -1 : ((v >> 6) & 3);
  return OASR_OK;
}
void gemm_set_stagger(int sleeps, int phases) {  // sleeps < 0: stagger off everywhere (A/B baseline)
  g_hooks.stagger = sleeps;
  g_hooks.stagger_phases = phases < 2 ? 2 : phases;
}

int launch_gemm(const GemmArgs& args, hipStream_t stream) {
  OASR_REQUIRE(args.A.ptr && args.B.ptr, "gemm: null operand");
  GemmArgs a = args;  // the call with the process-wide hooks and launch rules applied
  if (g_hooks.epi_flags >= 0) a.epi_flags = g_hooks.epi_flags;
  if (a.stagger == 0 && g_hooks.stagger > 0) {
    a.stagger = g_hooks.stagger;
    a.stagger_phases = g_hooks.stagger_phases;
  } else if (a.stagger == 0 && g_hooks.stagger == 0 && a.N <= 1024 && a.K <= 1024 && a.M >= 16384 && a.out && !a.out_f32) {
    // measured (scripts/gemm_stagger_ab.py, M = 192000): +14 % on N = 1024, K = 1024 (tiles of ~8 us whose epilogues collide),
    // 0..-3 % on every longer tile -> only the short ones are staggered: 8 phases x one s_sleep(127)
    a.stagger = 1;
    a.stagger_phases = 8;
  }
  OASR_REQUIRE(a.M > 0 && a.N > 0 && a.K > 0, "gemm: bad shape %d %d %d", a.M, a.N, a.K);
  OASR_REQUIRE((a.N % 4) == 0, "gemm: N (%d) must be a multiple of 4", a.N);
  OASR_REQUIRE((a.A.ld % 8) == 0 && (a.B.ld % 8) == 0, "gemm: operand leading dims must be multiples of 8 (16-byte loads)");
  OASR_REQUIRE(a.ta || (a.K % 8) == 0 || a.A.rpb, "gemm: K must be a multiple of 8 for k-contiguous A");
  // (a k-contiguous operand is fetched in 16-byte chunks that are bounds-checked at their first element: a last chunk that straddles K
  //  would bring in up to 7 elements past it, and NaN / Inf there survives the other operand's zero fill)
  OASR_REQUIRE(a.tb || (a.K % 8) == 0 || a.B.rpb, "gemm: K must be a multiple of 8 for k-contiguous B");
  OASR_REQUIRE(a.split_k >= 1, "gemm: split_k");
  OASR_REQUIRE(a.split_k == 1 || (a.atomic && a.out_f32 && !a.out && !a.out_pre), "gemm: split_k > 1 needs atomic fp32 output only");
  OASR_REQUIRE(a.out || a.out_f32 || a.out_pre, "gemm: no output");
  OASR_REQUIRE(!a.colsum || (a.out && (a.N % 8) == 0 && a.split_k == 1), "gemm: colsum needs a bf16 `out`, N % 8 == 0, split_k == 1");
  static const int env_gm = [] {
    const char* e = oasr_experiment_env("OASR_GEMM_GM");
    return e ? atoi(e) : 0;
  }();
  if (a.raster_gm == 0 && env_gm > 0) a.raster_gm = env_gm;
  static const int env_geom = [] {
    const char* e = oasr_experiment_env("OASR_GEMM_GEOM");
    return e ? atoi(e) : 0;
  }();
  const GemmRoute r = gemm_route(a, g_hooks, env_geom);
  int rc;
  switch (r.family) {
    case GemmFamily::Skinny: rc = gemm_launch_skinny(a, stream); break;
    case GemmFamily::Fast: rc = gemm_launch_fast(a, r, stream); break;
    case GemmFamily::PingPong: rc = gemm_launch_pp(a, r, g_hooks.pp_persistent, stream); break;
    default: rc = gemm_launch_general(a, stream); break;
  }
  if (rc != OASR_OK || r.post == GemmPost::None) return rc;
  if (r.post == GemmPost::ColsumFromScratch) return launch_colsum_accum(a.colsum_scratch, a.N, 2L * cdiv(a.M, 256), a.N, a.colsum, stream);
  return launch_colsum_accum(a.out, a.ldc, a.M, a.N, a.colsum, stream);
}

void gemm_profile_enable(int on) {
  g_prof.on = on != 0;
  if (on) g_prof.recs.clear();
}
int gemm_profile_lane(int lane) {
  const int old = g_prof.lane;
  if (lane >= 0) g_prof.lane = lane;  // (negative: query only)
  return old;
}

// Sums elapsed ms / algorithmic flops / launch count per operand layout (index = 2*ta + tb) and, as text
// "symbol\tlaunches\tms\tflops\n", per kernel symbol (so bench.py can be checked against rocprofv3's per-kernel
// averages).  Synchronises.
int gemm_profile_collect(double ms[4], double flops[4], long count[4], char* by_symbol, int cap) {
  for (int i = 0; i < 4; ++i) {
    ms[i] = 0;
    flops[i] = 0;
    count[i] = 0;
  }
  struct Agg {
    long n = 0;
    double ms = 0, flops = 0;
  };
  std::map<std::string, Agg> agg;
  for (size_t i = 0; i < g_prof.recs.size(); ++i) {
    OASR_CHECK_HIP(hipEventSynchronize(g_prof.events[2 * i + 1]));
    float t = 0.f;
    OASR_CHECK_HIP(hipEventElapsedTime(&t, g_prof.events[2 * i], g_prof.events[2 * i + 1]));
    const int k = g_prof.recs[i].kind;
    if (g_prof.recs[i].lane != 1) {  // per-layout totals: main-stream launches only (side-stream spans are queueing times)
      ms[k] += t;
      flops[k] += g_prof.recs[i].flops;
      count[k] += 1;
    }
    static const bool by_shape = oasr_experiment_env("OASR_PROF_SHAPES") != nullptr;  // experiments: one line per (symbol, shape, epilogue)
    std::string key = g_prof.recs[i].name;
    if (g_prof.recs[i].lane) key += g_prof.recs[i].lane == 1 ? " [side]" : " [shared]";
    if (by_shape) {
      char sfx[96];
      snprintf(sfx, sizeof(sfx), " M=%d N=%d K=%d epi=%d", g_prof.recs[i].M, g_prof.recs[i].N, g_prof.recs[i].K, g_prof.recs[i].epi);
      key += sfx;
    }
    Agg& a = agg[key];
    a.n += 1;
    a.ms += t;
    a.flops += g_prof.recs[i].flops;
  }
  if (by_symbol && cap > 0) {
    std::string out;
    for (auto& kv : agg) {
      char line[512];
      snprintf(line, sizeof(line), "%s\t%ld\t%.6f\t%.6e\n", kv.first.c_str(), kv.second.n, kv.second.ms, kv.second.flops);
      out += line;
    }
    snprintf(by_symbol, cap, "%s", out.c_str());
  }
  g_prof.recs.clear();
  return OASR_OK;
}

// Tests: one text line per launch recorded since gemm_profile_enable(1) (collect() clears them), in launch order:
// "symbol\tM\tN\tK\tta\ttb\tepilogue flag word\tsplit_k\tatomic\tatomic_on_pp\tcolsum_scratch used\tstagger\tstagger_phases\tpersistent\tlane\n".
// Does not synchronise.  Returns the number of records, or -1 when `cap` bytes do not hold them.
int gemm_profile_records(char* buf, int cap) {
  std::string out;
  for (const GemmProfile::Rec& r : g_prof.recs) {
    char line[512];
    snprintf(line, sizeof(line), "%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n", r.name, r.M, r.N, r.K, r.ta, r.tb, r.flags, r.split_k,
             r.atomic, r.atomic_on_pp, r.scratch, r.stagger, r.stagger_phases, r.persistent, r.lane);
    out += line;
  }
  if (!buf || (size_t)cap <= out.size()) return -1;
  memcpy(buf, out.c_str(), out.size() + 1);
  return (int)g_prof.recs.size();
}

void gemm_force_general(int on) { g_hooks.path = (on >= 1 && on <= 4) ? (ForcedPath)on : ForcedPath::Auto; }

// include/oasr_testing.h: gemm_route on facts given as plain integers, for a call that passes launch_gemm's argument checks.  The forced
// path and the schedule override are parameters: the process-wide hooks are not read.
extern "C" int oasr_gemm_route_debug(int M, int N, int K, int ta, int tb, int a_view, int b_view, int split_k, int atomic, int atomic_on_pp, int outputs,
                                     int sides, long long ldc, long long ldr, long long ldu, int misalign, int colsum, int colsum_scratch, int forced_path,
                                     int pp_schedule, int geom_env, char* symbol, int cap, int* post) {
  OASR_REQUIRE(symbol && cap > 0 && post, "oasr_gemm_route_debug: null output");
  OASR_REQUIRE(forced_path >= 0 && forced_path <= 4, "oasr_gemm_route_debug: forced_path %d is not a code of oasr_gemm_force_general", forced_path);
  // (the route compares pointers with null and reads their low four bits, nothing else: stand-ins that are never dereferenced)
  const uintptr_t here = 0x1000, odd = here | (uintptr_t)(misalign & 15);
  GemmArgs a = gemm_defaults();
  a.M = M, a.N = N, a.K = K, a.ta = ta, a.tb = tb;
  a.A.rpb = a_view ? 1 : 0, a.B.rpb = b_view ? 1 : 0;
  a.split_k = split_k, a.atomic = atomic, a.atomic_on_pp = atomic_on_pp;
  a.out = (outputs & 1) ? (bf16_t*)odd : nullptr;
  a.out_pre = (outputs & 2) ? (bf16_t*)odd : nullptr;
  a.out_f32 = (outputs & 4) ? (float*)here : nullptr;
  a.bias = (sides & 1) ? (const float*)here : nullptr;
  a.resid = (sides & 2) ? (const bf16_t*)odd : nullptr;
  a.dgelu_u = (sides & 4) ? (const bf16_t*)odd : nullptr;
  a.pos = (sides & 8) ? (const float*)here : nullptr;
  a.ldc = ldc, a.ldr = ldr, a.ldu = ldu;
  a.colsum = colsum ? (float*)here : nullptr;
  a.colsum_scratch = colsum_scratch ? (float*)here : nullptr;
  GemmHooks hooks;
  hooks.path = (ForcedPath)forced_path;
  hooks.pp_schedule = pp_schedule;
  const GemmRoute r = gemm_route(a, hooks, geom_env);
  const GemmKernel* k = route_kernel(a, r);
  OASR_REQUIRE(k, "oasr_gemm_route_debug: the route names a kernel that is not compiled (schedule %d)", r.pp_var);
  OASR_REQUIRE((size_t)cap > k->symbol.size(), "oasr_gemm_route_debug: %d bytes do not hold the symbol", cap);
  memcpy(symbol, k->symbol.c_str(), k->symbol.size() + 1);
  *post = (int)r.post;
  return OASR_OK;
}
