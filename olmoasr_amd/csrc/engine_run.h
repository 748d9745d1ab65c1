// Host-side engine: workspace planning and the explicit forward / backward schedule of the OLMoASR training micro-step (the parameter
// layout it runs over is engine.hip's, its entry points are engine_step.hip / engine_decode.hip).  One header per concern:
//   engine_plan.h  the workspace plan (Plan, make_plan)        engine_side.h  the span step's side streams (SideStreams, SideMode)
//   engine_gemm.h  the GEMM calls (linear, dgrad, wgrad, ...)  engine_fwd.h   the forward schedule (block_fwd, encoder_fwd, decoder_fwd)
//   engine_bwd.h   the hand-written backward (block_bwd, backward_decoder / _encoder, train_backward)
// Runner<T> is all of them over one stream; its pure host decisions are plain C++ with CPU tests (train_plan.h).
#pragma once
#include "engine_bwd.h"

namespace {

// One call's workspace plan and runner.  A training plan's runner saves GELU'(u), sums bias gradients through the plan's scratch and sends
// adapted weights' gradients to the plan's (Runner::train / cs_scratch / lora_dw).  A null workspace is a dry run: A.cur is the plan's size.
template <typename T>
struct Step {
  Arena A;
  Plan<T> p;
  Runner<T> r;
  Step(const oasr_ctx* c, void* workspace, size_t bytes, void* stream, int B, int S, const int32_t* text_len, bool train, int stage = STAGE_ALL)
      : A(workspace, bytes), r(c, (hipStream_t)stream, B, S, text_len) {
    make_plan(c, A, p, B, S, train, stage);
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
