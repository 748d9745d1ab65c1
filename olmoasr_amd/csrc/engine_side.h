// Side streams of the supervised-span step: the stream a runner launches on, and the fork / join bookkeeping of the two lowest-priority streams
// that take the decoder's filler work (oasr_ctx::Side).  No launch is decided here: the schedules (engine_fwd.h, engine_bwd.h) say what goes where.
//
// The decoder-side GEMMs of a span step run over R ~ 18.7k rows: 292 tiles of 256 x 256 for an N = 1024 output = 1.14 rounds over the 256
// CUs, the second round 14 % full.  A weight gradient and the data gradient launched after it are independent (both read dy), so the
// weight gradients go to a second, lowest-priority stream whose workgroups take the CUs the main stream's tails leave idle; the main
// stream waits for them (join_side) before the LayerNorm backward that ends each section of block_bwd -- the next kernel that may
// overwrite something a weight gradient reads -- so the per-block events (DDP buckets) still mean "this block's gradients are complete".
// The encoder-sized GEMMs of the cross-attention key|value side (the projection of xa in the forward -- it depends on the encoder output
// only, so all L_dec of them are issued when the decoder starts; its weight gradient and d(xa) in the backward) run on a second side
// stream the same way: short workgroups by the thousand, the filler for every tail of the decoder's own launches.
#pragma once
#include "engine_ctx.h"

namespace {

// Runner::side_mode (oasr_span_set_side_streams, OASR_SIDE_STREAMS): which work of a span step leaves the main stream
enum SideMode : int {
  SIDE_WGRAD = 1,        // the decoder backward's weight gradients over the R active rows: Side::stream, joined before each LayerNorm backward
  SIDE_KV_FWD = 2,       // the forward's key|value projections of xa: Side::big, every layer's issued when the decoder starts (Side::kv_ready)
  SIDE_KV_BWD = 4,       // the backward's key|value weight gradient and d(xa): Side::big, joined before the block's event
  SIDE_KV_INFLIGHT = 8,  // experiments without segment events: that join waits until the next block's attention backward needs p.gkv
  SIDE_ALL = 15,
};

// The GEMM launch statistics' lane tag (gemm_profile_lane) is process-wide: a step that changes it puts it back to its value on entry
// when its scope ends, on every path -- an early error return must not leave every later launch of the process mislabelled.
struct LaneScope {
  const int entry = gemm_profile_lane(-1);
  ~LaneScope() { gemm_profile_lane(entry); }
};

struct SideStreams {
  const oasr_ctx* c;
  hipStream_t st;  // where the next launch goes
  int side_mode = 0;
  bool side_pending = false, big_pending = false;
  LaneScope lane;  // (decoder_fwd tags the main stream "[shared]" while side-stream filler is in flight)
  SideStreams(const oasr_ctx* c_, hipStream_t st_) : c(c_), st(st_) {}

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
        nw.destroy();
        return rc;
      }
      sd = nw;
    }
    side_mode = mode;
    return OASR_OK;
  }
  // the side streams have drained: what follows has the chip to itself (the encoder's 192k-row GEMMs fill it on their own)
  void side_end() {
    side_mode = 0;
    gemm_profile_lane(lane.entry);
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
  // the main stream waits for what is pending on a side stream (nothing pending: nothing happens)
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
};

}  // namespace
