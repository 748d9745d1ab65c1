"""The training step's weight gradients are launched as the host plan says (csrc/train_plan.h, asked through
oasr_train_wgrad_plan_debug): ties what tests/test_train_plan_cpu.py pins on the CPU to the launches of a real step."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def test_step_weight_gradients_follow_the_plan():
    """One plain fused step and one span step (default side streams) of the tiny model, B = 2: every atomic GEMM whose reduction runs over
    token rows (the conv stem's rank-B corrections reduce over B rows) went through Runner::wgrad, so its (split_k, atomic_on_pp) is the
    plan's answer for dW[M, N] over K tokens -- the conv weight gradients' window operands are plain views."""
    from olmoasr_amd import _native as N
    from olmoasr_amd import ops
    from olmoasr_amd.config.model_dims import VARIANT_TO_DIMS
    from olmoasr_amd.model import OLMoASR
    from olmoasr_amd.synth import synth_samples
    B = 2
    net = OLMoASR(VARIANT_TO_DIMS["tiny"], device=DEV, seed=0)
    pcm, ti, ty, tl = synth_samples([11, 12], DEV)
    mel = ops.log_mel(pcm)
    lib = N.lib()
    seen = {}
    for span in (None, True):
        net.zero_grad()
        lib.oasr_profile_gemm(1)
        try:
            net.loss_and_backward(mel, ti, ty, tl, loss_scale=1024.0, span=span)
            torch.cuda.synchronize()
            recs = ops.gemm_launch_records()
        finally:
            lib.oasr_profile_gemm(0)
        wgrads = [r for r in recs if r["atomic"] == 1 and r["K"] > B]
        assert wgrads and len(wgrads) < len(recs), (span, len(wgrads), len(recs))
        for r in wgrads:
            split, pp = C.c_int(-7), C.c_int(-7)
            N.check(lib.oasr_train_wgrad_plan_debug(r["K"], r["M"], r["N"], 0, C.byref(split), C.byref(pp)), "oasr_train_wgrad_plan_debug")
            assert (r["split_k"], r["atomic_on_pp"]) == (split.value, pp.value), (span, r)
            seen[split.value] = seen.get(split.value, 0) + 1
        print(f"   {'span' if span else 'plain'} step: {len(wgrads)} weight-gradient launches of {len(recs)} GEMMs, by split so far {sorted(seen.items())}")
    assert len(seen) > 1, seen  # (more than one answer was exercised)
    del net
    torch.cuda.empty_cache()
