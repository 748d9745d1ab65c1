"""Times the teacher-forced score (csrc/score.hip, OLMoASR.score) against the routes it replaces, alternating on the same box:

  rows   ops.score_rows on [57344, 51968] bf16 logits, every row valid, against ops.cross_entropy_(write_grad=False) followed by
         ops.argmax_rows_ on the same logits (two passes over the matrix)
  model  OLMoASR.score at --variant, B = --batch, with the context trimmed to the batch's span and at S = 448, against model.forward plus
         torch's cross-entropy and argmax on the returned fp32 logits

Medians with (min .. max) over --reps alternating repetitions; events on the current stream."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from olmoasr_amd import ops, validation  # noqa: E402

V, VP, IGNORE = 51865, 51968, 51864


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(routes, reps):
    for fn in routes.values():  # warm-up (allocations, code objects)
        fn()
    times = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            times[k].append(timed(fn))
    return times


def show(name, ts, extra=""):
    print(f"{name}: median {statistics.median(ts):.3f} ms (min {min(ts):.3f} .. max {max(ts):.3f}, n = {len(ts)}){extra}", flush=True)


def bench_rows(reps):
    B, S = 128, 448
    rows = B * S
    lg = torch.randn(rows, VP, device="cuda", dtype=torch.bfloat16)
    tgt = torch.randint(0, 50000, (B, S), device="cuda")
    span = torch.full((B,), S, dtype=torch.int32, device="cuda")
    tab = torch.full((B, 16), 0x3fffffff, dtype=torch.int32)
    tab[:, :S // 64] = (torch.arange(B)[:, None] * S + 64 * torch.arange(S // 64)[None, :]).to(torch.int32)
    tab = tab.cuda()
    pred = torch.empty(B, S, dtype=torch.int32, device="cuda")
    ce, am = [], []

    def two_pass():
        ce.append(timed(lambda: ops.cross_entropy_(lg, V, tgt.view(-1), IGNORE, write_grad=False)))
        am.append(timed(lambda: ops.argmax_rows_(lg, V, tab, span, pred)))
    t = alternate({"score_rows": lambda: ops.score_rows(lg, V, tgt, span), "two_pass": two_pass}, reps)
    ce, am = ce[1:], am[1:]  # (the warm-up call)
    both = [a + b for a, b in zip(ce, am)]
    med = statistics.median(t["score_rows"])
    show("score_rows [57344, 51968] bf16", t["score_rows"],
         f"; {rows * 2 * V / med / 1e9:.2f} TB/s = {rows * 2 * V / med / 1e9 / 8:.2f} of 8 TB/s (2 V bytes per row)")
    show("cross_entropy_(write_grad=False)", ce, f"; {rows * 2 * V / statistics.median(ce) / 1e9 / 8:.2f} of 8 TB/s")
    show("argmax_rows_", am)
    show("two passes (sum of the two kernels)", both)
    print(f"score_rows median / two-pass minimum = {med / min(both):.3f}", flush=True)
    nll, p = ops.score_rows(lg, V, tgt, span)
    _, rl = ops.cross_entropy_(lg, V, tgt.view(-1), IGNORE, write_grad=False)
    ops.argmax_rows_(lg, V, tab, span, pred)
    print(f"agreement: pred equal {bool(torch.equal(p, pred))}, max |row_nll - row_loss| = {float((nll.view(-1) - rl).abs().max()):.2e}", flush=True)


def bench_model(variant, B, reps):
    from olmoasr_amd.config.model_dims import VARIANT_TO_DIMS
    from olmoasr_amd.model import OLMoASR
    from olmoasr_amd.synth import supervised_span_host
    net = OLMoASR(VARIANT_TO_DIMS[variant], device="cuda", seed=0)
    net.eval()
    pcm, ti, ty, tl = validation.synthetic_batch(range(4096 + 8, 4096 + 8 + B))
    span_h = supervised_span_host(ty, tl)
    St = validation.trimmed_context(span_h)
    mel = ops.log_mel(pcm.cuda())
    ti, ty, tl, span = ti.cuda(), ty.cuda(), tl.cuda(), span_h.cuda()

    def torch_route(S):
        L = net(mel, ti[:, :S], tl)
        nll = F.cross_entropy(L.view(-1, V), ty[:, :S].reshape(-1), ignore_index=IGNORE, reduction="none").view(B, S)
        return nll.sum(1), L.argmax(-1)
    routes = {f"score S={St} (trimmed)": lambda: net.score(mel, ti[:, :St], ty[:, :St], tl, span=span),
              f"forward + torch CE + argmax S={St}": lambda: torch_route(St),
              "score S=448": lambda: net.score(mel, ti, ty, tl, span=span),
              "forward + torch CE + argmax S=448": lambda: torch_route(448)}
    t = alternate(routes, reps)
    print(f"OLMoASR-{variant}, B = {B}, spans {int(span_h.min())} .. {int(span_h.max())} (sum {int(span_h.sum())} of {B * 448} positions)", flush=True)
    for k, ts in t.items():
        show(k, ts)
    a = net.score(mel, ti[:, :St], ty[:, :St], tl, span=span)
    s, _ = torch_route(St)
    print(f"agreement at S={St}: max |nll_sum - torch| / nll_sum = {float(((a.nll_sum - s).abs() / s).max()):.2e}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="rows,model")
    ap.add_argument("--variant", default="medium")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--model_reps", type=int, default=7)
    opt = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    if "rows" in opt.what:
        bench_rows(opt.reps)
    if "model" in opt.what:
        bench_model(opt.variant, opt.batch, opt.model_reps)
