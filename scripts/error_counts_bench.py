"""Measurements behind DESIGN.md section 3i (profiles/train_error_counts.txt), on one MI355X:

  step     a LOGGING optimizer step's micro-batches (log-mel, forward, loss, backward, predictions, error counts read on the host) two
           ways in the same process, alternating: the host path (plain step, fp32 logits, gen_pred, token_error_rate) and the device path
           (span step with pred_out, metrics.ErrorCounter).  Host clock around work that ends in a device synchronise; peak device memory
           from torch's allocator statistics.
  kernels  the argmax pass (oasr_test_argmax_rows on a bf16 [B * len, 51968] matrix) and ops.edit_counts alone, HIP events over --reps
           launches after a warm-up.

    python scripts/error_counts_bench.py --variant medium --batch 128 --micro 2 --rounds 3
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
V, LD = 51865, 51968


def train_script():
    spec = importlib.util.spec_from_file_location("tt_bench", os.path.join(ROOT, "scripts", "training", "train_timestamps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def bench_step(args):
    from olmoasr_amd import metrics, ops
    from olmoasr_amd.config.model_dims import VARIANT_TO_DIMS
    from olmoasr_amd.model import OLMoASR
    from olmoasr_amd.synth import synth_samples
    tt = train_script()
    dev = torch.device("cuda")
    net = OLMoASR(VARIANT_TO_DIMS[args.variant], device=dev, seed=0)
    B, n_micro = args.batch, args.micro
    batches = [synth_samples(list(range(m * B, (m + 1) * B)), dev) for m in range(n_micro)]
    spans = [net.supervised_span(ty, tl) for _, _, ty, tl in batches]
    loss_buf = torch.zeros(1, device=dev)
    pred_buf = torch.empty(B, net.dims.n_text_ctx, dtype=torch.int32, device=dev)
    counter = metrics.ErrorCounter(dev)

    def host_path():
        preds, tgts = [], []
        net.zero_grad()
        for i, (pcm, ti, ty, tl) in enumerate(batches):
            _, logits = net.loss_and_backward(ops.log_mel(pcm), ti, ty, tl, accumulation_steps=n_micro, loss_out=loss_buf, accumulate_loss=i > 0,
                                              return_logits=True)
            p, t = tt.gen_pred(logits, ty)
            preds += p
            tgts += t
        torch.cuda.synchronize()
        t_gpu = time.perf_counter()
        errs, n = tt.token_error_counts(preds, tgts)
        return float(loss_buf), errs, n, t_gpu

    def device_path():
        net.zero_grad()
        counter.reset()
        for i, (pcm, ti, ty, tl) in enumerate(batches):
            mel, cm = ops.log_mel(pcm, finalize=False)
            net.loss_and_backward(mel, ti, ty, tl, accumulation_steps=n_micro, loss_out=loss_buf, accumulate_loss=i > 0, span=spans[i],
                                  mel_clip_max=cm, pred_out=pred_buf)
            counter.add(pred_buf, ty)
        vals = torch.cat([loss_buf.double(), counter.total.double()]).cpu().tolist()  # the one read
        errs, n = metrics.ErrorCounter.fraction([int(v) for v in vals[1:]])
        return vals[0], errs, n, [int(v) for v in vals[1:]]

    out = {"variant": args.variant, "clips": B * n_micro, "micro_batches": n_micro, "host": [], "device": []}
    for name, fn in (("device", device_path), ("host", host_path)):  # warm-up of every shape either path uses
        fn()
        torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, fn in (("host", host_path), ("device", device_path)):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            rec = {"ms": round((t1 - t0) * 1e3, 2), "peak_GB": round(torch.cuda.max_memory_allocated() / 1e9, 3), "loss": res[0], "errors": res[1],
                   "ref_tokens": res[2]}
            if name == "host":
                rec["ms_gpu_part"] = round((res[3] - t0) * 1e3, 2)  # up to the last synchronise, before the Python edit-distance loop
            else:
                rec["S_D_I_H"] = res[3]
            out[name].append(rec)
            print(json.dumps({"path": name, **rec}), flush=True)
    for name in ("host", "device"):
        out[name + "_median_ms"] = statistics.median(r["ms"] for r in out[name])
    print(json.dumps({"summary": "logging step", **{k: v for k, v in out.items() if not isinstance(v, list)}}), flush=True)


def events_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def bench_kernels(args):
    from olmoasr_amd import ops
    dev = torch.device("cuda")
    B, S = args.pairs, 448
    g = torch.Generator(device=dev).manual_seed(0)
    for length in (224, 448):
        n64 = (length + 63) // 64 * 64
        rows = B * n64
        mat = torch.empty(rows, LD, dtype=torch.bfloat16, device=dev)
        for r0 in range(0, rows, 8192):  # (filled in slabs: no fp32 copy of the whole matrix)
            mat[r0:r0 + 8192] = torch.randn(min(8192, rows - r0), LD, device=dev, generator=g).to(torch.bfloat16)
        # the span step's own layout: position-block-major active chunks
        tab = torch.full((B, 16), 0x3fffffff, dtype=torch.int32)
        for c in range(n64 // 64):
            tab[:, c] = 64 * (c * B + torch.arange(B, dtype=torch.int32))
        tab, span = tab.to(dev), torch.full((B,), n64, dtype=torch.int32, device=dev)
        pred = torch.empty(B, S, dtype=torch.int32, device=dev)
        med, lo, hi = events_ms(lambda: ops.argmax_rows_(mat, V, tab, span, pred), args.reps)
        want = torch.argmax(mat[:4096, :V].float(), dim=1).cpu()  # spot check of the first chunk rows
        got = pred[:, :64].cpu()
        ok = all(int(got[b, s]) == int(want[64 * b + s]) for b in range(min(B, 64)) for s in range(64))
        print(json.dumps({"kernel": "argmax_rows", "pairs": B, "length": length, "active_rows": rows, "ms": round(med, 4), "ms_min": round(lo, 4),
                          "ms_max": round(hi, 4), "TB_per_s": round(rows * V * 2 / (med * 1e-3) / 1e12, 3), "matches_torch_argmax": ok}), flush=True)
        del mat
        hyp = torch.randint(0, 50, (B, length), device=dev, dtype=torch.int32, generator=g)
        ref = hyp.clone()
        noise = torch.rand(B, length, device=dev, generator=g) < 0.2
        ref[noise] = torch.randint(0, 50, (int(noise.sum()),), device=dev, dtype=torch.int32, generator=g)
        ln = torch.full((B,), length, dtype=torch.int32, device=dev)
        out = torch.empty(B, 4, dtype=torch.int32, device=dev)
        med, lo, hi = events_ms(lambda: ops.edit_counts(hyp, ln, ref, ln, out=out), args.reps)
        same = torch.equal(out.cpu(), ops.edit_counts_host(hyp.cpu(), ln.cpu(), ref.cpu(), ln.cpu()))
        print(json.dumps({"kernel": "edit_counts", "pairs": B, "length": length, "ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                          "cells_per_s": round(B * length * length / (med * 1e-3), 0), "equals_host_twin": same}), flush=True)
        t0 = time.perf_counter()
        ops.edit_counts_host(hyp.cpu(), ln.cpu(), ref.cpu(), ln.cpu())
        print(json.dumps({"host_twin": "edit_counts_host", "pairs": B, "length": length, "ms_cpu": round((time.perf_counter() - t0) * 1e3, 2)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="step,kernels")
    ap.add_argument("--variant", default="medium")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--micro", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this is a GPU measurement: no device, no number"
    if "kernels" in a.what:
        bench_kernels(a)
    if "step" in a.what:
        bench_step(a)
