"""What SpecAugment costs, measured in one run on one GPU:

  op     ``ops.spec_augment_`` on [128, 80, 3000] under the LD policy against torch's ``masked_fill_`` with a PREBUILT boolean mask of the same
         plan (so the torch side pays neither for the plan nor for building the mask), by HIP events over windows of --calls launches,
         alternating the two
  step   one training micro-batch of --variant (--micro_batch clips, the supervised-span step) three ways, by wall time around a device
         synchronise, alternating: "off" (today's step: un-finalized log-mel, floor / scale applied by the encoder's transpose),
         "finalized" (finalized log-mel, no masks) and "LD" (finalized log-mel + spec_augment_ + the host-side cell count)
Each figure is the median of --reps repetitions after warm-up, with min and max.  Prints JSON lines and writes them to --out.

  python scripts/spec_augment_bench.py [--variant medium] [--micro_batch 32] [--reps 20] [--calls 20] [--no_step] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from olmoasr_amd import augment, ops  # noqa: E402
from olmoasr_amd.config.model_dims import VARIANT_TO_DIMS  # noqa: E402

DEV = torch.device("cuda", 0)


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1000 * (time.perf_counter() - t0)


def alternate(fns, measure, reps, warmup=3):
    out = {k: [] for k in fns}
    for r in range(warmup + reps):
        for k, fn in fns.items():
            t = measure(fn)
            if r >= warmup:
                out[k].append(t)
    return {k: stats(v) for k, v in out.items()}


def op_cost(policy, reps, calls, B=128, n_mels=80, T=3000, seed=0, first=0):
    mel = torch.randn(B, n_mels, T, device=DEV)
    mask = torch.zeros(B, n_mels, T, dtype=torch.bool)
    for b in range(B):
        f_iv, t_iv = augment.plan(policy, seed, first + b, n_mels, T)
        for s, w in f_iv:
            mask[b, s:s + w, :] = True
        for s, w in t_iv:
            mask[b, :, s:s + w] = True
    cells = int(mask.sum())
    assert cells == augment.masked_cells(policy, seed, first, B, n_mels, T)
    mask = mask.to(DEV)
    a, b_ = mel.clone(), mel.clone()
    policy.apply_(a, seed, first)
    b_.masked_fill_(mask, policy.fill)
    assert torch.equal(a, b_)  # the two sides do the same work
    rec = {"what": "op", "shape": [B, n_mels, T], "policy": "LD", "masked_cells": cells, "masked_share": round(cells / mask.numel(), 4),
           "calls_per_window": calls}
    rec.update(alternate({"native": lambda: policy.apply_(mel, seed, first), "torch_masked_fill": lambda: mel.masked_fill_(mask, policy.fill)},
                         lambda fn: window(fn, calls), reps))
    rec["native_stored_bytes"] = 4 * cells
    rec["native_store_GBps"] = round(4 * cells / (rec["native"]["median_ms"] * 1e-3) / 1e9, 1)
    return rec


def step_cost(policy, variant, mb, reps):
    from olmoasr_amd.model import OLMoASR
    from olmoasr_amd.synth import supervised_span_host, synth_samples
    net = OLMoASR(VARIANT_TO_DIMS[variant], device=DEV, seed=0)
    pcm, ti, ty, tl = synth_samples(list(range(mb)), DEV)
    span = supervised_span_host(ty.cpu(), tl.cpu())
    loss = torch.zeros(1, device=DEV)
    counter = [0]

    def step(mode):
        net.zero_grad()
        if mode == "off":
            mel, cm = ops.log_mel(pcm, finalize=False)
        else:
            mel, cm = ops.log_mel(pcm), None
            if mode == "LD":
                first = counter[0] * mb
                counter[0] += 1
                policy.apply_(mel, 0, first)
                augment.masked_cells(policy, 0, first, *mel.shape)
        net.loss_and_backward(mel, ti, ty, tl, loss_scale=65536.0, loss_out=loss, span=span, mel_clip_max=cm, span_forward=True)

    rec = {"what": "step", "variant": variant, "micro_batch": mb, "step": "log-mel + supervised-span forward / loss / backward of one micro-batch"}
    rec.update(alternate({m: (lambda m=m: step(m)) for m in ("off", "finalized", "LD")}, wall, reps))
    for m in ("finalized", "LD"):
        rec[m + "_over_off_percent"] = round(100 * (rec[m]["median_ms"] / rec["off"]["median_ms"] - 1), 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="medium")
    ap.add_argument("--micro_batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no_step", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "spec_augment.txt"))
    args = ap.parse_args()
    policy = augment.SpecAugment.preset("LD")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# scripts/spec_augment_bench.py on {torch.cuda.get_device_name(0)}: SpecAugment (LD) as an operator and inside a micro-step, "
                f"median / min / max of {args.reps} repetitions (ms)\n")
        recs = [op_cost(policy, args.reps, args.calls)]
        if not args.no_step:
            recs.append(step_cost(policy, args.variant, args.micro_batch, args.reps))
        for rec in recs:
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
