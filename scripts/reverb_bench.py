"""What reverberation costs, measured in one run on one GPU:

  op     ``ops.reverb`` on int16 [128, 480000] (--batch, --samples) against a bank of --rows seeded synthetic room responses of K = 1024, 4096
         and 8192 taps (--taps), by HIP events over windows of --calls calls, with every clip drawn (prob = 1; both launches: the expansion of
         the bank and the convolution) and with no clip drawn (prob = 0: the expansion and a copy); beside it, in the same alternating loop,
         ``ops.log_mel`` and ``ops.noise_mix`` on the same batch as yardsticks.
Each figure is the median of --reps repetitions after warm-up, with min and max, and is reported per clip and as the share of the dense int8
matrix-core peak (--peak_ops, 5e15 op/s) by 8 N (K + 64) operations per clip: four byte products of two operations per (sample, tap), the
taps rounded up to the 64-wide k-step the MFMA takes.  Prints JSON lines and writes them to --out.

  python scripts/reverb_bench.py [--batch 128] [--samples 480000] [--rows 16] [--taps 1024,4096,8192] [--reps 20] [--calls 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from olmoasr_amd import augment, ops  # noqa: E402

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


def alternate(fns, measure, reps, warmup=3):
    out = {k: [] for k in fns}
    for r in range(warmup + reps):
        for k, fn in fns.items():
            t = measure(fn)
            if r >= warmup:
                out[k].append(t)
    return {k: stats(v) for k, v in out.items()}


def responses(R, K, seed):
    """Seeded synthetic rooms: a direct path after a few samples, then exponentially decaying noise."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(R):
        h = rng.standard_normal(K) * 0.2 * np.exp(-np.arange(K) / (K / 3.0))
        h[:8 + i] *= 0.05
        h[8 + i] = 1.0
        out.append(h)
    return out


def op_cost(B, N, R, K, reps, calls, peak, seed=0, first=0):
    g = torch.Generator().manual_seed(0)
    pcm = (torch.randn(B, N, generator=g) * 3276.7).round().clamp(-32768, 32767).to(torch.int16)
    n_valid_host = torch.full((B,), N, dtype=torch.int32)
    bank, delay = augment.rir_bank(responses(R, K, 1))
    noise_bank = (torch.randn(R, N, generator=g) * 1000).round().clamp(-32768, 32767).to(torch.int16).to(DEV)
    # the two sides of the contract once, before timing: the device equals the host twin on the head of the first clips
    head = 3 * 4096 + 77
    short = torch.tensor([head, head // 2], dtype=torch.int32)
    want = ops.reverb_host(pcm[:2, :head].contiguous(), short, bank, delay, prob=1.0, seed=seed, first_clip=first)
    pcm, n_valid, bank, delay = pcm.to(DEV), n_valid_host.to(DEV), bank.to(DEV), delay.to(DEV)
    got = ops.reverb(pcm[:2, :head], short.to(DEV), bank, delay, prob=1.0, seed=seed, first_clip=first)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(got, want)) and all(r >= 0 for r in want[1].tolist())
    out = torch.empty_like(pcm)
    every, none = augment.Reverb(prob=1.0), augment.Reverb(prob=0.0)
    noise = augment.NoiseMix(prob=1.0, snr_db=(5, 20))
    fns = {"reverb": lambda: every.apply(pcm, n_valid, bank, delay, seed, first, out=out),
           "copy": lambda: none.apply(pcm, n_valid, bank, delay, seed, first, out=out),
           "log_mel": lambda: ops.log_mel(pcm),
           "noise_mix": lambda: noise.apply(pcm, n_valid, noise_bank, seed, first, out=out)}
    ops_per_clip = 8 * N * (K + 64)
    rec = {"what": "op", "shape": [B, N], "bank": [R, K], "calls_per_window": calls, "int8_ops_per_clip": ops_per_clip, "peak_ops_per_s": peak}
    rec.update(alternate(fns, lambda fn: window(fn, calls), reps))
    for k in fns:
        us = 1000 * rec[k]["median_ms"] / B
        rec[k]["us_per_clip"] = round(us, 3)
    rec["reverb"]["share_of_int8_peak"] = round(ops_per_clip / (rec["reverb"]["us_per_clip"] * 1e-6) / peak, 4)
    rec["reverb_over_log_mel"] = round(rec["reverb"]["median_ms"] / rec["log_mel"]["median_ms"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--samples", type=int, default=480000)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--taps", default="1024,4096,8192")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--peak_ops", type=float, default=5e15)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "reverb.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# scripts/reverb_bench.py on {torch.cuda.get_device_name(0)}: reverberation as an operator beside the log-mel and noise mixing, "
                f"median / min / max of {args.reps} repetitions (ms per call on the whole batch)\n")
        for K in (int(k) for k in args.taps.split(",")):
            line = json.dumps(op_cost(args.batch, args.samples, args.rows, K, args.reps, args.calls, args.peak_ops))
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
