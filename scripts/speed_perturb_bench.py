"""What speed perturbation costs, measured in one run on one GPU:

  op     ``ops.speed_perturb`` on int16 [128, 480000] (--batch, --samples) with the timestamp tokens of two [128, 448] tensors, by HIP events over
         windows of --calls launches, for the 3-way policy (a third of the clips each at 9/10, 1/1, 11/10 -- about a fifth of the slow-downs
         fall back to the copy), for every clip at 11/10, every clip at 9/10 and every clip copied, alternating; beside it ``ops.log_mel`` on
         the same batch, the front end the augmentation sits ahead of.
Each figure is the median of --reps repetitions after warm-up, with min and max, and is reported per clip and as the share of 8 TB/s that one
read plus one write of the PCM (2 x 2 N bytes per clip: the operator's floor) would reach in that time.  Prints JSON lines and writes them
to --out.

  python scripts/speed_perturb_bench.py [--batch 128] [--samples 480000] [--reps 20] [--calls 10] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from olmoasr_amd import augment, ops  # noqa: E402

DEV = torch.device("cuda", 0)
PEAK_BYTES_PER_S = 8e12


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


def op_cost(B, N, reps, calls, seed=0, first=0):
    g = torch.Generator().manual_seed(0)
    pcm = (torch.randn(B, N, generator=g) * 3276.7).round().clamp(-32768, 32767).to(torch.int16)
    n_valid_host = torch.randint(N // 2, N + 1, (B,), generator=g, dtype=torch.int64).to(torch.int32)  # the synthetic clips' 15 .. 30 s
    for b in range(B):
        pcm[b, int(n_valid_host[b]):] = 0
    pcm, n_valid = pcm.to(DEV), n_valid_host.to(DEV)
    out = torch.empty_like(pcm)
    tok = torch.randint(50257, 51865, (2, B, 448), generator=g, dtype=torch.int64).to(DEV)
    policies = {"3way": augment.SpeedPerturb.preset("3way"), "all_11_10": augment.SpeedPerturb(factors=((11, 10),)),
                "all_9_10": augment.SpeedPerturb(factors=((9, 10),)), "copy": augment.SpeedPerturb(factors=((1, 1),))}
    # the two sides of the contract once, before timing: the device equals the host twin on the first clips
    want = ops.speed_perturb_host(pcm[:2].cpu(), n_valid_host[:2], factors=policies["3way"].factors, seed=seed, first_clip=first)
    got = policies["3way"].apply(pcm[:2], n_valid[:2], seed, first)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(got, want))
    fns = {k: (lambda p=p: p.apply(pcm, n_valid, seed, first, tokens=(tok[0], tok[1]), out=out)) for k, p in policies.items()}
    fns["log_mel"] = lambda: ops.log_mel(pcm)
    rec = {"what": "op", "shape": [B, N], "calls_per_window": calls, "floor_bytes_per_clip": 4 * N,
           "factor_counts_3way": policies["3way"].factor_counts(seed, first, n_valid_host.tolist(), N)}
    rec.update(alternate(fns, lambda fn: window(fn, calls), reps))
    for k in fns:
        us = 1000 * rec[k]["median_ms"] / B
        rec[k]["us_per_clip"] = round(us, 3)
        if k != "log_mel":
            rec[k]["share_of_8TBps"] = round(4 * N / (us * 1e-6) / PEAK_BYTES_PER_S, 4)
    rec["3way_over_log_mel"] = round(rec["3way"]["median_ms"] / rec["log_mel"]["median_ms"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--samples", type=int, default=480000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "speed_perturb.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# scripts/speed_perturb_bench.py on {torch.cuda.get_device_name(0)}: speed perturbation as an operator, median / min / max of "
                f"{args.reps} repetitions (ms per launch of the whole batch)\n")
        line = json.dumps(op_cost(args.batch, args.samples, args.reps, args.calls))
        print(line, flush=True)
        f.write(line + "\n")


if __name__ == "__main__":
    main()
