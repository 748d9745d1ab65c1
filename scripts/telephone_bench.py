"""What the telephone channel costs, measured in one run on one GPU:

  op     ``ops.telephone`` on int16 [256, 480000] (--batch, --samples), by HIP events over windows of --calls calls: every clip drawn
         (prob = 1) through mu-law with the band-pass, through the three codecs drawn per clip, without the band-pass (decimate, compand,
         interpolate), and with no clip drawn (prob = 0: a copy); beside it, in the same alternating loop, ``ops.log_mel`` on the same
         batch -- the stage after it.
Each figure is the median of --reps repetitions after warm-up, with min and max, and is reported per clip, as the ratio to the log-mel, and
as the share of 8 TB/s by the operator's algorithmic bytes: every sample read once and written once, 4 bytes per sample.  Prints JSON lines
and writes them to --out.

  python scripts/telephone_bench.py [--batch 256] [--samples 480000] [--reps 20] [--calls 10] [--out FILE]"""
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


def op_cost(B, N, reps, calls, full, seed=0, first=0):
    g = torch.Generator().manual_seed(0)
    pcm = (torch.randn(B, N, generator=g) * 3276.7).round().clamp(-32768, 32767).to(torch.int16)
    if full:
        n_valid_host = torch.full((B,), N, dtype=torch.int32)
    else:
        n_valid_host = torch.randint(N // 2, N + 1, (B,), generator=g, dtype=torch.int64).to(torch.int32)  # the synthetic clips' 15 .. 30 s
    for b in range(B):
        pcm[b, int(n_valid_host[b]):] = 0
    # the two sides of the contract once, before timing: the device equals the host twin on the first clips
    want = ops.telephone_host(pcm[:2], n_valid_host[:2], prob=1.0, seed=seed, first_clip=first)
    pcm, n_valid = pcm.to(DEV), n_valid_host.to(DEV)
    got = ops.telephone(pcm[:2], n_valid[:2], prob=1.0, seed=seed, first_clip=first)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(got, want)) and all(c >= 0 for c in want[1].tolist())
    out = torch.empty_like(pcm)
    mulaw, three = augment.TelephoneChannel(prob=1.0, codecs=("mulaw",)), augment.TelephoneChannel(prob=1.0)
    narrow, none = augment.TelephoneChannel(prob=1.0, codecs=("mulaw",), bandpass=False), augment.TelephoneChannel(prob=0.0)
    fns = {"telephone": lambda: mulaw.apply(pcm, n_valid, seed, first, out=out),
           "telephone_three_codecs": lambda: three.apply(pcm, n_valid, seed, first, out=out),
           "telephone_no_bandpass": lambda: narrow.apply(pcm, n_valid, seed, first, out=out),
           "copy": lambda: none.apply(pcm, n_valid, seed, first, out=out),
           "log_mel": lambda: ops.log_mel(pcm)}
    rec = {"what": "op", "shape": [B, N], "n_valid_mean": round(float(n_valid_host.double().mean()), 1), "calls_per_window": calls,
           "algorithmic_bytes_per_clip": 4 * N}
    rec.update(alternate(fns, lambda fn: window(fn, calls), reps))
    for k in fns:
        us = 1000 * rec[k]["median_ms"] / B
        rec[k]["us_per_clip"] = round(us, 3)
        if k != "log_mel":
            rec[k]["share_of_8TBps"] = round(4 * N / (us * 1e-6) / PEAK_BYTES_PER_S, 4)
    rec["telephone_over_log_mel"] = round(rec["telephone"]["median_ms"] / rec["log_mel"]["median_ms"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--samples", type=int, default=480000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "telephone.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# scripts/telephone_bench.py on {torch.cuda.get_device_name(0)}: the telephone channel as an operator beside the log-mel, "
                f"median / min / max of {args.reps} repetitions (ms per call on the whole batch)\n")
        for full in (True, False):  # every clip 30 s long, then the synthetic clips' 15 .. 30 s
            line = json.dumps(op_cost(args.batch, args.samples, args.reps, args.calls, full))
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
