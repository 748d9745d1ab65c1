"""What noise mixing costs, measured in one run on one GPU:

  op     ``ops.noise_mix`` on int16 [128, 480000] (--batch, --samples) against a bank of --rows recordings of the same length, by HIP events
         over windows of --calls calls, with every clip drawn (prob = 1), out of place and in place, and with no clip drawn (prob = 0: a copy,
         and in place nothing at all); beside it, in the same alternating loop, ``ops.speed_perturb`` (3way) and ``ops.log_mel`` on the same
         batch -- the stages before and after it.
Each figure is the median of --reps repetitions after warm-up, with min and max, and is reported per clip and as the share of 8 TB/s by the
algorithmic bytes of a mixed clip: x and v read twice (energies, then the mix) and y written once, 10 bytes per valid sample (and a plain
copy, 4 bytes, of the padding behind it).  Prints JSON lines and writes them to --out.

  python scripts/noise_mix_bench.py [--batch 128] [--samples 480000] [--rows 16] [--reps 20] [--calls 10] [--out FILE]"""
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


def op_cost(B, N, M, reps, calls, full, seed=0, first=0):
    g = torch.Generator().manual_seed(0)
    pcm = (torch.randn(B, N, generator=g) * 3276.7).round().clamp(-32768, 32767).to(torch.int16)
    if full:
        n_valid_host = torch.full((B,), N, dtype=torch.int32)
    else:
        n_valid_host = torch.randint(N // 2, N + 1, (B,), generator=g, dtype=torch.int64).to(torch.int32)  # the synthetic clips' 15 .. 30 s
    for b in range(B):
        pcm[b, int(n_valid_host[b]):] = 0
    bank = (torch.randn(M, N, generator=g) * 1000).round().clamp(-32768, 32767).to(torch.int16)
    # the two sides of the contract once, before timing: the device equals the host twin on the first clips
    want = ops.noise_mix_host(pcm[:2], n_valid_host[:2], bank, prob=1.0, snr_db=(5, 20), seed=seed, first_clip=first)
    pcm, n_valid, bank = pcm.to(DEV), n_valid_host.to(DEV), bank.to(DEV)
    got = ops.noise_mix(pcm[:2], n_valid[:2], bank, prob=1.0, snr_db=(5, 20), seed=seed, first_clip=first)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(got, want)) and all(r >= 0 for r in want[1].tolist())
    out, work = torch.empty_like(pcm), pcm.clone()
    every, none = augment.NoiseMix(prob=1.0, snr_db=(5, 20)), augment.NoiseMix(prob=0.0, snr_db=(5, 20))
    speed = augment.SpeedPerturb.preset("3way")
    fns = {"mix": lambda: every.apply(pcm, n_valid, bank, seed, first, out=out),
           "mix_in_place": lambda: every.apply(work, n_valid, bank, seed, first, out=work),  # (its own buffer: the noise piles up there, the cost does not change)
           "copy": lambda: none.apply(pcm, n_valid, bank, seed, first, out=out),
           "nothing_in_place": lambda: none.apply(work, n_valid, bank, seed, first, out=work),
           "speed_3way": lambda: speed.apply(pcm, n_valid, seed, first, out=out),
           "log_mel": lambda: ops.log_mel(pcm)}
    valid = float(n_valid_host.double().mean())
    bytes_mixed = 10 * valid + 4 * (N - valid)
    rec = {"what": "op", "shape": [B, N], "bank": [M, N], "n_valid_mean": round(valid, 1), "calls_per_window": calls,
           "algorithmic_bytes_per_mixed_clip": round(bytes_mixed)}
    rec.update(alternate(fns, lambda fn: window(fn, calls), reps))
    for k in fns:
        us = 1000 * rec[k]["median_ms"] / B
        rec[k]["us_per_clip"] = round(us, 3)
        if k.startswith("mix"):
            rec[k]["share_of_8TBps"] = round(bytes_mixed / (us * 1e-6) / PEAK_BYTES_PER_S, 4)
    rec["mix_over_log_mel"] = round(rec["mix"]["median_ms"] / rec["log_mel"]["median_ms"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--samples", type=int, default=480000)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "noise_mix.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# scripts/noise_mix_bench.py on {torch.cuda.get_device_name(0)}: noise mixing as an operator beside speed perturbation and the log-mel, "
                f"median / min / max of {args.reps} repetitions (ms per call on the whole batch)\n")
        for full in (True, False):  # every clip 30 s long (N valid samples: 10 bytes per sample throughout), then the synthetic clips' 15 .. 30 s
            line = json.dumps(op_cost(args.batch, args.samples, args.rows, args.reps, args.calls, full))
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
