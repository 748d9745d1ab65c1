"""Per-token wall time of ``decode`` with beam search (beam 5, what the reference evaluates with), for the two beam backends: "host"
(BeamSearchDecoder.update in Python, four device -> host copies per token) and "native" (``ops.beam_update`` + ``kv_cache_reorder_native``,
csrc/beam.hip; the host reads the status words every 8th step).

Random-weight models of --variants on the bf16 engine, 1 and 8 windows of already-encoded audio, a fixed sample_len of 64 without
timestamps; a positive finite ``suppress_mask`` bias on 64 text tokens keeps eot from winning, so every decode runs its full length.  Each
figure is the median of --reps decodes after warm-up, with min and max, divided by the 64 tokens.  Prints one JSON line per (variant,
windows) and appends the same lines to --out.

The script runs unchanged against an older tree (``--tree DIR``: the checkout whose ``olmoasr_amd`` is imported): it passes ``beam_backend``
only when native is asked for, so a tree from before the option gives the baseline series.

  python scripts/beam_bench.py [--beam_backend host|native] [--variants tiny,medium] [--windows 1,8] [--reps 10] [--tree DIR] [--label NAME] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE_LEN, BEAM = 64, 5


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beam_backend", default="host", choices=("host", "native"))
    ap.add_argument("--variants", default="tiny,medium")
    ap.add_argument("--windows", default="1,8")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tree", default=HERE, help="the checkout whose olmoasr_amd is measured (its library must be built)")
    ap.add_argument("--label", default=None, help="what the lines are tagged with (default: the backend)")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "beam_native.txt"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from olmoasr_amd.config.model_dims import VARIANT_TO_DIMS
    from olmoasr_amd.decoding import DecodingOptions, decode
    from olmoasr_amd.model import OLMoASR
    dev = torch.device("cuda", 0)
    extra = {"beam_backend": "native"} if args.beam_backend == "native" else {}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for variant in args.variants.split(","):
            dims = VARIANT_TO_DIMS[variant]
            net = OLMoASR(dims, device=dev, seed=0, inference=True)
            bias = torch.zeros(dims.n_vocab)
            bias[1000:1064] = 30.0
            opts = DecodingOptions(sample_len=SAMPLE_LEN, beam_size=BEAM, without_timestamps=True, suppress_mask=bias, **extra)
            for n in (int(x) for x in args.windows.split(",")):
                mel = torch.randn(n, 80, 3000, device=dev, generator=torch.Generator(device=dev).manual_seed(n)) * 0.3
                xa = net.embed_audio(mel)
                ms, lengths = [], set()
                for rep in range(args.warmup + args.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = decode(net, xa, opts)
                    torch.cuda.synchronize()
                    if rep >= args.warmup:
                        ms.append(1000 * (time.perf_counter() - t0) / SAMPLE_LEN)
                    lengths |= {len(r.tokens) for r in out}
                assert lengths == {SAMPLE_LEN}, f"a decode stopped early ({sorted(lengths)} tokens): the figures would not be per token"
                rec = {"label": args.label or args.beam_backend, "variant": variant, "windows": n, "beam": BEAM, "sample_len": SAMPLE_LEN,
                       "reps": args.reps, "per_token": stats(ms), "device": torch.cuda.get_device_name(0)}
                line = json.dumps(rec)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()
            del net
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
