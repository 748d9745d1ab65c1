"""Word-timestamp alignment of ONE 30 s window, both backends of ``timing.find_alignment`` timed in the same run on the same GPU:
"torch" (torch ops + host DTW) and "native" (``ops.alignment_matrix`` + ``ops.dtw``, csrc/align.hip).

For every model variant's default alignment heads (all heads of the upper half of the decoder), at n_tok tokens x 1500 frames:
  matrix   score planes -> [n_tok, 1500] matrix alone, by HIP events (synthetic planes of the variant's shape; no model needed)
  dtw      the path from that matrix alone, wall time including its synchronisation and copies
  whole    ``find_alignment`` on a random-weight model of the variant (two decoder passes + the two steps above), wall time
Each figure is the median of --reps repetitions after warm-up, with min and max.  Prints one JSON line per (variant, n_tok) and writes the
same lines to --out.

  python scripts/align_bench.py [--variants tiny,base,small,medium,large] [--n_tok 32,128,448] [--reps 20] [--no_whole] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from olmoasr_amd import ops, timing  # noqa: E402
from olmoasr_amd.config.model_dims import VARIANT_TO_DIMS  # noqa: E402

DEV = torch.device("cuda", 0)
N_SOT = 1


class WordTok:
    """Scripted tokenizer with whisper's attribute names: every text token is one word."""
    eot, sot_sequence, no_timestamps, timestamp_begin = 50256, (50257,), 50362, 50363

    def decode(self, ids):
        return "".join(f" w{int(i)}" for i in ids if i < self.eot)

    def encode(self, s):
        return [int(x[1:]) for x in s.split()]

    def split_to_word_tokens(self, tokens):
        return [f" w{t}" if t < self.eot else "<|eot|>" for t in tokens], [[t] for t in tokens]


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def by_events(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return stats(out)


def by_wall(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1000 * (time.perf_counter() - t0))
    return stats(out)


def planes(dims, n_tok):
    """Synthetic score planes of the variant's upper decoder half: randn * 3 with a diagonal ridge, so that the matrix has a path to find."""
    g = torch.Generator(device=DEV).manual_seed(n_tok)
    layers = list(range(dims.n_text_layer // 2, dims.n_text_layer))
    i = torch.arange(n_tok, device=DEV)
    qks = {}
    for l in layers:
        q = torch.randn(dims.n_text_head, n_tok, 1500, device=DEV, generator=g) * 3
        q[:, i, (i * 1500) // n_tok] += 6.0
        qks[l] = q
    return qks, [(l, h) for l in layers for h in range(dims.n_text_head)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="tiny,base,small,medium,large")
    ap.add_argument("--n_tok", default="32,128,448")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no_whole", action="store_true", help="skip find_alignment as a whole (it builds a random-weight model per variant)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "alignment_native.txt"))
    args = ap.parse_args()
    reps = max(20, args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# scripts/align_bench.py on {torch.cuda.get_device_name(0)}: one window's word-timestamp alignment, torch vs native backend, "
                f"median / min / max of {reps} repetitions (ms)\n")
        for variant in args.variants.split(","):
            dims = VARIANT_TO_DIMS[variant]
            net = None
            if not args.no_whole:
                from olmoasr_amd.model import OLMoASR
                net = OLMoASR(dims, device=DEV, seed=0, inference=True)
                mel = torch.randn(80, 3000, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)) * 0.3
                xa = net.embed_audio(mel[None])
            for n_tok in (int(x) for x in args.n_tok.split(",")):
                qks, heads = planes(dims, n_tok)
                layers = sorted(qks)
                hpl = [[h for ll, h in heads if ll == l] for l in layers]
                rec = {"variant": variant, "heads": len(heads), "n_tok": n_tok, "frames": 1500}
                rec["matrix_torch"] = by_events(lambda: timing.alignment_matrix_torch(qks, heads, 1500, 7, 1.0), reps)
                rec["matrix_native"] = by_events(lambda: ops.alignment_matrix([qks[l] for l in layers], hpl, 1500, 7, 1.0), reps)
                m_t = timing.alignment_matrix_torch(qks, heads, 1500, 7, 1.0)
                m_n = ops.alignment_matrix([qks[l] for l in layers], hpl, 1500, 7, 1.0)
                rec["matrix_max_abs_diff"] = float((m_t - m_n).abs().max())
                rec["dtw_torch"] = by_wall(lambda: timing.dtw(-m_t[N_SOT:-1].double().cpu().numpy()), reps)
                rec["dtw_native"] = by_wall(lambda: ops.dtw(m_n[N_SOT:-1], negate=True), reps)
                del qks, m_t, m_n
                if net is not None:
                    text = [1000 + 7 * k for k in range(n_tok - N_SOT - 2)]
                    for backend in timing.BACKENDS:
                        rec["whole_" + backend] = by_wall(lambda: timing.find_alignment(net, WordTok(), text, None, 3000, backend=backend,
                                                                                        audio_features=xa), reps)
                line = json.dumps(rec)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()
            del net
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
