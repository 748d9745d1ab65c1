"""BASELINE config 5: OLMoASR-small greedy long-form transcribe (inf_model path) on one GPU, 10 min of synthetic audio.
Random-init weights (no checkpoints offline): every window decodes the full sample_len = 224 tokens unless EOT is sampled,
i.e. the slowest case.  Prints audio-seconds per second and the per-token decode latency.
  python scripts/transcribe_bench.py [variant] [seconds] [windows per batch] [ts] [--word_timestamps] [--alignment_backend torch|native]
--word_timestamps adds the word-level alignment of every window (a scripted tokenizer: every token is one word; windows are then
sequential), --alignment_backend picks its backend (olmoasr_amd/timing.py), so the long-form line can be taken both ways."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from olmoasr_amd.config.model_dims import VARIANT_TO_DIMS  # noqa: E402
from olmoasr_amd.model import OLMoASR  # noqa: E402


# BASELINE config 5 is greedy (temperature 0, no fallback, no timestamps): the reference's defaults would walk the
# temperature tuple on a random-init model whose avg_logprob is far below the -1.0 threshold
GREEDY = dict(without_timestamps=True, temperature=0.0, logprob_threshold=None, no_speech_threshold=None)


class WordTok:
    """Scripted tokenizer with whisper's attribute names: every text token is one word."""
    eot, sot_sequence, no_timestamps, timestamp_begin = 50256, (50257,), 50362, 50363

    def decode(self, ids):
        return "".join(f" w{int(i)}" for i in ids if i < self.eot)

    def encode(self, s):
        return [int(x[1:]) for x in s.split()]

    def split_to_word_tokens(self, tokens):
        return [f" w{t}" if t < self.eot else "<|eot|>" for t in tokens], [[t] for t in tokens]


def main():
    words, backend = "--word_timestamps" in sys.argv, "torch"
    if words:
        sys.argv.remove("--word_timestamps")
    if "--alignment_backend" in sys.argv:
        at = sys.argv.index("--alignment_backend")
        backend = sys.argv[at + 1]
        del sys.argv[at:at + 2]
    variant = sys.argv[1] if len(sys.argv) > 1 else "small"
    seconds = int(sys.argv[2]) if len(sys.argv) > 2 else 600
    bw = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    opts = dict(GREEDY)
    if len(sys.argv) > 4 and sys.argv[4] == "ts":  # the reference's default: timestamp tokens on, windows strictly sequential (seek depends on them)
        opts["without_timestamps"] = False
    if words:
        opts.update(word_timestamps=True, alignment_backend=backend, tokenizer=WordTok(), compression_ratio_threshold=None)
    dev = torch.device("cuda", 0)
    net = OLMoASR(VARIANT_TO_DIMS[variant], device=dev, seed=0, inference=True)
    g = torch.Generator().manual_seed(0)
    audio = (torch.randn(seconds * 16000, generator=g) * 0.1).clamp_(-1, 1)
    net.transcribe(audio[:16000 * 60], batch_windows=bw, **opts)  # warm-up (workspaces, tables)
    torch.cuda.synchronize()
    t0 = time.time()
    out = net.transcribe(audio, batch_windows=bw, **opts)
    torch.cuda.synchronize()
    dt = time.time() - t0
    ntok = sum(len(s["tokens"]) for s in out["segments"])
    print(json.dumps({"config": f"OLMoASR-{variant} greedy transcribe, {seconds} s synthetic audio, {bw} windows per decode batch, KV cache" + (", timestamp tokens (sequential windows)" if not opts["without_timestamps"] else "") + (f", word timestamps ({backend} alignment)" if words else ""),
                      "audio_seconds_per_second": round(seconds / dt, 1), "wall_s": round(dt, 3), "windows": len(out["segments"]),
                      "tokens": ntok, "ms_per_decode_step": round(1000 * dt / max(1, ntok / (bw if opts["without_timestamps"] and not words else 1)), 3)}))


if __name__ == "__main__":
    main()
