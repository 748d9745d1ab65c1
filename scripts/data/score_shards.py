"""Model-based quality scores of (audio, transcript) pairs: every sample of a shard directory is scored by a trained model with
``OLMoASR.score`` (teacher-forced, forward only) and one JSON line per sample is written IN SHARD ORDER (the order of
``data.load_samples_dicts``):

    {"index", "audio_file", "nll_sum", "n_tok", "n_hit", "nll_max", "mean_nll"}

``mean_nll`` = nll_sum / n_tok (null for a sample without a valid target) is how well the model explains the transcript given the audio: a
curation signal beside the text heuristics.  Usage:

    python scripts/data/score_shards.py --samples_dicts_dir DIR --ckpt CKPT.pt --out scores.jsonl [--batch_size 32] [--precision bfloat16]

``--ckpt`` takes a training or an inference checkpoint (``hub.load_for_finetuning``); without it a seeded fresh model of ``--model_variant``
is scored (dry runs)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples_dicts_dir", required=True)
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--model_variant", default="tiny")
    ap.add_argument("--out", required=True)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--precision", default="bfloat16", choices=("bfloat16", "float32"))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda")
    opt = ap.parse_args(argv)
    if opt.batch_size < 1:
        ap.error("--batch_size must be positive")
    return opt


def load_net(opt):
    from olmoasr_amd import hub
    from olmoasr_amd.config.model_dims import VARIANT_TO_DIMS
    from olmoasr_amd.model import OLMoASR
    if opt.ckpt:
        dims, sd = hub.finetuning_state_dict(hub.load_checkpoint(opt.ckpt), seed=opt.seed)
        net = OLMoASR(dims, device=opt.device, compute_dtype=opt.precision)
        net.load_state_dict(sd)
        return net
    if opt.model_variant not in VARIANT_TO_DIMS:
        raise SystemExit(f"--model_variant must be one of {sorted(VARIANT_TO_DIMS)}, got {opt.model_variant!r}")
    return OLMoASR(VARIANT_TO_DIMS[opt.model_variant], device=opt.device, seed=opt.seed, compute_dtype=opt.precision)


def main(argv=None, net=None):
    """Returns the number of lines written.  ``net``: a model to score with instead of loading one (tests)."""
    opt = parse_args(argv)
    from olmoasr_amd import data, validation
    samples = data.load_samples_dicts(opt.samples_dicts_dir)
    shards = data.AudioTextShards(samples)
    net = net if net is not None else load_net(opt)
    dev = torch.device(opt.device)
    n = 0
    with open(opt.out, "wt") as f:
        scores = validation.score_set(net, len(shards), lambda pos: validation.shard_batch(shards, pos), dev, opt.batch_size)
        for sc in scores:
            # (one read per batch: the tool is paced by the host's file loads)
            cols = [t.cpu().tolist() for t in (sc.nll_sum, sc.n_tok, sc.n_hit, sc.nll_max)]
            for nll_sum, n_tok, n_hit, nll_max in zip(*cols):
                f.write(json.dumps({"index": n, "audio_file": samples[n].get("audio_file"), "nll_sum": nll_sum, "n_tok": n_tok, "n_hit": n_hit,
                                    "nll_max": nll_max, "mean_nll": nll_sum / n_tok if n_tok else None}) + "\n")
                n += 1
    print(json.dumps({"event": "scored", "samples": n, "out": opt.out}), flush=True)
    return n


if __name__ == "__main__":
    main()
