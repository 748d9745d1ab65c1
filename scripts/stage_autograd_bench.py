"""The staged autograd path (model.encoder / model.decoder with a grad_fn) against the fused autograd step, and a
d(mel) workload for the conv1 fold kernel.

  --ab    (default) one reference-style step per round on OLMoASR-``--variant`` with ``--batch`` synthetic clips, alternated:
            fused:  logits = model(mel, tokens, mask)                                        (_TrainStep)
            staged: logits = model.decoder(tokens, model.encoder(mel), padding_mask=mask)    (_EncoderStage + _DecoderStage)
          each followed by the same F.cross_entropy(ignore_index=51864) and .backward(); prints the per-step medians and their ratio.
  --dmel  every parameter frozen, ``mel.requires_grad``: ``--reps`` encoder-stage forward + backward with d(mel) (saliency), for a
          ``rocprofv3 --kernel-trace --stats`` run that times conv1_col2im_mel_kernel.

Prints one JSON line; ``--out`` also writes it to a file.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="medium")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dmel", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import torch.nn.functional as F
    from bench import synth_batch
    from olmoasr_amd import ops
    from olmoasr_amd.config.model_dims import VARIANT_TO_DIMS
    from olmoasr_amd.model import OLMoASR

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    net = OLMoASR(VARIANT_TO_DIMS[args.variant], device=dev, seed=0)
    B = args.batch
    pcm, ti, ty, tl = synth_batch(range(B), dev)
    mel = ops.log_mel(pcm)
    out = {"variant": args.variant, "batch": B, "device": torch.cuda.get_device_name(dev)}

    if args.dmel:
        net.requires_grad_(False)
        for _ in range(args.reps):
            m = mel.clone().requires_grad_(True)
            net.encoder(m).float().sum().backward()
        torch.cuda.synchronize(dev)
        out.update(workload="encoder stage forward + backward with d(mel), every parameter frozen", reps=args.reps,
                   dmel_abs_mean=float(m.grad.abs().mean()))
    else:
        mask = torch.zeros(B, 448, 448, device=dev)
        for b, n in enumerate(tl.tolist()):
            mask[b, :, n:] = -float("inf")

        def step(staged):
            logits = net.decoder(ti, net.encoder(mel), padding_mask=mask) if staged else net(mel, ti, mask)
            F.cross_entropy(logits.view(-1, logits.shape[-1]), ty.view(-1), ignore_index=51864).backward()

        for _ in range(args.warmup):
            step(False)
            step(True)
        times = {False: [], True: []}
        for r in range(args.rounds):
            for staged in ((False, True) if r % 2 == 0 else (True, False)):  # alternated, order flipped every round
                net.zero_grad()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                e0.record()
                step(staged)
                e1.record()
                torch.cuda.synchronize(dev)
                times[staged].append(e0.elapsed_time(e1))
        fused, staged = statistics.median(times[False]), statistics.median(times[True])
        out.update(workload="reference-style autograd step (forward, F.cross_entropy, backward), alternated A/B", rounds=args.rounds,
                   fused_ms=round(fused, 2), staged_ms=round(staged, 2), ratio_staged_vs_fused=round(staged / fused, 4),
                   fused_ms_all=[round(t, 2) for t in times[False]], staged_ms_all=[round(t, 2) for t in times[True]])
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
