"""Step time of frozen-parameter fine-tuning on one GPU: OLMoASR-medium, 2 x 128 synthetic clips per step (bench.py's workload: span
step, loss scale, clip, fused AdamW), for three masks in ONE process on the same weights:

  all          every parameter trainable (bench.py's headline step)
  enc          encoder frozen (model.encoder.requires_grad_(False): Whisper's usual fine-tuning recipe)
  enc+tok      encoder and decoder.token_embedding frozen

plus the executed GEMM FLOPs of one step per mask (oasr_profile_gemm_collect).  The all-trainable step is timed again at the end, so box
drift during the run shows.  Prints one JSON line; ``--out`` also writes it to a file.

    python scripts/finetune_bench.py --steps 5 --warmup 2 [--out profiles/finetune_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="medium")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--micro-batch", type=int, default=128)
    ap.add_argument("--accum", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from bench import spread, synth_batch
    from olmoasr_amd.config.model_dims import VARIANT_TO_DIMS
    from olmoasr_amd import _native as N
    from olmoasr_amd import ops
    from olmoasr_amd.model import OLMoASR

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dims = VARIANT_TO_DIMS[args.variant]
    net = OLMoASR(dims, device=dev, seed=0)
    net.init_optimizer_state()
    mb, accum = args.micro_batch, args.accum
    pcm, ti, ty, tl = synth_batch(range(mb * accum), dev)
    sp = OLMoASR.supervised_span(ty, tl)
    spans = [sp[i * mb:(i + 1) * mb].contiguous() for i in range(accum)]
    loss_buf = torch.zeros(1, device=dev)
    loss_scale = 65536.0
    state = {"step": 0}

    def one_step():
        state["step"] += 1
        net.zero_grad()
        for i in range(accum):
            sl = slice(i * mb, (i + 1) * mb)
            mel, clip_max = ops.log_mel(pcm[sl], finalize=False)
            net.loss_and_backward(mel, ti[sl], ty[sl], tl[sl], loss_scale=loss_scale, accumulation_steps=accum, loss_out=loss_buf,
                                  accumulate_loss=i > 0, span=spans[i], mel_clip_max=clip_max)
        net.optim_step(step=state["step"], lr=1.5e-4, inv_loss_scale=1.0 / loss_scale, max_grad_norm=1.0)

    def set_mask(kind):
        for name, p in net.named_parameters():
            frozen = (kind in ("enc", "enc+tok") and name.startswith("encoder.")) or (kind == "enc+tok" and name == "decoder.token_embedding.weight")
            p.requires_grad_(not frozen)

    def timed():
        for _ in range(args.warmup):
            one_step()
        torch.cuda.synchronize(dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
        ev[0].record()
        for k in range(args.steps):
            one_step()
            ev[k + 1].record()
        torch.cuda.synchronize(dev)
        ms = [ev[k].elapsed_time(ev[k + 1]) for k in range(args.steps)]
        return sum(ms) / len(ms), spread(ms)

    def gemm_flops():
        lib = N.lib()
        torch.cuda.synchronize(dev)
        lib.oasr_profile_gemm(1)
        one_step()
        torch.cuda.synchronize(dev)
        ms, fl, cnt = (ctypes.c_double * 4)(), (ctypes.c_double * 4)(), (ctypes.c_int64 * 4)()
        N.check(lib.oasr_profile_gemm_collect(ms, fl, cnt, None, 0), "profile_collect")
        lib.oasr_profile_gemm(0)
        return sum(fl), int(sum(cnt))

    res = {}
    for kind in ("all", "enc", "enc+tok", "all"):
        set_mask(kind)
        ms, spr = timed()
        flops, launches = gemm_flops()
        key = kind if kind not in res else kind + "_again"
        res[key] = {"ms_per_step": round(ms, 2), "spread": spr, "gemm_tflop_per_step": round(flops / 1e12, 2), "gemm_launches": launches,
                    "loss": round(float(loss_buf), 4), "trainable_params": sum(p.numel() for p in net.parameters() if p.requires_grad)}
        print(f"[finetune_bench] {key}: {res[key]}", file=sys.stderr, flush=True)
    base = min(res["all"]["ms_per_step"], res["all_again"]["ms_per_step"])
    out = {"workload": f"OLMoASR-{args.variant} bf16 span train step, {accum} x {mb} synthetic 30 s clips, one GPU", "steps": args.steps,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(dev), "results": res,
           "ratio_enc_frozen": round(res["enc"]["ms_per_step"] / base, 3),
           "ratio_enc_tok_frozen": round(res["enc+tok"]["ms_per_step"] / base, 3),
           "gemm_flops_ratio_enc_frozen": round(res["enc"]["gemm_tflop_per_step"] / res["all"]["gemm_tflop_per_step"], 3)}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
