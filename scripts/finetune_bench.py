"""Step time of frozen-parameter and LoRA fine-tuning on one GPU: OLMoASR-medium, 2 x 128 synthetic clips per step (bench.py's workload:
span step, loss scale, clip, fused AdamW), for the masks of ``--masks`` in ONE process on the same base weights:

  all              every parameter trainable (bench.py's headline step)
  enc              encoder frozen (model.encoder.requires_grad_(False): Whisper's usual fine-tuning recipe)
  enc+tok          encoder and decoder.token_embedding frozen
  lora-qv          base frozen, rank-16 adapters (alpha 32) on attn.query / attn.value of every block (olmoasr_amd.lora)
  enc+lora-qv-dec  the same adapters, those of the encoder frozen too: decoder adapters only, no encoder backward
  dec-cached       encoder frozen and its output of the clips computed once (embed_audio): every step is
                   loss_and_backward(None, ..., audio_features=xa, span=...) + optim_step -- multi-epoch fine-tuning on fixed clips

plus the executed GEMM FLOPs of one step per mask (oasr_profile_gemm_collect).  The LoRA masks run on a second model with adapters (built
from the same seed after the first one is freed).  A mask listed twice is timed again, so box drift during the run shows (the default
list ends with ``all`` for that).  Prints one JSON line; ``--out`` also writes it to a file.

    python scripts/finetune_bench.py --steps 5 --warmup 2 [--masks all,enc,lora-qv,enc+lora-qv-dec,all] [--out profiles/x.json]
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
    ap.add_argument("--masks", default="all,enc,enc+tok,all")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from bench import spread, synth_batch
    from olmoasr_amd.config.model_dims import VARIANT_TO_DIMS
    from olmoasr_amd import _native as N
    from olmoasr_amd import ops
    from olmoasr_amd.model import OLMoASR

    from olmoasr_amd import lora

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dims = VARIANT_TO_DIMS[args.variant]
    models = {"net": None, "lora": None}
    lora_shapes = []  # (rows, cols, rank) of every adapted weight

    def model(with_lora):
        key, other = ("lora", "net") if with_lora else ("net", "lora")
        if models[key] is None:
            models[other] = None  # (two medium models and their workspaces do not need to share the device)
            torch.cuda.empty_cache()
            m = OLMoASR(dims, device=dev, seed=0)
            if with_lora:
                lora.add_lora(m, r=16, alpha=32, target_modules=lora.DEFAULT_TARGETS, seed=0)
                shapes = {n: sh for n, _, _, sh in m._table}
                lora_shapes[:] = [(shapes[n[: -len(".lora_A")] + ".weight"][0], sh[1], sh[0]) for n, _, _, sh in m._table if n.endswith(".lora_A")]
            m.init_optimizer_state()
            models[key] = m
            state["step"] = 0
        return models[key]

    mb, accum = args.micro_batch, args.accum
    pcm, ti, ty, tl = synth_batch(range(mb * accum), dev)
    sp = OLMoASR.supervised_span(ty, tl)
    spans = [sp[i * mb:(i + 1) * mb].contiguous() for i in range(accum)]
    loss_buf = torch.zeros(1, device=dev)
    loss_scale = 65536.0
    state = {"step": 0, "xa": None}
    net = None

    def one_step():
        state["step"] += 1
        net.zero_grad()
        for i in range(accum):
            sl = slice(i * mb, (i + 1) * mb)
            if state["xa"] is not None:  # dec-cached: the frozen encoder's output of these clips, computed once
                net.loss_and_backward(None, ti[sl], ty[sl], tl[sl], loss_scale=loss_scale, accumulation_steps=accum, loss_out=loss_buf,
                                      accumulate_loss=i > 0, span=spans[i], audio_features=state["xa"][i])
                continue
            mel, clip_max = ops.log_mel(pcm[sl], finalize=False)
            net.loss_and_backward(mel, ti[sl], ty[sl], tl[sl], loss_scale=loss_scale, accumulation_steps=accum, loss_out=loss_buf,
                                  accumulate_loss=i > 0, span=spans[i], mel_clip_max=clip_max)
        net.optim_step(step=state["step"], lr=1.5e-4, inv_loss_scale=1.0 / loss_scale, max_grad_norm=1.0)

    def set_mask(kind):
        nonlocal net
        net = model(kind.startswith("lora") or kind.startswith("enc+lora"))
        for name, p in net.named_parameters():
            if ".lora_" in name:  # the LoRA masks: adapters trainable (the encoder's frozen in enc+lora-qv-dec), base frozen
                p.requires_grad_(not (kind == "enc+lora-qv-dec" and name.startswith("encoder.")))
                continue
            frozen = (kind in ("enc", "enc+tok", "dec-cached") and name.startswith("encoder.")) or (kind == "enc+tok" and name == "decoder.token_embedding.weight")
            p.requires_grad_(not frozen and net is models["net"])
        state["xa"] = None
        if kind == "dec-cached":
            state["xa"] = [net.embed_audio(ops.log_mel(pcm[i * mb:(i + 1) * mb])) for i in range(accum)]

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
    kinds = [k.strip() for k in args.masks.split(",") if k.strip()]
    known = ("all", "enc", "enc+tok", "lora-qv", "enc+lora-qv-dec", "dec-cached")
    if any(k not in known for k in kinds):
        raise SystemExit(f"--masks: each of {known}")
    for kind in kinds:
        set_mask(kind)
        ms, spr = timed()
        flops, launches = gemm_flops()
        key = kind if kind not in res else kind + "_again"
        res[key] = {"ms_per_step": round(ms, 2), "spread": spr, "gemm_tflop_per_step": round(flops / 1e12, 2), "gemm_launches": launches,
                    "loss": round(float(loss_buf), 4), "trainable_params": sum(p.numel() for p in net.parameters() if p.requires_grad)}
        print(f"[finetune_bench] {key}: {res[key]}", file=sys.stderr, flush=True)
    out_lora = lora_kernel_times(lora_shapes, N, torch, dev, accum) if lora_shapes else None
    out = {"workload": f"OLMoASR-{args.variant} bf16 span train step, {accum} x {mb} synthetic 30 s clips, one GPU", "steps": args.steps,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(dev), "results": res}
    if "all" in res:
        base = min(res["all"]["ms_per_step"], res.get("all_again", res["all"])["ms_per_step"])
        for kind, key in (("enc", "ratio_enc_frozen"), ("enc+tok", "ratio_enc_tok_frozen"), ("lora-qv", "ratio_lora_qv"),
                          ("enc+lora-qv-dec", "ratio_enc_lora_qv_dec")):
            if kind in res:
                out[key] = round(res[kind]["ms_per_step"] / base, 3)
        if out_lora is not None:
            out["lora_kernels"] = out_lora
            for kind in ("lora-qv", "enc+lora-qv-dec"):
                if kind in res:
                    out_lora[f"share_of_{kind}_step"] = round(out_lora["ms_per_step"] / res[kind]["ms_per_step"], 5)
        if "enc" in res:
            out["gemm_flops_ratio_enc_frozen"] = round(res["enc"]["gemm_tflop_per_step"] / res["all"]["gemm_tflop_per_step"], 3)
    if "enc" in res and "dec-cached" in res:  # the cached-features step against the frozen-encoder step it replaces
        enc_ms = min(res["enc"]["ms_per_step"], res.get("enc_again", res["enc"])["ms_per_step"])
        out["ratio_dec_cached_vs_enc"] = round(res["dec-cached"]["ms_per_step"] / enc_ms, 3)
        out["gemm_flops_ratio_dec_cached_vs_enc"] = round(res["dec-cached"]["gemm_tflop_per_step"] / res["enc"]["gemm_tflop_per_step"], 3)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def lora_kernel_times(shapes, N, torch, dev, accum, reps=20):
    """The adapter kernels of one lora-qv step on their own (cuda events around `reps` repetitions of every target's launch): one
    lora_merge per target (the compute-copy refresh at the end of optim_step) and `accum` lora_grad projections (one per micro-batch)."""
    lib = N.lib()
    sc = 2.0
    bufs = []
    for rows, cols, r in shapes:
        w = torch.randn(rows, cols, device=dev)
        a, b = torch.randn(r, cols, device=dev) * 0.05, torch.randn(rows, r, device=dev) * 0.05
        bufs.append(dict(w=w, a=a, b=b, out=torch.empty(rows, cols, device=dev, dtype=torch.bfloat16), da=torch.zeros_like(a), db=torch.zeros_like(b),
                         scratch=torch.empty(lib.oasr_lora_grad_scratch_bytes(rows, cols, r), device=dev, dtype=torch.uint8)))

    def run(kind):
        for (rows, cols, r), t in zip(shapes, bufs):
            if kind == "merge":
                N.check(lib.oasr_lora_merge_op(N.ptr(t["w"]), N.ptr(t["a"]), N.ptr(t["b"]), rows, cols, r, sc, 0, N.ptr(t["out"]), N.stream_ptr()), "merge")
            else:
                N.check(lib.oasr_lora_grad_op(N.ptr(t["w"]), N.ptr(t["a"]), N.ptr(t["b"]), rows, cols, r, sc, N.ptr(t["da"]), N.ptr(t["db"]),
                                              N.ptr(t["scratch"]), N.stream_ptr()), "grad")

    res = {}
    for kind in ("merge", "grad"):
        run(kind)
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            run(kind)
        e1.record()
        torch.cuda.synchronize(dev)
        res[kind] = e0.elapsed_time(e1) / reps
    rows, cols, r = shapes[0]
    return {"targets": len(shapes), "shape_0": [rows, cols, r], "merge_ms_all_targets": round(res["merge"], 4), "grad_ms_all_targets": round(res["grad"], 4),
            "merge_bytes_per_target": rows * cols * 6 + (rows + cols) * r * 4,
            "grad_bytes_per_target": rows * cols * 4 + (rows + cols) * r * 8 + 2 * 4 * ((rows + 127) // 128 * r * cols + (cols + 255) // 256 * rows * r),
            "ms_per_step": round(res["merge"] + accum * res["grad"], 4)}


if __name__ == "__main__":
    main()
