#!/usr/bin/env python
"""torchrun entry point of the MI355X-native training path -- flag-compatible with the part of the reference's
``scripts/training/train_timestamps.py::main`` (train_timestamps.py:2098-2134) that drives the hot loop.

    torchrun --nnodes 1:1 --nproc_per_node 8 --master-addr 127.0.0.1 scripts/training/train_timestamps.py \
        --model_variant medium --precision bfloat16 --eff_batch_size 2048 --train_batch_size 32 --train_steps 100 \
        --lr 1.5e-3 --betas '(0.9, 0.98)' --eps 1e-6 --weight_decay 0.1 --max_grad_norm 1.0 --synthetic True

What is kept from the reference loop (citations into /root/reference/scripts/training/train_timestamps.py):
  env rank discovery :2227-2230 * setup("nccl") :564-574 * accumulation rule + warmup/linear-decay LambdaLR :764-781 *
  GradScaler semantics (enabled for bf16 too, :2349: scale 65536, x2 every 2000 clean steps, x0.5 + skipped step on
  inf/nan) * per-step clip(1.0)+AdamW :1509-1512 * throughput metric audio_min_per_GPU_second :1525-1527 * loss
  all-reduce every train_log_freq :1553 * checkpoint dict keys and file names :930-972.
What is replaced: tokenizer/W&B/eval plumbing (out of scope); model/loss/backward/optimizer/DDP -> the HIP
engine (olmoasr_amd).  Data: ``--samples_dicts_dir DIR --synthetic False`` reads the reference's shard files (:577-604, :2255-2266)
through the on-device input path (olmoasr_amd/data.py: DistributedSampler order, int16 clips via pinned ring slots and a copy
stream, log-mel on the GPU, ``text_len`` instead of the [448, 448] mask -- SURVEY.md section 8f-1; tokens come pre-tokenised or from
a ``text_fn`` plug because the whisper tokenizer is not vendored); the default is a seeded synthetic dataset with the reference's
token layout, sharded like DistributedSampler (:633-638).
"""
import ast
import glob
import json
import math
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HARDWARE_TO_FLOPS = {"H100": 900 * 10 ** 12, "L40": 366 * 10 ** 12, "A100": 312 * 10 ** 12, "MI355X": 2500 * 10 ** 12}


# The reference's entry is ``Fire(main)`` (train_timestamps.py:2098-2134): flags are ``--name=value`` / ``--name value`` with
# Python-literal values (``--betas='(0.9, 0.98)'``, ``--pin_memory=True``, ``--ckpt_file_name=None``).  Same flag names and
# defaults here; the flags of subsystems that are out of scope (data curation, eval sets, W&B) are
# ACCEPTED -- the reference launcher (configs/job_configs/training/filtered/*_sn.sh:65-100) passes all of them -- and
# reported as ignored.
REFERENCE_FLAGS = dict(
    model_variant="tiny", exp_name="olmoasr_amd_run", job_type="train", samples_dicts_dir=None, train_steps=10, epoch_steps=0,
    ckpt_file_name=None, ckpt_dir="checkpoints", log_dir="logs", eval_dir="data/eval", run_id_dir="run_ids", lr=1.5e-3,
    betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1, max_grad_norm=1.0, eff_batch_size=256, train_batch_size=8, eval_batch_size=32,
    num_workers=10, prefetch_factor=2, pin_memory=True, shuffle=True, persistent_workers=True, run_eval=False, train_log_freq=20000,
    eval_freq=20000, ckpt_freq=2500, verbose=False, precision="bfloat16", hardware="MI355X", async_eval=False, eval_script_path=None,
    eval_wandb_log=False, eval_on_gpu=True)
IGNORED_FLAGS = ("eval_dir", "eval_batch_size", "pin_memory", "persistent_workers", "verbose",
                 "async_eval", "eval_script_path", "eval_wandb_log", "eval_on_gpu", "job_type", "log_dir")
NATIVE_FLAGS = dict(  # additions of this implementation
    synthetic=True, n_synthetic=4096, timestamps=False, seed=0, bucket_cap_mb=128.0, reducer="allreduce", resume=False,
    force_dist=False,  # run the RCCL group / bucketed exchange / sharded step even at world_size 1 (single-GPU rehearsal of the N > 1 path)
    zero_stage=0,  # zero_stage 1: AdamW moments sharded over the ranks (olmoasr_amd/zero.py; the reference's FSDP script's role)
    span_backward=True,  # decoder backward over the supervised span only (oasr_train_step's span_host; same loss / gradients, forward over all 448)
    span_forward=True,  # the decoder's forward leaves the padded positions out too (their logits are read by nothing; -4.7 % more); False = forward over all 448
    freeze_encoder=False,  # fine-tuning: encoder.* get requires_grad=False (no gradient, no update; the backward skips the encoder)
    # LoRA fine-tuning (olmoasr_amd/lora.py): rank-r adapters with scale alpha / r on the modules --lora_targets selects (comma-separated
    # fnmatch patterns), every base parameter frozen; 0 = off.  With --freeze_encoder the encoder's adapters stay frozen as well.
    lora_rank=0, lora_alpha=32, lora_targets="*.attn.query,*.attn.value",
    # SpecAugment on the finalized log-mel of every TRAINING micro-batch (olmoasr_amd/augment.py, csrc/specaug.hip): off | LD (2 + 2 masks) |
    # LB (1 + 1); the --spec_* overrides replace single fields of the preset.  Masks are seeded by --seed and the step counter (spec_offset).
    spec_augment="off", spec_freq_masks=None, spec_freq_width=None, spec_time_masks=None, spec_time_width=None, spec_time_ratio=None,
    spec_fill=None,
    # Token error counts of a logging step (train_token_error_rate).  "host": the plain step returns fp32 logits, gen_pred + token_error_rate
    # score them in Python.  "device": the logging step stays on the span step (needs --span_backward; the un-finalized log-mel shortcut stays
    # in use), which hands back the argmax ids (loss_and_backward(pred_out=...)); olmoasr_amd.metrics scores them with the edit-distance
    # kernel (ops.edit_counts), the counts are read where the loss is read and all-reduced with it, and the record gains train_subs /
    # train_dels / train_ins; evaluate() scores with the same kernel.  ONE difference: a prediction without <|endoftext|> inside the computed
    # prefix ends at span[b] rounded up to 64 instead of at position 448 -- the host path also scores the argmax of padded positions, which
    # the loss ignores (and which the span step's forward does not compute).
    train_error_counts="host",
    # Regularisers of the fused step's objective (loss_and_backward(label_smoothing=, z_loss=); csrc/loss.hip): label smoothing eps in [0, 1)
    # -- F.cross_entropy(label_smoothing=eps), the usual companion of SpecAugment -- and the z-loss coefficient z >= 0 -- + z * mean(logsumexp^2),
    # PaLM's auxiliary term.  Both 0 = the reference's objective, step and log records unchanged.  With either set, train_loss is the regularised
    # objective and a logging step's record gains train_nll (the plain cross-entropy) and train_lse_sq (mean logsumexp^2), read with the loss.
    label_smoothing=0.0, z_loss=0.0,
    # Speed perturbation of the int16 clips of every TRAINING micro-batch, ahead of the log-mel (olmoasr_amd/augment.py, csrc/speed.hip): off |
    # 3way (each clip 0.9, 1.0 or 1.1 times its speed; the transcript's timestamp tokens move along).  --speed_factors replaces the preset's list
    # of (P, Q) pairs, P / Q times faster.  Drawn from --seed and the step counter (spec_offset), like the SpecAugment masks.
    speed_perturb="off", speed_factors=None,
    # Noise mixing on the int16 clips of every TRAINING micro-batch, after speed perturbation and ahead of the log-mel (olmoasr_amd/augment.py,
    # csrc/noise.hip): --noise_bank PATH.npy (int16 [M, L], or an object array of 1-D int16 recordings, tiled to the longest) turns it on;
    # --noise_prob (default 0.5) is a clip's chance to take noise, --noise_snr_db LO,HI (default 5,20) the whole dB the SNR is drawn among.
    # Drawn from --seed and the step counter (spec_offset), like the masks and the speed factors.
    noise_bank=None, noise_prob=None, noise_snr_db=None,
    # Reverberation of the int16 clips of every TRAINING micro-batch, after speed perturbation and ahead of noise mixing (the far-field recipe;
    # olmoasr_amd/augment.py, csrc/reverb.hip): --rir_bank PATH.npy (room impulse responses at 16 kHz: a 2-D float array, one response per
    # row, or an object array of 1-D float responses) turns it on; --reverb_prob (default 0.5) is a clip's chance to be reverberated.  Drawn
    # from --seed and the step counter (spec_offset), like the masks, the speed factors and the noise.
    rir_bank=None, reverb_prob=None,
    # The telephone channel on the int16 clips of every TRAINING micro-batch, after noise mixing -- the channel carries the noise too -- and ahead
    # of the log-mel (olmoasr_amd/augment.py, csrc/telephone.hip): --telephone_prob P (a clip's chance to go through the channel) turns it on;
    # --telephone_codecs (default mulaw,alaw,linear) lists the G.711 codecs one is drawn from, repeats acting as weights, and
    # --telephone_bandpass (default True) keeps or drops the 300 - 3400 Hz band-pass ahead of the codec.  Drawn from --seed and the step
    # counter (spec_offset), like the masks, the speed factors, the room responses and the noise.
    telephone_prob=None, telephone_codecs=None, telephone_bandpass=None,
    # Held-out loss (OLMoASR.score, csrc/score.hip: forward only, no fp32 logits, no gradient write).  --val_freq N (0 = off: step and log
    # records unchanged) scores a validation set every N optimizer steps, after the step: with --synthetic the --n_val indices
    # n_synthetic + 8 + i (disjoint from every training shard and from evaluate()'s clips), else the shards under --val_samples_dicts_dir
    # (its first --n_val samples).  Validation clips are never augmented; each rank scores ddp.shard_indices of the set in batches of
    # --val_batch_size (default: train_batch_size) trimmed to the batch's largest span rounded up to 64, the totals are all-reduced as one
    # tensor and rank 0 prints {"event": "val", val_loss (token-weighted), val_token_acc, val_n_tokens, val_subs / val_dels / val_ins}.
    val_freq=0, val_samples_dicts_dir=None, n_val=256, val_batch_size=None)
ERROR_COUNTS = ("host", "device")
SPEC_OVERRIDES = ("spec_freq_masks", "spec_freq_width", "spec_time_masks", "spec_time_width", "spec_time_ratio", "spec_fill")
SPEC_PRESETS = ("off", "LD", "LB")
SPEED_PRESETS = ("off", "3way")


class Args(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def _literal(v):
    if not isinstance(v, str):
        return v
    try:
        return ast.literal_eval(v)
    except (ValueError, SyntaxError):
        return v


def spec_policy(args):
    """--spec_augment and its overrides -> augment.SpecAugment, or None for "off"."""
    given = [f for f in SPEC_OVERRIDES if args[f] is not None]
    if args.spec_augment not in SPEC_PRESETS:
        raise SystemExit(f"--spec_augment must be one of {' | '.join(SPEC_PRESETS)}, got {args.spec_augment!r}")
    if args.spec_augment == "off":
        if given:
            raise SystemExit(f"--{' --'.join(given)} given with --spec_augment=off: name a policy ({' | '.join(SPEC_PRESETS[1:])}) to override")
        return None
    from olmoasr_amd import augment
    over = {f[len("spec_"):]: args[f] for f in given}
    for k in ("time_ratio", "fill"):
        if k in over:
            try:
                over[k] = float(over[k])  # ("nan" / "inf" are not Python literals)
            except (TypeError, ValueError):
                raise SystemExit(f"--spec_{k} must be a number, got {over[k]!r}")
    try:
        return augment.SpecAugment.preset(args.spec_augment, **over)
    except ValueError as e:
        raise SystemExit(f"--spec_augment={args.spec_augment}: {e}")


def speed_policy(args):
    """--speed_perturb and --speed_factors -> augment.SpeedPerturb, or None for "off"."""
    if args.speed_perturb not in SPEED_PRESETS:
        raise SystemExit(f"--speed_perturb must be one of {' | '.join(SPEED_PRESETS)}, got {args.speed_perturb!r}")
    if args.speed_perturb == "off":
        if args.speed_factors is not None:
            raise SystemExit(f"--speed_factors given with --speed_perturb=off: name a policy ({' | '.join(SPEED_PRESETS[1:])}) to override")
        return None
    from olmoasr_amd import augment
    over = {}
    if args.speed_factors is not None:
        f = args.speed_factors
        if not (isinstance(f, (tuple, list)) and f and all(isinstance(pq, (tuple, list)) and len(pq) == 2 for pq in f)):
            raise SystemExit(f"--speed_factors must be a list of (P, Q) pairs such as '((9,10),(1,1),(11,10))', got {f!r}")
        over["factors"] = tuple(tuple(pq) for pq in f)
    try:
        return augment.SpeedPerturb.preset(args.speed_perturb, **over)
    except ValueError as e:
        raise SystemExit(f"--speed_perturb={args.speed_perturb}: {e}")


def noise_policy(args):
    """--noise_bank, --noise_prob and --noise_snr_db -> augment.NoiseMix, or None without a bank (the bank itself is loaded by load_noise_bank)."""
    if args.noise_bank is None:
        for f in ("noise_prob", "noise_snr_db"):
            if args[f] is not None:
                raise SystemExit(f"--{f} given without --noise_bank: name a bank of noise recordings (PATH.npy) to mix from")
        return None
    if not isinstance(args.noise_bank, str) or not os.path.isfile(args.noise_bank):
        raise SystemExit(f"--noise_bank must name an existing .npy file, got {args.noise_bank!r}")
    over = {}
    if args.noise_prob is not None:
        over["prob"] = args.noise_prob
    if args.noise_snr_db is not None:
        snr = args.noise_snr_db
        if not (isinstance(snr, (tuple, list)) and len(snr) == 2):
            raise SystemExit(f"--noise_snr_db must be LO,HI in whole dB such as '5,20', got {snr!r}")
        over["snr_db"] = tuple(snr)
    from olmoasr_amd import augment
    try:
        return augment.NoiseMix(**over)
    except ValueError as e:
        raise SystemExit(f"--noise_prob / --noise_snr_db: {e}")


def reverb_policy(args):
    """--rir_bank and --reverb_prob -> augment.Reverb, or None without a bank (the bank itself is loaded by load_rir_bank)."""
    if args.rir_bank is None:
        if args.reverb_prob is not None:
            raise SystemExit("--reverb_prob given without --rir_bank: name a bank of room impulse responses (PATH.npy) to convolve with")
        return None
    if not isinstance(args.rir_bank, str) or not os.path.isfile(args.rir_bank):
        raise SystemExit(f"--rir_bank must name an existing .npy file, got {args.rir_bank!r}")
    from olmoasr_amd import augment
    try:
        return augment.Reverb(**({} if args.reverb_prob is None else {"prob": args.reverb_prob}))
    except ValueError as e:
        raise SystemExit(f"--reverb_prob: {e}")


def telephone_policy(args):
    """--telephone_prob, --telephone_codecs and --telephone_bandpass -> augment.TelephoneChannel, or None without --telephone_prob."""
    if args.telephone_prob is None:
        for f in ("telephone_codecs", "telephone_bandpass"):
            if args[f] is not None:
                raise SystemExit(f"--{f} given without --telephone_prob: give the chance of a clip to go through the channel to turn it on")
        return None
    over = {"prob": args.telephone_prob}
    if args.telephone_codecs is not None:
        c = args.telephone_codecs
        over["codecs"] = tuple(t.strip() for t in c.split(",")) if isinstance(c, str) else tuple(c) if isinstance(c, (tuple, list)) else c
    if args.telephone_bandpass is not None:
        over["bandpass"] = args.telephone_bandpass
    from olmoasr_amd import augment
    try:
        return augment.TelephoneChannel(**over)
    except ValueError as e:
        raise SystemExit(f"--telephone_prob / --telephone_codecs / --telephone_bandpass: {e}")


def load_rir_bank(path):
    """The bank of --rir_bank as (int16 [R, K] Q15 taps, int32 [R] direct-path delays) on the CPU, from a 2-D float array (one response per
    row) or an object array (or list) of 1-D float responses: augment.rir_bank scales each to unit energy, K = min(8192, the longest)."""
    import numpy as np
    from olmoasr_amd import augment
    try:
        arr = np.load(path, allow_pickle=True)
    except (OSError, ValueError) as e:
        raise SystemExit(f"--rir_bank {path}: {e}")
    try:
        if arr.dtype.kind == "f" and arr.ndim == 2 and arr.shape[0]:
            return augment.rir_bank(list(arr))
        if arr.dtype == object and arr.ndim == 1 and len(arr) and all(isinstance(r, np.ndarray) for r in arr):
            return augment.rir_bank(list(arr))
    except ValueError as e:
        raise SystemExit(f"--rir_bank {path}: {e}")
    raise SystemExit(f"--rir_bank {path}: expected a float [R, K] array or an object array of 1-D float responses, got {arr.dtype} {arr.shape}")


def load_noise_bank(path):
    """The bank of --noise_bank as int16 [M, L] on the CPU: a 2-D int16 array as it is, an object array (or list) of 1-D int16 recordings
    tiled cyclically to the longest of them."""
    import numpy as np
    from olmoasr_amd import augment
    try:
        arr = np.load(path, allow_pickle=True)
    except (OSError, ValueError) as e:
        raise SystemExit(f"--noise_bank {path}: {e}")
    try:
        if arr.dtype == np.int16 and arr.ndim == 2:
            return augment.noise_bank(list(arr), int(arr.shape[1]))
        if arr.dtype == object and arr.ndim == 1 and len(arr) and all(isinstance(r, np.ndarray) for r in arr):
            return augment.noise_bank(list(arr), min(1 << 26, max(int(r.size) for r in arr)))
    except ValueError as e:
        raise SystemExit(f"--noise_bank {path}: {e}")
    raise SystemExit(f"--noise_bank {path}: expected int16 [M, L] or an object array of 1-D int16 recordings, got {arr.dtype} {arr.shape}")


def spec_offset(global_step, micro, accum, world_size, rank, train_batch_size):
    """Stream id of row 0 of micro-batch ``micro`` of the step that follows ``global_step`` completed ones, on ``rank``; row b is + b.  A
    function of the step counter, not of process lifetime: a resumed run draws the masks the uninterrupted run would have drawn, and the
    id ranges of different (step, micro, rank) never overlap."""
    return ((global_step * accum + micro) * world_size + rank) * train_batch_size


def parse_args(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = Args({**REFERENCE_FLAGS, **NATIVE_FLAGS})
    given = set()
    i = 0
    while i < len(argv):
        tok = argv[i]
        if not tok.startswith("--"):
            raise SystemExit(f"unexpected positional argument {tok!r} (flags are --name=value, as with the reference's Fire entry)")
        if "=" in tok:
            name, val = tok[2:].split("=", 1)
        elif i + 1 < len(argv) and not argv[i + 1].startswith("--"):
            name, val = tok[2:], argv[i + 1]
            i += 1
        else:
            name, val = tok[2:], "True"  # bare flag
        name = name.replace("-", "_")
        if name not in args:
            raise SystemExit(f"unknown flag --{name}; known: {sorted(args)}")
        args[name] = _literal(val)
        given.add(name)
        i += 1
    ignored = sorted(f for f in given if f in IGNORED_FLAGS)
    if ignored and int(os.environ.get("RANK", "0")) == 0:
        print(json.dumps({"event": "ignored_flags", "flags": ignored,
                          "why": "data curation / eval sets / W&B are outside the hot path (SURVEY.md section 2)"}), flush=True)
    if args.ckpt_file_name in (None, "None"):
        args.ckpt_file_name = ""            # train_timestamps.py:2198-2199
    if isinstance(args.betas, str):
        args.betas = ast.literal_eval(args.betas)
    if args.precision == "float16":
        raise SystemExit("--precision float16: the MI355X-native engine computes in bfloat16 (production, = the reference's "
                         "autocast(bfloat16) path) or float32 (validation kernels); the fp16 autocast path of the reference "
                         "(train_timestamps.py:2128 default) has no native counterpart -- pass --precision bfloat16")
    if args.precision not in ("bfloat16", "float32"):
        raise SystemExit(f"--precision must be bfloat16 | float32 | float16, got {args.precision!r}")
    if not isinstance(args.lora_rank, int) or args.lora_rank < 0:
        raise SystemExit(f"--lora_rank must be a non-negative integer (0 = no adapters), got {args.lora_rank!r}")
    for flag, ok, want in (("label_smoothing", lambda v: 0.0 <= v < 1.0, "a number in [0, 1) (0 = off)"),
                           ("z_loss", lambda v: v >= 0.0, "a non-negative number (0 = off)")):
        v = args[flag]
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not ok(v):
            raise SystemExit(f"--{flag} must be {want}, got {v!r}")
        args[flag] = float(v)
    if isinstance(args.lora_targets, str):
        args.lora_targets = tuple(t.strip() for t in args.lora_targets.split(",") if t.strip())
    args.lora_targets = tuple(args.lora_targets)
    args.spec_policy = spec_policy(args)
    args.speed_policy = speed_policy(args)
    args.noise_policy = noise_policy(args)
    args.reverb_policy = reverb_policy(args)
    args.telephone_policy = telephone_policy(args)
    if args.train_error_counts not in ERROR_COUNTS:
        raise SystemExit(f"--train_error_counts must be one of {' | '.join(ERROR_COUNTS)}, got {args.train_error_counts!r}")
    if args.train_error_counts == "device" and not args.span_backward:
        raise SystemExit("--train_error_counts=device takes the predictions from the span step: it needs --span_backward=True")
    if args.val_batch_size is None:
        args.val_batch_size = args.train_batch_size
    for flag, low in (("val_freq", 0), ("n_val", 1), ("val_batch_size", 1)):
        v = args[flag]
        if isinstance(v, bool) or not isinstance(v, int) or v < low:
            raise SystemExit(f"--{flag} must be an integer >= {low}, got {v!r}")
    if args.val_samples_dicts_dir and not args.val_freq:
        raise SystemExit("--val_samples_dicts_dir names a validation set but --val_freq is 0: pass --val_freq N to score it every N steps")
    if args.val_freq and not args.synthetic and not args.val_samples_dicts_dir:
        raise SystemExit("--val_freq with --synthetic False needs --val_samples_dicts_dir (the held-out shards)")
    return args


def val_indices(args):
    """The synthetic validation set: --n_val indices past the training range [0, n_synthetic) and past evaluate()'s eight held-out clips."""
    return [int(args.n_synthetic) + 8 + i for i in range(int(args.n_val))]


class GradScalerState:
    """torch.cuda.amp.GradScaler defaults (init 65536, growth 2, backoff 0.5, interval 2000), host-side bookkeeping;
    the inf check and the unscale run inside the fused optimizer kernel."""

    def __init__(self):
        self.scale, self.growth_tracker = 65536.0, 0

    def update(self, found_inf: bool):
        if found_inf:
            self.scale *= 0.5
            self.growth_tracker = 0
        else:
            self.growth_tracker += 1
            if self.growth_tracker == 2000:
                self.scale *= 2.0
                self.growth_tracker = 0

    def state_dict(self):
        return {"scale": self.scale, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000,
                "_growth_tracker": self.growth_tracker}

    def load_state_dict(self, sd):
        self.scale, self.growth_tracker = float(sd["scale"]), int(sd["_growth_tracker"])


def accumulation_steps(eff_batch_size, world_size, train_batch_size):
    """prepare_sched, train_timestamps.py:764-770."""
    if eff_batch_size <= world_size * train_batch_size:
        return 1
    return eff_batch_size // (world_size * train_batch_size)


def lr_lambda(global_step, train_steps):
    """prepare_sched, train_timestamps.py:771-781."""
    warmup = math.ceil(0.002 * train_steps)
    if global_step < warmup:
        return float(global_step) / float(max(1, warmup))
    return max(0.0, float(train_steps - global_step) / float(max(1, train_steps - warmup)))


TAGS = ["ddp-train", "grad-acc", "fp16"]  # train_timestamps.py:2201-2206 (part of the checkpoint file names)


def scheduler_state(lr, train_steps, global_step):
    """``LambdaLR.state_dict()`` of the reference's scheduler after ``global_step`` steps (what its load_ckpt feeds to
    ``scheduler.load_state_dict``, :1056): produced by a real LambdaLR on a dummy parameter, so every key this torch
    version expects is present (function lambdas are saved as None, as torch does)."""
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.AdamW([p], lr=lr)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda step: lr_lambda(step, train_steps))
    sd = sched.state_dict()
    sd["last_epoch"] = global_step
    sd["_step_count"] = global_step + 1
    sd["_last_lr"] = [lr * lr_lambda(global_step, train_steps)]
    return sd


def build_checkpoint(model_sd, optimizer_sd, scaler_sd, *, global_step, local_step, epoch, dims, lr, train_steps, cursor=0,
                     optimizer_steps=None, best_eval_wer=None):
    """The reference's checkpoint dict (train_timestamps.py:930-958), un-prefixed model keys.  ``dims`` is stored as a
    ``types.SimpleNamespace`` of the ModelDimensions fields: the reference's load_ckpt does ``OLMoASR(dims=ckpt['dims'])``
    (attribute access, :1036) and gen_inf_ckpt reads ``dims.__dict__`` -- both work on it, and it unpickles without this
    package (or the reference's) being importable."""
    import types
    fields = dims if isinstance(dims, dict) else dims.__dict__
    return {"global_step": global_step, "local_step": local_step, "epoch": epoch, "best_eval_wer": best_eval_wer,
            "model_state_dict": model_sd, "optimizer_state_dict": optimizer_sd, "scaler_state_dict": scaler_sd,
            "scheduler_state_dict": scheduler_state(lr, train_steps, global_step), "dims": types.SimpleNamespace(**fields),
            "data_cursor": cursor, "optimizer_steps": global_step if optimizer_steps is None else optimizer_steps}


def run_dir(args, run_id):
    return os.path.join(args.ckpt_dir, f"{args.exp_name}_{run_id}")  # {ckpt_dir}/{exp_name}_{run_id} (:956)


def save_ckpt(net, scaler, global_step, local_step, epoch, args, dims, rank, run_id, cursor=0, optimizer_steps=None,
              file_name="latesttrain", sharded=None):
    """save_ckpt (train_timestamps.py:894-972): the ``_ddp`` file carries ``module.`` keys, the ``_non_ddp`` file plain ones."""
    moments = sharded.gather_state() if sharded is not None else None  # (collective: every rank takes part)
    if rank != 0:
        return None
    os.makedirs(run_dir(args, run_id), exist_ok=True)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    steps = global_step if optimizer_steps is None else optimizer_steps
    base = build_checkpoint(sd, net.optimizer_state_dict(step=steps, lr=args.lr * lr_lambda(global_step, args.train_steps), betas=args.betas,
                                                         eps=args.eps, weight_decay=args.weight_decay, moments=moments),
                            scaler.state_dict(), global_step=global_step, local_step=local_step, epoch=epoch, dims=dims, lr=args.lr,
                            train_steps=args.train_steps, cursor=cursor, optimizer_steps=steps)
    tag = f"{file_name}_{global_step:08}_{args.model_variant}_{'_'.join(TAGS)}"
    paths = []
    for suffix, prefix in (("ddp", "module."), ("non_ddp", "")):
        ck = dict(base)
        ck["model_state_dict"] = {prefix + k: v for k, v in sd.items()}
        p = os.path.join(run_dir(args, run_id), f"{tag}_{suffix}.pt")
        torch.save(ck, p)
        paths.append(p)
    return paths


def find_ckpt(args, run_id):
    """File selection of the reference's load_ckpt (train_timestamps.py:1012-1030): an explicit path, a file-name prefix in
    the run directory, or the latest ``*_fp16_ddp.pt`` of this run."""
    name = args.ckpt_file_name
    if name and "/" in name:
        return name
    pat = os.path.join(run_dir(args, run_id), f"{name or '*'}_*_{args.model_variant}_*_fp16_ddp.pt")
    files = [f for f in glob.glob(pat) if not f.endswith("_non_ddp.pt")]
    if not files:
        raise FileNotFoundError(f"no checkpoint matches {pat}")
    return max(files, key=lambda f: int(os.path.basename(f).split("_")[1]))


def load_ckpt(net, scaler, path, sharded=None):
    """Resume (train_timestamps.py:975-1074): model (``module.`` keys), AdamW moments, GradScaler, counters.  Accepts files
    written by the reference (``dims`` pickled as ``olmoasr.config.model_dims.ModelDimensions``: see hub.load_checkpoint)."""
    from olmoasr_amd import hub
    ck = hub.load_checkpoint(path)
    net.load_state_dict({k[len("module."):] if k.startswith("module.") else k: v for k, v in ck["model_state_dict"].items()})
    net.refresh_shadow()
    if sharded is not None:  # fill full-length scratch moments, keep this rank's range
        full = (torch.zeros_like(net.flat_params), torch.zeros_like(net.flat_params))
        opt_steps = net.load_optimizer_state_dict(ck["optimizer_state_dict"], into=full)
        sharded.load_state(*full)
        del full
    else:
        opt_steps = net.load_optimizer_state_dict(ck["optimizer_state_dict"])
    scaler.load_state_dict(ck["scaler_state_dict"])
    # torch's AdamW does not advance its step on a GradScaler-skipped iteration: opt_steps <= global_step
    if not 0 <= opt_steps <= ck["global_step"]:  # (checkpoints written elsewhere may count differently: report, do not refuse)
        print(f"[load_ckpt] optimizer step {opt_steps} outside [0, global_step = {ck['global_step']}]")
    return ck["global_step"], ck["local_step"], ck["epoch"], int(ck.get("data_cursor", 0)), int(ck.get("optimizer_steps", opt_steps))


def get_run_id(args, rank, world_size):
    """Run id bookkeeping of main() (train_timestamps.py:2182-2196): {run_id_dir}/{exp_name}.txt names the run whose
    checkpoint directory is {ckpt_dir}/{exp_name}_{run_id}; a new id is drawn when there is none (the reference takes
    W&B's)."""
    path = os.path.join(args.run_id_dir, f"{args.exp_name}.txt")
    run_id = None
    if os.path.exists(path):
        run_id = open(path).read().strip()
        if not os.path.exists(run_dir(args, run_id)):
            run_id = None
    if run_id is None:
        import uuid
        obj = [uuid.uuid4().hex[:8] if rank == 0 else None]
        if world_size > 1:
            dist.broadcast_object_list(obj, src=0)
        run_id = obj[0]
        if rank == 0:
            os.makedirs(args.run_id_dir, exist_ok=True)
            with open(path, "w") as f:
                f.write(run_id)
    return run_id


def gen_pred(logits, text_y):
    """gen_pred (train_timestamps.py:1077-1122) at token level: ``pred = argmax(softmax(logits))`` per position (a HIP
    kernel over the fp32 logits: argmax is invariant under softmax), predictions cut after the first <|endoftext|>
    (remove_after_endoftext), targets with the 51864 padding filtered out and closed by <|endoftext|>.  Decoding ids to text
    (tokenizer.decode_with_timestamps) and the WER on text need the un-vendored tokenizer / jiwer: callers get ids."""
    from olmoasr_amd import ops
    B, S, V = logits.shape
    pred, _ = ops.pick_tokens(logits.reshape(B * S, V), want_logprob=False)
    preds, tgts = [], []
    for row in pred.view(B, S).cpu().tolist():
        preds.append(row[:row.index(50256) + 1] if 50256 in row else row)
    for row in text_y.cpu().tolist():
        row = [t for t in row if t != 51864]
        tgts.append((row[:row.index(50256)] if 50256 in row else row) + [50256])
    return preds, tgts


def token_error_counts(preds, tgts):
    """(edit distance summed over the pairs, reference tokens): numerator and denominator of ``token_error_rate``."""
    errs = n = 0
    for p, t in zip(preds, tgts):
        prev = list(range(len(t) + 1))
        for i, a in enumerate(p, 1):
            cur = [i]
            for j, b in enumerate(t, 1):
                cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a != b)))
            prev = cur
        errs += prev[-1]
        n += len(t)
    return errs, n


def token_error_rate(preds, tgts):
    """Token-level analogue of calc_pred_wer (:1125-1180): (substitutions + deletions + insertions) / reference tokens."""
    errs, n = token_error_counts(preds, tgts)
    return errs / max(1, n)


def evaluate(net, indices, dev, timestamps=False, sample_len=32, batch=8, error_counts="host"):
    """evaluate() of the reference (train_timestamps.py:1835-1919) on held-out SYNTHETIC clips (the eval sets themselves are
    out of scope): greedy ``model.decode(audio_input, DecodingOptions(language="en", without_timestamps=True))`` (:1916-1919),
    scored as token error rate against the transcript ids (``error_counts="device"``: by ops.edit_counts instead of the Python loop)."""
    from olmoasr_amd import ops
    from olmoasr_amd.decoding import DecodingOptions
    from olmoasr_amd.synth import synth_samples
    preds, tgts = [], []
    for i in range(0, len(indices), batch):
        pcm, ti, ty, tl = synth_samples(indices[i:i + batch], dev, timestamps)
        res = net.decode(ops.log_mel(pcm), DecodingOptions(language="en", without_timestamps=True, sample_len=sample_len))
        preds += [r.tokens for r in res]
        tgts += [[t for t in row[1:n] if t < 50257][:sample_len] for row, n in zip(ti.cpu().tolist(), tl.cpu().tolist())]
    if error_counts == "device":
        from olmoasr_amd import metrics
        counter = metrics.ErrorCounter(dev)
        counter.add_sequences(*metrics.pad_sequences(preds, dev), *metrics.pad_sequences(tgts, dev))
        return counter.rate()
    return token_error_rate(preds, tgts)


def validate(net, dev, rank, world_size, batch, *, indices=None, shards=None, timestamps=False):
    """One pass over the validation set (``indices``: synthetic sample ids; else the first samples of ``shards``): this rank scores
    ddp.shard_indices of it with ``net.score``, never augmented.  Returns ONE float64 device tensor [8] = ValidationTotals.packed() followed
    by the (S, D, I, H) counts of the teacher-forced predictions, summed over the ranks; nothing is read here."""
    from olmoasr_amd import ddp, metrics, validation
    n = len(indices) if indices is not None else len(shards)
    mine = ddp.shard_indices(n, rank, world_size)

    def fetch(pos):  # positions in this rank's share -> a host batch
        if indices is not None:
            return validation.synthetic_batch([indices[mine[j]] for j in pos], timestamps)
        return validation.shard_batch(shards, [mine[j] for j in pos])
    totals, counter = metrics.ValidationTotals(dev), metrics.ErrorCounter(dev)
    for _ in validation.score_set(net, len(mine), fetch, dev, batch, totals, counter):
        pass
    t = torch.cat([totals.packed(), counter.total.double()])
    if world_size > 1:
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t


def val_record(t, global_step):
    """The "val" log record from ``validate``'s tensor: the one device-to-host copy of a validation pass."""
    from olmoasr_amd import metrics
    t = t.cpu()
    rec = metrics.ValidationTotals().load_packed(t[:4]).record()
    sdih = [int(round(v)) for v in t[4:].tolist()]
    return {"event": "val", "global_step": global_step, "val_loss": rec["val_loss"], "val_token_acc": rec["val_token_acc"],
            "val_n_tokens": rec["val_n_tokens"], "val_n_samples": rec["val_n_samples"], "val_subs": sdih[0], "val_dels": sdih[1], "val_ins": sdih[2]}


def host_cores():
    n = len(os.sched_getaffinity(0))
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = max(1, min(n, int(float(q) / float(p))))
    except Exception:
        pass
    return n


def main(argv=None):
    args = parse_args(argv)
    from olmoasr_amd import augment, ddp, ops
    from olmoasr_amd.config.model_dims import VARIANT_TO_DIMS
    from olmoasr_amd.model import OLMoASR
    from olmoasr_amd.synth import SynthLoader

    local_rank = int(os.environ.get("LOCAL_RANK", "0"))          # env rank discovery, train_timestamps.py:2227-2230
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1")))
    rank = int(os.environ.get("RANK", "0"))
    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    force_dist = bool(args.force_dist) and world_size == 1
    own_group = (world_size > 1 or force_dist) and not dist.is_initialized()
    if own_group and not force_dist:
        # world_size > 1: every rank must name the SAME rendezvous, so it has to come from the launcher (torchrun exports both).  A
        # per-process default would make each rank wait on a different port until the RCCL timeout instead of failing here.
        missing = [k for k in ("MASTER_ADDR", "MASTER_PORT") if k not in os.environ]
        if missing:
            raise SystemExit(f"train_timestamps.py: WORLD_SIZE={world_size} but {' and '.join(missing)} not set -- launch with "
                             f"torchrun (train_timestamps.py:2227-2230 reads the same environment), or export them for every rank")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if own_group:
        if force_dist:  # the single-rank rehearsal needs no launcher: loopback rendezvous on a port of its own
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", str(29500 + os.getpid() % 400))
        dist.init_process_group("nccl", device_id=dev, rank=rank, world_size=world_size, pg_options=ddp.rccl_options())  # RCCL over xGMI

    betas = tuple(args.betas)
    dims = VARIANT_TO_DIMS[args.model_variant]
    net = OLMoASR(dims, device=dev, seed=args.seed, compute_dtype=args.precision)
    if args.lora_rank:
        from olmoasr_amd import lora
        lora.add_lora(net, r=args.lora_rank, alpha=args.lora_alpha, target_modules=args.lora_targets, seed=args.seed)
    if args.freeze_encoder:
        net.encoder.requires_grad_(False)
    ddp.broadcast_parameters(net.flat_params)  # DDP ctor _sync_module_states
    net.refresh_shadow()
    sharded = None
    if int(args.zero_stage) == 1:
        from olmoasr_amd import zero
        sharded = zero.ShardedOptimizer(net.flat_params, net.flat_grads, zero.NativeBackend(net), force=force_dist)  # moments for the owned range only
    else:
        net.init_optimizer_state()
    reducer = (ddp.GradReducer(net.flat_grads, net.grad_segments, bucket_cap_mb=args.bucket_cap_mb, algo=args.reducer, force=force_dist,
                               trainable=net.trainable_ranges())
               if (world_size > 1 or force_dist) and sharded is None else None)
    scaler = GradScalerState()
    accum = accumulation_steps(args.eff_batch_size, world_size, args.train_batch_size)
    mine = ddp.shard_indices(args.n_synthetic, rank, world_size)
    # label smoothing / z-loss: the objective's two parts sit behind the loss in ONE buffer, so a logging step still reads the device once
    regularised = args.label_smoothing > 0.0 or args.z_loss > 0.0
    loss_all = torch.zeros(3 if regularised else 1, device=dev)
    loss_buf = loss_all[:1]
    step_reg = dict(label_smoothing=args.label_smoothing, z_loss=args.z_loss, loss_parts_out=loss_all[1:]) if regularised else {}
    global_step, local_step, cursor, epoch, optimizer_steps = 0, 0, 0, 0, 0
    run_id = get_run_id(args, rank, world_size)
    if args.resume or args.ckpt_file_name:
        global_step, local_step, epoch, cursor, optimizer_steps = load_ckpt(net, scaler, find_ckpt(args, run_id), sharded)
    # every rank of a node shares the host cores: the reference's --num_workers is per rank, but oversubscribing a 16-core
    # cgroup with 8 x 10 generator threads would make the loader, not the GPU, set the pace
    workers = max(1, min(int(args.num_workers), host_cores() // max(1, local_world)))
    log = []
    if rank == 0:
        print(json.dumps({"event": "start", "world_size": world_size, "accumulation_steps": accum, "model": args.model_variant,
                          "precision": args.precision, "params": net.flat_params.numel(), "run_id": run_id, "loader_threads": workers,
                          "hardware_peak_flops": HARDWARE_TO_FLOPS.get(args.hardware)}), flush=True)

    def batch_order(start):  # the sampler: this rank's shard, cyclic, train_batch_size indices per micro-batch
        c = start
        while True:
            yield [mine[(c + j) % len(mine)] for j in range(args.train_batch_size)]
            c += args.train_batch_size
            if c >= len(mine):
                c = 0

    # --samples_dicts_dir (with --synthetic False): the reference's shard files through the on-device input path (olmoasr_amd/data.py)
    real_data = bool(args.samples_dicts_dir) and not bool(args.synthetic)
    if real_data:
        from olmoasr_amd import data
        shards = data.AudioTextShards(data.load_samples_dicts(args.samples_dicts_dir))
        per_rank = -(-len(shards) // world_size)  # DistributedSampler pads every rank's share to ceil(n / world)
        if rank == 0:
            print(json.dumps({"event": "data", "samples": len(shards), "per_rank": per_rank, "shuffle": bool(args.shuffle)}), flush=True)
        loader = data.ShardLoader(shards, data.epoch_batches(len(shards), rank, world_size, args.train_batch_size, epoch, cursor, bool(args.shuffle)),
                                  dev, batch=args.train_batch_size, workers=workers, depth=max(1, int(args.prefetch_factor)))
    else:
        per_rank = len(mine)
        loader = SynthLoader(batch_order(cursor), dev, workers=workers, depth=max(1, int(args.prefetch_factor)), timestamps=bool(args.timestamps))
    held_out = [args.n_synthetic + i for i in range(8)]  # evaluate(): clips outside every rank's training shard (never masked)
    val_set = {}
    if args.val_freq:
        if args.val_samples_dicts_dir:
            from olmoasr_amd import data
            val_samples = data.load_samples_dicts(args.val_samples_dicts_dir)[:int(args.n_val)]
            val_set = dict(shards=data.AudioTextShards(val_samples))
        else:
            val_set = dict(indices=val_indices(args), timestamps=bool(args.timestamps))
    policy, spec_seed = args.spec_policy, int(args.seed) & ((1 << 64) - 1)
    if policy is not None and rank == 0:
        print(json.dumps({"event": "spec_augment", "policy": args.spec_augment, "freq_masks": policy.freq_masks, "freq_width": policy.freq_width,
                          "time_masks": policy.time_masks, "time_width": policy.time_width, "time_ratio": policy.time_ratio,
                          "fill": policy.fill if math.isfinite(policy.fill) else str(policy.fill), "seed": spec_seed}), flush=True)
    speed = args.speed_policy
    if speed is not None and rank == 0:
        print(json.dumps({"event": "speed_perturb", "policy": args.speed_perturb, "factors": [list(pq) for pq in speed.factors],
                          "seed": spec_seed}), flush=True)
    noise = args.noise_policy
    if noise is not None:
        noise_bank = load_noise_bank(args.noise_bank).to(dev)
        if rank == 0:
            print(json.dumps({"event": "noise_mix", "bank": list(noise_bank.shape), "prob": noise.prob, "snr_db": list(noise.snr_db),
                              "seed": spec_seed}), flush=True)
    reverb = args.reverb_policy
    if reverb is not None:
        rir_bank, rir_delay = (t.to(dev) for t in load_rir_bank(args.rir_bank))
        if rank == 0:
            print(json.dumps({"event": "reverb", "bank": list(rir_bank.shape), "prob": reverb.prob, "seed": spec_seed}), flush=True)
    phone = args.telephone_policy
    if phone is not None and rank == 0:
        print(json.dumps({"event": "telephone", "prob": phone.prob, "codecs": list(phone.codecs), "bandpass": phone.bandpass, "seed": spec_seed}),
              flush=True)
    if regularised and rank == 0:
        print(json.dumps({"event": "loss_regularisers", "label_smoothing": args.label_smoothing, "z_loss": args.z_loss}), flush=True)
    device_counts = args.train_error_counts == "device"
    if device_counts:
        from olmoasr_amd import metrics
        counter = metrics.ErrorCounter(dev)
        pred_buf = torch.empty(args.train_batch_size, dims.n_text_ctx, dtype=torch.int32, device=dev)
    while global_step < args.train_steps:
        start_step = time.time()
        net.zero_grad()
        log_now = ((global_step + 1) % args.train_log_freq) == 0  # gen_pred condition of the reference (:1480)
        preds, tgts = [], []
        spec_cells = 0  # cells masked on this rank in this step: from the host plan, no device read-back
        speed_counts = [0] * (len(speed.factors) + 1) if speed is not None else None  # this rank's clips per factor (last entry: fell back to the copy): from the host plan too
        noise_drawn = noise_snr_sum = 0  # this rank's clips that drew noise in this step and the sum of their SNRs: from the host plan too
        reverb_drawn = 0  # this rank's clips that drew a room response in this step: from the host plan too
        phone_counts = {}  # this rank's clips that drew the telephone channel in this step, per codec: from the host plan too
        for i in range(accum):
            pcm, ti, ty, tl = next(loader)
            cursor += args.train_batch_size  # (position in this rank's epoch order; a short last batch also ends the epoch)
            if cursor >= per_rank:
                cursor, epoch = 0, epoch + 1
            last = i == accum - 1
            # (a logging step with --train_error_counts=host wants the logits back: it takes the plain step; every other step limits the decoder's
            # backward to the span and lets the encoder's transpose apply the log-mel floor / scale instead of a second pass over the tensor)
            use_span = bool(args.span_backward) and (device_counts or not log_now)
            want_pred = device_counts and log_now
            if speed is not None:  # a new pcm tensor; the timestamp ids of ti / ty move in place (the token count, hence the span, stays)
                first = spec_offset(global_step, i, accum, world_size, rank, args.train_batch_size) & ((1 << 64) - 1)
                n_samples = int(pcm.shape[1])
                pcm, n_speed, _ = speed.apply(pcm, loader.last_n_valid, spec_seed, first, tokens=(ti, ty))
                speed_counts = [c + d for c, d in zip(speed_counts, speed.factor_counts(spec_seed, first, loader.last_n_valid_host.tolist(), n_samples))]
            n_cur, ours = (n_speed, True) if speed is not None else (loader.last_n_valid, False)  # the clips' lengths; is pcm a tensor of this step's
            if reverb is not None:  # out of place: a new pcm tensor; the length speed perturbation left stays, and so do the timestamps
                first = spec_offset(global_step, i, accum, world_size, rank, args.train_batch_size) & ((1 << 64) - 1)
                pcm, ours = reverb.apply(pcm, n_cur, rir_bank, rir_delay, spec_seed, first)[0], True
                reverb_drawn += reverb.drawn(spec_seed, first, int(pcm.shape[0]), int(rir_bank.shape[0]))
            if noise is not None:  # on the clip as the log-mel will see it: its length is what speed perturbation left (in place on a new tensor)
                first = spec_offset(global_step, i, accum, world_size, rank, args.train_batch_size) & ((1 << 64) - 1)
                if ours:
                    noise.apply(pcm, n_cur, noise_bank, spec_seed, first, out=pcm)
                else:
                    pcm = noise.apply(pcm, n_cur, noise_bank, spec_seed, first)[0]
                d_, s_ = noise.drawn(spec_seed, first, int(pcm.shape[0]), *noise_bank.shape)
                noise_drawn, noise_snr_sum = noise_drawn + d_, noise_snr_sum + s_
            if phone is not None:  # last on the PCM: the channel carries the noise too (out of place: a new pcm tensor; lengths and timestamps stay)
                first = spec_offset(global_step, i, accum, world_size, rank, args.train_batch_size) & ((1 << 64) - 1)
                pcm = phone.apply(pcm, n_cur, spec_seed, first)[0]
                for name, c in phone.drawn(spec_seed, first, int(pcm.shape[0])).items():
                    phone_counts[name] = phone_counts.get(name, 0) + c
            if policy is not None:  # masks go on the FINALIZED log-mel, so the span step takes it finalized as well (mel_clip_max=None)
                mel, clip_max = ops.log_mel(pcm), None
                first = spec_offset(global_step, i, accum, world_size, rank, args.train_batch_size) & ((1 << 64) - 1)
                policy.apply_(mel, spec_seed, first)
                spec_cells += augment.masked_cells(policy, spec_seed, first, *mel.shape)
            else:
                mel, clip_max = ops.log_mel(pcm, finalize=False) if use_span else (ops.log_mel(pcm), None)
            _, logits = net.loss_and_backward(mel, ti, ty, tl, loss_scale=scaler.scale, accumulation_steps=accum, loss_out=loss_buf,
                                              accumulate_loss=i > 0, return_logits=log_now and not device_counts,
                                              segment_events=reducer.segment_events() if (reducer and last) else None,
                                              span=loader.last_span if use_span else None, mel_clip_max=clip_max,
                                              span_forward=use_span and bool(args.span_forward),
                                              **({"pred_out": pred_buf[:ti.shape[0]]} if want_pred else {}), **step_reg)
            if want_pred:
                if i == 0:
                    counter.reset()
                counter.add(pred_buf[:ti.shape[0]], ty)
            elif log_now:
                p_, t_ = gen_pred(logits, ty)
                preds += p_
                tgts += t_
            local_step += 1
        div = 1.0
        if reducer:
            reducer.reduce()
            div = reducer.grad_divisor
        lr = args.lr * lr_lambda(global_step, args.train_steps)
        # torch's AdamW advances its per-parameter step only when GradScaler lets the step through: the bias correction
        # follows the number of APPLIED steps, not global_step
        hyper = dict(step=optimizer_steps + 1, lr=lr, max_grad_norm=args.max_grad_norm, betas=betas, eps=args.eps, weight_decay=args.weight_decay)
        if sharded is not None:
            stats = sharded.step(inv_loss_scale=1.0 / (scaler.scale * sharded.grad_divisor), **hyper)
        else:
            stats = net.optim_step(inv_loss_scale=1.0 / (scaler.scale * div), **hyper)
        found_inf = bool(stats[1].item() != 0)  # host sync once per optimizer step, like scaler.step()
        scaler.update(found_inf)
        if not found_inf:
            optimizer_steps += 1
        global_step += 1
        time_per_step = time.time() - start_step
        throughput = ((args.train_batch_size * accum * 30) / 60) / time_per_step  # audio_min_per_GPU_second (:1525-1527)
        if global_step % args.train_log_freq == 0 or global_step == 1:
            scored = device_counts and global_step % args.train_log_freq == 0  # (global_step was advanced: this is log_now of the step just run)
            if scored:  # the counts ride with the loss: one all-reduce, one read (float64 holds both exactly enough: counts < 2^53)
                t = torch.cat([loss_all.double(), counter.total.double()])
            else:
                t = loss_all.clone()
            if world_size > 1:
                dist.all_reduce(t, op=dist.ReduceOp.SUM)
            if scored or regularised:
                t, *rest = t.cpu().tolist()  # the step's one read of the device: loss, its parts and the counts together
                parts, sdih = rest[:loss_all.numel() - 1], [int(v) for v in rest[loss_all.numel() - 1:]]
            if rank == 0:
                rec = {"global_step": global_step, "train_loss": float(t) / world_size, "lr": lr, "loss_scale": scaler.scale,
                       "time_per_step": round(time_per_step, 4), "audio_min_per_GPU_second": round(throughput, 3),
                       "audio_sec_per_sec_node": round(throughput * 60 * world_size, 1), "found_inf": found_inf,
                       "spec_masked_cells": spec_cells}
                if speed is not None:
                    rec["speed_factor_counts"] = speed_counts
                if noise is not None:
                    rec.update(noise_drawn=noise_drawn, noise_snr_db_mean=round(noise_snr_sum / noise_drawn, 3) if noise_drawn else None)
                if reverb is not None:
                    rec["reverb_drawn"] = reverb_drawn
                if phone is not None:
                    rec.update(telephone_drawn=sum(phone_counts.values()), telephone_codec_counts=phone_counts)
                if regularised:
                    rec.update(train_nll=parts[0] / world_size, train_lse_sq=parts[1] / world_size)
                if preds:
                    rec["train_token_error_rate"] = round(token_error_rate(preds, tgts), 4)
                if scored:
                    errs, n_ref = metrics.ErrorCounter.fraction(sdih)
                    rec.update(train_token_error_rate=round(errs / max(1, n_ref), 4), train_subs=sdih[0], train_dels=sdih[1], train_ins=sdih[2])
                log.append(rec)
                print(json.dumps(rec), flush=True)
        if args.val_freq and global_step % int(args.val_freq) == 0:
            t_val = time.time()
            rec = val_record(validate(net, dev, rank, world_size, int(args.val_batch_size), **val_set), global_step)
            if rank == 0:
                rec["val_seconds"] = round(time.time() - t_val, 4)
                log.append(rec)
                print(json.dumps(rec), flush=True)
        if args.run_eval and args.eval_freq and global_step % int(args.eval_freq) == 0 and rank == 0:
            print(json.dumps({"event": "eval", "global_step": global_step,
                              "token_error_rate": round(evaluate(net, held_out, dev, bool(args.timestamps), error_counts=args.train_error_counts), 4)}), flush=True)
        if args.ckpt_freq and global_step % args.ckpt_freq == 0:
            save_ckpt(net, scaler, global_step, local_step, epoch, args, dims, rank, run_id, cursor, optimizer_steps, sharded=sharded)
    loader.close()
    if args.ckpt_freq and (global_step % args.ckpt_freq) != 0:
        save_ckpt(net, scaler, global_step, local_step, epoch, args, dims, rank, run_id, cursor, optimizer_steps, sharded=sharded)
    if own_group:
        dist.barrier()
        dist.destroy_process_group()
    return log


if __name__ == "__main__":
    main()
