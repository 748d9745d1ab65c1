"""LoRA fine-tuning of the native model -- what ``peft.get_peft_model(model, LoraConfig(r, lora_alpha, target_modules))`` does to the
reference's ``nn.Linear`` layers, built into the engine.

An adapted ``Linear`` with weight ``W0 [out, in]`` gains ``lora_A [r, in]`` and ``lora_B [out, r]`` and computes with

    W = W0 + (alpha / r) * lora_B @ lora_A

(= a ``torch.nn.utils.parametrize`` LoRA parametrization of the weight).  ``W0`` is frozen, the adapters are ordinary trainable
parameters: ``.grad`` views of the gradient arena, stepped by ``OLMoASR.optim_step`` or any ``torch.optim`` optimizer.  Wrapping
``nn.Linear`` modules in Python would change nothing here -- the engine runs whole stacks from the flat arena -- so ``add_lora``
re-creates the engine context with the adapters in its parameter table (``oasr_create_ex3``)::

    model = hub.load_for_finetuning("medium")
    lora.add_lora(model, r=16, alpha=32)                 # query / value of every attention block, base frozen
    ... train ...
    torch.save(lora.lora_state_dict(model), "adapter.pt")   # ~12.6 MB for medium instead of 3 GB
    lora.merge_lora(model)                               # plain OLMoASR state_dict again
"""
import fnmatch
import math
import re
from typing import Iterable, List, Sequence

import torch

from . import _native as N

DEFAULT_TARGETS = ("*.attn.query", "*.attn.value")
# the Linears the engine can adapt: every projection of a residual block (self / cross attention, MLP); not the token embedding (tied to
# the logits) and not the conv stem
_TARGETABLE = re.compile(r"^(encoder|decoder)\.blocks\.\d+\.((cross_)?attn\.(query|key|value|out)|mlp\.[02])$")


def _is_pattern(p: str) -> bool:
    return any(ch in p for ch in "*?[")


def resolve_targets(names: Iterable[str], patterns) -> List[str]:
    """The module names (of ``names``, in their order) that ``patterns`` select.  A pattern with a wildcard is an ``fnmatch`` pattern over
    the whole name (``*.attn.query`` matches ``decoder.blocks.3.attn.query``, not ``decoder.blocks.3.cross_attn.query``); a plain name
    matches itself and, like peft's ``target_modules``, every name ending in ``.`` + it.  Raises ValueError when a pattern matches nothing
    or selects a module the engine cannot adapt (the token embedding, the conv stem, LayerNorms, containers)."""
    if isinstance(patterns, str):
        patterns = [patterns]
    patterns = list(patterns)
    if not patterns:
        raise ValueError("resolve_targets: no target patterns")
    names = list(names)
    out, hit = [], {p: False for p in patterns}
    for n in names:
        sel = False
        for p in patterns:
            m = fnmatch.fnmatchcase(n, p) if _is_pattern(p) else (n == p or n.endswith("." + p))
            if m:
                hit[p] = sel = True
        if sel:
            if not _TARGETABLE.match(n):
                raise ValueError(f"LoRA target {n!r} is not a block Linear: adapters go on attn / cross_attn query|key|value|out and mlp.0 / "
                                 "mlp.2 of the encoder and decoder blocks (not the token embedding, the conv stem or a LayerNorm)")
            out.append(n)
    missing = [p for p, h in hit.items() if not h]
    if missing:
        raise ValueError(f"LoRA target pattern(s) {missing} match no module")
    return out


def lora_modules(model) -> List[str]:
    """Names of the adapted modules, in parameter-table order."""
    return [name[: -len(".lora_A")] for name, *_ in model._table if name.endswith(".lora_A")]


def add_lora(model, r: int = 16, alpha: float = 32, target_modules: Sequence[str] = DEFAULT_TARGETS, seed: int = 0,
             lora_dropout: float = 0.0) -> List[str]:
    """Adds rank-``r`` adapters with scale ``alpha / r`` to the modules ``target_modules`` selects (``resolve_targets``), freezes every base
    parameter and re-creates the engine context and arena (base weights kept).  ``lora_A`` is kaiming-uniform (a = sqrt(5), peft's init)
    from ``torch.Generator().manual_seed(seed)``, ``lora_B`` zeros: the adapted model computes exactly what the base model computes until
    ``lora_B`` moves.  Call it before the gradient arena, the optimizer state or a data-parallel wrapper exists.  Returns the adapted
    module names."""
    if lora_dropout:
        raise ValueError("lora_dropout != 0 is not supported: the adapters live in weight space (W0 + s * B @ A), where there is no "
                         "adapter-input activation to drop out")
    r = int(r)
    if not 1 <= r <= N.LORA_MAX_RANK:
        raise ValueError(f"LoRA rank must be in 1..{N.LORA_MAX_RANK}, got {r}")
    if lora_modules(model):
        raise N.NativeError("the model already carries LoRA adapters: merge_lora() them first")
    if model.inference:
        raise N.NativeError("add_lora needs the training layout (OLMoASR(..., inference=False), hub.load_for_finetuning)")
    from .model import Linear
    linears = [n for n, m in model.named_modules() if n]
    targets = resolve_targets(linears, target_modules)
    assert all(isinstance(model.get_submodule(n), Linear) for n in targets)
    index = {name: i for i, (name, *_) in enumerate(model._table)}
    idx = [index[t + ".weight"] for t in targets]
    scale = float(alpha) / r
    gen = torch.Generator().manual_seed(int(seed))

    def init(name, t):
        if name.endswith(".lora_A"):
            a = torch.empty(t.shape)
            torch.nn.init.kaiming_uniform_(a, a=math.sqrt(5), generator=gen)
            t.copy_(a)
        else:
            t.zero_()

    for p in model.parameters():
        p.requires_grad_(False)
    with torch.no_grad():
        model._swap_context(idx, r, scale, init)
    for t in targets:
        mod = model.get_submodule(t)
        mod.lora_scale = scale
    model.lora_config = {"r": r, "lora_alpha": alpha, "target_modules": list(targets), "lora_dropout": 0.0}
    return targets


def lora_state_dict(model) -> dict:
    """The adapter tensors only (``<module>.lora_A`` / ``.lora_B``), detached CPU copies."""
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if k.endswith(".lora_A") or k.endswith(".lora_B")}


def load_lora_state_dict(model, sd: dict) -> None:
    """Loads adapter tensors saved by ``lora_state_dict`` into a model with the same adapters (``add_lora`` with the same targets / r)."""
    own = {k: v for k, v in model.state_dict().items() if k.endswith(".lora_A") or k.endswith(".lora_B")}
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    if set(sd) != set(own):
        raise KeyError(f"adapter keys differ: missing {sorted(set(own) - set(sd))[:4]}, unexpected {sorted(set(sd) - set(own))[:4]}")
    with torch.no_grad():
        for k, v in sd.items():
            if tuple(v.shape) != tuple(own[k].shape):
                raise ValueError(f"{k}: shape {tuple(v.shape)} vs {tuple(own[k].shape)}")
            own[k].copy_(v.to(own[k].device, torch.float32))
    model.refresh_shadow()


def merge_lora(model) -> None:
    """Folds the adapters into the base weights (W0 <- W0 + s * B @ A, the fp32 value the compute copy is rounded from) and removes them:
    ``state_dict()`` then has the keys and shapes of a model that never had adapters.  Base parameters stay frozen (as peft's
    ``merge_and_unload`` leaves them)."""
    if not lora_modules(model):
        raise N.NativeError("merge_lora: the model has no LoRA adapters")
    names = lora_modules(model)
    N.call("oasr_lora_merge", model._ctx, N.STREAM, device=model.device)
    with torch.no_grad():
        model._swap_context((), 0, 0.0, None)
    for t in names:
        mod = model.get_submodule(t)
        mod.__dict__.pop("lora_scale", None)
    model.__dict__.pop("lora_config", None)
