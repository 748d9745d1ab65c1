"""model.encoder(mel) and model.decoder(tokens, xa) as differentiable modules: the staged autograd entries
(oasr_train_encode / _encode_bwd / _decode / _decode_bwd), d(mel) through the conv1 fold kernel (csrc/conv_grad.hip), and the fused step
from given encoder features (loss_and_backward(None, ..., audio_features=xa), oasr_train_step from xa).

"The fused rule" below is test_gpu_freeze.py's: bit-identical where the fused step repeats bit-identically, otherwise within 4x its own
run-to-run spread (split-K weight gradients accumulate with fp32 atomics).  The stages keep their activations in other buffers than the fused
step, and the order of fp32 atomic adds can follow the buffers' placement, so "bit-identical" admits ulps of a tensor's largest entry.  Oracle bounds are those of test_gpu_freeze.py /
test_gpu_model.py: fp32 rel-L2 <= 1e-3 per tensor; bf16 <= max(2 x the bf16 mirror's error, 3 %) per tensor with cosine > 0.999."""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 51864
DTYPES = ["float32", "bfloat16"]


def _dims(mo_dims):
    from olmoasr_amd.config.model_dims import ModelDimensions
    return ModelDimensions(**{k: getattr(mo_dims, k) for k in ModelDimensions.__dataclass_fields__})


def _net(c, dtype, lora_targets=None):
    from olmoasr_amd.model import OLMoASR
    net = OLMoASR(_dims(c["dims"]), device=DEV, seed=0, compute_dtype=dtype)
    net.load_state_dict(c["sd"])
    if lora_targets:
        from olmoasr_amd import lora
        lora.add_lora(net, r=16, alpha=32, target_modules=lora_targets, seed=0)
        g = torch.Generator().manual_seed(100)
        with torch.no_grad():
            for n, p in net.named_parameters():
                if n.endswith(".lora_B"):
                    p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        net.refresh_shadow()
    return net


def _args(c):
    return c["mel"].to(DEV), c["tokens"].to(DEV), c["targets"].to(DEV), c["text_len"].to(DEV)


def _mask(tl):
    m = torch.zeros(tl.numel(), 448, 448)
    for b, n in enumerate(tl.tolist()):
        m[b, :, n:] = -float("inf")
    return m.to(DEV)


def _ce(logits, targets):
    return F.cross_entropy(logits.view(-1, logits.shape[-1]), targets.view(-1), ignore_index=PAD)


def _grads(net):
    return {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in net.named_parameters()}


def _fused_rule(got, ref0, ref1, what=""):
    """got vs ref0, with ref1 a second run of ref0's computation (dicts of tensors or tensors)."""
    if isinstance(got, dict):
        for k in got:
            _fused_rule(got[k], ref0[k], ref1[k], f"{what}{k}")
        return
    if got is None:
        assert ref0 is None and ref1 is None, what
        return
    # bit-identical where the fused step repeats bit-identically, else within 4x its spread -- up to the order of fp32 atomic adds, which can
    # follow where the buffers sit (the token embedding's scatter, LayerNorm bias sums, split-K weight gradients): a change of order moves an
    # entry by ulps of the tensor's largest entry
    diff = float((got - ref0).abs().max())
    floor = float(ref0.abs().max()) * 2.0 ** -16
    spread = float((ref1 - ref0).abs().max())
    assert diff <= max(4 * spread, floor), (what, diff, spread, floor)


def _staged_step(net, c, mel=None):
    mel_d, tok, tgt, tl = _args(c)
    xa = net.encoder(mel_d if mel is None else mel)
    logits = net.decoder(tok, xa, padding_mask=_mask(c["text_len"]))
    _ce(logits, tgt).backward()
    torch.cuda.synchronize()
    return logits.detach(), _grads(net)


def _fused_graph_step(net, c):
    mel_d, tok, tgt, tl = _args(c)
    logits = net(mel_d, tok, _mask(c["text_len"]))
    _ce(logits, tgt).backward()
    torch.cuda.synchronize()
    return logits.detach(), _grads(net)


# ---- 1. the stages compose to the fused training graph ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_stages_equal_the_fused_graph(tiny_case, dtype):
    c = tiny_case
    net = _net(c, dtype)
    xa = net.encoder(c["mel"].to(DEV))
    assert xa.requires_grad and xa.grad_fn is not None and xa.dtype == net._act_dtype
    ls, gs = _staged_step(_net(c, dtype), c)
    l0, g0 = _fused_graph_step(_net(c, dtype), c)
    l1, g1 = _fused_graph_step(_net(c, dtype), c)
    assert torch.equal(ls, l0)
    _fused_rule(gs, g0, g1)
    if dtype == "float32":  # training-mode and inference forwards are bit-equal in fp32 (test_gpu_fp32_mode.py): so are the stages
        mel_d, tok, _, _ = _args(c)
        xa = net.encoder(mel_d)
        assert torch.equal(xa.detach(), net.embed_audio(mel_d))
        lg = net.decoder(tok, xa.detach(), padding_mask=_mask(c["text_len"]))
        assert lg.requires_grad and torch.equal(lg.detach(), net.logits(tok, xa.detach(), _mask(c["text_len"])))


def test_stages_equal_the_fused_graph_medium():
    """The same comparison at medium dims, B = 2 (bf16 production engine, seeded weights)."""
    from oracle import mel_oracle as me
    from oracle import model_oracle as mo
    from olmoasr_amd.model import OLMoASR
    import numpy as np
    dims = mo.VARIANTS["medium"]
    pcm, ti, ty, tl = mo.synthetic_batch([0, 1])
    c = dict(mel=torch.from_numpy(me.log_mel_batch(pcm.numpy(), dtype=np.float32)), tokens=ti, targets=ty, text_len=tl)
    nets = [OLMoASR(_dims(dims), device=DEV, seed=0) for _ in range(3)]
    ls, gs = _staged_step(nets[0], c)
    l0, g0 = _fused_graph_step(nets[1], c)
    l1, g1 = _fused_graph_step(nets[2], c)
    assert torch.equal(ls, l0)
    _fused_rule(gs, g0, g1)


# ---- 2./3./4. each stage against the oracle ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def enc_oracle(tiny_case):
    """Encoder-only loss (xa * R).sum() with R zero on sample 1: fp32 oracle and bf16-mirror gradients of the encoder and of mel."""
    from oracle import model_oracle as mo
    c = tiny_case
    torch.set_num_threads(min(32, len(os.sched_getaffinity(0))))
    g = torch.Generator().manual_seed(7)
    R = torch.randn(2, c["dims"].n_audio_ctx, c["dims"].n_audio_state, generator=g)
    R[1] = 0
    out = {"R": R}
    for key, bf in (("fp32", False), ("bf16", True)):
        leaves = {k: v.detach().clone().requires_grad_(k != "encoder.positional_embedding") for k, v in c["sd"].items() if k.startswith("encoder.")}
        mel = c["mel"].clone().requires_grad_(True)
        xa = mo.encoder_forward(leaves, c["dims"], mel, autocast_bf16=bf)
        (xa.float() * R).sum().backward()
        out[key] = ({k: v.grad for k, v in leaves.items() if v.grad is not None}, mel.grad)
    return out


@pytest.fixture(scope="module")
def dec_oracle(tiny_case):
    """Decoder-only CE loss on a random xa: fp32 oracle and bf16-mirror gradients of the decoder and of xa (per engine dtype: xa rounded
    to the engine's activation type first, as the engine stores it)."""
    from oracle import model_oracle as mo
    c = tiny_case
    g = torch.Generator().manual_seed(11)
    xa0 = torch.randn(2, c["dims"].n_audio_ctx, c["dims"].n_audio_state, generator=g)
    out = {"xa": xa0}
    pm = mo.build_padding_mask(c["text_len"], c["dims"].n_text_ctx)
    for dtype in DTYPES:
        xin = xa0 if dtype == "float32" else xa0.bfloat16().float()
        for key, bf in (("fp32", False), ("bf16", True)):
            leaves = {k: v.detach().clone().requires_grad_(True) for k, v in c["sd"].items() if k.startswith("decoder.")}
            xa = xin.clone().requires_grad_(True)
            logits = mo.decoder_forward(leaves, c["dims"], c["tokens"], xa, pm, autocast_bf16=bf)
            mo.loss_fn(logits, c["targets"]).backward()
            out[(dtype, key)] = ({k: v.grad for k, v in leaves.items()}, xa.grad)
    return out


def _check(got, ref, mirror, dtype, what):
    got = got.detach().float().cpu()
    rel = float((got - ref).norm() / (ref.norm() + 1e-12))
    if dtype == "float32":
        assert rel <= 1e-3, (what, rel)
    else:
        env = float((mirror.float() - ref).norm() / (ref.norm() + 1e-12))
        cos = float((got * ref).sum() / (got.norm() * ref.norm() + 1e-20))
        assert rel <= max(2.0 * env, 0.03) and cos > 0.999, (what, rel, env, cos)


@pytest.mark.parametrize("dtype", DTYPES)
def test_encoder_stage_against_the_oracle(tiny_case, enc_oracle, dtype):
    c = tiny_case
    net = _net(c, dtype)
    mel = c["mel"].to(DEV).requires_grad_(True)
    xa = net.encoder(mel)
    (xa.float() * enc_oracle["R"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    (g32, dm32), (gbf, dmbf) = enc_oracle["fp32"], enc_oracle["bf16"]
    for n, p in net.named_parameters():
        if n.startswith("encoder."):
            _check(p.grad, g32[n], gbf[n], dtype, n)
        else:
            assert p.grad is None or not bool(p.grad.any()), n  # the decoder's gradients are untouched
    dmel = mel.grad
    assert dmel.shape == mel.shape and dmel.dtype == torch.float32
    _check(dmel[0], dm32[0], dmbf[0], dtype, "d(mel)")
    for t in (0, mel.shape[-1] - 1):  # the first and last frame: their taps into the zero padding are dropped
        _check(dmel[0, :, t], dm32[0, :, t], dmbf[0, :, t], dtype, f"d(mel)[:, {t}]")
    # the loss reads sample 0 only: a tap that leaks across the sample boundary would make sample 1's d(mel) nonzero
    assert int(torch.count_nonzero(dmel[1])) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_decoder_stage_against_the_oracle(tiny_case, dec_oracle, dtype):
    c = tiny_case
    net = _net(c, dtype)
    xa = dec_oracle["xa"].to(DEV).requires_grad_(True)
    logits = net.decoder(c["tokens"].to(DEV), xa, padding_mask=_mask(c["text_len"]))
    _ce(logits, c["targets"].to(DEV)).backward()
    torch.cuda.synchronize()
    (g32, dx32), (gbf, dxbf) = dec_oracle[(dtype, "fp32")], dec_oracle[(dtype, "bf16")]
    for n, p in net.named_parameters():
        if n.startswith("decoder."):
            _check(p.grad, g32[n], gbf[n], dtype, n)
        else:
            assert p.grad is None or not bool(p.grad.any()), n
    assert xa.grad.dtype == torch.float32 and xa.grad.shape == xa.shape
    _check(xa.grad, dx32, dxbf, dtype, "d(xa)")


@pytest.mark.parametrize("dtype", DTYPES)
def test_frozen_and_all_frozen(tiny_case, enc_oracle, dtype):
    c = tiny_case
    net = _net(c, dtype)
    net.encoder.requires_grad_(False)
    xa = net.encoder(c["mel"].to(DEV))
    assert not xa.requires_grad and net._slots["enc"].buf is None and net._slots["dec"].buf is None  # the inference forward: no graph, no saved activations
    assert torch.equal(xa, net.embed_audio(c["mel"].to(DEV)))
    # every parameter frozen, mel requires grad: saliency -- d(mel) as above, no p.grad, the gradient arena not written
    net = _net(c, dtype)
    net.requires_grad_(False)
    before = net.flat_grads.clone()
    mel = c["mel"].to(DEV).requires_grad_(True)
    (net.encoder(mel).float() * enc_oracle["R"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    (_, dm32), (_, dmbf) = enc_oracle["fp32"], enc_oracle["bf16"]
    _check(mel.grad[0], dm32[0], dmbf[0], dtype, "d(mel), all frozen")
    assert int(torch.count_nonzero(mel.grad[1])) == 0
    assert all(p.grad is None for p in net.parameters())
    assert torch.equal(net.flat_grads, before)
    # the same through the decoder: d(xa) of a frozen decoder
    xa = torch.randn(2, c["dims"].n_audio_ctx, c["dims"].n_audio_state, device=DEV, requires_grad=True)
    _ce(net.decoder(c["tokens"].to(DEV), xa, padding_mask=_mask(c["text_len"])), c["targets"].to(DEV)).backward()
    assert xa.grad is not None and bool(xa.grad.any())
    assert all(p.grad is None for p in net.parameters()) and torch.equal(net.flat_grads, before)
    # the all-frozen error stays for the fused entries
    from olmoasr_amd import _native as N
    with pytest.raises(N.NativeError):
        net.loss_and_backward(*_args(c))


# ---- 5. LoRA ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_lora_adapter_gradients(tiny_case, dtype):
    c = tiny_case
    tg = ("*.attn.query", "*.attn.value")
    _, gs = _staged_step(_net(c, dtype, tg), c)
    _, g0 = _fused_graph_step(_net(c, dtype, tg), c)
    _, g1 = _fused_graph_step(_net(c, dtype, tg), c)
    names = [n for n in gs if ".lora_" in n]
    assert names and all(gs[n] is not None and bool(gs[n].any()) for n in names)
    assert any(n.startswith("encoder.") for n in names) and any(n.startswith("decoder.") for n in names)
    _fused_rule({n: gs[n] for n in names}, g0, g1)


# ---- 6. the fused step from cached encoder features ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_cached_features_step(tiny_case, dtype):
    c = tiny_case
    mel_d, tok, tgt, tl = _args(c)

    def run(features):
        net = _net(c, dtype)
        net.encoder.requires_grad_(False)
        xa = None
        if features == "train":
            xa = net.encoder(mel_d.clone().requires_grad_(True)).detach()  # the training-mode forward: the fused step's own bits
        elif features == "infer":
            xa = net.embed_audio(mel_d)
        losses, grads = [], None
        for step in range(1, 4):
            net.zero_grad()
            if xa is None:
                loss, _ = net.loss_and_backward(mel_d, tok, tgt, tl, span=True)
            else:
                loss, _ = net.loss_and_backward(None, tok, tgt, tl, audio_features=xa, span=True)
            losses.append(loss.clone())
            if step == 1:
                grads = net.flat_grads.clone()
            net.optim_step(step=step, lr=1e-3)
        torch.cuda.synchronize()
        return torch.cat(losses), grads, net.flat_params.clone()

    l0, g0, p0 = run(None)
    l1, g1, p1 = run(None)
    ls, gs, ps = run("train")
    _fused_rule(ls[:1], l0[:1], l1[:1], "loss")
    _fused_rule(gs, g0, g1, "grads")
    _fused_rule(ps, p0, p1, "params after 3 steps")
    li, gi, pi = run("infer")
    if dtype == "float32":
        _fused_rule(gi, g0, g1, "grads (embed_audio)")
        _fused_rule(pi, p0, p1, "params (embed_audio)")
    else:  # the inference GELU epilogue rounds differently: test_gpu_autograd.py's per-tensor bound
        net = _net(c, dtype)
        for name, off, numel, _ in net._table:
            if name.startswith("encoder."):
                continue
            a, b = gi[off:off + numel], g0[off:off + numel]
            assert float((a - b).norm() / (b.norm() + 1e-20)) < 9e-3, name
    net = _net(c, dtype)
    with pytest.raises(ValueError):  # a trainable encoder parameter
        net.loss_and_backward(None, tok, tgt, tl, audio_features=net.embed_audio(mel_d))


# ---- 7. lifetime and workspace hygiene ------------------------------------------------------------------------------------------------
def test_stale_stage_backward_raises(tiny_case):
    c = tiny_case
    net = _net(c, "bfloat16")
    mel_d, tok, tgt, _ = _args(c)
    xa1 = net.encoder(mel_d)
    xa2 = net.encoder(mel_d)
    with pytest.raises(RuntimeError, match="activations of this forward are gone"):
        xa1.float().sum().backward()
    xa2.float().sum().backward()  # the newest forward is still good
    with pytest.raises(RuntimeError):
        xa2 = net.encoder(mel_d)
        loss = xa2.float().sum()
        loss.backward(retain_graph=True)
        loss.backward()  # a second backward through the same stage graph
    lg1 = net.decoder(tok, xa1.detach(), padding_mask=_mask(c["text_len"]))
    net.decoder(tok, xa1.detach(), padding_mask=_mask(c["text_len"]))
    with pytest.raises(RuntimeError, match="activations of this forward are gone"):
        _ce(lg1, tgt).backward()


@pytest.mark.parametrize("dtype", DTYPES)
def test_other_calls_between_stage_forward_and_backward(tiny_case, dtype):
    c = tiny_case
    mel_d, tok, tgt, tl = _args(c)
    _, g0 = _staged_step(_net(c, dtype), c)
    _, g1 = _staged_step(_net(c, dtype), c)
    net = _net(c, dtype)
    pending = net(mel_d, tok, _mask(c["text_len"]))  # a _TrainStep graph
    xa = net.encoder(mel_d)
    logits = net.decoder(tok, xa, padding_mask=_mask(c["text_len"]))
    _ce(pending, tgt).backward()  # the stage forwards did not invalidate the pending fused graph
    net.embed_audio(mel_d)
    net.logits(tok, xa.detach(), _mask(c["text_len"]))
    net(mel_d, tok, _mask(c["text_len"]))
    net.loss_and_backward(mel_d, tok, tgt, tl, span=True)
    net.zero_grad()
    _ce(logits, tgt).backward()
    torch.cuda.synchronize()
    _fused_rule(_grads(net), g0, g1)


@pytest.fixture(scope="module")
def fused_graph_grads(tiny_case):
    """Per compute dtype: the gradients of model(mel, tokens, mask) + backward on two fresh models (_fused_rule's ref0 / ref1)."""
    return {dtype: [_fused_graph_step(_net(tiny_case, dtype), tiny_case)[1] for _ in range(2)] for dtype in DTYPES}


def _interpose(net, c, what):
    mel_d, tok, tgt, tl = _args(c)
    if what == "embed_audio":
        net.embed_audio(mel_d)
    elif what == "logits":
        xa = torch.zeros(2, c["dims"].n_audio_ctx, c["dims"].n_audio_state, device=DEV)
        net.logits(tok, xa, _mask(c["text_len"]))
    elif what == "no_grad_forward":
        with torch.no_grad():
            net(mel_d, tok, _mask(c["text_len"]))
    elif what == "loss_and_backward":
        net.loss_and_backward(mel_d, tok, tgt, tl)
    elif what == "drop_workspace":
        net._workspace = None
    elif what == "to_device":
        net.to(net.device)
    else:
        raise AssertionError(what)


@pytest.mark.parametrize("what", ["embed_audio", "logits", "no_grad_forward", "loss_and_backward", "drop_workspace", "to_device"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_backward_after_the_workspace_was_reused_or_dropped_raises(tiny_case, fused_graph_grads, dtype, what):
    """model(mel, tokens, mask) leaves its activations (and the plan's index tables) in the workspace every other entry of the model plans
    over from offset 0: after any of them, or after the buffer was freed or moved, the backward must refuse in Python -- not run over what
    the later call left there.  The model stays usable: the next forward / backward pair gives a fresh model's gradients."""
    c = tiny_case
    mel_d, tok, tgt, _ = _args(c)
    net = _net(c, dtype)
    loss = _ce(net(mel_d, tok, _mask(c["text_len"])), tgt)
    _interpose(net, c, what)
    with pytest.raises(RuntimeError, match=r"OLMoASR\.forward backward: .*activations of this forward are gone"):
        loss.backward()
    net.zero_grad()  # (loss_and_backward accumulated its own gradients)
    _, gs = _fused_graph_step(net, c)
    g0, g1 = fused_graph_grads[dtype]
    _fused_rule(gs, g0, g1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dirty_stage_workspaces(tiny_case, dtype):
    c = tiny_case
    l0, g0 = _staged_step(_net(c, dtype), c)
    l1, g1 = _staged_step(_net(c, dtype), c)
    net = _net(c, dtype)
    _staged_step(net, c)
    for stage in ("enc", "dec"):
        net._slots[stage].buf.view(torch.int16).fill_(0x7FC0)  # bf16 NaN bytes (both stage buffers exist after a staged step)
    net.zero_grad()
    ls, gs = _staged_step(net, c)
    assert torch.equal(ls, l0)
    _fused_rule(gs, g0, g1)


def test_stage_call_under_ddp_raises(tiny_case, tmp_path):
    import torch.distributed as dist
    from olmoasr_amd import _native as N
    from olmoasr_amd import ddp
    c = tiny_case
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", init_method=f"file://{tmp_path}/rdzv", rank=0, world_size=1, device_id=torch.device(DEV, 0))
    try:
        model = ddp.DistributedDataParallel(_net(c, "float32"), device_ids=[0])
        with pytest.raises(N.NativeError, match=r"model\(mel, tokens, mask\)"):
            model.module.encoder(c["mel"].to(DEV))
        with torch.no_grad():  # no graph: the inference forward is fine
            model.module.encoder(c["mel"].to(DEV))
    finally:
        if created:
            dist.destroy_process_group()
