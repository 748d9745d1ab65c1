"""Frozen-parameter fine-tuning (``requires_grad_(False)``, e.g. Whisper's frozen-encoder recipe): a frozen parameter gets no gradient
(``.grad is None``), the optimizer leaves it alone, the clip norm covers the trainable gradients only, and the backward does not run the
work that only served frozen tensors (oasr_set_trainable, the pruned backward of csrc/engine_bwd.h).  Every check runs in the fp32
validation mode against the fp32 oracle (the bounds of test_gpu_fp32_mode.py) and on the bf16 engine (the bounds of test_gpu_model.py)."""
import ctypes
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


def _net(c, dtype):
    from olmoasr_amd.model import OLMoASR
    net = OLMoASR(_dims(c["dims"]), device=DEV, seed=0, compute_dtype=dtype)
    net.load_state_dict(c["sd"])
    return net


def _args(c):
    return c["mel"].to(DEV), c["tokens"].to(DEV), c["targets"].to(DEV), c["text_len"].to(DEV)


def _mask(tl):
    m = torch.zeros(tl.numel(), 448, 448)
    for b, n in enumerate(tl.tolist()):
        m[b, :, n:] = -float("inf")
    return m


@pytest.fixture(scope="module")
def oracle(tiny_case):
    """fp32 oracle gradients of the WHOLE model, and the gradients of its bf16 mirror (the envelope of a bf16 evaluation)."""
    from oracle import model_oracle as mo
    c = tiny_case
    torch.set_num_threads(min(32, len(os.sched_getaffinity(0))))
    loss, grads, _ = mo.loss_and_grads(c["sd"], c["dims"], c["mel"], c["tokens"], c["targets"], c["text_len"])
    _, gb, _ = mo.loss_and_grads(c["sd"], c["dims"], c["mel"], c["tokens"], c["targets"], c["text_len"], autocast_bf16=True)
    return dict(loss=float(loss), grads=grads, bf16=gb)


def _check_trainable_grads(net, oracle, dtype, frozen):
    """Frozen parameters have no gradient; every trainable one matches the oracle's full-model gradient of that tensor (freezing
    changes no other tensor's gradient).  fp32: rel-L2 <= 1e-3 per tensor.  bf16: <= max(2 x the bf16 mirror's error, 3 %) per
    tensor, cosine > 0.999, <= 2 % over the trainable gradient."""
    num = den = 0.0
    n_tr = 0
    for name, p in net.named_parameters():
        if frozen(name):
            assert not p.requires_grad and p.grad is None, name
            continue
        n_tr += 1
        gn = p.grad.detach().float().cpu()
        gr = oracle["grads"][name]
        rel = float((gn - gr).norm() / (gr.norm() + 1e-12))
        if dtype == "float32":
            assert rel <= 1e-3, (name, rel)
        else:
            env = float((oracle["bf16"][name].float() - gr).norm() / (gr.norm() + 1e-12))
            cos = float((gn * gr).sum() / (gn.norm() * gr.norm() + 1e-20))
            assert rel <= max(2.0 * env, 0.03) and cos > 0.999, (name, rel, env, cos)
        num += float((gn - gr).double().pow(2).sum())
        den += float(gr.double().pow(2).sum())
    assert n_tr > 0
    if dtype != "float32":
        assert (num / den) ** 0.5 <= 0.02


def _freeze(net, frozen):
    for name, p in net.named_parameters():
        p.requires_grad_(not frozen(name))


def _enc(name):
    return name.startswith("encoder.")


@pytest.mark.parametrize("dtype", DTYPES)
def test_autograd_encoder_frozen(tiny_case, oracle, dtype):
    """The reference-style loop: model.encoder.requires_grad_(False); loss.backward() -> encoder grads None, the rest = the oracle's."""
    c = tiny_case
    net = _net(c, dtype)
    net.encoder.requires_grad_(False)
    logits = net(c["mel"].to(DEV), c["tokens"].to(DEV), _mask(c["text_len"]).to(DEV))
    loss = F.cross_entropy(logits.view(-1, logits.shape[-1]), c["targets"].to(DEV).view(-1), ignore_index=PAD)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss.detach()) - oracle["loss"]) < (1e-4 if dtype == "float32" else 2e-2)
    _check_trainable_grads(net, oracle, dtype, _enc)
    # torch's own AdamW over model.parameters() skips the None-grad parameters
    before = {n: p.detach().clone() for n, p in net.named_parameters() if _enc(n)}
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=0.1)
    torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
    opt.step()
    assert all(torch.equal(p, before[n]) for n, p in net.named_parameters() if _enc(n))


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_step_encoder_frozen(tiny_case, dtype):
    """loss_and_backward + optim_step with the encoder frozen: encoder masters and their bf16 compute copies are bit-identical after the
    step; every trainable weight is the oracle's clip + AdamW over the trainable subset (norm over that subset only)."""
    from oracle import model_oracle as mo
    c = tiny_case
    net = _net(c, dtype)
    net.encoder.requires_grad_(False)
    net.init_optimizer_state()
    for t in net._opt_state:
        t.zero_()
    scale = 1024.0
    net.zero_grad()
    net.loss_and_backward(*_args(c), loss_scale=scale)
    names = [n for n, p in net.named_parameters() if p.requires_grad]
    assert names and not any(_enc(n) for n in names)
    grads = {n: p.grad.detach().cpu() / scale for n, p in net.named_parameters() if p.requires_grad}
    params = {n: c["sd"][n].clone() for n in names}
    total, coef = mo.clip_coef(grads, 1.0)
    for n in names:
        grads[n] = grads[n] * coef
    m = {n: torch.zeros_like(params[n]) for n in names}
    v = {n: torch.zeros_like(params[n]) for n in names}
    mo.adamw_step(params, grads, m, v, step=1, lr=1.5e-3)
    numel = net.flat_params.numel()
    shadow_before = net._shadow[:2 * numel].clone() if dtype == "bfloat16" else None
    stats = net.optim_step(step=1, lr=1.5e-3, inv_loss_scale=1.0 / scale)
    torch.cuda.synchronize()
    assert float(stats[1]) == 0.0
    assert abs(float(stats[0].sqrt()) / scale - float(total)) / float(total) < 1e-4
    for n, p in net.named_parameters():
        if _enc(n):
            assert torch.equal(p.detach().cpu(), c["sd"][n]), n
        else:
            diff = float((p.detach().cpu() - params[n]).abs().max())
            assert diff < 2e-6, (n, diff)
    m_nat, v_nat = net._opt_state
    for n, off, k, _ in net._param_slices():
        if _enc(n):
            assert not m_nat[off:off + k].any() and not v_nat[off:off + k].any(), n
    if dtype == "bfloat16":  # the bf16 compute copy of the encoder is untouched by the step
        sh_after = net._shadow[:2 * numel].view(torch.bfloat16)
        sh_before = shadow_before.view(torch.bfloat16)
        for n, off, k, _ in net._param_slices():
            if _enc(n):
                assert torch.equal(sh_after[off:off + k], sh_before[off:off + k]), n
    # and through forward: the stepped model computes what a fresh model loaded with its weights computes
    fresh = _net(c, dtype)
    fresh.load_state_dict({k: t.detach().clone() for k, t in net.state_dict().items()})
    with torch.no_grad():
        a = net.eval()(c["mel"].to(DEV), c["tokens"].to(DEV), c["text_len"].to(DEV).to(torch.int32))
        b = fresh.eval()(c["mel"].to(DEV), c["tokens"].to(DEV), c["text_len"].to(DEV).to(torch.int32))
    assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_mixed_masks(tiny_case, oracle, dtype):
    """(a) token embedding frozen: the tied-logits weight gradient and the embedding scatter are skipped, everything else is the oracle's.
    (b) decoder blocks 0..1 frozen, encoder trainable: the data gradient still flows through the frozen blocks into d(xa), so every
    encoder gradient equals the oracle's."""
    c = tiny_case
    cases = [lambda n: n == "decoder.token_embedding.weight",
             lambda n: n.startswith("decoder.blocks.0.") or n.startswith("decoder.blocks.1.")]
    for frozen in cases:
        net = _net(c, dtype)
        _freeze(net, frozen)
        net.zero_grad()
        loss, _ = net.loss_and_backward(*_args(c))
        torch.cuda.synchronize()
        assert abs(float(loss) - oracle["loss"]) < (1e-4 if dtype == "float32" else 2e-2)
        _check_trainable_grads(net, oracle, dtype, frozen)
        del net


def _gemm_flops(net, c):
    from olmoasr_amd import _native as N
    lib = N.lib()
    torch.cuda.synchronize()
    lib.oasr_profile_gemm(1)
    net.zero_grad()
    net.loss_and_backward(*_args(c))
    torch.cuda.synchronize()
    ms, fl, cnt = (ctypes.c_double * 4)(), (ctypes.c_double * 4)(), (ctypes.c_int64 * 4)()
    N.check(lib.oasr_profile_gemm_collect(ms, fl, cnt, None, 0), "profile_collect")
    lib.oasr_profile_gemm(0)
    return sum(fl), sum(cnt)


def test_frozen_encoder_skips_its_backward(tiny_case):
    """Executed GEMM FLOPs (oasr_profile_gemm_collect) drop by at least 95 % of the encoder backward's GEMMs plus the d(xa) GEMMs of the
    cross-attention, both counted from the dims."""
    c = tiny_case
    dm = c["dims"]
    net = _net(c, "bfloat16")
    f_all, n_all = _gemm_flops(net, c)
    net.encoder.requires_grad_(False)
    f_frz, n_frz = _gemm_flops(net, c)
    B, d = c["tokens"].shape[0], dm.n_audio_state
    Me = B * dm.n_audio_ctx
    enc_blocks = dm.n_audio_layer * 2 * 2 * Me * d * d * (3 + 1 + 4 + 4)  # wgrad + dgrad of q|k|v, out, mlp.0, mlp.2
    conv2 = 2 * 2 * Me * d * 3 * d                                           # conv2 wgrad + dgrad
    dxa = dm.n_text_layer * 2 * Me * 2 * d * d                               # d(xa) = d(k|v) . W_kv per decoder layer
    expect = enc_blocks + conv2 + dxa
    print(f"GEMM flops all-trainable {f_all:.4g} ({n_all} launches), encoder frozen {f_frz:.4g} ({n_frz}); dropped {f_all - f_frz:.4g}, "
          f"expected >= {expect:.4g}")
    assert f_all - f_frz >= 0.95 * expect


@pytest.mark.parametrize("dtype", DTYPES)
def test_toggled_mask_is_the_default_step(tiny_case, dtype):
    """Freeze (and run a step that way), unfreeze: gradients and optimizer step are those of a model that was never toggled."""
    c = tiny_case

    def step(net):
        net.init_optimizer_state()
        for t in net._opt_state:
            t.zero_()
        net.zero_grad()
        net.loss_and_backward(*_args(c), span=True)
        g = net.flat_grads.clone()
        net.optim_step(step=1, lr=1e-3)
        torch.cuda.synchronize()
        return g, net.flat_params.clone()

    g0, p0 = step(_net(c, dtype))
    g1, p1 = step(_net(c, dtype))
    net = _net(c, dtype)
    net.encoder.requires_grad_(False)
    net.zero_grad()
    net.loss_and_backward(*_args(c), span=True)
    net.encoder.requires_grad_(True)
    g2, p2 = step(net)
    assert all(p.grad is not None for p in net.parameters())
    # the never-toggled step twice gives the run-to-run spread (fp32 atomics of split-K weight gradients may reorder sums): the
    # toggled model must be as close to it as it is to itself -- bit-identical wherever the step is deterministic
    if torch.equal(g0, g1) and torch.equal(p0, p1):
        assert torch.equal(g2, g0) and torch.equal(p2, p0)
    else:
        assert float((g2 - g0).abs().max()) <= 4 * float((g1 - g0).abs().max())
        assert float((p2 - p0).abs().max()) <= 4 * float((p1 - p0).abs().max())


def test_all_frozen_is_an_error(tiny_case):
    from olmoasr_amd import _native as N
    c = tiny_case
    net = _net(c, "bfloat16")
    net.requires_grad_(False)
    with pytest.raises(N.NativeError):
        net.loss_and_backward(*_args(c))


def test_train_script_freeze_encoder(tmp_path):
    """train_timestamps.py --freeze_encoder True: a few steps; the checkpoint's encoder tensors are the initial ones, bit for bit, the
    decoder moved, and the loss is finite."""
    import importlib.util
    from olmoasr_amd.config.model_dims import VARIANT_TO_DIMS
    from olmoasr_amd.model import OLMoASR
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("tt_gpu_freeze", os.path.join(root, "scripts", "training", "train_timestamps.py"))
    tt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tt)
    log = tt.main(["--model_variant=tiny", "--eff_batch_size=4", "--train_batch_size=2", "--train_steps=4", "--lr=1e-3",
                   "--train_log_freq=1", "--n_synthetic=4", "--ckpt_freq=4", f"--ckpt_dir={tmp_path}", f"--run_id_dir={tmp_path}/run_ids",
                   "--exp_name=f", "--ckpt_file_name=None", "--freeze_encoder", "True"])
    assert len(log) == 4 and all(torch.isfinite(torch.tensor(float(r["train_loss"]))) for r in log)
    run_id = open(tmp_path / "run_ids" / "f.txt").read().strip()
    rdir = tmp_path / f"f_{run_id}"
    ck = torch.load(rdir / sorted(os.listdir(rdir))[0], weights_only=False)
    sd = {k[len("module."):]: v for k, v in ck["model_state_dict"].items()}
    init = OLMoASR(VARIANT_TO_DIMS["tiny"], device=DEV, seed=0).state_dict()
    enc = [k for k in sd if k.startswith("encoder.") and k != "encoder.positional_embedding"]
    assert enc and all(torch.equal(sd[k].cpu(), init[k].cpu()) for k in enc)
    assert not torch.equal(sd["decoder.ln.weight"].cpu(), init["decoder.ln.weight"].cpu())
