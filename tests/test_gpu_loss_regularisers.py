"""Label smoothing and z-loss in the fused cross-entropy (csrc/loss.hip ce_kernel<true>, csrc/fp32ref.hip ce_f32_kernel<true>; DESIGN.md
section 3j).  For a valid row with logits x over V classes, lse = logsumexp(x), p = softmax(x):

    row_loss  = lse - (1 - eps) x_t - eps / V sum_{c<V} x_c + z lse^2
    dlogits_c = g [(1 + 2 z lse) p_c - (1 - eps) [c == t] - eps / V]           g = gscale / n_valid

1. the operator against float64, 2. zero coefficients are the plain kernel bit for bit, 3. the fused step against torch.autograd over
F.cross_entropy(label_smoothing=) + z mean(lse^2), 4. the span step against the plain step, 5. the loss parts through the step."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
PAD = 51864
REG = [(0.1, 0.0), (0.0, 1e-2), (0.1, 1e-2)]
GSCALE = 1024.0  # with z = 1e-2 (2 z lse ~ 0.3): g eps / V and the z factor sit far above any absolute tolerance


def _dims(mo_dims):
    from olmoasr_amd.config.model_dims import ModelDimensions
    return ModelDimensions(**{k: getattr(mo_dims, k) for k in ModelDimensions.__dataclass_fields__})


def _mask(tl):
    m = torch.zeros(tl.numel(), 448, 448)
    for b, n in enumerate(tl.tolist()):
        m[b, :, n:] = -float("inf")
    return m


# ---- 1. the operator, bf16, against float64 --------------------------------------------------------------------------------------------
_OP_CASES = {}


def _op_case(V, ld):
    """64 rows of randn * 2.5 plus a per-row offset in [-6, 6] (sum_c x_c is far from 0: a wrong eps / V sum x term cannot hide), the padded
    columns filled with 7.0, every 5th row ignored, one target at V - 2 (inside a chunk that straddles V), one at 0.  Built once per shape;
    the float64 statistics are shared by every (eps, z)."""
    if (V, ld) not in _OP_CASES:
        rows, ignore = 64, V - 1
        g = torch.Generator().manual_seed(5)
        logits = torch.full((rows, ld), 7.0, dtype=BF)
        off = torch.rand(rows, 1, generator=g) * 12 - 6
        logits[:, :V] = (torch.randn(rows, V, generator=g) * 2.5 + off).to(BF)
        tgt = torch.randint(1, V - 2, (rows,), generator=g)
        tgt[::5] = ignore
        tgt[1] = V - 2
        tgt[2] = 0
        valid = tgt != ignore
        x = logits[:, :V].double()
        lse = torch.logsumexp(x, -1)
        onehot = torch.zeros_like(x)
        onehot[valid, tgt[valid]] = 1.0
        _OP_CASES[(V, ld)] = dict(logits=logits, tgt=tgt, ignore=ignore, valid=valid, n=int(valid.sum()), x=x, lse=lse, p=torch.exp(x - lse[:, None]),
                                  onehot=onehot, xt=(x * onehot).sum(-1), xsum=x.sum(-1))
    return _OP_CASES[(V, ld)]


def _want(c, V, eps, z):
    row = c["lse"] - (1 - eps) * c["xt"] - eps / V * c["xsum"] + z * c["lse"] ** 2
    row = torch.where(c["valid"], row, torch.zeros_like(row))
    g = GSCALE / c["n"]
    grad = g * ((1 + 2 * z * c["lse"][:, None]) * c["p"] - (1 - eps) * c["onehot"] - eps / V)
    grad[~c["valid"]] = 0.0
    return row, float(row.sum() / c["n"]), grad, g


@pytest.mark.parametrize("eps,z", REG)
@pytest.mark.parametrize("V,ld", [(51865, 51968), (1000, 1024)])  # the model's head; fewer chunks (128) than threads (1024)
def test_op_against_float64(V, ld, eps, z):
    from olmoasr_amd import ops
    c = _op_case(V, ld)
    row_w, loss_w, grad_w, g = _want(c, V, eps, z)
    lg = c["logits"].to(DEV)
    loss, row_loss, parts = ops.cross_entropy_(lg, V, c["tgt"].to(DEV), c["ignore"], gscale=GSCALE, label_smoothing=eps, z_loss=z, return_parts=True)
    torch.cuda.synchronize()
    assert abs(float(loss) - loss_w) <= 1e-4 * abs(loss_w), (float(loss), loss_w)
    row_err = (row_loss.cpu().double() - row_w).abs()
    assert bool((row_err <= 1e-4 * row_w.abs()).all()), float((row_err / row_w.abs().clamp_min(1e-30)).max())
    # every stored gradient within one bf16 ulp of the float64 value (test_cross_entropy_gradient_is_the_fp32_gradient_rounded_once's
    # criterion) plus 2^-17 g (p_c + eps / V): p_c - eps / V cancels where p_c ~ eps / V, and the fp32 exponent x log2(e) for
    # |x - max| <= 32 carries up to ~2^-18.5 relative error on p_c; the slack doubles that.  The same formula in float32 torch, rounded to
    # bf16, stays inside this bound against float64 on these inputs: its worst excess over one ulp is 0.0084 of the slack (V = 51865,
    # eps = 0.1, z = 1e-2), so the bound is used as stated.
    got = lg[:, :V].float().cpu().double()
    ulp = torch.where(grad_w == 0, torch.zeros_like(grad_w), torch.exp2(torch.floor(torch.log2(grad_w.abs().clamp_min(1e-300))) - 7))
    bound = ulp * 1.0001 + 2.0 ** -17 * g * (c["p"] + eps / V) + 1e-300
    err = (got - grad_w).abs()
    worst = float(((err - ulp * 1.0001) / (bound - ulp * 1.0001))[c["valid"]].max())
    print(f"   V={V} eps={eps} z={z}: loss {float(loss):.6f} vs {loss_w:.6f}; worst gradient excess over one ulp = {worst:.3g} of the slack")
    assert bool((err <= bound)[c["valid"]].all()), worst
    # the padded columns (the tied-head GEMM reads them) and the ignored rows are bit-zero
    assert not bool(lg[:, V:].view(torch.int16).any()) and not bool(lg[~c["valid"].to(DEV)].view(torch.int16).any())
    # the parts: the plain NLL is the eps = z = 0 row loss of the same input, lse^2 is float64's
    lg0 = c["logits"].to(DEV)
    _, row0 = ops.cross_entropy_(lg0, V, c["tgt"].to(DEV), c["ignore"], gscale=GSCALE)
    assert parts.shape == (2, 64)
    assert bool(((parts[0] - row0).abs() <= 1e-6 * row0.abs()).all())
    lse2 = torch.where(c["valid"], c["lse"] ** 2, torch.zeros_like(c["lse"]))
    assert bool(((parts[1].cpu().double() - lse2).abs() <= 1e-5 * lse2).all())


# ---- 2. off means off ----------------------------------------------------------------------------------------------------------------------
def test_zero_coefficients_are_the_plain_operator():
    from olmoasr_amd import _native as N
    c = _op_case(51865, 51968)
    V, rows, tgt = 51865, 64, c["tgt"].to(DEV)
    out = []
    for ex in (False, True):
        lg = c["logits"].to(DEV)
        nv = torch.zeros(1, device=DEV, dtype=torch.int32)
        row_loss = torch.empty(rows, device=DEV)
        loss = torch.zeros(1, device=DEV)
        head = (N.ptr(lg), lg.stride(0), V, N.ptr(tgt), rows, c["ignore"], GSCALE, N.ptr(nv), N.ptr(row_loss), N.ptr(loss), 1)
        if ex:
            N.check(N.lib().oasr_cross_entropy_ex(*head, 0.0, 0.0, None, N.stream_ptr()), "oasr_cross_entropy_ex")
        else:
            N.check(N.lib().oasr_cross_entropy(*head, N.stream_ptr()), "oasr_cross_entropy")
        torch.cuda.synchronize()
        out.append((loss, row_loss, lg))
    for a, b in zip(*out):
        assert torch.equal(a.view(torch.int16) if a.dtype == BF else a, b.view(torch.int16) if b.dtype == BF else b)


def _tiny_net(c, dtype):
    from olmoasr_amd.model import OLMoASR
    net = OLMoASR(_dims(c["dims"]), device=DEV, seed=0, compute_dtype=dtype)
    net.load_state_dict(c["sd"])
    return net


def _tiny_args(c):
    return c["mel"].to(DEV), c["tokens"].to(DEV), c["targets"].to(DEV), c["text_len"].to(DEV)


def test_zero_coefficients_are_the_plain_step(tiny_case):
    """loss_and_backward(label_smoothing=0.0, z_loss=0.0) is the call without the keywords: same launches on the same buffers.  The loss (a
    deterministic reduction) must be torch.equal.  The gradients cannot be held to torch.equal: the plain step does not repeat them bit for
    bit -- the conv stem's and the split-K weight gradients, the embedding scatter and the LayerNorm bias sums are fp32 atomic adds whose
    order changes from run to run (measured here: of three identical plain-keyword-plain runs, encoder.conv1.weight differed in one session
    and decoder.blocks.0.attn_ln.bias in another, each time between runs that launch the same kernels).  So the call without the keywords
    runs twice and every gradient tensor is held to test_gpu_stage_autograd.py's _fused_rule: bit-identical where the step repeats
    bit-identically, else within 4 x the spread of the plain step's own two runs (floor: 2^-16 of the tensor's largest entry)."""
    net = _tiny_net(tiny_case, "bfloat16")
    args = _tiny_args(tiny_case)
    res = []
    for kw in ({}, dict(label_smoothing=0.0, z_loss=0.0), {}):
        net.zero_grad()
        loss, _ = net.loss_and_backward(*args, loss_scale=1024.0, **kw)
        torch.cuda.synchronize()
        res.append((loss.clone(), {n: p.grad.clone() for n, p in net.named_parameters()}))
    (l0, g0), (lk, gk), (l1, g1) = res
    assert torch.equal(l0, lk) and torch.equal(l0, l1)
    same = sum(torch.equal(gk[n], g0[n]) for n in g0)
    print(f"   {same} of {len(g0)} gradient tensors torch.equal with the zero keywords; the two plain runs agree on {sum(torch.equal(g1[n], g0[n]) for n in g0)}")
    for n in g0:
        diff = float((gk[n] - g0[n]).abs().max())
        spread = float((g1[n] - g0[n]).abs().max())
        floor = float(g0[n].abs().max()) * 2.0 ** -16
        assert diff <= max(4 * spread, floor), (n, diff, spread, floor)


# ---- 3. the fused step against the autograd bridge ---------------------------------------------------------------------------------------
def _bridge_loss(net, c, eps, z):
    logits = net(c["mel"].to(DEV), c["tokens"].to(DEV), _mask(c["text_len"]).to(DEV))
    lg, tg = logits.view(-1, logits.shape[-1]), c["targets"].to(DEV).view(-1)
    valid = tg != PAD
    return F.cross_entropy(lg, tg, ignore_index=PAD, label_smoothing=eps) + z * (torch.logsumexp(lg[valid], -1) ** 2).mean()


@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
def test_step_against_the_autograd_bridge(tiny_case, dtype):
    eps, z = 0.1, 1e-3
    c = tiny_case
    net = _tiny_net(c, dtype)
    net.zero_grad()
    loss_f, _ = net.loss_and_backward(*_tiny_args(c), loss_scale=1024.0, label_smoothing=eps, z_loss=z)
    fused = {n: p.grad.clone() for n, p in net.named_parameters()}
    plain, _ = net.loss_and_backward(*_tiny_args(c), loss_scale=1024.0)
    assert abs(float(loss_f) - float(plain)) > 1e-2 * abs(float(plain))  # (the regularisers are in the objective at all)
    net.zero_grad()
    loss = _bridge_loss(net, c, eps, z)
    (loss * 1024.0).backward()
    assert abs(float(loss.detach()) - float(loss_f)) < 1e-4 * abs(float(loss_f)), (float(loss), float(loss_f))
    tol = 2e-5 if dtype == "float32" else 9e-3  # test_autograd_backward_equals_the_fused_step's bounds
    worst = max((float((p.grad - fused[n]).norm() / (fused[n].norm() + 1e-20)), n) for n, p in net.named_parameters())
    print(f"   [{dtype}] regularised step vs autograd: loss {float(loss_f):.6f} vs {float(loss.detach()):.6f}, worst per-tensor rel-L2 {worst[0]:.3g} {worst[1]}")
    assert worst[0] < tol, worst


# ---- 4. the span step equals the plain step ------------------------------------------------------------------------------------------------
def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
def test_span_step_equals_plain_step_with_regularisers(dtype):
    from olmoasr_amd import ops
    from olmoasr_amd.config.model_dims import VARIANT_TO_DIMS
    from olmoasr_amd.model import OLMoASR
    from olmoasr_amd.synth import synth_samples
    eps, z = 0.1, 1e-3
    B = 6
    net = OLMoASR(VARIANT_TO_DIMS["tiny"], device=DEV, seed=0, compute_dtype=dtype)
    pcm, ti, ty, tl = synth_samples(list(range(70, 70 + B)), DEV)
    mel = ops.log_mel(pcm)
    kw = dict(loss_scale=1024.0, label_smoothing=eps, z_loss=z)
    tol_l, tol_g, tol_t = 1e-6, 1e-5, 1e-4  # test_span_step_equals_plain_step's bounds

    def compare(tag, loss1, loss0, f0, g0):
        worst = max((_rel(p.grad, g0[n]), n) for n, p in net.named_parameters() if p.grad is not None and n in g0)
        total = _rel(net.flat_grads, f0)
        print(f"   {tag} ({dtype}): loss {float(loss1):.6f} vs {float(loss0):.6f}, grads rel-L2 {total:.2e}, worst tensor {worst[0]:.2e} {worst[1]}")
        assert abs(float(loss1) - float(loss0)) <= tol_l * abs(float(loss0)), (tag, float(loss1), float(loss0))
        assert total <= tol_g and worst[0] <= tol_t, (tag, total, worst)

    net.zero_grad()
    loss0, _ = net.loss_and_backward(mel, ti, ty, tl, **kw)
    torch.cuda.synchronize()
    g0, f0 = {n: p.grad.clone() for n, p in net.named_parameters()}, net.flat_grads.clone()
    preds = {}
    for span_forward in (False, True):
        for reg in (True, False):  # reg = False: only for the predictions of the eps = z = 0 step
            net.zero_grad()
            pred = torch.full((B, 448), -7, dtype=torch.int32, device=DEV)
            loss1, _ = net.loss_and_backward(mel, ti, ty, tl, span=True, span_forward=span_forward, pred_out=pred,
                                             **(kw if reg else dict(loss_scale=1024.0)))
            torch.cuda.synchronize()
            preds[reg] = pred
            if reg:
                compare(f"span step, span_forward={span_forward}", loss1, loss0, f0, g0)
        assert torch.equal(preds[True], preds[False])  # the regularisers do not touch the predictions
    # once from given encoder features (the decoder alone; the encoder is frozen and its gradient ranges stay zero on both sides)
    net.encoder.requires_grad_(False)
    xa = net.encoder(mel.clone().requires_grad_(True)).detach()
    net.zero_grad()
    loss0, _ = net.loss_and_backward(None, ti, ty, tl, audio_features=xa, **kw)
    torch.cuda.synchronize()
    g0 = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    f0 = net.flat_grads.clone()
    net.zero_grad()
    loss1, _ = net.loss_and_backward(None, ti, ty, tl, audio_features=xa, span=True, **kw)
    torch.cuda.synchronize()
    compare("span step from audio_features", loss1, loss0, f0, g0)


# ---- 5. the loss parts through the step ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("span", [None, True])
def test_loss_parts_through_the_step(tiny_case, span):
    eps, z = 0.1, 1e-3
    c = tiny_case
    net = _tiny_net(c, "bfloat16")
    args = _tiny_args(c)
    net.zero_grad()
    plain, logits = net.loss_and_backward(*args, return_logits=True)
    parts = torch.full((2,), 123.0, device=DEV)
    loss, _ = net.loss_and_backward(*args, span=span, label_smoothing=eps, z_loss=z, loss_parts_out=parts)
    torch.cuda.synchronize()
    assert abs(float(parts[0]) - float(plain)) <= 1e-6 * abs(float(plain)), (float(parts[0]), float(plain))
    # loss - (1 - eps) nll - z lse^2 = eps mean_valid(lse - mean_c x), from the plain step's own fp32 logits
    lg, tg = logits.view(-1, logits.shape[-1]).double(), c["targets"].to(DEV).view(-1)
    lg = lg[tg != PAD]
    lse = torch.logsumexp(lg, -1)
    want = eps * float((lse - lg.mean(-1)).mean())
    got = float(loss) - (1 - eps) * float(parts[0]) - z * float(parts[1])
    assert abs(got - want) <= 1e-4 * abs(float(loss)), (got, want, float(loss))
    assert abs(float(parts[1]) - float((lse ** 2).mean())) <= 1e-4 * float(parts[1])
    # accumulate_loss: two micro-steps of a window of two add up to the one-step values
    loss2 = torch.zeros(1, device=DEV)
    parts2 = torch.zeros(2, device=DEV)
    for i in range(2):
        net.loss_and_backward(*args, span=span, label_smoothing=eps, z_loss=z, accumulation_steps=2, loss_out=loss2, accumulate_loss=i > 0,
                              loss_parts_out=parts2)
    torch.cuda.synchronize()
    assert abs(float(loss2) - float(loss)) <= 1e-6 * abs(float(loss))
    assert bool(((parts2 - parts).abs() <= 1e-6 * parts.abs()).all()), (parts2.tolist(), parts.tolist())


# ---- 6. the training script ---------------------------------------------------------------------------------------------------------------
def test_train_script_flags(tmp_path, capsys):
    """train_timestamps.py --label_smoothing / --z_loss: the first step of a run with them starts from the weights of a run without, so
    its train_nll is that run's train_loss; the record carries both parts, the default run's record carries neither."""
    import importlib.util
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("tt_gpu_reg", os.path.join(root, "scripts", "training", "train_timestamps.py"))
    tt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tt)
    common = ["--model_variant=tiny", "--eff_batch_size=4", "--train_batch_size=2", "--lr=1e-3", "--train_log_freq=1", "--n_synthetic=4",
              f"--ckpt_dir={tmp_path}", f"--run_id_dir={tmp_path}/run_ids", "--ckpt_file_name=None", "--ckpt_freq=0", "--train_steps=1"]
    eps, z = 0.1, 1e-3
    plain = tt.main(common + ["--exp_name=p"])
    capsys.readouterr()
    reg = tt.main(common + ["--exp_name=r", f"--label_smoothing={eps}", f"--z_loss={z}"])
    events = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert {"event": "loss_regularisers", "label_smoothing": eps, "z_loss": z} in events
    assert len(plain) == 1 and len(reg) == 1
    assert "train_nll" not in plain[0] and "train_lse_sq" not in plain[0]
    r = reg[0]
    assert abs(r["train_nll"] - plain[0]["train_loss"]) <= 1e-6 * plain[0]["train_loss"], (r, plain[0])
    assert 100.0 < r["train_lse_sq"] < 200.0  # lse ~ log(51865) + a little = 11 .. 14 at initialisation
    # loss = (1 - eps) nll + z lse^2 + eps mean(lse - mean_c x), and the last term is positive (lse >= max x >= mean x)
    rest = r["train_loss"] - (1 - eps) * r["train_nll"] - z * r["train_lse_sq"]
    assert 0.0 < rest < eps * 2 * r["train_nll"], (rest, r)
