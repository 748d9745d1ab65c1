"""The fused unscale + clip + AdamW step on planted arenas: parameters, gradients and BOTH moments are written directly, the moments
non-zero, v >= 0 and independent of the gradients.  (One step from zero moments moves every parameter by lr * g / (|g| + eps): the
gradient's scale cancels, and with it a wrong clip coefficient, inv_scale or gmul.)  Covers oasr_optim_step, the ZeRO-1 range entries
(oasr_grad_sumsq_range / oasr_optim_step_range) and the run-table kernels of a partly frozen model, on a one-layer width-64 model
(205,504 parameters in 49 tensors: the float64 reference of a step takes milliseconds).

Reference: float64 unscale + clip_grad_norm_ + AdamW from the hyperparameters as the fp32 values the C ABI receives, restarted from the
device's fp32 state at every step.  Errors are counted in units of what fp32 must round, e = 2^-24:
    m: e (b1 |m0| + (1 - b1) |g|)      v: e (b2 v0 + (1 - b2) g^2)      p: e (|p0| + |update|)      (g: unscaled, clipped)
Budget: torch's own fp32 path on the CPU (clip_grad_norm_ + torch.optim.AdamW(foreach=False)) on the same plants against the same
reference, worst over all regimes and steps; the kernel may use no more (margin 1 x: it accumulates the norm in double).

Measured (worst units m / v / p over the four regimes x three steps; printed by test_regimes_within_the_torch_fp32_budget):
    torch fp32 on the CPU   100.92 / 199.27 / 146.15   (the log-uniform regime: the fp32 norm and clip coefficient)
    the kernel (MI355X)       2.83 /   5.24 /   4.67
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
E = 2.0 ** -24
SCALE = 65536.0


def f32(x):
    return float(torch.tensor(x, dtype=F32))


HYPER = dict(lr=f32(1e-3), betas=(f32(0.9), f32(0.98)), eps=f32(1e-6), weight_decay=f32(0.1), max_grad_norm=1.0, inv_loss_scale=1.0 / SCALE)


@pytest.fixture(scope="module")
def net():
    from olmoasr_amd.config.model_dims import ModelDimensions
    from olmoasr_amd.model import OLMoASR
    m = OLMoASR(ModelDimensions(80, 1500, 64, 1, 1, 503, 448, 64, 1, 1), device=DEV, seed=0)
    m.init_optimizer_state()
    m.flat_grads  # the gradient arena
    return m


def plants(n, regime, seed=0):
    """CPU fp32 (p, scaled g, m, v): moments independent of the gradients, v > 0."""
    g = torch.Generator().manual_seed(seed)
    p = 0.05 * torch.randn(n, generator=g)
    m = 0.01 * torch.randn(n, generator=g)
    v = (0.01 * torch.randn(n, generator=g)) ** 2 + 1e-8
    if regime == "clipped":          # norm = 0.05 sqrt(n) = 22.7 >> max_norm
        gu = 0.05 * torch.randn(n, generator=g)
    elif regime == "unclipped":      # norm = 0.045: the coefficient clamps to exactly 1
        gu = 1e-4 * torch.randn(n, generator=g)
    elif regime == "zero":           # coef = min(1, max_norm / 1e-6) = 1
        gu = torch.zeros(n)
    else:                            # log-uniform magnitudes over 1e-6 .. 10
        gu = 10.0 ** (torch.rand(n, generator=g) * 7.0 - 6.0) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)
    return p.to(F32), (gu.to(F32) * SCALE), m.to(F32), v.to(F32)


def plant(net, p, g, m, v):
    net.flat_params.copy_(p)
    net.flat_grads.copy_(g)
    net._opt_state[0].copy_(m)
    net._opt_state[1].copy_(v)
    net.refresh_shadow()


def state(net):
    torch.cuda.synchronize()
    n = net.flat_params.numel()
    return dict(p=net.flat_params.detach().cpu().clone(), m=net._opt_state[0].cpu().clone(), v=net._opt_state[1].cpu().clone(),
                sh=net._shadow[: 2 * n].cpu().clone().view(torch.int16), g=net.flat_grads.cpu().clone())


def same(a, b, keys=("p", "m", "v", "sh"), sel=None):
    for k in keys:
        x, y = (a[k], b[k]) if sel is None else (a[k][sel], b[k][sel])
        xi, yi = (x, y) if x.dtype == torch.int16 else (x.view(torch.int32), y.view(torch.int32))
        if not torch.equal(xi, yi):
            i = int((xi != yi).nonzero()[0])
            return f"{k} differs at {i} ({int((xi != yi).sum())} elements): {x[i].item()!r} vs {y[i].item()!r}"
    return None


def reference(p0, g_scaled, m0, v0, step, live=None):
    """float64 unscale + clip_grad_norm_ + AdamW (decoupled decay).  live: bool mask of the trainable elements (norm and update)."""
    lr, (b1, b2), eps, wd = HYPER["lr"], HYPER["betas"], HYPER["eps"], HYPER["weight_decay"]
    gu = g_scaled.to(F64) * HYPER["inv_loss_scale"]
    if live is not None:
        gu = torch.where(live, gu, torch.zeros((), dtype=F64))
    sumsq_scaled = float((gu / HYPER["inv_loss_scale"]).pow(2).sum())
    norm = float(gu.pow(2).sum().sqrt())
    coef = min(1.0, HYPER["max_grad_norm"] / (norm + 1e-6))
    gc = gu * coef
    m = b1 * m0.to(F64) + (1 - b1) * gc
    v = b2 * v0.to(F64) + (1 - b2) * gc * gc
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    upd = (lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps)
    p = p0.to(F64) * (1 - lr * wd) - upd
    units = dict(m=E * (b1 * m0.to(F64).abs() + (1 - b1) * gc.abs()), v=E * (b2 * v0.to(F64) + (1 - b2) * gc * gc),
                 p=E * (p0.to(F64).abs() + upd.abs()))
    return dict(p=p, m=m, v=v), units, sumsq_scaled, coef


def torch_fp32_step(p0, g_scaled, m0, v0, step):
    """torch's own fp32 path on the CPU: GradScaler's unscale (a multiply by 2^-16, exact), clip_grad_norm_, AdamW(foreach=False)."""
    P = torch.nn.Parameter(p0.clone())
    P.grad = g_scaled * HYPER["inv_loss_scale"]
    torch.nn.utils.clip_grad_norm_([P], HYPER["max_grad_norm"], foreach=False)
    opt = torch.optim.AdamW([P], lr=HYPER["lr"], betas=HYPER["betas"], eps=HYPER["eps"], weight_decay=HYPER["weight_decay"], foreach=False)
    opt.state[P] = {"step": torch.tensor(float(step - 1)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    opt.step()
    return dict(p=P.detach(), m=opt.state[P]["exp_avg"], v=opt.state[P]["exp_avg_sq"])


def worst_units(got, ref, units):
    return {k: float(((got[k].to(F64) - ref[k]).abs() / units[k].clamp_min(1e-300)).max()) for k in ("m", "v", "p")}


def shadow_is_the_rounded_master(net):
    n = net.flat_params.numel()
    return torch.equal(net._shadow[: 2 * n].view(torch.int16), net.flat_params.detach().to(BF).view(torch.int16))


REGIMES = ("clipped", "unclipped", "zero", "loguniform")


def test_regimes_within_the_torch_fp32_budget(net):
    n = net.flat_params.numel()
    kernel, budget = {}, {}
    for regime in REGIMES:
        p, g, m, v = plants(n, regime)
        plant(net, p, g, m, v)
        cur = dict(p=p, m=m, v=v)
        for step in (6, 7, 8):
            ref, units, sumsq, coef = reference(cur["p"], g, cur["m"], cur["v"], step)
            tor = torch_fp32_step(cur["p"], g, cur["m"], cur["v"], step)
            stats = net.optim_step(step=step, **HYPER)
            new = state(net)
            st = stats.cpu()
            assert float(st[1]) == 0.0
            assert abs(float(st[0]) - sumsq) <= 1e-6 * sumsq, (regime, step, float(st[0]), sumsq)
            if regime in ("unclipped", "zero"):
                assert coef == 1.0
            elif regime == "clipped":
                assert coef < 0.1
            kernel[(regime, step)] = worst_units(new, ref, units)
            budget[(regime, step)] = worst_units(tor, ref, units)
            assert shadow_is_the_rounded_master(net), (regime, step)
            assert torch.equal(new["g"], g), "the step must not touch the gradients"
            cur = new
    for key in kernel:
        print(f"{key[0]:>10} step {key[1]}: kernel m/v/p {kernel[key]['m']:.2f} / {kernel[key]['v']:.2f} / {kernel[key]['p']:.2f} units   "
              f"torch fp32 {budget[key]['m']:.2f} / {budget[key]['v']:.2f} / {budget[key]['p']:.2f}")
    kw = {k: max(x[k] for x in kernel.values()) for k in ("m", "v", "p")}
    bw = {k: max(x[k] for x in budget.values()) for k in ("m", "v", "p")}
    print(f"worst over regimes and steps, n = {n}: kernel {kw['m']:.2f} / {kw['v']:.2f} / {kw['p']:.2f}   torch fp32 budget {bw['m']:.2f} / {bw['v']:.2f} / {bw['p']:.2f}")
    for k in ("m", "v", "p"):
        assert kw[k] <= bw[k], (k, kw, bw)


def _trainable_runs(net, live_tensor):
    """Arena ranges (sorted) with the flag of each tensor, by the given rule on the tensor's ordinal in arena order."""
    views = sorted(net._param_views, key=lambda t: t[1])
    return [(off, numel, bool(live_tensor(i))) for i, (_, off, numel, _) in enumerate(views)], views


def _unfreeze(net, views):
    """All tensors trainable again, and the engine told NOW: the model zeroes the gradient of a tensor that becomes trainable again when it
    next syncs the mask, which must not happen after a later test has planted its gradients."""
    for pp, *_ in views:
        pp.requires_grad_(True)
    net._sync_trainable()


def _set_mask(net, flags, views):
    for (p, *_), (_, _, live) in zip(views, flags):
        p.requires_grad_(live)


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")], ids=["+inf", "-inf", "nan"])
def test_one_non_finite_gradient_skips_the_step_everywhere(net, bad):
    from olmoasr_amd import zero
    n = net.flat_params.numel()
    p, g, m, v = plants(n, "clipped", seed=1)
    # the full step: element 0 and the arena's last element
    for at in (0, n - 1):
        gb = g.clone()
        gb[at] = bad
        plant(net, p, gb, m, v)
        before = state(net)
        stats = net.optim_step(step=6, **HYPER)
        after = state(net)
        assert float(stats.cpu()[1]) != 0.0 and same(before, after) is None, (at, same(before, after))
    # a ZeRO range: its first and last element
    be = zero.NativeBackend(net)
    off, ln = 4 * 1000, 4 * 30001
    for at in (off, off + ln - 1):
        gb = g.clone()
        gb[at] = bad
        plant(net, p, gb, m, v)
        before = state(net)
        stats = be.sumsq(off, ln).clone()
        ms, vs = m[off:off + ln].to(DEV), v[off:off + ln].to(DEV)
        be.step(off, ln, ms, vs, stats, step=6, **HYPER)
        after = state(net)
        assert float(stats.cpu()[1]) != 0.0 and same(before, after, keys=("p", "sh")) is None
        assert torch.equal(ms.cpu().view(torch.int32), m[off:off + ln].view(torch.int32)) and torch.equal(vs.cpu().view(torch.int32), v[off:off + ln].view(torch.int32))
        for lo, k in ((off - 4, 4), (off + ln, 4)):  # neighbours of the range: the flag is the range's own
            assert float(be.sumsq(lo, k).cpu()[1]) == 0.0
    # a trainable run of a partly frozen model: its first and last element
    flags, views = _trainable_runs(net, lambda i: 10 <= i < 30)
    try:
        _set_mask(net, flags, views)
        runs = net.trainable_ranges()
        assert len(runs) == 1
        lo, ln = runs[0]
        for at in (lo, lo + ln - 1):
            gb = g.clone()
            gb[at] = bad
            plant(net, p, gb, m, v)
            before = state(net)
            stats = net.optim_step(step=6, **HYPER)
            after = state(net)
            assert float(stats.cpu()[1]) != 0.0 and same(before, after) is None, (at, same(before, after))
    finally:
        _unfreeze(net, views)


@pytest.mark.parametrize("mask", ["one_run", "alternate_tensors"])
def test_frozen_tensors(net, mask):
    """Frozen ranges of all four arenas are bit-identical after the step; NaN and 1e30 in frozen gradients neither set the flag nor move the
    norm; the trainable ranges equal, bit for bit, the all-trainable kernel on the same arenas with the frozen gradients zeroed."""
    n = net.flat_params.numel()
    p, g, m, v = plants(n, "clipped", seed=2)
    flags, views = _trainable_runs(net, (lambda i: 10 <= i < 30) if mask == "one_run" else (lambda i: i % 2 == 0))
    live = torch.zeros(n, dtype=torch.bool)
    for off, numel, t in flags:
        live[off:off + numel] = t
    g_frozen_poison = g.clone()
    frozen_idx = (~live).nonzero().flatten()
    g_frozen_poison[frozen_idx[0::2]] = float("nan")
    g_frozen_poison[frozen_idx[1::2]] = 1e30
    try:
        _set_mask(net, flags, views)
        runs = net.trainable_ranges()
        assert (len(runs) == 1) if mask == "one_run" else (len(runs) >= 20), len(runs)
        plant(net, p, g_frozen_poison, m, v)
        before = state(net)
        ref, units, sumsq, coef = reference(p, g, m, v, 6, live=live)
        stats = net.optim_step(step=6, **HYPER).cpu().clone()
        after = state(net)
        assert float(stats[1]) == 0.0, "a non-finite FROZEN gradient must not raise the flag"
        assert abs(float(stats[0]) - sumsq) <= 1e-6 * sumsq, (float(stats[0]), sumsq)
        assert same(before, after, sel=~live) is None, same(before, after, sel=~live)
        assert torch.equal(after["g"].view(torch.int32), g_frozen_poison.view(torch.int32))
        w = {k: float(((after[k].to(F64) - ref[k]).abs() / units[k].clamp_min(1e-300))[live].max()) for k in ("m", "v", "p")}
        print(f"frozen ({mask}, {len(runs)} runs): kernel m/v/p {w['m']:.2f} / {w['v']:.2f} / {w['p']:.2f} units on the trainable ranges")
        assert shadow_is_the_rounded_master(net)
    finally:
        _unfreeze(net, views)
    # the all-trainable kernel, frozen gradients zeroed: the same clip norm, so the trainable ranges must agree bit for bit
    plant(net, p, torch.where(live, g, torch.zeros(())), m, v)
    stats_all = net.optim_step(step=6, **HYPER).cpu().clone()
    full = state(net)
    assert float(stats_all[0]) == float(stats[0]), (float(stats_all[0]), float(stats[0]))
    assert same(after, full, sel=live) is None, same(after, full, sel=live)


def test_three_unequal_zero_ranges_reproduce_the_full_step(net):
    from olmoasr_amd import zero
    n = net.flat_params.numel()
    p, g, m, v = plants(n, "loguniform", seed=3)
    plant(net, p, g, m, v)
    stats_full = net.optim_step(step=7, **HYPER).clone()
    full = state(net)
    plant(net, p, g, m, v)
    be = zero.NativeBackend(net)
    cuts = [0, 4 * 1000, 4 * 1000 + 4 * 30001, n]
    ranges = [(cuts[i], cuts[i + 1] - cuts[i]) for i in range(3)]
    assert len({ln for _, ln in ranges}) == 3 and all(off % 4 == 0 and ln % 4 == 0 and ln > 0 for off, ln in ranges)
    total = torch.zeros(2, device=DEV)
    for off, ln in ranges:
        total += be.sumsq(off, ln)
    assert abs(float(total[0]) - float(stats_full[0])) <= 1e-6 * float(stats_full[0]) and float(total[1]) == 0.0
    ms, vs = [], []
    for off, ln in ranges:
        a, b = m[off:off + ln].to(DEV), v[off:off + ln].to(DEV)
        be.step(off, ln, a, b, stats_full, step=7, **HYPER)
        ms.append(a)
        vs.append(b)
    sharded = state(net)
    sharded["m"], sharded["v"] = torch.cat(ms).cpu(), torch.cat(vs).cpu()
    assert same(full, sharded) is None, same(full, sharded)


def test_a_finite_gradient_whose_square_overflows_fp32(net):
    """include/oasr.h at oasr_optim_step: the sum of squares is formed from fp32 squares, so a finite scaled gradient above 1.8e19 makes
    stats[0] +inf WITHOUT the non-finite flag; the clip coefficient is then max_norm / inf = 0 and the step runs with every gradient taken
    as zero (moments decay, weight decay and the momentum term apply) -- where torch would run a clipped step.  Pinned here: exactly the
    zero-gradient step, everything finite."""
    n = net.flat_params.numel()
    p, g, m, v = plants(n, "unclipped", seed=4)
    g[[5, n // 2, n - 3]] = 1e20
    plant(net, p, g, m, v)
    stats = net.optim_step(step=6, **HYPER).cpu().clone()
    got = state(net)
    assert float(stats[1]) == 0.0 and float(stats[0]) == float("inf"), stats
    for k in ("p", "m", "v"):
        assert bool(torch.isfinite(got[k]).all()), k
    plant(net, p, torch.zeros(n), m, v)
    net.optim_step(step=6, **HYPER)
    zero_step = state(net)
    assert same(got, zero_step) is None, same(got, zero_step)
