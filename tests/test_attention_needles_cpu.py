"""Power of the planted-score attention tests (tests/attn_needles.py), in float64 on the CPU: every scenario, emulated without a
flaw, lies far inside the bounds the GPU tests use; emulated with a flaw it is built to expose (key at kv_len admitted, zero
phantom key admitted, causal diagonal shifted by one, a rescale that forgets O or l), it misses them by at least 10x."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_needles as an  # noqa: E402

# (scenario, B, H, Tq, Tk, causal, kv_len): the GPU test's shapes, with fewer heads (the margins are per slice)
CASES = [
    ("masked", 3, 2, 448, 448, True, [7, 220, 448]),
    ("masked", 2, 2, 448, 1500, False, [1000, 1437]),
    ("masked", 2, 1, 128, 130, False, [64, 129]),
    ("phantom", 1, 2, 100, 65, False, None),
    ("phantom", 1, 2, 100, 127, False, None),
    ("phantom", 1, 2, 100, 257, False, None),
    ("phantom", 1, 2, 100, 1000, False, None),
    ("phantom", 2, 1, 160, 1500, False, None),
    ("plateau", 1, 2, 256, 1500, False, None),
    ("plateau", 2, 1, 128, 1024, False, None),
    ("onehot", 2, 6, 130, 1500, False, [1200, 1500]),
    ("onehot", 2, 6, 130, 1500, False, None),
    ("onehot", 2, 3, 64, 257, False, [200, 257]),
    ("uniform", 2, 1, 100, 1000, False, None),
    ("uniform", 2, 1, 100, 1500, False, [700, 1500]),
    ("offset", 2, 1, 100, 1500, False, None),
]


def _id(c):
    return f"{c[0]}-B{c[1]}H{c[2]}-{c[3]}x{c[4]}{'-causal' if c[5] else ''}{'-kvlen' if c[6] else ''}"


@pytest.mark.parametrize("spec", CASES, ids=[_id(c) for c in CASES])
def test_each_flaw_misses_the_bound_by_10x(spec):
    sc, B, H, Tq, Tk, causal, kv_len = spec
    case = an.make(sc, B, H, Tq, Tk, causal=causal, kv_len=kv_len, seed=1)
    ref = an.reference(case)
    tol_o, tol_lse = an.fwd_bounds(case, ref)
    o, lse = an.emulate(case)
    clean = max(an.margin(o, ref["o"], tol_o), an.margin(lse, ref["lse"], tol_lse))
    assert clean < 1e-6, f"the flawless emulation is off the reference by {clean:.3g} of the bound"
    flaws = an.applicable_flaws(case)
    assert flaws, "every scenario is built to expose at least one flaw"
    report = []
    for flaw in flaws:
        o, lse = an.emulate(case, flaw)
        m = max(an.margin(o, ref["o"], tol_o), an.margin(lse, ref["lse"], tol_lse))
        report.append(f"{flaw} {m:.3g}x")
        assert m >= 10.0, f"{flaw}: misses the bound by only {m:.3g}x"
    print(f"{_id(spec)}: margins over the GPU bound: " + ", ".join(report))


def test_plateau_step_crosses_the_rescale_threshold_in_even_waves_only():
    """Even rows of even waves step +6 nats (> 8 log2 units over the plateau's maximum, noise included), every other row +5 (< 8):
    the emulated forward raises its maximum at the stepped tile in even waves and never in odd ones."""
    case = an.make("plateau", 1, 1, 128, 1500, seed=3)
    s = (case.q[0, :, 0].double() @ case.k[0, :, 0].double().T) * an.SCALE * an.LOG2E
    plateau_max = s[:, :an.STEP0].max(-1).values
    step_max = s[:, an.STEP0:an.STEP0 + 64].max(-1).values
    jump = step_max - plateau_max
    i = torch.arange(128)
    even = ((i // 32) % 2 == 0) & (i % 2 == 0)
    assert bool((jump[even] > an.RESCALE_THR + 0.3).all()) and bool((jump[~even] < an.RESCALE_THR - 0.6).all())
    wave_fires = [bool((jump[w:w + 32] > an.RESCALE_THR).any()) for w in range(0, 128, 32)]
    assert wave_fires == [True, False, True, False]
    # the mass before the step is a few percent of the total
    p = torch.softmax(s / an.LOG2E, -1)
    pre = p[:, :an.STEP0].sum(-1)
    assert 0.02 < float(pre[even].max()) < 0.05 and 0.05 < float(pre[~even].min()) and float(pre.max()) < 0.12


@pytest.mark.parametrize("sc", an.SCENARIOS)
def test_planted_scores_survive_bf16_rounding(sc):
    """Channel 0 carries r_i t_j exactly; with the noise channels zeroed the bf16 operands give exactly the planted scores."""
    causal = sc == "masked"
    Tk = 1500 if sc == "plateau" else 448
    case = an.make(sc, 2, 3, 448 if causal else 96, 448 if causal else Tk, causal=causal, kv_len=[300, 448] if causal else None,
                   seed=2, noise=False)
    q, k = case.q.double(), case.k.double()
    assert torch.equal(q[..., 1:], torch.zeros_like(q[..., 1:])) and case.noise_bound == 0.0
    s = torch.einsum("bihc,bjhc->bhij", q, k) * an.SCALE
    planted = case.r[..., :, None] * case.t[..., None, :]
    assert torch.equal(s, planted)
    assert torch.equal(q[..., 0].permute(0, 2, 1), 8 * case.r) and torch.equal(k[..., 0].permute(0, 2, 1), case.t)
    # and with noise, the noise stays inside its documented bound
    noisy = an.make(sc, 2, 3, 448 if causal else 96, 448 if causal else Tk, causal=causal, kv_len=[300, 448] if causal else None, seed=2)
    s2 = torch.einsum("bihc,bjhc->bhij", noisy.q.double(), noisy.k.double()) * an.SCALE
    p2 = noisy.r[..., :, None] * noisy.t[..., None, :]
    assert float((s2 - p2).abs().max()) <= noisy.noise_bound
    if sc != "offset":
        assert noisy.noise_bound <= 2.0


def test_causal_ramp_puts_every_future_key_above_every_visible_one():
    case = an.make("masked", 1, 1, 448, 448, causal=True, kv_len=[448], seed=4)
    t = case.t[0, 0]
    assert bool((t[1:] > t[:-1]).all())
    gap = (t[1:] - t[:-1]) * case.r[0, 0, 0]
    assert float(gap.min()) >= 1.0 and 2 * case.noise_bound < 1.0  # >= 1 nat per step against <= 0.5 nats of noise


def test_closed_forms():
    """one-hot: O = V[peak] to 1e-12; uniform: O = mean(V[:kv_len]), lse = -30 + log(kv_len)."""
    case = an.make("onehot", 2, 6, 64, 1500, kv_len=[1200, 1500], seed=5)
    ref = an.reference(case)
    for b in range(2):
        for h in range(6):
            pk = int(case.peak[b, h])
            want = case.v[b, pk, h].double()
            assert float((ref["o"][b, :, h] - want).abs().max()) < 1e-12 * (1 + float(want.abs().max()))
    peaks = {int(p) for p in case.peak.flatten()}
    assert {0, 63, 64, 127, 128, 255, 256, 1199, 1499} <= peaks
    case = an.make("uniform", 2, 1, 32, 1000, kv_len=[700, 1000], seed=6)
    ref = an.reference(case)
    for b, n in enumerate((700, 1000)):
        mean = case.v[b, :n, 0].double().mean(0)
        assert float((ref["o"][b, :, 0] - mean).abs().max()) < 1e-12
        assert float((ref["lse"][b, 0] - (-30 + math.log(n))).abs().max()) < 1e-12


def test_reference_backward_equals_float64_autograd():
    """The explicit backward of an.reference (P, dP, delta) against torch autograd of the same float64 softmax attention."""
    case = an.make("masked", 2, 2, 96, 96, causal=True, kv_len=[50, 96], seed=7)
    B, H, Tq, Tk = case.shape
    d_o = (torch.randn(B, Tq, H * 64, generator=torch.Generator().manual_seed(1)) * 0.5).to(an.BF)
    ref = an.reference(case, d_o)
    q, k, v = (x.double().requires_grad_(True) for x in (case.q, case.k, case.v))
    s = torch.einsum("bihc,bjhc->bhij", q, k) * an.SCALE
    mask = torch.ones(Tq, Tk, dtype=torch.bool).triu(1)[None, None] | (torch.arange(Tk)[None, None, None, :] >= torch.tensor([50, 96])[:, None, None, None])
    o = torch.einsum("bhij,bjhc->bihc", torch.softmax(s.masked_fill(mask, -math.inf), -1), v)
    o.backward(d_o.double().reshape(B, Tq, H, 64))
    for name, g in (("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        assert float((ref[name] - g).abs().max()) < 1e-9 * (1 + float(g.abs().max())), name
    assert float((ref["o"] - o.detach()).abs().max()) < 1e-12
