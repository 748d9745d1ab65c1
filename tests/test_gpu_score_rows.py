"""csrc/score.hip as operators (``ops.score_rows`` / ``ops.score_reduce``): the planted cross-entropy rows of tests/vocab_planted.py under
that file's own row-loss bound, the argmax rows and reduce cases of tests/score_cases.py exactly, and the span rule."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_cases as sc  # noqa: E402
import vocab_planted as vp  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
LAYOUTS = ("bf16", "fp32_padded", "fp32_ld_V")


def _logits(case, layout):
    if layout == "bf16":
        return case["logits"]
    return vp.ce_f32_logits(case, padded=layout == "fp32_padded")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", vp.CE_CASES)
def test_planted_cross_entropy_rows(name, layout):
    """row_nll against float64 of the same logits under check_ce's row_loss bound, 2^-21 max(1, |x_max|, |x_t|) + 1e-6 |want|; exactly 0 for
    ignored and out-of-range targets; pred = the float64 row's argmax.  The pad columns hold NaN / 3e38 and must not matter."""
    from olmoasr_amd import ops
    case = vp.ce_case(name)
    e = vp.ce_expect(case)
    lg = _logits(case, layout).to(DEV)
    rows = lg.shape[0]
    nll, pred = ops.score_rows(lg, case["V"], case["targets"].view(1, rows).to(DEV), ignore=case["ignore"])
    nll, pred = nll.cpu().view(rows).double(), pred.cpu().view(rows).long()
    valid = e["valid"]
    mag = torch.maximum(torch.maximum(e["xmax"].abs(), e["xt"].abs()), torch.ones_like(e["xt"]))
    bound = 2.0 ** -21 * mag + 1e-6 * e["row_loss"].abs()
    err = (nll - e["row_loss"]).abs()
    worst = float((err / bound)[valid].max()) if bool(valid.any()) else 0.0
    print(f"   {name} {layout}: worst row_nll error / bound = {worst:.3f}")
    assert bool(torch.isfinite(nll).all())
    assert bool((err <= bound)[valid].all()), [(case["labels"][i], float(err[i]), float(bound[i])) for i in torch.nonzero(valid & (err > bound))[:4, 0]]
    assert bool((nll[~valid] == 0).all())
    assert torch.equal(pred, torch.argmax(case["x"], dim=1))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("V,ld", sc.ARGMAX_SHAPES)
def test_argmax_rows(V, ld, layout):
    """pred == torch.argmax(x[:, :V]) exactly: equal maxima in different threads, waves and chunks, the maximum at V - 1, poison above every
    logit in [V, ld), an all-equal row, an all -inf row (index 0).  The targets are ignored, so row_nll is exactly 0."""
    from olmoasr_amd import ops
    case = sc.argmax_case(V, ld)
    x = case["x"] if layout != "fp32_ld_V" else case["x"][:, :V].contiguous()
    lg = x.to(torch.bfloat16 if layout == "bf16" else torch.float32).to(DEV)
    rows = lg.shape[0]
    tgt = torch.full((rows, 1), sc.IGNORE, dtype=torch.int64, device=DEV)
    nll, pred = ops.score_rows(lg, V, tgt)
    got = pred.cpu().view(rows).long()
    want = case["want"]  # torch.argmax on the CPU (every planted value is exact in bf16)
    assert torch.equal(got, want), [(case["labels"][i], int(got[i]), int(want[i])) for i in torch.nonzero(got != want)[:6, 0]]
    assert bool((nll == 0).all())


@pytest.mark.parametrize("layout", LAYOUTS)
def test_span_rows_are_not_read(layout):
    """Rows at or past span give (0, -1) and are not read: NaN there changes nothing.  span = 0 for a whole sample works."""
    from olmoasr_amd import ops
    V, ld = vp.V_HEAD, (vp.V_HEAD if layout == "fp32_ld_V" else vp.LD_HEAD)
    B, S = 3, 8
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(B * S, ld, generator=g) * 2.5).to(torch.bfloat16 if layout == "bf16" else torch.float32)
    tgt = torch.randint(0, V, (B, S), generator=g)
    tgt[1, 2] = sc.IGNORE
    span = torch.tensor([0, 5, 8], dtype=torch.int32)
    clean = x.to(DEV)
    nll0, pred0 = ops.score_rows(clean, V, tgt.to(DEV), span.to(DEV))
    dirty = x.clone().view(B, S, ld)
    for b in range(B):
        dirty[b, int(span[b]):] = float("nan")
    nll1, pred1 = ops.score_rows(dirty.to(DEV), V, tgt.to(DEV), span.to(DEV))  # [B, S, ld] form
    assert torch.equal(nll0, nll1) and torch.equal(pred0, pred1)
    nll0, pred0 = nll0.cpu(), pred0.cpu()
    active = torch.arange(S)[None, :] < span[:, None]
    assert bool((nll0[~active] == 0).all()) and bool((pred0[~active] == -1).all())
    ref = x.view(B, S, ld)[:, :, :V].double()
    want = torch.logsumexp(ref, -1) - ref.gather(2, tgt.clamp(max=V - 1)[:, :, None])[:, :, 0]
    counted = active & (tgt != sc.IGNORE)
    xt = ref.gather(2, tgt.clamp(max=V - 1)[:, :, None])[:, :, 0]
    mag = torch.maximum(torch.maximum(ref.amax(-1).abs(), xt.abs()), torch.ones_like(xt))
    assert bool(((nll0.double() - want).abs() <= 2.0 ** -21 * mag + 1e-6 * want.abs())[counted].all())  # the planted rows' bound
    assert torch.equal(pred0[active].long(), torch.argmax(ref, -1)[active])
    assert float(nll0[1, 2]) == 0.0 and int(pred0[1, 2]) >= 0
    # without a span every row is scored
    nll2, pred2 = ops.score_rows(clean, V, tgt.to(DEV))
    assert bool((pred2 >= 0).all()) and torch.equal(nll2.cpu()[active], nll0[active])


@pytest.mark.parametrize("S", sc.REDUCE_S)
def test_reduce_is_the_host_twin_and_the_sequential_double_sum(S):
    from olmoasr_amd import ops
    case = sc.reduce_case(S)
    args = (case["row_nll"], case["pred"], case["targets"], case["span"])
    host = ops.score_reduce_host(*args, V=case["V"], ignore=case["ignore"])
    dev = ops.score_reduce(*(t.to(DEV) for t in args), V=case["V"], ignore=case["ignore"])
    for name, h, d, w in zip(("nll_sum", "nll_max", "n_tok", "n_hit"), host, dev, case["want"]):
        assert torch.equal(d.cpu(), h), name
        assert torch.equal(d.cpu(), w), (name, d.cpu().tolist(), w.tolist())
    for b in (0, 4):  # span 0; no valid target
        assert int(dev[2][b]) == 0 and float(dev[0][b]) == 0.0 and float(dev[1][b]) == 0.0
    if case["planted"]:
        assert float(np.float32(16777216.0) + np.float32(1.0)) == 16777216.0  # what a float32 accumulator would do with the plant


def test_operator_refusals():
    from olmoasr_amd import ops
    lg = torch.zeros(4, 16, dtype=torch.bfloat16, device=DEV)
    tgt = torch.zeros(2, 2, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        ops.score_rows(lg.cpu(), 9, tgt)
    with pytest.raises(ValueError):
        ops.score_rows(lg, 17, tgt)  # V > row width
    with pytest.raises(ValueError):
        ops.score_rows(lg[:3], 9, tgt)  # rows != B * S
    with pytest.raises(ValueError):
        ops.score_rows(lg, 9, tgt, span=torch.zeros(3, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.score_reduce(torch.zeros(2, 2, device=DEV), torch.zeros(2, 2, dtype=torch.int64, device=DEV), tgt, V=9)  # pred not int32
