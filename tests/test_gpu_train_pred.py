"""Teacher-forced predictions of the span step (csrc/argmax.hip, ``loss_and_backward(pred_out=...)``): the kernel alone on planted
matrices through oasr_test_argmax_rows, the step at tiny against the plain step's fp32 logits, the refusals, the decoder-only step, and the
counts of ``metrics.ErrorCounter`` on the step's own predictions against the host path."""
import importlib.util
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 51865
EOT, IGNORE = 50256, 51864
SPANS = [5, 64, 130]


def ceil64(x):
    return (x + 63) // 64 * 64


# ---- the kernel alone -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,LD", [(torch.bfloat16, 51968), (torch.float32, 51968), (torch.float32, V)], ids=["bf16", "fp32", "fp32_ld_V"])
def test_argmax_rows_on_planted_matrices(dtype, LD):
    """Three samples of S = 128 positions whose 64-position chunks sit in a permuted order in a [384, 51968] matrix; spans 128 / 64 / 64.
    Rows with the maximum at column 0, at column 51864, two and three equal maxima, a huge value in the padded columns and an all-equal row
    sit among random ones (where bf16 ties among 51865 values occur by themselves).  ld = V is the fp32 engine's own row stride: rows that are
    not 16-byte aligned, read column by column."""
    from olmoasr_amd import ops
    B, S = 3, 128
    g = torch.Generator().manual_seed(0)
    mat = torch.randn(B * S, LD, generator=g).to(dtype)
    tab = torch.full((B, 16), 0x3fffffff, dtype=torch.int32)
    tab[0, :2], tab[1, :2], tab[2, :2] = torch.tensor([128, 0]), torch.tensor([192, 320]), torch.tensor([64, 256])
    span = torch.tensor([128, 64, 64], dtype=torch.int32)
    mat[:, V:] = 1.0e30  # the padding of every row: never a candidate
    r = int(tab[0, 0])  # sample 0, positions 0 .. 5
    mat[r + 0, 0] = 50.0
    mat[r + 1, V - 1] = 50.0
    mat[r + 2, 40000], mat[r + 2, 100] = 50.0, 50.0
    mat[r + 3, 51864], mat[r + 3, 7], mat[r + 3, 30001] = 50.0, 50.0, 50.0
    mat[r + 4, :V] = -3.0
    mat[r + 4, 12345] = -2.5
    mat[r + 5, :V] = 0.25
    r2 = int(tab[0, 1])  # sample 0, position 64 + 9: the second chunk, equal maxima in one 16-byte piece and across the last piece
    mat[r2 + 9, 8], mat[r2 + 9, 9], mat[r2 + 9, V - 1] = 60.0, 60.0, 60.0
    dmat = mat.to(DEV)
    pred = torch.full((B + 1, S), -777, dtype=torch.int32, device=DEV)  # one guard row
    ops.argmax_rows_(dmat, V, tab.to(DEV), span.to(DEV), pred[:B])
    got = pred.cpu()
    assert (got[B] == -777).all()
    best = torch.argmax(dmat[:, :V].float(), dim=1).cpu()
    want = torch.full((B, S), -1, dtype=torch.int64)
    for b in range(B):
        for s in range(int(span[b])):
            want[b, s] = best[int(tab[b, s >> 6]) + (s & 63)]
    assert torch.equal(got[:B].long(), want)
    assert want[0, :6].tolist() == [0, V - 1, 100, 7, 12345, 0] and int(want[0, 73]) == 8
    assert (got[1, 64:] == -1).all() and (got[2, 64:] == -1).all() and (got[:B, :64] >= 0).all()


# ---- the step ---------------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _batch():
    """B = 3 clips with hand-made token rows supervised exactly up to SPANS (so the spans 5 / 64 / 130 are legal bounds)."""
    from olmoasr_amd import ops
    from olmoasr_amd.synth import synth_samples
    pcm, _, _, _ = synth_samples([11, 12, 13], DEV)
    g = torch.Generator().manual_seed(4)
    ti = torch.randint(0, 50000, (3, 448), generator=g)
    ty = torch.randint(0, 50000, (3, 448), generator=g)
    for b, n in enumerate(SPANS):
        ti[b, n:], ty[b, n:] = EOT, IGNORE
        ty[b, n - 1] = EOT
    return ops.log_mel(pcm), ti.to(DEV), ty.to(DEV), torch.tensor(SPANS, dtype=torch.int32, device=DEV)


def _near_max(L, pred, dtype):
    """Per computed position: the picked logit is within one ulp (of the engine's logit type) of the row maximum of the plain step's logits."""
    ok = torch.ones_like(pred, dtype=torch.bool)
    same = total = 0
    for b, n in enumerate(SPANS):
        rows = L[b, :ceil64(n)]
        mx, am = rows.max(dim=1)
        p = pred[b, :ceil64(n)].long()
        picked = rows.gather(1, p.clamp(min=0)[:, None])[:, 0]
        if dtype == "bfloat16":  # one bf16 ulp of the maximum: 8 significant bits
            ulp = torch.exp2(torch.floor(torch.log2(mx.abs().clamp(min=1e-30))) - 7)
        else:
            ulp = torch.zeros_like(mx)
        ok[b, :ceil64(n)] = (p >= 0) & (p < V) & (picked >= mx - ulp)
        same += int((p == am).sum())
        total += p.numel()
    return ok, same / total


@pytest.fixture(scope="module")
def tt():
    spec = importlib.util.spec_from_file_location("tt_pred_gpu", os.path.join(ROOT, "scripts", "training", "train_timestamps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("span_forward", [True, False], ids=["fwd_active", "fwd_all"])
@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
def test_span_step_predictions(dtype, span_forward, tt):
    from olmoasr_amd import metrics, ops
    from olmoasr_amd.config.model_dims import VARIANT_TO_DIMS
    from olmoasr_amd.model import OLMoASR
    net = OLMoASR(VARIANT_TO_DIMS["tiny"], device=DEV, seed=0, compute_dtype=dtype)
    mel, ti, ty, tl = _batch()
    net.zero_grad()
    _, L = net.loss_and_backward(mel, ti, ty, tl, return_logits=True)  # the plain step: fp32 copy of the engine's logits, all 448 positions
    net.zero_grad()
    loss0, _ = net.loss_and_backward(mel, ti, ty, tl, span=SPANS, span_forward=span_forward)
    torch.cuda.synchronize()
    g0 = net.flat_grads.clone()
    pred = torch.full((4, 448), -777, dtype=torch.int32, device=DEV)  # one guard row
    net.zero_grad()
    loss1, lg = net.loss_and_backward(mel, ti, ty, tl, span=SPANS, span_forward=span_forward, pred_out=pred[:3])
    torch.cuda.synchronize()
    assert lg is None
    assert torch.equal(loss1, loss0), (float(loss1), float(loss0))  # the forward's arithmetic is the same
    rel = _rel(net.flat_grads, g0)
    assert rel <= 1e-6, rel  # the step's own run-to-run spread (fp32 atomics), tests/test_gpu_span.py
    assert (pred[3] == -777).all()
    p = pred[:3]
    for b, n in enumerate(SPANS):
        assert (p[b, ceil64(n):] == -1).all() and (p[b, :ceil64(n)] >= 0).all(), b
    ok, share = _near_max(L, p, dtype)
    print(f"   pred_out ({dtype}, span_forward={span_forward}): grads rel-L2 {rel:.2e}; share of positions with pred == argmax(plain logits): {share:.4f}")
    assert bool(ok.all()), ok.logical_not().nonzero().tolist()[:8]
    # end to end: the device counts of these predictions against the host path on the same ids (cut by the -1 rule)
    counter = metrics.ErrorCounter(DEV)
    counter.add(p, ty)
    preds, tgts = [], []
    for row in p.cpu().tolist():
        row = row[:row.index(-1)] if -1 in row else row
        preds.append(row[:row.index(EOT) + 1] if EOT in row else row)
    for row in ty.cpu().tolist():
        row = [t for t in row if t != IGNORE]
        tgts.append((row[:row.index(EOT)] if EOT in row else row) + [EOT])
    s, d, i, h = counter.counts()
    assert (s + d + i, s + d + h) == tt.token_error_counts(preds, tgts)
    hp, hl = metrics.pad_sequences(preds)
    rp, rl = metrics.pad_sequences(tgts)
    assert (s, d, i, h) == tuple(ops.edit_counts_host(hp, hl, rp, rl).sum(dim=0).tolist())
    assert s + d + h == sum(SPANS)
    del net
    torch.cuda.empty_cache()


def test_pred_out_refusals_and_decoder_only_step():
    from olmoasr_amd.config.model_dims import VARIANT_TO_DIMS
    from olmoasr_amd.model import OLMoASR
    net = OLMoASR(VARIANT_TO_DIMS["tiny"], device=DEV, seed=0)
    mel, ti, ty, tl = _batch()
    pred = torch.full((3, 448), -777, dtype=torch.int32, device=DEV)
    net.zero_grad()
    with pytest.raises(ValueError):
        net.loss_and_backward(mel, ti, ty, tl, pred_out=pred)                                    # without span
    with pytest.raises(ValueError):
        net.loss_and_backward(mel, ti, ty, tl, span=SPANS, return_logits=True, pred_out=pred)
    with pytest.raises(ValueError):
        net.loss_and_backward(mel, ti, ty, tl, span=SPANS, text_ctx=192, pred_out=pred)
    with pytest.raises(ValueError):
        net.loss_and_backward(mel, ti, ty, tl, span=SPANS, pred_out=pred.long())                 # not int32
    with pytest.raises(ValueError):
        net.loss_and_backward(mel, ti, ty, tl, span=SPANS, pred_out=pred[:2])                    # not [B, n_text_ctx]
    assert (pred == -777).all()  # nothing ran
    _, L = net.loss_and_backward(mel, ti, ty, tl, return_logits=True)
    net.zero_grad()
    loss_m, _ = net.loss_and_backward(mel, ti, ty, tl, span=SPANS, pred_out=pred)
    # the decoder alone on embed_audio's features
    xa = net.embed_audio(mel)
    net.encoder.requires_grad_(False)
    pred_d = torch.full((3, 448), -777, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        net.loss_and_backward(None, ti, ty, tl, audio_features=xa, pred_out=pred_d)              # without span
    net.zero_grad()
    loss_d, _ = net.loss_and_backward(None, ti, ty, tl, audio_features=xa, span=SPANS, pred_out=pred_d)
    torch.cuda.synchronize()
    for b, n in enumerate(SPANS):
        assert (pred_d[b, ceil64(n):] == -1).all()
    ok, share = _near_max(L, pred_d, "bfloat16")
    agree = float((pred_d == pred).float().mean())
    print(f"   decoder-only pred_out: loss {float(loss_d):.6f} vs {float(loss_m):.6f}; pred == argmax(plain logits) at {share:.4f}, == the mel step's "
          f"pred_out at {agree:.4f} of the positions")
    assert bool(ok.all()), ok.logical_not().nonzero().tolist()[:8]
    assert math.isfinite(float(loss_d))
    del net
    torch.cuda.empty_cache()
