"""Compact grids of the span-limited attention launches (include/oasr.h: oasr_attn_args.qblk128 / qblk256, csrc/attention.hip): with a
block table the chunked-row kernels start one workgroup per query block INSIDE the spans instead of one per block of the padded context.
Nothing a workgroup computes changes, so everything here is an equality:

 * the tables the device kernel builds (the one oasr_train_step uses) against a host restatement;
 * forward and backward, decoder self-attention and cross-attention, with the table == the same call with the hook forcing the full
   grid (whole buffers, sentinel rows included) == the plain layout's result inside the spans; rows past the span keep their sentinel;
 * the fused bias gradients, from a scratch buffer that holds garbage on entry (the rows of the blocks that are not launched any more
   are zeroed by the launcher);
 * an all-zero span batch launches nothing and changes nothing;
 * one whole span-forward training step with the tables against the same step on full grids.

Shapes: H = 2, Tq = 448, spans [0, 64, 128, 192, 448, 320]: a sample without a block, half-filled 128-blocks, a second 256-block;
n128 * H = 22 and n256 * H = 14 workgroups (no multiple of 8: the remainder branch of xcd_remap), and B = 5 for n128 * H = 16."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DEV = "cuda"
H, TQ, TK_CROSS = 2, 448, 192
D = H * 64
SPANS = [0, 64, 128, 192, 448, 320]
KV_LEN = [0, 50, 128, 130, 448, 300]  # decoder self-attention: the first masked key column, <= the span
SENT = -7.0  # finite, exact in bf16: torch.equal can compare buffers that still hold it


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(DEV)


@pytest.fixture
def lib(monkeypatch):
    from olmoasr_amd import _native as N
    monkeypatch.setenv("OASR_TESTING_HOOKS", "1")
    handle = N.lib()
    yield handle
    handle.oasr_attention_set_span_grid(1)
    handle.oasr_attention_set_pingpong(1)


def host_block_table(spans, heads, gran):
    out = []
    for b, s in enumerate(spans):
        s64 = (s + 63) // 64 * 64
        nb = (s64 + gran - 1) // gran
        out += [(b << 16) | (h << 4) | j for h in range(heads) for j in range(nb)]
    return out


@pytest.mark.parametrize("spans,heads,S", [(SPANS, H, TQ), (SPANS[:5], H, TQ), ([0, 0], 3, TQ), ([1, 65, 129, 448, 257, 0, 300], 5, TQ),
                                           ([1024, 7, 513], 2, 1024)])
def test_block_tables_match_the_host_restatement(spans, heads, S):
    from olmoasr_amd import ops
    B = len(spans)
    blk128, blk256, n128, n256 = ops.span_block_tables(spans, B, S, heads)
    torch.cuda.synchronize()
    for blk, n, gran in ((blk128, n128, 128), (blk256, n256, 256)):
        ref = host_block_table(spans, heads, gran)
        assert n * heads == len(ref)
        got = blk.cpu().tolist()
        assert got[:len(ref)] == ref
        assert all(v == -1 for v in got[len(ref):])  # nothing written past the last entry
    if spans == SPANS:
        assert (n128 * heads, n256 * heads) == (22, 14)
    if spans == SPANS[:5]:
        assert n128 * heads == 16


_problems = {}


def _problem(kind, B):
    """Operands in both layouts and the plain layout's forward for the first B samples (built once per case and left unchanged)."""
    if (kind, B) in _problems:
        return _problems[(kind, B)]
    from olmoasr_amd import ops
    causal = kind == "self"
    Tk = TQ if causal else TK_CROSS
    g = torch.Generator().manual_seed(5)
    pairs = [(b, c) for b in range(B) for c in range(TQ // 64)]
    tab = ops.chunk_rows_table([pairs[i] for i in torch.randperm(len(pairs), generator=g).tolist()], B, TQ // 64)
    if causal:
        qkv = rnd(len(SPANS), TQ, 3 * D, seed=21)[:B].contiguous()
        q, k, v = (qkv[:, :, i * D:(i + 1) * D].unflatten(2, (H, 64)) for i in range(3))
        qkv_c = ops.to_chunked(qkv, tab)
        qc, kc, vc = (qkv_c[:, i * D:(i + 1) * D].unflatten(1, (H, 64)) for i in range(3))
        kv_len = torch.tensor(KV_LEN[:B], dtype=torch.int32, device=DEV)
    else:
        qb, kvb = rnd(len(SPANS), TQ, D, seed=22)[:B].contiguous(), rnd(len(SPANS), Tk, 2 * D, seed=23)[:B].contiguous()
        q = qb.unflatten(2, (H, 64))
        k, v = (kvb[:, :, i * D:(i + 1) * D].unflatten(2, (H, 64)) for i in range(2))
        qc = ops.to_chunked(qb, tab).unflatten(1, (H, 64))
        kc, vc, kv_len = k, v, None
    o, lse, o_lo = ops.attention_fwd(q, k, v, kv_len, causal, want_o_lo=True)
    d_o = rnd(len(SPANS), TQ, D, seed=24, scale=0.5)[:B].contiguous()
    keep = (torch.arange(TQ)[None, :] < torch.tensor(SPANS[:B])[:, None]).to(DEV)  # [B, Tq]
    p = dict(causal=causal, Tk=Tk, tab=tab, tab_d=tab.to(DEV), q=q, k=k, v=v, qc=qc, kc=kc, vc=vc, kv_len=kv_len, o=o, lse=lse, o_lo=o_lo,
             d_o=d_o, keep=keep, bwd={})
    _problems[(kind, B)] = p
    return p


def _plain_bwd(p, pingpong):
    """The plain layout's backward with d_o zero past the spans (once per kernel path)."""
    from olmoasr_amd import ops
    if pingpong not in p["bwd"]:
        d_o0 = torch.where(p["keep"][:, :, None], p["d_o"], torch.zeros_like(p["d_o"]))
        p["bwd"][pingpong] = ops.attention_bwd(p["q"], p["k"], p["v"], p["o"], p["lse"], d_o0, p["kv_len"], p["causal"], o_lo=p["o_lo"])
    return p["bwd"][pingpong]


@pytest.mark.parametrize("B", [6, 5])
@pytest.mark.parametrize("kind,pingpong", [("self", 1), ("cross", 1), ("cross", 0)])
def test_compact_grid_equals_full_grid_and_plain_layout(lib, kind, pingpong, B):
    from olmoasr_amd import ops
    assert lib.oasr_attention_set_pingpong(pingpong) == 0
    p = _problem(kind, B)
    causal, Tk, tab = p["causal"], p["Tk"], p["tab"]
    spans = SPANS[:B]
    span_d = torch.tensor(spans, dtype=torch.int32, device=DEV)
    blocks = ops.span_block_tables(spans, B, TQ, H)
    assert (blocks[2] * H, blocks[3] * H) == ((22, 14) if B == 6 else (16, 10))
    kv_len, kc, vc, q_rows, k_rows = p["kv_len"], p["kc"], p["vc"], p["tab_d"], (p["tab_d"] if causal else None)
    keep = p["keep"]
    keep_d = keep[:, :, None].expand(B, TQ, D)

    def unchunk(xc):  # [B * Tq, d] chunked -> [B, Tq, d]
        return ops.from_chunked(xc, tab, B, TQ)

    # ---- forward: table == full grid on the whole buffers; == plain inside the spans; sentinel past them
    fwd = {}
    for grid in (1, 0):
        assert lib.oasr_attention_set_span_grid(grid) == 0
        fwd[grid] = ops.attention_fwd_rows(p["qc"], kc, vc, B, H, TQ, Tk, q_rows, k_rows, kv_len, causal, want_o_lo=True, q_span=span_d,
                                           q_blocks=blocks, fill=SENT)
    for got, ref, name in zip(fwd[1], fwd[0], ("o", "lse", "o_lo")):
        assert torch.equal(got, ref), f"forward {name}: table vs full grid"
    oc, lse_c, o_lo_c = fwd[1]
    for got_c, ref, name in ((oc, p["o"], "o"), (o_lo_c, p["o_lo"], "o_lo")):
        got = unchunk(got_c)
        assert torch.equal(got[keep_d], ref[keep_d]), name + " inside the spans vs the plain layout"
        assert bool((got[~keep_d] == SENT).all()), name + " rows past the span must stay untouched"
    keep_l = keep[:, None, :].expand(B, H, TQ)
    assert torch.equal(lse_c[keep_l], p["lse"][keep_l])
    assert bool((lse_c[~keep_l] == SENT).all())

    # ---- backward: d_o / o / o_lo hold NaN past the spans (never read); gradients and bias gradients table == full grid
    nan = float("nan")
    doc = ops.to_chunked(torch.where(p["keep"][:, :, None], p["d_o"], torch.full_like(p["d_o"], nan)), tab)
    oc_p = ops.to_chunked(torch.where(p["keep"][:, :, None], p["o"], torch.full_like(p["o"], nan)), tab)
    olo_p = ops.to_chunked(torch.where(p["keep"][:, :, None], p["o_lo"], torch.full_like(p["o_lo"], nan)), tab)
    cs0 = [rnd(D, seed=31).float(), rnd(D, seed=32).float()]  # the accumulators' values on entry
    bwd, cs = {}, {}
    for grid in (1, 0):
        assert lib.oasr_attention_set_span_grid(grid) == 0
        cs[grid] = [cs0[0].clone(), cs0[1].clone()]
        bwd[grid] = ops.attention_bwd_rows(p["qc"], kc, vc, oc_p, p["lse"], doc, B, H, TQ, Tk, q_rows, k_rows, span_d, kv_len,
                                           causal, o_lo=olo_p, dq_colsum=cs[grid][0], dv_colsum=cs[grid][1], fill=SENT, q_blocks=blocks,
                                           scratch_fill=12345.0)
    torch.cuda.synchronize()
    for got, ref, name in zip(bwd[1], bwd[0], ("dq", "dk", "dv")):
        assert torch.equal(got, ref), f"backward {name}: table vs full grid"
    print(f"   bias gradients ({kind}, pingpong {pingpong}, B={B}): max |table - full grid| dq {float((cs[1][0] - cs[0][0]).abs().max()):.3e}, "
          f"dv {float((cs[1][1] - cs[0][1]).abs().max()):.3e}")
    assert torch.equal(cs[1][0], cs[0][0]), "dq_colsum: table vs full grid"
    assert torch.equal(cs[1][1], cs[0][1]), "dv_colsum: table vs full grid"
    assert float((cs[1][0] - cs0[0]).abs().max()) > 0 and float((cs[1][0]).abs().max()) < 1e4  # accumulated, and no scratch garbage in it

    dq_p, dk_p, dv_p = _plain_bwd(p, pingpong)
    dqc, dkc, dvc = bwd[1]
    got_q, ref_q = unchunk(dqc.reshape(B * TQ, D)), dq_p.reshape(B, TQ, D)
    assert torch.equal(got_q[keep_d], ref_q[keep_d]), "dq inside the spans vs the plain layout"
    assert bool((got_q[~keep_d] == SENT).all()), "dq rows past the span must stay untouched"
    if causal:
        for got, ref, name in ((dkc, dk_p, "dk"), (dvc, dv_p, "dv")):
            g2, r2 = unchunk(got.reshape(B * TQ, D)), ref.reshape(B, TQ, D)
            assert torch.equal(g2[keep_d], r2[keep_d]), name + " inside the spans vs the plain layout"
            assert bool((g2[~keep_d] == SENT).all()), name + " rows past the span must stay untouched"
    else:
        assert torch.equal(dkc, dk_p) and torch.equal(dvc, dv_p)


@pytest.mark.parametrize("kind", ["self", "cross"])
def test_an_all_zero_span_batch_launches_nothing(lib, kind):
    from olmoasr_amd import ops
    B = 5
    p = _problem(kind, B)
    causal, Tk = p["causal"], p["Tk"]
    kv_len, kc, vc, q_rows, k_rows = p["kv_len"], p["kc"], p["vc"], p["tab_d"], (p["tab_d"] if causal else None)
    span_d = torch.zeros(B, dtype=torch.int32, device=DEV)
    blocks = ops.span_block_tables([0] * B, B, TQ, H)
    assert blocks[2:] == (0, 0)
    assert lib.oasr_attention_set_span_grid(1) == 0
    oc, lse_c, o_lo_c = ops.attention_fwd_rows(p["qc"], kc, vc, B, H, TQ, Tk, q_rows, k_rows, kv_len, causal, want_o_lo=True, q_span=span_d,
                                               q_blocks=blocks, fill=SENT)
    assert all(bool((t == SENT).all()) for t in (oc, lse_c, o_lo_c))
    cs0 = [rnd(D, seed=41).float(), rnd(D, seed=42).float()]
    cs = [cs0[0].clone(), cs0[1].clone()]
    poison = torch.full((B * TQ, D), float("nan"), device=DEV, dtype=BF)
    dq, dk, dv = ops.attention_bwd_rows(p["qc"], kc, vc, poison, p["lse"], poison, B, H, TQ, Tk, q_rows, k_rows, span_d, kv_len,
                                        causal, o_lo=poison, dq_colsum=cs[0], dv_colsum=cs[1], fill=SENT, q_blocks=blocks, scratch_fill=12345.0)
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in (dq, dk, dv))  # (cross-attention too: without a query block the whole backward is skipped)
    assert torch.equal(cs[0], cs0[0]) and torch.equal(cs[1], cs0[1])


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def test_whole_span_step_with_tables_equals_the_step_on_full_grids(lib):
    """One span-forward training step of the tiny model: the loss and the predictions (everything on the activation side) are equal, the
    gradients equal up to the order of the fp32 atomics of the weight-gradient sums -- the bound tests/test_gpu_span.py holds the span step
    to against the plain step."""
    from olmoasr_amd import ops
    from olmoasr_amd.config.model_dims import VARIANT_TO_DIMS
    from olmoasr_amd.model import OLMoASR
    from olmoasr_amd.synth import synth_samples
    B = 4
    net = OLMoASR(VARIANT_TO_DIMS["tiny"], device=DEV, seed=0)
    pcm, ti, ty, tl = synth_samples(list(range(70, 70 + B)), DEV)
    mel = ops.log_mel(pcm)
    span = (net.supervised_span(ty, tl) + torch.tensor([0, 200, 448, 70], dtype=torch.int32)).clamp(max=448)  # mixed: any upper bound is legal
    assert len({(int(s) + 63) // 64 for s in span}) >= 3, span
    res = {}
    for grid in (1, 0):
        assert lib.oasr_attention_set_span_grid(grid) == 0
        net.zero_grad()
        pred = torch.full(tuple(ti.shape), -5, dtype=torch.int32, device=DEV)
        loss, _ = net.loss_and_backward(mel, ti, ty, tl, loss_scale=1024.0, span=span, span_forward=True, pred_out=pred)
        torch.cuda.synchronize()
        res[grid] = (float(loss), pred, net.flat_grads.clone())
    total = _rel(res[1][2], res[0][2])
    print(f"   span step, tables vs full grids (tiny, B={B}, spans {span.tolist()}): loss {res[1][0]:.7f} vs {res[0][0]:.7f}, grads rel-L2 {total:.2e}")
    assert res[1][0] == res[0][0]
    assert torch.equal(res[1][1], res[0][1])
    assert bool(torch.isfinite(res[1][2]).all())
    assert total <= 1e-5, total
    del net
    torch.cuda.empty_cache()
