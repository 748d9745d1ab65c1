"""Every attention kernel on planted-score inputs (tests/attn_needles.py) against the float64 reference, within bounds derived from
the kernels' rounding points (attn_needles.fwd_bounds / bwd_bounds: one bf16 rounding of P before its MFMA and one of each output,
fp32 scores and sums; the lse is fp32 throughout).  tests/test_attention_needles_cpu.py shows that each flaw a scenario targets
misses these bounds by >= 10x.  Which kernel branch each scenario reaches:
  masked   per-element boundary mask of the last kv_len tile (attn_fwd_kernel, attn_bwd_dq_kernel, attn_bwd_dkdv_kernel) and the
           causal diagonal tiles; attn_decode_kernel's t < n clamp; dK/dV blocks that are all padding (early exit, zeros written);
  phantom  the zero-filled tail rows of the last 64-key tile: masked in the general kernels, multiplied by zero K / V rows in the
           unmasked ping-pong backward kernels;
  plateau  the RESCALE_THR branch of attn_fwd_kernel at the stepped tile in even waves only; the stale-maximum regime (P up to
           2^7.2 packed to bf16) in odd waves; in the decode kernel, the merge of two segments whose maxima differ by 6 nats;
  onehot   O = V[peak] with the peak on tile edges (0, 63, 64, 127, 128, 255, 256, Tk - 1, kv_len - 1); dV[peak] = dO;
  uniform  O = mean(V): P = 1 exactly, only the fp32 sums and O's rounding remain;
  offset   scores near -80 nats: the running maximum starts from -1e30 and every P is relative to it."""
import functools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_needles as an  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def ops():
    from olmoasr_amd import ops as o
    return o


def _d_o(B, Tq, H, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, Tq, H * 64, generator=g) * 0.5).to(BF)


@functools.lru_cache(maxsize=None)
def _case_ref(spec, with_bwd=True):
    """(case on the CPU, d_o, float64 reference incl. the backward) -- shared by both attention paths."""
    sc, B, H, Tq, Tk, causal, kv_len = spec
    case = an.make(sc, B, H, Tq, Tk, causal=causal, kv_len=list(kv_len) if kv_len else None, seed=B * 100 + H)
    d_o = _d_o(B, Tq, H, seed=Tq + Tk) if with_bwd else None
    return case, d_o, an.reference(case, d_o)


def _check(name, got, want, tol):
    m = an.margin(got.cpu(), want, tol)
    assert m <= 1.0, f"{name}: off by {m:.3g}x the rounding-point bound"
    return m


# (scenario, B, H, Tq, Tk, causal, kv_len)
CASES = [
    ("masked", 3, 6, 448, 448, True, (7, 220, 448)),       # decoder self-attention: causal ramp + key padding
    ("masked", 2, 20, 448, 448, True, (64, 129)),
    ("masked", 2, 6, 448, 1500, False, (1000, 1437)),      # cross-attention with per-sample key length
    ("masked", 2, 1, 130, 130, False, (64, 129)),
    ("phantom", 2, 1, 100, 65, False, None),
    ("phantom", 2, 1, 100, 127, False, None),
    ("phantom", 2, 1, 100, 257, False, None),
    ("phantom", 2, 6, 300, 1000, False, None),
    ("phantom", 2, 6, 448, 1500, False, None),
    ("plateau", 2, 6, 448, 1500, False, None),
    ("plateau", 2, 1, 1500, 1500, False, None),            # encoder shape
    ("onehot", 2, 6, 448, 1500, False, None),
    ("onehot", 2, 20, 448, 1500, False, (1200, 1500)),
    ("onehot", 2, 1, 1500, 1500, False, None),
    ("uniform", 2, 6, 448, 1500, False, None),
    ("uniform", 2, 6, 200, 1500, False, (700, 1500)),
    ("offset", 2, 6, 1500, 1500, False, None),
    ("offset", 2, 1, 448, 1500, False, None),
]


def _id(c):
    return f"{c[0]}-B{c[1]}H{c[2]}-{c[3]}x{c[4]}{'-causal' if c[5] else ''}{'-kvlen' if c[6] else ''}"


def _with_paths(cases):
    """unmasked cases under both backward paths (1: ping-pong kernels, 0: general kernels); masked ones always run the general kernels"""
    out = []
    for c in cases:
        masked = c[5] or c[6]
        for p in ((1,) if masked else (1, 0)):
            out.append(pytest.param(c, p, id=f"{_id(c)}-{'pingpong' if p and not masked else 'general'}"))
    return out


@pytest.fixture
def set_path():
    from olmoasr_amd import _native as N
    yield lambda p: N.lib().oasr_attention_set_pingpong(p)
    N.lib().oasr_attention_set_pingpong(1)


@pytest.mark.parametrize("spec,path", _with_paths(CASES))
def test_attention_fwd_bwd_on_planted_scores(spec, path, set_path):
    set_path(path)
    case, d_o, ref = _case_ref(spec)
    B, H, Tq, Tk = case.shape
    c = an.to_device(case, DEV)
    kv_len = case.kv_len_tensor(DEV)
    o, lse, o_lo = ops().attention_fwd(c.q, c.k, c.v, kv_len, case.causal, want_o_lo=True)
    tol_o, tol_lse = an.fwd_bounds(case, ref)
    mo = _check("o", o.view(B, Tq, H, 64), ref["o"], tol_o)
    ml = _check("lse", lse, ref["lse"], tol_lse)
    if case.scenario == "onehot":  # closed form: O = V[peak] to one bf16 rounding
        vpk = torch.stack([torch.stack([case.v[b, int(case.peak[b, h]), h] for h in range(H)]) for b in range(B)]).double()
        assert float(((o.view(B, Tq, H, 64).cpu().double() - vpk[:, None]).abs() - an.EPS_BF * vpk[:, None].abs()).max()) <= 0
    if case.scenario == "uniform":  # closed form: O = mean(V[:kv_len])
        for b, n in enumerate(case.lens()):
            mean = case.v[b, :n].double().mean(0)
            assert float(((o.view(B, Tq, H, 64)[b].cpu().double() - mean).abs() - (2 * an.EPS_BF + n * an.EPS_F32) * case.v[b, :n].double().abs().mean(0)).max()) <= 0
    dq, dk, dv = ops().attention_bwd(c.q, c.k, c.v, o, lse, d_o.to(DEV), kv_len, case.causal, o_lo=o_lo)
    tq, tk, tv = an.bwd_bounds(ref)
    m = [_check(n, g, ref[n], t) for n, g, t in (("dq", dq, tq), ("dk", dk, tk), ("dv", dv, tv))]
    for b, n in enumerate(case.lens()):  # a key masked for every query gets exactly zero gradients
        if n < Tk:
            assert int(torch.count_nonzero(dk[b, n:])) == 0 and int(torch.count_nonzero(dv[b, n:])) == 0, b
    print(f"{_id(spec)} path {path}: max err / bound  o {mo:.2g}  lse {ml:.2g}  dq {m[0]:.2g}  dk {m[1]:.2g}  dv {m[2]:.2g}")


@pytest.mark.parametrize("path", [1, 0], ids=["pingpong", "general"])
def test_one_hot_row_passes_its_output_gradient_to_the_peak(path, set_path):
    """dO nonzero in one query row only: dV[peak] = P dO = dO (P = 1 to 1e-15, exact in bf16), every other key's dV ~ e^-40."""
    set_path(path)
    B, H, Tq, Tk = 2, 6, 448, 1500
    case = an.to_device(an.make("onehot", B, H, Tq, Tk, seed=9), DEV)
    o, lse, o_lo = ops().attention_fwd(case.q, case.k, case.v, None, False, want_o_lo=True)
    d_o = torch.zeros(B, Tq, H * 64, dtype=BF, device=DEV)
    d_o[:, 131] = _d_o(B, 1, H, seed=5)[:, 0].to(DEV)
    dq, dk, dv = ops().attention_bwd(case.q, case.k, case.v, o, lse, d_o, None, False, o_lo=o_lo)
    dov = d_o.view(B, Tq, H, 64)[:, 131].float()
    for b in range(B):
        for h in range(H):
            pk = int(case.peak[b, h])
            got = dv[b, pk, h].float()
            assert float((got - dov[b, h]).abs().max()) <= an.EPS_BF * float(dov[b, h].abs().max()), (b, h, pk)
            rest = torch.cat([dv[b, :pk, h], dv[b, pk + 1:, h]]).float()
            assert float(rest.abs().max()) < 1e-15


# ---- chunked token rows ----------------------------------------------------------------------------------------------------
def _placement(B, n_chunks, seed):
    g = torch.Generator().manual_seed(seed)
    pairs = [(b, c) for b in range(B) for c in range(n_chunks)]
    order = [pairs[i] for i in torch.randperm(len(pairs), generator=g).tolist()]
    return ops().chunk_rows_table(order, B, n_chunks)


@pytest.mark.parametrize("spec,path", [pytest.param(("masked", 3, 6, 448, 448, True, (7, 220, 448)), 1, id="masked-decoder-self"),
                                       pytest.param(("onehot", 2, 6, 448, 1500, False, None), 1, id="onehot-cross-pingpong"),
                                       pytest.param(("onehot", 2, 6, 448, 1500, False, None), 0, id="onehot-cross-general")])
def test_attention_on_chunked_rows_with_a_span(spec, path, set_path):
    """attention_fwd_rows / attention_bwd_rows (q_rows, k_rows for the decoder's self-attention, q_span): the same bounds on the rows
    inside the span; d_o and o past the span hold NaN in the chunked buffers and must not be read."""
    set_path(path)
    o_ = ops()
    sc, B, H, Tq, Tk, causal, kv_len = spec
    span = [64, 256, 448][:B]
    case = an.make(sc, B, H, Tq, Tk, causal=causal, kv_len=list(kv_len) if kv_len else None, seed=B * 100 + H)
    d_o = _d_o(B, Tq, H, seed=Tq + Tk)
    keep = torch.arange(Tq)[None, :, None] < torch.tensor(span)[:, None, None]
    ref = an.reference(case, torch.where(keep, d_o, torch.zeros_like(d_o)))
    tab = _placement(B, Tq // 64, 11)
    tab_d = tab.to(DEV)
    d = H * 64
    c = an.to_device(case, DEV)
    kv = case.kv_len_tensor(DEV)
    if causal:
        qkv = (c.q._base if c.q._base is not None else c.q)
        qkv_c = o_.to_chunked(qkv, tab)
        qc, kc, vc = (qkv_c[:, i * d:(i + 1) * d].unflatten(1, (H, 64)) for i in range(3))
        k_rows = tab_d
    else:
        qc = o_.to_chunked(c.q.reshape(B, Tq, d).contiguous(), tab).unflatten(1, (H, 64))
        kc, vc, k_rows = c.k, c.v, None
    oc, lse, olo_c = o_.attention_fwd_rows(qc, kc, vc, B, H, Tq, Tk, tab_d, k_rows, kv, causal, want_o_lo=True)
    tol_o, tol_lse = an.fwd_bounds(case, ref)
    _check("o (rows)", o_.from_chunked(oc, tab, B, Tq).view(B, Tq, H, 64), ref["o"], tol_o)
    _check("lse (rows)", lse, ref["lse"], tol_lse)
    nan = float("nan")
    keep_d = keep.to(DEV)
    doc = o_.to_chunked(torch.where(keep_d, d_o.to(DEV), torch.full((B, Tq, d), nan, dtype=BF, device=DEV)), tab)
    o_plain = o_.from_chunked(oc, tab, B, Tq)
    olo_plain = o_.from_chunked(olo_c, tab, B, Tq)
    oc_p = o_.to_chunked(torch.where(keep_d, o_plain, torch.full_like(o_plain, nan)), tab)
    olo_p = o_.to_chunked(torch.where(keep_d, olo_plain, torch.full_like(olo_plain, nan)), tab)
    span_d = torch.tensor(span, dtype=torch.int32, device=DEV)
    dqc, dkc, dvc = o_.attention_bwd_rows(qc, kc, vc, oc_p, lse, doc, B, H, Tq, Tk, tab_d, k_rows, span_d, kv, causal, o_lo=olo_p)
    tq, tk, tv = an.bwd_bounds(ref)
    dq = o_.from_chunked(dqc.reshape(B * Tq, d), tab, B, Tq).view(B, Tq, H, 64)
    if causal:
        dk = o_.from_chunked(dkc.reshape(B * Tq, d), tab, B, Tq).view(B, Tq, H, 64)
        dv = o_.from_chunked(dvc.reshape(B * Tq, d), tab, B, Tq).view(B, Tq, H, 64)
    else:
        dk, dv = dkc, dvc
    for b, n in enumerate(span):
        _check(f"dq[{b}] (rows)", dq[b, :n], ref["dq"][b, :n], tq[b, :n])
        nk = n if causal else Tk  # chunked key rows past the span are not written
        _check(f"dk[{b}] (rows)", dk[b, :nk], ref["dk"][b, :nk], tk[b, :nk])
        _check(f"dv[{b}] (rows)", dv[b, :nk], ref["dv"][b, :nk], tv[b, :nk])


# ---- the Tq = 1 decode-step kernel -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kv", [False, True], ids=["full", "kv_len"])
@pytest.mark.parametrize("Tk", [1, 63, 64, 65, 448, 1500])
def test_decode_step_kernel_on_planted_scores(Tk, kv):
    B, H = 3, 6
    kv_len = [Tk, max(1, Tk // 2), max(1, Tk - 3)] if kv else None
    report = []
    for sc in an.SCENARIOS:
        if (sc == "masked" and not kv) or (sc == "plateau" and Tk < an.STEP0 + 64):
            continue
        case = an.make(sc, B, H, 1, Tk, kv_len=kv_len, seed=Tk)
        ref = an.reference(case)
        c = an.to_device(case, DEV)
        o, lse = ops().attention_fwd(c.q, c.k, c.v, case.kv_len_tensor(DEV), False)
        tol_o, tol_lse = an.fwd_bounds(case, ref)
        mo = _check(f"{sc} o", o.view(B, 1, H, 64), ref["o"], tol_o)
        ml = _check(f"{sc} lse", lse, ref["lse"], tol_lse)
        report.append(f"{sc} {mo:.2g}/{ml:.2g}")
    print(f"decode Tk={Tk} kv={kv}: " + ", ".join(report))


# ---- oasr_attention_scores ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("spec", [("masked", 3, 6, 448, 448, True, (7, 220, 448)), ("masked", 2, 20, 7, 1500, False, (1000, 1437)),
                                  ("onehot", 2, 1, 65, 1500, False, (1200, 1500)), ("plateau", 1, 6, 64, 1024, False, None)],
                         ids=lambda s: _id(s))
def test_attention_scores_are_the_planted_scores(spec, dtype):
    """Noise channels zeroed: every visible score is exactly r_i t_j (exact in fp32), every masked one exactly -inf."""
    sc, B, H, Tq, Tk, causal, kv_len = spec
    case = an.make(sc, B, H, Tq, Tk, causal=causal, kv_len=list(kv_len) if kv_len else None, seed=3, noise=False)
    c = an.to_device(case, DEV)
    q, k = (c.q, c.k) if dtype == BF else (c.q.float(), c.k.float())
    got = ops().attention_scores(q, k, case.kv_len_tensor(DEV), causal).cpu().double()
    want = case.r[..., :, None] * case.t[..., None, :]
    mask = torch.zeros(B, 1, Tq, Tk, dtype=torch.bool)
    if causal:
        mask |= torch.ones(Tq, Tk, dtype=torch.bool).triu(1)
    if kv_len:
        mask |= torch.arange(Tk)[None, None, None, :] >= torch.tensor(kv_len)[:, None, None, None]
    mask = mask.expand(B, H, Tq, Tk)
    assert bool((got[mask] == -math.inf).all())
    assert torch.equal(got[~mask], want[~mask])
