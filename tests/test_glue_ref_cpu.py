"""CPU power test of tests/glue_ref.py: at the shapes and plants tests/test_gpu_glue_ops.py runs on the GPU, the checkers accept the
reference -- cross-checked here against a second, vectorised evaluation of the same definition -- and reject every flawed stand-in of
``glue_ref.FLAWS``; the exactness claims of the plants (bf16-representable operands, partial sums below 2^24, fold / 2 representable) are
asserted where the plants are built.  Also the CPU-side measurements the GPU tests lean on: the share of not-correctly-rounded products of
a torch fp32 exact-erf GELU' (the yardstick of the 2 x rule), and the LayerNorm forward rule against fp32 evaluations.

LayerNorm forward rule, measured here (worst |err| / rule over every shape and input kind): a two-pass fp32 torch evaluation 0.50 (the
bf16 rounding itself); this torch build's fp32 ``F.layer_norm`` 0.50 as well, 0.18 of the rule's second term alone on unrounded
``100 + 0.05 noise`` rows with an fp32 output.  The rule comes from the fp32 rounding of a mean of up to 2048 values, not from either
evaluation: do not re-derive it from ``F.layer_norm``, whose algorithm (and error on offset rows) is the torch build's business.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_exact as ge  # noqa: E402
import glue_ref as gr  # noqa: E402

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def rejects(name, got, want):
    with pytest.raises(AssertionError):
        gr.check_exact(name, got, want)


# ---- embedding -------------------------------------------------------------------------------------------------------------------------
def _emb_tables(seed=4):
    p = gr.EMB
    g = torch.Generator().manual_seed(seed)
    return torch.randn(p["n_embed"], p["d"], generator=g), torch.randn(p["S"], p["d"], generator=g)


@pytest.mark.parametrize("with_tab", [False, True])
def test_embedding_fwd_checker(with_tab):
    p = gr.EMB
    tok = gr.embedding_tokens()
    assert {0, 96, -1, 97} <= set(tok.flatten().tolist()) and p["pad_id"] == 96
    E, pos = _emb_tables()
    tab, n_rows = gr.permuted_rowtab(p["B"], p["S"]) if with_tab else (None, p["B"] * p["S"])
    want, written = gr.embedding_fwd_ref(tok, E, pos, BF, tab, n_rows)
    assert int(written.sum()) == p["B"] * p["S"] and (not with_tab or int((~written).sum()) >= 64)
    # second evaluation: gather with a zero row appended for the ids outside the table
    Ez = torch.cat([E, torch.zeros(1, p["d"])])
    t = torch.where((tok >= 0) & (tok < p["n_embed"]), tok, torch.full_like(tok, p["n_embed"]))
    x2 = (Ez[t] + pos[None]).to(BF)
    for b in range(p["B"]):
        for s in (0, 63, 64, 127):
            assert torch.equal(want[gr.row_of(tab, b, s, p["S"])], x2[b, s])
    oob = ((tok < 0) | (tok >= p["n_embed"])).nonzero()
    assert len(oob) >= 4
    for b, s in oob.tolist():
        assert torch.equal(want[gr.row_of(tab, b, s, p["S"])], pos[s].to(BF))  # ids outside the table: bf16(pos[s])
    gr.check_exact("reference", want, want.clone())
    for flaw in gr.FLAWS["embedding_fwd"]:
        if flaw == "rowtab_ignored" and not with_tab:
            continue
        got, _ = gr.embedding_fwd_ref(tok, E, pos, BF, tab, n_rows, flaw=flaw)
        rejects(flaw, got, want)


@pytest.mark.parametrize("variant", ["plain", "tab", "tab_span"])
def test_embedding_bwd_checker(variant):
    p = gr.EMB
    tok = gr.embedding_tokens()
    tab, n_rows = gr.permuted_rowtab(p["B"], p["S"]) if variant != "plain" else (None, p["B"] * p["S"])
    span = torch.tensor([0, 64, 128, 64, 128], dtype=torch.int32) if variant == "tab_span" else None
    dx, dE0, dpos0 = gr.embedding_bwd_plants(tok, tab, n_rows, span)
    dE, dpos = gr.embedding_bwd_ref(tok, dx, dE0, dpos0, p["pad_id"], tab, span)
    assert not torch.isnan(dE).any() and not torch.isnan(dpos).any()
    # second evaluation: index_add_ over the live (b, s) pairs
    live = torch.ones(p["B"], p["S"], dtype=torch.bool) if span is None else torch.arange(p["S"])[None, :] < span[:, None]
    rows = torch.tensor([[gr.row_of(tab, b, s, p["S"]) for s in range(p["S"])] for b in range(p["B"])])
    vals = torch.where(live[..., None], dx[rows.clamp(max=n_rows - 1)], torch.zeros((), dtype=F64))
    scat = live & (tok != p["pad_id"]) & (tok >= 0) & (tok < p["n_embed"])
    dE2 = dE0.clone().index_add_(0, tok[scat], vals[scat])
    assert torch.equal(dE, dE2) and torch.equal(dpos, dpos0 + vals.sum(0))
    # rows of the pad id and of ids nothing scatters to are unchanged
    assert torch.equal(dE[p["pad_id"]], dE0[p["pad_id"]])
    assert float(dE.abs().max()) < 2 ** 24 and bool((dE == dE.round()).all())
    for flaw in gr.FLAWS["embedding_bwd"]:
        if flaw == "span_ignored" and span is None:
            continue
        fE, fpos = gr.embedding_bwd_ref(tok, dx, dE0, dpos0, p["pad_id"], tab, span, flaw=flaw)
        with pytest.raises(AssertionError):
            gr.check_exact(flaw, fE.to(F32), dE.to(F32))
            gr.check_exact(flaw, fpos.to(F32), dpos.to(F32))


# ---- column sum ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,ncols,ld", gr.COLSUM_SHAPES)
def test_colsum_checker(M, ncols, ld):
    x, pre = gr.colsum_plants(M, ncols, ld)
    assert torch.isnan(x[:, ncols:]).all() and torch.isnan(x[M:]).all()
    want = gr.colsum_ref(x, M, ncols, pre)
    assert torch.equal(want, pre + x[:M, :ncols].sum(0))
    if M > 12288:  # the launcher's grid: 1024 row groups of 4 -> the 4-way unrolled body runs once, then the remainder loop
        gx = -(-ncols // 512)
        gy = min(2048 // gx, (M + 3) // 4)
        assert gx == 2 and gy == 1024 and M > 3 * 4 * gy and M % (16 * gy) != 0 and ncols - 512 == 8
    for flaw in gr.FLAWS["colsum"]:
        got = gr.colsum_ref(x, M, ncols, pre, flaw=flaw)
        applies = {"rows_past_m": M % 4 != 0, "remainder_rows_dropped": M > 16384, "last_column_block_dropped": ncols > 512}[flaw]
        if applies:
            rejects(flaw, got.to(F32), want.to(F32))


# ---- conv2 fold + GELU' ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T1,d", gr.CONV2_SHAPES)
def test_conv2_fold_checker(B, T1, d):
    dA = gr.conv2_plants(B, T1, d)
    T2 = T1 // 2
    fold = gr.conv2_fold_ref(dA, B, T1, d)
    # second evaluation: conv_transpose1d with a one-hot kernel is the fold (stride 2, padding 1, kernel 3; output length 2 T2 - 1 + pad row)
    cols = dA[:B * T2].view(B, T2, 3, d).permute(0, 3, 2, 1).reshape(B * d, 3, T2)  # [B*d, kk, t']
    full = torch.zeros(B * d, 2 * T2 + 1, dtype=F64)
    for kk in range(3):
        full[:, kk:kk + 2 * T2:2] += cols[:, kk]
    assert torch.equal(fold, full[:, 1:1 + T1].view(B, d, T1).transpose(1, 2))
    # (a) u = 0: every output is bf16(fold / 2) exactly
    half = fold / 2
    assert gr.is_bf16(half) and gr.is_bf16(fold) and float(fold.abs().max()) <= 508
    if T1 == 6:  # every boundary row by name
        h = gr.conv2_half_codes(B, T2, d)
        for b in range(B):
            assert torch.equal(fold[b, 0], 2 * h[b, 0, 1]) and torch.equal(fold[b, 5], 2 * h[b, 2, 2])
            assert torch.equal(fold[b, 1], 2 * (h[b, 0, 2] + h[b, 1, 0])) and torch.equal(fold[b, 4], 2 * h[b, 2, 1])
    want = half.to(BF)
    for flaw in gr.FLAWS["conv2"]:
        got = (gr.conv2_fold_ref(dA, B, T1, d, flaw=flaw) / 2).to(BF)
        with pytest.raises(AssertionError) as e:
            gr.check_exact(flaw, got, want, where=lambda i: f"(b={i[0]}, t={i[1]}, column={i[2]})", code=gr.conv2_code(B, T1, d))
        assert "taps (t'=" in str(e.value) and "(b=" in str(e.value)


def test_dgelu_rule_and_the_torch_fp32_share():
    """(b): the one-ulp rule accepts a torch fp32 exact-erf evaluation and a correctly rounded one, rejects a two-ulp error; the share of
    not-correctly-rounded outputs of the torch fp32 evaluation is the yardstick the GPU test doubles."""
    B, T1, d = gr.CONV2_SHAPES[1]
    fold = gr.conv2_fold_ref(gr.conv2_plants(B, T1, d), B, T1, d).to(BF)
    u = ((torch.rand(B, T1, d, generator=torch.Generator().manual_seed(9), dtype=F64) * 12 - 6)).to(BF)
    want = fold.to(F64) * ge.dgelu64(u.to(F64))
    assert gr.dgelu_stats(want.to(BF), fold, u, "correctly rounded", BF) == 0.0
    share = gr.torch_fp32_dgelu_share(fold, u)
    print(f"torch fp32 exact-erf GELU' x fold: {share:.4%} of {fold.numel()} outputs are not the correctly rounded bf16 value")
    assert 0.0 < share < 0.2  # (the cancellation of 1 + erf(u / sqrt 2) in the negative tail)
    assert gr.share_allowed(2 * share, share, fold.numel()) and not gr.share_allowed(2.1 * share, share, fold.numel())
    assert gr.share_allowed(4 / 1000, 0.0, 1000) and not gr.share_allowed(5 / 1000, 0.0, 1000)
    off = (want.to(BF).to(F64) + 2.5 * ge.bf16_ulp(want) * (want != 0)).to(BF)
    with pytest.raises(AssertionError):
        gr.dgelu_stats(off, fold, u, "two ulps off", BF)
    # fp32: a float64 evaluation rounded once passes; an error of 2^-20 of the larger term does not
    uf = (torch.rand(4096, generator=torch.Generator().manual_seed(10), dtype=F64) * 12 - 6).to(F32)
    ff = torch.randint(-500, 501, (4096,), generator=torch.Generator().manual_seed(11)).to(F32)
    w32 = (ff.to(F64) * ge.dgelu64(uf.to(F64)))
    assert gr.dgelu_stats(w32.to(F32), ff, uf, "fp32 rounded once", F32) == 0.0
    with pytest.raises(AssertionError):
        gr.dgelu_stats((w32 * (1 + 2.0 ** -18)).to(F32), ff, uf, "fp32 2^-18 off", F32)


# ---- conv1 fold ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nm", gr.CONV1_NM)
@pytest.mark.parametrize("T1", gr.CONV1_T)
def test_conv1_fold_checker(T1, nm):
    B = 3
    dcol = gr.conv1_plants(B, T1, nm)
    assert torch.isnan(dcol[:, 3 * nm:]).all()
    want = gr.conv1_fold_ref(dcol, B, T1, nm)
    # second evaluation: three shifted slices per sample
    v = dcol[:, :3 * nm].view(B, T1, 3, nm)
    full = torch.zeros(B, T1 + 2, nm, dtype=F64)
    for k in range(3):
        full[:, k:k + T1] += v[:, :, k]
    assert torch.equal(want, full[:, 1:1 + T1].transpose(1, 2))
    assert float(want.abs().max()) <= 3 * 127
    prefill = 777.0
    for flaw in gr.FLAWS["conv1"]:
        applies = {"tap_from_neighbouring_sample": True, "halo_row_dropped": T1 > 32, "rotated_slot_read_unrotated": 3 * nm > 32,
                   "partial_tile_unwritten": T1 % 32 != 0}[flaw]
        if applies:
            got = gr.conv1_fold_ref(dcol, B, T1, nm, flaw=flaw, prefill=prefill)
            rejects(flaw, got.to(F32), want.to(F32))


# ---- mel transpose, packs, casts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,T", [(80, 33), (128, 64), (80, 3000)])
def test_mel_reference_and_flaws(C, T):
    mel, clip_max = gr.mel_plants(2, C, T)
    for dtype in (BF, F32):
        want = gr.mel_ref(mel, clip_max, dtype)
        assert want.shape == (2, T, C)
        b, t, c = 1, T - 1, C - 1
        assert want[b, t, c] == ((max(mel[b, c, t], clip_max[b] - 8.0) + 4.0) * 0.25).to(dtype)
        assert torch.equal(gr.mel_ref(mel, None, dtype)[0, 5, 3], mel[0, 3, 5].to(dtype))
        for flaw in gr.FLAWS["mel"]:
            if flaw == "tail_tile_zero" and T % 32 == 0:
                continue
            rejects(flaw, gr.mel_ref(mel, clip_max, dtype, flaw=flaw), want)


@pytest.mark.parametrize("co,ci,ldk", gr.PACK_CONV_SHAPES)
def test_pack_conv_checkers(co, ci, ldk):
    g = torch.Generator().manual_seed(12)
    w = torch.randn(co, ci, 3, generator=g)
    want = gr.pack_conv_ref(w, ldk, BF)
    assert want[co - 1, 2 * ci + 3] == w[co - 1, 3, 2].to(BF) and bool((want[:, 3 * ci:] == 0).all())
    for flaw in gr.FLAWS["pack_conv"]:
        if flaw == "pad_not_zeroed" and ldk == 3 * ci:
            continue
        rejects(flaw, gr.pack_conv_ref(w, ldk, BF, flaw=flaw), want)
    grad = torch.randint(-9, 10, (co, ldk), generator=g).to(F32)
    dw0 = torch.randint(-9, 10, (co, ci, 3), generator=g).to(F32)
    dw = gr.unpack_conv_ref(grad, dw0, ci)
    assert dw[1, 2, 1] == dw0[1, 2, 1] + grad[1, ci + 2]
    rejects("overwrites", gr.unpack_conv_ref(grad, dw0, ci, flaw="overwrites"), dw)


def test_cast_reference_is_round_to_nearest_even():
    n = 8 * 300 + 5
    x = gr.cast_values(n)
    want = gr.cast_ref(x)
    assert gr.cast_equal(x.to(BF), want)  # torch's own conversion agrees with the integer arithmetic
    f = want.to(F32)
    assert f[5] == 1.0 and f[6] == 1.015625 and f[7] == -1.0 and f[8] == -1.015625  # ties to even, both ways
    assert f[9] != 0 and abs(float(f[9])) < 1.2e-38  # the denormal stays a denormal
    assert torch.isinf(f[11]) and torch.isinf(f[12]) and torch.isnan(f[13]) and torch.isfinite(f[14]) and torch.isinf(f[15])
    assert bool((x[n - 5:] == x[n - 5:]).sum() >= 3)
    assert not gr.cast_equal(ge.trunc_bf16(torch.where(torch.isfinite(x), x, torch.zeros_like(x))), want)


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", gr.LN_KINDS)
def test_layernorm_forward_rule_against_fp32_evaluations(kind):
    worst = {}
    for rows, d in gr.LN_SHAPES:
        x, gamma, beta = gr.ln_inputs(rows, d, kind)
        y, mu, rs = gr.ln_fwd_ref(x, gamma, beta)
        tol = gr.ln_fwd_tol(x, gamma, y, rs)
        two = gr.ln_fwd_fp32_two_pass(x, gamma, beta)
        lib = F.layer_norm(x.to(F32), (d,), gamma, beta, 1e-5).to(BF)
        worst[(rows, d)] = (float(((two.to(F64) - y).abs() / tol).max()), float(((lib.to(F64) - y).abs() / tol).max()))
        assert worst[(rows, d)][0] <= 1.0, (kind, rows, d, worst)
        if kind == "constant":
            assert torch.equal(two, beta.to(BF).expand(rows, d)) and bool(((rs - 1e-5 ** -0.5).abs() <= 1e-9).all())
    print(f"LayerNorm forward, {kind}: worst |err| / rule (fp32 two-pass, fp32 F.layer_norm) = {worst}")


def test_layernorm_backward_checkers_reject_the_flaws():
    rows, d = 37, 512
    x, gamma, beta = gr.ln_inputs(rows, d, "random")
    _, mu, rs = gr.ln_fwd_ref(x, gamma, beta)
    mean, rstd = mu.to(F32), rs.to(F32)
    g = torch.Generator().manual_seed(13)
    dy = torch.randn(rows, d, generator=g).to(BF)
    dres = torch.randn(rows, d, generator=g).to(BF)
    for res in (None, dres):
        dx_ref, dg_ref, db_ref, tol, xh = gr.ln_bwd_ref(dy, x, gamma, mean, rstd, res)
        dx, dg, db, ds = gr.ln_bwd_emulate(dy, x, gamma, mean, rstd, res)
        assert bool(((dx.to(F64) - dx_ref).abs() <= tol).all())
        pre = gr.ln_dsum_prefill(dx_ref)
        assert bool((pre != 0).all())
        assert len(gr.ln_dsum_ok(ds + pre, pre, dx)) == 0
        for flaw in gr.FLAWS["layernorm_bwd"]:
            _, fg, fb, fs = gr.ln_bwd_emulate(dy, x, gamma, mean, rstd, res, flaw=flaw)
            assert len(gr.ln_dsum_ok(fs + pre, pre, dx)) > 0, flaw
    # needle rows: a dropped or doubled row cannot hide
    for r in (0, rows - 1):
        nd = torch.zeros_like(dy)
        nd[r] = dy[r]
        _, dg_ref, db_ref, _, xh = gr.ln_bwd_ref(nd, x, gamma, mean, rstd)
        assert torch.equal(dg_ref, nd[r].to(F64) * xh[r]) and torch.equal(db_ref, nd[r].to(F64))
        for flaw, caught in (("last_row_dropped", r == rows - 1), ("dead_second_row_counted", r == rows - 1), (None, False)):
            _, fg, fb, _ = gr.ln_bwd_emulate(nd, x, gamma, mean, rstd, flaw=flaw)
            bad = bool(((fg.to(F64) - dg_ref).abs() > 4 * gr.E24 * dg_ref.abs()).any()) or bool(((fb.to(F64) - db_ref).abs() > 4 * gr.E24 * db_ref.abs()).any())
            assert bad == caught, (r, flaw)


def test_guard_helper_sees_a_write_past_the_end():
    g, t = gr.guarded(torch.zeros(3, 8, dtype=F32))
    assert t.shape == (3, 8) and t.data_ptr() % 16 == 0
    g.check("untouched")
    g.buf[0, ge.COL0 + 24] = 0.0
    with pytest.raises(AssertionError):
        g.check("one element past the end")
