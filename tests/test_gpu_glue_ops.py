"""Operator-level tests of the glue kernels on the GPU: embedding gather / scatter, the column sum, the two conv folds, the mel transpose,
the packs and casts, and LayerNorm with its column sums -- each through its ``oasr_test_*`` unit operator (include/oasr_testing.h), against
the plain references of tests/glue_ref.py.

Common to every case (tests/glue_ref.py has the reasoning): outputs sit between guard bands that must come back bit-identical, accumulated
outputs start from a non-zero pre-fill, everything the contract says is not read holds NaN, and wherever the operation is a sum the plants
are small integers, so that the comparison is bit for bit.  tests/test_glue_ref_cpu.py shows that the same checkers reject a kernel with a
tap from the neighbouring sample, a scattered pad id, a row past M and the other flaws of ``glue_ref.FLAWS``.

Measured on an MI355X (printed by the tests):
  conv2 fold x GELU'(u), u in [-6, 6], bf16 [3 x 3000 x 512]: 0.267 % of the outputs are not the correctly rounded product, against 6.62 % for a
  torch fp32 exact-erf evaluation of the same inputs (1 + erf cancels in the negative tail); the rule allows twice the latter.  dgelu_mul:
  0.259 % against 6.55 %.
  LayerNorm: worst |err| / rule 0.500 forward and backward (the bf16 rounding itself), every shape, input kind and instantiation.
  The fp32 validation GELU' used 0.5 (1 + erf(u / sqrt 2)) and missed the 4 * 2^-24 rule on 24 % of the outputs (all of Phi's digits are gone by
  u = -5.5); it now takes Phi from erfc on the negative side and passes.
"""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_exact as ge  # noqa: E402
import glue_ref as gr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DTYPES = [pytest.param(BF, id="bf16"), pytest.param(F32, id="fp32")]


@pytest.fixture(scope="module")
def ops():
    from olmoasr_amd import ops as o
    return o


def out_buf(prefill, dtype=None):
    """An output allocation between guard bands whose logical region holds ``prefill`` (a CPU tensor), or the sentinel when prefill is a shape."""
    if isinstance(prefill, (tuple, list, torch.Size)):
        g, t = gr.guarded(torch.zeros(tuple(prefill), dtype=dtype), device=DEV)
        t.view(torch.int16 if dtype == BF else torch.int32).fill_(ge.SENTINEL_BF16 if dtype == BF else ge.SENTINEL_F32)
        return g, t
    return gr.guarded(prefill, device=DEV)


def in_buf(t, dtype=None):
    """An input allocation followed and preceded by NaN."""
    return gr.guarded(t if dtype is None else t.to(dtype), fill="nan", device=DEV)[1]


def is_sentinel(t):
    return gr.bits(t) == (ge.SENTINEL_BF16 if t.dtype == BF else ge.SENTINEL_F32)


def span_tables(span, S):
    """The chunk-row table of oasr_test_span_tables for the given spans (CPU int32 [B, ROWTAB])."""
    from olmoasr_amd import _native as N
    B = len(span)
    sp = torch.tensor(span, dtype=torch.int32)
    tg = torch.zeros(B, S, dtype=torch.int64, device=DEV)
    rows = torch.full((B, gr.ROWTAB), -1, dtype=torch.int32, device=DEV)
    span_d = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    tphys = torch.zeros(B * S, dtype=torch.int64, device=DEV)
    act = C.c_int64(0)
    N.check(N.lib().oasr_test_span_tables(C.c_void_p(sp.data_ptr()), B, S, N.ptr(tg), N.ptr(rows), N.ptr(span_d), N.ptr(tphys), C.byref(act),
                                          N.stream_ptr()), "oasr_test_span_tables")
    torch.cuda.synchronize()
    return rows.cpu(), span_d.cpu()


SPANS = [0, 64, 128, 64, 128]


def _tab(kind):
    p = gr.EMB
    if kind == "plain":
        return None, p["B"] * p["S"]
    if kind == "sparse":  # 1.5 x as many 64-row slots as chunks, the chunks scattered over them
        return gr.permuted_rowtab(p["B"], p["S"])
    tab, _ = span_tables(SPANS, p["S"])  # the engine's own table: active chunks first, position-block-major
    return tab, p["B"] * p["S"] + 64


# ---- embedding ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tabkind", ["plain", "span_tables", "sparse"])
def test_embedding_fwd(ops, dtype, tabkind):
    p = gr.EMB
    tok = gr.embedding_tokens()
    g = torch.Generator().manual_seed(4)
    E, pos = torch.randn(p["n_embed"], p["d"], generator=g), torch.randn(p["S"], p["d"], generator=g)
    tab, n_rows = _tab(tabkind)
    if tab is not None:
        live = tab[:, :p["S"] // 64].flatten().tolist()
        assert len(set(live)) == len(live) and max(live) + 64 <= n_rows and min(live) >= 0  # every store stays inside the allocation
    want, written = gr.embedding_fwd_ref(tok, E, pos, dtype, tab, n_rows)
    xg, x = out_buf((n_rows, p["d"]), dtype)
    ops.embedding_fwd_(tok.to(DEV), in_buf(E), in_buf(pos), x, p["n_embed"], None if tab is None else tab.to(DEV))
    torch.cuda.synchronize()
    got = x.cpu()
    gr.check_exact("x", got[written], want[written], where=lambda i: f"(written row {i[0]}, column {i[1]})")
    assert bool(is_sentinel(got[~written]).all()), "rows no chunk maps to were written"
    assert tab is None or int((~written).sum()) >= 64
    xg.check("x")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", ["plain", "tab", "tab_span", "dE_null", "dpos_null"])
def test_embedding_bwd(ops, dtype, variant):
    p = gr.EMB
    tok = gr.embedding_tokens()
    tab, n_rows = _tab("plain" if variant in ("plain", "dE_null", "dpos_null") else ("sparse" if variant == "tab" else "span_tables"))
    span = None
    if variant == "tab_span":
        span = torch.tensor(SPANS, dtype=torch.int32)
        assert sorted(set(SPANS)) == [0, 64, 128]
    dx, dE0, dpos0 = gr.embedding_bwd_plants(tok, tab, n_rows, span)
    dE_want, dpos_want = gr.embedding_bwd_ref(tok, dx, dE0, dpos0, p["pad_id"], tab, span)
    assert span is None or int(torch.isnan(dx).any(1).sum()) >= 64 + 128 + 64  # every dx row at s >= span[b] is NaN
    Eg, dE = out_buf(dE0.to(F32))
    Pg, dpos = out_buf(dpos0.to(F32))
    ops.embedding_bwd_(tok.to(DEV), in_buf(dx, dtype), None if variant == "dE_null" else dE, None if variant == "dpos_null" else dpos, p["pad_id"],
                       p["n_embed"], p["d"], None if tab is None else tab.to(DEV), None if span is None else span.to(DEV))
    torch.cuda.synchronize()

    def where_E(i):
        hits = (tok == i[0]).nonzero().tolist()
        return f"(token {i[0]}, column {i[1]}); the token sits at (b, s) = {hits[:6]}"
    gr.check_exact("dE", dE.cpu(), (dE0 if variant == "dE_null" else dE_want).to(F32), where=where_E)
    gr.check_exact("dpos", dpos.cpu(), (dpos0 if variant == "dpos_null" else dpos_want).to(F32),
                   where=lambda i: f"(s={i[0]}, column {i[1]}); tokens {tok[:, i[0]].tolist()}")
    assert torch.equal(dE.cpu()[p["pad_id"]], dE0[p["pad_id"]].to(F32)), "the pad id's row changed"
    Eg.check("dE")
    Pg.check("dpos")


# ---- column sum -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,ncols,ld", gr.COLSUM_SHAPES)
def test_colsum(ops, dtype, M, ncols, ld):
    x, pre = gr.colsum_plants(M, ncols, ld)
    want = gr.colsum_ref(x, M, ncols, pre)
    og, out = out_buf(pre.to(F32))
    ops.colsum_(in_buf(x, dtype), ld, M, ncols, out)
    torch.cuda.synchronize()
    gr.check_exact("colsum", out.cpu(), want.to(F32), where=lambda i: f"(column {i[0]})", code=lambda i: f"pre-fill {pre[i[0]].item()}")
    og.check("colsum")


# ---- conv2 fold + GELU' ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T1,d", gr.CONV2_SHAPES)
def test_conv2_fold_at_u_zero_is_exact(ops, dtype, B, T1, d):
    """(a) GELU'(0) = 1/2 to within the kernel's 1.5e-7 erf error, far inside half a bf16 ulp of values whose halves are representable."""
    dA = gr.conv2_plants(B, T1, d)
    fold = gr.conv2_fold_ref(dA, B, T1, d)
    og, out = out_buf((B, T1, d), dtype)
    ops.conv2_col2im_dgelu_(in_buf(dA, dtype), in_buf(torch.zeros(B, T1, d), dtype), out, B, T1, d)
    torch.cuda.synchronize()
    gr.check_exact("dpre1", out.cpu(), (fold / 2).to(dtype), where=lambda i: f"(b={i[0]}, t={i[1]}, column={i[2]})", code=gr.conv2_code(B, T1, d))
    og.check("dpre1")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T1,d", gr.CONV2_SHAPES)
def test_conv2_fold_times_dgelu(ops, dtype, B, T1, d):
    """(b) u random in [-6, 6]: the one-ulp rule (fp32: 4 * 2^-24 on the terms, glue_ref.dgelu_stats), and the share of outputs that are not the
    correctly rounded product at most twice that of a torch fp32 exact-erf evaluation of the same inputs."""
    dA = gr.conv2_plants(B, T1, d)
    fold = gr.conv2_fold_ref(dA, B, T1, d).to(dtype)  # (exact: |fold| <= 508 and even)
    u = (torch.rand(B, T1, d, generator=torch.Generator().manual_seed(9), dtype=F64) * 12 - 6).to(dtype)
    og, out = out_buf((B, T1, d), dtype)
    ops.conv2_col2im_dgelu_(in_buf(dA, dtype), in_buf(u), out, B, T1, d)
    torch.cuda.synchronize()
    share = gr.dgelu_stats(out.cpu(), fold, u, "dpre1", dtype)
    og.check("dpre1")
    if dtype == BF:
        ref_share = gr.torch_fp32_dgelu_share(fold, u)
        print(f"conv2 fold x GELU' [{B}x{T1}x{d}]: kernel {share:.4%} not correctly rounded, torch fp32 {ref_share:.4%}")
        assert gr.share_allowed(share, ref_share, out.numel()), (share, ref_share)


# ---- conv1 fold -> d(mel) -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nm", gr.CONV1_NM)
@pytest.mark.parametrize("T1", gr.CONV1_T)
def test_conv1_fold(ops, dtype, T1, nm):
    B = 3
    dcol = gr.conv1_plants(B, T1, nm)
    want = gr.conv1_fold_ref(dcol, B, T1, nm).to(F32)
    og, out = out_buf((B, nm, T1), F32)
    ops.conv1_col2im_mel_(in_buf(dcol, dtype), out, B, T1, nm)
    torch.cuda.synchronize()
    got = out.cpu()
    for b in range(B):  # the halo rows of every clip by name
        for t in (0, T1 - 1):
            gr.check_exact(f"d(mel): frame {t} of clip {b} (T1 = {T1})", got[b, :, t], want[b, :, t], where=lambda i: f"(channel {i[0]})")
    gr.check_exact("d(mel)", got, want, where=lambda i: f"(b={i[0]}, channel={i[1]}, t={i[2]})",
                   code=lambda i: "taps " + ", ".join(f"(t'={i[2] + 1 - k}, k={k}) = {dcol[i[0] * T1 + i[2] + 1 - k, k * nm + i[1]].item()}"
                                                      for k in range(3) if 0 <= i[2] + 1 - k < T1))
    og.check("d(mel)")


# ---- mel transpose --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("C_", [80, 128])
@pytest.mark.parametrize("T", [33, 64, 3000])
def test_mel_to_time_major(ops, dtype, clip, C_, T):
    B = 2
    mel, clip_max = gr.mel_plants(B, C_, T)
    want = gr.mel_ref(mel, clip_max if clip else None, dtype)
    og, out = out_buf((B, T, C_), dtype)
    ops.mel_to_time_major_(in_buf(mel), out, B, C_, T, in_buf(clip_max) if clip else None)
    torch.cuda.synchronize()
    gr.check_exact("mel", out.cpu(), want, where=lambda i: f"(b={i[0]}, t={i[1]}, channel={i[2]})",
                   code=lambda i: f"mel {mel[i[0], i[2], i[1]].item()!r}, floor {(clip_max[i[0]] - 8.0).item()!r}")
    og.check("mel")


# ---- packs and casts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("co,ci,ldk", gr.PACK_CONV_SHAPES)
def test_pack_conv_weight(ops, dtype, co, ci, ldk):
    w = torch.randn(co, ci, 3, generator=torch.Generator().manual_seed(12))
    og, out = out_buf((co, ldk), dtype)
    ops.pack_conv_weight_(in_buf(w), out, co, ci, ldk)
    torch.cuda.synchronize()
    got = out.cpu()
    gr.check_exact("packed conv weight", got, gr.pack_conv_ref(w, ldk, dtype), where=lambda i: f"(co={i[0]}, k={i[1]}: tap {i[1] // ci}, ci {i[1] % ci})")
    assert bool((gr.bits(got[:, 3 * ci:]) == 0).all()), "pad columns must be +0"
    og.check("packed conv weight")


@pytest.mark.parametrize("co,ci,ldk", gr.PACK_CONV_SHAPES)
def test_unpack_conv_grad(ops, co, ci, ldk):
    g = torch.Generator().manual_seed(12)
    grad = torch.full((co, ldk), float("nan"))
    grad[:, :3 * ci] = torch.randint(-9, 10, (co, 3 * ci), generator=g).to(F32)  # the pad columns are not read
    dw0 = torch.randint(-9, 10, (co, ci, 3), generator=g).to(F32)
    og, dw = out_buf(dw0)
    ops.unpack_conv_grad_(in_buf(grad), dw, co, ci, ldk)
    torch.cuda.synchronize()
    gr.check_exact("dw", dw.cpu(), gr.unpack_conv_ref(grad, dw0, ci), where=lambda i: f"(co={i[0]}, ci={i[1]}, tap={i[2]})")
    og.check("dw")


def test_pack_embedding(ops):
    rows, rows_pad, d = 51, 64, 24
    e = torch.randn(rows, d, generator=torch.Generator().manual_seed(14))
    og, out = out_buf((rows_pad, d), BF)
    ops.pack_embedding_(in_buf(e), out, rows, rows_pad, d)  # (rows past `rows` of e are NaN: they must not be read)
    torch.cuda.synchronize()
    got = out.cpu()
    gr.check_exact("packed embedding", got, gr.pack_embedding_ref(e, rows_pad), where=lambda i: f"(row {i[0]}, column {i[1]})")
    assert bool((gr.bits(got[rows:]) == 0).all())
    og.check("packed embedding")


@pytest.mark.parametrize("dtype", DTYPES)
def test_dgelu_mul(ops, dtype):
    n = 8 * 4099
    g = torch.Generator().manual_seed(15)
    dy = torch.randint(-254, 255, (n,), generator=g).to(dtype)
    u = (torch.rand(n, generator=g, dtype=F64) * 12 - 6).to(dtype)
    og, out = out_buf((n,), dtype)
    ops.dgelu_mul_(in_buf(dy), in_buf(u), out, n)
    torch.cuda.synchronize()
    share = gr.dgelu_stats(out.cpu(), dy, u, "dgelu_mul", dtype)
    og.check("dgelu_mul")
    if dtype == BF:
        ref_share = gr.torch_fp32_dgelu_share(dy, u)
        print(f"dgelu_mul: kernel {share:.4%} not correctly rounded, torch fp32 {ref_share:.4%}")
        assert gr.share_allowed(share, ref_share, n), (share, ref_share)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dlogits_and_logits_copies_past_the_grid_cap(ops, dtype):
    rows, V, ld = 70000, 13, 16  # 1,120,000 elements against 4096 workgroups x 256 lanes: the grid-stride loop turns over
    g = torch.Generator().manual_seed(16)
    src = torch.randn(rows, V, generator=g)
    og, dst = out_buf((rows, ld), dtype)
    ops.dlogits_from_f32_(in_buf(src), V, rows, ld, dst)
    torch.cuda.synchronize()
    want = torch.zeros(rows, ld, dtype=dtype)
    want[:, :V] = src.to(dtype)
    got = dst.cpu()
    gr.check_exact("dlogits", got, want, where=lambda i: f"(row {i[0]}, column {i[1]})")
    assert bool((gr.bits(got[:, V:]) == 0).all())
    og.check("dlogits")
    lg = torch.full((rows, ld), float("nan"))
    lg[:, :V] = torch.randn(rows, V, generator=g)
    lg = lg.to(dtype)
    og, out = out_buf((rows, V), F32)
    ops.logits_to_f32_(in_buf(lg), ld, rows, V, out)
    torch.cuda.synchronize()
    gr.check_exact("logits", out.cpu(), lg[:, :V].to(F32), where=lambda i: f"(row {i[0]}, column {i[1]})")
    og.check("logits")


def test_cast_f32_bf16(ops):
    from olmoasr_amd import _native as N
    n = 8 * 300 + 5
    x = gr.cast_values(n)
    og, out = out_buf((n,), BF)
    N.check(N.lib().oasr_cast_f32_bf16(N.ptr(in_buf(x)), N.ptr(out), n, N.stream_ptr()), "cast")
    torch.cuda.synchronize()
    got, want = out.cpu(), gr.cast_ref(x)
    if not gr.cast_equal(got, want):
        i = int(((gr.bits(got) != gr.bits(want)) & ~(torch.isnan(got) & torch.isnan(want))).nonzero()[0])
        raise AssertionError(f"cast: element {i}: {x[i].item()!r} -> {got[i].item()!r} (bits {int(gr.bits(got)[i]) & 0xFFFF:#06x}), want {want[i].item()!r}")
    og.check("cast")


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", gr.LN_KINDS)
@pytest.mark.parametrize("rows,d", gr.LN_SHAPES)
def test_layernorm_fwd(ops, rows, d, kind):
    x, gamma, beta = gr.ln_inputs(rows, d, kind)
    y_ref, mu_ref, rs_ref = gr.ln_fwd_ref(x, gamma, beta)
    y, mean, rstd = ops.layernorm_fwd(x.to(DEV), gamma.to(DEV), beta.to(DEV))
    torch.cuda.synchronize()
    y, mean, rstd = y.cpu(), mean.cpu(), rstd.cpu()
    ratio = (y.to(F64) - y_ref).abs() / gr.ln_fwd_tol(x, gamma, y_ref, rs_ref)
    print(f"layernorm fwd {rows}x{d} {kind}: worst |err| / rule {float(ratio.max()):.3f}")
    assert float(ratio.max()) <= 1.0, (int(ratio.argmax()) // d, int(ratio.argmax()) % d, float(ratio.max()))
    if kind == "constant":
        gr.check_exact("y of constant rows", y, beta.to(BF).expand(rows, d).contiguous(), where=lambda i: f"(row {i[0]}, column {i[1]}), x = {x[i[0], 0].item()}")
        assert bool(((rstd.to(F64) * 1e-5 ** 0.5 - 1.0).abs() <= 2.0 ** -22).all()), "rstd of a constant row is 1/sqrt(1e-5) to fp32 rounding"
        assert torch.equal(mean, x[:, 0].to(F32))


def _ln_bwd_case(ops, rows, d, kind, with_dres, dy=None):
    x, gamma, beta = gr.ln_inputs(rows, d, kind)
    xd, gd = x.to(DEV), gamma.to(DEV)
    _, mean_d, rstd_d = ops.layernorm_fwd(xd, gd, beta.to(DEV))
    g = torch.Generator().manual_seed(17 + rows)
    if dy is None:
        dy = torch.randn(rows, d, generator=g).to(BF)
    dres = torch.randn(rows, d, generator=g).to(BF) if with_dres else None
    torch.cuda.synchronize()
    return dict(x=x, gamma=gamma, dy=dy, dres=dres, mean=mean_d.cpu(), rstd=rstd_d.cpu(), xd=xd, gd=gd, mean_d=mean_d, rstd_d=rstd_d,
                dyd=in_buf(dy), dresd=None if dres is None else in_buf(dres))


@pytest.mark.parametrize("with_dres", [False, True], ids=["plain", "dres"])
@pytest.mark.parametrize("kind", gr.LN_KINDS)
@pytest.mark.parametrize("rows,d", gr.LN_SHAPES)
def test_layernorm_bwd(ops, rows, d, kind, with_dres):
    """dx by the forward's rule applied to its own terms (glue_ref.ln_bwd_ref), for every (dgamma, dbeta) null combination with and without
    dsum: dx of every instantiation inside the rule, the column sums against float64 from a pre-fill of one term's size."""
    c = _ln_bwd_case(ops, rows, d, kind, with_dres)
    dx_ref, dg_ref, db_ref, tol, xh = gr.ln_bwd_ref(c["dy"], c["x"], c["gamma"], c["mean"], c["rstd"], c["dres"])
    terms_g = (c["dy"].to(F64) * xh).abs().sum(0)
    terms_b = c["dy"].to(F64).abs().sum(0)
    pre_g = ((terms_g / rows).clamp_min(2.0 ** -100)).to(F32)
    pre_b = ((terms_b / rows).clamp_min(2.0 ** -100)).to(F32)
    pre_s = gr.ln_dsum_prefill(dx_ref)
    worst = 0.0
    for want_g in (True, False):
        for want_b in (True, False):
            for want_s in (True, False):
                xg, dx = out_buf((rows, d), BF)
                gg, dg = out_buf(pre_g)
                bg, db = out_buf(pre_b)
                sg, ds = out_buf(pre_s)
                ops.layernorm_bwd_(c["dyd"], c["xd"], c["gd"], c["mean_d"], c["rstd_d"], c["dresd"], dx, dg if want_g else None,
                                   db if want_b else None, ds if want_s else None)
                torch.cuda.synchronize()
                what = f"layernorm bwd {rows}x{d} {kind} dgamma={want_g} dbeta={want_b} dsum={want_s}"
                dxc = dx.cpu()  # (the instantiations may differ from each other in the last bit: each is held to the rule on its own)
                ratio = (dxc.to(F64) - dx_ref).abs() / tol
                worst = max(worst, float(ratio.max()))
                assert float(ratio.max()) <= 1.0, (what, int(ratio.argmax()) // d, int(ratio.argmax()) % d, float(ratio.max()))
                for name, got, pre, ref, terms, wanted in (("dgamma", dg, pre_g, dg_ref, terms_g, want_g), ("dbeta", db, pre_b, db_ref, terms_b, want_b)):
                    if wanted:  # fp32 sums over the rows, as the dsum rule: 2^-20 of the sum of the terms' magnitudes
                        err = (got.cpu().to(F64) - pre.to(F64) - ref).abs()
                        bad = (err > 2.0 ** -20 * terms).nonzero().flatten()
                        assert len(bad) == 0, (what, name, bad[:4].tolist(), err[bad[:4]].tolist(), terms[bad[:4]].tolist())
                    else:
                        gr.check_exact(what + f": null {name} left alone", got.cpu(), pre)
                if want_s:
                    bad = gr.ln_dsum_ok(ds.cpu(), pre_s, dxc)
                    assert len(bad) == 0, (what, "dsum columns", bad[:8].tolist())
                else:
                    gr.check_exact(what + ": null dsum left alone", ds.cpu(), pre_s)
                for gd_, nm in ((xg, "dx"), (gg, "dgamma"), (bg, "dbeta"), (sg, "dsum")):
                    gd_.check(what + " " + nm)
    print(f"layernorm bwd {rows}x{d} {kind} {'dres' if with_dres else 'plain'}: worst |dx err| / rule over the 8 instantiations {worst:.3f}")


@pytest.mark.parametrize("r", gr.NEEDLE_ROWS)
def test_layernorm_bwd_needle_row(ops, r):
    """dy is zero except row r: dgamma == dy[r] * xhat[r] and dbeta == dy[r] to 4 * 2^-24 relative on top of the pre-fill -- a row dropped or
    taken twice by the two-rows-per-wave walk (second loop iteration from row 4096, dead second row from row 4101) cannot hide."""
    rows, d = gr.LN_SHAPES[0]
    dy = torch.zeros(rows, d, dtype=BF)
    dy[r] = torch.randn(d, generator=torch.Generator().manual_seed(18 + r)).to(BF)
    c = _ln_bwd_case(ops, rows, d, "random", False, dy=dy)
    _, dg_ref, db_ref, _, xh = gr.ln_bwd_ref(dy, c["x"], c["gamma"], c["mean"], c["rstd"])
    assert torch.equal(dg_ref, dy[r].to(F64) * xh[r]) and torch.equal(db_ref, dy[r].to(F64))
    pre_g, pre_b = (0.25 * dg_ref).to(F32), (0.25 * db_ref).to(F32)  # a pre-fill below the value: the add rounds at the value's own magnitude
    xg, dx = out_buf((rows, d), BF)
    gg, dg = out_buf(pre_g)
    bg, db = out_buf(pre_b)
    ops.layernorm_bwd_(c["dyd"], c["xd"], c["gd"], c["mean_d"], c["rstd_d"], None, dx, dg, db, None)
    torch.cuda.synchronize()
    for name, got, pre, ref in (("dgamma", dg, pre_g, dg_ref), ("dbeta", db, pre_b, db_ref)):
        err = (got.cpu().to(F64) - pre.to(F64) - ref).abs()
        bad = (err > 4 * gr.E24 * ref.abs()).nonzero().flatten()
        assert len(bad) == 0, (f"needle row {r}", name, bad[:4].tolist(), (got.cpu().to(F64) - pre.to(F64))[bad[:4]].tolist(), ref[bad[:4]].tolist())
    for gd_, nm in ((xg, "dx"), (gg, "dgamma"), (bg, "dbeta")):
        gd_.check(f"needle row {r} {nm}")
