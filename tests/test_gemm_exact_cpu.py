"""The exact-integer GEMM cases (tests/gemm_exact.py) must have power: an integer stand-in for the kernels with one deliberate flaw at a
time is caught by the exact comparison or by the guard check, on the cases the builder makes -- and the regimes' input statistics,
computed from the reference alone, keep the rounding test from going vacuous.  No GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_exact as gx  # noqa: E402

F64 = torch.float64


def _case(regime, M, N, K, seed=0):
    A, B = gx.operands(regime, M, N, K, seed)
    return A, B, gx.reference(regime, A, B)


@pytest.mark.parametrize("K", [64, 128, 200, 1024, 1536, 4096])
def test_regime_r_statistics(K):
    """At every K the GPU tests use: >= 40 % of the sums need rounding, >= 5 % are exact ties, truncation differs from RNE on >= 20 %."""
    _, _, acc = _case("R", 512, 512, K)
    needs, ties, trunc = gx.rounding_stats(acc)
    print(f"K={K}: amplitude {gx.amplitude(K)}, max|acc| {int(acc.abs().max())}, need rounding {needs:.1%}, ties {ties:.1%}, truncation differs {trunc:.1%}")
    assert needs >= 0.40 and ties >= 0.05 and trunc >= 0.20, (K, needs, ties, trunc)


def test_regime_r_amplitude_covers_the_long_wgrads():
    assert gx.amplitude(1536) == 15 and gx.amplitude(4096) == 15 and gx.amplitude(57344) == 15
    assert gx.amplitude(192000) == 7 and 192000 * 49 < 2 ** 24 and gx.amplitude(74565) == 15 and gx.amplitude(74566) == 7


@pytest.mark.parametrize("K", [8, 64, 200, 1024, 4096])
def test_regime_s_bounds_and_rounding_points_are_identities(K):
    A, B, acc = _case("S", 300, 264, K, seed=K)
    assert int(acc.abs().max()) <= 64
    bias, resid, pos, u = gx.side_inputs(acc, seed=1, pos_period=100)
    pre = acc.to(F64) + bias
    m = torch.arange(300) % 100
    for name, v in (("pre", pre), ("pre + resid", pre + resid), ("pre + pos", pre + pos[m]), ("pre * u", pre * u),
                    ("pre + pos + resid'", (pre + pos[m]))):
        assert float(v.abs().max()) <= 256
        assert torch.equal(gx.rne_bf16(v).to(F64), v), name  # already a bf16 value: the rounding point is an identity
    _, _, _, u1 = gx.side_inputs(acc, seed=1, colsum=True)
    assert set(u1.unique().tolist()) <= {0.0, 1.0, -1.0} and 300 * 256 < 2 ** 24


def test_rne_bf16_is_round_to_nearest_even():
    v = torch.arange(-70000, 70000, dtype=torch.int64)
    r = gx.rne_bf16(v)
    assert torch.equal(r, v.to(torch.float32).to(gx.BF))  # torch's own conversion, an independent implementation
    assert gx.rne_bf16(torch.tensor([257, 258, 259, 385, 387])).tolist() == [256.0, 258.0, 260.0, 384.0, 388.0]
    assert gx.trunc_bf16(torch.tensor([259, -259])).tolist() == [258.0, -258.0]
    x = torch.tensor([1.0, 1.5, 255.0, 256.0, 2.0 ** -126, 0.0, 3.0e38], dtype=F64)
    assert gx.bf16_ulp(x).tolist() == [2.0 ** -7, 2.0 ** -7, 1.0, 2.0, 2.0 ** -133, 2.0 ** -133, 2.0 ** 120]


def test_gelu64_matches_autograd():
    x = torch.linspace(-12, 12, 4001, dtype=F64).requires_grad_(True)
    y = torch.nn.functional.gelu(x)
    y.sum().backward()
    assert float((gx.gelu64(x.detach()) - y.detach()).abs().max()) < 1e-14
    assert float((gx.dgelu64(x.detach()) - x.grad).abs().max()) < 1e-14


def test_embed_and_guard_check():
    t = torch.arange(12 * 20, dtype=torch.float32).view(12, 20)
    for dtype in (gx.BF, torch.float32):
        g = gx.embed(t.to(dtype))
        assert g.ld % 8 == 0 and g.ld >= 20 + 72 and g.buf.shape[0] == 12 + 512 and g.view.stride(0) == g.ld
        assert g.view.data_ptr() % 16 == 0 and (g.ld * g.buf.element_size()) % 16 == 0
        assert torch.equal(g.view, t.to(dtype))
        g.check()
        g.view.fill_(3.0)
        g.check()
        for r, c in ((gx.PAD_ROWS - 1, gx.COL0), (gx.PAD_ROWS + 12, gx.COL0 + 19), (gx.PAD_ROWS, gx.COL0 - 1), (gx.PAD_ROWS + 11, gx.COL0 + 20)):
            keep = g.buf[r, c].clone()
            g.buf[r, c] = 1.0
            with pytest.raises(AssertionError):
                g.check()
            g.buf[r, c] = keep
            g.check()
    assert bool(torch.isnan(gx.embed(t.to(gx.BF), fill="nan").buf[0, 0])) and bool(torch.isinf(gx.embed(t.to(gx.BF), fill="inf").buf[-1, -1]))
    v = gx.embed_vec(torch.zeros(24))
    v.check()
    v.buf[0, gx.COL0 + 24] = 0.0
    with pytest.raises(AssertionError):
        v.check()


# ---- one flaw at a time ---------------------------------------------------------------------------------------------------------------
def _run(flaw, regime="R", M=300, N=264, K=200, with_bias=False, with_resid=False, split_k=1, colsum=False):
    A, B, acc = _case(regime, M, N, K, seed=3)
    g = torch.Generator().manual_seed(4)
    if regime == "S":
        bias, resid, _, _ = gx.side_inputs(acc, seed=5)
    else:
        bias = torch.randint(-64, 65, (N,), generator=g).to(F64)
        resid = torch.randint(-128, 129, (M, N), generator=g).to(F64)
    bias = bias if with_bias else None
    resid = resid if with_resid else None
    ldb = torch.full((N, K + 8), float("nan"), dtype=F64)
    ldb[:, :K] = B.to(F64)
    outs = []
    for f in (None, flaw):
        out = gx.embed(torch.zeros(M, N, dtype=gx.BF))
        o, cs = gx.emulate(A, B, flaw=f, out=out, ldb_pad=ldb, bias=bias, resid=resid, split_k=split_k, colsum=colsum)
        outs.append((o, cs, out))
    (want, want_cs, clean), (got, got_cs, dirty) = outs
    clean.check("flawless emulation")
    value_caught = not torch.equal(torch.nan_to_num(got, nan=1e30), want) or (colsum and not torch.equal(got_cs, want_cs))
    try:
        dirty.check(flaw)
        guard_caught = False
    except AssertionError:
        guard_caught = True
    return value_caught, guard_caught


@pytest.mark.parametrize("flaw,kw,by", [
    ("truncating_pack", {}, "value"),
    ("double_rounding_11_bits", {"K": 1024}, "value"),
    ("last_k_chunk_dropped", {"K": 200}, "value"),
    ("split_range_off_by_one_tile", {"K": 1536, "split_k": 3}, "value"),
    ("row_panel_one_tile_too_far", {"M": 300}, "guard"),
    ("store_16_bytes_past_n", {"N": 132}, "guard"),
    ("pad_column_of_b_read", {"K": 200}, "value"),
    ("colsum_includes_rows_past_m", {"regime": "S", "colsum": True}, "value"),
    ("resid_before_bias", {"with_bias": True, "with_resid": True}, "value"),
])
def test_each_flaw_is_caught(flaw, kw, by):
    value_caught, guard_caught = _run(flaw, **kw)
    print(f"{flaw}: caught by the exact comparison: {value_caught}, by the guard check: {guard_caught}")
    assert (value_caught if by == "value" else guard_caught), flaw
    assert flaw in gx.FLAWS


def test_every_listed_flaw_has_a_power_case():
    params = [m.args[1] for m in test_each_flaw_is_caught.pytestmark if m.name == "parametrize"][0]
    assert {p[0] for p in params} == set(gx.FLAWS)


def test_residual_order_does_not_matter_in_regime_s_but_does_in_regime_r():
    """The docstring's claim about S, tested: with every rounding point an identity, adding the residual before the bias changes
    nothing; in regime R (sums that round) the same flaw is caught."""
    value_caught, guard_caught = _run("resid_before_bias", regime="S", K=1024, with_bias=True, with_resid=True)
    assert not value_caught and not guard_caught
    value_caught, _ = _run("resid_before_bias", regime="R", K=1024, with_bias=True, with_resid=True)
    assert value_caught


def test_k_not_a_multiple_of_8_is_refused_for_a_k_contiguous_b():
    """ta = 1, tb = 0, K % 8 != 0: B's last 16-byte chunk would bring in up to 7 elements past K (bounds are checked per chunk), where
    NaN / Inf survives A's zero fill.  The launcher refuses the combination before anything is launched."""
    import ctypes as C
    import os
    import __graft_entry__ as g
    from olmoasr_amd import _native as N
    if not os.path.isfile(N.LIB_PATH):
        g.build()
    a = N.GemmArgs()
    a.A = N.Operand(16, 8, 0, 0, 0, 0, 0)  # (addresses are never dereferenced: the argument checks come first)
    a.B = N.Operand(16, 208, 0, 0, 0, 0, 0)
    a.M, a.N, a.K, a.ta, a.tb, a.alpha, a.split_k = 8, 8, 203, 1, 0, 1.0, 1
    a.out, a.ldc = 16, 8
    rc = N.lib().oasr_gemm(C.byref(a), None)
    assert rc != 0 and b"k-contiguous B" in N.lib().oasr_last_error()
    a.ta, a.tb, a.A = 0, 1, N.Operand(16, 208, 0, 0, 0, 0, 0)
    rc = N.lib().oasr_gemm(C.byref(a), None)
    assert rc != 0 and b"k-contiguous A" in N.lib().oasr_last_error()
