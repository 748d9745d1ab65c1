"""Every GEMM kernel on exact-integer operands (tests/gemm_exact.py): bit-exact results against an integer reference on the CPU, guard
bands around every operand and output, and the kernel that ran checked against the kernel the case names.

Every case states the kernel family it expects (general 128x128, direct-to-LDS 256x128 / 256x256, ping-pong 256x256, skinny <1> / <2>).
After the call the launch records (include/oasr_testing.h: oasr_profile_gemm_records) are read and the case FAILS if another kernel
ran.  The parametrisation is generated from the eligibility rules of launch_gemm (``takes``), so no (path, shape) pair that cannot take
its path is generated and nothing here skips.

 a. edge matrix (regime R, one rounding): M, N, K tails, all four layouts, split-K with uneven and empty ranges, fp32 outputs with
    beta = 1 and ldc32 > N, the skinny kernel's decode shapes, conv-window views against an integer conv1d;
 b. epilogues (regime S, every rounding point an identity): the seven compiled epilogue modes and seven more that take the generic
    instantiation, on every path, with interior and partial wave blocks, both productions of the fused column sums;
 c. GELU / GELU' over every finite bf16 value through the epilogue of every path, against float64;
 d. the medium training step's own launch configurations at its own sizes (one B = 128 micro-batch);
 e. a ledger: one medium B = 128 span step launches nothing (kernel symbol, epilogue flags, N, K, split_k, atomic_on_pp, stagger) that
    (a) - (d) do not cover.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_exact as gx  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
F64 = torch.float64
LAYOUTS = {"NT": (False, False), "NN": (False, True), "TN": (True, False), "TT": (True, True)}

PATHS, takes, family_of = gx.PATHS, gx.takes, gx.family_of  # (shared with tests/test_gemm_route_cpu.py, which holds them to the library's route)
FLAG = dict(BIAS=1, RESID=2, U=4, UDERIV=8, PRE=16, OUT=32, GELU=64, DERIV=128, POS=256, SCALE=512, NT_ST=1024, NT_LD=2048)
COVERED = set()  # ledger keys of the cases that ran (e)


def ops():
    from olmoasr_amd import ops as o
    return o


def ledger_key(r):
    """What (e) compares: layout and kernel variant are part of the symbol; the non-temporal policy bits are not a launch property."""
    return (r["symbol"], r["flags"] & ~(FLAG["NT_ST"] | FLAG["NT_LD"]), r["N"], r["K"], r["split_k"], r["atomic_on_pp"],
            int(r["stagger"] > 0 and r["stagger_phases"] > 1))


class forced:
    """Force a kernel path for the duration of a block and record what is launched inside it; the process-wide hooks are restored."""

    def __init__(self, path):
        self.path = path

    def __enter__(self):
        from olmoasr_amd import _native as N
        mode, variant, _ = PATHS[self.path] if self.path in PATHS else (0, -1, None)
        N.check(N.lib().oasr_gemm_force_general(mode), "force")
        N.check(N.lib().oasr_gemm_set_variant(variant), "variant")
        N.lib().oasr_profile_gemm(1)
        return self

    def __exit__(self, *exc):
        from olmoasr_amd import _native as N
        try:
            self.records = ops().gemm_launch_records()
        finally:
            N.lib().oasr_profile_gemm(0)
            N.lib().oasr_gemm_force_general(0)
            N.lib().oasr_gemm_set_variant(-1)
        return False


def check_ran(records, path, M, *, n=1, csum=None, persistent=None):
    """The launches were ``n`` GEMMs of the family ``path`` names (skinny: <1> for M <= 32, <2> above)."""
    fam = PATHS[path][2]
    assert len(records) == n, (path, [r["symbol"] for r in records])
    for r in records:
        assert family_of(r["symbol"]) == fam, f"case names {path}, but {r['symbol']} ran"
        if fam == "skinny":
            assert r["symbol"] == ("gemm_skinny_kernel<1>" if M <= 32 else "gemm_skinny_kernel<2>"), r["symbol"]
        if csum is not None:  # fused column sums: the CSUM instantiation (last template argument of the fast kernel, 4th of the ping-pong one)
            args = r["symbol"][r["symbol"].index("<") + 1:-1].split(", ")
            assert (args[3] if fam == "pp" else args[6]) == ("true" if csum else "false"), r["symbol"]
        if persistent is not None:
            assert r["persistent"] == int(persistent), (path, r)
        COVERED.add(ledger_key(r))


def to_bf(t):
    return t.to(torch.float32).to(BF)


def stored(X, transposed, fill):
    """The logical operand X [rows, K] as the kernel reads it ([K, rows] when transposed), guard-banded with NaN / Inf, on the device."""
    return gx.embed(to_bf(X.t().contiguous() if transposed else X), fill=fill, device=DEV)


def fresh_out(M, N, dtype=BF, prefill=None):
    t = torch.full((M, N), float("nan"), dtype=dtype) if prefill is None else prefill.to(dtype)
    return gx.embed(t, device=DEV)


def assert_equal(got, want, name):
    got = got.detach().to(want.device)
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype)
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{name}: {int(bad.sum())}/{bad.numel()} elements differ; first at {i}: got {got[tuple(i)].item()!r}, want {want[tuple(i)].item()!r}")


def case_seed(*parts):
    return sum((i + 1) * 7919 * int(p) for i, p in enumerate(parts)) % (2 ** 31)


def accumulator(regime, A, B, big, seed):
    """The integer sums [M, N] of the logical operands, preconditions asserted.  Small cases: float64 on the CPU.  Production-sized
    cases (``big``: operands live on the device): torch's fp32 matmul on the device -- in these regimes any correct fp32 GEMM gives the
    same bits, a premise that is asserted itself: at least 1,024 output rows (first and last of every 256-row tile plus seeded random
    rows, all columns) are recomputed in float64 integer arithmetic on the CPU and must be equal."""
    if not big:
        return gx.reference(regime, A, B)
    acc = A.float() @ B.float().t()
    rows = gx.sample_rows(A.shape[0], seed)
    want = gx.matmul_int(A[rows.to(DEV)].cpu(), B.cpu())
    assert torch.equal(acc[rows.to(DEV)].cpu().to(torch.int64), want), "device fp32 reference differs from the CPU integer product"
    gx.check_regime(regime, A, B, acc)
    return acc.to(torch.int64)


def _ids(cases):
    return ["-".join(str(x) for x in c).replace(" ", "").replace("(", "").replace(")", "").replace(",", "x") for c in cases]


# ======================================================================================================================================
# a. edge matrix, regime R
# ======================================================================================================================================
EDGE_SHAPES = [(8, 8, 64), (255, 12, 200), (256, 132, 128), (257, 136, 128), (300, 264, 1536), (2560 + 64, 1024, 64), (300, 256, 200),
               (256, 8, 128), (264, 136, 1536)]
EDGE_PATHS = ("general", "fast128", "fast256", "pp", "pp_nt")
EDGE_CASES = [(p, lay, s) for s in EDGE_SHAPES for lay in LAYOUTS for p in EDGE_PATHS if takes(p, *s, *LAYOUTS[lay])]
# persistent launches need more than 256 tiles: 11 x 25 tiles of 256 x 256 with ragged last row and column panels
EDGE_CASES += [(p, lay, (2560 + 64, 6152, 128)) for p in ("pp_persistent", "pp_persistent_nt") for lay in ("NT", "NN")]
EDGE_CASES += [("general", "TT", (256, 136, 203)), ("general", "TT", (255, 12, 203))]  # K % 8 != 0: both operands transposed


def run_rounding(path, layout, shape, *, big=False, auto=False):
    """Regime R, plain bf16 `out`.  auto: no path is forced, ``path`` is what launch_gemm must choose by itself."""
    M, N, K = shape
    ta, tb = LAYOUTS[layout]
    seed = case_seed(M, N, K, ta, tb)
    A, B = gx.operands("R", M, N, K, seed, device=DEV if big else "cpu")
    acc = accumulator("R", A, B, big, seed)
    fill = "inf" if seed % 2 else "nan"
    Ag, Bg, out = stored(A, ta, fill), stored(B, tb, fill), fresh_out(M, N)
    with forced("auto" if auto else path) as f:
        ops().gemm(Ag.view, Bg.view, M, N, K, ta=ta, tb=tb, out=out.view)
        torch.cuda.synchronize()
    check_ran(f.records, path, M, persistent=path.startswith("pp_persistent"))
    if big:  # the device's own fp32 -> bf16 conversion, held to the integer-arithmetic RNE on the sampled rows
        want = acc.to(torch.float32).to(BF)
        rows = gx.sample_rows(M, seed).to(DEV)
        assert torch.equal(want[rows], gx.rne_bf16(acc[rows]))
    else:
        want = gx.rne_bf16(acc)
    assert_equal(out.view, want, f"{path} {layout} {shape}")
    out.check(f"{path} {layout} {shape} out")


@pytest.mark.parametrize("path,layout,shape", EDGE_CASES, ids=_ids(EDGE_CASES))
def test_edge_bf16_output(path, layout, shape):
    """out = RNE_bf16(sum) with a single rounding, every guard byte intact, operand pads (NaN / Inf in turn) never reach a sum."""
    run_rounding(path, layout, shape)


def test_edge_k_tail_with_k_contiguous_b_is_refused():
    """ta = 1, tb = 0, K % 8 != 0 (B's last 16-byte chunk would straddle K): refused by the launcher, nothing is launched or written."""
    from olmoasr_amd import _native as N
    M, N_, K = 256, 136, 203
    A, B = gx.operands("R", M, N_, K, 1)
    Ag, out = stored(A, True, "nan"), fresh_out(M, N_)
    Bg = gx.embed(to_bf(B), pad_cols=77, fill="nan", device=DEV)  # ld = 288: a multiple of 8 although K is not
    assert Bg.ld % 8 == 0
    with forced("general") as f:
        with pytest.raises(N.NativeError, match="k-contiguous B"):
            ops().gemm(Ag.view, Bg.view, M, N_, K, ta=True, tb=False, out=out.view)
        torch.cuda.synchronize()
    assert f.records == []
    assert bool(torch.isnan(out.view).all())
    out.check("refused call")


@pytest.mark.parametrize("alpha", [0.5, 2.0])
@pytest.mark.parametrize("path", ["general", "fast128", "fast256", "pp", "skinny"])
def test_edge_alpha(path, alpha):
    """alpha * sum is exact in fp32 for alpha = 0.5 and 2; the output rounds it once."""
    M, N, K = (40, 264, 128) if path == "skinny" else (300, 264, 128)
    assert takes(path, M, N, K, False, False)
    A, B = gx.operands("R", M, N, K, 5)
    acc = gx.reference("R", A, B)
    Ag, Bg, out = stored(A, False, "nan"), stored(B, False, "inf"), fresh_out(M, N)
    with forced(path) as f:
        ops().gemm(Ag.view, Bg.view, M, N, K, alpha=alpha, out=out.view)
        torch.cuda.synchronize()
    check_ran(f.records, path, M)
    assert_equal(out.view, gx.rne_bf16(acc.to(torch.float32) * alpha), f"{path} alpha={alpha}")
    out.check(f"{path} alpha")


# ---- fp32 outputs: the integer itself --------------------------------------------------------------------------------------------------
F32_SHAPES = [(304, 264, 1600), (300, 132, 1600), (8, 8, 64)]  # K = 1600: 25 K-tiles, divisible by no split below
F32_CASES = [(p, lay, s, split) for s in F32_SHAPES for lay in LAYOUTS for p in ("general", "fast128", "fast256", "pp")
             for split in (1, 3, 4, 8, 16) if takes(p, *s, *LAYOUTS[lay], atomic_only=True)]


def run_atomic(path, layout, shape, split, *, big=False, auto=False, alpha=1.0, **engine):
    """Regime R, out_f32 += alpha * sum with fp32 atomics over ``split`` K ranges, on a pre-filled integer output with ldc32 > N."""
    M, N, K = shape
    ta, tb = LAYOUTS[layout]
    seed = case_seed(M, N, K, ta, tb, split)
    dev = DEV if big else "cpu"
    A, B = gx.operands("R", M, N, K, seed, device=dev)
    acc = accumulator("R", A, B, big, seed)
    pre = torch.randint(-1000, 1001, (M, N), generator=torch.Generator(device=dev).manual_seed(seed), device=dev)
    want = acc * int(alpha) + pre
    assert int(want.abs().max()) < 2 ** 24 and alpha == int(alpha)
    fill = "inf" if seed % 2 else "nan"
    Ag, Bg, out = stored(A, ta, fill), stored(B, tb, fill), fresh_out(M, N, torch.float32, pre)
    assert out.ld > N
    with forced("auto" if auto else path) as f:
        ops().gemm(Ag.view, Bg.view, M, N, K, ta=ta, tb=tb, out_f32=out.view, atomic=True, split_k=split, alpha=alpha, **engine)
        torch.cuda.synchronize()
    check_ran(f.records, path, M)
    assert_equal(out.view, want.to(torch.float32), f"{path} {layout} {shape} split {split}")
    out.check("out_f32")
    return f.records


@pytest.mark.parametrize("path,layout,shape,split", F32_CASES, ids=_ids(F32_CASES))
def test_edge_f32_atomic_split_k(path, layout, shape, split):
    """out_f32 += sum over split-K ranges with fp32 atomics (uneven and empty last ranges; splits of 8 and 16 take the XCD-owned
    mapping): pre-filled integers plus the integer sum, exactly; ldc32 > N."""
    run_atomic(path, layout, shape, split)


F32_STORE_CASES = [("general", lay, s, beta) for s in [(300, 132, 200), (255, 12, 200), (304, 264, 1536)] for lay in LAYOUTS
                   for beta in (0.0, 1.0) if takes("general", *s, *LAYOUTS[lay], f32=True)]
F32_STORE_CASES += [("skinny", "NT", s, beta) for s in [(33, 776, 128), (8, 40, 64)] for beta in (0.0, 1.0)]


@pytest.mark.parametrize("path,layout,shape,beta", F32_STORE_CASES, ids=_ids(F32_STORE_CASES))
def test_edge_f32_store_and_beta(path, layout, shape, beta):
    """out_f32 = beta * out_f32 + sum (non-atomic): the integer exactly, on a pre-filled integer output for beta = 1; next to a bf16 `out`."""
    M, N, K = shape
    ta, tb = LAYOUTS[layout]
    seed = case_seed(M, N, K, ta, tb, int(beta))
    A, B = gx.operands("R", M, N, K, seed)
    acc = gx.reference("R", A, B)
    pre = torch.randint(-1000, 1001, (M, N), generator=torch.Generator().manual_seed(seed))
    Ag, Bg = stored(A, ta, "nan"), stored(B, tb, "inf")
    o32, out = fresh_out(M, N, torch.float32, pre), fresh_out(M, N)
    with forced(path) as f:
        ops().gemm(Ag.view, Bg.view, M, N, K, ta=ta, tb=tb, out_f32=o32.view, beta=beta, out=out.view)
        torch.cuda.synchronize()
    check_ran(f.records, path, M)
    assert_equal(o32.view, (acc + (pre if beta else 0)).to(torch.float32), f"{path} {layout} {shape} beta {beta}")
    assert_equal(out.view, gx.rne_bf16(acc), "bf16 out beside the fp32 one")
    o32.check("out_f32")
    out.check("out")


# ---- skinny kernel: decode shapes ------------------------------------------------------------------------------------------------------
SKINNY_SHAPES = [(1, 768, 768), (20, 2304, 768), (33, 776, 3072), (64, 51864, 384), (8, 40, 64), (32, 776, 128), (33, 40, 128), (64, 776, 64)]


@pytest.mark.parametrize("M,N,K", SKINNY_SHAPES)
def test_edge_skinny_decode_shapes(M, N, K):
    """No path is forced: M <= 64 in the NT layout must route to gemm_skinny_kernel<1> (M <= 32) or <2> by itself."""
    assert takes("skinny", M, N, K, False, False)
    A, B = gx.operands("R", M, N, K, case_seed(M, N, K))
    acc = gx.reference("R", A, B)
    Ag, Bg, out = stored(A, False, "inf"), stored(B, False, "nan"), fresh_out(M, N)
    with forced("skinny") as f:
        ops().gemm(Ag.view, Bg.view, M, N, K, out=out.view)
        torch.cuda.synchronize()
    check_ran(f.records, "skinny", M)
    assert_equal(out.view, gx.rne_bf16(acc), f"skinny {M}x{N}x{K}")
    out.check("skinny out")


# ---- conv-window views -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["conv1", "conv2"])
def test_edge_conv_window_views(which):
    """Conv1d(k = 3, p = 1[, s = 2]) as a window GEMM over a time-major activation, forward and weight gradient, with integer inputs
    against an integer conv1d on the CPU.  The batches of the activation lie apart (bstride > T ci) with NaN between, before and after
    them: the lead / trail rows of every batch must come from the implicit zeros, not from the neighbouring memory."""
    from olmoasr_amd import _native as N_
    B_, T = 2, 3000
    ci, co, stride = (80, 128, 1) if which == "conv1" else (128, 128, 2)
    ldk = 256 if which == "conv1" else 3 * ci
    Tout = T // stride
    g = torch.Generator().manual_seed(17)
    x = torch.randint(-15, 16, (B_, T, ci), generator=g)
    w = torch.randint(-15, 16, (co, ci, 3), generator=g)
    wp = torch.zeros(co, ldk, dtype=torch.int64)
    wp[:, :3 * ci] = w.permute(0, 2, 1).reshape(co, 3 * ci)  # k = kk * ci + c; columns past 3 ci belong to the logical operand: zeros
    ref = F.conv1d(x.to(F64).permute(0, 2, 1), w.to(F64), stride=stride, padding=1).permute(0, 2, 1).reshape(B_ * Tout, co)
    assert float(ref.abs().max()) < 2 ** 24 and 3 * ci * 225 < 2 ** 24
    gap = 40  # rows of NaN between the batches; one whole NaN batch before the first
    xbuf = torch.full((B_ + 1, T + gap, ci), float("nan"), dtype=BF, device=DEV)
    xbuf[1:, :T] = to_bf(x).to(DEV)
    xv = xbuf[1:]
    view = N_.Operand(xv.data_ptr(), ci * stride, Tout, (T + gap) * ci, ci, 3 * ci, (2 * ci) if stride == 1 else 3 * ci)
    wg, out = gx.embed(to_bf(wp), fill="nan", device=DEV), fresh_out(B_ * Tout, co)
    with forced("auto") as f:
        ops().gemm(None, wg.view, B_ * Tout, co, ldk, a_view=view, out=out.view)
        torch.cuda.synchronize()
    assert [family_of(r["symbol"]) for r in f.records] == ["general"], f.records
    COVERED.update(ledger_key(r) for r in f.records)
    assert_equal(out.view, gx.rne_bf16(ref.to(torch.int64)), which + " forward")
    out.check(which + " out")
    # weight gradient through the same window view: dWp[co, ldk] += dY^T . windows  (TT with a viewed B, split-K atomics)
    dY = torch.randint(-15, 16, (B_ * Tout, co), generator=g)
    assert B_ * Tout * 225 < 2 ** 24
    wf = w.to(F64).requires_grad_(True)
    F.conv1d(x.to(F64).permute(0, 2, 1), wf, stride=stride, padding=1).backward(dY.to(F64).view(B_, Tout, co).permute(0, 2, 1))
    ref_w = torch.zeros(co, ldk, dtype=F64)
    ref_w[:, :3 * ci] = wf.grad.permute(0, 2, 1).reshape(co, 3 * ci)
    pre = torch.randint(-1000, 1001, (co, ldk), generator=g)
    assert float((ref_w + pre).abs().max()) < 2 ** 24
    dyg, dW = gx.embed(to_bf(dY), fill="inf", device=DEV), fresh_out(co, ldk, torch.float32, pre)
    with forced("auto") as f:
        ops().gemm(dyg.view, None, co, ldk, B_ * Tout, ta=True, tb=True, b_view=view, out_f32=dW.view, atomic=True, split_k=2)
        torch.cuda.synchronize()
    assert [family_of(r["symbol"]) for r in f.records] == ["general"], f.records
    COVERED.update(ledger_key(r) for r in f.records)
    assert_equal(dW.view, (ref_w + pre).to(torch.float32), which + " wgrad")
    dW.check(which + " dW")


# ======================================================================================================================================
# b. epilogues, regime S
# ======================================================================================================================================
# name -> (layout, options).  The first seven are gemm_common.h's EPI_MODES in order; the rest take the generic instantiation (MODE < 0).
EPILOGUES = {
    "bias": ("NT", dict(bias=1)),
    "bias_resid": ("NT", dict(bias=1, resid=1)),
    "bias_act2": ("NT", dict(bias=1, act=2, out_pre=1)),
    "bias_act1": ("NT", dict(bias=1, act=1)),
    "plain": ("NN", dict()),
    "resid": ("NN", dict(resid=1)),
    "u_deriv": ("NN", dict(u=1, deriv=1)),
    "bias_pos": ("NT", dict(bias=1, pos=1)),
    "bias_alpha": ("NT", dict(bias=1, alpha=0.5)),
    "pre_only": ("NT", dict(bias=1, out_pre=1, out=0)),
    "u_gelu_deriv": ("NN", dict(u=1)),
    "bias_act1_pre": ("NT", dict(bias=1, act=1, out_pre=1)),
    "bias_pre_resid": ("NT", dict(bias=1, out_pre=1, resid=1)),
    "bias_act1_pre_pos": ("NT", dict(bias=1, act=1, out_pre=1, pos=1)),  # the conv stem: GELU, then the positional embedding
}
EPI_SHAPES = [(300, 384, 64), (300, 384, 1024), (640, 384, 64), (640, 384, 1024)]
EPI_PATHS = ("general", "fast128", "fast256", "pp", "pp_nt")
EPI_CASES = [(p, e, s) for e in EPILOGUES for s in EPI_SHAPES for p in EPI_PATHS if takes(p, *s, *LAYOUTS[EPILOGUES[e][0]])]
EPI_CASES += [("skinny", e, s) for e in EPILOGUES for s in [(24, 384, 64), (48, 264, 1024)] if EPILOGUES[e][0] == "NT"]
GELU_C = 1.5e-7      # common.h: |erf err| <= 1.5e-7 -> |Phi err| <= 0.75e-7, and as much again for the fp32 polynomial on v_rcp_f32 / v_exp_f32
FLOOR = 2.0 ** -126  # subnormal results may be flushed


def gelu_bound(got, want, x):
    return 0.5 * gx.bf16_ulp(torch.maximum(got.abs(), want.abs())) + GELU_C * x.abs() + FLOOR


def dgelu_bound(got, want, scale=1.0):
    return 0.5 * gx.bf16_ulp(torch.maximum(got.abs(), want.abs())) + GELU_C * scale + FLOOR


def is_bf16(v):
    return torch.equal(gx.rne_bf16(v).to(F64), v)


def epilogue_flags(o):
    return ((FLAG["BIAS"] if o.get("bias") else 0) | (FLAG["RESID"] if o.get("resid") else 0) | (FLAG["U"] if o.get("u") else 0) |
            (FLAG["UDERIV"] if o.get("deriv") else 0) | (FLAG["PRE"] if o.get("out_pre") else 0) | (FLAG["OUT"] if o.get("out", 1) else 0) |
            (FLAG["GELU"] if o.get("act") else 0) | (FLAG["DERIV"] if o.get("act") == 2 else 0) | (FLAG["POS"] if o.get("pos") else 0) |
            (FLAG["SCALE"] if o.get("alpha", 1.0) != 1.0 else 0))


def run_epilogue(path, epi, shape, *, colsum=None, seed=None, big=False, auto=False, pos_period=100):
    """One regime S GEMM with the epilogue ``epi`` on ``path``; side inputs and outputs guard-banded.  colsum: None, "atomic" or "scratch".
    big: operands drawn and expectations formed on the device (``accumulator``); auto: no path is forced.  Returns the launch records."""
    M, N, K = shape
    layout, o = EPILOGUES[epi]
    ta, tb = LAYOUTS[layout]
    seed = case_seed(M, N, K, len(epi)) if seed is None else seed
    dev = DEV if big else "cpu"
    A, B = gx.operands("S", M, N, K, seed, device=dev)
    acc = accumulator("S", A, B, big, seed).to(F64)
    bias, resid, pos, u = gx.side_inputs(acc, seed + 1, colsum=colsum is not None, pos_period=pos_period, device=dev)
    fill = "inf" if seed % 2 else "nan"
    alpha = o.get("alpha", 1.0)
    # ---- expected, in float64, with every rounding point asserted to be an identity
    v = acc * alpha + (bias if o.get("bias") else 0.0)
    assert is_bf16(v) and float(v.abs().max()) <= 128
    pre = v
    act = o.get("act", 0)
    inexact_out = None  # the bound, when `out` carries a transcendental
    if act:
        v = gx.gelu64(pre)
        inexact_out = lambda got, want: gelu_bound(got, want, pre)  # noqa: E731
    if o.get("pos"):
        if act:  # bf16(gelu) + pos: the GELU value is rounded before the add (kernels.h), half an ulp of it on top of the final rounding
            mid_half_ulp = 0.5 * gx.bf16_ulp(v)
            inexact_out = lambda got, want: gelu_bound(got, want, pre) + mid_half_ulp  # noqa: E731
        v = v + pos[torch.arange(M, device=dev) % pos_period]
        assert float(v.abs().max()) <= 256 and (act or is_bf16(v))
    if o.get("u"):
        if o.get("deriv"):
            v = v * u
            assert is_bf16(v)
        else:
            v = v * gx.dgelu64(u)
            inexact_out = lambda got, want: dgelu_bound(got, want, pre.abs())  # noqa: E731
    if o.get("resid"):
        v = v + resid
        assert is_bf16(v) and float(v.abs().max()) <= 256
    # ---- device side
    Ag, Bg = stored(A, ta, fill), stored(B, tb, fill)
    kw = dict(alpha=alpha, act=act)
    if o.get("bias"):
        kw["bias"] = bias.to(torch.float32).to(DEV)
    if o.get("pos"):
        kw["pos"], kw["pos_period"] = pos.to(torch.float32).to(DEV), pos_period
    if o.get("u"):
        ug = gx.embed(to_bf(u), fill=fill, device=DEV)
        kw["dgelu_u"], kw["dgelu_deriv"] = ug.view, bool(o.get("deriv"))
    if o.get("resid"):
        rg = gx.embed(to_bf(resid), fill=fill, device=DEV)
        kw["resid"] = rg.view
    out = fresh_out(M, N) if o.get("out", 1) else None
    opre = fresh_out(M, N) if o.get("out_pre") else None
    if out is not None:
        kw["out"] = out.view
    if opre is not None:
        kw["out_pre"] = opre.view
    cs = scratch = None
    if colsum is not None:
        cs_pre = torch.randint(-500, 501, (N,), generator=torch.Generator().manual_seed(seed + 2)).to(torch.float32).to(dev)
        cs = gx.embed_vec(cs_pre, device=DEV)
        kw["colsum"] = cs.view[0]
        if colsum == "scratch":
            rows = 2 * ((M + 255) // 256)  # the kernel's partial rows, then 64 guard rows
            scratch = torch.full((rows + 64, N), gx.SENTINEL_F32, dtype=torch.int32, device=DEV).view(torch.float32)
            kw["colsum_scratch"] = scratch
    with forced("auto" if auto else path) as f:
        ops().gemm(Ag.view, Bg.view, M, N, K, ta=ta, tb=tb, **kw)
        torch.cuda.synchronize()
    name = f"{path} {epi} {shape} colsum={colsum}"
    if out is not None:
        if inexact_out is None:
            assert_equal(out.view, v.to(BF), name + " out")
        else:
            g64 = out.view.to(dev).to(F64)
            err = (g64 - v).abs()
            bad = ~(err <= inexact_out(g64, v))
            assert not bool(bad.any()), f"{name} out: {int(bad.sum())} outside the GELU bound, worst |err| {float(err[bad].max()):.3g}"
        out.check(name + " out")
    if opre is not None:
        if act == 2:
            want_d = gx.dgelu64(pre)
            gp = opre.view.to(dev).to(F64)
            bad = ~((gp - want_d).abs() <= dgelu_bound(gp, want_d))
            assert not bool(bad.any()), f"{name} out_pre (GELU'): {int(bad.sum())} outside the bound"
        else:
            assert_equal(opre.view, pre.to(BF), name + " out_pre")
        opre.check(name + " out_pre")
    if cs is not None:
        # column sums of the bf16 values stored to `out`: exact integers, the epilogue being linear
        assert inexact_out is None and float(v.abs().max()) * M < 2 ** 24
        assert_equal(cs.view[0], (cs_pre.to(F64) + v.sum(0)).to(torch.float32), name + " colsum")
        cs.check(name + " colsum")
        if scratch is not None:
            tail = scratch.view(torch.int32)[2 * ((M + 255) // 256):]
            assert bool((tail == gx.SENTINEL_F32).all()), name + ": colsum_scratch written past 2 ceil(M / 256) rows"
    return f.records


@pytest.mark.parametrize("path,epi,shape", EPI_CASES, ids=_ids(EPI_CASES))
def test_epilogue(path, epi, shape):
    recs = run_epilogue(path, epi, shape)
    check_ran(recs, path, shape[0])
    assert recs[0]["flags"] & 1023 == epilogue_flags(EPILOGUES[epi][1]), recs[0]  # the epilogue the kernel saw is the one the case names


COLSUM_CASES = [(p, e, s, how) for e in ("plain", "resid", "u_deriv", "bias", "bias_resid") for s in [(300, 384, 64), (640, 384, 1024)]
                for p in EPI_PATHS[:4] for how in ("atomic", "scratch") if takes(p, *s, *LAYOUTS[EPILOGUES[e][0]])]


@pytest.mark.parametrize("path,epi,shape,how", COLSUM_CASES, ids=_ids(COLSUM_CASES))
def test_epilogue_column_sums(path, epi, shape, how):
    """colsum += column sums of the stored bf16 `out`, on a non-zero integer pre-fill: fused into the NN kernels' epilogues (CSUM
    instantiation) through fp32 atomics or through colsum_scratch's partial rows, a separate pass elsewhere."""
    recs = run_epilogue(path, epi, shape, colsum=how)
    fused = EPILOGUES[epi][0] == "NN" and path in ("fast128", "pp")
    check_ran(recs, path, shape[0], csum=fused if path != "general" else None)
    assert recs[0]["scratch"] == int(how == "scratch")


# ======================================================================================================================================
# c. GELU / GELU' over every finite bf16 value
# ======================================================================================================================================
def all_finite_bf16():
    bits = torch.arange(0, 65536, dtype=torch.int32)
    bits = bits[((bits >> 7) & 0xFF) != 0xFF]
    assert bits.numel() == 65280
    return torch.where(bits >= 32768, bits - 65536, bits).to(torch.int16).view(BF).view(255, 256)


@pytest.mark.parametrize("path", ["general", "fast128", "fast256", "pp", "skinny"])
def test_gelu_sweep_every_finite_bf16(path):
    """X [255, 256] holds all 65,280 finite bf16 values and B = I, so the pre-activation is x itself (-0 arrives as +0).
    GELU:  |got - want| <= 1/2 ulp_bf16(max(|got|, |want|)) + c |x|;  GELU': ... + c;  c = 1.5e-7 (GELU_C), with an absolute floor of
    2^-126 in case subnormals are flushed -- measured: none of the five kernels flushes a subnormal bf16 pre-activation (0 of 254
    stored as zero on each).  Prints the worst excess over 1/2 ulp (in units of |x|, resp. absolute); measured 1.45e-8 |x| for GELU
    and 5.9e-10 for GELU' on every path.  The ends where x x overflows inside the exponential and v_rcp_f32 sees inf are part of the
    sweep."""
    X = all_finite_bf16()
    x = X.to(F64)
    M, N, K = 255, 256, 256
    eye = torch.eye(256, dtype=BF)
    e0 = torch.zeros(256, 256, dtype=BF)
    e0[:, 0] = 1.0  # A = B = e0 rows: every product sum is exactly 1
    blocks = [(0, 255)] if path != "skinny" else [(r, min(255, r + 64)) for r in range(0, 255, 64)]
    got = {k: torch.empty(M, N, dtype=BF) for k in ("gelu1", "gelu2", "deriv2", "pre1", "uderiv")}
    for r0, r1 in blocks:
        m = r1 - r0
        Xg, Ig = gx.embed(X[r0:r1], fill="nan", device=DEV), gx.embed(eye, fill="inf", device=DEV)
        Og, Ug = gx.embed(e0[:m], fill="nan", device=DEV), gx.embed(e0, fill="nan", device=DEV)
        o1, p1, o2, p2, o3 = (fresh_out(m, N) for _ in range(5))
        with forced(path) as f:
            ops().gemm(Xg.view, Ig.view, m, N, K, act=1, out=o1.view, out_pre=p1.view)
            ops().gemm(Xg.view, Ig.view, m, N, K, act=2, out=o2.view, out_pre=p2.view)
            ops().gemm(Og.view, Ug.view, m, N, K, dgelu_u=Xg.view, out=o3.view)
            torch.cuda.synchronize()
        check_ran(f.records, path, m, n=3)
        for k, g in (("gelu1", o1), ("pre1", p1), ("gelu2", o2), ("deriv2", p2), ("uderiv", o3)):
            g.check(f"{path} sweep {k}")
            got[k][r0:r1] = g.view.cpu()
    sub = (x.abs() < 2.0 ** -126) & (x != 0)
    flushed = int((got["pre1"].to(F64)[sub] == 0).sum())
    print(f"\n   [{path}] subnormal pre-activations stored as zero: {flushed} of {int(sub.sum())}")
    normal = ~sub
    assert torch.equal(got["pre1"][normal], X[normal]), "out_pre must be x itself"
    want_g, want_d = gx.gelu64(x), gx.dgelu64(x)
    nz = x != 0
    worst = {}
    for k in ("gelu1", "gelu2"):
        g = got[k].to(F64)
        err = (g - want_g).abs()
        half = 0.5 * gx.bf16_ulp(torch.maximum(g.abs(), want_g.abs()))
        worst[k] = float((((err - half - FLOOR).clamp_min(0.0))[nz] / x.abs()[nz]).max())
        bad = ~(err <= gelu_bound(g, want_g, x))
        assert not bool(bad.any()), (f"{path} {k}: {int(bad.sum())} values outside the bound, worst excess {worst[k]:.3g} |x| "
                                     f"at x = {x[bad][0].item()!r}: got {g[bad][0].item()!r}, want {want_g[bad][0].item()!r}")
    for k in ("deriv2", "uderiv"):
        g = got[k].to(F64)
        err = (g - want_d).abs()
        half = 0.5 * gx.bf16_ulp(torch.maximum(g.abs(), want_d.abs()))
        worst[k] = float((err - half - FLOOR).clamp_min(0.0).max())
        bad = ~(err <= dgelu_bound(g, want_d))
        assert not bool(bad.any()), (f"{path} {k}: {int(bad.sum())} values outside the bound, worst excess {worst[k]:.3g} "
                                     f"at x = {x[bad][0].item()!r}: got {g[bad][0].item()!r}, want {want_d[bad][0].item()!r}")
    print(f"   [{path}] worst excess over 1/2 ulp: GELU act=1 {worst['gelu1']:.3g} |x|, act=2 {worst['gelu2']:.3g} |x|; "
          f"GELU' saved by act=2 {worst['deriv2']:.3g}, from dgelu_u {worst['uderiv']:.3g}  (bound {GELU_C:.3g})")


# ======================================================================================================================================
# d. the medium training step's launch configurations (one B = 128 micro-batch: 192,000 encoder tokens, 57,344 decoder rows of which a
#    span step keeps 18,944 = 64 x 296; 18,752 = 64 x 293 is a span-step row count with M % 256 == 64)
# ======================================================================================================================================
def wgrad_config(tokens, N, K):
    """(split_k, atomic_on_pp) as Runner::wgrad (csrc/engine_gemm.h, csrc/train_plan_host.cpp) configures dW[N, K] over ``tokens`` rows: the split that minimises
    (K-tiles per split + 16 + split) x waves of the 768 resident 256 x 128 workgroups, or the ping-pong kernel's table -- 192k tokens:
    [1024 x 1024] split 16, [4096 x 1024] 8, [1024 x 4096] 4, [2048 x 1024] 8; 57k tokens: the two 4:1 shapes split 4."""
    tiles, kt = ((N + 255) // 256) * ((K + 127) // 128), (tokens + 63) // 64
    split, best = 1, 1e30
    for s_ in (1, 2, 4, 8, 16, 24, 32):
        if s_ > 1 and (kt // s_ < 8 or tiles >= 768):
            break
        w, per = tiles * s_, kt / s_ + 16.0 + s_
        waves = 0.7 + 0.3 * w / 768.0 if w <= 768 else float(-(-w // 768))
        if per * waves < 0.97 * best:
            best, split = per * waves, s_
    if tokens >= 40000 and N % 256 == 0 and K % 256 == 0:
        t256, long_tokens = (N // 256) * (K // 256), tokens >= 150000
        pp = 16 if (t256 == 16 and long_tokens) else ((8 if (long_tokens and N > K) else 4) if t256 == 64 else (8 if (t256 == 32 and long_tokens) else 0))
        if pp:
            return pp, 1
    return split, 0


ENC, DEC, SPAN, SPAN64 = 192000, 57344, 64 * 296, 64 * 293
# (kind, expected kernel family, layout or epilogue, (M, N, K)).  One M per launch configuration -- with both an M % 256 == 0 and an
# M % 256 == 64 row count per configuration this file cost several times what tests/test_gpu_ops.py does; the configurations only the
# decoder launches run at the span step's M % 256 == 64 row count, the ones the encoder shares at its 192,000 rows (M % 256 == 0).
PRODUCTION = (
    [("R", "pp", "NT", (SPAN64, 51968, 1024))] +                                             # tied logits
    [("S", "pp", "bias", (SPAN64, 1024, 1024))] +                                            # cross-attention query (automatic stagger)
    [("S", "pp", "bias", (ENC, 2048, 1024))] +                                               # cross-attention key | value
    [("S", "pp", "bias", (ENC, 3072, 1024))] +                                               # q | k | v
    [("S", "pp", "bias_resid", (ENC, 1024, 1024))] +                                         # attention output projection (stagger)
    [("S", "pp", "bias_resid", (SPAN64, 1024, 4096))] +                                      # mlp.2
    [("S", "pp", "bias_act2", (ENC, 4096, 1024))] +                                          # mlp.0, training
    [("S", "pp", "bias_act1_pre", (2 * ENC, 1024, 256)), ("S", "general", "bias_act1_pre", (128, 1024, 256))] +      # conv1 (+ edge rows)
    [("S", "pp", "bias_act1_pre_pos", (ENC, 1024, 3072)), ("S", "general", "bias_act1_pre_pos", (128, 1024, 3072))] +  # conv2 + positions
    [("R", "pp", "NN", (SPAN64, 1024, 1024))] +                                              # dgrads
    [("R", "pp", "NN", (ENC, 1024, 2048))] +
    [("R", "pp", "NN", (ENC, 1024, 3072))] +
    [("R", "pp", "NN", (SPAN64, 1024, 4096))] +
    [("R", "pp", "NN", (SPAN64, 1024, 51968))] +
    [("R", "pp", "NN", (ENC, 3072, 1024))] +
    [("S", "pp", "resid", (ENC, 1024, 2048))] +                                              # d(xa) accumulating over the decoder layers
    [("S", "pp", "u_deriv", (SPAN64, 4096, 1024))] +                                         # dgrad through GELU' + fused bias gradient
    # weight gradients dW[N_w, K_w] over `tokens` rows, configured as Runner::wgrad does: (tokens, N_w, K_w)
    [("W", fam, "TT", shape) for fam, shape in (
        ("pp", (ENC, 1024, 1024)), ("pp", (ENC, 4096, 1024)), ("pp", (ENC, 1024, 4096)), ("pp", (ENC, 2048, 1024)),
        ("fast128", (ENC, 3072, 1024)), ("fast128", (ENC, 1024, 3072)), ("fast128", (2 * ENC, 1024, 256)),
        ("fast128", (DEC, 1024, 1024)), ("pp", (DEC, 4096, 1024)), ("pp", (DEC, 1024, 4096)),
        ("fast128", (SPAN, 1024, 1024)), ("fast128", (SPAN, 4096, 1024)), ("fast128", (SPAN, 1024, 4096)),
        ("fast128", (SPAN, 3072, 1024)), ("fast128", (SPAN, 51864, 1024)), ("general", (SPAN, 1, 1024)))] +
    # the conv stems' rank-B corrections: alpha = -1 over the B = 128 edge rows
    [("C", "fast128", "TT", (1024, 80, 128)), ("C", "fast128", "TT", (1024, 1024, 128))]
)
RAN = set()


def run_production(i):
    kind, fam, what, shape = PRODUCTION[i]
    big = shape[0] * shape[1] > 1 << 22
    if kind == "R":
        run_rounding(fam, what, shape, big=big, auto=True)
    elif kind == "S":
        colsum = "scratch" if what == "u_deriv" else None  # Runner::dgrad always passes colsum_scratch with colsum
        recs = run_epilogue(fam, what, shape, colsum=colsum, big=big, auto=fam != "general", pos_period=1500 if shape[0] == ENC else 100)
        check_ran(recs, fam, shape[0], csum=(colsum is not None) if fam == "pp" else None)
        assert recs[0]["flags"] & 1023 == epilogue_flags(EPILOGUES[what][1])
        assert recs[0]["scratch"] == int(colsum is not None)
        auto_stagger = shape[0] >= 16384 and shape[1] <= 1024 and shape[2] <= 1024  # launch_gemm's rule for short tiles
        assert (recs[0]["stagger"], recs[0]["stagger_phases"]) == ((1, 8) if auto_stagger else (0, 0)), recs[0]
    elif kind == "W":
        tokens, Nw, Kw = shape
        split, on_pp = wgrad_config(tokens, Nw, Kw)
        recs = run_atomic(fam, what, (Nw, Kw, tokens), split, big=True, auto=True, atomic_on_pp=on_pp)
        assert (recs[0]["split_k"], recs[0]["atomic_on_pp"]) == (split, on_pp)
    else:
        run_atomic(fam, what, shape, 1, auto=True, alpha=-1.0)
    RAN.add(i)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("i", range(len(PRODUCTION)), ids=_ids(PRODUCTION))
def test_production_configuration(i):
    """Full-output comparison at the step's own (M, N, K), no path forced: the case names the kernel launch_gemm must choose."""
    run_production(i)


# ======================================================================================================================================
# e. ledger
# ======================================================================================================================================
def test_ledger_the_step_launches_nothing_the_suite_does_not_cover():
    """One medium B = 128 default (span) training step with launch records on: every (kernel symbol, epilogue flags, N, K, split_k,
    atomic_on_pp, stagger) it launches is the key of a case above.  A new engine configuration fails here, with the missing key printed,
    until an exact case is added for it."""
    from olmoasr_amd import _native as N
    from olmoasr_amd.config.model_dims import VARIANT_TO_DIMS
    from olmoasr_amd.model import OLMoASR
    from olmoasr_amd.synth import synth_samples
    for i in range(len(PRODUCTION)):  # (run alone, this test runs the cases it compares with itself)
        if i not in RAN:
            run_production(i)
    torch.cuda.empty_cache()
    B = 128
    net = OLMoASR(VARIANT_TO_DIMS["medium"], device=DEV, seed=0)
    try:
        pcm, ti, ty, tl = synth_samples(list(range(B)), DEV)
        mel = ops().log_mel(pcm)
        net.zero_grad()
        N.lib().oasr_profile_gemm(1)
        try:
            net.loss_and_backward(mel, ti, ty, tl, loss_scale=1024.0, span=True)
            torch.cuda.synchronize()
            recs = ops().gemm_launch_records()
        finally:
            N.lib().oasr_profile_gemm(0)
    finally:
        net._workspace = None
        del net
        torch.cuda.empty_cache()
    assert len(recs) > 500
    step = {}
    for r in recs:
        step.setdefault(ledger_key(r), set()).add(r["M"])
    missing = {k: sorted(v) for k, v in step.items() if k not in COVERED}
    print(f"\n   span step: {len(recs)} GEMM launches, {len(step)} distinct configurations, {len(missing)} without an exact case")
    assert not missing, "launched by the step but covered by no exact case (symbol, flags, N, K, split_k, atomic_on_pp, stagger) -> M: " + repr(missing)
