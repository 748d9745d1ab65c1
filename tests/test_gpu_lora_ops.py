"""The two LoRA kernels of csrc/lora.hip through their unit operators (oasr_lora_merge_op, oasr_lora_grad_op), on the operands of
tests/lora_cases.py: exact integers at three scales (2, 0.5 and fp32(32/3): the single rounding of fmaf(s, sum, x0)), planted single
entries on both sides of every row-group, sub-batch and slab boundary, random floats under the derived summation bound -- from non-zero
dA0 / dB0, between guard bands, with a scratch buffer that holds NaN (or another shape's partial sums) beforehand -- and every refusal
before any launch.  Then the engine: adapters of ranks 1, 3 and 64 on all six kinds of block Linear of a one-layer width-64 model, whose
projections share one scratch between 64 x 64, 256 x 64 and 64 x 256 targets, held to the projection of the merged model's own weight
gradient.

Measured on an MI355X (printed by the tests; the bounds are derived in tests/lora_cases.py, nothing here was fitted to these):
    floats, worst |error| in units of the derived bound over the eight cases        dA 0.0825   dB 0.0154
    engine, worst over both compute dtypes, three ranks and 2 x 16 adapters         dA 0.0679   dB 0.0578
    run-to-run difference of the reference dW (two runs of the merged model)        0, bit-identical, in all six configurations
"""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lora_cases as L  # noqa: E402
from gemm_exact import SENTINEL_BF16, SENTINEL_F32  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
PAD = 256            # guard elements on each side of an output (keeps the 16-byte alignment the kernels' vector accesses need)
SCRATCH_GUARD = 4096  # guard bytes on each side of the scratch
EINVAL = -1          # csrc/common.h: OASR_EINVAL
GRAD_IDS = [L.case_id(c) for c in L.GRAD_CASES]
MERGE_IDS = [L.case_id(c) for c in L.MERGE_CASES]


def _N():
    from olmoasr_amd import _native as N
    N.lib()
    return N


class Guarded:
    """A contiguous matrix in the middle of a longer allocation whose every other element holds a sentinel bit pattern."""

    def __init__(self, shape, dtype, init=None):
        self.two = dtype == BF
        self.bits = SENTINEL_BF16 if self.two else SENTINEL_F32
        self.n = int(torch.Size(shape).numel())
        self.raw = torch.full((PAD + self.n + PAD,), self.bits, dtype=torch.int16 if self.two else torch.int32, device=DEV)
        self.view = self.raw.view(dtype)[PAD:PAD + self.n].view(shape)
        if init is not None:  # (else the matrix holds the sentinel too)
            self.view.copy_(init)

    def check(self, what):
        for side, p in (("before", self.raw[:PAD]), ("after", self.raw[PAD + self.n:])):
            bad = p != self.bits
            assert not bool(bad.any()), f"{what}: {int(bad.sum())} guard elements {side} the matrix changed; first at {int(bad.nonzero()[0])}"

    def untouched(self):
        return bool((self.raw == self.bits).all())


def _scratch(nbytes, fill=0xFF):
    return torch.full((SCRATCH_GUARD + nbytes + SCRATCH_GUARD,), fill, dtype=torch.uint8, device=DEV)


def _check_scratch_guards(buf, nbytes, what):
    assert bool((buf[:SCRATCH_GUARD] == 0xFF).all()) and bool((buf[SCRATCH_GUARD + nbytes:] == 0xFF).all()), f"{what}: the scratch guard bands changed"


def run_grad(op, s, *, dA=True, dB=True, scratch=None, what=""):
    """oasr_lora_grad_op on CPU operands ``op`` (dW, A, B, dA0, dB0): returns (dA, dB) on the CPU (None for a NULL output).  Outputs sit
    between guard bands; the scratch (``scratch``: a caller's buffer with its guard bands, else a fresh one) holds 0xFF bytes = NaN."""
    N = _N()
    rows, cols = op["dW"].shape
    r = op["A"].shape[0]
    dev = {k: op[k].to(DEV).contiguous() for k in ("dW", "A", "B")}
    gA, gB = Guarded(op["dA0"].shape, F32, op["dA0"]), Guarded(op["dB0"].shape, F32, op["dB0"])
    nbytes = N.lib().oasr_lora_grad_scratch_bytes(rows, cols, r)
    assert nbytes == 4 * (L.cdiv(rows, L.GRAD_RG) * r * cols + L.cdiv(cols, L.GRAD_SLAB) * rows * r)
    buf = _scratch(nbytes) if scratch is None else scratch
    assert buf.numel() >= nbytes + 2 * SCRATCH_GUARD
    rc = N.lib().oasr_lora_grad_op(N.ptr(dev["dW"]), N.ptr(dev["A"]), N.ptr(dev["B"]), rows, cols, r, s, N.ptr(gA.view) if dA else None,
                                   N.ptr(gB.view) if dB else None, C.c_void_p(buf.data_ptr() + SCRATCH_GUARD), N.stream_ptr())
    N.check(rc, "oasr_lora_grad_op")
    torch.cuda.synchronize()
    gA.check(what + " dA")
    gB.check(what + " dB")
    _check_scratch_guards(buf, buf.numel() - 2 * SCRATCH_GUARD, what)
    for k in ("dW", "A", "B"):
        assert torch.equal(dev[k].cpu(), op[k]), f"{what}: operand {k} changed"
    outA, outB = gA.view.cpu(), gB.view.cpu()
    if not dA:
        assert torch.equal(outA, op["dA0"]), f"{what}: a NULL dA, yet the buffer next to it changed"
    if not dB:
        assert torch.equal(outB, op["dB0"]), f"{what}: a NULL dB"
    return (outA if dA else None), (outB if dB else None)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---- lora_grad ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.GRAD_CASES, ids=GRAD_IDS)
def test_grad_exact_integers_from_a_poisoned_scratch(case):
    """Every scale: dA and dB equal the integer reference from non-zero dA0 / dB0 although the scratch held NaN, inside untouched guard
    bands; with one output NULL the other is bit-identical to the two-output run."""
    op = L.grad_int_operands(case)
    for name, s in L.SCALES.items():
        what = f"{L.case_id(case)} s = {name}"
        want = L.grad_int_reference(op, s)
        dA, dB = run_grad(op, s, what=what)
        L.check_grad_exact(dA, dB, want, what)
        onlyB = run_grad(op, s, dA=False, what=what + " (dA NULL)")
        onlyA = run_grad(op, s, dB=False, what=what + " (dB NULL)")
        assert onlyB[0] is None and torch.equal(_bits(onlyB[1]), _bits(dB)), what
        assert onlyA[1] is None and torch.equal(_bits(onlyA[0]), _bits(dA)), what


def test_grad_reuses_the_scratch_of_a_larger_target():
    """The engine's shared scratch: (160, 516, 64), then (33, 260, 3) into the same buffer without clearing it -- the reduce of the second
    reads only what its own first pass wrote."""
    N = _N()
    big, small = (160, 516, 64), (33, 260, 3)
    nbytes = N.lib().oasr_lora_grad_scratch_bytes(*big)
    assert nbytes > N.lib().oasr_lora_grad_scratch_bytes(*small)
    buf = _scratch(nbytes)
    for case in (big, small, big):
        op = L.grad_int_operands(case)
        dA, dB = run_grad(op, L.S_THIRDS, scratch=buf, what=f"{L.case_id(case)} in the shared scratch")
        L.check_grad_exact(dA, dB, L.grad_int_reference(op, L.S_THIRDS), L.case_id(case) + " in the shared scratch")
    assert bool((buf[SCRATCH_GUARD:SCRATCH_GUARD + nbytes].view(F32).isnan().logical_not()).all()), "the largest target writes its whole scratch"


@pytest.mark.parametrize("case", L.GRAD_CASES, ids=GRAD_IDS)
def test_grad_planted_entries(case):
    """One non-zero element of dW at a time: one row of dB and one column of dA are single exact products, everything else == 0."""
    rows, cols, r = case
    A, B = L.planted_operands(case)
    zA, zB = torch.zeros_like(A), torch.zeros_like(B)
    for name, s in L.SCALES.items():
        for o, i in L.planted_positions(rows, cols):
            op = dict(dW=L.planted_dw(rows, cols, o, i), A=A, B=B, dA0=zA, dB0=zB)
            what = f"{L.case_id(case)} s = {name}"
            dA, dB = run_grad(op, s, what=what)
            L.check_planted(dA, dB, A, B, o, i, s, what)


def test_grad_floats_within_the_derived_bound_and_deterministic():
    worst = [0.0, 0.0]
    for case in L.GRAD_CASES:
        op = L.grad_float_operands(case)
        ref, bound = L.projection_reference(op["dW"], op["A"], op["B"], L.S_THIRDS, op["dA0"], op["dB0"])
        dA, dB = run_grad(op, L.S_THIRDS, what=L.case_id(case))
        again = run_grad(op, L.S_THIRDS, what=L.case_id(case))
        assert torch.equal(_bits(dA), _bits(again[0])) and torch.equal(_bits(dB), _bits(again[1])), f"{case}: two runs differ"
        # print first, assert afterwards
        ua, ub = L.worst_in_bound_units(dA, ref[0], bound[0])[0], L.worst_in_bound_units(dB, ref[1], bound[1])[0]
        print(f"lora_grad {L.case_id(case):>11}: worst error {ua:.4f} (dA) and {ub:.4f} (dB) x the derived bound")
        worst = [max(worst[0], ua), max(worst[1], ub)]
        L.check_bound(dA, ref[0], bound[0], f"{case} dA", "k, i")
        L.check_bound(dB, ref[1], bound[1], f"{case} dB", "o, k")
    print(f"lora_grad floats, worst over the cases: {worst[0]:.4f} (dA) and {worst[1]:.4f} (dB) x the derived bound")


def _grad_refusal_args():
    rows, cols, r = 8, 8, 65
    t = dict(dW=torch.ones(rows, cols, device=DEV), A=torch.ones(r, cols, device=DEV), B=torch.ones(rows, r, device=DEV))
    return rows, cols, t


def test_grad_refusals_come_before_any_launch():
    N = _N()
    rows, cols, t = _grad_refusal_args()
    gA, gB = Guarded((65, cols), F32), Guarded((rows, 65), F32)  # sentinel throughout
    nbytes = 4 * 2 * 65 * 16 * 16
    buf = _scratch(nbytes)
    sc = C.c_void_p(buf.data_ptr() + SCRATCH_GUARD)
    p = {k: N.ptr(v) for k, v in t.items()}
    calls = {"cols % 4 != 0": (rows, 6, 4, N.ptr(gA.view), N.ptr(gB.view), sc),
             "rank 0": (rows, cols, 0, N.ptr(gA.view), N.ptr(gB.view), sc),
             "rank 65": (rows, cols, 65, N.ptr(gA.view), N.ptr(gB.view), sc),
             "both outputs NULL": (rows, cols, 4, None, None, sc),
             "NULL scratch": (rows, cols, 4, N.ptr(gA.view), N.ptr(gB.view), None)}
    for name, (m, n, r, a, b, s) in calls.items():
        rc = N.lib().oasr_lora_grad_op(p["dW"], p["A"], p["B"], m, n, r, 2.0, a, b, s, N.stream_ptr())
        torch.cuda.synchronize()
        assert rc == EINVAL and N.lib().oasr_last_error(), (name, rc)
        assert gA.untouched() and gB.untouched(), f"{name}: refused, yet an output changed"
        assert bool((buf == 0xFF).all()), f"{name}: refused, yet the scratch changed"
    assert N.lib().oasr_lora_grad_scratch_bytes(0, 8, 4) == 0 and N.lib().oasr_lora_grad_scratch_bytes(8, 8, 0) == 0


# ---- lora_merge --------------------------------------------------------------------------------------------------------------------------
def run_merge(op, s, out_dtype, *, in_place=False, what=""):
    """oasr_lora_merge_op on CPU operands ``op`` (W0, A, B): the merged matrix on the CPU.  in_place: out is w0 (fp32 only)."""
    N = _N()
    rows, cols = op["W0"].shape
    r = op["A"].shape[0]
    dev = {k: op[k].to(DEV).contiguous() for k in ("W0", "A", "B")}
    out = Guarded((rows, cols), out_dtype, dev["W0"] if in_place else None)
    assert not in_place or out_dtype == F32
    w0 = out.view if in_place else dev["W0"]
    rc = N.lib().oasr_lora_merge_op(N.ptr(w0), N.ptr(dev["A"]), N.ptr(dev["B"]), rows, cols, r, s, 1 if out_dtype == F32 else 0, N.ptr(out.view),
                                    N.stream_ptr())
    N.check(rc, "oasr_lora_merge_op")
    torch.cuda.synchronize()
    out.check(what)
    for k in ("A", "B") + (() if in_place else ("W0",)):
        assert torch.equal(dev[k].cpu(), op[k]), f"{what}: operand {k} changed"
    return out.view.cpu()


@pytest.mark.parametrize("case", L.MERGE_CASES, ids=MERGE_IDS)
def test_merge_exact(case):
    """Every scale: the fp32 output is the single-rounded reference, the in-place form equals it bit for bit, the bf16 output is that value
    rounded to nearest even (ties among them); guard bands and operands untouched."""
    op = L.merge_int_operands(case)
    for name, s in L.SCALES.items():
        what = f"merge {L.case_id(case)} s = {name}"
        w32, w16 = L.merge_reference(op, s)
        L.assert_ties(case, w32)
        got32 = run_merge(op, s, F32, what=what + " f32")
        L.check_exact(got32, w32, what + " f32", "o, i")
        inpl = run_merge(op, s, F32, in_place=True, what=what + " in place")
        assert torch.equal(_bits(inpl), _bits(got32)), what + ": in place differs from out of place"
        L.check_exact(run_merge(op, s, BF, what=what + " bf16"), w16, what + " bf16", "o, i")


def test_merge_refusals_come_before_any_launch():
    N = _N()
    rows, cols = 8, 8
    w0, A, B = torch.ones(rows, cols, device=DEV), torch.ones(65, cols, device=DEV), torch.ones(rows, 65, device=DEV)
    out = Guarded((rows, cols), F32)
    calls = {"cols % 4 != 0": (rows, 6, 4, 1, N.ptr(out.view)), "rank 0": (rows, cols, 0, 1, N.ptr(out.view)),
             "rank 65": (rows, cols, 65, 1, N.ptr(out.view)), "NULL out": (rows, cols, 4, 1, None),
             "out_dtype 2": (rows, cols, 4, 2, N.ptr(out.view)), "out_dtype -1": (rows, cols, 4, -1, N.ptr(out.view))}
    for name, (m, n, r, dt, o) in calls.items():
        rc = N.lib().oasr_lora_merge_op(N.ptr(w0), N.ptr(A), N.ptr(B), m, n, r, 2.0, dt, o, N.stream_ptr())
        torch.cuda.synchronize()
        assert rc == EINVAL and N.lib().oasr_last_error(), (name, rc)
        assert out.untouched(), f"{name}: refused, yet the output changed"
        assert bool((w0 == 1).all()), name


# ---- the engine: six kinds of target, one shared scratch ---------------------------------------------------------------------------------
TARGETS = ("*attn.query", "*attn.key", "*attn.value", "*attn.out", "*.mlp.0", "*.mlp.2")  # (*attn: self and cross attention)
ENGINE_RANKS = {1: 3.0, 3: 32.0, 64: 24.0}  # rank -> alpha: s = 3, 32/3, 0.375 -- none a power of two
PAD_ID = 51864
ENGINE_WORST = {}


def _dims():
    from olmoasr_amd.config.model_dims import ModelDimensions
    return ModelDimensions(80, 1500, 64, 1, 1, 503, 448, 64, 1, 1)


@pytest.fixture(scope="module")
def batch():
    g = torch.Generator().manual_seed(11)
    n = 9
    tokens = torch.randint(0, 503, (1, 448), generator=g)
    targets = torch.full((1, 448), PAD_ID)
    targets[0, :n] = torch.randint(0, 503, (n,), generator=g)
    mel = torch.randn(1, 80, 3000, generator=g) * 0.5
    return [t.to(DEV) for t in (mel, tokens, targets, torch.tensor([n]))]


def _adapted(dtype, rank, adapters=None):
    """The one-layer width-64 model with adapters on all six kinds of block Linear; lora_B random (or ``adapters``: a lora_state_dict)."""
    from olmoasr_amd import lora
    from olmoasr_amd.model import OLMoASR
    net = OLMoASR(_dims(), device=DEV, seed=0, compute_dtype=dtype)
    names = lora.add_lora(net, r=rank, alpha=ENGINE_RANKS[rank], target_modules=TARGETS, seed=1)
    assert len(names) == 16 and {tuple(net.get_submodule(n).weight.shape) for n in names} == {(64, 64), (256, 64), (64, 256)}
    if adapters is None:
        g = torch.Generator().manual_seed(100 + rank)
        with torch.no_grad():
            for n, p in net.named_parameters():
                if n.endswith(".lora_B"):
                    p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        net.refresh_shadow()
    else:
        lora.load_lora_state_dict(net, adapters)
    return net, names


def _step(net, batch):
    net.zero_grad()
    loss, _ = net.loss_and_backward(*batch)
    torch.cuda.synchronize()
    return float(loss)


@pytest.mark.parametrize("rank", list(ENGINE_RANKS), ids=[f"r{r}" for r in ENGINE_RANKS])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_engine_adapter_gradients_are_the_projection_of_the_merged_models_dw(batch, dtype, rank):
    """The adapted model's lora_A.grad / lora_B.grad lie within the derived bound of s B^T dW and s dW A^T (float64), dW being the weight
    gradient of the same step of the merged model (bit-identical compute copies); with lora_A frozen, lora_B.grad is bit-identical."""
    from olmoasr_amd import lora
    s = float(torch.tensor(ENGINE_RANKS[rank] / rank, dtype=F32))
    assert s == ENGINE_RANKS[rank] / rank or rank == 3  # (3 and 0.375 are fp32 values; 32/3 is rounded once, as the C ABI receives it)
    net, names = _adapted(dtype, rank)
    sd = lora.lora_state_dict(net)
    loss = _step(net, batch)
    got = {n: p.grad.detach().cpu().clone() for n, p in net.named_parameters() if ".lora_" in n}
    assert len(got) == 32 and all(p.grad is None for n, p in net.named_parameters() if ".lora_" not in n)
    # the reference: the same model merged, its six kinds of target weight trainable
    ref, _ = _adapted(dtype, rank, adapters=sd)
    lora.merge_lora(ref)
    for n, p in ref.named_parameters():
        p.requires_grad_(n[: -len(".weight")] in names and n.endswith(".weight"))
    runs = []
    for _ in range(2):
        loss_ref = _step(ref, batch)
        runs.append({n: ref.get_submodule(n).weight.grad.detach().cpu().clone() for n in names})
    assert abs(loss_ref - loss) <= 1e-6 * abs(loss), (loss_ref, loss)  # the same compute copies, the same forward
    delta = max(float((runs[0][n] - runs[1][n]).abs().max()) for n in names)
    print(f"engine {dtype} r = {rank}: the reference dW of two runs differs by at most {delta:g}" + (" (bit-identical)" if delta == 0 else ""))
    worst = [0.0, 0.0]
    fails = []
    for n in names:
        dW, A, B = runs[0][n], sd[n + ".lora_A"], sd[n + ".lora_B"]
        assert float(dW.abs().max()) > 0, n
        (refA, refB), (bA, bB) = L.projection_reference(dW, A, B, s)
        d = (runs[0][n] - runs[1][n]).to(F64).abs()
        bA, bB = bA + s * (B.to(F64).abs().t() @ d), bB + s * (d @ A.to(F64).abs().t())
        ua, at_a = L.worst_in_bound_units(got[n + ".lora_A"], refA, bA)
        ub, at_b = L.worst_in_bound_units(got[n + ".lora_B"], refB, bB)
        print(f"engine {dtype} r = {rank} {n:>36} {tuple(dW.shape)}: worst error {ua:.4f} (dA) and {ub:.4f} (dB) x the derived bound")
        worst = [max(worst[0], ua), max(worst[1], ub)]
        if ua > 1 or ub > 1:
            fails.append((n, ua, at_a, ub, at_b))
    ENGINE_WORST[(dtype, rank)] = worst
    print(f"engine {dtype} r = {rank}: worst over the 16 targets {worst[0]:.4f} (dA) and {worst[1]:.4f} (dB); over the runs so far "
          f"{max(w[0] for w in ENGINE_WORST.values()):.4f} and {max(w[1] for w in ENGINE_WORST.values()):.4f}")
    assert not fails, fails
    # lora_A frozen: no gradient for it, and every lora_B gradient is the all-trainable run's
    half, _ = _adapted(dtype, rank, adapters=sd)
    for n, p in half.named_parameters():
        if n.endswith(".lora_A"):
            p.requires_grad_(False)
    assert abs(_step(half, batch) - loss) <= 1e-6 * abs(loss)
    for n, p in half.named_parameters():
        if n.endswith(".lora_A"):
            assert p.grad is None, n
        elif n.endswith(".lora_B"):
            assert torch.equal(_bits(p.grad.detach().cpu()), _bits(got[n])), n
