"""Operands, references and checkers for the two LoRA kernels of csrc/lora.hip (plain torch on the CPU, no GPU needed).

    lora_merge   W[o][i]   = fmaf(s, sum_k B[o][k] A[k][i], W0[o][i])            fp32, or that value rounded once more to bf16
    lora_grad    dA[k][i] += s * sum_o B[o][k] dW[o][i]        dB[o][k] += s * sum_i dW[o][i] A[k][i]        (A [r, cols], B [rows, r])

Both document a fixed summation order and ONE final rounding, fmaf(s, sum, x0), so a correct kernel has one right answer on the operands
built here.  Four kinds of operands:

  exact integers   dW, A, B uniform in [-3, 3], W0 / dA0 / dB0 uniform in [-2048, 2048], stored as fp32.  With rows <= 384 and
                   cols <= 2048 every partial sum is an integer below 2^24 (|sum| <= 9 * 2048), exact in fp32 IN ANY ORDER; the reference is
                   integer arithmetic.  s = 2 and s = 0.5 give integers / half-integers; s = fp32(32/3) gives float64(s) * sum + x0, which
                   is exact in float64 (``f64_is_exact`` asserts it from the operand ranges) and is rounded ONCE to fp32 -- what fmaf
                   returns.  A separate multiply and add rounds twice and differs on a fraction of the elements (the CPU test shows it is
                   never zero).  One column in sixteen of the merge's A is zero, so W = W0 there whatever the scale.
  bf16 merge       the exact fp32 value rounded to nearest even by CPU torch.  |W| reaches 4096, where bf16 values are 16 - 32 apart, so
                   ties occur by themselves: ``tie_stats`` counts them, and every case with at least 4096 outputs holds at least 16 with
                   both rounding directions among them ((1, 4, 1) has four outputs in all).
  planted          dW is zero except for v = 3 at one (o, i); A, B hold non-zero multiples of 1/8 in [-4, 4]; dA0 = dB0 = 0.  Then
                   dB[o][k] = s v A[k][i] and dA[k][i] = s v B[o][k] are single exact products and EVERYTHING else is exactly zero.  The
                   positions (``planted_positions``): the four corners, both sides of every sub-batch boundary (31 | 32, which includes
                   the row-group boundaries 127 | 128), both sides of every slab boundary (255 | 256), the last row and column.
  floats           randn operands, s = fp32(32/3), non-zero dA0 / dB0, float64 reference, and the textbook bound of an fp32 FMA summation
                   of n terms in any order plus the final fused scale-and-add, u = 2^-24:
                       |dA - ref| <= (rows + ceil(rows / 128) + 4) u (s |B|^T |dW| + |dA0|)
                       |dB - ref| <= (cols + ceil(cols / 256) + 4) u (s |dW| |A|^T + |dB0|)
                   derived, not measured: the kernel gets no margin on top.

``tiled_grad`` / ``tiled_merge`` restate the documented tiling (row groups of 128, sub-batches of 32, slabs of 256, then the reduce; 4 rows
x 1024 columns per merge workgroup) with one deliberate flaw at a time (``GRAD_FLAWS``, ``MERGE_FLAWS``); tests/test_lora_cases_cpu.py
shows that the restatement passes every checker and that every flaw is rejected at every case whose shape contains its path.
"""
import math

import torch

from gemm_exact import bf16_ulp, matmul_int, trunc_bf16

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
MERGE_ROWS, MERGE_COLS = 4, 1024                # csrc/lora.hip: rows per workgroup, columns per blockIdx.y
GRAD_RG, GRAD_SUB, GRAD_SLAB = 128, 32, 256     # csrc/lora.hip: row group, sub-batch, column slab
MAX_RANK = 64                                   # include/oasr.h: OASR_LORA_MAX_RANK
U = 2.0 ** -24

# (rows, cols, rank): the smallest shapes at which each index path first changes
GRAD_CASES = [(1, 4, 1), (33, 260, 3), (129, 256, 16), (127, 252, 17), (128, 512, 8), (160, 516, 64), (384, 384, 64), (64, 1024, 5)]
MERGE_CASES = [(1, 4, 1), (5, 1028, 3), (4, 1024, 64), (7, 2048, 17), (384, 384, 16)]
S_THIRDS = float(torch.tensor(32.0 / 3.0, dtype=F32))  # the fp32 value the C ABI receives
SCALES = {"2": 2.0, "0.5": 0.5, "32/3": S_THIRDS}
AMP, AMP0 = 3, 2048       # |dW|, |A|, |B| <= AMP; |W0|, |dA0|, |dB0| <= AMP0
PLANT = 3.0
MIN_TIES, TIE_MIN_OUTPUTS = 16, 4096


def cdiv(a, b):
    return (a + b - 1) // b


def case_id(case):
    return "x".join(str(v) for v in case)


# (1, 4, 1) has five gradient outputs and four merged ones, and a double rounding shows on a few per cent of the elements: its integer
# draws are the first at which those few elements tell every flaw apart (tests/test_lora_cases_cpu.py holds every case to that, this one
# included).  (case, salt) -> shift of the seed
SEED_SHIFT = {((1, 4, 1), 1): 24, ((1, 4, 1), 4): 36}


def _seed(case, salt):
    rows, cols, r = case
    return (rows * 1000003 + cols * 1009 + r) * 16 + salt + 65536 * SEED_SHIFT.get((case, salt), 0)


def _ints(gen, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).to(F32)


# ---- what makes the references exact -------------------------------------------------------------------------------------------------
def f64_is_exact(s, max_sum, max_x0):
    """float64(s) * sum + x0 for integers |sum| <= max_sum, |x0| <= max_x0 and an fp32 s is an integer multiple of s's last place: it
    is exact in float64 when that integer stays below 2^53.  Returns the number of bits it needs."""
    m, e = math.frexp(s)
    k = m * 2.0 ** 24
    assert k == int(k), "s must be an fp32 value"
    lsb = e - 24  # s = k * 2^lsb
    total = int(abs(k)) * int(max_sum) + (int(max_x0) << -lsb if lsb < 0 else int(max_x0))
    bits = total.bit_length()
    assert bits < 53, (s, max_sum, max_x0, bits)
    return bits


def assert_integer_ranges(rows, cols, r, terms):
    """From the operand ranges alone: every partial sum of ``terms`` products stays below 2^24 (exact in fp32 in any order), the s = 2 and
    s = 0.5 results are fp32 values, and the 32/3 reference is exact in float64."""
    assert rows <= 384 and cols <= 2048 and 1 <= r <= MAX_RANK
    max_sum = AMP * AMP * terms
    assert max_sum < 2 ** 24
    for s in (2.0, 0.5):
        assert 2 * (s * max_sum + AMP0) < 2 ** 24  # (a half-integer below 2^23 has 24 significant bits at the most)
    f64_is_exact(S_THIRDS, max_sum, AMP0)
    return max_sum


def fma32(s, acc, x0):
    """fmaf(s, acc, x0) on fp32 tensors: the float64 value (exact for the integer and planted operands, see f64_is_exact) rounded once."""
    return (acc.to(F64) * s + x0.to(F64)).to(F32)


def mul_then_add32(s, acc, x0):
    """The double rounding fmaf avoids: fp32(s * acc), then fp32(. + x0)."""
    return (acc.to(F32) * s).to(F32) + x0.to(F32)


# ---- lora_grad: exact integers ---------------------------------------------------------------------------------------------------------
def grad_int_operands(case):
    rows, cols, r = case
    g = torch.Generator().manual_seed(_seed(case, 1))
    return dict(dW=_ints(g, -AMP, AMP, (rows, cols)), A=_ints(g, -AMP, AMP, (r, cols)), B=_ints(g, -AMP, AMP, (rows, r)),
                dA0=_ints(g, -AMP0, AMP0, (r, cols)), dB0=_ints(g, -AMP0, AMP0, (rows, r)))


def grad_int_sums(op):
    """(sum_o B[o][k] dW[o][i] [r, cols], sum_i dW[o][i] A[k][i] [rows, r]) as int64, with the exactness preconditions asserted."""
    rows, cols = op["dW"].shape
    r = op["A"].shape[0]
    assert_integer_ranges(rows, cols, r, max(rows, cols))
    for k in ("dW", "A", "B"):
        assert float(op[k].abs().max()) <= AMP and torch.equal(op[k], op[k].round())
    for k in ("dA0", "dB0"):
        assert float(op[k].abs().max()) <= AMP0 and torch.equal(op[k], op[k].round())
    sA = matmul_int(op["B"].t().contiguous(), op["dW"].t().contiguous())
    sB = matmul_int(op["dW"], op["A"])
    assert int(sA.abs().max()) < 2 ** 24 and int(sB.abs().max()) < 2 ** 24
    return sA, sB


def grad_int_reference(op, s):
    """(dA, dB) fp32: float64(s) * integer sum + x0, exact in float64, rounded once."""
    sA, sB = grad_int_sums(op)
    dA, dB = fma32(s, sA, op["dA0"]), fma32(s, sB, op["dB0"])
    if s in (2.0, 0.5):  # nothing was rounded at all
        assert torch.equal(dA.to(F64), sA.to(F64) * s + op["dA0"].to(F64)) and torch.equal(dB.to(F64), sB.to(F64) * s + op["dB0"].to(F64))
    return dA, dB


def first_difference(got, want):
    """None when ``got`` equals ``want`` element for element (NaN equals nothing), else (index tuple, got, want) of the first difference."""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    bad = ~(got == want)
    if not bool(bad.any()):
        return None
    at = tuple(bad.nonzero()[0].tolist())
    return at, float(got[at]), float(want[at]), int(bad.sum())


def check_exact(got, want, what, index_names):
    d = first_difference(got.cpu(), want)
    assert d is None, f"{what}: {d[3]} of {want.numel()} elements differ; first at ({index_names}) = {d[0]}: got {d[1]!r}, want {d[2]!r}"


def check_grad_exact(dA, dB, want, what=""):
    """dA [r, cols], dB [rows, r] against ``want`` = (dA, dB); a None output (a frozen half) is not compared."""
    if dA is not None:
        check_exact(dA, want[0], f"{what} dA", "k, i")
    if dB is not None:
        check_exact(dB, want[1], f"{what} dB", "o, k")


# ---- lora_grad: planted single entries ---------------------------------------------------------------------------------------------------
def planted_positions(rows, cols):
    """(o, i) plants: the corners, every special row (both sides of each sub-batch boundary -- the row-group boundaries among them -- and the
    last row) and every special column (both sides of each slab boundary, the last column), each at least once."""
    rs, cs = {0, rows - 1}, {0, cols - 1}
    for b in range(GRAD_SUB, rows, GRAD_SUB):
        rs |= {b - 1, b}
    for b in range(GRAD_SLAB, cols, GRAD_SLAB):
        cs |= {b - 1, b}
    rs, cs = sorted(rs), sorted(cs)
    pos = {(o, i) for o in (0, rows - 1) for i in (0, cols - 1)}
    pos |= {(o, cs[n % len(cs)]) for n, o in enumerate(rs)}
    pos |= {(rs[(5 * n + 1) % len(rs)], i) for n, i in enumerate(cs)}
    return sorted(pos)


def planted_operands(case):
    """A [r, cols], B [rows, r]: non-zero multiples of 1/8 in [-4, 4]."""
    rows, cols, r = case
    g = torch.Generator().manual_seed(_seed(case, 2))

    def eighths(shape):
        return (torch.randint(1, 33, shape, generator=g) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).to(F32) / 8

    return eighths((r, cols)), eighths((rows, r))


def planted_dw(rows, cols, o, i):
    dW = torch.zeros(rows, cols)
    dW[o, i] = PLANT
    return dW


def check_planted(dA, dB, A, B, o, i, s, what=""):
    """Row o of dB is s v A[:, i], column i of dA is s v B[o, :] (single exact products, rounded once), everything else == 0."""
    assert f64_is_exact(s, int(PLANT * 4 * 8), 0) < 53  # (v A in eighths: an integer below 96 times 1/8)
    wantA, wantB = torch.zeros_like(A), torch.zeros_like(B)
    wantA[:, i] = fma32(s, PLANT * B[o, :], torch.zeros(()))
    wantB[o, :] = fma32(s, PLANT * A[:, i], torch.zeros(()))
    assert bool((wantA[:, i] != 0).all()) and bool((wantB[o, :] != 0).all())
    check_exact(dA, wantA, f"{what} plant at (o, i) = ({o}, {i}): dA", "k, i")
    check_exact(dB, wantB, f"{what} plant at (o, i) = ({o}, {i}): dB", "o, k")


# ---- lora_grad: floats with a derived bound ------------------------------------------------------------------------------------------------
def grad_float_operands(case):
    rows, cols, r = case
    g = torch.Generator().manual_seed(_seed(case, 3))
    return {k: torch.randn(shape, generator=g) for k, shape in (("dW", (rows, cols)), ("A", (r, cols)), ("B", (rows, r)), ("dA0", (r, cols)),
                                                                ("dB0", (rows, r)))}


def projection_reference(dW, A, B, s, dA0=None, dB0=None):
    """float64 (dA, dB) and the per-element bounds (n + 4) u mag of the module docstring.  dA0 / dB0 None: zero."""
    rows, cols = dW.shape
    dW, A, B = dW.to(F64), A.to(F64), B.to(F64)
    zA = torch.zeros(A.shape, dtype=F64) if dA0 is None else dA0.to(F64)
    zB = torch.zeros(B.shape, dtype=F64) if dB0 is None else dB0.to(F64)
    refA, refB = s * (B.t() @ dW) + zA, s * (dW @ A.t()) + zB
    magA, magB = abs(s) * (B.abs().t() @ dW.abs()) + zA.abs(), abs(s) * (dW.abs() @ A.abs().t()) + zB.abs()
    nA, nB = rows + cdiv(rows, GRAD_RG), cols + cdiv(cols, GRAD_SLAB)
    return (refA, refB), ((nA + 4) * U * magA, (nB + 4) * U * magB)


def worst_in_bound_units(got, ref, bound):
    """max |got - ref| / bound; an element whose bound is zero must be exact (it then counts as 0, else as inf).  NaN counts as inf."""
    err = (got.cpu().to(F64) - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    units = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    at = tuple((units == units.max()).nonzero()[0].tolist())
    return float(units.max()), at


def check_bound(got, ref, bound, what, index_names, extra=None):
    """Asserts |got - ref| <= bound (+ extra) everywhere; returns the worst error in units of the bound."""
    worst, at = worst_in_bound_units(got, ref, bound if extra is None else bound + extra)
    assert worst <= 1.0, f"{what}: worst error {worst:.3f} x the derived bound at ({index_names}) = {at}: got {float(got[at])!r}, reference {float(ref[at])!r}"
    return worst


# ---- lora_merge ------------------------------------------------------------------------------------------------------------------------
def merge_int_operands(case):
    rows, cols, r = case
    g = torch.Generator().manual_seed(_seed(case, 4))
    A = _ints(g, -AMP, AMP, (r, cols))
    A[:, 5::16] = 0.0  # W = W0 in these columns at every scale: integers, hence bf16 ties, at 32/3 too
    return dict(A=A, B=_ints(g, -AMP, AMP, (rows, r)), W0=_ints(g, -AMP0, AMP0, (rows, cols)))


def merge_reference(op, s):
    """(fp32, bf16): float64(s) * integer sum + W0 rounded once to fp32, and that value rounded to nearest even by torch."""
    rows, cols = op["W0"].shape
    r = op["A"].shape[0]
    assert_integer_ranges(rows, cols, r, r)
    assert float(op["A"].abs().max()) <= AMP and float(op["B"].abs().max()) <= AMP and float(op["W0"].abs().max()) <= AMP0
    acc = matmul_int(op["B"], op["A"].t().contiguous())
    w32 = fma32(s, acc, op["W0"])
    if s in (2.0, 0.5):
        assert torch.equal(w32.to(F64), acc.to(F64) * s + op["W0"].to(F64))
    return w32, w32.to(BF)


def tie_stats(w32):
    """(exact bf16 ties among the fp32 values, ties torch rounded away from zero, ties it rounded towards zero)."""
    v = w32.to(F64)
    r, t = w32.to(BF).to(F64), trunc_bf16(w32).to(F64)
    tie = (r != v) & ((v - t).abs() * 2 == bf16_ulp(v))
    return int(tie.sum()), int((tie & (r.abs() > v.abs())).sum()), int((tie & (r.abs() < v.abs())).sum())


def assert_ties(case, w32):
    n, up, down = tie_stats(w32)
    if w32.numel() >= TIE_MIN_OUTPUTS:
        assert n >= MIN_TIES and up > 0 and down > 0, (case, n, up, down)
    return n, up, down


# ---- the documented tiling, restated, with one flaw at a time -------------------------------------------------------------------------------
GRAD_FLAWS = ("slab_tail_columns_dropped", "last_row_of_a_sub_batch_dropped", "last_row_group_not_reduced", "k_read_with_the_wrong_stride",
              "accumulate_is_an_overwrite", "scale_is_a_separate_multiply_and_add")
MERGE_FLAWS = ("scale_is_a_separate_multiply_and_add", "product_rounded_to_bf16_before_w0", "last_row_unwritten_when_rows_mod_4")


def flaw_applies(flaw, case):
    """Does the case's shape contain the path the flaw breaks?"""
    rows, cols, r = case
    return {"slab_tail_columns_dropped": cols % GRAD_SLAB != 0,
            "last_row_of_a_sub_batch_dropped": True,
            "last_row_group_not_reduced": rows > GRAD_RG,
            "k_read_with_the_wrong_stride": r > 1 and rows > 1,
            "accumulate_is_an_overwrite": True,
            "scale_is_a_separate_multiply_and_add": True,   # (rejected by the 32/3 cases only)
            "product_rounded_to_bf16_before_w0": True,
            "last_row_unwritten_when_rows_mod_4": rows % MERGE_ROWS != 0}[flaw]


def tiled_grad(dW, A, B, s, dA0, dB0, flaw=None, scratch_fill=float("nan")):
    """lora_grad as csrc/lora.hip documents it, in fp32: workgroup (g, c) walks its 128 x 256 block of dW 32 rows at a time and writes
    partA[g] [r, slab] and partB[c] [rows of the group, r] into a scratch that holds ``scratch_fill`` beforehand; the reduce adds the
    partials in ascending g / c and finishes with one fmaf.  Returns (dA, dB)."""
    assert flaw is None or flaw in GRAD_FLAWS
    rows, cols = dW.shape
    r = A.shape[0]
    nG, nC = cdiv(rows, GRAD_RG), cdiv(cols, GRAD_SLAB)
    partA, partB = torch.full((nG, r, cols), scratch_fill), torch.full((nC, rows, r), scratch_fill)
    Bk = B.reshape(-1)[: rows * r].reshape(r, rows).t() if flaw == "k_read_with_the_wrong_stride" else B  # element (o, k) from k * rows + o
    for g in range(nG):
        g0, gn = g * GRAD_RG, min(GRAD_RG, rows - g * GRAD_RG)
        for c in range(nC):
            c0, cn = c * GRAD_SLAB, min(GRAD_SLAB, cols - c * GRAD_SLAB)
            if flaw == "slab_tail_columns_dropped" and cn < GRAD_SLAB:
                cn = 0
            acc = torch.zeros(r, cn)
            for s0 in range(0, gn, GRAD_SUB):
                sn = min(GRAD_SUB, gn - s0)
                if flaw == "last_row_of_a_sub_batch_dropped":
                    sn -= 1
                o0 = g0 + s0
                tile = dW[o0:o0 + sn, c0:c0 + cn]
                acc = acc + Bk[o0:o0 + sn].t() @ tile
                partB[c, o0:o0 + sn] = tile @ A[:, c0:c0 + cn].t()
            partA[g, :, c0:c0 + cn] = acc
    sumA, sumB = torch.zeros(r, cols), torch.zeros(rows, r)
    for g in range(nG - 1 if flaw == "last_row_group_not_reduced" and nG > 1 else nG):
        sumA = sumA + partA[g]
    for c in range(nC):
        sumB = sumB + partB[c]
    if flaw == "accumulate_is_an_overwrite":
        dA0, dB0 = torch.zeros_like(dA0), torch.zeros_like(dB0)
    fin = mul_then_add32 if flaw == "scale_is_a_separate_multiply_and_add" else fma32
    return fin(s, sumA, dA0), fin(s, sumB, dB0)


def tiled_merge(w0, A, B, s, bf16, flaw=None):
    """lora_merge as documented: 4 rows x 1024 columns per workgroup, the k sum in fp32, one fmaf, then (bf16) one more rounding.  The
    output starts as NaN, so an element that is never written is seen."""
    assert flaw is None or flaw in MERGE_FLAWS
    rows, cols = w0.shape
    out = torch.full((rows, cols), float("nan"))
    for o0 in range(0, rows, MERGE_ROWS):
        nrow = min(MERGE_ROWS, rows - o0)
        write = nrow - 1 if flaw == "last_row_unwritten_when_rows_mod_4" and nrow < MERGE_ROWS else nrow
        for c0 in range(0, cols, MERGE_COLS):
            acc = B[o0:o0 + nrow] @ A[:, c0:c0 + MERGE_COLS]
            w = w0[o0:o0 + nrow, c0:c0 + MERGE_COLS]
            if flaw == "product_rounded_to_bf16_before_w0":
                v = (acc * s).to(BF).to(F32) + w
            elif flaw == "scale_is_a_separate_multiply_and_add":
                v = mul_then_add32(s, acc, w)
            else:
                v = fma32(s, acc, w)
            out[o0:o0 + write, c0:c0 + MERGE_COLS] = v[:write]
    return out.to(BF) if bf16 else out
