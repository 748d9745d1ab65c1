"""Power test of tests/lora_cases.py (no GPU): the restated tiling of csrc/lora.hip passes every checker at every case, each deliberate
flaw is rejected at every case whose shape contains its path, and the operand ranges make the references exact."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lora_cases as L  # noqa: E402
from gemm_exact import rne_bf16  # noqa: E402

GRAD_IDS = [L.case_id(c) for c in L.GRAD_CASES]
MERGE_IDS = [L.case_id(c) for c in L.MERGE_CASES]

# flaw -> the cases whose shape contains the broken path (written out; held to lora_cases.flaw_applies below)
CONTAINS = {
    "slab_tail_columns_dropped": ["1x4x1", "33x260x3", "127x252x17", "160x516x64", "384x384x64"],
    "last_row_of_a_sub_batch_dropped": GRAD_IDS,
    "last_row_group_not_reduced": ["129x256x16", "160x516x64", "384x384x64"],
    "k_read_with_the_wrong_stride": [i for i in GRAD_IDS if i != "1x4x1"],
    "accumulate_is_an_overwrite": GRAD_IDS,
    "scale_is_a_separate_multiply_and_add": GRAD_IDS,
    "product_rounded_to_bf16_before_w0": MERGE_IDS,
    "last_row_unwritten_when_rows_mod_4": ["1x4x1", "5x1028x3", "7x2048x17"],
}


def rejected(check, *args, **kw):
    try:
        check(*args, **kw)
    except AssertionError:
        return True
    return False


def test_the_listed_cases_are_the_ones_that_contain_each_path():
    for flaw in L.GRAD_FLAWS:
        assert CONTAINS[flaw] == [L.case_id(c) for c in L.GRAD_CASES if L.flaw_applies(flaw, c)], flaw
    for flaw in L.MERGE_FLAWS:
        if flaw != "scale_is_a_separate_multiply_and_add":
            assert CONTAINS[flaw] == [L.case_id(c) for c in L.MERGE_CASES if L.flaw_applies(flaw, c)], flaw
    # every tile edge the kernels have is met by some case
    assert any(r % L.GRAD_SUB == 1 for r, _, _ in L.GRAD_CASES) and any(r % L.GRAD_RG == 1 for r, _, _ in L.GRAD_CASES)
    assert any(r % L.GRAD_RG == L.GRAD_SUB for r, _, _ in L.GRAD_CASES) and any(c % L.GRAD_SLAB == 4 for _, c, _ in L.GRAD_CASES)
    assert {1, L.MAX_RANK} <= {k for _, _, k in L.GRAD_CASES} and any(256 % k for _, _, k in L.GRAD_CASES)
    assert any(r % L.MERGE_ROWS == 1 for r, _, _ in L.MERGE_CASES) and any(c == L.MERGE_COLS + 4 for _, c, _ in L.MERGE_CASES)


def test_operand_ranges_make_the_references_exact():
    for rows, cols, r in L.GRAD_CASES + L.MERGE_CASES:
        assert L.assert_integer_ranges(rows, cols, r, max(rows, cols)) == 9 * max(rows, cols) < 2 ** 24
    # float64(32/3) * sum + x0: 24 bits x 15 bits, plus an integer 20 binary places above the product's last one
    bits = L.f64_is_exact(L.S_THIRDS, 9 * 2048, 2048)
    assert bits <= 24 + 15 and bits < 53
    assert float(torch.tensor(L.S_THIRDS, dtype=torch.float32)) == L.S_THIRDS and L.S_THIRDS != 32.0 / 3.0
    with pytest.raises(AssertionError):
        L.f64_is_exact(L.S_THIRDS, 2 ** 30, 2048)  # the assertion can fail
    with pytest.raises(AssertionError):
        L.f64_is_exact(32.0 / 3.0, 9, 0)           # not an fp32 value
    # fma32 rounds once: against exact rational arithmetic on a few integer sums
    from fractions import Fraction
    for acc, x0 in ((18431, -2047), (-7, 2048), (3455, 1), (1, -1)):
        exact = Fraction(L.S_THIRDS) * acc + x0
        got = float(L.fma32(L.S_THIRDS, torch.tensor([acc]), torch.tensor([float(x0)]))[0])
        lo, hi = sorted((got, float(torch.nextafter(torch.tensor(got), torch.tensor(float("inf") if exact > Fraction(got) else -float("inf"))))))
        assert abs(Fraction(got) - exact) <= abs(Fraction(hi) - Fraction(lo)) / 2, (acc, x0)


@pytest.mark.parametrize("case", L.GRAD_CASES, ids=GRAD_IDS)
def test_grad_restatement_passes_and_every_flaw_is_rejected(case):
    op = L.grad_int_operands(case)
    caught = {f: [] for f in L.GRAD_FLAWS}
    # exact integers, every scale; the restatement's scratch starts as NaN (an unwritten partial would show), the flawed ones' as zero
    # (a flaw must be seen by the VALUE it leaves, not by the poison)
    for name, s in L.SCALES.items():
        want = L.grad_int_reference(op, s)
        L.check_grad_exact(*L.tiled_grad(op["dW"], op["A"], op["B"], s, op["dA0"], op["dB0"]), want, name)
        for flaw in L.GRAD_FLAWS:
            if L.flaw_applies(flaw, case):
                got = L.tiled_grad(op["dW"], op["A"], op["B"], s, op["dA0"], op["dB0"], flaw=flaw, scratch_fill=0.0)
                if rejected(L.check_grad_exact, *got, want):
                    caught[flaw].append("int " + name)
    # the double rounding: rejected at 32/3 only, and on a non-zero share of the elements of these operands
    assert caught["scale_is_a_separate_multiply_and_add"] == ["int 32/3"], caught
    sA, sB = L.grad_int_sums(op)
    two = (L.mul_then_add32(L.S_THIRDS, sA, op["dA0"]), L.mul_then_add32(L.S_THIRDS, sB, op["dB0"]))
    one = L.grad_int_reference(op, L.S_THIRDS)
    share = [float((two[j] != one[j]).float().mean()) for j in (0, 1)]
    print(f"{L.case_id(case)}: a separate multiply and add differs on {share[0]:.1%} of dA and {share[1]:.1%} of dB")
    assert max(share) > 0
    # planted entries at every position
    A, B = L.planted_operands(case)
    zA, zB = torch.zeros_like(A), torch.zeros_like(B)
    rows, cols, r = case
    positions = L.planted_positions(rows, cols)
    for name, s in L.SCALES.items():
        for o, i in positions:
            dW = L.planted_dw(rows, cols, o, i)
            L.check_planted(*L.tiled_grad(dW, A, B, s, zA, zB), A, B, o, i, s)
    structural = L.GRAD_FLAWS[:4]
    for flaw in structural:
        if L.flaw_applies(flaw, case):
            hits = [(o, i) for o, i in positions
                    if rejected(L.check_planted, *L.tiled_grad(L.planted_dw(rows, cols, o, i), A, B, 2.0, zA, zB, flaw=flaw, scratch_fill=0.0), A, B, o, i, 2.0)]
            if hits:
                caught[flaw].append(f"planted at {hits[0]}")
    # floats within the derived bound; the flaws far outside it
    fo = L.grad_float_operands(case)
    ref, bound = L.projection_reference(fo["dW"], fo["A"], fo["B"], L.S_THIRDS, fo["dA0"], fo["dB0"])
    got = L.tiled_grad(fo["dW"], fo["A"], fo["B"], L.S_THIRDS, fo["dA0"], fo["dB0"])
    wa = L.check_bound(got[0], ref[0], bound[0], "dA", "k, i")
    wb = L.check_bound(got[1], ref[1], bound[1], "dB", "o, k")
    print(f"{L.case_id(case)}: the fp32 restatement uses {wa:.3f} (dA) and {wb:.3f} (dB) of the derived bound")
    for flaw in L.GRAD_FLAWS[:5]:
        if L.flaw_applies(flaw, case):
            bad = L.tiled_grad(fo["dW"], fo["A"], fo["B"], L.S_THIRDS, fo["dA0"], fo["dB0"], flaw=flaw, scratch_fill=0.0)
            if rejected(L.check_bound, bad[0], ref[0], bound[0], "dA", "k, i") or rejected(L.check_bound, bad[1], ref[1], bound[1], "dB", "o, k"):
                caught[flaw].append("float bound")
    # every flaw whose path the shape contains: rejected by the exact-integer check at EVERY scale it can show at, the structural ones by
    # a plant as well, all but the double rounding by the float bound too
    for flaw in L.GRAD_FLAWS:
        if not L.flaw_applies(flaw, case):
            assert L.case_id(case) not in CONTAINS[flaw]
            continue
        assert L.case_id(case) in CONTAINS[flaw]
        if flaw == "scale_is_a_separate_multiply_and_add":
            continue
        assert [c for c in caught[flaw] if c.startswith("int")] == ["int 2", "int 0.5", "int 32/3"], (flaw, caught[flaw])
        assert "float bound" in caught[flaw], (flaw, caught[flaw])
        if flaw in structural:
            assert any(c.startswith("planted") for c in caught[flaw]), (flaw, caught[flaw])


def test_the_checkers_name_the_offending_element():
    case = (33, 260, 3)
    op = L.grad_int_operands(case)
    want = L.grad_int_reference(op, 2.0)
    dA, dB = want[0].clone(), want[1].clone()
    dB[32, 2] += 1
    with pytest.raises(AssertionError, match=r"dB: 1 of 99 elements differ; first at \(o, k\) = \(32, 2\)"):
        L.check_grad_exact(dA, dB, want)
    dA[1, 259] = float("nan")
    with pytest.raises(AssertionError, match=r"dA: 1 of 780 elements differ; first at \(k, i\) = \(1, 259\)"):
        L.check_grad_exact(dA, None, want)
    L.check_grad_exact(None, want[1], want)  # a frozen half is not compared
    A, B = L.planted_operands(case)
    o, i = 32, 256
    gA, gB = L.tiled_grad(L.planted_dw(33, 260, o, i), A, B, 2.0, torch.zeros_like(A), torch.zeros_like(B))
    L.check_planted(gA, gB, A, B, o, i, 2.0)
    gB[31, 0] = 2.0 ** -20  # a leak into the row next to the plant, far below any norm-relative tolerance
    with pytest.raises(AssertionError, match=r"plant at \(o, i\) = \(32, 256\): dB.*\(o, k\) = \(31, 0\)"):
        L.check_planted(gA, gB, A, B, o, i, 2.0)
    # the bound checker: NaN and a non-zero value where the bound is zero are failures, not skips
    ref, bound = torch.zeros(2, 2, dtype=torch.float64), torch.zeros(2, 2, dtype=torch.float64)
    assert L.check_bound(torch.zeros(2, 2), ref, bound, "z", "a, b") == 0.0
    for bad in (float("nan"), 1e-30):
        g = torch.zeros(2, 2)
        g[1, 0] = bad
        with pytest.raises(AssertionError, match=r"\(a, b\) = \(1, 0\)"):
            L.check_bound(g, ref, bound, "z", "a, b")


def test_planted_positions_cover_every_boundary():
    for rows, cols, _ in L.GRAD_CASES:
        pos = L.planted_positions(rows, cols)
        rs, cs = {o for o, _ in pos}, {i for _, i in pos}
        assert all(0 <= o < rows and 0 <= i < cols for o, i in pos)
        assert {(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1)} <= set(pos)
        for b in range(L.GRAD_SUB, rows, L.GRAD_SUB):  # (every row-group boundary is one of these)
            assert {b - 1, b} <= rs, (rows, b)
        for b in range(L.GRAD_SLAB, cols, L.GRAD_SLAB):
            assert {b - 1, b} <= cs, (cols, b)
        assert len(pos) <= 40
    assert {127, 128, 255, 256, 383} <= {o for o, _ in L.planted_positions(384, 384)}
    assert {255, 256, 511, 512, 767, 768, 1023} <= {i for _, i in L.planted_positions(64, 1024)}


@pytest.mark.parametrize("case", L.MERGE_CASES, ids=MERGE_IDS)
def test_merge_restatement_passes_and_every_flaw_is_rejected(case):
    op = L.merge_int_operands(case)
    caught = {f: [] for f in L.MERGE_FLAWS}
    for name, s in L.SCALES.items():
        w32, w16 = L.merge_reference(op, s)
        n, up, down = L.assert_ties(case, w32)
        print(f"{L.case_id(case)} s = {name}: {n} exact bf16 ties of {w32.numel()} outputs ({up} rounded away from zero, {down} towards)")
        # torch's conversion is round-to-nearest-even: against the integer arithmetic of gemm_exact.rne_bf16
        assert torch.equal(w16.view(torch.int16), rne_bf16(w32).view(torch.int16))
        L.check_exact(L.tiled_merge(op["W0"], op["A"], op["B"], s, False), w32, name + " f32", "o, i")
        L.check_exact(L.tiled_merge(op["W0"], op["A"], op["B"], s, True), w16, name + " bf16", "o, i")
        for flaw in L.MERGE_FLAWS:
            if L.flaw_applies(flaw, case):
                for bf16, want in ((False, w32), (True, w16)):
                    if rejected(L.check_exact, L.tiled_merge(op["W0"], op["A"], op["B"], s, bf16, flaw=flaw), want, "", "o, i"):
                        caught[flaw].append(f"{'bf16' if bf16 else 'f32'} {name}")
    assert caught["scale_is_a_separate_multiply_and_add"] == ["f32 32/3"] or caught["scale_is_a_separate_multiply_and_add"] == ["f32 32/3", "bf16 32/3"], caught
    assert "f32 32/3" in caught["product_rounded_to_bf16_before_w0"], caught
    if L.flaw_applies("last_row_unwritten_when_rows_mod_4", case):
        assert len(caught["last_row_unwritten_when_rows_mod_4"]) == 6, caught
        assert L.case_id(case) in CONTAINS["last_row_unwritten_when_rows_mod_4"]
    # (at s = 2 and 0.5 the product s * sum of these small integers is a bf16 value already: the early rounding shows at 32/3 only)
    # a truncating conversion fails the bf16 check wherever there are ties
    if w32.numel() >= L.TIE_MIN_OUTPUTS:
        from gemm_exact import trunc_bf16
        assert rejected(L.check_exact, trunc_bf16(w32), w16, "", "o, i")
