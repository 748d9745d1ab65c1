"""CPU half of the native word-timestamp alignment (csrc/align.hip): the torch restatement of the alignment matrix against float64, the
kernel's DTW text (csrc/dtw_core.h) run by its host driver against timing.dtw, and the argument checks that must fire before any launch."""
import numpy as np
import pytest
import torch

from alignment_cases import DTW_FAMILIES, DTW_SHAPES, MATRIX_CASES, dtw_cost, dtw_want, matrix_planes, matrix_reference


@pytest.fixture(scope="module")
def native():
    import os

    import __graft_entry__ as g
    from olmoasr_amd import _native
    if not os.path.isfile(_native.LIB_PATH):
        g.build()
    _native.lib()
    return _native


@pytest.mark.parametrize("case", MATRIX_CASES, ids=lambda c: "x".join(map(str, c)))
def test_alignment_matrix_torch_against_float64_and_the_inline_expression(case):
    from olmoasr_amd import timing
    Hsel, n, F, sc = case
    qk = matrix_planes(*case)
    m64, e32, _ = matrix_reference(case)
    assert np.isfinite(m64).all()
    print(f"case {case}: max|z| {np.abs(m64).max():.3f}, fp32 torch path vs float64 {e32:.2e}")
    assert e32 <= 1e-5
    # the function is a pure move of find_alignment's former inline lines: the same ops in the same order give the same bits
    qks, heads = {3: qk}, [(3, s) for s in range(Hsel)]
    got = timing.alignment_matrix_torch(qks, heads, F, 7, 1.0)
    weights = torch.stack([qks[l][h] for l, h in heads])
    weights = weights[:, :, :F]
    weights = (weights * 1.0).softmax(dim=-1)
    std, mean = torch.std_mean(weights, dim=-2, keepdim=True, unbiased=False)
    weights = (weights - mean) / std
    weights = timing.median_filter(weights, 7)
    assert torch.equal(got, weights.mean(dim=0)) and got.shape == (n, F) and got.dtype == torch.float32


@pytest.mark.parametrize("family", DTW_FAMILIES)
@pytest.mark.parametrize("N,M", DTW_SHAPES)
def test_host_driver_of_the_kernel_dtw_equals_timing_dtw(native, N, M, family):
    from olmoasr_amd import ops
    x = dtw_cost(N, M, family)
    want = dtw_want(N, M, family)
    got = ops.dtw_host(x)
    assert got[0].dtype == torch.int64 and np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy(), want[1])


def test_host_driver_negates_and_honours_the_row_stride(native):
    from olmoasr_amd import ops
    for N, M, family in ((65, 63, "randn"), (5, 64, "ties"), (130, 129, "ridge")):
        x = dtw_cost(N, M, family)
        big = torch.full((N + 3, M + 5), float("nan"))
        big[2:-1, :M] = x
        want = dtw_want(N, M, family, True)
        got = ops.dtw_host(big[2:-1, :M], negate=True)
        assert np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy(), want[1])


class _Tok:
    eot, sot_sequence, no_timestamps = 50256, (50257,), 50362


class _CpuModel:
    device = torch.device("cpu")


def test_find_alignment_refuses_unknown_and_unavailable_backends():
    from olmoasr_amd import timing
    mel = torch.zeros(80, 3000)
    with pytest.raises(ValueError, match="backend"):
        timing.find_alignment(_CpuModel(), _Tok(), [1, 2], mel, 3000, backend="bogus")
    with pytest.raises(ValueError, match="native"):
        timing.find_alignment(_CpuModel(), _Tok(), [1, 2], mel, 3000, backend="native")
    with pytest.raises(ValueError, match="num_frames"):  # (no audio token to align to: refused the same way for either backend)
        timing.find_alignment(_CpuModel(), _Tok(), [1, 2], mel, 1, backend="torch")
    with pytest.raises(ValueError, match="backend"):  # (also with nothing to align: the argument is checked first)
        timing.find_alignment(_CpuModel(), _Tok(), [], mel, 3000, backend="bogus")


def test_out_of_range_arguments_raise_value_error_without_a_launch(native):
    """The shapes are refused by the binding itself, on tensors that are not even on a GPU: nothing can have been launched."""
    from olmoasr_amd import ops
    for n, m in ((0, 5), (449, 5), (5, 0), (5, 1501)):
        with pytest.raises(ValueError, match="dtw"):
            ops.dtw(torch.zeros(n, m))
        with pytest.raises(ValueError, match="dtw"):
            ops.dtw_host(torch.zeros(n, m))
    with pytest.raises(ValueError, match="dtw"):
        ops.dtw(torch.zeros(4, 4, dtype=torch.float64))
    qk = [torch.zeros(3, 4, 20), torch.zeros(3, 4, 20)]
    heads = [[0, 2], [1]]
    for F in (0, 21, -1):
        with pytest.raises(ValueError, match="n_frames"):
            ops.alignment_matrix(qk, heads, F)
    for w in (0, 2, 4, 17, -7):
        with pytest.raises(ValueError, match="medfilt_width"):
            ops.alignment_matrix(qk, heads, 10, medfilt_width=w)
    with pytest.raises(ValueError, match="head"):
        ops.alignment_matrix(qk, [[0, 3], [1]], 10)
    with pytest.raises(ValueError, match="head"):
        ops.alignment_matrix(qk, [[], []], 10)
    with pytest.raises(ValueError, match="repeated"):  # (a head named twice would weigh twice in the torch path's mean)
        ops.alignment_matrix(qk, [[0, 2, 0], [1]], 10)
    with pytest.raises(ValueError):
        ops.alignment_matrix(qk, [[0]], 10)
    # and the library refuses the same on its own (OASR_EINVAL), for callers that come through the C ABI
    lib = native.lib()
    assert lib.oasr_dtw_workspace_bytes(449, 5) == 0 and lib.oasr_dtw_workspace_bytes(5, 1501) == 0 and lib.oasr_dtw_workspace_bytes(448, 1500) > 0
    buf = torch.zeros(64, dtype=torch.int32)
    assert lib.oasr_dtw(native.ptr(buf), 5, 449, 5, 0, native.ptr(buf), native.ptr(buf), native.ptr(buf), native.ptr(buf), 1 << 30, None) == -1
    assert lib.oasr_dtw(native.ptr(buf), 5, 5, 1501, 0, native.ptr(buf), native.ptr(buf), native.ptr(buf), native.ptr(buf), 1 << 30, None) == -1
    a = native.AlignArgs()
    a.qk[0], a.head_mask[0], a.n_layers, a.H, a.n_tok, a.Tk, a.qk_scale = buf.data_ptr(), 1, 1, 2, 4, 20, 1.0
    a.out, a.ldo = buf.data_ptr(), 20
    import ctypes
    for F, w in ((0, 7), (21, 7), (10, 4), (10, 17)):
        a.n_frames, a.medfilt_width = F, w
        assert lib.oasr_alignment_matrix(ctypes.byref(a), native.ptr(buf), 1 << 30, None) == -1, (F, w)
