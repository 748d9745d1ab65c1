"""Inputs and references shared by tests/test_alignment_cpu.py and tests/test_gpu_alignment.py (word-timestamp alignment: the alignment
matrix and the DTW of olmoasr_amd/timing.py, and their device operators of csrc/align.hip)."""
import functools

import numpy as np
import torch

# ---- DTW --------------------------------------------------------------------------------------------------------------------------------
# one row, one column, both sides of the 64-lane wave boundary, N > M, M > N, the maximum
DTW_SHAPES = [(1, 1), (1, 9), (7, 1), (2, 2), (5, 64), (64, 5), (65, 63), (130, 129), (448, 3), (3, 1500), (446, 1500), (448, 1500)]
DTW_FAMILIES = ["randn", "ties", "zeros", "ridge"]


def dtw_cost(N, M, family):
    """fp32 [N, M]: seeded randn; integers from {0, 1, 2} (ties of all three kinds in every neighbourhood: only the tie rule decides the
    path); all zeros; randn with a planted negative diagonal ridge."""
    g = torch.Generator().manual_seed(N * 10007 + M * 13 + DTW_FAMILIES.index(family))
    if family == "randn":
        return torch.randn(N, M, generator=g)
    if family == "ties":
        return torch.randint(0, 3, (N, M), generator=g).float()
    if family == "zeros":
        return torch.zeros(N, M)
    x = torch.randn(N, M, generator=g)
    j = torch.arange(M)
    x[(j * N) // M, j] -= 4.0
    return x


@functools.lru_cache(maxsize=None)
def dtw_want(N, M, family, negate=False):
    """timing.dtw's path for dtw_cost(N, M, family) (of its negation), computed once per session."""
    from olmoasr_amd import timing
    x = dtw_cost(N, M, family).numpy()
    return timing.dtw(-x if negate else x)


# ---- alignment matrix -----------------------------------------------------------------------------------------------------------------
# (selected heads, tokens, frames, score scale); (2, 4, 3, 2) pins the skipped filter (F <= 7 // 2), (2, 4, 4, 2) the first filtered length
MATRIX_CASES = [(3, 5, 9, 2), (6, 8, 1500, 2), (12, 70, 130, 4), (24, 130, 1500, 3), (4, 448, 1500, 3), (2, 4, 3, 2), (2, 4, 4, 2)]
TK = 1500


def matrix_planes(Hsel, n, F, sc):
    """qk fp32 [Hsel, n, 1500]: randn * sc with +6 at frame i * F // n of token row i in every head."""
    g = torch.Generator().manual_seed(Hsel * 1000 + n)
    qk = torch.randn(Hsel, n, TK, generator=g) * sc
    i = torch.arange(n)
    qk[:, i, (i * F) // n] += 6.0
    return qk


def deal_out(qk, F):
    """The planes dealt out over layer tensors [H, n, 1500] at non-contiguous head indices, as the operator reads them: every unselected
    head and every frame >= F is NaN.  Returns ({layer: tensor}, [(layer, head)] in plane order)."""
    Hsel, n, _ = qk.shape
    n_layers = 2 if Hsel < 12 else 3
    H = 2 * ((Hsel + n_layers - 1) // n_layers) + 1
    layers = {l: torch.full((H, n, TK), float("nan")) for l in range(n_layers)}
    heads = []
    for s in range(Hsel):
        l, h = s % n_layers, 2 * (s // n_layers) + (s % n_layers) % 2  # heads 0, 2, 4 .. in even layers, 1, 3, 5 .. in odd ones
        layers[l][h, :, :F] = qk[s, :, :F]
        heads.append((l, h))
    return layers, heads


def matrix_float64(qk, F, width=7, scale=1.0):
    """Float64 restatement of the alignment matrix: numpy softmax, population std over the tokens, scipy's median filter in mirror mode
    (skipped when F <= width // 2), mean over the heads."""
    from scipy.ndimage import median_filter as sp
    w = qk[:, :, :F].double().numpy() * scale
    w = np.exp(w - w.max(-1, keepdims=True))
    w = w / w.sum(-1, keepdims=True)
    z = (w - w.mean(-2, keepdims=True)) / w.std(-2, keepdims=True)
    if F > width // 2 and width > 1:
        z = sp(z, size=(1, 1, width), mode="mirror")
    return z.mean(0)


@functools.lru_cache(maxsize=None)
def matrix_reference(case):
    """(float64 matrix, e32 = max |alignment_matrix_torch in fp32 - float64|, DTW path of the float64 matrix's rows [2:-1] negated),
    computed once per session and shared."""
    from olmoasr_amd import timing
    Hsel, n, F, sc = case
    qk = matrix_planes(*case)
    m64 = matrix_float64(qk, F)
    m32 = timing.alignment_matrix_torch({0: qk}, [(0, s) for s in range(Hsel)], F, 7, 1.0).numpy()
    e32 = float(np.abs(m32.astype(np.float64) - m64).max())
    path = timing.dtw(-m64[2:-1]) if n > 3 else None
    return m64, e32, path
