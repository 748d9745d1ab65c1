"""GEMM operands with exactly one right answer, an integer reference and guard bands (plain torch, no GPU needed).

The GEMM tests used to feed iid N(0, 1) operands and compare with an fp32 product under a 1 % tolerance: five bf16 roundings wide, so
a truncating pack, a double rounding or an epilogue that rounds at the wrong point all passed.  The operands built here are small
integers.  A bf16 x bf16 product is exact in fp32, and a sum of integers whose partial sums stay below 2^24 is exact in fp32 IN ANY
ORDER -- inside the MFMA, across split-K ranges, through fp32 atomics or a persistent tile walk.  A correct kernel therefore has one
right answer per output element, the reference is integer arithmetic on the CPU and the comparison is ``torch.equal``.

Two regimes (``operands(regime, ...)``; the preconditions are asserted from the integer reference by ``reference()`` on every case):

  R (rounding)    A, B iid uniform integers in [-a, a]; a = 15 while K a^2 < 2^24, else 7 (192,000 tokens x 49 < 2^24; 5 beyond that).  The fp32
                  accumulator holds the integer sum exactly; a bf16 output is that integer rounded to nearest even ONCE
                  (``rne_bf16``).  At K = 64 ... 4096, 46 ... 87 % of the sums need rounding, 9 ... 22 % are exact ties, and a
                  truncating conversion differs on 23 ... 44 % of them (tests/test_gemm_exact_cpu.py asserts the floor).  For every
                  output that rounds once (plain ``out``), every fp32 output (expected = the integer itself) and alpha in {0.5, 2}.
  S (small sums)  every row of A holds exactly min(K, 32) entries +-1 (at ``start + j * step mod K``, step coprime to K, both drawn per
                  row) and zeros elsewhere; B uniform in {-2..2}: |acc| <= 64 by construction.  Bias, pos and resid are integers with
                  |acc + bias| <= 128 and |pre + side| <= 256 (``side_inputs``); u for dgelu_deriv = 1 is drawn from
                  {0, +-0.25, +-0.5, +-1, +-2}, or {0, +-1} when column sums are taken (M max|out| < 2^24).  Every value at every
                  rounding point kernels.h documents (out_pre <- bf16(v), bf16(v) + pos, bf16(v) * u, bf16(v) + resid) is then a bf16
                  value already: the roundings are identities, the result is bit-exact whatever order or precision the epilogue
                  uses in between, and column sums are exact integers.  For all linear epilogue combinations.

Reference: float64 matmul of the integer operands (every partial sum is an integer below 2^53, so float64 IS integer arithmetic here;
torch has no BLAS for int64), with max|acc| < 2^24 and the regime's bound asserted.

Guard bands: ``embed`` places a logical matrix inside a larger allocation (>= 256 rows before and after, >= 72 extra columns, the
view starts 8 elements into the row, ld % 8 == 0 -- the 16-byte alignment the fast kernels ask for is kept, so the pad does not change
the kernel choice).  Operand pads hold NaN or +Inf: an element outside the logical region that reaches an accumulator poisons the
result.  Output pads hold a non-canonical NaN pattern (bf16 0x7FC1, fp32 0x7FC00001) and ``Guarded.check`` requires every byte
outside the logical region to be bit-identical afterwards, compared as integers.  Everything stays inside the test's own allocation:
an over-read or over-write is observed as data, never provoked as a fault.

``emulate`` is an integer stand-in for the kernels with one deliberate flaw at a time (``FLAWS``); the CPU power test shows that the
exact comparison or the guard check catches each of them on the cases built here.
"""
import math

import torch

BF = torch.bfloat16
F64 = torch.float64
SENTINEL_BF16 = 0x7FC1
SENTINEL_F32 = 0x7FC00001
PAD_ROWS = 256
PAD_COLS = 72
COL0 = 8  # the view starts this many elements into each row of the allocation (16-byte aligned for bf16 and fp32)
U_VALUES = (0.0, 0.25, -0.25, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0)

# The kernel paths the GPU suite forces (tests/test_gpu_gemm_exact.py) and the hand-written rule of which call can run on which;
# tests/test_gemm_route_cpu.py holds the rule to the library's own route (csrc/gemm.hip: gemm_route) without a GPU.
# path -> (oasr_gemm_force_general mode, oasr_gemm_set_variant value, kernel family)
PATHS = {
    "general": (1, -1, "general"),
    "fast128": (2, -1, "fast128"),
    "fast256": (3, -1, "fast256"),
    "pp": (4, 24, "pp"),                          # default schedule, plain launch
    "pp_nt": (4, 24 | 64 | 128, "pp"),            # + non-temporal epilogue stores and side-input loads
    "pp_persistent": (4, 40, "pp"),               # one workgroup per CU walking the plain launch's grid
    "pp_persistent_nt": (4, 40 | 64 | 128, "pp"),
    "skinny": (0, -1, "skinny"),
}


def family_of(symbol):
    if symbol.startswith("gemm_kernel<"):
        return "general"
    if symbol.startswith("gemm_skinny_kernel<"):
        return "skinny"
    if symbol.startswith("oasr_gemm_pp_kernel<"):
        return "pp"
    assert symbol.startswith("oasr_gemm_fast_kernel<"), symbol
    return "fast128" if symbol.split(", ")[2] == "128" else "fast256"


def takes(path, M, N, K, ta, tb, *, atomic_only=False, f32=False):
    """launch_gemm's routing rules: can a call of this shape run on ``path`` (forced as PATHS says)?"""
    if N % 4 or ((not ta or not tb) and K % 8):
        return False
    fam = PATHS[path][2]
    if fam == "general":
        return True
    if fam == "skinny":
        return M <= 64 and not ta and not tb and K % 64 == 0 and not atomic_only
    ok = K % 64 == 0 and (not ta or M % 8 == 0) and (not tb or N % 8 == 0) and M >= 8 and N >= 8 and (atomic_only or (not f32 and N % 8 == 0))
    if path.startswith("pp_persistent"):  # (the ping-pong launcher, csrc/gemm_pp.hip: more virtual blocks than CUs; this suite only uses it unsplit)
        ok = ok and not atomic_only and ((M + 255) // 256) * ((N + 255) // 256) > 256
    return ok


def amplitude(K):
    """Regime R: 15 while K a^2 < 2^24, then 7 (the 192,000-token weight gradients), then 5 (conv1's 384,000 window rows)."""
    return 15 if K * 15 * 15 < 2 ** 24 else (7 if K * 7 * 7 < 2 ** 24 else 5)


def operands(regime, M, N, K, seed, device="cpu"):
    """Logical integer operands A [M, K], B [N, K] as int16 tensors (out[m, n] = sum_k A[m, k] B[n, k]), drawn on ``device``."""
    g = torch.Generator(device=device).manual_seed(seed)
    if regime == "R":
        a = amplitude(K)
        assert K * a * a < 2 ** 24
        A = torch.randint(-a, a + 1, (M, K), generator=g, dtype=torch.int16, device=device)
        B = torch.randint(-a, a + 1, (N, K), generator=g, dtype=torch.int16, device=device)
        return A, B
    assert regime == "S"
    nz = min(K, 32)
    coprime = torch.tensor([s for s in range(1, K + 1) if math.gcd(s, K) == 1], device=device)
    step = coprime[torch.randint(0, len(coprime), (M,), generator=g, device=device)]
    start = torch.randint(0, K, (M,), generator=g, device=device)
    pos = (start[:, None] + step[:, None] * torch.arange(nz, device=device)[None, :]) % K  # nz distinct k per row
    sign = (torch.randint(0, 2, (M, nz), generator=g, dtype=torch.int16, device=device) * 2 - 1)
    A = torch.zeros(M, K, dtype=torch.int16, device=device)
    A.scatter_(1, pos, sign)
    B = torch.randint(-2, 3, (N, K), generator=g, dtype=torch.int16, device=device)
    return A, B


def matmul_int(A, B, chunk=16384):
    """sum_k A[m, k] B[n, k] of integer tensors, exactly (float64 holds every partial sum); K is walked in chunks to bound the memory."""
    acc = torch.zeros(A.shape[0], B.shape[0], dtype=F64, device=A.device)
    for k0 in range(0, A.shape[1], chunk):
        acc += A[:, k0:k0 + chunk].to(F64) @ B[:, k0:k0 + chunk].to(F64).t()
    return acc.to(torch.int64)


def check_regime(regime, A, B, acc):
    """The regime's preconditions, from the operands and the integer accumulator alone."""
    K = A.shape[1]
    assert int(A.abs().max()) * int(B.abs().max()) * K < 2 ** 24, "partial sums must stay exact in fp32 in any order"
    assert int(acc.abs().max()) < 2 ** 24
    if regime == "S":
        nnz = (A != 0).sum(1)
        assert int(nnz.min()) == int(nnz.max()) == min(K, 32) and int(A.abs().max()) == 1
        assert int(B.abs().max()) <= 2 and int(acc.abs().max()) <= 64


def sample_rows(M, seed, at_least=1024, tile=256):
    """Output rows a production-sized case recomputes on the CPU: the first and last row of every ``tile``-row tile plus seeded random
    rows, ``at_least`` of them (all rows when there are no more)."""
    if M <= at_least:
        return torch.arange(M)
    rows = set(range(0, M, tile)) | set(min(M, r + tile) - 1 for r in range(0, M, tile))
    extra = torch.randperm(M, generator=torch.Generator().manual_seed(seed)).tolist()
    for r in extra:
        if len(rows) >= at_least:
            break
        rows.add(r)
    return torch.tensor(sorted(rows))


def reference(regime, A, B):
    """Integer accumulator [M, N] (int64) with the regime's preconditions asserted."""
    acc = matmul_int(A, B)
    check_regime(regime, A, B, acc)
    return acc


def side_inputs(acc, seed, *, colsum=False, pos_period=0, device="cpu"):
    """Regime S side inputs for the accumulator ``acc`` [M, N]: integer bias [N] with |acc + bias| <= 128, integer resid [M, N] and pos
    [pos_period, N] with |pre + side| <= 256, u [M, N] of ``U_VALUES`` ({0, +-1} with column sums).  Float64 tensors on ``device``."""
    g = torch.Generator(device=device).manual_seed(seed)
    M, N = acc.shape
    bias = torch.randint(-64, 65, (N,), generator=g, device=device).to(F64)
    resid = torch.randint(-128, 129, (M, N), generator=g, device=device, dtype=torch.int16).to(F64)
    pos = torch.randint(-128, 129, (max(pos_period, 1), N), generator=g, device=device).to(F64)
    vals = torch.tensor((0.0, 1.0, -1.0) if colsum else U_VALUES, dtype=F64, device=device)
    u = vals[torch.randint(0, len(vals), (M, N), generator=g, device=device)]
    assert float((acc + bias).abs().max()) <= 128
    return bias, resid, pos, u


# ---- bf16 helpers ------------------------------------------------------------------------------------------------------------------
def _f32_bits(x):
    return x.to(torch.float32).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def _from_bits(bits):
    b = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32)
    return b.view(torch.float32)


def rne_bf16(v):
    """Round-to-nearest-even bf16 of integers |v| < 2^24 (or of fp32 values), by integer arithmetic on the fp32 bit pattern -- not by
    torch's own conversion, which the CPU test compares it with.  Returns a bf16 tensor."""
    bits = _f32_bits(v)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return _from_bits(bits).to(BF)


def trunc_bf16(v):
    return _from_bits(_f32_bits(v) & 0xFFFF0000).to(BF)


def round_bits(v, bits):
    """Round-to-nearest-even of fp32-exact values to ``bits`` significand bits (11: an fp16-like intermediate)."""
    drop = 24 - bits
    b = _f32_bits(v)
    b = (b + (1 << (drop - 1)) - 1 + ((b >> drop) & 1)) & ~((1 << drop) - 1)
    return _from_bits(b)


def bf16_ulp(x):
    """Spacing of bf16 values at |x| (float64 in, float64 out): 2^(floor(log2 |x|) - 7), 2^-133 in the subnormal range and at 0."""
    ax = x.to(F64).abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(ax)) - 7.0)


def gelu64(x):
    """x Phi(x) in float64; Phi through erfc so that the negative tail keeps its relative accuracy."""
    x = x.to(F64)
    return x * 0.5 * torch.special.erfc(-x / math.sqrt(2.0))


def dgelu64(x):
    x = x.to(F64)
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def rounding_stats(acc):
    """Shares of the integer sums that need rounding to bf16, that are exact ties, and on which truncation differs from RNE."""
    r = rne_bf16(acc).to(F64)
    t = trunc_bf16(acc).to(F64)
    a = acc.to(F64)
    ulp = bf16_ulp(a)
    needs = r != a
    tie = needs & ((a - t).abs() * 2 == ulp)
    n = acc.numel()
    return float(needs.sum()) / n, float(tie.sum()) / n, float((r != t).sum()) / n


# ---- guard bands -------------------------------------------------------------------------------------------------------------------
def _ld(width, pad_cols):
    return (COL0 + width + pad_cols + 7) // 8 * 8


class Guarded:
    """A logical [R, C] matrix (``view``) inside a larger allocation (``buf``) whose every other element holds ``fill_bits``."""

    def __init__(self, buf, view, r0, fill_bits):
        self.buf, self.view, self.r0, self.fill_bits = buf, view, r0, fill_bits
        self.ld = buf.shape[1]

    def _ints(self):
        return self.buf.view(torch.int16 if self.buf.element_size() == 2 else torch.int32)

    def check(self, name=""):
        """Every element outside the logical region still holds the fill pattern, bit for bit."""
        R, C = self.view.shape
        b = self._ints()
        fill = self.fill_bits - (1 << (8 * self.buf.element_size())) if self.fill_bits >= 1 << (8 * self.buf.element_size() - 1) else self.fill_bits
        parts = {"rows before": b[:self.r0], "rows after": b[self.r0 + R:], "row gap (left)": b[self.r0:self.r0 + R, :COL0],
                 "row gap (right)": b[self.r0:self.r0 + R, COL0 + C:]}
        for what, p in parts.items():
            bad = p != fill
            assert not bool(bad.any()), f"{name}: {int(bad.sum())} guard elements changed in the {what}; first at {bad.nonzero()[0].tolist()}"


def embed(t, pad_rows=PAD_ROWS, pad_cols=PAD_COLS, fill="sentinel", device=None):
    """Place the logical 2-D tensor ``t`` (bf16 or fp32) inside a larger allocation: ``pad_rows`` rows before and after, the view
    ``COL0`` elements into the row, ld = COL0 + width + pad_cols rounded up to a multiple of 8.  fill: "sentinel" (outputs), "nan" or
    "inf" (operands).  Returns a ``Guarded`` whose ``view`` is the strided logical matrix holding ``t``'s values."""
    assert t.dim() == 2 and t.dtype in (BF, torch.float32) and pad_rows >= 0 and pad_cols >= 0
    R, C = t.shape
    ld = _ld(C, pad_cols)
    two = t.dtype == BF
    bits = {"sentinel": SENTINEL_BF16 if two else SENTINEL_F32, "nan": 0x7FC0 if two else 0x7FC00000, "inf": 0x7F80 if two else 0x7F800000}[fill]
    device = device if device is not None else t.device
    ibuf = torch.full((R + 2 * pad_rows, ld), bits, dtype=torch.int16 if two else torch.int32, device=device)
    buf = ibuf.view(t.dtype)
    view = buf[pad_rows:pad_rows + R, COL0:COL0 + C]
    view.copy_(t)
    return Guarded(buf, view, pad_rows, bits)


def embed_vec(t, pad=PAD_ROWS, fill="sentinel", device=None):
    """A vector of length N inside a longer one, as a one-row ``Guarded`` ([1, N] view; ``.view[0]`` is the vector)."""
    assert t.dim() == 1
    g = embed(t[None, :], pad_rows=0, pad_cols=2 * pad, fill=fill, device=device)
    return g


# ---- integer stand-in for the kernels, one flaw at a time ----------------------------------------------------------------------------
FLAWS = ("truncating_pack", "double_rounding_11_bits", "last_k_chunk_dropped", "split_range_off_by_one_tile", "row_panel_one_tile_too_far",
         "store_16_bytes_past_n", "pad_column_of_b_read", "colsum_includes_rows_past_m", "resid_before_bias")


def emulate(A, B, *, flaw=None, out=None, ldb_pad=None, bias=None, resid=None, split_k=1, colsum=False, tile_m=256, rows_in_buffer=None):
    """What a GEMM kernel with the given flaw would leave behind.  A [M, K], B [N, K] integer tensors.  ``out``: a ``Guarded`` bf16 output
    that is written in place (flaws that store out of bounds write into its pad).  ``ldb_pad``: B's allocation [N, K + pad] whose pad
    columns hold NaN (float64), read by the pad-column flaw.  Returns (bf16 out [M, N] as float64, column sums float64 [N] or None)."""
    M, K = A.shape
    N = B.shape[0]
    Af, Bf = A.to(F64), B.to(F64)
    if flaw == "last_k_chunk_dropped" and K % 64:
        Af = Af[:, :K - K % 64]
        Bf = Bf[:, :K - K % 64]
    if flaw == "split_range_off_by_one_tile" and split_k > 1:
        kt = (K + 63) // 64
        per = (kt + split_k - 1) // split_k
        acc = torch.zeros(M, N, dtype=F64)
        for s in range(split_k):
            k0, k1 = s * per * 64, min(K, (s + 1) * per * 64)
            if s == 1:
                k0 += 64  # this split starts one K-tile late
            if k0 < k1:
                acc += Af[:, k0:k1] @ Bf[:, k0:k1].t()
    elif flaw == "pad_column_of_b_read":
        acc = torch.cat([Af, torch.zeros(M, 1, dtype=F64)], 1) @ ldb_pad[:, :K + 1].t()  # A's zero fill meets B's first pad column
    else:
        acc = Af @ Bf.t()
    v = acc
    if flaw == "resid_before_bias" and resid is not None:
        v = rne_bf16(v + resid).to(F64)  # rounds acc + resid, then adds the bias
        if bias is not None:
            v = v + bias
    else:
        if bias is not None:
            v = v + bias
        if resid is not None:
            v = rne_bf16(v).to(F64) + resid
    if flaw == "truncating_pack":
        o = trunc_bf16(v)
    elif flaw == "double_rounding_11_bits":
        o = rne_bf16(round_bits(v, 11))
    else:
        o = rne_bf16(v)
    cs = None
    if colsum:
        cs = o.to(F64).sum(0)
        if flaw == "colsum_includes_rows_past_m":  # the clamped source rows of the last tile are summed as well
            extra = (M + tile_m - 1) // tile_m * tile_m - M
            cs = cs + o[M - 1:M].to(F64).sum(0) * extra
    if out is not None:
        out.view.copy_(o)
        if flaw == "row_panel_one_tile_too_far":  # the last row panel stores its clamped rows as well
            extra = (M + tile_m - 1) // tile_m * tile_m - M
            out.buf[out.r0 + M:out.r0 + M + extra, COL0:COL0 + N] = o[M - 1:M]
        if flaw == "store_16_bytes_past_n" and N % 8 == 4:
            out.buf[out.r0:out.r0 + M, COL0 + N:COL0 + N + 4] = 0.0
    return o.to(F64), cs
