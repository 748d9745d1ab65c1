"""Plain references, planted inputs, checkers and deliberately flawed stand-ins for the glue kernels (plain torch on the CPU, no GPU needed).

The kernels between the GEMMs and the attention -- embedding gather / scatter, the two conv folds, the column sum, the mel transpose, the
packs and casts, LayerNorm's column sums -- go wrong in a FEW ROWS: a tap kept or dropped at a sample boundary, a pad id scattered, a row
past M summed.  A relative L2 norm over a whole-model gradient cannot see that.  The tests built on this module therefore give every
operator inputs with exactly one right answer:

  * wherever the operation is a sum, the plants are small integers: every bf16 operand is representable, every partial sum stays below
    2^24, so an fp32 sum is exact IN ANY ORDER (atomics, grid-stride partials, LDS reductions) and the comparison is bit for bit;
  * every value is a code of its own position, so a value taken from the wrong place differs from the right one;
  * every accumulated output starts from a non-zero integer pre-fill, every output sits between guard bands (gemm_exact.embed_vec) and
    everything the contract says is not read holds NaN.

The references are written from the operators' definitions (csrc/kernels.h), as explicit loops over what is summed -- for the conv folds
over (sample, window, tap), adding into the input row the tap covers and dropping rows outside the sample -- not from the kernels' index
arithmetic.  ``FLAWS`` lists, per operator, stand-ins with one mistake each; tests/test_glue_ref_cpu.py shows that the checkers accept the
reference and reject every one of them at the shapes and plants the GPU tests use.
"""
import math

import torch

import gemm_exact as ge

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
ROWTAB = 16            # include/oasr.h: OASR_ROWTAB
NO_ROW = 0x3FFFFFFF    # chunk-row table entry of a chunk that has no rows
E24 = 2.0 ** -24


# ---- helpers -----------------------------------------------------------------------------------------------------------------------
def bits(t):
    """The tensor's bytes as integers (int16 for bf16, int32 for fp32) -- NaN payloads and signed zeros compare like any other value."""
    t = t.contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def is_bf16(x):
    """Every value survives a round trip through bf16 (float64 / fp32 in)."""
    return bool((x.to(BF).to(x.dtype) == x).all())


def assert_exact_plants(name, *, operands=(), partial_abs_sum=None):
    """The exactness claims of an integer plant: bf16 operands representable, the sum of absolute values of anything that is ever added
    together below 2^24 (then so is every partial sum, in any order)."""
    for o in operands:
        assert is_bf16(o.to(F64)), f"{name}: operand not representable in bf16"
        assert bool((o.to(F64) == o.to(F64).round()).all()), f"{name}: operand not an integer"
    if partial_abs_sum is not None:
        assert float(partial_abs_sum.max()) < 2 ** 24, f"{name}: partial sums may reach {float(partial_abs_sum.max())} >= 2^24"


def check_exact(name, got, want, where=None, code=None):
    """Bit-for-bit comparison.  ``where(flat_index) -> str`` names the element ((b, t, column), ...), ``code(flat_index) -> str`` its plant."""
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    bad = bits(got) != bits(want)
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), got.shape))
        msg = f"{name}: {int(bad.sum())} of {bad.numel()} elements differ; first at {idx}"
        if where is not None:
            msg += f" = {where(idx)}"
        msg += f": got {got.flatten()[i].item()!r}, want {want.flatten()[i].item()!r}"
        if code is not None:
            msg += f"; planted {code(idx)}"
        raise AssertionError(msg)


def guarded(t, fill="sentinel", device=None):
    """``t`` (any shape, bf16 / fp32) flattened inside a longer allocation (gemm_exact.embed_vec): returns (Guarded, tensor of t's shape that
    aliases the logical region).  fill = "sentinel" for outputs (check with ``.check``), "nan" for inputs (a read past the end poisons)."""
    g = ge.embed_vec(t.reshape(-1), fill=fill, device=device)
    return g, g.view[0].view(t.shape)


# ---- embedding -----------------------------------------------------------------------------------------------------------------------
EMB = dict(B=5, S=128, d=264, n_embed=97, pad_id=96)  # d = 264: the backward's column loop runs a second time (d > 256), 8 columns wide


def embedding_tokens(seed=0):
    """int64 [B, S]: ids 0, n_embed - 1 (= the training pad id), -1 and n_embed planted; tokens repeat inside a position across the batch
    (column 7: all samples the same id; column 9: two and two) and across positions (a vocabulary of 97 over 640 slots)."""
    p = EMB
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(0, p["n_embed"] - 1, (p["B"], p["S"]), generator=g)
    tok[:, 7] = 13
    tok[0, 9] = tok[1, 9] = 21
    tok[2, 9] = tok[3, 9] = 22
    tok[0, 0], tok[1, 0], tok[2, 0], tok[3, 0], tok[4, 0] = 0, 96, -1, 97, 96
    tok[4, 127], tok[3, 127], tok[2, 127], tok[1, 63], tok[0, 64] = 97, 0, 96, -1, 96
    tok[1, 30:34] = 96  # a run of pads
    tok[3, 100] = 2 ** 40  # far outside the table
    return tok


def permuted_rowtab(B, S, seed=1):
    """A chunk-row table [B, ROWTAB] that scatters the (b, chunk) pairs over 1.5 x as many 64-row slots as there are chunks: the slots no
    chunk maps to must keep the sentinel."""
    nch = S // 64
    nslot = (3 * B * nch + 1) // 2
    perm = torch.randperm(nslot, generator=torch.Generator().manual_seed(seed))[: B * nch]
    tab = torch.full((B, ROWTAB), NO_ROW, dtype=torch.int32)
    tab[:, :nch] = (64 * perm).view(B, nch).to(torch.int32)
    return tab, nslot * 64


def row_of(tab, b, s, S):
    return b * S + s if tab is None else int(tab[b, s >> 6]) + (s & 63)


def embedding_fwd_ref(tok, E, pos, dtype, tab=None, n_rows=None, flaw=None):
    """x rows as the contract lays them out; rows nothing maps to are None-marked through the returned mask.  fp32 add (torch), then the
    activation dtype: the operation's own definition, element for element.  Returns (x [n_rows, d] dtype, written [n_rows] bool)."""
    B, S = tok.shape
    n_embed, d = E.shape
    n_rows = B * S if n_rows is None else n_rows
    x = torch.zeros(n_rows, d, dtype=dtype)
    written = torch.zeros(n_rows, dtype=torch.bool)
    for b in range(B):
        for s in range(S):
            t = int(tok[b, s])
            if 0 <= t < n_embed:
                e = E[t]
            elif flaw == "oob_id_clamped":
                e = E[min(max(t, 0), n_embed - 1)]
            else:
                e = torch.zeros(d)
            r = row_of(None if flaw == "rowtab_ignored" else tab, b, s, S)
            x[r] = (e + pos[s]).to(dtype)
            written[r] = True
    return x, written


def embedding_bwd_plants(tok, tab=None, n_rows=None, span=None, seed=2):
    """dx integers in [-8, 8] in the activation rows (fp64 holder [n_rows, d]); rows no chunk maps to and rows at s >= span[b] are NaN.
    Integer pre-fills for dE [n_embed, d] and dpos [S, d]."""
    p = EMB
    B, S, d = p["B"], p["S"], p["d"]
    n_rows = B * S if n_rows is None else n_rows
    g = torch.Generator().manual_seed(seed)
    vals = torch.randint(-8, 9, (B, S, d), generator=g).to(F64)
    dx = torch.full((n_rows, d), float("nan"), dtype=F64)
    for b in range(B):
        for s in range(S):
            if span is None or s < int(span[b]):
                dx[row_of(tab, b, s, S)] = vals[b, s]
    dE0 = torch.randint(-50, 51, (p["n_embed"], d), generator=g).to(F64)
    dpos0 = torch.randint(-50, 51, (S, d), generator=g).to(F64)
    # exactness: at most B * S values of magnitude <= 8 meet in one dE row, B in one dpos row, on top of a pre-fill <= 50
    assert_exact_plants("embedding_bwd", operands=(vals,), partial_abs_sum=torch.tensor([50.0 + 8.0 * B * S]))
    return dx, dE0, dpos0


def embedding_bwd_ref(tok, dx, dE0, dpos0, pad_id, tab=None, span=None, flaw=None):
    """dE / dpos after the call (float64, exact integers).  A null output is simply not compared by the caller."""
    B, S = tok.shape
    n_embed, d = dE0.shape
    dE, dpos = dE0.clone(), dpos0.clone()
    if flaw == "dpos_overwritten":
        dpos.zero_()
    for b in range(B):
        for s in range(S):
            if span is not None and s >= int(span[b]) and flaw != "span_ignored":
                continue
            g = dx[row_of(tab, b, s, S)].clone()
            if flaw == "second_column_pass_missing":
                g[256:] = 0.0
            dpos[s] += g
            t = int(tok[b, s])
            if t == pad_id and flaw != "pad_id_scattered":
                continue
            if not 0 <= t < n_embed:
                if flaw != "oob_id_clamped":
                    continue
                t = min(max(t, 0), n_embed - 1)
            dE[t] += g
    return dE, dpos


# ---- column sum ----------------------------------------------------------------------------------------------------------------------
COLSUM_SHAPES = ((16389, 520, 528), (1, 8, 8), (3, 8, 16), (5, 8, 8))  # (M, ncols, ld)


def colsum_plants(M, ncols, ld, seed=3):
    """x [M + 4][ld] float64: integers in {-4..4} in the live region, NaN in the columns >= ncols and in the 4 rows after M; integer pre-fill."""
    g = torch.Generator().manual_seed(seed + M)
    x = torch.full((M + 4, ld), float("nan"), dtype=F64)
    x[:M, :ncols] = torch.randint(-4, 5, (M, ncols), generator=g).to(F64)
    pre = torch.randint(-100, 101, (ncols,), generator=g).to(F64)
    assert_exact_plants("colsum", operands=(x[:M, :ncols],), partial_abs_sum=torch.tensor([100.0 + 4.0 * M]))
    return x, pre


def colsum_ref(x, M, ncols, pre, flaw=None, grid_y=1024):
    out = pre.clone()
    rows = M
    if flaw == "rows_past_m":
        rows = (M + 3) // 4 * 4  # a whole group of 4 row lanes
    for m in range(rows):
        if flaw == "remainder_rows_dropped" and m >= (M // (16 * grid_y)) * 16 * grid_y and M > 16 * grid_y:
            break
        out += x[m, :ncols]
    if flaw == "last_column_block_dropped" and ncols > 512:
        out[512:] = pre[512:]
    return out


# ---- conv2 fold + GELU' --------------------------------------------------------------------------------------------------------------
CONV2_SHAPES = ((3, 6, 8), (3, 3000, 512))  # (B, T1, d)


def conv2_half_codes(B, T2, d):
    """h [B, T2, 3, d] integers in [-127, 127]: a code of (b, t', kk) that also varies along the columns; dA = 2 h (even integers)."""
    w = (torch.arange(B * T2 * 3, dtype=torch.int64) * 37).view(B, T2, 3, 1)
    c = (torch.arange(d, dtype=torch.int64) * 11).view(1, 1, 1, d)
    return ((w + c) % 255 - 127).to(F64)


def conv2_plants(B, T1, d):
    """dA float64 [B * T2 + 1, 3, d]: the even codes, followed by one window row of NaN (what a tap past the last sample would read)."""
    T2 = T1 // 2
    h = conv2_half_codes(B, T2, d)
    dA = torch.full((B * T2 + 1, 3, d), float("nan"), dtype=F64)
    dA[:B * T2] = (2 * h).view(B * T2, 3, d)
    # fold = at most two codes: |fold| <= 508 is an even integer (bf16 holds every even integer up to 512), fold / 2 an integer <= 254
    assert_exact_plants("conv2 fold", operands=(dA[:B * T2],), partial_abs_sum=torch.tensor([508.0]))
    return dA


def conv2_code(B, T1, d):
    T2 = T1 // 2
    h = conv2_half_codes(B, T2, d)

    def code(idx):
        b, t, c = idx
        taps = [(t2, kk) for t2 in range(T2) for kk in range(3) if 2 * t2 - 1 + kk == t] if T2 <= 8 else \
               [(t2, t - 2 * t2 + 1) for t2 in (t // 2, t // 2 + 1) if t2 < T2 and 0 <= t - 2 * t2 + 1 < 3]
        return "taps " + ", ".join(f"(t'={t2}, kk={kk}) = {int(2 * h[b, t2, kk, c])}" for t2, kk in taps)
    return code


def conv2_fold_ref(dA, B, T1, d, flaw=None):
    """fold [B, T1, d] float64: window t' of sample b adds its tap kk into input row 2 t' - 1 + kk of the SAME sample; rows outside [0, T1)
    are the conv's zero padding."""
    T2 = T1 // 2
    fold = torch.zeros(B, T1, d, dtype=F64)
    for b in range(B):
        for t2 in range(T2):
            for kk in range(3):
                t = 2 * t2 - 1 + kk
                if 0 <= t < T1:
                    if flaw == "boundary_tap_dropped" and kk == 0 and t2 == T2 - 1:
                        continue  # `(t >> 1) + 1 < T2 - 1`
                    fold[b, t] += dA[b * T2 + t2, kk]
    if flaw == "last_odd_row_kk0_kept":  # no `(t >> 1) + 1 < T2`: the next sample's first window (past the last sample: NaN)
        for b in range(B):
            fold[b, T1 - 1] += dA[(b + 1) * T2, 0]
    if flaw == "tap_from_neighbouring_sample":  # the fold runs over B * T1 rows as if they were one sample
        for b in range(1, B):
            fold[b - 1, T1 - 1] += dA[b * T2, 0]
    if flaw == "even_row_tap_0":
        for b in range(B):
            for t2 in range(T2):
                fold[b, 2 * t2] += dA[b * T2 + t2, 0] - dA[b * T2 + t2, 1]
    return fold


def dgelu_stats(got, fold_rounded, u, name, dtype):
    """The one-ulp rule for products with GELU': every output within one ulp (bf16) / 4 * 2^-24 relative (fp32) of the float64 product
    ``fold_rounded * gelu'(u)``; returns the share of outputs that are not the correctly rounded value (bf16 only, else 0)."""
    want = fold_rounded.to(F64) * ge.dgelu64(u.to(F64))
    err = (got.to(F64) - want).abs()
    if dtype == BF:
        tol = ge.bf16_ulp(want)
    else:
        # 4 * 2^-24 relative.  gelu'(u) = Phi(u) + u pdf(u) changes sign at u = -0.7518: relative to the RESULT no fp32 evaluation can be held to
        # any bound there, so the figure applies to each of the two terms; the exponent u^2 / 2 of the pdf is itself an fp32 value (up to 18 at
        # |u| = 6), whose rounding exp carries through as u^2 / 2 * 2^-24 relative.  One more 2^-24 for the product with the fold.
        ud = u.to(F64)
        cdf = 0.5 * torch.special.erfc(-ud / math.sqrt(2.0))
        updf = ud.abs() * torch.exp(-0.5 * ud * ud) / math.sqrt(2.0 * math.pi)
        tol = E24 * (fold_rounded.to(F64).abs() * (4 * cdf + updf * (4 + 0.5 * ud * ud)) + want.abs()) + 2.0 ** -140
    bad = err > tol
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), got.shape))
        raise AssertionError(f"{name}: {int(bad.sum())} outputs off by more than the rule; first at {idx}: got {got.flatten()[i].item()!r}, "
                             f"want {want.flatten()[i].item()!r} (fold {fold_rounded.flatten()[i].item()}, u {u.flatten()[i].item()})")
    if dtype != BF:
        return 0.0
    return float((bits(got) != bits(want.to(BF))).sum()) / got.numel()


def torch_fp32_dgelu_share(fold_rounded, u):
    """The same share for a torch fp32 exact-erf evaluation of the same inputs (the yardstick of the 2 x rule)."""
    uf = u.to(F32)
    d = 0.5 * (1.0 + torch.erf(uf * (1.0 / math.sqrt(2.0)))) + uf * torch.exp(-0.5 * uf * uf) * (1.0 / math.sqrt(2.0 * math.pi))
    got = (fold_rounded.to(F32) * d).to(BF)
    want = (fold_rounded.to(F64) * ge.dgelu64(u.to(F64))).to(BF)
    return float((bits(got) != bits(want)).sum()) / got.numel()


def share_allowed(kernel_share, torch_share, n):
    """At most twice the torch fp32 share, or 4 elements when that is larger."""
    return kernel_share <= max(2.0 * torch_share, 4.0 / n)


# ---- conv1 fold -> d(mel) ------------------------------------------------------------------------------------------------------------
CONV1_T = (70, 96, 3000)
CONV1_NM = (8, 80)


def conv1_plants(B, T1, nm):
    """dcol float64 [B * T1, 256]: integer codes of (b, t', column) in [-127, 127]; columns >= 3 * n_mels NaN."""
    r = (torch.arange(B * T1, dtype=torch.int64) * 53).view(-1, 1)
    c = (torch.arange(3 * nm, dtype=torch.int64) * 7).view(1, -1)
    dcol = torch.full((B * T1, 256), float("nan"), dtype=F64)
    dcol[:, :3 * nm] = ((r + c) % 255 - 127).to(F64)
    assert_exact_plants("conv1 fold", operands=(dcol[:, :3 * nm],), partial_abs_sum=torch.tensor([3 * 127.0]))
    return dcol


def conv1_fold_ref(dcol, B, T1, nm, flaw=None, prefill=None):
    """dmel [B, nm, T1] float64: window t' of sample b adds its tap k (columns k * nm ..) into frame t' - 1 + k of the same sample."""
    dmel = torch.zeros(B, nm, T1, dtype=F64)
    for b in range(B):
        for t2 in range(T1):
            for k in range(3):
                t = t2 - 1 + k
                if 0 <= t < T1:
                    if flaw == "halo_row_dropped" and (t // 32) != (t2 // 32):
                        continue  # a tile that reads only its own 32 window rows
                    dmel[b, :, t] += dcol[b * T1 + t2, k * nm:(k + 1) * nm]
    if flaw == "tap_from_neighbouring_sample":  # one run of B * T1 rows
        for b in range(B - 1):
            dmel[b, :, T1 - 1] += dcol[(b + 1) * T1, 0:nm]            # window 0 of the next sample, tap 0 -> frame -1 = last of this one
            dmel[b + 1, :, 0] += dcol[(b + 1) * T1 - 1, 2 * nm:3 * nm]  # last window of this sample, tap 2 -> frame T1 = first of the next
    if flaw == "rotated_slot_read_unrotated":  # columns of the 16-byte chunks past the first 32 / VEC read one slot off (VEC = 8)
        for k in range(3):
            for c in range(nm):
                col = k * nm + c
                ch = col // 8
                rot = ch // 4
                if rot & 7:
                    src = ch * 8 + ((col - rot) & 7)
                    kk, cc = src // nm, src % nm
                    if kk < 3:
                        dmel[:, c, :] += _conv1_single(dcol, B, T1, nm, kk, cc) - _conv1_single(dcol, B, T1, nm, k, c)
    if flaw == "partial_tile_unwritten" and T1 % 32 and prefill is not None:
        dmel[:, :, T1 // 32 * 32:] = prefill
    return dmel


def _conv1_single(dcol, B, T1, nm, k, c):
    out = torch.zeros(B, T1, dtype=F64)
    v = dcol[:, k * nm + c].view(B, T1)
    lo, hi = max(0, 1 - k), min(T1, T1 + 1 - k)  # window rows t' whose frame t' - 1 + k is inside
    out[:, lo - 1 + k:hi - 1 + k] = v[:, lo:hi]
    return out


# ---- mel transpose -------------------------------------------------------------------------------------------------------------------
def mel_plants(B, C, T, seed=5):
    g = torch.Generator().manual_seed(seed + C + T)
    mel = (torch.randn(B, C, T, generator=g) * 1.5 - 2.0).to(F32)  # log10 power: spread over ~ [-8, 4]
    clip_max = mel.amax(dim=(1, 2)) - torch.tensor([0.0, 3.5])[:B]     # the second sample's floor sits 3.5 above its own max - 8
    assert bool((mel < (clip_max - 8.0).view(B, 1, 1)).any()) and bool((mel > (clip_max - 8.0).view(B, 1, 1)).any())
    return mel, clip_max.to(F32)


def mel_ref(mel, clip_max, dtype, flaw=None):
    """[B, T, C]: the same three fp32 operations in torch, then the activation dtype."""
    v = mel
    if clip_max is not None:
        floor = clip_max.view(-1, 1, 1) - 8.0
        if flaw == "floor_of_sample_0":
            floor = floor[:1].expand_as(floor)
        v = (torch.maximum(v, floor) + 4.0) * 0.25
    out = v.transpose(1, 2).contiguous()
    if flaw == "tail_tile_zero" and mel.shape[2] % 32:
        out[:, mel.shape[2] // 32 * 32:] = 0.0
    return out.to(dtype)


# ---- packs and casts -----------------------------------------------------------------------------------------------------------------
PACK_CONV_SHAPES = ((5, 80, 256), (7, 16, 48))  # (co, ci, ldk)


def pack_conv_ref(w, ldk, dtype, flaw=None):
    co, ci, _ = w.shape
    out = torch.zeros(co, ldk, dtype=F32)
    for kk in range(3):
        out[:, kk * ci:(kk + 1) * ci] = w[:, :, kk]
    if flaw == "tap_major_read_as_channel_major":
        out[:, :3 * ci] = w.reshape(co, 3 * ci)
    if flaw == "pad_not_zeroed":
        out[:, 3 * ci:] = 1.0
    return out.to(dtype)


def unpack_conv_ref(g, dw0, ci, flaw=None):
    co = dw0.shape[0]
    dw = torch.zeros_like(dw0) if flaw == "overwrites" else dw0.clone()
    for kk in range(3):
        dw[:, :, kk] += g[:, kk * ci:(kk + 1) * ci]
    return dw


def pack_embedding_ref(e, rows_pad):
    rows, d = e.shape
    out = torch.zeros(rows_pad, d, dtype=BF)
    out[:rows] = e.to(BF)
    return out


def cast_values(n):
    """fp32 values for the cast: random, plus exact ties both ways, a denormal, +-inf and NaN -- spread over the vector body and the scalar tail."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, generator=g) * 100.0
    special = torch.tensor([1.00390625, 1.01171875, -1.00390625, -1.01171875,   # 1 + 2^-8 (tie, rounds down to even), 1 + 3 * 2^-8 (tie, rounds up to even)
                            1e-40, -1e-40, float("inf"), float("-inf"), float("nan"), 3.3895313892515355e38, 3.4028234663852886e38, 0.0, -0.0],
                           dtype=F32)  # (the largest bf16 stays, the largest fp32 rounds to +inf)
    k = len(special)
    x[5:5 + k] = special
    x[n - k:] = special  # the last 5 of them are the scalar tail (n % 8 == 5)
    return x


def cast_ref(x):
    """Round to nearest even by integer arithmetic on the bit pattern (gemm_exact.rne_bf16) for finite values; inf stays inf, NaN stays NaN."""
    out = ge.rne_bf16(torch.where(torch.isfinite(x), x, torch.zeros_like(x)))
    return torch.where(torch.isfinite(x), out, x.to(BF))


def cast_equal(got, want):
    """Bit-exact except that any NaN matches any NaN."""
    gn, wn = torch.isnan(got), torch.isnan(want)
    return bool((gn == wn).all()) and bool((bits(got)[~gn] == bits(want)[~wn]).all())


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------------
LN_SHAPES = ((6149, 1024), (37, 512), (5, 520), (9, 1544), (3, 2048))
LN_KINDS = ("random", "offset", "offset_wide", "constant", "large")
NEEDLE_ROWS = (0, 2047, 2048, 4095, 4096, 6148)


def ln_inputs(rows, d, kind, seed=7):
    """x bf16 [rows, d], gamma / beta fp32 [d]."""
    g = torch.Generator().manual_seed(seed + rows + d)
    noise = torch.randn(rows, d, generator=g)
    if kind == "random":
        x = noise
    elif kind == "offset":
        x = 100.0 + 0.05 * noise  # (in bf16, whose spacing at 100 is 0.5, these rows are constant; the fp32 kernel sees the noise)
    elif kind == "offset_wide":
        x = 100.0 + 0.5 * noise   # the same offset with a spread that survives bf16: a mean of 100 under deviations of one or two grid steps
    elif kind == "constant":
        x = torch.randint(-3, 4, (rows, 1), generator=g).to(F32).expand(rows, d).clone()  # small integers: the fp32 row sum is exact
    else:
        x = 1e4 * noise
    gamma = 1.0 + 0.2 * torch.randn(d, generator=g)
    beta = 0.3 * torch.randn(d, generator=g)
    return x.to(BF), gamma.to(F32), beta.to(F32)


def ln_fwd_ref(x, gamma, beta):
    """float64 two-pass: y, mean, rstd."""
    xd = x.to(F64)
    mu = xd.mean(1, keepdim=True)
    var = ((xd - mu) ** 2).mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(var + 1e-5)
    return (xd - mu) * rs * gamma.to(F64) + beta.to(F64), mu[:, 0], rs[:, 0]


def ln_fwd_tol(x, gamma, y_ref, rstd_ref, out_ulp=True):
    """1 bf16 ulp of y + 16 * 2^-24 * max|x_row| * rstd * |gamma_j| (the fp32 rounding of a mean of up to 2048 values, carried through)."""
    t = 16 * E24 * x.to(F64).abs().amax(1, keepdim=True) * rstd_ref.view(-1, 1) * gamma.to(F64).abs().view(1, -1)
    return t + (ge.bf16_ulp(y_ref) if out_ulp else 0.0)


def ln_fwd_fp32_two_pass(x, gamma, beta):
    xf = x.to(F32)
    mu = xf.mean(1, keepdim=True)
    var = ((xf - mu) ** 2).mean(1, keepdim=True)
    return ((xf - mu) * torch.rsqrt(var + 1e-5) * gamma + beta).to(BF)


def ln_bwd_ref(dy, x, gamma, mean, rstd, dres=None):
    """float64 backward FROM THE GIVEN fp32 mean / rstd (they are inputs of the operator).  Returns dx (before the bf16 store), the float64
    column sums dgamma, dbeta, the per-element tolerance of dx, and xhat."""
    xh = (x.to(F64) - mean.to(F64).view(-1, 1)) * rstd.to(F64).view(-1, 1)
    gy = dy.to(F64) * gamma.to(F64)
    s1 = gy.mean(1, keepdim=True)
    s2 = (gy * xh).mean(1, keepdim=True)
    rs = rstd.to(F64).view(-1, 1)
    dx = rs * (gy - s1 - xh * s2)
    # the same rule applied to dx's own terms: the two fp32 row means (of gy, of gy * xhat) carry 16 * 2^-24 of their largest term, scaled by
    # rstd (and by |xhat_j| for the second); every other fp32 operation is a relative 2^-24 on a term of the sum; then the bf16 store(s)
    t = 16 * E24 * rs * (gy.abs().amax(1, keepdim=True) + xh.abs() * (gy * xh).abs().amax(1, keepdim=True))
    t = t + 8 * E24 * rs * (gy.abs() + s1.abs() + (xh * s2).abs())
    tol = t + ge.bf16_ulp(dx)
    if dres is not None:
        dx = dx + dres.to(F64)
        tol = tol + ge.bf16_ulp(dx)  # second rounding: bf16(bf16(dx) + dres)
    return dx, (dy.to(F64) * xh).sum(0), dy.to(F64).sum(0), tol, xh


def ln_dsum_ok(dsum, prefill, dx_stored):
    """For every column |dsum - prefill - sum(stored dx)| <= 2^-20 * sum|stored dx| (float64 from the returned bf16 dx); returns the bad columns."""
    s = dx_stored.to(F64).sum(0)
    a = dx_stored.to(F64).abs().sum(0)
    return ((dsum.to(F64) - prefill.to(F64) - s).abs() > 2.0 ** -20 * a).nonzero().flatten()


def ln_dsum_prefill(dx_ref):
    """A non-zero pre-fill the rule above can live with: the fp32 sum rounds at the magnitude of pre-fill + partial sums, so the pre-fill is
    kept at the size of ONE term of the column (mean |dx| of the float64 reference, never the kernel's output)."""
    return dx_ref.abs().mean(0).clamp_min(2.0 ** -100).to(F32)


def ln_bwd_emulate(dy, x, gamma, mean, rstd, dres=None, flaw=None):
    """fp32 stand-in for the kernel: dx bf16, dgamma / dbeta / dsum fp32 (without pre-fill)."""
    f = lambda t: t.to(F32)
    xh = (f(x) - mean.view(-1, 1)) * rstd.view(-1, 1)
    gy = f(dy) * gamma
    s1 = gy.mean(1, keepdim=True)
    s2 = (gy * xh).mean(1, keepdim=True)
    o = rstd.view(-1, 1) * (gy - s1 - xh * s2)
    if dres is not None:
        o = o.to(BF).to(F32) + f(dres)
    dx = o.to(BF)
    keep = slice(None, -1) if flaw == "last_row_dropped" else slice(None)
    dg = (f(dy) * xh)[keep].to(F64).sum(0).to(F32)
    db = f(dy)[keep].to(F64).sum(0).to(F32)
    src = o if flaw == "dsum_from_unrounded_dx" else dx.to(F32)
    ds = src[keep].to(F64).sum(0).to(F32)
    if flaw == "dead_second_row_counted":  # the clamped re-read of row0 is reduced a second time
        ds = ds + dx[-1].to(F32)
        dg = dg + (f(dy) * xh)[-1]
        db = db + f(dy)[-1]
    return dx, dg, db, ds


FLAWS = {
    "embedding_fwd": ("oob_id_clamped", "rowtab_ignored"),
    "embedding_bwd": ("pad_id_scattered", "oob_id_clamped", "dpos_overwritten", "span_ignored", "second_column_pass_missing"),
    "colsum": ("rows_past_m", "remainder_rows_dropped", "last_column_block_dropped"),
    "conv2": ("tap_from_neighbouring_sample", "last_odd_row_kk0_kept", "boundary_tap_dropped", "even_row_tap_0"),
    "conv1": ("tap_from_neighbouring_sample", "halo_row_dropped", "rotated_slot_read_unrotated", "partial_tile_unwritten"),
    "mel": ("floor_of_sample_0", "tail_tile_zero"),
    "pack_conv": ("tap_major_read_as_channel_major", "pad_not_zeroed"),
    "unpack_conv": ("overwrites",),
    "layernorm_bwd": ("dsum_from_unrounded_dx", "last_row_dropped", "dead_second_row_counted"),
}
