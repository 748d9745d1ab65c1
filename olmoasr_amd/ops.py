"""Thin tensor-level wrappers over the unit operators of liboasr (used by the op-level parity tests and by the
host-side mirrors).  bf16 tensors are torch.bfloat16; everything runs on the current HIP stream of the tensors' device."""
import ctypes as C
import math

import torch

from . import _native as N

BF = torch.bfloat16


def _op(t, ld=None, rpb=0, bstride=0, lead=0, kvalid=0, trail_from=0):
    return N.Operand(t.data_ptr(), ld if ld is not None else t.stride(0), rpb, bstride, lead, kvalid, trail_from)


def gemm(A, B, M, N_, K, *, ta=False, tb=False, a_view=None, b_view=None, bias=None, act=0, pos=None, pos_period=0,
         dgelu_u=None, resid=None, out=None, out_pre=None, ldc=None, out_f32=None, beta=0.0, atomic=False, split_k=1,
         alpha=1.0, colsum=None, dgelu_deriv=False, ldc32=None, colsum_scratch=None, atomic_on_pp=None, raster_gm=None, stagger=None,
         stagger_phases=None):
    """C[M,N] = epilogue(alpha * sum_k A(m,k) B(n,k)); see olmoasr_amd/csrc/kernels.h GemmArgs.  The last five keywords are the launch
    options only the engine sets; giving any of them routes the call through oasr_test_gemm (include/oasr_testing.h)."""
    g = N.GemmArgs()
    g.A = a_view if a_view is not None else _op(A)
    g.B = b_view if b_view is not None else _op(B)
    g.M, g.N, g.K, g.ta, g.tb, g.alpha = M, N_, K, int(ta), int(tb), alpha
    g.bias = bias.data_ptr() if bias is not None else None
    g.act = act
    g.pos = pos.data_ptr() if pos is not None else None
    g.pos_period = pos_period
    g.dgelu_u = dgelu_u.data_ptr() if dgelu_u is not None else None
    g.ldu = dgelu_u.stride(0) if dgelu_u is not None else 0
    g.resid = resid.data_ptr() if resid is not None else None
    g.ldr = resid.stride(0) if resid is not None else 0
    g.out = out.data_ptr() if out is not None else None
    g.out_pre = out_pre.data_ptr() if out_pre is not None else None
    g.ldc = ldc if ldc is not None else (out.stride(0) if out is not None else (out_pre.stride(0) if out_pre is not None else 0))
    g.out_f32 = out_f32.data_ptr() if out_f32 is not None else None
    g.ldc32 = ldc32 if ldc32 is not None else (out_f32.stride(0) if out_f32 is not None else 0)
    g.beta, g.atomic, g.split_k = beta, int(atomic), split_k
    g.colsum = colsum.data_ptr() if colsum is not None else None
    g.dgelu_deriv = int(dgelu_deriv)
    dev = next((t.device for t in (out, out_f32, out_pre) if t is not None), None)
    engine_only = (colsum_scratch, atomic_on_pp, raster_gm, stagger, stagger_phases)
    if all(x is None for x in engine_only):
        N.call("oasr_gemm", C.byref(g), N.STREAM, device=dev)
    else:
        N.call("oasr_test_gemm", C.byref(g), colsum_scratch, int(atomic_on_pp or 0), int(raster_gm or 0), int(stagger or 0),
               int(stagger_phases or 0), N.STREAM, device=dev)


def gemm_launch_records():
    """The GEMM launches since ``lib().oasr_profile_gemm(1)`` as dicts (include/oasr_testing.h: oasr_profile_gemm_records)."""
    buf = C.create_string_buffer(1 << 22)
    n = N.lib().oasr_profile_gemm_records(buf, len(buf))
    N.check(0 if n >= 0 else n, "oasr_profile_gemm_records")
    keys = ("M", "N", "K", "ta", "tb", "flags", "split_k", "atomic", "atomic_on_pp", "scratch", "stagger", "stagger_phases", "persistent", "lane")
    recs = []
    for line in buf.value.decode().splitlines():
        f = line.split("\t")
        recs.append(dict(zip(keys, map(int, f[1:])), symbol=f[0]))
    assert len(recs) == n
    return recs


def layernorm_fwd(x, gamma, beta):
    rows, d = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(rows, device=x.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    N.call("oasr_layernorm_fwd", x, gamma, beta, y, mean, rstd, rows, d, N.STREAM)
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, dres=None):
    rows, d = x.shape
    dx = torch.empty_like(x)
    dg = torch.zeros(d, device=x.device, dtype=torch.float32)
    db = torch.zeros_like(dg)
    N.call("oasr_layernorm_bwd", dy, x, gamma, mean, rstd, dres, dx, dg, db, rows, d, N.STREAM)
    return dx, dg, db


def _attn_args(q, k, v, o, lse, kv_len, causal):
    B, Tq, H, D = q.shape
    Tk = k.shape[1]
    assert D == 64 and q.stride(3) == 1 and q.stride(2) == 64
    a = N.AttnArgs()
    a.q, a.k, a.v = q.data_ptr(), k.data_ptr(), v.data_ptr()
    a.ldq, a.ldk, a.ldv = q.stride(1), k.stride(1), v.stride(1)
    a.bsq, a.bsk, a.bsv = q.stride(0), k.stride(0), v.stride(0)
    a.o, a.ldo, a.bso = o.data_ptr(), o.stride(1), o.stride(0)
    a.lse = lse.data_ptr()
    a.kv_len = kv_len.data_ptr() if kv_len is not None else None
    a.B, a.H, a.Tq, a.Tk, a.causal = B, H, Tq, Tk, int(causal)
    return a


def attention_fwd(q, k, v, kv_len=None, causal=False, want_o_lo=False):
    """q [B,Tq,H,64], k/v [B,Tk,H,64] (any token/batch strides) -> o [B,Tq,H*64], lse [B,H,Tq] (, o_lo = bf16 rounding residual of o)."""
    B, Tq, H, _ = q.shape
    o = torch.empty(B, Tq, H * 64, device=q.device, dtype=BF)
    lse = torch.empty(B, H, Tq, device=q.device, dtype=torch.float32)
    a = _attn_args(q, k, v, o.view(B, Tq, H, 64), lse, kv_len, causal)
    o_lo = torch.empty(B, Tq, H * 64, device=q.device, dtype=torch.bfloat16) if want_o_lo else None
    a.o_lo = o_lo.data_ptr() if want_o_lo else None
    N.call("oasr_attention_fwd", C.byref(a), N.STREAM, device=q.device)
    return (o, lse, o_lo) if want_o_lo else (o, lse)


def attention_scores(q, k, kv_len=None, causal=False):
    """``qk`` of the reference's manual attention path (MultiHeadAttention.qkv_attention, olmoasr/model.py:347-442): q [B,Tq,H,64],
    k [B,Tk,H,64] (bf16 or fp32, any token/batch strides) -> fp32 [B, H, Tq, Tk] pre-softmax scaled scores, -inf where masked."""
    B, Tq, H, _ = q.shape
    Tk = k.shape[1]
    assert q.dtype == k.dtype and q.dtype in (BF, torch.float32)
    assert q.stride(3) == 1 and q.stride(2) == 64 and k.stride(3) == 1 and k.stride(2) == 64
    out = torch.empty(B, H, Tq, Tk, device=q.device, dtype=torch.float32)
    a = N.AttnArgs()
    a.q, a.k = q.data_ptr(), k.data_ptr()
    a.ldq, a.ldk, a.bsq, a.bsk = q.stride(1), k.stride(1), q.stride(0), k.stride(0)
    a.kv_len = kv_len.data_ptr() if kv_len is not None else None
    a.B, a.H, a.Tq, a.Tk, a.causal = B, H, Tq, Tk, int(causal)
    N.call("oasr_attention_scores", C.byref(a), 0 if q.dtype == BF else 1, out, N.STREAM)
    return out


def attention_bwd(q, k, v, o, lse, d_o, kv_len=None, causal=False, o_lo=None, dq_colsum=None, dv_colsum=None, qtile_flags=None):
    """qtile_flags: optional int32 [B, H, ceil(Tq/64)] workspace -- all-zero 64-query tiles of d_o are recorded and skipped (bit-identical)."""
    B, Tq, H, _ = q.shape
    # gradients use the operands' own (possibly fused-qkv) strides
    dq, dk, dv = (torch.empty_strided(t.shape, t.stride(), device=t.device, dtype=t.dtype) for t in (q, k, v))
    delta = torch.empty(B, H, Tq, device=q.device, dtype=torch.float32)
    a = _attn_args(q, k, v, o.view(B, Tq, H, 64), lse, kv_len, causal)
    a.d_o, a.delta = d_o.data_ptr(), delta.data_ptr()
    a.o_lo = o_lo.data_ptr() if o_lo is not None else None
    a.dq, a.dk, a.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    a.dq_colsum = dq_colsum.data_ptr() if dq_colsum is not None else None
    a.dv_colsum = dv_colsum.data_ptr() if dv_colsum is not None else None
    a.qtile_flags = qtile_flags.data_ptr() if qtile_flags is not None else None
    scratch = None
    if dq_colsum is not None or dv_colsum is not None:
        Tk = k.shape[1]
        scratch = torch.empty(B * ((Tq + 127) // 128 + (Tk + 127) // 128) * H * 64, device=q.device, dtype=torch.float32)
        a.colsum_scratch = scratch.data_ptr()
    N.call("oasr_attention_bwd", C.byref(a), N.STREAM, device=q.device)
    return dq, dk, dv


# ---- chunked token rows (include/oasr.h: oasr_attn_args.q_rows / k_rows / q_span) -----------------------------------------------------
def chunk_rows_table(order, B, n_chunks):
    """Chunk-row table int32 [B, ROWTAB] (CPU) for a given placement: ``order`` lists the (b, chunk) pairs in the order their 64 rows
    appear in memory.  Entries past ``n_chunks`` hold the out-of-range sentinel the kernels expect."""
    tab = torch.full((B, N.ROWTAB), 0x3FFFFFFF, dtype=torch.int32)
    for i, (b, c) in enumerate(order):
        tab[b, c] = 64 * i
    assert int((tab[:, :n_chunks] == 0x3FFFFFFF).sum()) == 0, "every (b, chunk) needs a place"
    return tab


def to_chunked(x, tab):
    """x [B, T, ...] -> [B*T, ...] with the 64-position chunk c of sample b at rows tab[b, c] .. +63 (test helper)."""
    B, T = x.shape[:2]
    out = torch.empty((B * T,) + tuple(x.shape[2:]), device=x.device, dtype=x.dtype)
    for b in range(B):
        for c in range(T // 64):
            r = int(tab[b, c])
            out[r:r + 64] = x[b, 64 * c:64 * c + 64]
    return out


def from_chunked(xc, tab, B, T):
    out = torch.empty((B, T) + tuple(xc.shape[1:]), device=xc.device, dtype=xc.dtype)
    for b in range(B):
        for c in range(T // 64):
            r = int(tab[b, c])
            out[b, 64 * c:64 * c + 64] = xc[r:r + 64]
    return out


def span_block_tables(span, B, S, H, device="cuda", with_rows=False):
    """The query-block tables of the span-limited attention launches (include/oasr.h: oasr_attn_args.qblk128 / qblk256) for the HOST
    spans ``span`` (int32 [B]) and H heads, built by the device kernel oasr_train_step uses: returns (blk128, blk256, n128, n256) --
    device int32 tensors with room for every block of the padded context, and the number of blocks inside the spans per head.
    with_rows: also the chunk-row table [B, ROWTAB] and the spans rounded up to 64 (device int32) of the same launch."""
    span = torch.as_tensor(span, dtype=torch.int32).cpu().contiguous()
    assert span.numel() == B
    blk128 = torch.full((B * ((S + 127) // 128) * H,), -1, dtype=torch.int32, device=device)
    blk256 = torch.full((B * ((S + 255) // 256) * H,), -1, dtype=torch.int32, device=device)
    targets = torch.full((B, S), 51864, dtype=torch.int64, device=device)
    rows = torch.empty(B, N.ROWTAB, dtype=torch.int32, device=device)
    span_d = torch.empty(B, dtype=torch.int32, device=device)
    tphys = torch.empty(B * S, dtype=torch.int64, device=device)
    counts = (C.c_int32 * 2)()
    N.call("oasr_test_span_block_tables", span, B, S, H, targets, rows, span_d, tphys, blk128, blk256, counts, N.STREAM)
    blocks = (blk128, blk256, int(counts[0]), int(counts[1]))
    return (blocks, rows, span_d) if with_rows else blocks


def _set_blocks(a, q_blocks):
    if q_blocks is not None:
        blk128, blk256, n128, n256 = q_blocks
        a.qblk128, a.qblk256, a.n128, a.n256 = blk128.data_ptr(), blk256.data_ptr(), n128, n256


def _attn_args_rows(qc, kc, vc, oc, lse, B, H, Tq, Tk, q_rows, k_rows, kv_len, causal):
    """qc / oc: chunked [B*Tq, H, 64] views (any token stride); kc / vc: chunked [B*Tk, H, 64] when k_rows is given, else plain [B, Tk, H, 64]."""
    a = N.AttnArgs()
    a.q, a.k, a.v, a.o = qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), oc.data_ptr()
    a.ldq, a.ldo = qc.stride(0), oc.stride(0)
    if k_rows is not None:
        a.ldk, a.ldv = kc.stride(0), vc.stride(0)
        a.k_rows = k_rows.data_ptr()
    else:
        a.ldk, a.ldv, a.bsk, a.bsv = kc.stride(1), vc.stride(1), kc.stride(0), vc.stride(0)
    a.lse = lse.data_ptr()
    a.kv_len = kv_len.data_ptr() if kv_len is not None else None
    a.B, a.H, a.Tq, a.Tk, a.causal = B, H, Tq, Tk, int(causal)
    a.q_rows = q_rows.data_ptr()
    return a


def attention_fwd_rows(qc, kc, vc, B, H, Tq, Tk, q_rows, k_rows=None, kv_len=None, causal=False, want_o_lo=False, q_span=None, q_blocks=None,
                       fill=None):
    """attention_fwd on chunked token rows: returns oc [B*Tq, H*64] (chunked like qc), lse [B, H, Tq] (logical)(, o_lo).
    q_span (device int32 [B]): the span-limited forward -- rows past it are not computed; q_blocks: ``span_block_tables`` of the same spans
    (compact grid); fill: the outputs are pre-filled with it, so that a test can see which rows were left untouched."""
    oc = torch.empty(B * Tq, H * 64, device=qc.device, dtype=BF)
    lse = torch.empty(B, H, Tq, device=qc.device, dtype=torch.float32)
    o_lo = torch.empty_like(oc) if want_o_lo else None
    if fill is not None:
        for t in (oc, lse, o_lo):
            if t is not None:
                t.fill_(fill)
    a = _attn_args_rows(qc, kc, vc, oc.view(B * Tq, H, 64), lse, B, H, Tq, Tk, q_rows, k_rows, kv_len, causal)
    a.o_lo = o_lo.data_ptr() if want_o_lo else None
    a.q_span = q_span.data_ptr() if q_span is not None else None
    _set_blocks(a, q_blocks)
    N.call("oasr_attention_fwd", C.byref(a), N.STREAM, device=qc.device)
    return (oc, lse, o_lo) if want_o_lo else (oc, lse)


def attention_bwd_rows(qc, kc, vc, oc, lse, doc, B, H, Tq, Tk, q_rows, k_rows=None, q_span=None, kv_len=None, causal=False, o_lo=None,
                       dq_colsum=None, dv_colsum=None, fill=None, q_blocks=None, scratch_fill=None, qtile_flags=None):
    """attention_bwd on chunked token rows.  Gradients are allocated with the operands' strides and pre-filled with ``fill`` (e.g. NaN)
    so that a test can see which rows the kernels left untouched.  q_blocks: ``span_block_tables`` of the spans in q_span (compact
    grids); scratch_fill: what the bias gradients' scratch rows hold on entry (nothing may depend on it)."""
    def like(t):
        g = torch.empty_strided(t.shape, t.stride(), device=t.device, dtype=t.dtype)
        if fill is not None:
            g.fill_(fill)
        return g
    dq, dk, dv = like(qc), like(kc), like(vc)
    delta = torch.zeros(B, H, Tq, device=qc.device, dtype=torch.float32)
    a = _attn_args_rows(qc, kc, vc, oc.view(B * Tq, H, 64), lse, B, H, Tq, Tk, q_rows, k_rows, kv_len, causal)
    a.d_o, a.delta = doc.data_ptr(), delta.data_ptr()
    a.o_lo = o_lo.data_ptr() if o_lo is not None else None
    a.dq, a.dk, a.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    a.q_span = q_span.data_ptr() if q_span is not None else None
    a.dq_colsum = dq_colsum.data_ptr() if dq_colsum is not None else None
    a.dv_colsum = dv_colsum.data_ptr() if dv_colsum is not None else None
    a.qtile_flags = qtile_flags.data_ptr() if qtile_flags is not None else None  # (as in attention_bwd)
    scratch = None
    if dq_colsum is not None or dv_colsum is not None:
        scratch = torch.empty(B * ((Tq + 127) // 128 + (Tk + 127) // 128) * H * 64, device=qc.device, dtype=torch.float32)
        if scratch_fill is not None:
            scratch.fill_(scratch_fill)
        a.colsum_scratch = scratch.data_ptr()
    _set_blocks(a, q_blocks)
    N.call("oasr_attention_bwd", C.byref(a), N.STREAM, device=qc.device)
    return dq, dk, dv


# ---- word-timestamp alignment (csrc/align.hip; timing.find_alignment(backend="native")) --------------------------------------------------
_ws_cache = {}  # (operator, device index) -> uint8 workspace, grown on demand and reused by later calls on that device


def _workspace(kind, device, need):
    key = (kind, torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device())
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < need:
        _ws_cache[key] = None
        ws = _ws_cache[key] = torch.empty(max(int(need), 16), dtype=torch.uint8, device=device)
    return ws


MEDFILT_WIDTHS = (1, 3, 5, 7, 9, 11, 13, 15)  # 7 (whisper's), 1 and 3 are the required ones; the other odd widths run the generic network


def alignment_matrix(qk_layers, heads_per_layer, n_frames, medfilt_width=7, qk_scale=1.0, out=None):
    """The [tokens, frames] alignment matrix of ``timing.find_alignment`` from the cross-attention score planes, in one operator:

        out[i, j] = mean over the selected heads h of  median_w( z_h[i, reflect(j - w/2 .. j + w/2)] )
        z_h[i, j] = (p_h[i, j] - mean_i p_h[., j]) / std_i p_h[., j]       (population std over ALL rows)
        p_h[i, .] = softmax over j < n_frames of qk_scale * qk_h[i, j]

    ``qk_layers``: fp32 tensors [H, n_tok, Tk], contiguous, as ``timing.cross_attention_scores`` returns them (at most 32);
    ``heads_per_layer``: for each of them the head indices that take part (each at most once; the order is irrelevant).  The planes are read in place -- no stacked copy; unselected
    heads and frames >= n_frames are never read.  1 <= n_frames <= Tk; ``medfilt_width`` odd, 1 .. 15; no filter when
    n_frames <= medfilt_width // 2 (``timing.median_filter``'s rule).  Returns fp32 [n_tok, n_frames] (``out``: a caller's tensor of that
    shape with unit column stride).  Bad arguments raise ValueError before anything is launched.  A column whose variance over the tokens
    is exactly zero is outside the contract, here as in ``timing.alignment_matrix_torch`` (which yields NaN there)."""
    qk_layers, heads_per_layer = list(qk_layers), [[int(h) for h in hs] for hs in heads_per_layer]
    if any(len(set(hs)) != len(hs) for hs in heads_per_layer):  # (a head named twice would count twice in the torch path's mean and once in a bit mask)
        raise ValueError("alignment_matrix: a head index is repeated within a layer")
    if not qk_layers or len(qk_layers) != len(heads_per_layer) or len(qk_layers) > N.AlignArgs.MAX_LAYERS:
        raise ValueError(f"alignment_matrix: {len(qk_layers)} score tensors for {len(heads_per_layer)} head lists (1 .. {N.AlignArgs.MAX_LAYERS}, one list each)")
    shape = tuple(qk_layers[0].shape)
    for t in qk_layers:
        if not (isinstance(t, torch.Tensor) and t.dim() == 3 and tuple(t.shape) == shape and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError("alignment_matrix: every score tensor is a contiguous fp32 [H, n_tok, Tk] of the same shape")
    H, n_tok, Tk = shape
    if not (1 <= H <= 32 and 1 <= n_tok <= 65535 and Tk >= 1):
        raise ValueError(f"alignment_matrix: H = {H} (1 .. 32), n_tok = {n_tok} (1 .. 65535), Tk = {Tk}")
    if any(h < 0 or h >= H for hs in heads_per_layer for h in hs) or not any(heads_per_layer):
        raise ValueError(f"alignment_matrix: head indices must lie in [0, {H}) and at least one head must be selected")
    n_frames, medfilt_width = int(n_frames), int(medfilt_width)
    if not 1 <= n_frames <= Tk:
        raise ValueError(f"alignment_matrix: n_frames = {n_frames} outside [1, Tk = {Tk}]")
    if medfilt_width not in MEDFILT_WIDTHS:
        raise ValueError(f"alignment_matrix: medfilt_width = {medfilt_width}: an odd width from 1 to 15")
    dev = qk_layers[0].device
    for t in qk_layers:
        N.require_gpu(t, "alignment_matrix: score tensor")
        if t.device != dev:
            raise ValueError("alignment_matrix: score tensors on different devices")
    if out is None:
        out = torch.empty(n_tok, n_frames, device=dev, dtype=torch.float32)
    elif not (out.dtype == torch.float32 and tuple(out.shape) == (n_tok, n_frames) and out.device == dev and (out.stride(1) == 1 or n_frames == 1)
              and out.stride(0) >= n_frames):
        raise ValueError("alignment_matrix: out must be fp32 [n_tok, n_frames] on the scores' device with unit column stride")
    a = N.AlignArgs()
    for l, (t, hs) in enumerate(zip(qk_layers, heads_per_layer)):
        a.qk[l] = t.data_ptr()
        a.head_mask[l] = sum(1 << h for h in hs)
    a.n_layers, a.H, a.n_tok, a.Tk, a.n_frames, a.medfilt_width, a.qk_scale = len(qk_layers), H, n_tok, Tk, n_frames, medfilt_width, float(qk_scale)
    a.out, a.ldo = out.data_ptr(), out.stride(0)
    nsel = sum(len(hs) for hs in heads_per_layer)
    ws = _workspace("alignment_matrix", dev, N.lib().oasr_alignment_workspace_bytes(nsel, n_tok, n_frames))
    N.call("oasr_alignment_matrix", C.byref(a), ws, ws.numel(), N.STREAM)
    return out


def _dtw_check(cost):
    if not (isinstance(cost, torch.Tensor) and cost.dim() == 2 and cost.dtype == torch.float32):
        raise ValueError("dtw: cost must be an fp32 [N, M] tensor")
    n, m = cost.shape
    if not (1 <= n <= N.DTW_MAX_N and 1 <= m <= N.DTW_MAX_M):
        raise ValueError(f"dtw: cost of {n} x {m}: 1 <= N <= {N.DTW_MAX_N} (n_text_ctx) and 1 <= M <= {N.DTW_MAX_M} (n_audio_ctx)")
    if m > 1 and cost.stride(1) != 1:
        raise ValueError("dtw: cost needs unit column stride (any row stride)")
    if n > 1 and cost.stride(0) < m:
        raise ValueError("dtw: cost rows overlap")
    return int(n), int(m)


def dtw_device(cost, negate=False, path=None, workspace=None):
    """``dtw`` with everything left on the device: returns (path, workspace) -- ``path`` int32 [2 * (N + M - 1) + 1] holds the text indices, the
    time indices (the first ``len`` of N + M - 1 entries each) and ``len`` in its last element.  ``path`` / ``workspace``: caller's buffers."""
    n, m = _dtw_check(cost)
    N.require_gpu(cost, "dtw: cost")
    P = n + m - 1
    need = N.lib().oasr_dtw_workspace_bytes(n, m)
    if path is None:
        path = torch.empty(2 * P + 1, device=cost.device, dtype=torch.int32)
    if workspace is None:
        workspace = _workspace("dtw", cost.device, need)
    assert path.dtype == torch.int32 and path.numel() == 2 * P + 1 and path.is_contiguous() and workspace.dtype == torch.uint8
    ld = cost.stride(0) if n > 1 else max(m, cost.stride(0))
    N.call("oasr_dtw", cost, ld, n, m, int(bool(negate)), path, path[P:], path[2 * P:], workspace, workspace.numel(), N.STREAM)
    return path, workspace


def dtw(cost, negate=False):
    """``timing.dtw`` on the device, bit for bit: cost fp32 [N, M] (any row stride; ``negate``: the alignment of ``-cost``),
    1 <= N <= 448, 1 <= M <= 1500 -> (text_indices, time_indices), int64 CPU tensors, after ONE device-to-host copy of the path.
    Out-of-range shapes raise ValueError before anything is launched."""
    n, m = _dtw_check(cost)
    path, _ = dtw_device(cost, negate)
    host = path.cpu()
    P, ln = n + m - 1, int(host[-1])
    return host[:ln].to(torch.int64), host[P:P + ln].to(torch.int64)


def dtw_host(cost, negate=False):
    """include/oasr_testing.h: oasr_test_dtw_host -- the kernel's wavefront, skewed trace and backtrace run on the CPU (``cost``: CPU fp32)."""
    n, m = _dtw_check(cost)
    assert not cost.is_cuda
    P = n + m - 1
    path = torch.full((2 * P + 1,), -1, dtype=torch.int32)
    ws = torch.empty(N.lib().oasr_dtw_workspace_bytes(n, m), dtype=torch.uint8)
    ld = cost.stride(0) if n > 1 else max(m, cost.stride(0))
    N.call("oasr_test_dtw_host", cost, ld, n, m, int(bool(negate)), path, path[P:], path[2 * P:], ws)
    ln = int(path[-1])
    return path[:ln].to(torch.int64), path[P:P + ln].to(torch.int64)


def _edit_args(hyp, hyp_len, ref, ref_len, cuda):
    """Checks and converts the operands of ``edit_counts`` / ``edit_counts_host``: (EditArgs, out, keep-alive tuple)."""
    what = "edit_counts" if cuda else "edit_counts_host"
    for t, nm in ((hyp, "hyp"), (ref, "ref"), (hyp_len, "hyp_len"), (ref_len, "ref_len")):
        if not (isinstance(t, torch.Tensor) and t.dtype in (torch.int32, torch.int64)):
            raise ValueError(f"{what}: {nm} must be an int32 / int64 tensor")
        if t.is_cuda != cuda:
            raise ValueError(f"{what}: {nm} must be a {'GPU' if cuda else 'CPU'} tensor")
        if t.device != hyp.device:
            raise ValueError(f"{what}: operands on different devices")
    if hyp.dim() != 2 or ref.dim() != 2 or hyp_len.dim() != 1 or ref_len.dim() != 1:
        raise ValueError(f"{what}: hyp [B, Lh], ref [B, Lr], hyp_len [B], ref_len [B]")
    B, Lh = hyp.shape
    Lr = ref.shape[1]
    if B < 1 or ref.shape[0] != B or hyp_len.numel() != B or ref_len.numel() != B:
        raise ValueError(f"{what}: B mismatch (hyp {tuple(hyp.shape)}, ref {tuple(ref.shape)}, hyp_len {hyp_len.numel()}, ref_len {ref_len.numel()}; B >= 1)")

    def rows(t):  # int32, unit column stride, rows that do not overlap (any row stride beyond that: a view is passed as it is)
        t = t.to(torch.int32)
        ok = (t.shape[1] <= 1 or t.stride(1) == 1) and (B == 1 or t.stride(0) >= t.shape[1])
        return t if ok else t.contiguous()
    hyp, ref = rows(hyp), rows(ref)
    hyp_len, ref_len = hyp_len.to(torch.int32).contiguous(), ref_len.to(torch.int32).contiguous()
    out = torch.empty(B, 4, dtype=torch.int32, device=hyp.device)
    a = N.EditArgs()
    a.hyp, a.ref, a.hyp_len, a.ref_len, a.out = hyp.data_ptr(), ref.data_ptr(), hyp_len.data_ptr(), ref_len.data_ptr(), out.data_ptr()
    a.ld_hyp, a.ld_ref = (hyp.stride(0) if B > 1 else Lh), (ref.stride(0) if B > 1 else Lr)
    a.B, a.Lh, a.Lr = B, Lh, Lr
    return a, out, (hyp, ref, hyp_len, ref_len)


def edit_counts(hyp, hyp_len, ref, ref_len, out=None):
    """Batched token edit distance with its split (include/oasr.h: oasr_edit_counts; the rule: csrc/editdist_core.h): ``hyp`` [B, Lh] and
    ``ref`` [B, Lr] token ids, ``hyp_len`` / ``ref_len`` [B] with 0 <= length <= min(1023, row width), all on the GPU (int32; int64 is
    converted) -> int32 [B, 4] = (substitutions, deletions, insertions, hits) per pair, H = ref_len - S - D.  Ties prefer the diagonal, then
    the deletion, then the insertion.  One launch on the current stream and no host read: the lengths stay on the device, so a pair whose
    length is outside the contract yields (-1, -1, -1, -1) instead of an exception.  Wrong shapes / dtypes / devices raise ValueError
    before anything is launched.  ``out``: a caller's contiguous int32 [B, 4]."""
    a, res, keep = _edit_args(hyp, hyp_len, ref, ref_len, True)
    if out is not None:
        if not (isinstance(out, torch.Tensor) and out.dtype == torch.int32 and tuple(out.shape) == (a.B, 4) and out.is_contiguous()
                and out.device == keep[0].device):
            raise ValueError("edit_counts: out must be a contiguous int32 [B, 4] on the operands' device")
        res, a.out = out, out.data_ptr()
    N.call("oasr_edit_counts", C.byref(a), N.STREAM, device=res.device)
    return res


def edit_counts_host(hyp, hyp_len, ref, ref_len):
    """``edit_counts`` on CPU tensors through the library's host twin (oasr_edit_counts_host: the same rule from the same text, no GPU).
    Here the lengths are readable, so one outside [0, min(1023, row width)] raises ValueError."""
    a, out, keep = _edit_args(hyp, hyp_len, ref, ref_len, False)
    for nm, ln, w in (("hyp_len", keep[2], a.Lh), ("ref_len", keep[3], a.Lr)):
        if int(ln.min()) < 0 or int(ln.max()) > min(N.EditArgs.MAX_LEN, w):
            raise ValueError(f"edit_counts_host: {nm} outside [0, min({N.EditArgs.MAX_LEN}, row width {w})]")
    N.call("oasr_edit_counts_host", C.byref(a))
    return out


SCORE_IGNORE = 51864  # the training layout's pad id (csrc/engine_ctx.h: PAD_ID)


def _score_targets(what, targets, span, cuda):
    """Checks and converts ``targets`` [B, S] / ``span`` [B] (None: every row) of the score operators: (targets i64, span i32, B, S)."""
    if not (isinstance(targets, torch.Tensor) and targets.dim() == 2 and targets.dtype in (torch.int32, torch.int64)):
        raise ValueError(f"{what}: targets must be an int32 / int64 tensor [B, S]")
    B, S = targets.shape
    if B < 1 or S < 1:
        raise ValueError(f"{what}: targets {tuple(targets.shape)}: B and S must be positive")
    if targets.is_cuda != cuda:
        raise ValueError(f"{what}: targets must be a {'GPU' if cuda else 'CPU'} tensor")
    if span is None:
        span = torch.full((B,), S, dtype=torch.int32, device=targets.device)
    if not (isinstance(span, torch.Tensor) and span.dtype in (torch.int32, torch.int64) and span.dim() == 1 and span.numel() == B):
        raise ValueError(f"{what}: span must be an int32 / int64 tensor [B = {B}]")
    if span.device != targets.device:
        raise ValueError(f"{what}: targets on {targets.device}, span on {span.device}")
    return targets.to(torch.int64).contiguous(), span.to(torch.int32).contiguous(), B, S


def score_rows(logits, V, targets, span=None, ignore=SCORE_IGNORE):
    """Per-row negative log-likelihood and argmax of computed logits in one read of each row (include/oasr.h: oasr_score_rows).

    ``logits`` bf16 / fp32 [B * S, ld] or [B, S, ld] on the GPU (unit column stride, rows ld apart), of which the first ``V`` columns are
    valid; ``targets`` int [B, S]; ``span`` int [B] or None (every row).  Returns (row_nll f32 [B, S], pred int32 [B, S]): rows at or past
    the span hold (0, -1) and are not read; the others hold the argmax over c < V (lowest index among equal maxima) and, for a valid target
    (0 <= t < V, t != ignore), logsumexp(x[:V]) - x_t, else exactly 0.  One launch on the current stream, no host read."""
    if not (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dtype in (BF, torch.float32)):
        raise ValueError("score_rows: logits must be a bf16 / fp32 GPU tensor")
    targets, span, B, S = _score_targets("score_rows", targets, span, True)
    if logits.dim() == 3:
        if logits.shape[:2] != (B, S) or (B > 1 and logits.stride(0) != S * logits.stride(1)):
            raise ValueError(f"score_rows: logits {tuple(logits.shape)} must be [B = {B}, S = {S}, ld] with evenly spaced rows")
        ld, width, unit = logits.stride(1), logits.shape[2], logits.stride(2)
    elif logits.dim() == 2 and logits.shape[0] == B * S:
        ld, width, unit = logits.stride(0), logits.shape[1], logits.stride(1)
    else:
        raise ValueError(f"score_rows: logits {tuple(logits.shape)} must be [B * S = {B * S}, ld] or [B, S, ld]")
    V = int(V)
    if not (1 <= V <= width) or (width > 1 and unit != 1) or (B * S > 1 and ld < width):
        raise ValueError(f"score_rows: need 1 <= V = {V} <= {width} columns, unit column stride and a row stride >= the row width")
    if targets.device != logits.device:
        raise ValueError("score_rows: logits and targets on different devices")
    row_nll = torch.empty(B, S, dtype=torch.float32, device=logits.device)
    pred = torch.empty(B, S, dtype=torch.int32, device=logits.device)
    N.call("oasr_score_rows", logits, 0 if logits.dtype == BF else 1, ld if B * S > 1 else width, V, targets, span, B, S, int(ignore), row_nll,
           pred, N.STREAM)
    return row_nll, pred


def _score_reduce(what, row_nll, pred, targets, span, V, ignore, cuda):
    targets, span, B, S = _score_targets(what, targets, span, cuda)
    for t, nm, dt in ((row_nll, "row_nll", torch.float32), (pred, "pred", torch.int32)):
        if not (isinstance(t, torch.Tensor) and t.dtype == dt and tuple(t.shape) == (B, S) and t.device == targets.device):
            raise ValueError(f"{what}: {nm} must be a {dt} tensor [B = {B}, S = {S}] on the targets' device")
    if int(V) < 1:
        raise ValueError(f"{what}: V = {V} must be positive")
    dev = targets.device
    out = (torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev),
           torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
    args = (row_nll.contiguous(), pred.contiguous(), targets, span, B, S, int(V), int(ignore)) + out
    if cuda:
        N.call("oasr_score_reduce", *args, N.STREAM)
    else:
        N.call("oasr_score_reduce_host", *args)
    return out


def score_reduce(row_nll, pred, targets, span=None, *, V, ignore=SCORE_IGNORE):
    """Per-sample totals of ``score_rows``' output (include/oasr.h: oasr_score_reduce; the rule: csrc/score_core.h): over the rows with
    s < span[b] and a valid target, (nll_sum f32 [B]: a double sum in ascending s rounded once, nll_max f32 [B]: 0 if none, n_tok int32 [B],
    n_hit int32 [B]: pred == target).  GPU tensors, one launch on the current stream, no host read."""
    return _score_reduce("score_reduce", row_nll, pred, targets, span, V, ignore, True)


def score_reduce_host(row_nll, pred, targets, span=None, *, V, ignore=SCORE_IGNORE):
    """``score_reduce`` on CPU tensors through the library's host twin (oasr_score_reduce_host: the same rule from the same text, no GPU);
    the two agree bit for bit."""
    return _score_reduce("score_reduce_host", row_nll, pred, targets, span, V, ignore, False)


class BeamState:
    """What a device-resident beam search keeps between steps (include/oasr.h at oasr_beam_update), on one device -- the GPU, or the CPU
    for ``beam_update_host``: the two ``[n, n_ctx]`` int64 token buffers a step alternates between (``tokens`` is the current one, ``len``
    tokens of each row are meaningful), the fp32 ``sums``, the int32 ``sources`` and int64 ``last_token`` of the last step, the pool of
    finished sequences (``pool_tokens`` [n_audio, C, n_ctx], ``pool_len``, ``pool_score`` f64) and ONE int32 ``status`` tensor
    [3, n_audio] = (pool_count, pool_full_len, short_step) so that a poll is a single device read.  Built by ``beam_state``."""

    def __init__(self, n_audio, beam, max_candidates, n_ctx, init_tokens, device, fill=0, guard=0):
        init = [int(t) for t in init_tokens]
        if not 1 <= beam <= N.BeamArgs.MAX_BEAM:
            raise ValueError(f"beam_state: beam must be in [1, {N.BeamArgs.MAX_BEAM}], got {beam}")
        if n_audio < 1 or max_candidates < 1 or not 1 <= len(init) < n_ctx:
            raise ValueError("beam_state: n_audio >= 1, max_candidates >= 1 and 1 <= len(init_tokens) < n_ctx")
        self.n_audio, self.beam, self.max_candidates, self.n_ctx, self.len = n_audio, beam, max_candidates, n_ctx, len(init)
        self.device, self.cur, self.backing, self.guard = torch.device(device), 0, {}, guard
        n = n_audio * beam

        def alloc(name, shape, dtype, value):  # `guard` rows of `fill` on either side of every tensor: nothing may write them
            back = torch.full((shape[0] + 2 * guard, *shape[1:]), fill, dtype=dtype, device=self.device)
            view = back[guard:guard + shape[0]]
            if value is not None:
                view.fill_(value)
            self.backing[name] = back
            return view
        self.buffers = [alloc("tokens0", (n, n_ctx), torch.int64, None), alloc("tokens1", (n, n_ctx), torch.int64, None)]
        self.buffers[0][:, :len(init)] = torch.tensor(init, dtype=torch.int64, device=self.device)
        self.sums = alloc("sums", (n,), torch.float32, 0.0)
        self.sources = alloc("sources", (n,), torch.int32, None)
        self.sources.copy_(torch.arange(n, dtype=torch.int32, device=self.device))
        self.last_token = alloc("last_token", (n,), torch.int64, init[-1])
        self.pool_tokens = alloc("pool_tokens", (n_audio, max_candidates, n_ctx), torch.int64, None)
        self.pool_len = alloc("pool_len", (n_audio, max_candidates), torch.int32, 0)
        self.pool_score = alloc("pool_score", (n_audio, max_candidates), torch.float64, None)
        self.status = alloc("status", (3, n_audio), torch.int32, 0)
        self.status[1].fill_(N.BeamArgs.NOT_FULL)

    @property
    def tokens(self):
        return self.buffers[self.cur]

    def read_status(self):
        """ONE device read: (completed, any short step, live length, pool counts).  ``completed``: every window's pool is full -- later
        updates are latched and change nothing; the live rows then hold ``live length`` tokens, those of the step that completed."""
        count, full_len, short = self.status.cpu().tolist()
        completed = all(f != N.BeamArgs.NOT_FULL for f in full_len)
        return completed, any(short), (max(full_len) + 1 if completed else self.len), count


def beam_state(n_audio, beam, max_candidates, n_ctx, init_tokens, device, fill=0, guard=0):
    """The state of a beam search over ``n_audio`` windows x ``beam`` rows whose rows all start as ``init_tokens`` (the sot sequence), with
    pools of ``max_candidates`` finished sequences per window (``BeamState``).  ``fill`` / ``guard``: every tensor is allocated with ``guard``
    extra rows on either side, and those rows, the unused token columns and the pool hold ``fill`` (tests plant a sentinel there)."""
    return BeamState(n_audio, beam, max_candidates, n_ctx, init_tokens, device, fill, guard)


def _beam_update(state, top_lp, top_tok, eot, cuda):
    what = "beam_update" if cuda else "beam_update_host"
    n, K = state.n_audio * state.beam, state.beam + 1
    if not isinstance(state, BeamState) or (state.device.type == "cuda") != cuda:
        raise ValueError(f"{what}: the state must live on the {'GPU' if cuda else 'CPU'}")
    for t, nm, dt in ((top_lp, "top_lp", torch.float32), (top_tok, "top_tok", torch.int64)):
        if not (isinstance(t, torch.Tensor) and t.dtype == dt and tuple(t.shape) == (n, K) and t.is_contiguous() and t.device == state.sums.device):
            raise ValueError(f"{what}: {nm} must be a contiguous {dt} [{n}, {K}] (rows, beam + 1) on the state's device")
    if state.len + 1 > state.n_ctx:
        raise ValueError(f"{what}: the rows already hold n_ctx = {state.n_ctx} tokens")
    a = N.BeamArgs()
    a.top_logprob, a.top_token = top_lp.data_ptr(), top_tok.data_ptr()
    a.tokens_in, a.tokens_out = state.buffers[state.cur].data_ptr(), state.buffers[1 - state.cur].data_ptr()
    a.sums, a.sources, a.last_token = state.sums.data_ptr(), state.sources.data_ptr(), state.last_token.data_ptr()
    a.pool_tokens, a.pool_len, a.pool_score = state.pool_tokens.data_ptr(), state.pool_len.data_ptr(), state.pool_score.data_ptr()
    a.pool_count, a.pool_full_len, a.short_step = state.status[0].data_ptr(), state.status[1].data_ptr(), state.status[2].data_ptr()
    a.n_audio, a.beam, a.max_candidates, a.n_ctx, a.len, a.eot = state.n_audio, state.beam, state.max_candidates, state.n_ctx, state.len, int(eot)
    if cuda:
        N.call("oasr_beam_update", C.byref(a), N.STREAM, device=state.sums.device)
    else:
        N.call("oasr_beam_update_host", C.byref(a))
    state.cur, state.len = 1 - state.cur, state.len + 1
    return state


def beam_update(state, top_lp, top_tok, *, eot):
    """One BeamSearchDecoder.update for every window of ``state`` in one launch and with no host read (include/oasr.h: oasr_beam_update;
    the rule: csrc/beam_core.h): ``top_lp`` f32 / ``top_tok`` int64 [n_audio * beam, beam + 1] from ``topk_tokens``.  Afterwards
    ``state.tokens`` (the other buffer) holds the next rows with ``state.len`` tokens each, ``state.sums`` their fp32 scores,
    ``state.sources`` the row each continues (``kv_cache_reorder_native``) and ``state.last_token`` the appended tokens (``kv_cache_step``);
    sequences that ended in ``eot`` went to the pool.  Wrong shapes / dtypes / devices raise ValueError before anything is launched."""
    return _beam_update(state, top_lp, top_tok, eot, True)


def beam_update_host(state, top_lp, top_tok, *, eot):
    """``beam_update`` on a CPU state and CPU tensors through the library's host twin (oasr_beam_update_host: the same rule from the same
    text, no GPU)."""
    return _beam_update(state, top_lp, top_tok, eot, False)


def kv_reorder_host(rows, pos, group, sources):
    """``OLMoASR.kv_cache_reorder_native`` on a host copy of the self-attention cache rows (oasr_decode_reorder_host): ``rows`` CPU bf16 / fp32
    [L, B, n_ctx, 3d], contiguous, in place -- row j of every layer continues row ``sources[j]`` over the k | v columns of positions
    < ``pos``.  A source outside its destination's group of ``group`` rows raises ValueError before anything moves."""
    if not (isinstance(rows, torch.Tensor) and not rows.is_cuda and rows.dim() == 4 and rows.is_contiguous() and rows.dtype in (BF, torch.float32)
            and rows.shape[3] % 3 == 0):
        raise ValueError("kv_reorder_host: rows must be a contiguous CPU bf16 / fp32 [L, B, n_ctx, 3d]")
    L, B, n_ctx, d3 = rows.shape
    src = torch.as_tensor(sources, dtype=torch.int32).reshape(-1).contiguous()
    if not (1 <= group <= N.BeamArgs.MAX_BEAM and B % group == 0 and src.numel() == B and 0 <= pos <= n_ctx):
        raise ValueError(f"kv_reorder_host: {B} sources, 1 <= group <= {N.BeamArgs.MAX_BEAM} dividing B, 0 <= pos <= n_ctx")
    lo = torch.arange(B, dtype=torch.int32) // group * group
    if bool(((src < lo) | (src >= lo + group)).any()):
        raise ValueError(f"kv_reorder_host: a source lies outside its destination's group of {group} rows (beams never cross windows)")
    N.call("oasr_decode_reorder_host", rows, rows.stride(0) * rows.element_size(), L, B, n_ctx, d3 // 3, rows.element_size(), int(pos), int(group), src)
    return rows


def check_loss_regularisers(label_smoothing, z_loss, who):
    """The refusals of the C side (``check_ce_reg``): label_smoothing in [0, 1), z_loss >= 0, both finite.  Returns them as floats."""
    eps, z = float(label_smoothing), float(z_loss)
    if not (math.isfinite(eps) and 0.0 <= eps < 1.0):
        raise ValueError(f"{who}: label_smoothing = {label_smoothing!r} must be finite and inside [0, 1)")
    if not (math.isfinite(z) and z >= 0.0):
        raise ValueError(f"{who}: z_loss = {z_loss!r} must be finite and >= 0")
    return eps, z


def cross_entropy_(logits, V, targets, ignore, gscale=1.0, write_grad=True, label_smoothing=0.0, z_loss=0.0, return_parts=False):
    """In place on bf16 logits [rows, ld]: returns (mean loss over non-ignored rows, row_loss); logits become the gradient.
    ``label_smoothing`` eps / ``z_loss`` z (``oasr_cross_entropy_ex``; both 0 and no parts: the plain kernel, as ``oasr_cross_entropy``): per valid row
    ``lse - (1 - eps) x_t - eps / V sum_{c<V} x_c + z lse^2`` with the gradient ``g [(1 + 2 z lse) softmax - (1 - eps) onehot - eps / V]``.
    ``return_parts``: a third result, f32 [2, rows] = per-row (lse - x_t, lse^2)."""
    eps, z = check_loss_regularisers(label_smoothing, z_loss, "cross_entropy_")
    rows, ld = logits.shape
    nv = torch.zeros(1, device=logits.device, dtype=torch.int32)
    row_loss = torch.empty(rows, device=logits.device, dtype=torch.float32)
    loss = torch.zeros(1, device=logits.device, dtype=torch.float32)
    parts = torch.empty(2, rows, device=logits.device, dtype=torch.float32) if return_parts else None
    N.call("oasr_cross_entropy_ex", logits, logits.stride(0), V, targets, rows, ignore, gscale, nv, row_loss, loss, int(write_grad), eps, z,
           parts, N.STREAM)
    return (loss, row_loss, parts) if return_parts else (loss, row_loss)


def cast_bf16(x):
    out = torch.empty(x.shape, device=x.device, dtype=BF)
    N.call("oasr_cast_f32_bf16", x, out, x.numel(), N.STREAM)
    return out


def log_mel(pcm, finalize: bool = True):
    """pcm int16 or float32 [B, n] on the GPU -> float32 [B, 80, n // 160].  ``finalize=False``: returns (mel_raw, clip_max [B]) --
    whisper's last two lines (floor at the clip maximum - 8, (x + 4) / 4) left to the consumer (``loss_and_backward(mel_clip_max=...)``)."""
    N.require_gpu(pcm, "pcm")
    assert pcm.dim() == 2 and pcm.is_contiguous()
    B, n = pcm.shape
    if pcm.dtype == torch.int16:
        dt = 1
    elif pcm.dtype == torch.float32:
        dt = 0
    else:
        raise N.NativeError(f"log_mel: unsupported dtype {pcm.dtype}")
    mel = torch.empty(B, 80, n // 160, device=pcm.device, dtype=torch.float32)
    ws = torch.empty(N.lib().oasr_log_mel_workspace_bytes(B), device=pcm.device, dtype=torch.uint8)
    if not finalize:
        cm = torch.empty(B, device=pcm.device, dtype=torch.float32)
        N.call("oasr_log_mel_raw", pcm, dt, B, n, mel, cm, ws, N.STREAM)
        return mel, cm
    N.call("oasr_log_mel", pcm, dt, B, n, mel, ws, N.STREAM)
    return mel


_U64 = (1 << 64) - 1


def specaug_policy(freq_masks, freq_width, time_masks, time_width, fill=0.0):
    """The ``oasr_specaug`` block of a policy, refused here (ValueError) for what the library would refuse (OASR_EINVAL)."""
    for name, v in (("freq_masks", freq_masks), ("freq_width", freq_width), ("time_masks", time_masks), ("time_width", time_width)):
        if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v < 2 ** 31:
            raise ValueError(f"spec_augment: {name} must be an integer in [0, 2^31), got {v!r}")
    if freq_masks > N.SpecAug.MAX_MASKS or time_masks > N.SpecAug.MAX_MASKS:
        raise ValueError(f"spec_augment: at most {N.SpecAug.MAX_MASKS} masks of each kind, got {freq_masks} frequency / {time_masks} time masks")
    return N.SpecAug(freq_masks, freq_width, time_masks, time_width, float(fill))


def _u64(name, v, who):
    if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v <= _U64:
        raise ValueError(f"{who}: {name} must be an integer in [0, 2^64), got {v!r}")
    return v


def spec_augment_(mel, *, freq_masks, freq_width, time_masks, time_width, fill=0.0, seed=0, first_clip=0):
    """SpecAugment in place on finalized log-mel (include/oasr.h: oasr_spec_augment): mel fp32 [B, n_mels, T] or [n_mels, T], contiguous, on
    the GPU.  Row ``b`` takes the masks of stream id ``first_clip + b`` (mod 2^64) under ``seed``: ``freq_masks`` bands of width <=
    ``freq_width`` over all frames and ``time_masks`` spans of width <= ``time_width`` over all bins are set to ``fill``; no other cell is
    written.  ``time_width`` is taken as given (``augment.SpecAugment`` applies the cap relative to T).  One launch on the current stream;
    returns ``mel``."""
    N.require_gpu(mel, "spec_augment: mel")
    if mel.dtype != torch.float32:
        raise N.NativeError(f"spec_augment: unsupported dtype {mel.dtype} (float32 log-mel only)")
    if mel.dim() not in (2, 3):
        raise ValueError(f"spec_augment: mel must be [B, n_mels, T] or [n_mels, T], got {tuple(mel.shape)}")
    if not mel.is_contiguous():
        raise ValueError("spec_augment: mel must be contiguous (it is modified in place; a copy would take the masks with it)")
    pol = specaug_policy(freq_masks, freq_width, time_masks, time_width, fill)
    seed, first_clip = _u64("seed", seed, "spec_augment"), _u64("first_clip", first_clip, "spec_augment")
    B = mel.shape[0] if mel.dim() == 3 else 1
    n_mels, T = mel.shape[-2:]
    if B == 0:
        return mel
    if n_mels < 1 or T < 1:
        raise ValueError(f"spec_augment: n_mels = {n_mels} and T = {T} must be >= 1")
    N.call("oasr_spec_augment", mel, B, n_mels, T, C.byref(pol), seed, first_clip, N.STREAM)
    return mel


def spec_augment_plan(*, freq_masks, freq_width, time_masks, time_width, seed=0, clip=0, n_mels=80, T=3000):
    """The masks ``spec_augment_`` gives stream id ``clip``, from the library's host twin (oasr_spec_augment_plan; no GPU):
    (frequency masks, time masks), each a list of (start, width)."""
    pol = specaug_policy(freq_masks, freq_width, time_masks, time_width)
    if not (isinstance(n_mels, int) and isinstance(T, int) and 1 <= n_mels < 2 ** 31 and 1 <= T < 2 ** 31):
        raise ValueError(f"spec_augment: n_mels = {n_mels!r} and T = {T!r} must be integers in [1, 2^31)")
    f_iv, t_iv = (C.c_int32 * (2 * max(1, freq_masks)))(), (C.c_int32 * (2 * max(1, time_masks)))()
    N.call("oasr_spec_augment_plan", C.byref(pol), _u64("seed", seed, "spec_augment"), _u64("clip", clip, "spec_augment"), n_mels, T, f_iv, t_iv)
    return ([(f_iv[2 * i], f_iv[2 * i + 1]) for i in range(freq_masks)], [(t_iv[2 * i], t_iv[2 * i + 1]) for i in range(time_masks)])


def speed_policy(factors):
    """The ``oasr_speed`` block of a list of (P, Q) factors -- P / Q times faster -- refused here (ValueError) for what the library would
    refuse (OASR_EINVAL): 1 .. 8 pairs of coprime integers in [1, 32] with a ratio inside [1/2, 2]."""
    try:
        pairs = [tuple(f) for f in factors]
    except TypeError:
        raise ValueError(f"speed_perturb: factors must be a sequence of (P, Q) pairs, got {factors!r}")
    if not 1 <= len(pairs) <= N.Speed.MAX_FACTORS:
        raise ValueError(f"speed_perturb: between 1 and {N.Speed.MAX_FACTORS} factors, got {len(pairs)}")
    pol = N.Speed()
    pol.n_factors = len(pairs)
    for i, pq in enumerate(pairs):
        if len(pq) != 2 or any(not isinstance(v, int) or isinstance(v, bool) for v in pq):
            raise ValueError(f"speed_perturb: factor {pq!r} is not a pair of integers (P, Q)")
        p, q = pq
        if not (1 <= p <= 32 and 1 <= q <= 32):
            raise ValueError(f"speed_perturb: factor {p}/{q}: P and Q must lie in [1, 32]")
        if math.gcd(p, q) != 1:
            raise ValueError(f"speed_perturb: factor {p}/{q}: P and Q must be coprime")
        if q > 2 * p or p > 2 * q:
            raise ValueError(f"speed_perturb: factor {p}/{q}: the ratio must lie in [1/2, 2]")
        pol.P[i], pol.Q[i] = p, q
    return pol


def _prob_q16(who, prob):
    """``prob`` in [0, 1] as the library keeps it: round(prob * 65536), the chance of a clip to be drawn."""
    if isinstance(prob, bool) or not isinstance(prob, (int, float)) or not 0.0 <= prob <= 1.0:  # (a NaN fails the comparison)
        raise ValueError(f"{who}: prob must be a number in [0, 1], got {prob!r}")
    return int(round(prob * 65536))


# ---- the PCM operators (speed_perturb, noise_mix, reverb, telephone): what their operand checks and their entry points have in common -------------
def _rows_ld(what, t, nm, pcm, cuda, dtype=torch.int16, shape=None):
    """The row stride of ``t``: a 2-D ``dtype`` matrix (of ``shape``, if given) with unit column stride and rows that do not overlap, on
    the device of ``pcm``."""
    if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.dim() == 2):
        raise ValueError(f"{what}: {nm} must be a 2-D {dtype} tensor")
    if t.is_cuda != cuda or t.device != pcm.device:
        raise ValueError(f"{what}: {nm} must be a {'GPU' if cuda else 'CPU'} tensor on the device of pcm")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {nm} must be {list(shape)}, got {tuple(t.shape)}")
    if (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise ValueError(f"{what}: {nm} needs unit column stride and rows that do not overlap")
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _i32_vec(what, t, nm, n, pcm):
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.dim() == 1 and t.numel() == n and t.is_contiguous()
            and t.device == pcm.device):
        raise ValueError(f"{what}: {nm} must be a contiguous int32 [{n}] on the device of pcm")


def _pcm_in(what, pcm, n_valid, cuda):
    """Checks ``pcm`` int16 [B, N] and ``n_valid`` int32 [B]: (ld_in, B, N)."""
    if not isinstance(pcm, torch.Tensor) or pcm.is_cuda != cuda:
        raise ValueError(f"{what}: pcm must be a GPU tensor ({what}_host takes CPU tensors)" if cuda else f"{what}: pcm must be a CPU tensor")
    ld_in = _rows_ld(what, pcm, "pcm", pcm, cuda)
    B, n = pcm.shape
    _i32_vec(what, n_valid, "n_valid", B, pcm)
    if not 1 <= n <= N.SpeedArgs.MAX_N or B > N.NoiseArgs.MAX_ROWS:
        raise ValueError(f"{what}: pcm [B, N] with B <= 65535 and 1 <= N <= 2^26, got {tuple(pcm.shape)}")
    return ld_in, B, n


def _span(t, ld):
    """The bytes [lo, hi) of an int16 matrix with row stride ``ld``."""
    return t.data_ptr(), t.data_ptr() + 2 * ((t.shape[0] - 1) * ld + t.shape[1])


def _pcm_out(what, pcm, ld_in, out, cuda, in_place=False, bank=None, ld_bank=0):
    """``out`` (allocated if None) as the int16 [B, N] result of ``pcm``: it may not overlap ``pcm`` -- unless ``in_place`` and it is
    ``pcm`` itself -- or the ``bank``: (out, ld_out)."""
    if out is None:
        out = torch.empty(pcm.shape, dtype=torch.int16, device=pcm.device)
    ld_out = _rows_ld(what, out, "out", pcm, cuda, shape=pcm.shape)
    if pcm.shape[0]:
        (lo_i, hi_i), (lo_o, hi_o) = _span(pcm, ld_in), _span(out, ld_out)
        if lo_i < hi_o and lo_o < hi_i:
            if not in_place:
                raise ValueError(f"{what}: out overlaps pcm (the operator works out of place)")
            if not (lo_i == lo_o and ld_in == ld_out):
                raise ValueError(f"{what}: out overlaps pcm without being pcm itself (in place: the same tensor)")
        if bank is not None:
            lo_b, hi_b = _span(bank, ld_bank)
            if lo_b < hi_o and lo_o < hi_b:
                raise ValueError(f"{what}: out overlaps the bank")
    return out, ld_out


def _pcm_call(entry, a, pcm, cuda, workspace_bytes=None):
    """Runs ``oasr_<entry>`` on the current stream, or ``oasr_<entry>_host``, on a checked block; an empty batch calls nothing."""
    if not a.B:
        return
    if not cuda:
        N.call(f"oasr_{entry}_host", C.byref(a))
        return
    if workspace_bytes is not None:
        ws = _workspace(entry, pcm.device, workspace_bytes())
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    N.call(f"oasr_{entry}", C.byref(a), N.STREAM, device=pcm.device)


def _speed_args(pcm, n_valid, factors, seed, first_clip, tokens, ts_begin, ts_max, out, cuda):
    """Checks and converts the operands of ``speed_perturb`` / ``speed_perturb_host``: (SpeedArgs, pcm_out, n_out, factor, keep-alive)."""
    what = "speed_perturb" if cuda else "speed_perturb_host"
    tokens = tuple(tokens)
    if len(tokens) > 2:
        raise ValueError(f"{what}: at most two token tensors, got {len(tokens)}")
    ld_in, B, n = _pcm_in(what, pcm, n_valid, cuda)
    a = N.SpeedArgs()
    a.policy = speed_policy(factors)
    a.seed, a.first_clip = _u64("seed", seed, what), _u64("first_clip", first_clip, what)
    if tokens:
        S = tokens[0].shape[1] if isinstance(tokens[0], torch.Tensor) and tokens[0].dim() == 2 else 0
        lds = [_rows_ld(what, t, f"tokens[{i}]", pcm, cuda, torch.int64, (B, S)) for i, t in enumerate(tokens)]
        if S < 1:
            raise ValueError(f"{what}: tokens must be [B, S] with S >= 1")
        for nm, v, hi in (("ts_begin", ts_begin, 2 ** 31 - 1), ("ts_max", ts_max, 1 << 24)):
            if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v <= hi:
                raise ValueError(f"{what}: {nm} must be an integer in [0, {hi}], got {v!r}")
        a.S, a.ts_begin, a.ts_max = S, ts_begin, ts_max
        a.tokens_a, a.ld_tokens_a = tokens[0].data_ptr(), lds[0]
        if len(tokens) == 2:
            a.tokens_b, a.ld_tokens_b = tokens[1].data_ptr(), lds[1]
    out, ld_out = _pcm_out(what, pcm, ld_in, out, cuda)
    n_out = torch.empty(B, dtype=torch.int32, device=pcm.device)
    factor = torch.empty(B, dtype=torch.int32, device=pcm.device)
    a.pcm_in, a.pcm_out, a.n_valid, a.n_out, a.factor_out = pcm.data_ptr(), out.data_ptr(), n_valid.data_ptr(), n_out.data_ptr(), factor.data_ptr()
    a.ld_in, a.ld_out, a.B, a.N = ld_in, ld_out, B, n
    return a, out, n_out, factor, (pcm, n_valid, tokens)


def speed_perturb(pcm, n_valid, *, factors, seed=0, first_clip=0, tokens=(), ts_begin=50363, ts_max=1500, out=None):
    """Speed perturbation of int16 PCM on the GPU (include/oasr.h: oasr_speed_perturb; the rule: csrc/speed_core.h): ``pcm`` int16 [B, N]
    (unit column stride, any row stride >= N), ``n_valid`` int32 [B] = each row's leading non-padding samples.  Row ``b`` draws one of
    ``factors`` -- (P, Q) pairs, P / Q times faster -- from stream id ``first_clip + b`` (mod 2^64) under ``seed`` (the hash stream of
    ``spec_augment_``, kind 3) and is resampled by the integer polyphase filter of that ratio; (1, 1), a slow-down that would not fit the row,
    and a row whose ``n_valid`` is outside [0, N] are copies of the row.  ``tokens``: up to two int64 [B, S] tensors whose timestamp ids
    ``ts_begin .. ts_begin + ts_max`` are rescaled IN PLACE by the row's ratio.  Returns ``(pcm_out, n_out, factor)``: the new int16 [B, N]
    (``out``, if given: int16 [B, N] that does not overlap ``pcm``), int32 [B] new lengths, int32 [B] the index taken (-1: fell back to the
    copy).  One launch on the current stream, no host read; wrong dtypes, shapes or devices raise ValueError before anything is launched."""
    a, out, n_out, factor, keep = _speed_args(pcm, n_valid, factors, seed, first_clip, tokens, ts_begin, ts_max, out, True)
    _pcm_call("speed_perturb", a, pcm, True)
    return out, n_out, factor


def speed_perturb_host(pcm, n_valid, *, factors, seed=0, first_clip=0, tokens=(), ts_begin=50363, ts_max=1500, out=None):
    """``speed_perturb`` on CPU tensors through the library's host twin (oasr_speed_perturb_host: the same rule from the same text, no GPU).
    Here the lengths are readable, so an ``n_valid`` outside [0, N] raises ValueError."""
    a, out, n_out, factor, keep = _speed_args(pcm, n_valid, factors, seed, first_clip, tokens, ts_begin, ts_max, out, False)
    if a.B and (int(n_valid.min()) < 0 or int(n_valid.max()) > a.N):
        raise ValueError(f"speed_perturb_host: n_valid outside [0, N = {a.N}]")
    _pcm_call("speed_perturb", a, pcm, False)
    return out, n_out, factor


def speed_plan(factors, seed, clip, n_valid, n):
    """What ``speed_perturb`` does to stream id ``clip`` with ``n_valid`` of ``n`` samples, from the library's host function
    (oasr_speed_plan; no GPU): ``(P, Q, n_out, factor)``; factor -1 and P = Q = 1 where a slow-down would not fit the row."""
    pol = speed_policy(factors)
    for nm, v in (("n_valid", n_valid), ("N", n)):
        if not isinstance(v, int) or isinstance(v, bool):
            raise ValueError(f"speed_plan: {nm} must be an integer, got {v!r}")
    if not (1 <= n <= N.SpeedArgs.MAX_N and 0 <= n_valid <= n):
        raise ValueError(f"speed_plan: 1 <= N <= 2^26 and 0 <= n_valid <= N, got N = {n}, n_valid = {n_valid}")
    P, Q, n_out, f = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    N.call("oasr_speed_plan", C.byref(pol), _u64("seed", seed, "speed_plan"), _u64("clip", clip, "speed_plan"), n_valid, n, C.byref(P),
           C.byref(Q), C.byref(n_out), C.byref(f))
    return P.value, Q.value, n_out.value, f.value


def speed_table(P, Q):
    """The library's Q15 tap table of the ratio P / Q (oasr_speed_table; host): ``(T, H)`` with T int32 [Q, 2 H], every row summing to 32768."""
    pol = speed_policy([(P, Q)])
    if P == Q:
        raise ValueError("speed_table: P == Q is the identity (a copy): it has no table")
    H = C.c_int()
    N.call("oasr_speed_table", pol.P[0], pol.Q[0], None, C.byref(H))
    T = torch.empty(Q, 2 * H.value, dtype=torch.int32)
    N.call("oasr_speed_table", P, Q, T, C.byref(H))
    return T, H.value


def noise_policy(prob, snr_db):
    """The ``oasr_noise`` block of a policy, refused here (ValueError) for what the library would refuse (OASR_EINVAL): ``prob`` in [0, 1]
    (kept as round(prob * 65536): the chance of a clip to be drawn), ``snr_db`` = (lo, hi), whole dB with -10 <= lo <= hi <= 50."""
    prob_q16 = _prob_q16("noise_mix", prob)
    try:
        lo, hi = snr_db
    except (TypeError, ValueError):
        raise ValueError(f"noise_mix: snr_db must be a pair (lo, hi) of whole dB, got {snr_db!r}")
    if any(not isinstance(v, int) or isinstance(v, bool) for v in (lo, hi)):
        raise ValueError(f"noise_mix: snr_db must be a pair of integers (whole dB), got {snr_db!r}")
    if not N.Noise.SNR_MIN <= lo <= hi <= N.Noise.SNR_MAX:
        raise ValueError(f"noise_mix: snr_db needs {N.Noise.SNR_MIN} <= lo <= hi <= {N.Noise.SNR_MAX}, got {snr_db!r}")
    return N.Noise(prob_q16, lo, hi)


def _noise_args(pcm, n_valid, bank, prob, snr_db, seed, first_clip, out, cuda):
    """Checks and converts the operands of ``noise_mix`` / ``noise_mix_host``: (NoiseArgs, pcm_out, row, snr, gain, keep-alive)."""
    what = "noise_mix" if cuda else "noise_mix_host"
    ld_in, B, n = _pcm_in(what, pcm, n_valid, cuda)
    ld_bank = _rows_ld(what, bank, "bank", pcm, cuda)
    M, L = bank.shape
    if not (1 <= L <= N.NoiseArgs.MAX_N and 1 <= M <= N.NoiseArgs.MAX_ROWS):
        raise ValueError(f"{what}: bank [M, L] with 1 <= M <= 65535 and 1 <= L <= 2^26, got {tuple(bank.shape)}")
    a = N.NoiseArgs()
    a.policy = noise_policy(prob, snr_db)
    a.seed, a.first_clip = _u64("seed", seed, what), _u64("first_clip", first_clip, what)
    out, ld_out = _pcm_out(what, pcm, ld_in, out, cuda, in_place=True, bank=bank, ld_bank=ld_bank)
    row = torch.empty(B, dtype=torch.int32, device=pcm.device)
    snr = torch.empty(B, dtype=torch.int32, device=pcm.device)
    gain = torch.empty(B, dtype=torch.int64, device=pcm.device)
    a.pcm_in, a.pcm_out, a.n_valid, a.bank = pcm.data_ptr(), out.data_ptr(), n_valid.data_ptr(), bank.data_ptr()
    a.row_out, a.snr_out, a.gain_out = row.data_ptr(), snr.data_ptr(), gain.data_ptr()
    a.ld_in, a.ld_out, a.ld_bank, a.B, a.N, a.M, a.L = ld_in, ld_out, ld_bank, B, n, M, L
    return a, out, row, snr, gain, (pcm, n_valid, bank)


def noise_mix(pcm, n_valid, bank, *, prob, snr_db, seed=0, first_clip=0, out=None):
    """Additive noise at a drawn SNR on int16 PCM on the GPU (include/oasr.h: oasr_noise_mix; the rule: csrc/noise_core.h): ``pcm`` int16
    [B, N] (unit column stride, any row stride >= N), ``n_valid`` int32 [B] = each row's leading non-padding samples, ``bank`` int16 [M, L]
    of noise recordings, every row fully valid (``augment.noise_bank`` tiles shorter ones).  Row ``b`` draws -- from stream id
    ``first_clip + b`` (mod 2^64) under ``seed``, the hash stream of ``spec_augment_``, kind 4 -- whether it takes noise (``prob``), a bank
    row, an offset into it (the row is read cyclically) and an SNR among the whole dB of ``snr_db`` = (lo, hi); the noise is scaled by an
    integer Q16 gain from the two exact energies over the row's first ``n_valid`` samples and added with saturation.  A row that is not
    drawn, has ``n_valid`` outside [1, N], or is silent (as is a silent stretch of noise) is copied.  Returns ``(pcm_out, row, snr, gain)``:
    int16 [B, N] (``out``, if given: int16 [B, N] that is ``pcm`` itself -- in place -- or does not overlap it), int32 [B] bank rows (-1: not
    mixed), int32 [B] SNRs (-128: not mixed), int64 [B] gains (0: not mixed).  Two launches on the current stream, no host read; wrong
    dtypes, shapes or devices raise ValueError before anything is launched."""
    a, out, row, snr, gain, keep = _noise_args(pcm, n_valid, bank, prob, snr_db, seed, first_clip, out, True)
    _pcm_call("noise_mix", a, pcm, True, lambda: N.lib().oasr_noise_workspace_bytes(a.B, a.N))
    return out, row, snr, gain


def noise_mix_host(pcm, n_valid, bank, *, prob, snr_db, seed=0, first_clip=0, out=None):
    """``noise_mix`` on CPU tensors through the library's host twin (oasr_noise_mix_host: the same rule from the same text, no GPU)."""
    a, out, row, snr, gain, keep = _noise_args(pcm, n_valid, bank, prob, snr_db, seed, first_clip, out, False)
    _pcm_call("noise_mix", a, pcm, False)
    return out, row, snr, gain


def noise_plan(prob, snr_db, seed, clip, M, L):
    """What ``noise_mix`` draws for stream id ``clip`` against a bank of ``M`` rows of ``L`` samples, from the library's host function
    (oasr_noise_plan; no GPU, no audio): ``(drawn, row, offset, snr_db)``."""
    pol = noise_policy(prob, snr_db)
    for nm, v, hi in (("M", M, N.NoiseArgs.MAX_ROWS), ("L", L, N.NoiseArgs.MAX_N)):
        if not isinstance(v, int) or isinstance(v, bool) or not 1 <= v <= hi:
            raise ValueError(f"noise_plan: {nm} must be an integer in [1, {hi}], got {v!r}")
    d, m, o, s = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    N.call("oasr_noise_plan", C.byref(pol), _u64("seed", seed, "noise_plan"), _u64("clip", clip, "noise_plan"), M, L, C.byref(d), C.byref(m),
           C.byref(o), C.byref(s))
    return bool(d.value), m.value, o.value, s.value


def reverb_policy(prob):
    """The ``oasr_reverb`` block of a policy, refused here (ValueError) for what the library would refuse (OASR_EINVAL): ``prob`` in [0, 1]
    (kept as round(prob * 65536): the chance of a clip to be drawn)."""
    return N.Reverb(_prob_q16("reverb", prob))


def _reverb_args(pcm, n_valid, bank, delay, prob, seed, first_clip, out, cuda):
    """Checks and converts the operands of ``reverb`` / ``reverb_host``: (ReverbArgs, pcm_out, row, keep-alive)."""
    what = "reverb" if cuda else "reverb_host"
    ld_in, B, n = _pcm_in(what, pcm, n_valid, cuda)
    ld_rir = _rows_ld(what, bank, "bank", pcm, cuda)
    R, K = bank.shape
    _i32_vec(what, delay, "delay", R, pcm)
    if not (1 <= K <= N.ReverbArgs.MAX_K and 1 <= R <= N.ReverbArgs.MAX_ROWS):
        raise ValueError(f"{what}: bank [R, K] with 1 <= R <= 65535 and 1 <= K <= 8192, got {tuple(bank.shape)}")
    a = N.ReverbArgs()
    a.policy = reverb_policy(prob)
    a.seed, a.first_clip = _u64("seed", seed, what), _u64("first_clip", first_clip, what)
    out, ld_out = _pcm_out(what, pcm, ld_in, out, cuda, bank=bank, ld_bank=ld_rir)
    row = torch.empty(B, dtype=torch.int32, device=pcm.device)
    a.pcm_in, a.pcm_out, a.n_valid, a.rir, a.delay, a.row_out = (pcm.data_ptr(), out.data_ptr(), n_valid.data_ptr(), bank.data_ptr(),
                                                                 delay.data_ptr(), row.data_ptr())
    a.ld_in, a.ld_out, a.ld_rir, a.B, a.N, a.R, a.K = ld_in, ld_out, ld_rir, B, n, R, K
    return a, out, row, (pcm, n_valid, bank, delay)


def reverb(pcm, n_valid, bank, delay, *, prob, seed=0, first_clip=0, out=None):
    """Reverberation of int16 PCM on the GPU (include/oasr.h: oasr_reverb; the rule: csrc/reverb_core.h): ``pcm`` int16 [B, N] (unit column
    stride, any row stride >= N), ``n_valid`` int32 [B] = each row's leading non-padding samples, ``bank`` int16 [R, K] of Q15 impulse
    responses with K <= 8192 and ``delay`` int32 [R] the index of each one's direct-path tap (``augment.rir_bank`` builds both).  Row ``b``
    draws -- from stream id ``first_clip + b`` (mod 2^64) under ``seed``, the hash stream of ``spec_augment_``, kind 5 -- whether it is
    reverberated (``prob``) and a bank row; its first ``n_valid`` samples become the exact convolution with that row, shifted back by the
    direct-path delay, rounded to Q0 and saturated, so that lengths and timestamps stay.  Taps are read clamped to +-32639 and delays to
    [0, K - 1].  A row that is not drawn or has ``n_valid`` outside [1, N] is copied.  Returns ``(pcm_out, row)``: int16 [B, N] (``out``, if
    given: int16 [B, N] that does not overlap ``pcm``) and int32 [B] bank rows (-1: copied).  Two launches on the current stream (the bank
    expanded into int8 matrix-core operands, then the convolution), no host read; wrong dtypes, shapes or devices raise ValueError before
    anything is launched."""
    a, out, row, keep = _reverb_args(pcm, n_valid, bank, delay, prob, seed, first_clip, out, True)
    _pcm_call("reverb", a, pcm, True, lambda: N.lib().oasr_reverb_workspace_bytes(a.R, a.K))
    return out, row


def reverb_host(pcm, n_valid, bank, delay, *, prob, seed=0, first_clip=0, out=None):
    """``reverb`` on CPU tensors through the library's host twin (oasr_reverb_host: the same rule from the same text, no GPU)."""
    a, out, row, keep = _reverb_args(pcm, n_valid, bank, delay, prob, seed, first_clip, out, False)
    _pcm_call("reverb", a, pcm, False)
    return out, row


def reverb_plan(prob, seed, clip, R):
    """What ``reverb`` draws for stream id ``clip`` against a bank of ``R`` responses, from the library's host function (oasr_reverb_plan; no
    GPU, no audio): ``(drawn, row)``."""
    pol = reverb_policy(prob)
    if not isinstance(R, int) or isinstance(R, bool) or not 1 <= R <= N.ReverbArgs.MAX_ROWS:
        raise ValueError(f"reverb_plan: R must be an integer in [1, {N.ReverbArgs.MAX_ROWS}], got {R!r}")
    d, r = C.c_int(), C.c_int()
    N.call("oasr_reverb_plan", C.byref(pol), _u64("seed", seed, "reverb_plan"), _u64("clip", clip, "reverb_plan"), R, C.byref(d), C.byref(r))
    return bool(d.value), r.value


TELEPHONE_CODECS = {"linear": N.Telephone.LINEAR, "mulaw": N.Telephone.MULAW, "alaw": N.Telephone.ALAW}


def _telephone_codec(who, c):
    """A codec by name ("linear", "mulaw", "alaw") or by the library's number (0, 1, 2), as the number."""
    if isinstance(c, str) and c in TELEPHONE_CODECS:
        return TELEPHONE_CODECS[c]
    if isinstance(c, int) and not isinstance(c, bool) and c in TELEPHONE_CODECS.values():
        return c
    raise ValueError(f"{who}: a codec must be one of {sorted(TELEPHONE_CODECS)} (or 0, 1, 2), got {c!r}")


def telephone_policy(prob, codecs, bandpass=True):
    """The ``struct oasr_telephone`` block of a policy, refused here (ValueError) for what the library would refuse (OASR_EINVAL): ``prob``
    in [0, 1] (kept as round(prob * 65536): the chance of a clip to be drawn), ``codecs`` 1 .. 8 of "linear" | "mulaw" | "alaw" (or 0 | 1 |
    2; repeats act as weights), ``bandpass`` a bool."""
    prob_q16 = _prob_q16("telephone", prob)
    if isinstance(codecs, (str, bytes)) or not hasattr(codecs, "__iter__"):
        raise ValueError(f"telephone: codecs must be a sequence of codec names, got {codecs!r}")
    ids = [_telephone_codec("telephone", c) for c in codecs]
    if not 1 <= len(ids) <= N.Telephone.MAX_CODECS:
        raise ValueError(f"telephone: between 1 and {N.Telephone.MAX_CODECS} codecs, got {len(ids)}")
    if not isinstance(bandpass, bool):
        raise ValueError(f"telephone: bandpass must be a bool, got {bandpass!r}")
    pol = N.Telephone()
    pol.prob_q16, pol.n_codecs, pol.bandpass = prob_q16, len(ids), int(bandpass)
    for i, c in enumerate(ids):
        pol.codecs[i] = c
    return pol


def _telephone_args(pcm, n_valid, prob, codecs, bandpass, seed, first_clip, out, cuda):
    """Checks and converts the operands of ``telephone`` / ``telephone_host``: (TelephoneArgs, pcm_out, codec, keep-alive)."""
    what = "telephone" if cuda else "telephone_host"
    ld_in, B, n = _pcm_in(what, pcm, n_valid, cuda)
    a = N.TelephoneArgs()
    a.policy = telephone_policy(prob, codecs, bandpass)
    a.seed, a.first_clip = _u64("seed", seed, what), _u64("first_clip", first_clip, what)
    out, ld_out = _pcm_out(what, pcm, ld_in, out, cuda)
    codec = torch.empty(B, dtype=torch.int32, device=pcm.device)
    a.pcm_in, a.pcm_out, a.n_valid, a.codec_out = pcm.data_ptr(), out.data_ptr(), n_valid.data_ptr(), codec.data_ptr()
    a.ld_in, a.ld_out, a.B, a.N = ld_in, ld_out, B, n
    return a, out, codec, (pcm, n_valid)


def telephone(pcm, n_valid, *, prob, codecs=("mulaw", "alaw", "linear"), bandpass=True, seed=0, first_clip=0, out=None):
    """The telephone channel on int16 PCM at 16 kHz on the GPU (include/oasr.h: oasr_telephone; the rule: csrc/telephone_core.h): ``pcm``
    int16 [B, N] (unit column stride, any row stride >= N), ``n_valid`` int32 [B] = each row's leading non-padding samples.  Row ``b`` draws
    -- from stream id ``first_clip + b`` (mod 2^64) under ``seed``, the hash stream of ``spec_augment_``, kind 6 -- whether it goes through
    the channel (``prob``) and one of ``codecs``; its first ``n_valid`` samples are band-passed to 300 - 3400 Hz at 8 kHz by a 129-tap
    integer filter (``bandpass=False``: every second sample is taken as it is), companded by the G.711 quantiser drawn ("mulaw", "alaw", or
    "linear": none), and interpolated back to 16 kHz by a 32-tap integer filter; both filters are zero-phase, so lengths and timestamps
    stay.  A row that is not drawn or has ``n_valid`` outside [1, N] is copied.  Returns ``(pcm_out, codec)``: int16 [B, N] (``out``, if
    given: int16 [B, N] that does not overlap ``pcm``) and int32 [B] codecs (0 linear, 1 mu-law, 2 A-law; -1: copied).  One launch on the
    current stream, no host read; wrong dtypes, shapes or devices raise ValueError before anything is launched."""
    a, out, codec, keep = _telephone_args(pcm, n_valid, prob, codecs, bandpass, seed, first_clip, out, True)
    _pcm_call("telephone", a, pcm, True)
    return out, codec


def telephone_host(pcm, n_valid, *, prob, codecs=("mulaw", "alaw", "linear"), bandpass=True, seed=0, first_clip=0, out=None):
    """``telephone`` on CPU tensors through the library's host twin (oasr_telephone_host: the same rule from the same text, no GPU)."""
    a, out, codec, keep = _telephone_args(pcm, n_valid, prob, codecs, bandpass, seed, first_clip, out, False)
    _pcm_call("telephone", a, pcm, False)
    return out, codec


def telephone_plan(prob, codecs, seed, clip, bandpass=True):
    """What ``telephone`` draws for stream id ``clip``, from the library's host function (oasr_telephone_plan; no GPU, no audio):
    ``(drawn, codec)`` -- the codec is the one the clip would take, drawn or not."""
    pol = telephone_policy(prob, codecs, bandpass)
    d, c = C.c_int(), C.c_int()
    N.call("oasr_telephone_plan", C.byref(pol), _u64("seed", seed, "telephone_plan"), _u64("clip", clip, "telephone_plan"), C.byref(d), C.byref(c))
    return bool(d.value), c.value


def telephone_tables():
    """The library's Q15 tap tables (oasr_telephone_tables; host): ``(h, u)`` -- the band-pass int32 [129] as h[k + 64], k = -64 .. 64, and
    the interpolator's odd phase int32 [32], which sums to 32768."""
    h, u = torch.empty(N.Telephone.BP_TAPS, dtype=torch.int32), torch.empty(N.Telephone.UP_TAPS, dtype=torch.int32)
    N.call("oasr_telephone_tables", h, u)
    return h, u


def telephone_quantize_host(x, codec):
    """The G.711 quantiser ``codec`` ("linear" | "mulaw" | "alaw") as expand(compress(x)) on a contiguous int16 CPU tensor of any shape,
    through the library's host function (oasr_telephone_quantize_host): a new tensor."""
    c = _telephone_codec("telephone_quantize_host", codec)
    if not (isinstance(x, torch.Tensor) and x.dtype == torch.int16 and not x.is_cuda and x.is_contiguous()):
        raise ValueError("telephone_quantize_host: x must be a contiguous int16 CPU tensor")
    out = torch.empty_like(x)
    if x.numel():
        N.call("oasr_telephone_quantize_host", x, out, x.numel(), c)
    return out


def pick_tokens(logits, mask=None, mask2=None, want_logprob=True):
    """logits fp32 [rows, V] (row stride free) -> (argmax ids int64 [rows], log_softmax at the argmax fp32 [rows] | None);
    ``mask`` / ``mask2``: additive fp32 [V] (0 / -inf)."""
    N.require_gpu(logits, "logits")
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    rows, V = logits.shape
    tok = torch.empty(rows, device=logits.device, dtype=torch.int64)
    lp = torch.empty(rows, device=logits.device, dtype=torch.float32) if want_logprob else None
    for m in (mask, mask2):
        assert m is None or (m.dtype == torch.float32 and m.numel() == V and m.is_contiguous())
    N.call("oasr_pick_tokens", logits, logits.stride(0), V, rows, mask, mask2, tok, lp, N.STREAM)
    return tok, lp


def _ts_args(logits, history, n_history, ids, mask, mask2, k=None):
    """What the three rule-aware selections share: the checks, the native arguments from ``logits`` to ``max_initial_index`` (``ids``:
    timestamp_begin, eot, no_timestamps, max_initial_index; ``n_history`` None: no timestamp rules) and the two outputs, ids int64 and
    log-probabilities f32 of shape [rows] or [rows, k]."""
    N.require_gpu(logits, "logits")
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    rows, V = logits.shape
    if n_history is not None and n_history > 0:
        assert (history.dtype == torch.int64 and history.dim() == 2 and history.shape[0] == rows and history.stride(1) == 1
                and history.shape[1] >= n_history and history.device == logits.device)
    for m in (mask, mask2):
        assert m is None or (m.dtype == torch.float32 and m.numel() == V and m.is_contiguous())
    nh = -1 if n_history is None else int(n_history)
    shape = (rows,) if k is None else (rows, k)
    tok = torch.empty(shape, device=logits.device, dtype=torch.int64)
    lp = torch.empty(shape, device=logits.device, dtype=torch.float32)
    return (logits, logits.stride(0), V, rows, mask, mask2, (history if nh > 0 else None), (history.stride(0) if nh > 0 else 0), nh,
            int(ids[0]), int(ids[1]), int(ids[2]), -1 if ids[3] is None else int(ids[3])), tok, lp


def pick_tokens_ts(logits, history, n_history, *, timestamp_begin, eot, no_timestamps, max_initial_index=None, mask=None, mask2=None):
    """``pick_tokens`` with whisper's ApplyTimestampRules evaluated on the device: ``history`` int64 [rows, >= n_history] holds the
    tokens sampled so far (after the sot sequence).  Returns (ids int64 [rows], log_softmax of the pick over the surviving columns)."""
    args, tok, lp = _ts_args(logits, history, int(n_history), (timestamp_begin, eot, no_timestamps, max_initial_index), mask, mask2)
    N.call("oasr_pick_tokens_ts", *args, tok, lp, N.STREAM)
    return tok, lp


def topk_tokens(logits, k, *, history=None, n_history=None, timestamp_begin=50363, eot=50256, no_timestamps=50362, max_initial_index=None,
                mask=None, mask2=None):
    """The k best (log_softmax value, token) pairs per row of the filtered distribution (suppress masks; ``n_history`` not None: whisper's
    ApplyTimestampRules from ``history``, as ``pick_tokens_ts``) -- BeamSearchDecoder.update's ``logprobs.topk(beam_size + 1)`` in one
    kernel.  Returns (logprob f32 [rows, k] descending, ids int64 [rows, k])."""
    args, tok, lp = _ts_args(logits, history, n_history, (timestamp_begin, eot, no_timestamps, max_initial_index), mask, mask2, k)
    N.call("oasr_topk_tokens", *args, int(k), tok, lp, N.STREAM)
    return lp, tok


def sample_tokens(logits, temperature, uniforms, *, history=None, n_history=None, timestamp_begin=50363, eot=50256, no_timestamps=50362,
                  max_initial_index=None, mask=None, mask2=None):
    """One draw per row from softmax(filtered logits / temperature) by inverse CDF on ``uniforms`` (f32 [rows] in [0, 1)); returns
    (ids int64 [rows], log_softmax of the draw at temperature 1) -- GreedyDecoder.update at temperature > 0."""
    args, tok, lp = _ts_args(logits, history, n_history, (timestamp_begin, eot, no_timestamps, max_initial_index), mask, mask2)
    assert uniforms.dtype == torch.float32 and uniforms.numel() == logits.shape[0] and uniforms.device == logits.device
    N.call("oasr_sample_tokens", *args, float(temperature), uniforms, tok, lp, N.STREAM)
    return tok, lp


# ---- unit operators of the glue kernels (include/oasr_testing.h: oasr_test_*; used by tests/test_gpu_glue_ops.py) -----------------------
# Every wrapper takes the caller's own (possibly guard-banded, pre-filled) output tensors and passes base addresses through: nothing is
# allocated or zeroed here, so a test sees exactly what the kernel wrote.  The activation dtype (bf16 / fp32) selects the kernel.
def _dt(t):
    assert t.dtype in (BF, torch.float32), t.dtype
    return 0 if t.dtype == BF else 1


def embedding_fwd_(tok, E, pos, x, n_embed, rows=None):
    """x[row(b, s)] = E[tok[b, s]] + pos[s]; tok int64 [B, S]; x: the output allocation (bf16 or fp32), rows: chunk-row table or None."""
    B, S = tok.shape
    N.call("oasr_test_embedding_fwd", tok, E, pos, x, _dt(x), B, S, E.shape[1], int(n_embed), rows, N.STREAM)


def embedding_bwd_(tok, dx, dE, dpos, pad_id, n_embed, d, rows=None, span=None):
    """dE[tok] += dx, dpos[s] += sum_b dx (either may be None); dx: activation rows [*, d]."""
    B, S = tok.shape
    N.call("oasr_test_embedding_bwd", tok, dx, _dt(dx), dE, dpos, B, S, d, int(pad_id), int(n_embed), rows, span, N.STREAM)


def colsum_(x, ld, M, ncols, out):
    N.call("oasr_test_colsum", x, _dt(x), ld, M, ncols, out, N.STREAM)


def conv2_col2im_dgelu_(dA, u1, dpre1, B, T1, d):
    assert dA.dtype == u1.dtype == dpre1.dtype
    N.call("oasr_test_conv2_col2im_dgelu", dA, u1, dpre1, _dt(dA), B, T1, d, N.STREAM)


def conv1_col2im_mel_(dcol, dmel, B, T1, n_mels):
    N.call("oasr_test_conv1_col2im_mel", dcol, _dt(dcol), dmel, B, T1, n_mels, N.STREAM)


def mel_to_time_major_(mel, out, B, n_mels, T, clip_max=None):
    N.call("oasr_test_mel_to_time_major", mel, out, _dt(out), B, n_mels, T, clip_max, N.STREAM)


def pack_conv_weight_(w, dst, co, ci, ldk):
    N.call("oasr_test_pack_conv_weight", w, dst, _dt(dst), co, ci, ldk, N.STREAM)


def unpack_conv_grad_(g, dw, co, ci, ldk):
    N.call("oasr_test_unpack_conv_grad", g, dw, co, ci, ldk, N.STREAM)


def pack_embedding_(e, dst, rows, rows_pad, d):
    N.call("oasr_test_pack_embedding", e, dst, rows, rows_pad, d, N.STREAM)


def dgelu_mul_(dy, u, out, n):
    assert dy.dtype == u.dtype == out.dtype
    N.call("oasr_test_dgelu_mul", dy, u, out, _dt(dy), n, N.STREAM)


def dlogits_from_f32_(src, V, rows, ld, dst):
    N.call("oasr_test_dlogits_from_f32", src, V, rows, ld, dst, _dt(dst), N.STREAM)


def logits_to_f32_(logits, ld, rows, V, out):
    N.call("oasr_test_logits_to_f32", logits, _dt(logits), ld, rows, V, out, N.STREAM)


def layernorm_bwd_(dy, x, gamma, mean, rstd, dres, dx, dgamma, dbeta, dsum):
    """launch_layernorm_bwd as the engine calls it: dx written, dgamma / dbeta / dsum (each may be None) ACCUMULATED into the caller's tensors."""
    rows, d = x.shape
    N.call("oasr_test_layernorm_bwd", dy, x, gamma, mean, rstd, dres, dx, dgamma, dbeta, dsum, _dt(x), rows, d, N.STREAM)


def argmax_rows_(logits, V, rows, span, pred_out):
    """include/oasr_testing.h: oasr_test_argmax_rows -- the prediction kernel of ``loss_and_backward(pred_out=...)`` on a caller's matrix:
    ``logits`` bf16 / fp32 [n_rows, ld], ``rows`` int32 [B, 16] chunk-row table, ``span`` int32 [B] (multiples of 64), ``pred_out`` int32 [B, S]."""
    B, S = pred_out.shape
    N.call("oasr_test_argmax_rows", logits, _dt(logits), logits.stride(0), V, logits.shape[0], rows, span, B, S, pred_out, N.STREAM)
    return pred_out


def cross_entropy_test_(logits, V, targets, ignore, gscale=1.0, write_grad=True, label_smoothing=0.0, z_loss=0.0):
    """include/oasr_testing.h: oasr_test_cross_entropy -- ``cross_entropy_`` on bf16 (the production kernel) or fp32 (the fp32 engine's kernel)
    logits [rows, ld], in place.  Returns (loss f32 [1], row_loss f32 [rows], n_valid int32 [1])."""
    rows = logits.shape[0]
    nv = torch.zeros(1, device=logits.device, dtype=torch.int32)
    row_loss = torch.empty(rows, device=logits.device, dtype=torch.float32)
    loss = torch.zeros(1, device=logits.device, dtype=torch.float32)
    N.call("oasr_test_cross_entropy", logits, _dt(logits), logits.stride(0), V, targets, rows, ignore, gscale, nv, row_loss, loss,
           int(write_grad), float(label_smoothing), float(z_loss), None, N.STREAM)
    return loss, row_loss, nv
