"""Checksums of the attention kernels' outputs on fixed seeded problems, to compare two builds of the library bit for bit (OASR_LIB
selects the build).  Forward (o, lse, o_lo): encoder, cross, causal + key lengths, ragged sizes.  Backward (dq, dk, dv; the wrappers do
not return delta) on small problems that reach every backward kernel: the ping-pong pair with a partial 256-row block and a partial
tile, the general pair through the testing switch, the key-length mask, and the chunked-row (row-table) forms with spans, block tables
and tile flags.  The fused bias gradients are reduced with fp32 atomics, whose order is not fixed: they are printed as a 4-digit norm,
not as a checksum."""
import os
import sys
import zlib

import torch

os.environ.setdefault("OASR_TESTING_HOOKS", "1")  # oasr_attention_set_pingpong
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from olmoasr_amd import _native as N  # noqa: E402
from olmoasr_amd import ops  # noqa: E402

BF = torch.bfloat16
DEV = "cuda"


def crc(t):
    return zlib.crc32(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())


def forward_cases(g):
    for name, B, H, Tq, Tk, causal in (("encoder", 4, 16, 1500, 1500, False), ("cross", 4, 16, 448, 1500, False), ("causal", 6, 16, 448, 448, True),
                                       ("ragged", 3, 5, 200, 333, False), ("short", 2, 3, 70, 1, False), ("causal-ragged", 3, 4, 130, 130, True)):
        q = torch.randn(B, Tq, H, 64, device=DEV, generator=g).to(BF)
        k = torch.randn(B, Tk, H, 64, device=DEV, generator=g).to(BF)
        v = torch.randn(B, Tk, H, 64, device=DEV, generator=g).to(BF)
        kv_len = torch.randint(1, Tk + 1, (B,), device=DEV, generator=g, dtype=torch.int32) if causal else None
        o, lse, o_lo = ops.attention_fwd(q, k, v, kv_len, causal, want_o_lo=True)
        print(f"fwd {name:14s} o {crc(o):08x} lse {crc(lse):08x} o_lo {crc(o_lo):08x}", flush=True)


def show_bwd(name, grads, colsums=None):
    line = f"bwd {name:30s} " + " ".join(f"{n} {crc(t):08x}" for n, t in zip(("dq", "dk", "dv"), grads))
    if colsums:
        line += " " + " ".join(f"{n}_colsum_l1 {float(c.abs().sum()):.4e}" for n, c in zip(("dq", "dv"), colsums))
    print(line, flush=True)


def plain_problem(g, B, H, Tq, Tk, causal):
    q, k, v = (torch.randn(B, T, H, 64, device=DEV, generator=g).to(BF) for T in (Tq, Tk, Tk))
    d_o = (0.5 * torch.randn(B, Tq, H * 64, device=DEV, generator=g)).to(BF)
    kv_len = torch.randint(1, Tk + 1, (B,), device=DEV, generator=g, dtype=torch.int32) if causal else None
    o, lse, o_lo = ops.attention_fwd(q, k, v, kv_len, causal, want_o_lo=True)
    return q, k, v, o, lse, o_lo, d_o, kv_len


def placement(B, n_chunks, seed):
    gc = torch.Generator().manual_seed(seed)
    pairs = [(b, c) for b in range(B) for c in range(n_chunks)]
    return ops.chunk_rows_table([pairs[i] for i in torch.randperm(len(pairs), generator=gc).tolist()], B, n_chunks)


def backward_cases(g):
    lib = N.lib()
    # unmasked: both ping-pong kernels (Tq = Tk = 320: a partial 256-row block, a partial 64-row tile); then the general kernels
    B, H, T = 2, 2, 320
    p = plain_problem(g, B, H, T, T, False)
    q, k, v, o, lse, o_lo, d_o, _ = p
    for pp in (1, 0):
        assert lib.oasr_attention_set_pingpong(pp) == 0
        tag = "pingpong" if pp else "general"
        show_bwd(f"unmasked {tag}", ops.attention_bwd(q, k, v, o, lse, d_o, None, False, o_lo=o_lo))
        cs = [torch.zeros(H * 64, device=DEV) for _ in range(2)]
        show_bwd(f"unmasked {tag} bias-grads", ops.attention_bwd(q, k, v, o, lse, d_o, None, False, o_lo=o_lo, dq_colsum=cs[0], dv_colsum=cs[1]), cs)
    assert lib.oasr_attention_set_pingpong(1) == 0
    # causal + key lengths: the general kernels with their masks
    q, k, v, o, lse, o_lo, d_o, kv_len = plain_problem(g, 3, 4, 130, 130, True)
    show_bwd("causal kv_len", ops.attention_bwd(q, k, v, o, lse, d_o, kv_len, True, o_lo=o_lo))

    # chunked rows, cross form: Tq = 128, Tk = 200, spans (64, 128), without and with the block tables; ping-pong and general
    B, H, Tq, Tk = 2, 2, 128, 200
    d = H * 64
    tab = placement(B, Tq // 64, 3)
    tab_d = tab.to(DEV)
    qb = torch.randn(B, Tq, d, device=DEV, generator=g).to(BF)
    kvb = torch.randn(B, Tk, 2 * d, device=DEV, generator=g).to(BF)
    kx, vx = (kvb[:, :, i * d:(i + 1) * d].unflatten(2, (H, 64)) for i in range(2))
    qc = ops.to_chunked(qb, tab).unflatten(1, (H, 64))
    span = torch.tensor([64, 128], dtype=torch.int32)
    keep = (torch.arange(Tq)[None, :, None] < span[:, None, None]).to(DEV)
    d_o = (0.5 * torch.randn(B, Tq, d, device=DEV, generator=g)).to(BF)
    doc = ops.to_chunked(torch.where(keep, d_o, torch.zeros_like(d_o)), tab)
    oc, lse, o_lo_c = ops.attention_fwd_rows(qc, kx, vx, B, H, Tq, Tk, tab_d, None, None, False, want_o_lo=True)
    print(f"fwd {'rows cross':14s} o {crc(oc):08x} lse {crc(lse):08x} o_lo {crc(o_lo_c):08x}", flush=True)
    blocks = ops.span_block_tables(span, B, Tq, H)
    for pp in (1, 0):
        assert lib.oasr_attention_set_pingpong(pp) == 0
        for qblk in (None, blocks):
            cs = [torch.zeros(d, device=DEV) for _ in range(2)]
            grads = ops.attention_bwd_rows(qc, kx, vx, oc, lse, doc, B, H, Tq, Tk, tab_d, None, span.to(DEV), None, False, o_lo=o_lo_c,
                                           dq_colsum=cs[0], dv_colsum=cs[1], fill=0.0, q_blocks=qblk, scratch_fill=float("nan"))
            show_bwd(f"rows cross {'pingpong' if pp else 'general'}{' blocks' if qblk else ''}", grads, cs)
    assert lib.oasr_attention_set_pingpong(1) == 0

    # chunked rows, self form: k_rows, causal, T = 128, spans (64, 0), tile flags
    B, H, T = 2, 2, 128
    d = H * 64
    tab = placement(B, T // 64, 4)
    tab_d = tab.to(DEV)
    qkv = torch.randn(B, T, 3 * d, device=DEV, generator=g).to(BF)
    qkv_c = ops.to_chunked(qkv, tab)
    qc, kc, vc = (qkv_c[:, i * d:(i + 1) * d].unflatten(1, (H, 64)) for i in range(3))
    span = torch.tensor([64, 0], dtype=torch.int32)
    keep = (torch.arange(T)[None, :, None] < span[:, None, None]).to(DEV)
    d_o = (0.5 * torch.randn(B, T, d, device=DEV, generator=g)).to(BF)
    doc = ops.to_chunked(torch.where(keep, d_o, torch.zeros_like(d_o)), tab)
    kv_len = torch.tensor([100, 128], dtype=torch.int32, device=DEV)
    oc, lse, o_lo_c = ops.attention_fwd_rows(qc, kc, vc, B, H, T, T, tab_d, tab_d, kv_len, True, want_o_lo=True)
    print(f"fwd {'rows self':14s} o {crc(oc):08x} lse {crc(lse):08x} o_lo {crc(o_lo_c):08x}", flush=True)
    for qblk in (None, ops.span_block_tables(span, B, T, H)):
        flags = torch.full((B, H, T // 64), -1, dtype=torch.int32, device=DEV)
        cs = [torch.zeros(d, device=DEV) for _ in range(2)]
        grads = ops.attention_bwd_rows(qc, kc, vc, oc, lse, doc, B, H, T, T, tab_d, tab_d, span.to(DEV), kv_len, True, o_lo=o_lo_c,
                                       dq_colsum=cs[0], dv_colsum=cs[1], fill=0.0, q_blocks=qblk, scratch_fill=float("nan"), qtile_flags=flags)
        show_bwd(f"rows self flags{' blocks' if qblk else ''}", grads, cs)


def main():
    g = torch.Generator(device=DEV).manual_seed(1)
    forward_cases(g)
    backward_cases(g)


if __name__ == "__main__":
    main()
