"""The decoder attentions of the span-forward training step, standalone at the bench's launch shape (B = 128, H = 16, Tq = 448, Tk = 448 self /
1500 cross; spans of the synthetic samples 0..127; chunk rows and block tables from the device kernel the step uses), timed with HIP events:

  (a) full grid, real spans      -- one workgroup per query block of the padded context, those past the span exit at once
  (b) full grid, every span 448  -- the same launch with every workgroup computing
  (c) compact grid, real spans   -- one workgroup per query block inside the spans (oasr_attn_args.qblk128 / qblk256)

If (a) is not clearly above active / all x (b), the empty workgroups cost nothing and (c) cannot help that launch.
Run under `rocprofv3 --kernel-trace --stats` for the per-kernel split of the backward pairs."""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from olmoasr_amd import _native as N  # noqa: E402
from olmoasr_amd import ops  # noqa: E402
from olmoasr_amd.synth import supervised_span_host, synth_sample  # noqa: E402

BF = torch.bfloat16
DEV = "cuda"


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(5):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(iters):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        best.append(ev[0].elapsed_time(ev[1]) / iters * 1e3)
    return min(best), sorted(best)[len(best) // 2]


def main():
    N.enable_testing_hooks()
    lib = N.lib()
    B, H, S, Te = int(os.environ.get("PB", 128)), 16, 448, 1500
    d = H * 64
    items = [synth_sample(i) for i in range(B)]
    real = supervised_span_host(torch.stack([it[2] for it in items]), torch.tensor([it[3] for it in items], dtype=torch.int32))
    kv_real = torch.tensor([it[3] for it in items], dtype=torch.int32)
    g = torch.Generator().manual_seed(0)
    qkv = (torch.randn(B * S, 3 * d, generator=g)).to(BF).to(DEV)
    qx = (torch.randn(B * S, d, generator=g)).to(BF).to(DEV)
    kvx = (torch.randn(B, Te, 2 * d, generator=g)).to(BF).to(DEV)
    doc = (torch.randn(B * S, d, generator=g) * 0.5).to(BF).to(DEV)
    csq, csv = torch.zeros(d, device=DEV), torch.zeros(d, device=DEV)
    scratch = torch.empty(B * (4 + 12) * d, device=DEV)
    stream = N.stream_ptr()
    print(f"B={B} H={H} Tq={S}; spans of samples 0..{B - 1}: mean {float(real.float().mean()):.1f}, rounded to 64: "
          f"{float(((real + 63) // 64 * 64).float().mean()):.1f}", flush=True)
    results = {}
    for case, span, grid in (("a", real, 0), ("b", torch.full((B,), S, dtype=torch.int32), 0), ("c", real, 1)):
        blocks, rows, span_d = ops.span_block_tables(span, B, S, H, with_rows=True)
        kv_len = (kv_real if case != "b" else torch.full((B,), S, dtype=torch.int32)).to(DEV)
        n128, n256 = blocks[2], blocks[3]
        N.check(lib.oasr_attention_set_span_grid(grid), "hook")
        for kind in ("self", "cross"):
            causal = kind == "self"
            Tk = S if causal else Te
            if causal:
                qc, kc, vc = (qkv[:, i * d:(i + 1) * d].unflatten(1, (H, 64)) for i in range(3))
                k_rows = rows
            else:
                qc = qx.unflatten(1, (H, 64))
                kc, vc = (kvx[:, :, i * d:(i + 1) * d].unflatten(2, (H, 64)) for i in range(2))
                k_rows = None
            oc = torch.zeros(B * S, d, device=DEV, dtype=BF)
            o_lo = torch.zeros_like(oc)
            lse = torch.zeros(B, H, S, device=DEV)
            a = ops._attn_args_rows(qc, kc, vc, oc.view(B * S, H, 64), lse, B, H, S, Tk, rows, k_rows, kv_len if causal else None, causal)
            a.o_lo, a.q_span = o_lo.data_ptr(), span_d.data_ptr()
            ops._set_blocks(a, blocks)
            N.check(lib.oasr_attention_fwd(C.byref(a), stream), "attention_fwd")
            t_f = timed(lambda: lib.oasr_attention_fwd(C.byref(a), stream), 20)
            dq, dk, dv = (torch.empty_strided(t.shape, t.stride(), device=DEV, dtype=BF) for t in (qc, kc, vc))
            delta = torch.zeros(B, H, S, device=DEV)
            a.d_o, a.delta = doc.data_ptr(), delta.data_ptr()
            a.dq, a.dk, a.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
            a.dq_colsum, a.dv_colsum, a.colsum_scratch = csq.data_ptr(), csv.data_ptr(), scratch.data_ptr()
            N.check(lib.oasr_attention_bwd(C.byref(a), stream), "attention_bwd")
            t_b = timed(lambda: lib.oasr_attention_bwd(C.byref(a), stream), 20)
            results[(case, kind)] = (t_f, t_b)
            print(f"({case}) {kind:5s} n128={n128} of {4 * B}, n256={n256} of {2 * B}: forward {t_f[0]:7.1f} us (median {t_f[1]:7.1f}), "
                  f"backward (dQ + dK/dV + bias sums) {t_b[0]:7.1f} us (median {t_b[1]:7.1f})", flush=True)
    lib.oasr_attention_set_span_grid(1)
    blocks = ops.span_block_tables(real, B, S, H)
    f128, f256 = blocks[2] / (4 * B), blocks[3] / (2 * B)
    print(f"active fraction of the grid: 128-query blocks {f128:.3f}, 256-query blocks {f256:.3f}")
    for kind in ("self", "cross"):
        (fa, ba), (fb, bb), (fc, bc) = (results[(c, kind)] for c in "abc")
        print(f"{kind:5s} forward : (a) {fa[0]:.1f}  active x (b) {f128 * fb[0]:.1f}  (c) {fc[0]:.1f} us")
        print(f"{kind:5s} backward: (a) {ba[0]:.1f}  (b) {bb[0]:.1f}  (c) {bc[0]:.1f} us")


if __name__ == "__main__":
    main()
