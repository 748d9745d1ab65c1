"""Times the fused cross-entropy kernel (fwd + in-place bwd) at the benchmarked shape: [57344, 51968] bf16 logits, all rows valid.
--label_smoothing / --z_loss (either non-zero): the regularised instantiation is timed against the plain one in the same run, alternating."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from olmoasr_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--label_smoothing", type=float, default=0.0)
ap.add_argument("--z_loss", type=float, default=0.0)
opt = ap.parse_args()
variants = [("plain", {})]
if opt.label_smoothing or opt.z_loss:
    variants.append((f"label_smoothing={opt.label_smoothing:g} z_loss={opt.z_loss:g}", dict(label_smoothing=opt.label_smoothing, z_loss=opt.z_loss)))

rows, V, Vp = 57344, 51865, 51968
lg = torch.randn(rows, Vp, device="cuda", dtype=torch.bfloat16)
for frac_valid in (1.0, 0.25):
    tgt = torch.randint(0, 50000, (rows,), device="cuda")
    if frac_valid < 1.0:
        tgt[torch.rand(rows, device="cuda") > frac_valid] = 51864
    for _, kw in variants:
        ops.cross_entropy_(lg, V, tgt, 51864, **kw)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = {name: 1e9 for name, _ in variants}
    for _ in range(3):
        for name, kw in variants:
            lg.normal_()
            torch.cuda.synchronize()
            e0.record()
            ops.cross_entropy_(lg, V, tgt, 51864, **kw)
            e1.record()
            torch.cuda.synchronize()
            best[name] = min(best[name], e0.elapsed_time(e1))
    nv = int((tgt != 51864).sum())
    actual = nv * 4 * Vp + (rows - nv) * 2 * Vp
    for name, _ in variants:
        b = best[name]
        tag = "" if len(variants) == 1 else f" [{name}]"
        print(f"valid rows {frac_valid:.2f}{tag}: {b:.3f} ms = {rows * 4 * Vp / b / 1e9:.2f} TB/s algorithmic (4 V' B/row), {actual / b / 1e9:.2f} TB/s of bytes actually moved")
    if len(variants) > 1:
        print(f"valid rows {frac_valid:.2f}: regularised / plain = {best[variants[1][0]] / best['plain']:.4f}")
