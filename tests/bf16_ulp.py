"""The bf16-against-bf16 report shared by the oracle parity tests of the training step (test_gpu_parity_sizes.py) and of the KV-cached
decoder step (test_gpu_decode_step_oracle.py): one definition of "ulp of the logit scale", one set of histogram edges."""
import math


def bf16_ulp_report(native, mirror, valid, tag):
    """native (bf16 engine) vs the oracle's autocast MIRROR (same rounding points, CPU accumulation order), in bf16 ulps of the logit
    scale: ulp = 2^(floor(log2 max|logit|) - 7), the spacing of bf16 at the largest logit.  Returns (fraction within 2 ulp, max in ulp)."""
    scale = float(mirror[valid].abs().max())
    ulp = 2.0 ** (math.floor(math.log2(scale)) - 7)
    d = (native - mirror).abs()[valid] / ulp
    hist = [float((d <= k).float().mean()) for k in (0.5, 1, 2, 4)]
    print(f"   [{tag}] bf16 engine vs autocast mirror, valid logits: scale {scale:.2f} -> ulp {ulp:.5f}; within 0.5/1/2/4 ulp: "
          f"{hist[0]:.5f} {hist[1]:.5f} {hist[2]:.5f} {hist[3]:.5f}; max {float(d.max()):.2f} ulp; mean {float(d.mean()):.3f} ulp")
    return hist[2], float(d.max())
