"""The argmax gate of tests/test_gpu_decode_step_oracle.py, checked without a GPU on the cases where it matters most: at least half of the
(b, p) positions have a top-2 gap of the fp32 oracle above twice the autocast mirror's envelope -- from the oracle alone, so the gate cannot
hide an engine's failure -- and both oracle evaluations are finite at the extremes of the audio context (1 and 1728 keys) and over the full
text context.  (Every GPU case asserts its own share before it looks at the engine; running all of them here would cost the CPU suite half a minute.)"""
import pytest
import torch

import test_gpu_decode_step_oracle as T

KEYS = [(d, H, B, 12, Te, True, seed) for d, H, B, _, Te, seed in T.C_CASES if B == 1 and Te in (1728, 5, 1)] + [T.D_KEY]


@pytest.mark.parametrize("key", KEYS, ids=[f"Te{k[4]}-S{k[3]}" for k in KEYS])
def test_half_the_positions_are_clear(key):
    c = T._build_case(*key)
    assert torch.isfinite(c["ref"]).all() and torch.isfinite(c["mir"]).all()
    share = float(c["clear"].float().mean())
    print(key, f"clear positions {share:.3f}, mirror envelope max {c['env_max']:.4f}")
    assert share >= 0.5, share
