"""CPU power test of tests/logmel_cases.py: what the GPU tests of the log-mel front end (tests/test_gpu_logmel.py) lean on.

  * the case table has the properties its docstrings claim (shapes, frame counts, alignment of the clips, which frame sees which burst);
  * gamma_ref: whisper's own fp32 arithmetic meets the rule on every cell of every case at the pinned GAMMA_REF, the measured figure is
    <= 8, and GAMMA_REF is that figure rounded up to one decimal place;
  * the float64 pipeline written out stage by stage agrees with the oracle's ``power_spectrogram`` route and passes the rule at gamma = 0
    (the rule's RHO term alone covers the fp32 store of the logarithm);
  * every planted flaw of ``logmel_cases.FLAWS`` is rejected by the case named next to it, at the gamma the kernels are held to.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logmel_cases as lc  # noqa: E402

from oracle import mel_oracle as me  # noqa: E402


@pytest.fixture(scope="module")
def gamma_by_case():
    return {c.name: lc.gamma_needed(c, lc.whisper_fp32(c)) for c in lc.cases()}


def test_case_table():
    by = {c.name: c for c in lc.cases()}
    assert len(by) == len(lc.cases()) == 1 + 2 + 2 * len(lc.STAGING_SHAPES) + 1
    assert all(c.pcm.shape[1] <= 65536 and c.pcm.dtype in (np.int16, np.float32) and c.pcm.ndim == 2 for c in lc.cases())
    # tone_sweep: 11 frames, clip k - 1 peaks in bin k in its interior frames
    t = by["tone_sweep/f32"]
    assert t.pcm.shape == (201, 1760)
    P = me.power_spectrogram(lc.as_float64(t.pcm))[:, :, 5]
    assert P.shape == (201, 201) and (P[:199].argmax(1) == np.arange(1, 200)).all() and P[199].argmax() == 0 and P[200].argmax() == 200
    # impulse_walk: 402 frames; every one of the 400 slots of the frame holds an impulse in some frame
    for name in ("impulse_walk/f32", "impulse_walk/i16"):
        x = lc.as_float64(by[name].pcm)
        assert x.shape == (1, 161 * 400) and x.shape[1] // 160 == 402
        fr = lc.frames64(x)[0, 1:401]  # (frames clear of the reflections)
        assert ((fr != 0).sum(0) >= 1).all() and (np.abs(x[x != 0]) >= 0.1 - 1e-4).all() and (np.abs(x) <= 0.9).all()
    # staging: the shapes of the issue, in both sample formats; the frame-count edges
    shapes = {(B, n, off) for B, n, off in lc.STAGING_SHAPES}
    assert {(3, 30720, 0), (3, 30723, 0), (2, 30728, 0), (2, 30720, 1)} <= shapes
    edges = {n: (n // 160, (n // 160) % 64, n % 160) for B, n, off in lc.STAGING_SHAPES if B == 2 and off == 0 and n < 30000}
    assert edges == {201: (1, 1, 41), 319: (1, 1, 159), 320: (2, 2, 0), 10240: (64, 0, 0), 10239: (63, 63, 159), 10400: (65, 1, 0),
                     20480: (128, 0, 0), 20639: (128, 0, 159)}
    for B, n, off in lc.STAGING_SHAPES:
        tag = f"{B}x{n}" + (f"+{off}" if off else "")
        i, f = by[f"staging/i16/{tag}"], by[f"staging/f32/{tag}"]
        assert i.pcm.shape == f.pcm.shape == (B, n) and i.pcm.dtype == np.int16 and f.pcm.dtype == np.float32 and i.offset == f.offset == off
        if n >= 10239:  # up to 60 dB between hops (a frame spans 2.5 of them): the loudest and the quietest frame of a clip are far apart
            nrm = np.sqrt((lc.frames64(lc.as_float64(f.pcm)) ** 2).sum(-1))
            assert (nrm.max(1) / nrm.min(1) > 10).all()
    # which clips start on a 16-byte boundary (clip b starts b * n + offset elements into a 16-byte aligned allocation)
    al = lambda B, n, off, size: [((b * n + off) * size) % 16 == 0 for b in range(B)]
    assert al(3, 30720, 0, 2) == al(3, 30720, 0, 4) == [True] * 3
    assert al(3, 30723, 0, 2) == al(3, 30723, 0, 4) == [True, False, False]
    assert al(2, 30720, 1, 2) == al(2, 30720, 1, 4) == [False, False]
    # floor: what each clip is there for
    fl = by["floor/f32"]
    assert fl.pcm.shape == (5, 20639)
    raw, cm = lc.pipeline64(fl)
    assert raw.shape == (5, 80, 128)
    assert bool((raw[2] == -10.0).all()) and cm[2] == -10.0
    assert cm[0] - cm[1] > 6.0 and cm[0] - cm[3] > 8.0          # a batch-wide floor would flatten clips 1 (partly) and 3 (wholly)
    assert bool((raw[1] < cm[0] - 8.0).any()) and not bool((raw[1] < cm[1] - 8.0).any()) and float(cm[3]) < -8.0
    assert float((raw[3] > raw[3].min()).float().mean()) > 0.9  # clip 3 is not flat against the clamp
    lp = np.log10(np.maximum(np.einsum("mk,btk->bmt", me.mel_filters().astype(np.float64),
                                       np.abs(np.fft.rfft(lc.frames64(lc.as_float64(fl.pcm)) * me.hann_window(), axis=-1)) ** 2), 1e-10))
    live3 = raw[3].numpy()
    assert lp[3, :, 128].max() - float(cm[3]) > 6.0 and (live3 < lp[3, :, 128].max() - 8.0).mean() > 0.1  # the dropped frame of clip 3 would floor live cells
    assert lp[3, :, :128].max() == pytest.approx(float(cm[3]), abs=1e-6)
    assert int(raw[4].amax(0).argmax()) in (99, 100, 101) and float(cm[4]) - float(raw[4, :, :64].max()) > 8.0  # the maximum lies in block 1


def test_gamma_ref(gamma_by_case):
    """whisper's fp32 arithmetic under the rule: the measured gamma, per family (printed; copied into the module docstring)."""
    fam = {}
    for name, g in gamma_by_case.items():
        fam[name.split("/")[0]] = max(fam.get(name.split("/")[0], 0.0), g)
    worst = max(gamma_by_case, key=gamma_by_case.get)
    print("gamma_ref per family:", {k: round(v, 3) for k, v in fam.items()}, "worst case:", worst, round(gamma_by_case[worst], 3))
    g = gamma_by_case[worst]
    assert math.isfinite(g) and g <= lc.GAMMA_CAP == 8.0, f"gamma_ref {g} at {worst}: the cases or the rule are wrong"
    assert g <= lc.GAMMA_REF < g + 0.1, f"logmel_cases.GAMMA_REF {lc.GAMMA_REF} is not the measured {g:.3f} rounded up to one decimal place"
    assert lc.GAMMA == 2.0 * lc.GAMMA_REF and lc.RHO == 2.0 ** -18
    for c in lc.cases():
        assert lc.check(c, lc.whisper_fp32(c), gamma=lc.GAMMA_REF) <= 1.0


def test_float64_pipeline_against_the_oracle():
    fb = me.mel_filters().astype(np.float64)
    for c in lc.cases():
        raw, cm = lc.pipeline64(c)
        want = np.log10(np.maximum(np.einsum("mk,bkt->bmt", fb, me.power_spectrogram(lc.as_float64(c.pcm))), 1e-10))
        assert np.array_equal(raw.numpy(), want.astype(np.float32)) or np.abs(raw.numpy().astype(np.float64) - want).max() < 2e-6, c.name
        assert np.abs(10.0 ** want - lc.reference(c).power).max() <= 1e-12 * lc.reference(c).power.max()
        assert lc.check(c, raw, gamma=0.0) <= 1.0            # the fp32 store of the logarithm fits RHO on its own
        assert lc.gamma_needed(c, raw) == 0.0
        assert not lc.clip_max_errors(raw, cm)
    # the rule's terms: non-negative, zero exactly where the frame is silent
    r = lc.reference(lc.case("floor/f32"))
    assert (r.lin >= 0).all() and (r.quad >= 0).all() and (r.lin[2] == 0).all() and (r.quad[2] == 0).all() and (r.power[2] == 1e-10).all()
    assert (r.quad[[0, 1, 3, 4]] > 0).all()


@pytest.mark.parametrize("flaw", sorted(lc.FLAWS))
def test_flaw_is_rejected(flaw):
    c = lc.case(lc.FLAWS[flaw])
    raw0, cm0 = lc.pipeline64(c)
    raw, cm = lc.pipeline64(c, flaw)
    if flaw in ("batch_wide_maximum", "dropped_frame_in_maximum", "maximum_of_block_0_only"):
        assert torch.equal(raw, raw0) and lc.check(c, raw) <= 1.0   # the cells are right, the floor is not
        bad = lc.clip_max_errors(raw, cm)
        assert bad, flaw
        loudest = int(cm0.argmax())
        want = {"batch_wide_maximum": [b for b in (0, 1, 2, 4, 3) if b != loudest], "dropped_frame_in_maximum": [3], "maximum_of_block_0_only": [4]}[flaw]
        assert set(want) <= set(bad), (flaw, bad)
        # ... and the finalised tensor differs where it matters: the clip's own floor
        assert not torch.equal(lc.finalize_ref(raw, cm)[want[-1]], lc.finalize_ref(raw0, cm0)[want[-1]])
        return
    with pytest.raises(AssertionError, match="cells off by more than the rule"):
        lc.check(c, raw)
    q = lc.ratios(c, raw)
    print(f"{flaw}: worst |err| / bound {q.max():.3g} on {c.name}, {int((q > 1).sum())} of {q.size} cells")
    if flaw == "bin_scaled_1e-4":      # the cells that catch it are the ones the tone at that bin dominates
        bad = np.argwhere(q > 1)                                   # (and its neighbours' leakage, and edge frames of others)
        assert lc.FLAW_BIN - 1 in set(bad[:, 0]) and set(bad[:, 1]) <= set(np.nonzero(me.mel_filters()[:, lc.FLAW_BIN])[0])
    if flaw == "filter_weight_1e-4":
        bad = np.argwhere(q > 1)
        assert set(bad[:, 1]) == {lc.FLAW_FILTER[0]} and lc.FLAW_FILTER[1] - 1 in set(bad[:, 0])


def test_checker_edges():
    c = lc.case("staging/f32/2x201")
    raw, cm = lc.pipeline64(c)
    bad = raw.clone()
    bad[1, 40, 0] = float("nan")
    with pytest.raises(AssertionError):
        lc.check(c, bad)
    with pytest.raises(AssertionError):
        lc.check(c, raw[:, :, :0])
    z = lc.case("floor/f32")
    rawz, _ = lc.pipeline64(z)
    off = rawz.clone()
    off[2, 7, 3] = -9.9999  # a silent frame has no gamma term: only RHO
    with pytest.raises(AssertionError):
        lc.check(z, off)
    assert lc.gamma_needed(z, off) == float("inf")
