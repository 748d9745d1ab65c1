"""The log-mel front end on the GPU against the cases and the per-cell rule of tests/logmel_cases.py (which has the reasoning; its CPU test
shows that the same checkers reject a scaled bin, swapped partner bins, a dropped sample slot, a shifted window tap, a filter weight off in
the fourth digit, the wrong padding and three ways of getting the per-clip floor wrong).

The default kernel (the quad-lane register FFT, csrc/logmel_quad.hip) runs every case in this process: the rule on the un-finalised values,
clip_max and the finalised tensor bit for bit against their definitions, guard bands around outputs and inputs (NaN / full-scale
sentinels), int16 against the same samples as f32, the same clip alone / inside a batch / at an unaligned address (the scalar and the
vector staging path feed identical arithmetic), run-to-run equality.  The three A/B kernels (OASR_LOGMEL=mfma|fft|fft32; the switch is
read once per process) run tone_sweep, staging and floor against the same rule in one fresh child interpreter each.

Measured on an MI355X (printed by the tests) at gamma = 4.2: worst |err| / bound per family, in brackets the gamma the kernel needs
(whisper's own fp32 arithmetic on the CPU needs 1.48 / 0.00 / 2.10 / 1.02 on tone_sweep / impulse_walk / staging / floor):
  default (quad)          tone_sweep 0.306 (1.23)   impulse_walk 0.308 (0.00)   staging 0.449 (1.14)   floor 0.695 (0.07)
  OASR_LOGMEL=mfma        tone_sweep 0.552 (2.24)                               staging 0.531 (1.15)   floor 0.911 (2.71)
  OASR_LOGMEL=fft, fft32  tone_sweep 0.240 (0.99)                               staging 0.520 (0.98)   floor 0.911 (2.71)
  quiet int16 clips (a few counts) between full-scale samples, default kernel: 0.425
Two properties of the quad kernel that these tests pin (csrc/logmel_quad.hip, end of the mel phase):
  * whisper's clamp at 1e-10 is applied to the logarithm, so a silent cell is exactly -10 and finalises to exactly -1.5 (the product
    fl(log2(1e-10f)) * fl(log10 2) is -10.00000095, one ulp below);
  * the mel weights carry 2^16 and the conversion to log10 is one fma that takes it out again, so one ulp of the hardware log2 is 1.9e-6
    and not 3.8e-6 for powers below 2.3e-10.  With the unscaled weights and a separately rounded product the cell floor / clip 3 / filter 31 /
    frame 9 (power 1.76e-10) needed gamma 4.40 against 4.2: the logarithm alone used up RHO there.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glue_ref as gr  # noqa: E402
import logmel_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32


@pytest.fixture(scope="module")
def ops():
    from olmoasr_amd import ops as o
    return o


@pytest.fixture(scope="module")
def runs(ops):
    """{case name: (raw, clip_max, finalised)} of the default kernel, on the CPU; every case runs once."""
    out = {}
    for c in lc.cases():
        pcm = lc.to_gpu(c, DEV)
        raw, cm = ops.log_mel(pcm, finalize=False)
        out[c.name] = (raw.cpu(), cm.cpu(), ops.log_mel(pcm).cpu())
    return out


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(lc.FAMILIES))
def test_every_cell_meets_the_rule(runs, family):
    worst = {c.name: lc.check(c, runs[c.name][0]) for c in lc.cases(family)}
    w = max(worst, key=worst.get)
    print(f"log-mel (default kernel) {family}: worst |err| / bound {worst[w]:.3f} at {w}, gamma {lc.GAMMA}; "
          f"gamma needed {max(lc.gamma_needed(c, runs[c.name][0]) for c in lc.cases(family)):.2f}")
    shapes = {runs[c.name][0].shape for c in lc.cases(family)}
    assert all(s[1] == 80 for s in shapes)


def test_clip_max_and_finalised_values_are_their_definitions(runs):
    for c in lc.cases():
        raw, cm, fin = runs[c.name]
        assert raw.shape == fin.shape == (c.pcm.shape[0], 80, c.pcm.shape[1] // 160) and cm.shape == (c.pcm.shape[0],)
        assert torch.equal(cm, raw.amax(dim=(1, 2))), f"{c.name}: clip_max differs from the clip's own maximum in clips {lc.clip_max_errors(raw, cm)}"
        assert torch.equal(fin, lc.finalize_ref(raw, cm)), c.name
        assert torch.equal(fin, lc.finalize_ref(raw.to(DEV), cm.to(DEV)).cpu()), c.name


def test_floor_is_per_clip(runs):
    c = lc.case("floor/f32")
    raw, cm, fin = runs[c.name]
    r = lc.reference(c)
    # the silent clip: log10 of the clamp, exactly
    assert bool((raw[2] == -10.0).all()) and float(cm[2]) == -10.0, (float(raw[2].min()), float(raw[2].max()))
    assert bool((fin[2] == -1.5).all())
    # every clip's maximum is its own: within the rule of the float64 maximum of its live frames (five clips, 50 dB apart)
    want = np.log10(r.power.max(axis=(1, 2)))
    assert np.abs(cm.numpy().astype(np.float64) - want).max() < 1e-5, (cm.tolist(), want.tolist())
    # clip 3: its 0.9 burst lies in the frame that is dropped; the clip keeps its own floor (none of its cells is 8 below its maximum ...)
    assert lc.ratios(c, raw)[3].max() <= 1.0
    assert float(cm[3]) < -8.0 and torch.equal(fin[3], (raw[3] + 4.0) * 0.25) and float((fin[3] > fin[3].min()).float().mean()) > 0.9
    # clip 4: the maximum lies in the second block of 64 frames
    assert int(raw[4].amax(0).argmax()) >= 64 and float(cm[4]) - float(raw[4, :, :64].max()) > 8.0
    # clip 1 under clip 0's maximum would lose cells to the floor; under its own it loses none
    assert torch.equal(fin[1], (raw[1] + 4.0) * 0.25) and bool((raw[1] < cm[0] - 8.0).any())


# ---- guard bands ---------------------------------------------------------------------------------------------------------------------
def pcm_between(t, fill, front=64, back=512):
    """The samples (CPU [B, n], int16 or f32) on the GPU with ``front`` / ``back`` elements of ``fill`` around them; front = 64 keeps the
    16-byte alignment of the first clip."""
    buf = torch.full((front + t.numel() + back,), fill, dtype=t.dtype, device=DEV)
    view = buf[front:front + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def native_log_mel(pcm_view, finalize):
    """oasr_log_mel / oasr_log_mel_raw through ctypes into outputs between guard bands.  Returns (mel, clip_max or None), both on the CPU."""
    from olmoasr_amd import _native as N
    B, n = pcm_view.shape
    dt = 1 if pcm_view.dtype == torch.int16 else 0
    gm, mel = gr.guarded(torch.zeros(B, 80, n // 160, dtype=F32), device=DEV)
    gc, cm = gr.guarded(torch.zeros(B, dtype=F32), device=DEV)
    ws = torch.empty(N.lib().oasr_log_mel_workspace_bytes(B), device=DEV, dtype=torch.uint8)
    if finalize:
        N.check(N.lib().oasr_log_mel(N.ptr(pcm_view), dt, B, n, N.ptr(mel), N.ptr(ws), N.stream_ptr()), "oasr_log_mel")
    else:
        N.check(N.lib().oasr_log_mel_raw(N.ptr(pcm_view), dt, B, n, N.ptr(mel), N.ptr(cm), N.ptr(ws), N.stream_ptr()), "oasr_log_mel_raw")
    torch.cuda.synchronize()
    gm.check("log-mel output")
    gc.check("clip_max output")
    assert not finalize or bool((cm == 0).all())  # (not an output of oasr_log_mel)
    return mel.cpu(), (None if finalize else cm.cpu())


GUARDED = ["floor/f32", "staging/f32/2x201", "staging/f32/2x319", "staging/f32/2x10239", "staging/f32/3x30723", "staging/i16/2x201",
           "staging/i16/2x10239", "staging/i16/3x30723", "impulse_walk/i16"]


@pytest.mark.parametrize("name", GUARDED)
def test_guard_bands_and_poisoned_surroundings(runs, name):
    """Outputs between sentinels, inputs between NaN (f32) / full-scale samples (int16): nothing outside a clip is read, nothing outside the
    outputs written -- the values are those of the plain run, bit for bit."""
    c = lc.case(name)
    t = torch.from_numpy(np.array(c.pcm))
    fills = (float("nan"),) if t.dtype == F32 else (32767, -32768)
    for fill in fills:
        buf, view = pcm_between(t, fill)
        raw, cm = native_log_mel(view, finalize=False)
        fin, _ = native_log_mel(view, finalize=True)
        assert torch.equal(raw, runs[name][0]) and torch.equal(cm, runs[name][1]) and torch.equal(fin, runs[name][2]), (name, fill)
        assert bool((buf[:64] != buf[:64]).all() if t.dtype == F32 else (buf[:64] == fill).all())  # the input is not written either
        assert torch.equal(view.cpu(), t)


def test_quiet_int16_clips_between_full_scale_samples(ops):
    """Clips at 1 / 256 of the staging amplitude (a few counts) between full-scale samples: one sample read from outside a clip would be the
    loudest thing in its frame."""
    src = lc.case("staging/i16/2x10239")
    quiet = lc.Case("quiet/i16/2x10239", (src.pcm.astype(np.int32) // 256).astype(np.int16))
    t = torch.from_numpy(np.array(quiet.pcm))
    assert 0 < int(t.abs().max()) < 128
    for fill in (32767, -32768):
        _, view = pcm_between(t, fill)
        raw, cm = native_log_mel(view, finalize=False)
        print(f"log-mel quiet int16 between {fill}: worst |err| / bound {lc.check(quiet, raw):.3f}")
        assert not lc.clip_max_errors(raw, cm)
        # the two clips are separated by nothing: each must also ignore its neighbour
        for b in range(2):
            alone, _ = ops.log_mel(t[b:b + 1].contiguous().to(DEV), finalize=False)
            assert torch.equal(alone.cpu()[0], raw[b])


# ---- one arithmetic, whatever the path -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", lc.STAGING_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}+{s[2]}")
def test_int16_equals_the_same_samples_as_f32(ops, runs, shape):
    B, n, off = shape
    name = f"staging/i16/{B}x{n}" + (f"+{off}" if off else "")
    c = lc.case(name)
    f = lc.Case(name + "/as_f32", (c.pcm.astype(np.float32) / np.float32(32768.0)), off)
    assert np.array_equal(f.pcm.astype(np.float64), lc.as_float64(c.pcm))
    pcm = lc.to_gpu(f, DEV)
    assert (pcm.data_ptr() % 16 == 0) == (off == 0)
    raw, cm = ops.log_mel(pcm, finalize=False)
    assert torch.equal(raw.cpu(), runs[name][0]) and torch.equal(cm.cpu(), runs[name][1])
    assert torch.equal(ops.log_mel(pcm).cpu(), runs[name][2])


@pytest.mark.parametrize("dtype", ["i16", "f32"])
def test_same_clip_alone_in_a_batch_and_unaligned(ops, dtype):
    """One clip's content (192 frames: block 1 can take the vector path) alone, as clip 1 of an aligned batch, in batches whose clips are
    not 16-byte aligned, and alone one element off: the vector and the scalar staging path feed the same arithmetic, and no clip sees
    its neighbours."""
    src = lc.case(f"staging/{dtype}/3x30720").pcm
    other = lc.case(f"staging/{dtype}/3x30723").pcm
    x = torch.from_numpy(np.array(src[1]))
    n = x.numel()

    def run(batch, b, offset=0):
        pcm = lc.to_gpu(lc.Case("tmp", batch.numpy(), offset), DEV)
        assert (pcm[b].data_ptr() % 16 == 0) == (offset == 0 and (b * batch.shape[1] * batch.element_size()) % 16 == 0)
        raw, cm = ops.log_mel(pcm, finalize=False)
        fin = ops.log_mel(pcm)
        return raw[b].cpu(), cm[b].cpu(), fin[b].cpu()

    alone = run(x[None], 0)
    batch = torch.from_numpy(np.array(other[:, :n]))
    batch[1] = x
    # a batch of clips of n + 3 samples whose clip 1 starts with the same n samples has other frames at its end: compare the common ones
    odd = torch.from_numpy(np.array(other))
    odd[1, :n] = x
    placements = {"aligned batch": run(batch, 1), "batch one element off": run(batch, 1, 1), "alone one element off": run(x[None], 0, 1),
                  "alone three elements off": run(x[None], 0, 3)}
    for what, got in placements.items():
        for a, g, part in zip(alone, got, ("raw", "clip_max", "finalised")):
            assert torch.equal(a, g), f"{dtype}, {what}: {part} differs from the clip run alone in {int((a != g).sum())} cells"
    # clip 1 of the 3 x 30723 batch is unaligned and 3 samples longer: frames whose 400 samples lie inside the common part are the same frames
    raw_odd, _, _ = run(odd, 1)
    last_common = (n - 200 - 3) // 160 - 1
    assert torch.equal(raw_odd[:, :last_common], alone[0][:, :last_common])


def test_two_runs_are_identical(ops, runs):
    for name in ("tone_sweep/f32", "floor/f32", "staging/i16/3x30723", "staging/f32/2x20639", "impulse_walk/f32"):
        pcm = lc.to_gpu(lc.case(name), DEV)
        raw, cm = ops.log_mel(pcm, finalize=False)
        assert torch.equal(raw.cpu(), runs[name][0]) and torch.equal(cm.cpu(), runs[name][1]) and torch.equal(ops.log_mel(pcm).cpu(), runs[name][2])


# ---- the three A/B kernels -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def default_report(ops):
    return lc.gpu_report()


def test_default_kernel_report(default_report):
    r = default_report
    print(f"log-mel default kernel: worst |err| / bound {r['worst']}, gamma needed {r['gamma_needed']}")
    assert not r["clip_max_errors"] and all(v <= 1.0 for v in r["worst"].values()) and all(v <= lc.GAMMA for v in r["gamma_needed"].values())


@pytest.mark.parametrize("kernel", ["mfma", "fft", "fft32"])
def test_ab_kernel_meets_the_rule(kernel, default_report):
    """OASR_LOGMEL is read once per process: one fresh child interpreter per kernel runs tone_sweep, staging and floor against the same
    rule (tests/logmel_cases.py as a program) and reports its worst ratios and the gamma it needs.  No bit equality between kernels is asked
    for -- but the digest of the child's outputs must differ from the default kernel's: another kernel did run."""
    env = dict(os.environ, OASR_LOGMEL=kernel, OASR_TESTING_HOOKS="1")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "logmel_cases.py")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"OASR_LOGMEL={kernel}: {r.stderr[-3000:]}"
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    print(f"log-mel OASR_LOGMEL={kernel}: worst |err| / bound {out['worst']}, gamma needed {out['gamma_needed']} over {out['cases']} cases")
    assert out["kernel"] == kernel and out["cases"] == default_report["cases"] == 2 + 2 * len(lc.STAGING_SHAPES)
    assert out["digest"] != default_report["digest"], f"OASR_LOGMEL={kernel} gave the default kernel's outputs bit for bit: the switch was not honoured"
    assert not out["clip_max_errors"], out["clip_max_errors"]
    assert set(out["worst"]) == {"tone_sweep", "staging", "floor"} and all(0.0 <= v <= 1.0 for v in out["worst"].values()), out["worst"]
    assert all(v <= lc.GAMMA for v in out["gamma_needed"].values()), out["gamma_needed"]
