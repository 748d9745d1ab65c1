"""Cases, float64 reference, error rule and deliberately flawed stand-ins for the log-mel front end (numpy / torch on the CPU, no GPU needed).

``ops.log_mel`` (csrc/logmel.hip and its kernel files csrc/logmel_quad.hip, logmel_fft.hip, logmel_dft.hip) goes wrong in a FEW CELLS: one (lane, register) slot of the quad-lane FFT, one unpack
partner, one filter's slot weight, one window tap, one staged sample at a block seam, a clip maximum that saw the frame whisper drops.  A
flat tolerance on the finalised value (2e-3 where the kernel's error is 1.6e-6) cannot see any of that.  This module gives the front end

  * inputs in which every bin, every sample slot of the frame, both staging paths, every frame-count edge and every way of getting the
    per-clip floor wrong is the dominant term of some output cell (``tone_sweep``, ``impulse_walk``, ``staging``, ``floor``), and
  * a per-cell bound derived in the POWER domain from the float64 oracle (oracle/mel_oracle.py: ``power_spectrogram``, ``mel_filters``):

        got = 10 ** raw                     (float64, raw = the kernel's un-finalised log10 value)
        ref = max(fb @ |X|^2, 1e-10)
        |got - ref| <= sum_k fb[m, k] (2 |X[k, t]| d_t + d_t^2) + RHO ref,      d_t = gamma 2^-24 max(||x_t||_2, max_k |X[k, t]|)

    d_t is the error an fp32 transform of the frame leaves in every bin, whatever its summation order; the first term is that error
    carried through |X|^2 and the filter.  It has two scales:
      * ||x_t||_2, the norm of the frame's 400 reflect-padded samples, UNWINDOWED: an fp32 hann table carries an absolute error of about
        2^-25, not a relative one, so the windowed norm under-scales the frames a loud edge leaks into.  This is the scale of noise-like
        and sparse frames, where roundings add up at random;
      * max_k |X[k, t]|, the largest bin (all 201): the transform's intermediate values grow to the size of its largest output, and one
        rounding of such a value is 2^-24 max|X| wherever it lands -- in a packed real transform, which torch's and this project's FFT
        kernels are, first of all in the partner bin 200 - k.  By Cauchy-Schwarz max|X| <= ||hann||_2 ||x_t||_2 = 12.25 ||x_t||_2; noise stays
        near 1.3 ||x_t||_2, a frame holding one tone reaches 7.07 ||x_t||_2 (|X[k0]| = 50 where ||x_t||_2 = 7.07) with bins five orders of magnitude
        smaller next to it, visible wherever the reflection at a clip's end breaks the tone.  With ||x_t||_2 alone whisper's own fp32
        arithmetic needs gamma = 10.4 on those frames of tone_sweep against 3.3 on noise; with both scales the families need the same.
    RHO = 2^-18 covers the filter's <= 20-term fma chain, a 1-2 ulp hardware log2 at |log2| < 64 and the fp32 store of the logarithm.

gamma is MEASURED, not chosen: ``gamma_needed`` returns the smallest gamma under which an output meets the rule on every cell, and
tests/test_logmel_cases_cpu.py applies it to whisper's own arithmetic (``whisper_fp32``: torch.stft in float32 on the CPU with
torch.hann_window(400), the fp32 filterbank matmul, torch.log10) over every case of the table:

    gamma_ref = 2.10 (staging/i16/2x20480); per family: tone_sweep 1.48, impulse_walk 0.00, staging 2.10, floor 1.02

The CPU test asserts gamma_ref <= 8 (a larger figure means the cases or the rule are wrong) and that GAMMA_REF below is the measured
figure rounded up to one decimal place.  The kernels get GAMMA = 2 GAMMA_REF = 4.2; the factor 2 is for a different but equally legitimate
fp32 summation order.  One gamma multiplies both scales: in units of ||x_t||_2 alone a noise-like frame is held to about 4.2 x 1.3 = 5.5, a
frame holding one tone to 4.2 x 7.07 = 30.  The gamma term matters only for the SMALL bins of such a frame; where a bin dominates its cell
the gamma term is far below RHO ref (2 d_t / |X| = 5e-7 against 3.8e-6 for the tones), so the checks on tone bins, slots and weights rest
on RHO, not on gamma: tests/test_logmel_cases_cpu.py rejects every planted flaw at GAMMA, the closest (a filter weight off by 1e-4) 15 times
over.

``pipeline64`` is the same front end written out step by step in float64 (frames, window, rfft, filterbank, log10, clip maximum), with one
planted mistake per entry of ``FLAWS``; the CPU test shows that the checkers accept it without a flaw at gamma = 0 and reject every flaw
on the case named next to it.

Run as a program (``python tests/logmel_cases.py``) it applies the rule to whichever kernel OASR_LOGMEL selects in THIS process (the switch
is read once per process) on tone_sweep, staging and floor and prints the worst ratios as one JSON line: the child of tests/test_gpu_logmel.py.
"""
import functools
import json
import os
import sys
from dataclasses import dataclass

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import mel_oracle as me  # noqa: E402

E24 = 2.0 ** -24
RHO = 2.0 ** -18
GAMMA_REF = 2.1            # measured (tests/test_logmel_cases_cpu.py::test_gamma_ref): 2.097, rounded up to one decimal place
GAMMA = 2.0 * GAMMA_REF    # what the kernels are held to
GAMMA_CAP = 8.0            # gamma_ref above this: the cases or the rule are wrong
NFFT, HOP, NMEL, QT = me.N_FFT, me.HOP_LENGTH, 80, 64


@dataclass(frozen=True, eq=False)
class Case:
    name: str          # family/detail
    pcm: np.ndarray    # [B, n] int16 or float32
    offset: int = 0    # the GPU tensor starts this many elements into a larger allocation (a base that is not 16-byte aligned)

    @property
    def family(self):
        return self.name.split("/")[0]


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def tone_sweep():
    """f32 [201, 1760]: clip k - 1 = 0.5 sin(2 pi k n / 400 + phi_k), k = 1..199; clip 199 constant 0.25; clip 200 alternating +-0.5."""
    rng = np.random.default_rng(101)
    n = np.arange(1760, dtype=np.float64)
    k = np.arange(1, 200, dtype=np.float64)[:, None]
    phi = rng.uniform(0.0, 2.0 * np.pi, (199, 1))
    x = np.empty((201, 1760), dtype=np.float64)
    x[:199] = 0.5 * np.sin(2.0 * np.pi * k * n / NFFT + phi)
    x[199] = 0.25
    x[200] = 0.5 * (1.0 - 2.0 * (np.arange(1760) % 2))
    return [Case("tone_sweep/f32", x.astype(np.float32))]


IMPULSE_N, IMPULSE_STEP = 161 * 400, 161


def impulse_walk():
    """One clip of 64400 samples, an impulse every 161 samples: it moves one slot per frame, so over 402 frames every one of the 400 sample
    slots of the frame is hit, each with its own signed amplitude in 0.1..0.9 (f32) / the same range in integer steps (int16)."""
    rng = np.random.default_rng(102)
    pos = np.arange(0, IMPULSE_N, IMPULSE_STEP)
    sign = rng.choice([-1.0, 1.0], pos.size)
    amp = rng.uniform(0.1, 0.9, pos.size) * sign
    f = np.zeros((1, IMPULSE_N), dtype=np.float32)
    f[0, pos] = amp.astype(np.float32)
    iamp = (rng.integers(3277, 29492, pos.size) * rng.choice([-1, 1], pos.size)).astype(np.int16)
    i = np.zeros((1, IMPULSE_N), dtype=np.int16)
    i[0, pos] = iamp
    return [Case("impulse_walk/f32", f), Case("impulse_walk/i16", i)]


STAGING_SHAPES = (  # (B, n, offset)
    (3, 30720, 0),   # every clip 16-byte aligned, 192 frames: block 1 takes the vector path
    (3, 30723, 0),   # odd clips unaligned: both paths in one launch
    (2, 30728, 0),   # f32: aligned; int16: clip 1 aligned too (30728 % 8 == 0) -- the vector path behind a frame that is dropped
    (2, 30720, 1),   # a view one element into a larger allocation: no block of any clip is aligned
    (2, 201, 0), (2, 319, 0), (2, 320, 0),                  # one frame with both reflections overlapping; one frame; two
    (2, 10240, 0), (2, 10239, 0), (2, 10400, 0),            # n_frames % 64 = 0, 63 (n % 160 = 159), 1
    (2, 20480, 0), (2, 20639, 0),                           # two whole blocks; the same with n % 160 = 159
)


def _hop_gain_noise(rng, B, n):
    """Noise whose gain changes every hop: 10^(-3 u), u uniform -- up to 60 dB between neighbouring hops."""
    u = rng.uniform(0.0, 1.0, (B, n // HOP + 1))
    gain = np.repeat(10.0 ** (-3.0 * u), HOP, axis=1)[:, :n]
    return np.clip(0.25 * rng.standard_normal((B, n)) * gain, -1.0, 1.0)


def staging():
    out = []
    for j, (B, n, off) in enumerate(STAGING_SHAPES):
        rng = np.random.default_rng(300 + j)
        x = _hop_gain_noise(rng, B, n)
        tag = f"{B}x{n}" + (f"+{off}" if off else "")
        out.append(Case(f"staging/i16/{tag}", np.round(x * 32767.0).astype(np.int16), off))
        out.append(Case(f"staging/f32/{tag}", _hop_gain_noise(rng, B, n).astype(np.float32), off))
    return out


FLOOR_N = 20639  # 128 frames; the frame whisper drops is centred on sample 20480 and is the only one that sees the last 119 samples


def floor():
    """f32 [5, 20639]: loud noise | noise at 1e-4 | zeros | 1e-5 noise with a 0.9 burst in the last 30 samples (only the dropped frame sees
    it) | 1e-5 noise with a 400-sample 0.9 burst centred on frame 100 (the clip maximum lies in block 1)."""
    rng = np.random.default_rng(104)
    x = np.zeros((5, FLOOR_N), dtype=np.float64)
    x[0] = np.clip(0.3 * rng.standard_normal(FLOOR_N), -1.0, 1.0)
    x[1] = 1e-4 * rng.standard_normal(FLOOR_N)
    x[3] = 1e-5 * rng.standard_normal(FLOOR_N)
    x[3, -30:] = 0.9 * rng.uniform(-1.0, 1.0, 30)
    x[4] = 1e-5 * rng.standard_normal(FLOOR_N)
    x[4, 100 * HOP - 200:100 * HOP + 200] = 0.9 * rng.uniform(-1.0, 1.0, 400)
    return [Case("floor/f32", x.astype(np.float32))]


FAMILIES = {"tone_sweep": tone_sweep, "impulse_walk": impulse_walk, "staging": staging, "floor": floor}


@functools.lru_cache(maxsize=None)
def cases(family=None):
    """The table (built once; the arrays are shared and must not be written to)."""
    out = []
    for name, fn in FAMILIES.items():
        if family in (None, name):
            out += fn()
    for c in out:
        c.pcm.setflags(write=False)
    return tuple(out)


def case(name):
    (c,) = [c for c in cases() if c.name == name]
    return c


def as_float64(pcm):
    """The samples as the front end defines them: int16 / 32768 (exact), float32 as is."""
    pcm = np.asarray(pcm)
    return pcm.astype(np.float64) / 32768.0 if pcm.dtype == np.int16 else pcm.astype(np.float64)


# ---- float64 reference and the rule ------------------------------------------------------------------------------------------------
def frames64(x, mode="reflect"):
    """[B, n] float64 -> [B, n // 160 + 1, 400]: the unwindowed frames of torch.stft(center=True), INCLUDING the last one, which whisper drops."""
    xp = np.pad(x, ((0, 0), (NFFT // 2, NFFT // 2)), mode=mode)
    T = x.shape[1] // HOP + 1
    idx = np.arange(NFFT)[None, :] + HOP * np.arange(T)[:, None]
    return xp[:, idx]


@dataclass(frozen=True, eq=False)
class Ref:
    power: np.ndarray   # [B, 80, T] max(fb @ |X|^2, 1e-10), float64
    lin: np.ndarray     # [B, 80, T] 2 s_t (fb @ |X|), s_t = 2^-24 max(||x_t||, max_k |X[k, t]|): the bound's term linear in gamma
    quad: np.ndarray    # [B, 80, T] s_t^2 sum_k fb[m, k]: the term quadratic in gamma


_REFS = {}


def reference(c):
    """The float64 oracle of a case and the two gamma terms of its bound, computed once per case."""
    if c.name not in _REFS:
        x = as_float64(c.pcm)
        P = me.power_spectrogram(x)                                   # [B, 201, T]
        fb = me.mel_filters().astype(np.float64)                      # [80, 201]
        T = P.shape[-1]
        nrm = E24 * np.maximum(np.sqrt((frames64(x)[:, :T] ** 2).sum(-1)), np.sqrt(P).max(axis=1))  # [B, T]
        power = np.maximum(np.einsum("mk,bkt->bmt", fb, P), 1e-10)
        lin = 2.0 * nrm[:, None, :] * np.einsum("mk,bkt->bmt", fb, np.sqrt(P))
        quad = (nrm ** 2)[:, None, :] * fb.sum(1)[None, :, None]
        _REFS[c.name] = Ref(power, lin, quad)
    return _REFS[c.name]


def _raw64(raw):
    return (raw.detach().cpu().numpy() if isinstance(raw, torch.Tensor) else np.asarray(raw)).astype(np.float64)


def ratios(c, raw, gamma=GAMMA):
    """|10^raw - ref| / bound per cell, [B, 80, T] (a cell whose bound is zero and whose error is not: inf)."""
    r = reference(c)
    raw = _raw64(raw)
    assert raw.shape == r.power.shape, (c.name, raw.shape, r.power.shape)
    err = np.abs(10.0 ** raw - r.power)
    bound = gamma * r.lin + gamma * gamma * r.quad + RHO * r.power
    with np.errstate(invalid="ignore"):
        out = err / bound
    return np.where(np.isfinite(raw), out, np.inf)


def check(c, raw, gamma=GAMMA):
    """Asserts the rule on every cell; returns the worst |err| / bound."""
    q = ratios(c, raw, gamma)
    bad = ~(q <= 1.0)
    if bad.any():
        b, m, t = (int(v) for v in np.argwhere(bad)[0])
        r = reference(c)
        raise AssertionError(f"{c.name}: {int(bad.sum())} of {bad.size} cells off by more than the rule (gamma {gamma}); first at clip {b}, "
                             f"filter {m}, frame {t}: got power {10.0 ** float(_raw64(raw)[b, m, t])!r}, want {float(r.power[b, m, t])!r}, "
                             f"|err| / bound {float(q[b, m, t]):.3g}; worst {float(np.nanmax(q)):.3g}")
    return float(q.max())


def gamma_needed(c, raw):
    """The smallest gamma under which ``raw`` meets the rule on every cell (inf if a cell with a zero frame norm misses RHO alone)."""
    r = reference(c)
    e = np.maximum(np.abs(10.0 ** _raw64(raw) - r.power) - RHO * r.power, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = 2.0 * e / (r.lin + np.sqrt(r.lin ** 2 + 4.0 * r.quad * e))  # root of quad g^2 + lin g = e, in the form that survives quad -> 0
    g = np.where(e == 0.0, 0.0, np.where(np.isfinite(g), g, np.inf))
    return float(g.max())


def finalize_ref(raw, clip_max):
    """whisper's last two lines as the kernels evaluate them: three fp32 operations in torch."""
    return (torch.maximum(raw, clip_max.view(-1, 1, 1) - 8.0) + 4.0) * 0.25


def clip_max_errors(raw, clip_max):
    """Clips whose reported maximum is not bit for bit the maximum of their own live cells."""
    raw = torch.as_tensor(raw)
    return (torch.as_tensor(clip_max) != raw.amax(dim=(1, 2))).nonzero().flatten().tolist()


# ---- whisper's own arithmetic in fp32 (the yardstick gamma_ref is measured on) --------------------------------------------------------
def whisper_fp32(c):
    """raw log10 mel power [B, 80, T] float32: torch.stft in float32 on the CPU with torch.hann_window(400), |.|^2 of all frames but the last,
    the fp32 filterbank matmul, log10 of the clamp -- whisper.audio.log_mel_spectrogram up to (not including) the floor."""
    x = torch.from_numpy(as_float64(c.pcm)).to(torch.float32)
    st = torch.stft(x, NFFT, HOP, window=torch.hann_window(NFFT), return_complex=True)
    mag = st[..., :-1].abs() ** 2
    mel = torch.from_numpy(me.mel_filters()) @ mag
    return torch.clamp(mel, min=1e-10).log10()


# ---- the front end step by step in float64, with one planted mistake at a time --------------------------------------------------------
FLAW_BIN, FLAW_SLOT, FLAW_TAP, FLAW_FILTER = 137, 313, 100, (59, 90)
FLAWS = {  # flaw -> the case that has to kill it
    "bin_scaled_1e-4": "tone_sweep/f32",            # X[137] (1 + 1e-4)
    "bins_k_and_200-k_swapped": "tone_sweep/f32",   # an unpack partner taken for the bin itself
    "sample_slot_zeroed": "impulse_walk/f32",       # slot 313 of every frame
    "window_tap_from_neighbour": "impulse_walk/i16",  # w[101] used for w[100]
    "filter_weight_1e-4": "tone_sweep/f32",         # fb[59, 90] (1 + 1e-4)
    "symmetric_padding": "staging/f32/2x201",       # the edge sample repeated
    "batch_wide_maximum": "floor/f32",
    "dropped_frame_in_maximum": "floor/f32",
    "maximum_of_block_0_only": "floor/f32",
}


def pipeline64(c, flaw=None):
    """(raw [B, 80, T] float32, clip_max [B] float32) from float64 arithmetic -- the front end's definition, stage by stage, stored in the
    kernels' output format."""
    assert flaw is None or flaw in FLAWS, flaw
    x = as_float64(c.pcm)
    fr = frames64(x, "symmetric" if flaw == "symmetric_padding" else "reflect")  # [B, T + 1, 400]
    w = me.hann_window()
    if flaw == "window_tap_from_neighbour":
        w = w.copy()
        w[FLAW_TAP] = w[FLAW_TAP + 1]
    if flaw == "sample_slot_zeroed":
        fr = fr.copy()
        fr[:, :, FLAW_SLOT] = 0.0
    X = np.fft.rfft(fr * w, axis=-1)  # [B, T + 1, 201]
    if flaw == "bin_scaled_1e-4":
        X[..., FLAW_BIN] *= 1.0 + 1e-4
    if flaw == "bins_k_and_200-k_swapped":
        X = X[..., ::-1]
    fb = me.mel_filters().astype(np.float64)
    if flaw == "filter_weight_1e-4":
        assert fb[FLAW_FILTER] > 0.0
        fb[FLAW_FILTER] *= 1.0 + 1e-4
    logp = np.log10(np.maximum(np.einsum("mk,btk->bmt", fb, X.real ** 2 + X.imag ** 2), 1e-10)).astype(np.float32)  # [B, 80, T + 1]
    raw = torch.from_numpy(np.ascontiguousarray(logp[..., :-1]))
    if flaw == "dropped_frame_in_maximum":
        cm = torch.from_numpy(logp).amax(dim=(1, 2))
    elif flaw == "maximum_of_block_0_only":
        cm = raw[..., :QT].amax(dim=(1, 2))
    else:
        cm = raw.amax(dim=(1, 2))
    if flaw == "batch_wide_maximum":
        cm = cm.max().expand_as(cm).clone()
    return raw, cm


# ---- GPU side (imported lazily: everything above runs without a GPU) -----------------------------------------------------------------
def to_gpu(c, device="cuda"):
    """The case's samples on the GPU, ``c.offset`` elements into their allocation."""
    t = torch.from_numpy(np.array(c.pcm))
    if not c.offset:
        return t.to(device)
    buf = torch.zeros(c.offset + t.numel() + 8, dtype=t.dtype, device=device)
    view = buf[c.offset:c.offset + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def gpu_report(families=("tone_sweep", "staging", "floor"), device="cuda"):
    """What the kernel this process runs does with the cases, un-finalised, per family: the worst |err| / bound at GAMMA, the gamma it needs, the
    clips whose clip_max is not their own maximum; and a digest of every raw output (evidence of WHICH kernel ran: the kernels sum in
    different orders).  Asserts nothing: the caller does."""
    import hashlib
    from olmoasr_amd import ops
    worst, need, bad_max, h = {}, {}, {}, hashlib.sha256()
    for fam in families:
        for c in cases(fam):
            raw, cm = ops.log_mel(to_gpu(c, device), finalize=False)
            raw, cm = raw.cpu(), cm.cpu()
            worst[fam] = max(worst.get(fam, 0.0), float(ratios(c, raw).max()))
            need[fam] = max(need.get(fam, 0.0), gamma_needed(c, raw))
            if clip_max_errors(raw, cm):
                bad_max[c.name] = clip_max_errors(raw, cm)
            h.update(raw.numpy().tobytes())
    return {"worst": worst, "gamma_needed": need, "clip_max_errors": bad_max, "digest": h.hexdigest(),
            "cases": sum(len(cases(f)) for f in families)}


if __name__ == "__main__":
    os.environ.setdefault("OASR_TESTING_HOOKS", "1")
    print(json.dumps(dict(gpu_report(), kernel=os.environ.get("OASR_LOGMEL", "quad"))))
