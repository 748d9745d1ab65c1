"""SpecAugment (Park et al. 2019, without time warping) for fine-tuning: seeded frequency / time masks on the finalized log-mel tensor,
applied by one native launch (``ops.spec_augment_``, csrc/specaug.hip) between ``ops.log_mel`` and ``loss_and_backward``.

    policy = augment.SpecAugment.preset("LD")            # 2 x <= 27 mel bins, 2 x <= 100 frames
    mel = ops.log_mel(pcm)                                # finalized: masks live in the (x + 4) / 4 domain, fill 0.0 by default
    policy.apply_(mel, seed, first_clip=stream_id_of_row_0)

A clip's masks are a pure integer function of (seed, clip stream id, policy, shape) -- include/oasr.h states the rule -- so the library's
host twin gives the same plan without a GPU (``plan``, ``masked_cells``), a resumed run draws what the uninterrupted run would have drawn,
and the masks of a clip do not depend on the micro-batch it travels in.

Speed perturbation (Ko et al. 2015; Kaldi's 0.9 / 1.0 / 1.1) works one stage earlier, on the int16 clips ahead of ``ops.log_mel``, and moves
the transcript's timestamp tokens with the audio (``ops.speed_perturb``, csrc/speed.hip):

    speed = augment.SpeedPerturb.preset("3way")          # 9/10, 1/1, 11/10 times faster, one drawn per clip
    pcm, n_out, factor = speed.apply(pcm, n_valid, seed, first_clip=stream_id_of_row_0, tokens=(text_input, text_y))

It is an integer function of the samples, drawn from the same hash stream as the masks (kind 3): ``SpeedPerturb.plan`` gives a clip's ratio,
new length and factor index without a GPU.

Noise mixing adds a recording from a bank at a drawn signal-to-noise ratio, after speed perturbation and ahead of ``ops.log_mel``
(``ops.noise_mix``, csrc/noise.hip):

    bank = augment.noise_bank(recordings, L=480000).to(device)   # int16 [M, L]; shorter recordings are tiled
    noise = augment.NoiseMix(prob=0.5, snr_db=(5, 20))
    pcm, row, snr, gain = noise.apply(pcm, n_out, bank, seed, first_clip=stream_id_of_row_0)

It too is an integer function of the samples (exact energies, an integer Q16 gain, a table of 61 amplitudes), drawn from the same hash
stream (kind 4): ``NoiseMix.plan`` gives a clip's draw without a GPU and without audio.

Reverberation convolves a clip with a room impulse response from a bank, between the two (the far-field recipe: speed, reverb, additive noise;
``ops.reverb``, csrc/reverb.hip):

    bank, delay = augment.rir_bank(responses)                     # float responses -> int16 [R, K] Q15 unit-energy taps, int32 [R]
    reverb = augment.Reverb(prob=0.5)
    pcm, row = reverb.apply(pcm, n_out, bank.to(device), delay.to(device), seed, first_clip=stream_id_of_row_0)

The bank is the only place floating point enters, on the host, once; the convolution is an exact integer sum (on the int8 matrix cores),
shifted back by the direct-path delay and cut at the clip's length, so lengths and timestamps stay.  It draws from the same hash stream
(kind 5): ``Reverb.plan`` gives a clip's draw without a GPU and without audio.

The telephone channel comes last, after the noise -- the channel carries the noise too -- and ahead of ``ops.log_mel`` (``ops.telephone``,
csrc/telephone.hip):

    phone = augment.TelephoneChannel(prob=0.3, codecs=("mulaw", "alaw", "linear"))
    pcm, codec = phone.apply(pcm, n_out, seed, first_clip=stream_id_of_row_0)

A drawn clip is band-passed to 300 - 3400 Hz at 8 kHz, companded by a drawn G.711 codec and interpolated back to 16 kHz, by zero-phase
integer filters: lengths and timestamps stay.  The two tap tables are the only place floating point enters, on the host, once.  It draws
from the same hash stream (kind 6): ``TelephoneChannel.plan`` gives a clip's draw without a GPU and without audio."""
import math
from dataclasses import dataclass

_U64 = (1 << 64) - 1
PRESETS = {"LD": dict(freq_masks=2, freq_width=27, time_masks=2, time_width=100),   # LibriSpeech double
           "LB": dict(freq_masks=1, freq_width=27, time_masks=1, time_width=100)}   # LibriSpeech basic


@dataclass(frozen=True)
class SpecAugment:
    freq_masks: int = 2
    freq_width: int = 27
    time_masks: int = 2
    time_width: int = 100
    time_ratio: float = 1.0  # a time mask is at most floor(time_ratio * T) frames wide (the paper's p; 1.0 = no cap but T itself)
    fill: float = 0.0        # in the finalized domain; what HF's Whisper masks with, near the middle of the (x + 4) / 4 range

    def __post_init__(self):
        from . import ops
        ops.specaug_policy(self.freq_masks, self.freq_width, self.time_masks, self.time_width, self.fill)
        if not (isinstance(self.time_ratio, (int, float)) and 0.0 <= self.time_ratio <= 1.0):
            raise ValueError(f"SpecAugment: time_ratio must lie in [0, 1], got {self.time_ratio!r}")

    @classmethod
    def preset(cls, name, **overrides):
        """The paper's LibriSpeech policies without warping: "LD" (two masks of each kind) or "LB" (one of each)."""
        if name not in PRESETS:
            raise ValueError(f"SpecAugment.preset: unknown policy {name!r}; known: {sorted(PRESETS)}")
        return cls(**{**PRESETS[name], **overrides})

    def time_cap(self, T: int) -> int:
        """The time width handed to the library for clips of T frames: an integer, so that no floating point enters the plan."""
        return min(self.time_width, int(math.floor(self.time_ratio * T)))

    def kwargs(self, T: int) -> dict:
        return dict(freq_masks=self.freq_masks, freq_width=self.freq_width, time_masks=self.time_masks, time_width=self.time_cap(T))

    def apply_(self, mel, seed, first_clip=0):
        """In place on finalized log-mel fp32 [B, n_mels, T] / [n_mels, T] on the GPU; row b takes stream id first_clip + b.  Returns mel."""
        from . import ops
        return ops.spec_augment_(mel, **self.kwargs(int(mel.shape[-1])), fill=self.fill, seed=seed, first_clip=first_clip)


SPEED_PRESETS = {"3way": ((9, 10), (1, 1), (11, 10))}  # Kaldi's speeds 0.9, 1.0, 1.1


@dataclass(frozen=True)
class SpeedPerturb:
    factors: tuple = SPEED_PRESETS["3way"]  # (P, Q) pairs: P / Q times faster; coprime, inside [1, 32], ratio inside [1/2, 2], at most 8
    ts_begin: int = 50363                   # <|0.00|> of the multilingual vocabulary the training script uses
    ts_max: int = 1500                      # <|30.00|> = ts_begin + 1500

    def __post_init__(self):
        from . import ops
        ops.speed_policy(self.factors)
        object.__setattr__(self, "factors", tuple((int(p), int(q)) for p, q in self.factors))

    @classmethod
    def preset(cls, name, **overrides):
        """"3way": each clip at 0.9, 1.0 or 1.1 times its speed, one third of the clips each."""
        if name not in SPEED_PRESETS:
            raise ValueError(f"SpeedPerturb.preset: unknown policy {name!r}; known: {sorted(SPEED_PRESETS)}")
        return cls(**{"factors": SPEED_PRESETS[name], **overrides})

    def apply(self, pcm, n_valid, seed, first_clip=0, tokens=(), out=None):
        """int16 [B, N] on the GPU -> (pcm_out, n_out, factor), out of place; row b takes stream id first_clip + b; the timestamp ids of
        ``tokens`` (up to two int64 [B, S]) move in place."""
        from . import ops
        return ops.speed_perturb(pcm, n_valid, factors=self.factors, seed=seed, first_clip=first_clip, tokens=tokens, ts_begin=self.ts_begin,
                                 ts_max=self.ts_max, out=out)

    def plan(self, seed, clip, n_valid, N):
        """(P, Q, n_out, factor) of stream id ``clip``, from the library's host function: no GPU needed."""
        from . import ops
        return ops.speed_plan(self.factors, seed, clip, n_valid, N)

    def factor_counts(self, seed, first_clip, n_valid, N):
        """Per factor, how many clips of a batch at stream ids first_clip .. take it (host ``n_valid``), from the plan alone: a list of
        len(factors) + 1 integers whose LAST entry counts the clips that fell back to the copy because the slow-down they drew would not
        fit the row -- so the list always sums to the number of clips."""
        counts = [0] * (len(self.factors) + 1)
        for b, nv in enumerate(n_valid):
            counts[self.plan(seed, (first_clip + b) & _U64, int(nv), N)[3]] += 1  # (-1, the fallback, indexes the last entry)
        return counts


@dataclass(frozen=True)
class NoiseMix:
    prob: float = 0.5        # the chance of a clip to take noise (kept in 1 / 65536)
    snr_db: tuple = (5, 20)  # (lo, hi): the SNR is drawn among the whole dB lo .. hi, inside [-10, 50]

    def __post_init__(self):
        from . import ops
        ops.noise_policy(self.prob, self.snr_db)
        object.__setattr__(self, "snr_db", tuple(self.snr_db))

    def apply(self, pcm, n_valid, bank, seed, first_clip=0, out=None):
        """int16 [B, N] on the GPU -> (pcm_out, row, snr, gain); row b takes stream id first_clip + b; ``out=pcm`` mixes in place."""
        from . import ops
        return ops.noise_mix(pcm, n_valid, bank, prob=self.prob, snr_db=self.snr_db, seed=seed, first_clip=first_clip, out=out)

    def plan(self, seed, clip, M, L):
        """(drawn, row, offset, snr_db) of stream id ``clip`` against a bank [M, L], from the library's host function: no GPU needed."""
        from . import ops
        return ops.noise_plan(self.prob, self.snr_db, seed, clip, M, L)

    def drawn(self, seed, first_clip, B, M, L):
        """(how many of the B clips at stream ids first_clip .. are drawn, the sum of their SNRs in dB), from the plan alone.  A drawn clip
        that is silent, empty, or lands on a silent stretch of noise is copied all the same: that takes the audio to know."""
        count = total = 0
        for b in range(B):
            d, _, _, s = self.plan(seed, (first_clip + b) & _U64, M, L)
            if d:
                count, total = count + 1, total + s
        return count, total


@dataclass(frozen=True)
class Reverb:
    prob: float = 0.5  # the chance of a clip to be reverberated (kept in 1 / 65536)

    def __post_init__(self):
        from . import ops
        ops.reverb_policy(self.prob)

    def apply(self, pcm, n_valid, bank, delay, seed, first_clip=0, out=None):
        """int16 [B, N] on the GPU -> (pcm_out, row), out of place; row b takes stream id first_clip + b; ``bank`` int16 [R, K] and ``delay``
        int32 [R] as ``rir_bank`` builds them, on the device of ``pcm``."""
        from . import ops
        return ops.reverb(pcm, n_valid, bank, delay, prob=self.prob, seed=seed, first_clip=first_clip, out=out)

    def plan(self, seed, clip, R):
        """(drawn, row) of stream id ``clip`` against a bank of R responses, from the library's host function: no GPU needed."""
        from . import ops
        return ops.reverb_plan(self.prob, seed, clip, R)

    def drawn(self, seed, first_clip, B, R):
        """How many of the B clips at stream ids first_clip .. are drawn, from the plan alone.  A drawn clip whose length is outside [1, N] is
        copied all the same: that takes the lengths to know."""
        return sum(self.plan(seed, (first_clip + b) & _U64, R)[0] for b in range(B))


TELEPHONE_CODECS = ("linear", "mulaw", "alaw")  # by the library's numbers 0, 1, 2


@dataclass(frozen=True)
class TelephoneChannel:
    prob: float = 0.3                            # the chance of a clip to go through the channel (kept in 1 / 65536)
    codecs: tuple = ("mulaw", "alaw", "linear")  # 1 .. 8 names, one drawn per clip; repeats act as weights
    bandpass: bool = True                        # False: material that is narrow-band already, only decimated and companded

    def __post_init__(self):
        from . import ops
        pol = ops.telephone_policy(self.prob, self.codecs, self.bandpass)
        object.__setattr__(self, "codecs", tuple(TELEPHONE_CODECS[pol.codecs[i]] for i in range(pol.n_codecs)))

    def apply(self, pcm, n_valid, seed, first_clip=0, out=None):
        """int16 [B, N] on the GPU -> (pcm_out, codec), out of place; row b takes stream id first_clip + b."""
        from . import ops
        return ops.telephone(pcm, n_valid, prob=self.prob, codecs=self.codecs, bandpass=self.bandpass, seed=seed, first_clip=first_clip, out=out)

    def plan(self, seed, clip):
        """(drawn, codec name) of stream id ``clip``, from the library's host function: no GPU needed."""
        from . import ops
        d, c = ops.telephone_plan(self.prob, self.codecs, seed, clip, self.bandpass)
        return d, TELEPHONE_CODECS[c]

    def drawn(self, seed, first_clip, B):
        """Per codec, how many of the B clips at stream ids first_clip .. are drawn, from the plan alone: {"linear": .., "mulaw": ..,
        "alaw": ..}.  A drawn clip whose length is outside [1, N] is copied all the same: that takes the lengths to know."""
        counts = {name: 0 for name in TELEPHONE_CODECS}
        for b in range(B):
            d, name = self.plan(seed, (first_clip + b) & _U64)
            counts[name] += int(d)
        return counts


def rir_bank(arrays, K=None):
    """(int16 [R, K] Q15 taps, int32 [R] direct-path delays) on the CPU from a list of 1-D float impulse responses at the clips' sample rate
    (tensors or arrays) -- what ``ops.reverb`` asks of its bank.  Per response: ``delay`` is the index of the largest ``|h|`` (the first of
    equal ones) and must lie below K; the taps are cut or zero-padded to K and scaled in double precision to unit energy,
    ``round(h / sqrt(sum h^2) * 2^15)``, clamped to +-32639.  K defaults to min(8192, the longest response)."""
    import numpy as np
    import torch
    rows = [np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a) for a in arrays]
    if not 1 <= len(rows) <= 65535:
        raise ValueError(f"rir_bank: between 1 and 65535 responses, got {len(rows)}")
    for i, h in enumerate(rows):
        if h.ndim != 1 or h.size < 1 or h.dtype.kind != "f":
            raise ValueError(f"rir_bank: response {i} must be a non-empty 1-D float array, got {h.dtype} {tuple(h.shape)}")
    if K is None:
        K = min(8192, max(int(h.size) for h in rows))
    if not isinstance(K, int) or isinstance(K, bool) or not 1 <= K <= 8192:
        raise ValueError(f"rir_bank: K must be an integer in [1, 8192], got {K!r}")
    bank, delay = np.zeros((len(rows), K), dtype=np.int16), np.zeros(len(rows), dtype=np.int32)
    for i, h in enumerate(rows):
        h = h.astype(np.float64)
        if not np.isfinite(h).all():
            raise ValueError(f"rir_bank: response {i} holds a value that is not finite")
        d = int(np.argmax(np.abs(h)))
        if h[d] == 0.0:
            raise ValueError(f"rir_bank: response {i} is all zero")
        if d >= K:
            raise ValueError(f"rir_bank: response {i} has its direct path at tap {d}, at or behind K = {K}")
        h = h[:K]
        q = np.rint(h / math.sqrt(float(np.sum(h * h))) * 32768.0)
        bank[i, :h.size] = np.clip(q, -32639, 32639).astype(np.int16)
        delay[i] = d
    return torch.from_numpy(bank), torch.from_numpy(delay)


def noise_bank(arrays, L):
    """int16 [M, L] on the CPU from a list of 1-D int16 recordings (tensors or arrays): each is repeated cyclically up to L samples, a longer
    one is cut, so that every row is fully valid -- what ``ops.noise_mix`` asks of its bank."""
    import torch
    if not isinstance(L, int) or isinstance(L, bool) or not 1 <= L <= 1 << 26:
        raise ValueError(f"noise_bank: L must be an integer in [1, 2^26], got {L!r}")
    rows = [torch.as_tensor(a) for a in arrays]
    if not 1 <= len(rows) <= 65535:
        raise ValueError(f"noise_bank: between 1 and 65535 recordings, got {len(rows)}")
    bank = torch.empty(len(rows), L, dtype=torch.int16)
    for i, r in enumerate(rows):
        if r.dtype != torch.int16 or r.dim() != 1 or r.numel() < 1:
            raise ValueError(f"noise_bank: recording {i} must be a non-empty 1-D int16 array, got {r.dtype} {tuple(r.shape)}")
        bank[i] = r.repeat(-(-L // r.numel()))[:L]
    return bank


def plan(policy: SpecAugment, seed: int, clip: int, n_mels: int = 80, T: int = 3000):
    """(frequency masks, time masks) of stream id ``clip``, each a list of (start, width), from the library's host twin: no GPU needed."""
    from . import ops
    return ops.spec_augment_plan(**policy.kwargs(T), seed=seed, clip=clip, n_mels=n_mels, T=T)


def _union(intervals):
    n, end = 0, 0
    for s, w in sorted(intervals):
        n += max(0, s + w - max(s, end))
        end = max(end, s + w)
    return n


def masked_cells(policy: SpecAugment, seed: int, first_clip: int, B: int, n_mels: int, T: int) -> int:
    """How many cells ``apply_`` sets in a batch of B clips at stream ids first_clip .. first_clip + B - 1: per clip the union of its masked
    rows and columns, computed on the host from the plan (no device read-back)."""
    total = 0
    for b in range(B):
        f_iv, t_iv = plan(policy, seed, (first_clip + b) & _U64, n_mels, T)
        rows, cols = _union(f_iv), _union(t_iv)
        total += rows * T + (n_mels - rows) * cols
    return total
