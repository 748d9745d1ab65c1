"""SpecAugment (Park et al. 2019, without time warping) for fine-tuning: seeded frequency / time masks on the finalized log-mel tensor,
applied by one native launch (``ops.spec_augment_``, csrc/specaug.hip) between ``ops.log_mel`` and ``loss_and_backward``.

    policy = augment.SpecAugment.preset("LD")            # 2 x <= 27 mel bins, 2 x <= 100 frames
    mel = ops.log_mel(pcm)                                # finalized: masks live in the (x + 4) / 4 domain, fill 0.0 by default
    policy.apply_(mel, seed, first_clip=stream_id_of_row_0)

A clip's masks are a pure integer function of (seed, clip stream id, policy, shape) -- include/oasr.h states the rule -- so the library's
host twin gives the same plan without a GPU (``plan``, ``masked_cells``), a resumed run draws what the uninterrupted run would have drawn,
and the masks of a clip do not depend on the micro-batch it travels in."""
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
