"""Reverberation's rule (include/oasr.h at oasr_reverb) written out again, twice, and the inputs the reverb tests share.  Nothing here is
imported from the package.

``restated`` evaluates the rule in Python integers, tap by sample, exactly as the header writes it (the zero extension and both clamps
spelled out, the floor by ``//``).  ``restated_float64`` takes the same sum through ``np.convolve`` in float64: every product is below 2^30
and every partial sum of at most 8192 of them below 2^44 < 2^53, so the float64 result is exact -- a second oracle that shares no loop with
the first.  Both return ``(pcm_out [B][N] lists of int, row_out [B])``."""
import numpy as np

M64 = (1 << 64) - 1
TAP_MAX = 32639
KIND = 5


def mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def plan(seed, clip, prob_q16, R, kind=KIND):
    h, t = mix(mix(seed) ^ clip), kind << 16
    return mix(h ^ t) % 65536 < prob_q16, mix(h ^ (t | 1)) % R


def clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def _wet_rows(x, nv, bank, prob_q16, seed, first):
    B, N = len(x), len(x[0])
    for b in range(B):
        drawn, r = plan(seed, (first + b) & M64, prob_q16, len(bank))
        yield b, r, drawn and 1 <= nv[b] <= N


def restated(x, nv, bank, delay, prob_q16, seed, first):
    """Python integers only.  x [B][N], bank [R][K], nv [B], delay [R]: lists (or arrays) of ints."""
    x, bank = [[int(v) for v in r] for r in x], [[int(v) for v in r] for r in bank]
    K = len(bank[0])
    out, rows = [], []
    for b, r, wet in _wet_rows(x, nv, bank, prob_q16, seed, first):
        rows.append(r if wet else -1)
        if not wet:
            out.append(list(x[b]))
            continue
        taps, d, n_valid = [clamp(t, -TAP_MAX, TAP_MAX) for t in bank[r]], clamp(int(delay[r]), 0, K - 1), int(nv[b])
        y = list(x[b])
        for n in range(n_valid):
            S = sum(taps[k] * (x[b][n + d - k] if 0 <= n + d - k < n_valid else 0) for k in range(K))
            y[n] = clamp((S + (1 << 14)) // (1 << 15), -32768, 32767)  # (// floors, as the arithmetic shift does)
        out.append(y)
    return out, rows


def restated_float64(x, nv, bank, delay, prob_q16, seed, first):
    """The same numbers through np.convolve in float64 (exact here: see the module's docstring)."""
    x, bank = np.asarray(x, dtype=np.int64), np.asarray(bank, dtype=np.int64)
    K = bank.shape[1]
    out, rows = [], []
    for b, r, wet in _wet_rows(x, nv, bank, prob_q16, seed, first):
        rows.append(r if wet else -1)
        y = x[b].copy()
        if wet:
            taps, d, n_valid = np.clip(bank[r], -TAP_MAX, TAP_MAX).astype(np.float64), clamp(int(delay[r]), 0, K - 1), int(nv[b])
            full = np.convolve(taps, x[b, :n_valid].astype(np.float64))  # full[m] = sum_k tap(k) x(m - k), m < n_valid + K - 1
            S = full[d:d + n_valid]
            assert np.abs(S).max(initial=0.0) < 2.0 ** 44
            y[:n_valid] = np.clip(np.floor((S + 16384.0) / 32768.0), -32768, 32767).astype(np.int64)  # (a power-of-two divisor: exact)
        out.append(y.tolist())
    return out, rows


def clips(B, N, seed, amp=12000):
    rng = np.random.default_rng(seed)
    return rng.integers(-amp, amp + 1, size=(B, N)).astype(np.int16)


def responses(R, length, seed, pre=7):
    """R seeded synthetic room responses as float64 arrays: a direct path of 1.0 after ``pre + i`` samples of weak precursor, then
    exponentially decaying noise (a reverberation time of about a third of the length)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(R):
        d = min(pre + i, length - 1)
        h = rng.standard_normal(length) * 0.2 * np.exp(-np.arange(length) / max(1.0, length / 3.0))
        h[:d] *= 0.05
        h[d] = 1.0
        out.append(h)
    return out


def quantized_bank(R, K, seed, pre=7):
    """int16 [R, K] Q15 unit-energy taps and int32 [R] delays of ``responses``, by the rule of ``augment.rir_bank`` written out again."""
    hs = responses(R, K, seed, pre)
    bank = np.stack([np.clip(np.rint(h / np.sqrt(np.sum(h * h)) * 32768.0), -TAP_MAX, TAP_MAX) for h in hs]).astype(np.int16)
    return bank, np.array([int(np.argmax(np.abs(h))) for h in hs], dtype=np.int32)


def ramp(N, start=-9000, step=37):
    """An asymmetric ramp that crosses every low byte and many high bytes and never repeats a window: under it a swapped operand map, a
    mirrored tap index or a wrong block gives another number."""
    v = (start + step * np.arange(N, dtype=np.int64) + (np.arange(N, dtype=np.int64) ** 2) // 97)
    return ((v + 32768) % 65536 - 32768).astype(np.int16)


def planted(K, k, value):
    """One response of K taps, all zero but ``value`` at tap k."""
    taps = np.zeros((1, K), dtype=np.int16)
    taps[0, k] = value
    return taps
