"""The telephone channel's rule (include/oasr.h at oasr_telephone) written out again in Python integers, and the inputs the telephone tests
share.  Nothing here is imported from the package.

``tables`` builds h and u from their formulas (``math``, double precision, as the header says the host does); ``restated`` evaluates the
rule tap by sample exactly as the header writes it (the zero extension spelled out, the floor by ``//``, the quantisers in closed form with
``int.bit_length`` for the logarithm).  It returns ``(pcm_out [B][N] lists of int, codec_out [B])``."""
import math

import numpy as np

M64 = (1 << 64) - 1
KIND = 6
LINEAR, MULAW, ALAW = 0, 1, 2
SEEDS = ((0, 0), (7, 3), (2 ** 63 + 5, 2 ** 40))
SUM_ABS_H, SUM_ABS_U = 76960, 81604  # as the header states them


def mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def plan(seed, clip, prob_q16, codecs):
    """(drawn, codec) of stream id ``clip``."""
    h, t = mix(mix(seed) ^ clip), KIND << 16
    return mix(h ^ t) % 65536 < prob_q16, codecs[mix(h ^ (t | 1)) % len(codecs)]


def sinc(t):
    return 1.0 if t == 0 else math.sin(math.pi * t) / (math.pi * t)


def tables():
    """(h as a list of 129 with h[k + 64], u as a list of 32)."""
    def lp(f, k):
        return (2 * f / 16000) * sinc(2 * f * k / 16000)
    h = [math.floor((lp(3400, k) - lp(300, k)) * (0.5 + 0.5 * math.cos(math.pi * k / 65)) * 32768 + 0.5) for k in range(-64, 65)]
    u = []
    for j in range(32):
        t = (j - 15) - 0.5
        u.append(math.floor(sinc(t) * (0.5 + 0.5 * math.cos(math.pi * t / 16)) * 32768 + 0.5))
    u[u.index(max(u))] += 32768 - sum(u)  # (index: the first of equal maxima)
    return h, u


H, U = tables()


def round_q15(S):
    return min(32767, max(-32768, (S + (1 << 14)) // (1 << 15)))  # (// floors, as the arithmetic shift does)


def mulaw(x):
    s = x < 0
    a = min(-x if s else x, 32635) + 132
    e = (a.bit_length() - 1) - 7
    m = (a >> (e + 3)) & 15
    y = (((m << 3) + 132) << e) - 132
    return -y if s else y


def alaw(x):
    s = x < 0
    a = -x - 1 if s else x
    v = a >> 3
    g = 0 if v < 32 else (v.bit_length() - 1) - 4
    m = (v >> 1) & 15 if g < 2 else (v >> g) & 15
    y = (m << 4) + 8 if g == 0 else ((m << 4) + 264) << (g - 1)
    return -y if s else y


def quantize(x, codec):
    return mulaw(x) if codec == MULAW else alaw(x) if codec == ALAW else x


def channel(x, n_valid, codec, bandpass):
    """One row through the channel: a new list."""
    x = [int(v) for v in x]

    def xs(i):
        return x[i] if 0 <= i < n_valid else 0
    M = (n_valid + 1) // 2
    if bandpass:
        z = [round_q15(sum(H[k + 64] * xs(2 * m - k) for k in range(-64, 65))) for m in range(M)]
    else:
        z = [xs(2 * m) for m in range(M)]
    c = [quantize(v, codec) for v in z]
    y = list(x)
    for m in range(M):
        y[2 * m] = c[m]
        if 2 * m + 1 < n_valid:
            y[2 * m + 1] = round_q15(sum(U[j] * c[m + j - 15] for j in range(32) if 0 <= m + j - 15 < M))
    return y


def restated(x, nv, prob_q16, codecs, bandpass, seed, first):
    """Python integers only.  x [B][N], nv [B]: lists (or arrays) of ints; codecs: a list of the numbers 0, 1, 2."""
    out, reports = [], []
    for b, row in enumerate(x):
        drawn, codec = plan(seed, (first + b) & M64, prob_q16, codecs)
        n = int(nv[b])
        if drawn and 1 <= n <= len(row):
            out.append(channel(row, n, codec, bandpass)), reports.append(codec)
        else:
            out.append([int(v) for v in row]), reports.append(-1)
    return out, reports


def clips(B, N, seed, amp=12000):
    rng = np.random.default_rng(seed)
    return rng.integers(-amp, amp + 1, size=(B, N)).astype(np.int16)


def wrap_row_bandpass(N, p):
    """A row on which the band-pass's sum at the even sample p is sum |h| * 2^15 or so, above 2^31: x[p - k] = 32767 where h[k] >= 0, else
    -32768.  The rule gives y[p] = 32767 (linear codec); a wrapped 32-bit accumulator gives a negative sample."""
    assert p % 2 == 0 and p - 64 >= 0 and p + 64 < N
    x = np.zeros(N, dtype=np.int16)
    for k in range(-64, 65):
        x[p - k] = 32767 if H[k + 64] >= 0 else -32768
    assert sum(H[k + 64] * int(x[p - k]) for k in range(-64, 65)) > 1 << 31
    return x


def wrap_row_interpolator(N, m):
    """The same over u, on the even samples around the odd sample 2 m + 1, for ``bandpass=False`` and the linear codec: c[m + j - 15] =
    32767 where u[j] >= 0, else -32768.  The rule gives y[2 m + 1] = 32767."""
    assert m - 15 >= 0 and 2 * (m + 16) < N
    x = np.zeros(N, dtype=np.int16)
    for j in range(32):
        x[2 * (m + j - 15)] = 32767 if U[j] >= 0 else -32768
    assert sum(U[j] * int(x[2 * (m + j - 15)]) for j in range(32)) > 1 << 31
    return x


def sine(freq, n=8000, amp=10000, phase=0.0):
    return np.round(amp * np.sin(2 * np.pi * freq * np.arange(n) / 16000.0 + phase)).astype(np.int16)


def db(num, den):
    """10 log10 of the ratio of two energies."""
    return 10 * math.log10(max(float(num), 1e-30) / float(den))
