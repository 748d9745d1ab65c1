"""CPU half of noise mixing (csrc/noise_core.h through its host twin: oasr_noise_mix_host, oasr_noise_plan): the mixer against the rule of
include/oasr.h written out again here in Python integers (math.isqrt, arbitrary-precision sums), the seeded draws, the 61 amplitudes against
their formula, known answers, the extremes of the gain, a quality guard on the achieved SNR, the argument checks that fire before anything
is written, the binding's struct sizes, ``augment.noise_bank`` and the training script's flags."""
import ctypes
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    from olmoasr_amd import _native
    if not os.path.isfile(_native.LIB_PATH):
        g.build()
    _native.lib()
    return _native


@pytest.fixture(scope="module")
def ops(native):
    from olmoasr_amd import ops
    return ops


@pytest.fixture(scope="module")
def tt():
    spec = importlib.util.spec_from_file_location("tt_noise_cpu", os.path.join(ROOT, "scripts", "training", "train_timestamps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the rule, from the text of include/oasr.h; nothing below is imported from the package --------------------------------------
def mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


A = [math.floor(10 ** (-s / 20) * 32768 + 0.5) for s in range(-10, 51)]


def plan(seed, clip, prob_q16, lo, hi, M, L):
    h, t = mix(mix(seed) ^ clip), 4 << 16
    return (mix(h ^ t) % 65536 < prob_q16, mix(h ^ (t | 1)) % M, mix(h ^ (t | 2)) % L, lo + mix(h ^ (t | 3)) % (hi - lo + 1))


def gain(Ex, Ev, s):
    """The Q16 gain, or None where the clip is not mixed."""
    sh = max(0, (Ex | Ev).bit_length() - 31)
    ex, ev = Ex >> sh, Ev >> sh
    if ex == 0 or ev == 0:
        return None
    g0 = math.isqrt((ex << 32) // ev)
    assert g0 < 2 ** 31.5
    g = (g0 * A[s + 10] + (1 << 14)) >> 15
    assert g < 1 << 34
    return g


def restated(x, nv, bank, prob, snr_db, seed, first):
    """(pcm, row, snr, gain) as lists of Python integers."""
    (B, N), (M, L) = x.shape, bank.shape
    X, V = x.tolist(), bank.tolist()
    out, rows, snrs, gains = [], [], [], []
    for b in range(B):
        drawn, m, o, s = plan(seed, (first + b) & M64, int(round(prob * 65536)), snr_db[0], snr_db[1], M, L)
        xs, n, g = X[b], int(nv[b]), None
        if drawn and 1 <= n <= N:
            v = [V[m][(o + i) % L] for i in range(n)]
            g = gain(sum(a * a for a in xs[:n]), sum(a * a for a in v), s)
        if g is None:
            out.append(list(xs)), rows.append(-1), snrs.append(-128), gains.append(0)
            continue
        assert all(abs(a * g) < 1 << 49 for a in v)
        y = [min(32767, max(-32768, xs[i] + ((v[i] * g + (1 << 15)) >> 16))) for i in range(n)] + xs[n:]
        out.append(y), rows.append(m), snrs.append(s), gains.append(g)
    return out, rows, snrs, gains


def i32(v):
    return torch.tensor(v, dtype=torch.int32)


def clips(B, N, seed, amp=3000):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-amp, amp + 1, (B, N), generator=g, dtype=torch.int64).to(torch.int16)


def assert_twin(ops, x, nv, bank, prob, snr_db, seed, first):
    got = ops.noise_mix_host(x, nv, bank, prob=prob, snr_db=snr_db, seed=seed, first_clip=first)
    want = restated(x, nv.tolist(), bank, prob, snr_db, seed, first)
    assert got[0].dtype == torch.int16 and got[1].dtype == torch.int32 and got[2].dtype == torch.int32 and got[3].dtype == torch.int64
    for name, g, w in zip(("pcm", "row", "snr", "gain"), got, want):
        assert g.tolist() == w, f"{name} differs from the restatement"
    return got


# ---- the mixer ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4096, 4099])
@pytest.mark.parametrize("L", [1000, 4099, 9000], ids=["L1000_wraps", "L4099", "L9000"])
def test_host_twin_equals_the_restatement(ops, N, L):
    B, M = 5, 3
    x = clips(B, N, 100 + N)
    x[0, :N // 2], x[0, N // 2:] = 32767, -32768  # a row that saturates
    bank = torch.zeros(M, L + 3, dtype=torch.int16)[:, :L]  # (a row stride above L)
    bank.copy_(clips(M, L, 7 + L, amp=20000))
    nv = i32([0, 1, 37, N - 1, N])
    mixed = set()
    for seed, first in ((0, 0), (7, 3), (2 ** 63 + 5, 2 ** 40)):
        got = assert_twin(ops, x, nv, bank, 0.75, (-10, 50), seed, first)
        mixed |= set(r >= 0 for r in got[1].tolist())
    assert mixed == {True, False}
    assert_twin(ops, x.flip(0), i32([N, N, N, N, N]), bank, 1.0, (5, 20), 11, M64 - 1)  # (stream ids wrap mod 2^64)


def test_in_place_equals_out_of_place(ops):
    N = 4099
    x, bank, nv = clips(4, N, 5), clips(2, 1000, 6), i32([N, 0, 2000, 37])
    want = ops.noise_mix_host(x, nv, bank, prob=0.75, snr_db=(0, 30), seed=3, first_clip=1)
    y = x.clone()
    got = ops.noise_mix_host(y, nv, bank, prob=0.75, snr_db=(0, 30), seed=3, first_clip=1, out=y)
    assert got[0].data_ptr() == y.data_ptr() and all(torch.equal(g, w) for g, w in zip(got, want))
    assert {r >= 0 for r in want[1].tolist()} == {True, False}


def test_plan_is_the_stated_hash(ops):
    from olmoasr_amd import augment
    seen = set()
    for seed in (0, 7, 2 ** 63 + 5):
        for first in (0, 2 ** 40):
            for b in range(24):
                for prob, lo, hi, M, L in ((0.5, 5, 20, 3, 1000), (1.0, -10, 50, 65535, 1 << 26), (0.0, 0, 0, 1, 1), (0.25, 50, 50, 7, 480000)):
                    want = plan(seed, first + b, int(round(prob * 65536)), lo, hi, M, L)
                    assert ops.noise_plan(prob, (lo, hi), seed, first + b, M, L) == want
                    assert augment.NoiseMix(prob=prob, snr_db=(lo, hi)).plan(seed, first + b, M, L) == want
                    assert 0 <= want[1] < M and 0 <= want[2] < L and lo <= want[3] <= hi
                    if prob == 0.5:
                        seen.add(want[0])
    assert seen == {True, False}
    pol = augment.NoiseMix(prob=0.5, snr_db=(5, 20))
    draws = [plan(9, (M64 - 3 + b) & M64, 32768, 5, 20, 4, 999) for b in range(8)]
    assert pol.drawn(9, M64 - 3, 8, 4, 999) == (sum(d[0] for d in draws), sum(d[3] for d in draws if d[0]))


def test_the_61_amplitudes_match_the_formula(ops):
    """Equal energies give g0 = 2^16 exactly, hence g = 2 A[s + 10]: the library's table, read through the gain it reports."""
    x, bank, nv = torch.full((1, 16), 100, dtype=torch.int16), torch.full((1, 5), -100, dtype=torch.int16), i32([16])
    table = []
    for s in range(-10, 51):
        g = int(ops.noise_mix_host(x, nv, bank, prob=1.0, snr_db=(s, s))[3][0])
        assert g % 2 == 0
        table.append(g // 2)
    assert table == A and (A[0], A[10], A[60]) == (103622, 32768, 104) and len(A) == 61
    for s, a in zip(range(-10, 51), table):  # a = round(10^(-s/20) 2^15) in exact integers: (2a - 1)^20 <= 2^320 10^-s < (2a + 1)^20
        lo, hi, mid = (2 * a - 1) ** 20 * 10 ** max(s, 0), (2 * a + 1) ** 20 * 10 ** max(s, 0), 2 ** 320 * 10 ** max(-s, 0)
        assert lo <= mid < hi, s


def seed_with(ops, L, offset=0, M=1):
    """A seed under which clip 0 is laid at ``offset`` of bank row 0 (from the restated plan)."""
    return next(s for s in range(100000) if plan(s, 0, 65536, 0, 0, M, L)[1:3] == (0, offset))


def test_known_answers(ops):
    N = 64
    x = clips(1, N, 1, amp=30000)
    seed = seed_with(ops, N)
    # the clip against itself at 0 dB: g = 2^16 and y = clamp(2 x)
    y, row, snr, g = ops.noise_mix_host(x, i32([N]), x.clone(), prob=1.0, snr_db=(0, 0), seed=seed)
    assert (row.tolist(), snr.tolist(), g.tolist()) == ([0], [0], [65536])
    assert torch.equal(y, (2 * x.long()).clamp(-32768, 32767).to(torch.int16)) and bool((y.abs() == 32767).any() or (y == -32768).any())
    # ... of which only the first 10 samples are valid: the rest is copied
    y = ops.noise_mix_host(x, i32([10]), x.clone(), prob=1.0, snr_db=(0, 0), seed=seed)[0]
    assert torch.equal(y[:, :10], (2 * x[:, :10].long()).clamp(-32768, 32767).to(torch.int16)) and torch.equal(y[:, 10:], x[:, 10:])
    none = ([-1], [-128], [0])
    bank = clips(1, N, 2)
    for xs, vs, nv in ((torch.zeros_like(x), bank, N), (x, torch.zeros_like(bank), N), (x, bank, 0)):  # silent clip, silent bank row, empty clip
        y, row, snr, g = ops.noise_mix_host(xs, i32([nv]), vs, prob=1.0, snr_db=(0, 0), seed=seed)
        assert torch.equal(y, xs) and (row.tolist(), snr.tolist(), g.tolist()) == none
    # a clip whose valid part is silent is copied although the padding is not
    xs = x.clone()
    xs[:, :10] = 0
    y, row, _, _ = ops.noise_mix_host(xs, i32([10]), bank, prob=1.0, snr_db=(0, 0), seed=seed)
    assert torch.equal(y, xs) and row.tolist() == [-1]


def test_extremes_of_the_gain(ops):
    """v = +-1 under a full-scale clip at -10 dB is the largest gain the rule meets (2^31 * 103622 >> 15, below 2^34) and still fits; noise
    whose energy vanishes at the common scale is not mixed.  (Ex = 2^56 - 1 against Ev = 1 itself takes 2^26 samples: the restatement and
    the stand-alone host check hold it on the gain function; here the same branch is taken by 2^42 against 1.)"""
    N = 4096
    x = torch.full((1, N), -32768, dtype=torch.int16)
    pm = torch.ones(1, N, dtype=torch.int16)
    pm[0, ::3] = -1
    got = assert_twin(ops, x, i32([N]), pm, 1.0, (-10, -10), 0, 0)
    assert got[3].tolist() == [(2 ** 31 * 103622 + (1 << 14)) >> 15] and got[3].tolist()[0] < 1 << 34
    assert set(got[0].unique().tolist()) == {-32768, 32767}
    one = torch.zeros(1, N, dtype=torch.int16)
    one[0, 5] = 1
    got = assert_twin(ops, x, i32([N]), one, 1.0, (-10, -10), 0, 0)
    assert got[1].tolist() == [-1] and torch.equal(got[0], x)
    assert gain((1 << 56) - 1, 1, -10) is None and gain(1, (1 << 56) - 1, 50) is None and gain(1 << 56, 1 << 26, -10) == 65536 * 103622
    got = assert_twin(ops, one, i32([N]), x, 1.0, (50, 50), 0, 0)  # ... and the other way round
    assert got[1].tolist() == [-1]


@pytest.mark.parametrize("s", [-10, -3, 0, 5, 13, 20, 27])
def test_quality_guard_on_the_achieved_snr(ops, s):
    """Unsaturated, scaled noise of at least 50 LSB rms: the achieved 10 log10(Ex / sum (y - x)^2) is within 0.05 dB of the drawn SNR (the
    restatement alone stays within 0.02 dB on such cases: the gain's rounding, and one rounding of at most 1/2 LSB per sample)."""
    N = 6000
    g = torch.Generator().manual_seed(50 + s)
    x = (torch.randn(2, N, generator=g) * 1500).round().clamp(-32768, 32767).to(torch.int16)
    bank = (torch.randn(3, 2500, generator=g) * torch.tensor([[30.0], [700.0], [6000.0]])).round().clamp(-32768, 32767).to(torch.int16)
    nv = [N, 4321]
    y, row, snr, _ = ops.noise_mix_host(x, i32(nv), bank, prob=1.0, snr_db=(s, s), seed=s + 10)
    for b in range(2):
        assert int(row[b]) >= 0 and int(snr[b]) == s
        xs, d = x[b, :nv[b]].double(), (y[b, :nv[b]].long() - x[b, :nv[b]].long()).double()
        assert int(y[b].abs().max()) < 32767, "the planted case saturated"
        rms = math.sqrt(float((d * d).sum()) / nv[b])
        assert rms >= 50, "the planted case is too quiet to be judged"
        achieved = 10 * math.log10(float((xs * xs).sum()) / float((d * d).sum()))
        print(f"s = {s} dB, row {b}: achieved {achieved:.4f} dB, noise rms {rms:.1f} LSB")
        assert abs(achieved - s) <= 0.05


def test_probability_ends(ops):
    B, N = 32, 256
    x, bank, nv = clips(B, N, 3), clips(2, 100, 4), i32([N] * B)
    y, row, snr, g = ops.noise_mix_host(x, nv, bank, prob=0.0, snr_db=(5, 20))
    assert torch.equal(y, x) and row.tolist() == [-1] * B and snr.tolist() == [-128] * B and g.tolist() == [0] * B
    y, row, snr, g = ops.noise_mix_host(x, nv, bank, prob=1.0, snr_db=(5, 20))
    assert all(r >= 0 for r in row.tolist()) and all(5 <= s <= 20 for s in snr.tolist()) and len(set(snr.tolist())) > 4
    assert not any(torch.equal(y[b], x[b]) for b in range(B))


# ---- refusals, sizes --------------------------------------------------------------------------------------------------------------------
def test_refusals(native, ops):
    lib = native.lib()
    N, L = 64, 32
    x, y = torch.full((2, N), 3, dtype=torch.int16), torch.full((2, N), 5, dtype=torch.int16)
    bank, nv = torch.full((2, L), 7, dtype=torch.int16), i32([N, 10])
    row, snr, g = i32([99, 99]), i32([99, 99]), torch.tensor([99, 99])

    def block(**kw):
        a = native.NoiseArgs()
        a.pcm_in, a.pcm_out, a.n_valid, a.bank = x.data_ptr(), y.data_ptr(), nv.data_ptr(), bank.data_ptr()
        a.row_out, a.snr_out, a.gain_out = row.data_ptr(), snr.data_ptr(), g.data_ptr()
        a.ld_in = a.ld_out = N
        a.ld_bank, a.B, a.N, a.M, a.L = L, 2, N, 2, L
        a.policy = native.Noise(65536, 5, 20)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(a, what):
        return lib.oasr_noise_mix_host(ctypes.byref(a)) == -1 and what in lib.oasr_last_error().decode()  # OASR_EINVAL

    both = torch.full((2, N + 32), 3, dtype=torch.int16)
    cases = [(dict(B=0), "B outside"), (dict(B=65536), "B outside"), (dict(N=0), "N outside"), (dict(N=(1 << 26) + 1, ld_in=1 << 27, ld_out=1 << 27), "N outside"),
             (dict(M=0), "M outside"), (dict(M=65536), "M outside"), (dict(L=0), "L outside"), (dict(L=(1 << 26) + 1, ld_bank=1 << 27), "L outside"),
             (dict(ld_in=N - 1), "stride"), (dict(ld_out=N - 1), "stride"), (dict(ld_bank=L - 1), "stride"),
             (dict(pcm_in=x.data_ptr() + 1), "2-byte"), (dict(pcm_out=y.data_ptr() + 1), "2-byte"), (dict(bank=bank.data_ptr() + 1), "2-byte"),
             (dict(row_out=row.data_ptr() + 2), "4-byte"), (dict(snr_out=snr.data_ptr() + 2), "4-byte"), (dict(gain_out=g.data_ptr() + 4), "8-byte"),
             (dict(pcm_in=None), "null"), (dict(pcm_out=None), "null"), (dict(n_valid=None), "null"), (dict(bank=None), "null"),
             (dict(pcm_in=both.data_ptr(), pcm_out=both[:, 32:].data_ptr(), ld_in=N + 32, ld_out=N + 32), "overlap"),  # partial overlap
             (dict(pcm_in=y.data_ptr(), ld_in=N + 1, B=1), "overlap"),                                               # the same buffer, another stride
             (dict(bank=y.data_ptr()), "bank and pcm_out"),
             (dict(policy=native.Noise(-1, 5, 20)), "prob_q16"), (dict(policy=native.Noise(65537, 5, 20)), "prob_q16"),
             (dict(policy=native.Noise(100, -11, 20)), "[-10, 50]"), (dict(policy=native.Noise(100, 5, 51)), "[-10, 50]"),
             (dict(policy=native.Noise(100, 21, 20)), "above")]
    for kw, what in cases:
        assert refused(block(**kw), what), (kw, lib.oasr_last_error().decode())
    assert lib.oasr_noise_mix_host(None) == -1
    out = [ctypes.c_int(-5) for _ in range(4)]
    for pol, M, L_ in ((native.Noise(65537, 5, 20), 1, 1), (native.Noise(1, 5, 20), 0, 1), (native.Noise(1, 5, 20), 1, 0), (native.Noise(1, 5, 20), 65536, 1),
                       (native.Noise(1, 5, 20), 1, (1 << 26) + 1), (native.Noise(1, 20, 5), 1, 1)):
        assert lib.oasr_noise_plan(ctypes.byref(pol), 0, 0, M, L_, *[ctypes.byref(o) for o in out]) == -1
    assert [o.value for o in out] == [-5] * 4
    assert bool((y == 5).all()) and bool((x == 3).all()) and bool((both == 3).all()) and row.tolist() == snr.tolist() == g.tolist() == [99, 99]
    assert lib.oasr_noise_mix_host(ctypes.byref(block())) == 0  # the block they were derived from is fine
    assert lib.oasr_noise_mix_host(ctypes.byref(block(pcm_in=y.data_ptr()))) == 0  # ... and so is in place
    y.fill_(5)
    # the Python surface: policy, dtypes, shapes, overlap
    for kw in (dict(prob=-0.1), dict(prob=1.5), dict(prob=float("nan")), dict(prob="1"), dict(prob=True), dict(snr_db=(-11, 0)), dict(snr_db=(0, 51)), dict(snr_db=(20, 5)),
               dict(snr_db=(5.0, 20)), dict(snr_db=5), dict(snr_db=(5, 10, 20)), dict(pcm=x.float()), dict(pcm=x[0]), dict(pcm=x.t()), dict(n_valid=nv.long()),
               dict(n_valid=nv[:1]), dict(bank=bank.float()), dict(bank=bank[0]), dict(bank=bank[:0]), dict(bank=bank[:, :0]), dict(bank=bank.t()),
               dict(out=torch.zeros(2, N)), dict(out=torch.zeros(2, N + 1, dtype=torch.int16)), dict(out=both[:, 1:N + 1], pcm=both[:, :N]), dict(out=bank.expand(2, L), pcm=x[:, :L]),
               dict(seed=-1), dict(first_clip=2 ** 64)):
        args = dict(pcm=x, n_valid=nv, bank=bank, prob=0.5, snr_db=(5, 20), out=y)
        args.update(kw)
        pcm, n_valid, bk = args.pop("pcm"), args.pop("n_valid"), args.pop("bank")
        with pytest.raises(ValueError):
            ops.noise_mix_host(pcm, n_valid, bk, **args)
    for bad in (dict(M=0), dict(M=65536), dict(L=0), dict(L=(1 << 26) + 1), dict(M=1.0), dict(seed=-1), dict(clip=2 ** 64), dict(prob=2.0), dict(snr_db=(0, 99))):
        args = dict(prob=0.5, snr_db=(5, 20), seed=0, clip=0, M=2, L=L)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.noise_plan(**args)
    with pytest.raises(ValueError, match="GPU"):
        ops.noise_mix(x, nv, bank, prob=0.5, snr_db=(5, 20))  # the device entry takes no CPU tensor, and says so before a launch
    from olmoasr_amd import augment
    for bad in (dict(prob=1.01), dict(snr_db=(5, 51)), dict(snr_db=(6, 5))):
        with pytest.raises(ValueError):
            augment.NoiseMix(**bad)
    assert bool((y == 5).all()) and bool((x == 3).all())
    empty = ops.noise_mix_host(x[:0], nv[:0], bank, prob=0.5, snr_db=(5, 20))  # B = 0: nothing to do, not an error
    assert tuple(empty[0].shape) == (0, N) and all(t.numel() == 0 for t in empty[1:])


def test_struct_sizes_and_version(native):
    lib = native.lib()
    assert lib.oasr_version() == 216 == native.ABI_VERSION
    assert lib.oasr_sizeof_noise() == ctypes.sizeof(native.Noise) == 12
    assert lib.oasr_sizeof_noise_args() == ctypes.sizeof(native.NoiseArgs)
    assert ("oasr_sizeof_noise", native.Noise) in native.STRUCT_SIZES and ("oasr_sizeof_noise_args", native.NoiseArgs) in native.STRUCT_SIZES
    assert native.Noise.NONE == -128
    for B, N in ((1, 1), (5, 4099), (128, 480000)):  # two u64 per 2048-sample tile of a row that may start anywhere on the 16-byte grid
        assert lib.oasr_noise_workspace_bytes(B, N) == B * ((N + 7 + 2047) // 2048) * 16
    assert lib.oasr_noise_workspace_bytes(0, 5) == 0


# ---- the bank, the training script ------------------------------------------------------------------------------------------------------
def test_noise_bank_tiles_cyclically():
    from olmoasr_amd import augment
    a, b, c = np.arange(1, 4, dtype=np.int16), torch.arange(10, 22, dtype=torch.int16), np.array([-5], dtype=np.int16)
    bank = augment.noise_bank([a, b, c], 8)
    assert bank.dtype == torch.int16 and bank.tolist() == [[1, 2, 3, 1, 2, 3, 1, 2], list(range(10, 18)), [-5] * 8]
    assert augment.noise_bank([a], 3).tolist() == [[1, 2, 3]]
    for bad in (([], 8), ([a.astype(np.int32)], 8), ([a.reshape(1, 3)], 8), ([a[:0]], 8), ([a], 0), ([a], (1 << 26) + 1), ([a], 8.0)):
        with pytest.raises(ValueError):
            augment.noise_bank(*bad)


def test_cli_flags(tt, native, tmp_path):
    off = tt.parse_args([])
    assert off.noise_bank is None and off.noise_prob is None and off.noise_snr_db is None and off.noise_policy is None
    assert all(f in tt.NATIVE_FLAGS for f in ("noise_bank", "noise_prob", "noise_snr_db"))
    for flag in ("--noise_prob=0.5", "--noise_snr_db=5,20"):
        with pytest.raises(SystemExit, match=flag[:flag.index("=")] + " given without --noise_bank"):
            tt.parse_args([flag])
    with pytest.raises(SystemExit, match="--noise_bank"):
        tt.parse_args([f"--noise_bank={tmp_path}/missing.npy"])
    grid = tmp_path / "grid.npy"
    np.save(grid, np.arange(24, dtype=np.int16).reshape(3, 8))
    on = tt.parse_args([f"--noise_bank={grid}"])
    assert (on.noise_policy.prob, on.noise_policy.snr_db) == (0.5, (5, 20))
    rest = {k: v for k, v in on.items() if k not in ("noise_bank", "noise_policy")}
    assert rest == {k: v for k, v in off.items() if k not in ("noise_bank", "noise_policy")}  # nothing else moves
    p = tt.parse_args(["--noise_bank", str(grid), "--noise_prob", "1.0", "--noise_snr_db", "-3,12"]).noise_policy
    assert (p.prob, p.snr_db) == (1.0, (-3, 12))
    assert tt.parse_args([f"--noise_bank={grid}", "--noise_snr_db=[0,0]"]).noise_policy.snr_db == (0, 0)
    for flag in ("--noise_prob=1.5", "--noise_prob=-1", "--noise_prob=often", "--noise_snr_db=5", "--noise_snr_db=5,20,30", "--noise_snr_db=20,5",
                 "--noise_snr_db=-11,5", "--noise_snr_db=5,51", "--noise_snr_db=5.5,20", "--noise_snr_db=quiet"):
        with pytest.raises(SystemExit, match="--noise_"):
            tt.parse_args([f"--noise_bank={grid}", flag])
    assert tt.load_noise_bank(str(grid)).tolist() == np.arange(24).reshape(3, 8).tolist()
    ragged = np.empty(2, dtype=object)
    ragged[0], ragged[1] = np.array([1, 2, 3], dtype=np.int16), np.array([4, 5, 6, 7, 8], dtype=np.int16)
    np.save(tmp_path / "ragged.npy", ragged, allow_pickle=True)
    assert tt.load_noise_bank(str(tmp_path / "ragged.npy")).tolist() == [[1, 2, 3, 1, 2], [4, 5, 6, 7, 8]]
    np.save(tmp_path / "floats.npy", np.zeros((2, 8), dtype=np.float32))
    with pytest.raises(SystemExit, match="--noise_bank"):
        tt.load_noise_bank(str(tmp_path / "floats.npy"))
