"""CPU half of reverberation (csrc/reverb_core.h through its host twin: oasr_reverb_host, oasr_reverb_plan): the twin against the rule of
include/oasr.h restated twice in tests/reverb_cases.py (Python integers; np.convolve in float64, exact here), the seeded draws, the contract's
clamps, ``augment.rir_bank``, the argument checks that fire before anything is written, the binding's struct sizes and the training
script's flags."""
import ctypes
import importlib.util
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reverb_cases as rc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
SEEDS = ((0, 0), (7, 3), (2 ** 63 + 5, 2 ** 40), (M64, M64 - 2))


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
    spec = importlib.util.spec_from_file_location("tt_reverb_cpu", os.path.join(ROOT, "scripts", "training", "train_timestamps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def i32(v):
    return torch.tensor(np.asarray(v), dtype=torch.int32)


def twin(ops, x, nv, bank, delay, prob_q16, seed, first):
    out, row = ops.reverb_host(torch.from_numpy(np.ascontiguousarray(x)), i32(nv), torch.from_numpy(np.ascontiguousarray(bank)), i32(delay),
                               prob=prob_q16 / 65536, seed=seed, first_clip=first)
    return out.tolist(), row.tolist()


# ---- the twin against both restatements -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 15, 16, 17, 81])
def test_host_twin_equals_both_restatements(ops, K):
    B, N, R = 5, 203, 4
    x = rc.clips(B, N, 50 + K, amp=32767)
    x[1] = np.where(np.arange(N) & 16, 32767, -32768)  # a saturating row
    bank, delay = rc.quantized_bank(R, K, 9 + K, pre=3)
    bank[0, 0], bank[1, K - 1] = 32767, -32768          # beyond the tap clamp, both ways
    delay[R - 1], delay[R - 2] = K + 5, -5               # beyond the delay clamp, both ways
    wet = set()
    for k, (seed, first) in enumerate(SEEDS):
        nv = [N, 0 if k % 2 else N // 2, N - 1, 1 if k % 3 else -1, N if k else N + 1]
        got = twin(ops, x, nv, bank, delay, 49152, seed, first)
        assert got == rc.restated(x, nv, bank, delay, 49152, seed, first)
        assert got == rc.restated_float64(x, nv, bank, delay, 49152, seed, first)
        wet |= {r >= 0 for r in got[1]}
    assert wet == {True, False}


@pytest.mark.parametrize("K", [1000, 4096, 8192])
def test_host_twin_equals_the_float64_convolution_at_long_responses(ops, K):
    B, N, R = 3, 9001, 3
    x = rc.clips(B, N, 60 + K, amp=32767)
    bank, delay = rc.quantized_bank(R, K, 19 + K)
    nv = [N, K // 2 + 1, N - 300]
    got = twin(ops, x, nv, bank, delay, 65536, 3, 11)
    assert got == rc.restated_float64(x, nv, bank, delay, 65536, 3, 11) and min(got[1]) >= 0
    # the extremes of the sum: all taps at the clamp against full-scale input saturate on both sides
    ext = np.full((1, K), 32767, dtype=np.int16)
    xs = np.stack([np.full(N, -32768), np.full(N, 32767), np.where(np.arange(N) & 1, 255, -129)]).astype(np.int16)
    got = twin(ops, xs, [N] * 3, ext, [K // 2], 65536, 0, 0)
    assert got == rc.restated_float64(xs, [N] * 3, ext, [K // 2], 65536, 0, 0)
    assert min(got[0][0]) == -32768 and max(got[0][1]) == 32767


def test_known_answers(ops):
    x = np.array([[100, -200, 300, -400, 500, 7, 7, 7]], dtype=np.int16)
    # the identity: one tap of 2^15 would be 1.0; the clamp leaves 32639 / 32768
    one = np.array([[32767, 0, 0]], dtype=np.int16)
    y, row = twin(ops, x, [5], one, [0], 65536, 0, 0)
    assert row == [0] and y[0] == [(v * 32639 + 16384) >> 15 for v in (100, -200, 300, -400, 500)] + [7, 7, 7]
    # a pure delay of 2 with the direct path AT 2 is undone by the shift; with the direct path declared at 0 the clip moves right and is cut
    late = np.array([[0, 0, 16384]], dtype=np.int16)
    assert twin(ops, x, [5], late, [2], 65536, 0, 0)[0][0] == [50, -100, 150, -200, 250, 7, 7, 7]
    assert twin(ops, x, [5], late, [0], 65536, 0, 0)[0][0] == [0, 0, 50, -100, 150, 7, 7, 7]
    # ... and declared beyond the response (clamped to K - 1 = 2) it is the first case again; a negative one is 0
    assert twin(ops, x, [5], late, [99], 65536, 0, 0)[0][0] == [50, -100, 150, -200, 250, 7, 7, 7]
    assert twin(ops, x, [5], late, [-99], 65536, 0, 0)[0][0] == [0, 0, 50, -100, 150, 7, 7, 7]
    # rounding: halves go up (an arithmetic shift floors after + 2^14): -1 * 16384 / 32768 = -0.5 -> 0,  -3 * 16384 / 32768 = -1.5 -> -1
    half = np.array([[16384]], dtype=np.int16)
    assert twin(ops, np.array([[-1, -3, 1, 3]], dtype=np.int16), [4], half, [0], 65536, 0, 0)[0][0] == [0, -1, 1, 2]
    # what lies behind n_valid is copied and is not heard
    a, b = x.copy(), x.copy()
    b[0, 5:] = [30000, -30000, 12345]
    echo = np.array([[16384, 8192, 4096]], dtype=np.int16)
    ya, yb = twin(ops, a, [5], echo, [1], 65536, 0, 0)[0][0], twin(ops, b, [5], echo, [1], 65536, 0, 0)[0][0]
    assert ya[:5] == yb[:5] and ya[5:] == [7, 7, 7] and yb[5:] == [30000, -30000, 12345]


def test_plan_is_the_stated_hash(ops):
    from olmoasr_amd import augment
    for seed, first in SEEDS:
        for prob_q16 in (0, 1, 32768, 65535, 65536):
            for R in (1, 2, 7, 65535):
                for b in range(8):
                    clip = (first + b) & M64
                    assert ops.reverb_plan(prob_q16 / 65536, seed, clip, R) == rc.plan(seed, clip, prob_q16, R)
    pol = augment.Reverb(prob=0.25)
    assert pol.plan(5, 9, 3) == rc.plan(5, 9, 16384, 3)
    assert pol.drawn(5, M64 - 3, 16, 3) == sum(rc.plan(5, (M64 - 3 + b) & M64, 16384, 3)[0] for b in range(16))  # (stream ids wrap mod 2^64)


@pytest.mark.parametrize("prob", [0.1, 0.5, 0.9])
def test_the_drawn_share_is_the_probability(ops, prob):
    n = 4096
    drawn = sum(ops.reverb_plan(prob, 1234, clip, 16)[0] for clip in range(n))
    assert abs(drawn - n * prob) <= 4 * math.sqrt(n * prob * (1 - prob))  # binomial, 4 sigma
    rows = [ops.reverb_plan(1.0, 1234, clip, 16)[1] for clip in range(n)]
    assert set(rows) == set(range(16))


def test_the_draws_are_not_the_noise_draws(ops):
    clips = range(4096)
    reverb = [ops.reverb_plan(0.5, 77, c, 16) for c in clips]
    noise = [ops.noise_plan(0.5, (5, 20), 77, c, 16, 1000)[:2] for c in clips]
    assert [d for d, _ in reverb] != [d for d, _ in noise] and [r for _, r in reverb] != [r for _, r in noise]
    agree = sum(a[0] == b[0] for a, b in zip(reverb, noise))
    assert abs(agree - 2048) <= 4 * math.sqrt(4096 * 0.25)  # independent fair coins agree half the time
    assert reverb == [rc.plan(77, c, 32768, 16) for c in clips] and [n[0] for n in noise] == [rc.plan(77, c, 32768, 16, kind=4)[0] for c in clips]


def test_probability_ends(ops):
    x, bank = rc.clips(6, 64, 1), rc.quantized_bank(2, 9, 2)[0]
    y, row = twin(ops, x, [64] * 6, bank, [0, 0], 0, 5, 5)
    assert row == [-1] * 6 and y == x.tolist()
    assert min(twin(ops, x, [64] * 6, bank, [0, 0], 65536, 5, 5)[1]) >= 0


# ---- the bank ---------------------------------------------------------------------------------------------------------------------------
def test_rir_bank():
    from olmoasr_amd import augment
    hs = rc.responses(5, 700, 3)
    bank, delay = augment.rir_bank(hs)
    assert bank.dtype == torch.int16 and delay.dtype == torch.int32 and tuple(bank.shape) == (5, 700) and tuple(delay.shape) == (5,)
    want_bank, want_delay = rc.quantized_bank(5, 700, 3)
    assert delay.tolist() == want_delay.tolist() == [int(np.argmax(np.abs(h))) for h in hs] and bank.tolist() == want_bank.tolist()
    for K in (700, 300, 64):  # unit energy in Q15: |rounding error| <= 1/2 per tap, Cauchy-Schwarz against the unit-energy vector
        q = augment.rir_bank(hs, K)[0].numpy().astype(np.int64)
        assert np.abs(q).max() < 32639  # no tap was clamped
        assert all(abs(int(np.sum(r * r)) - 2 ** 30) <= 2 ** 15 * math.sqrt(K) + K / 4 for r in q)
    # cut and zero-padded; float32 and torch inputs; the default K is min(8192, the longest)
    short = augment.rir_bank([hs[0][:100].astype(np.float32), torch.from_numpy(hs[1])], 256)[0]
    assert tuple(short.shape) == (2, 256) and bool((short[0, 100:] == 0).all()) and bool((short[1] != 0).any())
    assert tuple(augment.rir_bank([np.ones(3), np.ones(9000)])[0].shape) == (2, 8192)
    # a lone tap of any size is the clamp's 32639; its sign stays
    lone = augment.rir_bank([np.array([0.0, -3.5, 0.0])])
    assert lone[0].tolist() == [[0, -32639, 0]] and lone[1].tolist() == [1]
    late = np.zeros(50)
    late[40], late[3] = 1.0, 0.5
    assert augment.rir_bank([late], 41)[1].tolist() == [40]
    with pytest.raises(ValueError, match="direct path"):
        augment.rir_bank([late], 40)  # delay >= K
    for bad in (([],), ([np.ones((2, 3))],), ([np.ones(0)],), ([np.ones(3, dtype=np.int16)],), ([np.zeros(4)],), ([np.array([1.0, np.nan])],),
                ([np.ones(3)], 0), ([np.ones(3)], 8193), ([np.ones(3)], 8.0)):
        with pytest.raises(ValueError):
            augment.rir_bank(*bad)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(native, ops):
    lib = native.lib()
    N, K = 64, 32
    x, y = torch.full((2, N), 3, dtype=torch.int16), torch.full((2, N), 5, dtype=torch.int16)
    bank, nv, delay, row = torch.full((2, K), 7, dtype=torch.int16), i32([N, 10]), i32([0, 3]), i32([99, 99])

    def block(**kw):
        a = native.ReverbArgs()
        a.pcm_in, a.pcm_out, a.n_valid, a.rir, a.delay, a.row_out = x.data_ptr(), y.data_ptr(), nv.data_ptr(), bank.data_ptr(), delay.data_ptr(), row.data_ptr()
        a.ld_in = a.ld_out = N
        a.ld_rir, a.B, a.N, a.R, a.K = K, 2, N, 2, K
        a.policy = native.Reverb(65536)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(a, what):
        return lib.oasr_reverb_host(ctypes.byref(a)) == -1 and what in lib.oasr_last_error().decode()  # OASR_EINVAL

    both = torch.full((2, N + 32), 3, dtype=torch.int16)
    cases = [(dict(B=0), "B outside"), (dict(B=65536), "B outside"), (dict(N=0), "N outside"), (dict(N=(1 << 26) + 1, ld_in=1 << 27, ld_out=1 << 27), "N outside"),
             (dict(R=0), "R outside"), (dict(R=65536), "R outside"), (dict(K=0), "K outside"), (dict(K=8193, ld_rir=8193), "K outside"),
             (dict(ld_in=N - 1), "stride"), (dict(ld_out=N - 1), "stride"), (dict(ld_rir=K - 1), "stride"),
             (dict(pcm_in=x.data_ptr() + 1), "2-byte"), (dict(pcm_out=y.data_ptr() + 1), "2-byte"), (dict(rir=bank.data_ptr() + 1), "2-byte"),
             (dict(row_out=row.data_ptr() + 2), "4-byte"), (dict(delay=delay.data_ptr() + 2), "4-byte"), (dict(n_valid=nv.data_ptr() + 2), "4-byte"),
             (dict(pcm_in=None), "null"), (dict(pcm_out=None), "null"), (dict(n_valid=None), "null"), (dict(rir=None), "null"), (dict(delay=None), "null"),
             (dict(pcm_in=y.data_ptr()), "overlap"),                                                                    # in place is not offered
             (dict(pcm_in=both.data_ptr(), pcm_out=both[:, 32:].data_ptr(), ld_in=N + 32, ld_out=N + 32), "overlap"),  # partial overlap
             (dict(rir=y.data_ptr()), "rir and pcm_out"),
             (dict(policy=native.Reverb(-1)), "prob_q16"), (dict(policy=native.Reverb(65537)), "prob_q16")]
    for kw, what in cases:
        assert refused(block(**kw), what), (kw, lib.oasr_last_error().decode())
    assert lib.oasr_reverb_host(None) == -1
    out = [ctypes.c_int(-5) for _ in range(2)]
    for pol, R in ((native.Reverb(65537), 1), (native.Reverb(-1), 1), (native.Reverb(1), 0), (native.Reverb(1), 65536)):
        assert lib.oasr_reverb_plan(ctypes.byref(pol), 0, 0, R, *[ctypes.byref(o) for o in out]) == -1
    assert lib.oasr_reverb_plan(None, 0, 0, 1, *[ctypes.byref(o) for o in out]) == -1
    assert [o.value for o in out] == [-5] * 2
    assert bool((y == 5).all()) and bool((x == 3).all()) and bool((both == 3).all()) and row.tolist() == [99, 99]
    assert lib.oasr_reverb_host(ctypes.byref(block())) == 0           # the block they were derived from is fine
    assert lib.oasr_reverb_host(ctypes.byref(block(row_out=None))) == 0  # ... and the report is optional
    y.fill_(5)
    # the Python surface: policy, dtypes, shapes, overlap
    for kw in (dict(prob=-0.1), dict(prob=1.5), dict(prob=float("nan")), dict(prob="1"), dict(prob=True), dict(pcm=x.float()), dict(pcm=x[0]), dict(pcm=x.t()),
               dict(n_valid=nv.long()), dict(n_valid=nv[:1]), dict(delay=delay.long()), dict(delay=delay[:1]), dict(bank=bank.float()), dict(bank=bank[0]),
               dict(bank=bank[:0], delay=delay[:0]), dict(bank=bank[:, :0]), dict(bank=bank.t()), dict(bank=torch.zeros(2, 8193, dtype=torch.int16)),
               dict(out=torch.zeros(2, N)), dict(out=torch.zeros(2, N + 1, dtype=torch.int16)), dict(out=x), dict(out=both[:, 1:N + 1], pcm=both[:, :N]),
               dict(out=bank.expand(2, K), pcm=x[:, :K]), dict(seed=-1), dict(first_clip=2 ** 64)):
        args = dict(pcm=x, n_valid=nv, bank=bank, delay=delay, prob=0.5, out=y)
        args.update(kw)
        pcm, n_valid, bk, dl = args.pop("pcm"), args.pop("n_valid"), args.pop("bank"), args.pop("delay")
        with pytest.raises(ValueError):
            ops.reverb_host(pcm, n_valid, bk, dl, **args)
    for bad in (dict(R=0), dict(R=65536), dict(R=1.0), dict(R=True), dict(seed=-1), dict(clip=2 ** 64), dict(prob=2.0)):
        args = dict(prob=0.5, seed=0, clip=0, R=2)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.reverb_plan(**args)
    with pytest.raises(ValueError, match="GPU"):
        ops.reverb(x, nv, bank, delay, prob=0.5)  # the device entry takes no CPU tensor, and says so before a launch
    from olmoasr_amd import augment
    for bad in (dict(prob=1.01), dict(prob=-0.5), dict(prob=None)):
        with pytest.raises(ValueError):
            augment.Reverb(**bad)
    assert bool((y == 5).all()) and bool((x == 3).all())
    empty = ops.reverb_host(x[:0], nv[:0], bank, delay, prob=0.5)  # B = 0: nothing to do, not an error
    assert tuple(empty[0].shape) == (0, N) and empty[1].numel() == 0


def test_struct_sizes_and_version(native):
    lib = native.lib()
    assert lib.oasr_version() == 216 == native.ABI_VERSION
    assert lib.oasr_sizeof_reverb() == ctypes.sizeof(native.Reverb) == 4
    assert lib.oasr_sizeof_reverb_args() == ctypes.sizeof(native.ReverbArgs) == 128
    assert ("oasr_sizeof_reverb", native.Reverb) in native.STRUCT_SIZES and ("oasr_sizeof_reverb_args", native.ReverbArgs) in native.STRUCT_SIZES
    assert (native.ReverbArgs.MAX_K, native.ReverbArgs.TAP_MAX) == (8192, 32639)
    # the R tap sums, then per row and 64-tap k-step the two 1 KiB digit fragments; blocks c = 0 .. (K + 14) / 16, four to a k-step
    for R, K in ((1, 1), (3, 81), (16, 4096), (16, 8192), (65535, 50)):
        steps = ((K + 14) // 16 + 1 + 3) // 4
        assert lib.oasr_reverb_workspace_bytes(R, K) == (8 * R + 15) // 16 * 16 + R * steps * 2048
    for R, K in ((0, 5), (5, 0), (65536, 5), (5, 8193)):
        assert lib.oasr_reverb_workspace_bytes(R, K) == 0


# ---- the training script ----------------------------------------------------------------------------------------------------------------
def test_cli_flags(tt, native, tmp_path):
    off = tt.parse_args([])
    assert off.rir_bank is None and off.reverb_prob is None and off.reverb_policy is None
    assert all(f in tt.NATIVE_FLAGS for f in ("rir_bank", "reverb_prob"))
    with pytest.raises(SystemExit, match="--reverb_prob given without --rir_bank"):
        tt.parse_args(["--reverb_prob=0.5"])
    with pytest.raises(SystemExit, match="--rir_bank"):
        tt.parse_args([f"--rir_bank={tmp_path}/missing.npy"])
    hs = rc.responses(3, 120, 8)
    grid = tmp_path / "grid.npy"
    np.save(grid, np.stack(hs).astype(np.float32))
    on = tt.parse_args([f"--rir_bank={grid}"])
    assert on.reverb_policy.prob == 0.5
    rest = {k: v for k, v in on.items() if k not in ("rir_bank", "reverb_policy")}
    assert rest == {k: v for k, v in off.items() if k not in ("rir_bank", "reverb_policy")}  # nothing else moves
    assert tt.parse_args(["--rir_bank", str(grid), "--reverb_prob", "1.0"]).reverb_policy.prob == 1.0
    for flag in ("--reverb_prob=1.5", "--reverb_prob=-1", "--reverb_prob=often"):
        with pytest.raises(SystemExit, match="--reverb_prob"):
            tt.parse_args([f"--rir_bank={grid}", flag])
    from olmoasr_amd import augment
    bank, delay = tt.load_rir_bank(str(grid))
    want = augment.rir_bank([h.astype(np.float32) for h in hs])
    assert bank.tolist() == want[0].tolist() and delay.tolist() == want[1].tolist() and tuple(bank.shape) == (3, 120)
    ragged = np.empty(2, dtype=object)
    ragged[0], ragged[1] = hs[0][:50], hs[1]
    np.save(tmp_path / "ragged.npy", ragged, allow_pickle=True)
    bank, delay = tt.load_rir_bank(str(tmp_path / "ragged.npy"))
    assert tuple(bank.shape) == (2, 120) and bool((bank[0, 50:] == 0).all()) and delay.tolist() == [7, 8]
    np.save(tmp_path / "ints.npy", np.ones((2, 8), dtype=np.int16))
    with pytest.raises(SystemExit, match="--rir_bank"):
        tt.load_rir_bank(str(tmp_path / "ints.npy"))
    np.save(tmp_path / "silent.npy", np.zeros((2, 8), dtype=np.float32))
    with pytest.raises(SystemExit, match="--rir_bank"):
        tt.load_rir_bank(str(tmp_path / "silent.npy"))
