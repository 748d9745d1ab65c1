"""CPU half of the telephone channel (csrc/telephone_core.h through its host twin: oasr_telephone_host, oasr_telephone_plan,
oasr_telephone_tables, oasr_telephone_quantize_host): the twin against the rule of include/oasr.h restated in Python integers in
tests/telephone_cases.py, both quantisers over all 65536 inputs, the two tables against their formulas, the seeded draws, the rows on which
a 32-bit accumulator wraps, quality guards on the filters and the codecs, the argument checks that fire before anything is written, the
binding's struct sizes and the training script's flags."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import telephone_cases as tc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
NAMES = ("linear", "mulaw", "alaw")


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
    spec = importlib.util.spec_from_file_location("tt_telephone_cpu", os.path.join(ROOT, "scripts", "training", "train_timestamps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def i32(v):
    return torch.tensor(np.asarray(v), dtype=torch.int32)


def assert_twin(ops, x, nv, prob, codecs, bandpass, seed, first):
    got = ops.telephone_host(torch.from_numpy(x), i32(nv), prob=prob, codecs=[NAMES[c] for c in codecs], bandpass=bandpass, seed=seed, first_clip=first)
    want = tc.restated(x.tolist(), nv, int(round(prob * 65536)), codecs, bandpass, seed, first)
    assert got[0].dtype == torch.int16 and got[1].dtype == torch.int32
    assert got[1].tolist() == want[1], "codec_out differs from the restatement"
    for b, (g, w) in enumerate(zip(got[0].tolist(), want[0])):
        assert g == w, f"row {b} differs from the restatement"
    return got


# ---- the operator ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [299, 700])
def test_host_twin_equals_the_restatement(ops, N):
    B = 7
    x = tc.clips(B, N, 100 + N)
    x[5, :N // 2], x[5, N // 2:] = 32767, -32768  # a row that saturates the band-pass's output
    x[6, ::2], x[6, 1::2] = 32767, -32768
    wide = np.zeros((B, N + 3), dtype=np.int16)[:, :N]  # (a row stride above N)
    wide[:] = x
    nv = [0, 1, 2, 3, 37, N - 1, N]
    for codec in (tc.LINEAR, tc.MULAW, tc.ALAW):
        for bandpass in (True, False):
            seed, first = tc.SEEDS[(codec + bandpass) % 3]
            got = assert_twin(ops, x, nv, 1.0, [codec], bandpass, seed, first)
            assert got[1].tolist() == [-1] + [codec] * 6
    seen = set()
    for seed, first in tc.SEEDS:
        for bandpass in (True, False):
            got = assert_twin(ops, x, nv[::-1], 0.75, [tc.MULAW, tc.ALAW, tc.LINEAR], bandpass, seed, first)
            seen |= set(got[1].tolist())
    assert seen == {-1, 0, 1, 2}
    got = ops.telephone_host(torch.from_numpy(wide), i32(nv), prob=1.0, codecs=["alaw"], seed=11, first_clip=M64 - 1)  # (stream ids wrap mod 2^64)
    assert got[0].tolist() == tc.restated(x.tolist(), nv, 65536, [tc.ALAW], True, 11, M64 - 1)[0]
    for bad in (-1, N + 1, -2 ** 31, 2 ** 31 - 1):  # a length outside the contract copies the row
        got = ops.telephone_host(torch.from_numpy(x[:2]), i32([N, bad]), prob=1.0, codecs=["mulaw"])
        assert got[1].tolist() == [1, -1] and got[0][1].tolist() == x[1].tolist()


def test_out_is_written_and_the_tail_is_copied(ops):
    N = 300
    x = torch.from_numpy(tc.clips(2, N, 9))
    out = torch.full((2, N + 5), 77, dtype=torch.int16)
    got = ops.telephone_host(x, i32([N, 100]), prob=1.0, codecs=["linear"], out=out[:, :N])
    assert got[0].data_ptr() == out.data_ptr() and bool((out[:, N:] == 77).all())
    assert torch.equal(got[0][1, 100:], x[1, 100:]) and not torch.equal(got[0][1, :100], x[1, :100])


# ---- the quantisers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, levels, top, at0, at_minus1, worst", [("mulaw", 255, 32124, 0, 0, 644), ("alaw", 256, 32256, 8, -8, 512)])
def test_quantisers_over_all_inputs(ops, name, levels, top, at0, at_minus1, worst):
    x = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    q = ops.telephone_quantize_host(x, name)
    want = [tc.quantize(v, NAMES.index(name)) for v in range(-32768, 32768)]
    assert q.dtype == torch.int16 and q.tolist() == want
    assert len(set(want)) == levels and (min(want), max(want)) == (-top, top)
    assert (want[32768], want[32767]) == (at0, at_minus1)
    assert max(abs(w - v) for w, v in zip(want, range(-32768, 32768))) == worst
    assert all(a <= b for a, b in zip(want, want[1:])), "not monotone"
    assert torch.equal(ops.telephone_quantize_host(q, name), q), "not idempotent"
    assert torch.equal(ops.telephone_quantize_host(x, "linear"), x)
    assert torch.equal(ops.telephone_quantize_host(x.view(256, 256), NAMES.index(name)), q.view(256, 256))


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------
def test_tables_match_their_formulas(ops):
    h, u = ops.telephone_tables()
    assert h.dtype == u.dtype == torch.int32 and h.tolist() == tc.H and u.tolist() == tc.U
    assert len(tc.H) == 129 and len(tc.U) == 32
    assert sum(tc.U) == 32768
    assert tc.H == tc.H[::-1], "h is not symmetric"
    assert sum(abs(v) for v in tc.H) == tc.SUM_ABS_H == 76960 and sum(abs(v) for v in tc.U) == tc.SUM_ABS_U == 81604
    assert tc.SUM_ABS_H * 32768 > 2 ** 31 and tc.SUM_ABS_U * 32768 > 2 ** 31  # one 32-bit accumulator can wrap ...
    # ... and the partial sums a 32-bit implementation may keep cannot: even / odd taps of h, the two halves of u
    for group in (tc.H[0::2], tc.H[1::2], tc.U[:16], tc.U[16:]):
        assert sum(abs(v) for v in group) <= 65535


# ---- the draws ----------------------------------------------------------------------------------------------------------------------------
def test_plan_is_the_stated_hash(ops):
    from olmoasr_amd import augment
    seen = set()
    for seed, first in tc.SEEDS:
        for b in range(24):
            for prob, codecs in ((0.5, (1, 2, 0)), (1.0, (2,)), (0.0, (0, 0, 1)), (0.25, (1, 1, 1, 1, 1, 1, 1, 2))):
                want = tc.plan(seed, first + b, int(round(prob * 65536)), codecs)
                assert ops.telephone_plan(prob, [NAMES[c] for c in codecs], seed, first + b) == want
                assert augment.TelephoneChannel(prob=prob, codecs=tuple(NAMES[c] for c in codecs)).plan(seed, first + b) == (want[0], NAMES[want[1]])
                if prob == 0.5:
                    seen.add(want)
    assert {d for d, _ in seen} == {True, False} and {c for _, c in seen} == {0, 1, 2}
    pol = augment.TelephoneChannel(prob=0.5)
    draws = [tc.plan(9, (M64 - 3 + b) & M64, 32768, (1, 2, 0)) for b in range(16)]
    assert pol.drawn(9, M64 - 3, 16) == {n: sum(d and c == i for d, c in draws) for i, n in enumerate(NAMES)}


def test_a_batch_equals_its_clips_one_by_one(ops):
    B, N = 12, 200
    x, nv = torch.from_numpy(tc.clips(B, N, 33)), i32([N - b for b in range(B)])
    for first in (5, 2 ** 32 - 2, M64 - 1):
        kw = dict(prob=0.5, codecs=["mulaw", "alaw", "linear"], seed=17)
        batch = ops.telephone_host(x, nv, first_clip=first, **kw)
        assert {c >= 0 for c in batch[1].tolist()} == {True, False}
        for b in range(B):
            single = ops.telephone_host(x[b:b + 1], nv[b:b + 1], first_clip=(first + b) & M64, **kw)
            assert torch.equal(single[0][0], batch[0][b]) and int(single[1][0]) == int(batch[1][b])
            drawn, codec = tc.plan(17, (first + b) & M64, 32768, (1, 2, 0))
            assert int(batch[1][b]) == (codec if drawn else -1)


# ---- exact sums -----------------------------------------------------------------------------------------------------------------------------
def test_planted_wrap_rows(ops):
    """Sums above 2^31: the rule gives +32767 at the planted sample, a wrapped 32-bit accumulator a negative one."""
    N = 400
    x = tc.wrap_row_bandpass(N, 200)
    y = ops.telephone_host(torch.from_numpy(x[None]), i32([N]), prob=1.0, codecs=["linear"])[0][0]
    assert int(y[200]) == 32767 and y.tolist() == tc.channel(x, N, tc.LINEAR, True)
    x = tc.wrap_row_interpolator(N, 100)
    y = ops.telephone_host(torch.from_numpy(x[None]), i32([N]), prob=1.0, codecs=["linear"], bandpass=False)[0][0]
    assert int(y[201]) == 32767 and y.tolist() == tc.channel(x, N, tc.LINEAR, False)


# ---- quality guards -------------------------------------------------------------------------------------------------------------------------
def through(ops, x, codec="linear", bandpass=True):
    return ops.telephone_host(torch.from_numpy(x[None].copy()), i32([x.size]), prob=1.0, codecs=[codec], bandpass=bandpass)[0][0].numpy().astype(np.float64)


@pytest.mark.parametrize("freq, phase, bound, what", [(1000, 0.0, -70.0, "error"), (1000, 0.3, -70.0, "error"), (6000, 0.0, -60.0, "output"),
                                                      (100, 0.0, -40.0, "output")])
def test_quality_guard_on_the_filters(ops, freq, phase, bound, what):
    """Linear codec, amplitude 10000, 8000 samples, scored over samples 400 .. 7600.  Measured from the rule: 1 kHz passes with an error of
    -86 dB at lag 0 (the filters are zero-phase) when it starts at 0.3 rad, and bit for bit when it starts at 0 (it then repeats every 16
    samples); 6 kHz comes out at -78 dB, 100 Hz at -48.7 dB.  The margins cover the int16 output rounding."""
    x = tc.sine(freq, phase=phase)
    y, xf = through(ops, x)[400:7600], x.astype(np.float64)[400:7600]
    level = tc.db(np.sum((y - xf) ** 2) if what == "error" else np.sum(y ** 2), np.sum(xf ** 2))
    print(f"{freq} Hz: {what} at {level:.1f} dB of the input")
    assert level <= bound


@pytest.mark.parametrize("codec", ["mulaw", "alaw"])
def test_quality_guard_on_the_codecs(ops, codec):
    """A Gaussian clip of rms 3000 through the codec against the linear output of the same operator: G.711's 37 to 38 dB (measured from the
    rule: 37.0 dB for mu-law, 37.7 dB for A-law)."""
    x = np.clip(np.round(np.random.default_rng(5).standard_normal(8000) * 3000), -32768, 32767).astype(np.int16)
    lin, y = through(ops, x), through(ops, x, codec)
    snr = tc.db(np.sum(lin ** 2), np.sum((y - lin) ** 2))
    print(f"{codec}: {snr:.1f} dB against the linear channel")
    assert 33.0 <= snr <= 41.0


# ---- refusals, sizes --------------------------------------------------------------------------------------------------------------------
def test_refusals(native, ops):
    lib = native.lib()
    N = 64
    x, y = torch.full((2, N), 3, dtype=torch.int16), torch.full((2, N), 5, dtype=torch.int16)
    nv, cd = i32([N, 10]), i32([99, 99])

    def policy(prob_q16=65536, codecs=(1, 2), bandpass=1, n_codecs=None):
        p = native.Telephone()
        p.prob_q16, p.n_codecs, p.bandpass = prob_q16, len(codecs) if n_codecs is None else n_codecs, bandpass
        for i, c in enumerate(codecs):
            p.codecs[i] = c
        return p

    def block(**kw):
        a = native.TelephoneArgs()
        a.pcm_in, a.pcm_out, a.n_valid, a.codec_out = x.data_ptr(), y.data_ptr(), nv.data_ptr(), cd.data_ptr()
        a.ld_in = a.ld_out = N
        a.B, a.N, a.policy = 2, N, policy()
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(a, what):
        return lib.oasr_telephone_host(ctypes.byref(a)) == -1 and what in lib.oasr_last_error().decode()  # OASR_EINVAL

    both = torch.full((2, N + 32), 3, dtype=torch.int16)
    cases = [(dict(B=0), "B outside"), (dict(B=65536), "B outside"), (dict(N=0), "N outside"), (dict(N=(1 << 26) + 1, ld_in=1 << 27, ld_out=1 << 27), "N outside"),
             (dict(ld_in=N - 1), "stride"), (dict(ld_out=N - 1), "stride"), (dict(pcm_in=x.data_ptr() + 1), "2-byte"), (dict(pcm_out=y.data_ptr() + 1), "2-byte"),
             (dict(codec_out=cd.data_ptr() + 2), "4-byte"), (dict(n_valid=nv.data_ptr() + 2), "4-byte"),
             (dict(pcm_in=None), "null"), (dict(pcm_out=None), "null"), (dict(n_valid=None), "null"),
             (dict(pcm_in=both.data_ptr(), pcm_out=both[:, 32:].data_ptr(), ld_in=N + 32, ld_out=N + 32), "overlap"),  # partial overlap
             (dict(pcm_in=y.data_ptr()), "out of place"),                                                            # in place is not offered
             (dict(policy=policy(prob_q16=-1)), "prob_q16"), (dict(policy=policy(prob_q16=65537)), "prob_q16"),
             (dict(policy=policy(codecs=(), n_codecs=0)), "n_codecs"), (dict(policy=policy(n_codecs=9)), "n_codecs"),
             (dict(policy=policy(codecs=(1, 3))), "codec"), (dict(policy=policy(codecs=(-1,))), "codec"),
             (dict(policy=policy(bandpass=2)), "bandpass"), (dict(policy=policy(bandpass=-1)), "bandpass")]
    for kw, what in cases:
        assert refused(block(**kw), what), (kw, lib.oasr_last_error().decode())
    assert lib.oasr_telephone_host(None) == -1
    out = [ctypes.c_int(-5), ctypes.c_int(-5)]
    for pol in (policy(prob_q16=65537), policy(codecs=(3,)), policy(n_codecs=0), policy(bandpass=5)):
        assert lib.oasr_telephone_plan(ctypes.byref(pol), 0, 0, ctypes.byref(out[0]), ctypes.byref(out[1])) == -1
    assert lib.oasr_telephone_plan(None, 0, 0, ctypes.byref(out[0]), ctypes.byref(out[1])) == -1
    assert [o.value for o in out] == [-5, -5]
    assert lib.oasr_telephone_quantize_host(x.data_ptr(), y.data_ptr(), 4, 3) == -1 and lib.oasr_telephone_quantize_host(x.data_ptr(), y.data_ptr(), -1, 0) == -1
    assert lib.oasr_telephone_quantize_host(None, y.data_ptr(), 4, 0) == -1
    assert bool((y == 5).all()) and bool((x == 3).all()) and bool((both == 3).all()) and cd.tolist() == [99, 99]
    assert lib.oasr_telephone_host(ctypes.byref(block())) == 0  # the block they were derived from is fine
    assert lib.oasr_telephone_host(ctypes.byref(block(codec_out=None))) == 0  # ... and so is one without the report
    y.fill_(5)
    # the Python surface: policy, dtypes, shapes, overlap
    for kw in (dict(prob=-0.1), dict(prob=1.5), dict(prob=float("nan")), dict(prob="1"), dict(prob=True), dict(codecs=()), dict(codecs=["mulaw"] * 9),
               dict(codecs=["gsm"]), dict(codecs="mulaw"), dict(codecs=[3]), dict(codecs=[True]), dict(codecs=None), dict(bandpass=1), dict(bandpass=None),
               dict(pcm=x.float()), dict(pcm=x[0]), dict(pcm=x.t()), dict(n_valid=nv.long()), dict(n_valid=nv[:1]), dict(out=torch.zeros(2, N)),
               dict(out=torch.zeros(2, N + 1, dtype=torch.int16)), dict(out=both[:, 1:N + 1], pcm=both[:, :N]), dict(out=x), dict(seed=-1), dict(first_clip=2 ** 64)):
        args = dict(pcm=x, n_valid=nv, prob=0.5, codecs=["mulaw", "alaw"], out=y)
        args.update(kw)
        pcm, n_valid = args.pop("pcm"), args.pop("n_valid")
        with pytest.raises(ValueError):
            ops.telephone_host(pcm, n_valid, **args)
    for bad in (dict(seed=-1), dict(clip=2 ** 64), dict(prob=2.0), dict(codecs=["ulaw"]), dict(codecs=[])):
        args = dict(prob=0.5, codecs=["mulaw"], seed=0, clip=0)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.telephone_plan(**args)
    for bad in ((x.int(), "mulaw"), (x.t(), "mulaw"), (x, "gsm"), (x, 3), (x.tolist(), "alaw")):
        with pytest.raises(ValueError):
            ops.telephone_quantize_host(*bad)
    with pytest.raises(ValueError, match="GPU"):
        ops.telephone(x, nv, prob=0.5)  # the device entry takes no CPU tensor, and says so before a launch
    from olmoasr_amd import augment
    for bad in (dict(prob=1.01), dict(codecs=("mulaw", "amr")), dict(codecs=()), dict(bandpass="yes")):
        with pytest.raises(ValueError):
            augment.TelephoneChannel(**bad)
    assert bool((y == 5).all()) and bool((x == 3).all())
    empty = ops.telephone_host(x[:0], nv[:0], prob=0.5)  # B = 0: nothing to do, not an error
    assert tuple(empty[0].shape) == (0, N) and empty[1].numel() == 0


def test_struct_sizes_and_version(native):
    lib = native.lib()
    assert lib.oasr_version() == 216 == native.ABI_VERSION  # entry points only
    assert lib.oasr_sizeof_telephone() == ctypes.sizeof(native.Telephone) == 44
    assert lib.oasr_sizeof_telephone_args() == ctypes.sizeof(native.TelephoneArgs) == 120
    assert ("oasr_sizeof_telephone_args", native.TelephoneArgs) in native.STRUCT_SIZES and ("oasr_sizeof_telephone", native.Telephone) in native.STRUCT_SIZES
    assert (native.Telephone.LINEAR, native.Telephone.MULAW, native.Telephone.ALAW, native.Telephone.MAX_CODECS) == (0, 1, 2, 8)
    from olmoasr_amd import augment
    pol = augment.TelephoneChannel()
    assert (pol.prob, pol.codecs, pol.bandpass) == (0.3, ("mulaw", "alaw", "linear"), True)
    assert augment.TelephoneChannel(codecs=[1, "alaw", 0]).codecs == ("mulaw", "alaw", "linear")  # numbers come back as names


# ---- the training script ----------------------------------------------------------------------------------------------------------------
def test_cli_flags(tt, native):
    off = tt.parse_args([])
    assert off.telephone_prob is None and off.telephone_codecs is None and off.telephone_bandpass is None and off.telephone_policy is None
    assert all(f in tt.NATIVE_FLAGS for f in ("telephone_prob", "telephone_codecs", "telephone_bandpass"))
    for flag in ("--telephone_codecs=mulaw", "--telephone_bandpass=False"):
        with pytest.raises(SystemExit, match=flag[:flag.index("=")] + " given without --telephone_prob"):
            tt.parse_args([flag])
    on = tt.parse_args(["--telephone_prob=0.3"])
    p = on.telephone_policy
    assert (p.prob, p.codecs, p.bandpass) == (0.3, ("mulaw", "alaw", "linear"), True)
    keys = ("telephone_prob", "telephone_policy")
    assert {k: v for k, v in on.items() if k not in keys} == {k: v for k, v in off.items() if k not in keys}  # nothing else moves
    p = tt.parse_args(["--telephone_prob", "1.0", "--telephone_codecs", "mulaw,alaw,linear", "--telephone_bandpass", "True"]).telephone_policy
    assert (p.prob, p.codecs, p.bandpass) == (1.0, ("mulaw", "alaw", "linear"), True)
    p = tt.parse_args(["--telephone_prob=1", "--telephone_codecs=alaw", "--telephone_bandpass=False"]).telephone_policy
    assert (p.prob, p.codecs, p.bandpass) == (1, ("alaw",), False)
    assert tt.parse_args(["--telephone_prob=0.5", "--telephone_codecs=mulaw, mulaw ,alaw"]).telephone_policy.codecs == ("mulaw", "mulaw", "alaw")
    assert tt.parse_args(["--telephone_prob=0", "--telephone_codecs=('alaw','linear')"]).telephone_policy.codecs == ("alaw", "linear")
    for flag in ("--telephone_prob=1.5", "--telephone_prob=-1", "--telephone_prob=often", "--telephone_codecs=gsm", "--telephone_codecs=mulaw,amr",
                 "--telephone_codecs=", "--telephone_codecs=" + ",".join(["mulaw"] * 9), "--telephone_codecs=7", "--telephone_bandpass=1",
                 "--telephone_bandpass=maybe"):
        with pytest.raises(SystemExit, match="--telephone_"):
            tt.parse_args(["--telephone_prob=0.5", flag] if not flag.startswith("--telephone_prob") else [flag])
