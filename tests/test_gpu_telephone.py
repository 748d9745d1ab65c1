"""The telephone channel on the device (csrc/telephone.hip through ops.telephone / augment.TelephoneChannel): the expected tensors are always
the host twin's (ops.telephone_host -- the same rule from the same header, checked against a Python-integer restatement in
test_telephone_cpu.py), compared bit for bit: PCM and codecs."""
import importlib.util
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import telephone_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
GUARD = 64
SENTINEL = 0x5EA7
ALL = ("mulaw", "alaw", "linear")


def clips(B, N, seed, amp=12000):
    return torch.from_numpy(tc.clips(B, N, seed, amp))


def i32(v):
    return torch.tensor(v, dtype=torch.int32)


def lengths(N):
    """Inside the halo on both sides of the tile boundary at 2048, odd and even ends, the contract's ends."""
    return [0, 1, 2, 3, 37, 1950, 2047, 2048, 2049, 2150, N - 1, N]


def wide_view(t, lead, pad, fill=0):
    """``t`` [R, C] as a device view at an odd sample offset of a wider buffer: rows at addresses that are only 2-byte aligned, stride above C."""
    buf = torch.full((t.shape[0], lead + t.shape[1] + pad), fill, dtype=torch.int16, device=DEV)
    buf[:, lead:lead + t.shape[1]] = t.to(DEV)
    return buf, buf[:, lead:lead + t.shape[1]]


def assert_same(got, want):
    assert len(got) == len(want) == 2
    for name, g, w in zip(("pcm", "codec"), got, want):
        assert g.dtype == w.dtype and torch.equal(g.cpu(), w), f"{name} differs from the host twin"


@pytest.mark.parametrize("N", [4096, 4099], ids=["N4096", "N4099_ragged_unaligned_rows"])
@pytest.mark.parametrize("bandpass", [True, False], ids=["bandpass", "decimate_only"])
def test_equals_the_host_twin(N, bandpass):
    from olmoasr_amd import ops
    nv = i32(lengths(N))
    B = nv.numel()
    x = clips(B, N, 100 + N)
    _, xd = wide_view(x, 5, 32)  # 2-byte-aligned rows of a strided input
    runs = [dict(prob=1.0, codecs=[c], seed=s, first_clip=f) for c, (s, f) in zip(ALL, tc.SEEDS)]
    runs += [dict(prob=0.75, codecs=list(ALL), seed=s, first_clip=f) for s, f in tc.SEEDS]
    seen = set()
    for kw in runs:
        want = ops.telephone_host(x, nv, bandpass=bandpass, **kw)
        assert_same(ops.telephone(xd, nv.to(DEV), bandpass=bandpass, **kw), want)
        for lead in (3, 6):  # ... and 2-byte-aligned output rows on other grids than the input's: tiles that start on odd and on even samples
            _, out = wide_view(torch.zeros(B, N, dtype=torch.int16), lead, 9)
            assert_same(ops.telephone(xd, nv.to(DEV), bandpass=bandpass, out=out, **kw), want)
        seen |= set(want[1].tolist())
    assert seen == {-1, 0, 1, 2}  # every codec and copied rows occurred


@pytest.mark.parametrize("lead", [0, 1])
def test_planted_wrap_rows(lead):
    """Sums above 2^31 at a tile's first sample, inside a tile and across the boundary: +32767 by the rule, negative from a wrapped 32-bit
    accumulator."""
    from olmoasr_amd import ops
    N = 4099
    spots = (200, 2048 - 2 * lead, 2112, 3000)
    x = torch.from_numpy(np.stack([tc.wrap_row_bandpass(N, p) for p in spots]))
    nv = i32([N] * len(spots))
    want = ops.telephone_host(x, nv, prob=1.0, codecs=["linear"])
    assert [int(want[0][i, p]) for i, p in enumerate(spots)] == [32767] * len(spots)
    _, out = wide_view(torch.zeros_like(x), 8 - lead if lead else 0, 5)
    assert_same(ops.telephone(x.to(DEV), nv.to(DEV), prob=1.0, codecs=["linear"], out=out), want)
    ms = (100, 1023, 1024, 1500)
    x = torch.from_numpy(np.stack([tc.wrap_row_interpolator(N, m) for m in ms]))
    want = ops.telephone_host(x, nv, prob=1.0, codecs=["linear"], bandpass=False)
    assert [int(want[0][i, 2 * m + 1]) for i, m in enumerate(ms)] == [32767] * len(ms)
    _, out = wide_view(torch.zeros_like(x), 8 - lead if lead else 0, 5)
    assert_same(ops.telephone(x.to(DEV), nv.to(DEV), prob=1.0, codecs=["linear"], bandpass=False, out=out), want)


@pytest.mark.parametrize("codec", ALL)
def test_full_scale_impulses(codec):
    from olmoasr_amd import ops
    N, n_valid = 4099, 4001
    spots = (0, 1, 2047, 2048, n_valid - 1)
    x = torch.zeros(2 * len(spots), N, dtype=torch.int16)
    for i, p in enumerate(spots):
        x[2 * i, p], x[2 * i + 1, p] = 32767, -32768
    x[:, n_valid:] = 1234  # behind the audio: copied, and never heard by the filters
    nv = i32([n_valid] * x.shape[0])
    for bandpass in (True, False):
        want = ops.telephone_host(x, nv, prob=1.0, codecs=[codec], bandpass=bandpass)
        assert bool((want[0][:, n_valid:] == 1234).all())
        assert not bandpass or bool((want[0][:, :n_valid] != 0).any(dim=1).all())  # (without the band-pass an impulse on an odd sample is dropped)
        assert_same(ops.telephone(x.to(DEV), nv.to(DEV), prob=1.0, codecs=[codec], bandpass=bandpass), want)


def test_saturating_rows():
    from olmoasr_amd import ops
    B, N = 4, 4099
    x = clips(B, N, 3, amp=32767)
    x[0, :N // 2], x[0, N // 2:] = 32767, -32768
    x[1, ::2], x[1, 1::2] = 32767, -32768
    x[2, :] = 32767
    x[3, ::7] = -32768
    nv = i32([N, N, 3000, N])
    for codec in ALL:
        want = ops.telephone_host(x, nv, prob=1.0, codecs=[codec])
        assert_same(ops.telephone(x.to(DEV), nv.to(DEV), prob=1.0, codecs=[codec]), want)
    want = ops.telephone_host(x, nv, prob=1.0, codecs=["linear"])[0]
    assert bool(((want == 32767) | (want == -32768)).any()), "the planted case never met the clamp"


@pytest.mark.parametrize("N", [4096, 4099])
def test_guard_bands_survive(N):
    from olmoasr_amd import ops
    nv = i32(lengths(N))
    B = nv.numel()
    x = clips(B, N, 21)
    for prob in (1.0, 0.0, 0.5):
        kw = dict(prob=prob, codecs=list(ALL), seed=4, first_clip=9)
        buf, out = wide_view(torch.zeros(B, N, dtype=torch.int16), GUARD, GUARD, fill=SENTINEL)
        got = ops.telephone(x.to(DEV), nv.to(DEV), out=out, **kw)
        torch.cuda.synchronize()
        assert got[0].data_ptr() == out.data_ptr()
        host = buf.cpu()
        assert bool((host[:, :GUARD] == SENTINEL).all()) and bool((host[:, GUARD + N:] == SENTINEL).all()), "a guard band of the PCM was written"
        assert_same(got, ops.telephone_host(x, nv, **kw))
    # the report array, through the entry itself: 64 sentinel elements on either side
    from olmoasr_amd import _native as native
    import ctypes
    kw = dict(prob=1.0, codecs=list(ALL), seed=4, first_clip=9)
    xd, nvd = x.to(DEV), nv.to(DEV)
    out = torch.empty(B, N, dtype=torch.int16, device=DEV)
    codec = torch.full((GUARD + B + GUARD,), 77, dtype=torch.int32, device=DEV)
    a = native.TelephoneArgs()
    a.pcm_in, a.pcm_out, a.n_valid, a.codec_out = xd.data_ptr(), out.data_ptr(), nvd.data_ptr(), codec[GUARD:].data_ptr()
    a.ld_in = a.ld_out = N
    a.B, a.N = B, N
    a.policy, a.seed, a.first_clip = ops.telephone_policy(1.0, ALL), 4, 9
    native.call("oasr_telephone", ctypes.byref(a), native.STREAM, device=xd.device)
    torch.cuda.synchronize()
    want = ops.telephone_host(x, nv, **kw)
    t = codec.cpu()
    assert bool((t[:GUARD] == 77).all()) and bool((t[GUARD + B:] == 77).all()), "a guard band of the report was written"
    assert torch.equal(t[GUARD:GUARD + B], want[1]) and torch.equal(out.cpu(), want[0])
    a.codec_out = None  # the report is optional
    out.zero_()
    native.call("oasr_telephone", ctypes.byref(a), native.STREAM, device=xd.device)
    assert torch.equal(out.cpu(), want[0])


@pytest.mark.parametrize("first", [5, 2 ** 32 - 2, M64 - 1])
def test_a_batch_equals_its_clips_one_by_one(first):
    from olmoasr_amd import augment
    pol = augment.TelephoneChannel(prob=0.75)
    B, N = 4, 4099
    x = clips(B, N, 33).to(DEV)
    nv = i32([4099, 3000, 2000, 1500]).to(DEV)
    batch = pol.apply(x, nv, 17, first)
    for b in range(B):
        single = pol.apply(x[b:b + 1], nv[b:b + 1], 17, (first + b) & M64)
        assert torch.equal(single[0][0], batch[0][b]) and int(single[1][0]) == int(batch[1][b])
        drawn, name = pol.plan(17, (first + b) & M64)
        assert int(batch[1][b]) == (augment.TELEPHONE_CODECS.index(name) if drawn else -1)


@pytest.mark.parametrize("bad", [-1, "N+1", -2 ** 31, 2 ** 31 - 1])
def test_a_length_outside_the_contract_copies_the_row(bad):
    from olmoasr_amd import ops
    N = 4099
    bad = N + 1 if bad == "N+1" else bad
    x = clips(3, N, 41)
    kw = dict(prob=1.0, codecs=["mulaw"], seed=1, first_clip=0)
    got = ops.telephone(x.to(DEV), i32([3000, bad, 2000]).to(DEV), **kw)
    torch.cuda.synchronize()
    assert torch.equal(got[0][1].cpu(), x[1]) and int(got[1][1]) == -1
    assert_same(got, ops.telephone_host(x, i32([3000, bad, 2000]), **kw))  # the twin copies such a row too; the neighbours are what they would have been
    want = ops.telephone_host(x, i32([3000, 0, 2000]), **kw)
    assert_same(got, want)
    assert want[1].tolist() == [1, -1, 1]


def test_runs_on_the_current_stream():
    from olmoasr_amd import augment, ops
    pol = augment.TelephoneChannel(prob=1.0, codecs=("alaw",))
    B, N = 3, 4099
    x, nv = clips(B, N, 51), i32([4000, 3000, 3600])
    xd, nvd = x.to(DEV), nv.to(DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    assert s != torch.cuda.default_stream(DEV)
    with torch.cuda.stream(s):
        a = pol.apply(xd, nvd, 8, 40)
        b = pol.apply(a[0], nvd, 9, 50)  # consumes what the first call wrote: ordered by the stream alone
    s.synchronize()
    wa = ops.telephone_host(x, nv, prob=1.0, codecs=["alaw"], seed=8, first_clip=40)
    wb = ops.telephone_host(wa[0], nv, prob=1.0, codecs=["alaw"], seed=9, first_clip=50)
    assert_same(a, wa)
    assert_same(b, wb)


def test_refusals_come_before_any_launch():
    from olmoasr_amd import augment, ops
    N = 4096
    x = torch.full((2, N), 3, dtype=torch.int16, device=DEV)
    nv = i32([N, 100]).to(DEV)
    out = torch.full((2, N), 5, dtype=torch.int16, device=DEV)
    both = torch.full((2, N + 32), 3, dtype=torch.int16, device=DEV)
    cases = [dict(pcm=x.cpu()), dict(pcm=x.float()), dict(pcm=x[0]), dict(pcm=x.t()), dict(n_valid=nv.cpu()), dict(n_valid=nv.long()), dict(n_valid=nv[:1]),
             dict(out=out.cpu()), dict(out=out[:, :N - 1]), dict(out=out.float()), dict(out=both[:, 1:N + 1], pcm=both[:, :N]), dict(out=both[:, 32:], pcm=both[:, :N]),
             dict(out=x), dict(seed=-1), dict(first_clip=2 ** 64), dict(prob=-0.5), dict(prob=1.5), dict(prob=None), dict(codecs=()), dict(codecs=["gsm"]),
             dict(codecs=["mulaw"] * 9), dict(codecs="alaw"), dict(codecs=[3]), dict(bandpass=1), dict(bandpass=None)]
    for kw in cases:
        args = dict(pcm=x, n_valid=nv, prob=1.0, codecs=["mulaw"], out=out)
        args.update(kw)
        pcm, n_valid = args.pop("pcm"), args.pop("n_valid")
        with pytest.raises(ValueError):
            ops.telephone(pcm, n_valid, **args)
    with pytest.raises(ValueError):
        augment.TelephoneChannel(codecs=("mulaw", "amr"))
    empty = ops.telephone(x[:0], nv[:0], prob=1.0)  # B = 0: nothing to do, not an error
    assert tuple(empty[0].shape) == (0, N) and empty[1].numel() == 0
    torch.cuda.synchronize()
    assert bool((out == 5).all()) and bool((x == 3).all()) and bool((both == 3).all())


def test_the_real_shape():
    """B = 2, N = 480000: 235 tiles per row, the last one ragged; a drawn row and an undrawn one, chosen through the host plan."""
    from olmoasr_amd import augment, ops
    N = 480000
    pol = augment.TelephoneChannel(prob=0.5)
    x = clips(2, N, 9)
    nv = i32([400001, 470000])
    seed = next(s for s in range(256) if pol.plan(s, 0)[0] and not pol.plan(s, 1)[0])
    want = ops.telephone_host(x, nv, prob=0.5, seed=seed)
    assert want[1].tolist()[0] >= 0 and want[1].tolist()[1] == -1 and torch.equal(want[0][1], x[1]) and not torch.equal(want[0][0], x[0])
    assert_same(pol.apply(x.to(DEV), nv.to(DEV), seed), want)


# ---- the training script -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tt():
    spec = importlib.util.spec_from_file_location("tt_gpu_telephone", os.path.join(ROOT, "scripts", "training", "train_timestamps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TINY = ["--model_variant=tiny", "--eff_batch_size=2", "--train_batch_size=2", "--n_synthetic=4", "--timestamps=True"]


def test_the_run_trains_logs_its_draws_and_resumes_exactly(tt, tmp_path):
    """Two steps with --telephone_prob 1.0, a seeded synthetic noise bank and speed perturbation on: the run trains, every step's
    telephone_drawn and telephone_codec_counts are the host plan's, after --resume from the step-1 checkpoint step 2 lands on the same loss
    and counts, bit for bit, and the same run without the flag lands elsewhere and does not mention the feature."""
    from olmoasr_amd import augment
    rng = np.random.default_rng(1234)
    recordings = np.empty(3, dtype=object)
    for i, n in enumerate((16000, 48001, 30000)):
        recordings[i] = np.round(rng.standard_normal(n) * 2000).clip(-32768, 32767).astype(np.int16)
    np.save(tmp_path / "bank.npy", recordings, allow_pickle=True)
    base = TINY + ["--ckpt_freq=1", "--train_log_freq=1", f"--ckpt_dir={tmp_path}", f"--run_id_dir={tmp_path}/ids", "--speed_perturb=3way",
                   f"--noise_bank={tmp_path}/bank.npy", "--noise_prob=1.0", "--noise_snr_db=0,15", "--lr=1e-3"]
    common = base + ["--train_steps=2", "--exp_name=t", "--telephone_prob=1.0", "--telephone_codecs=mulaw,alaw,linear"]
    straight = tt.main(common)
    assert [r["global_step"] for r in straight] == [1, 2] and not any(r["found_inf"] for r in straight)
    assert all(math.isfinite(r["train_loss"]) for r in straight)
    pol = augment.TelephoneChannel(prob=1.0)
    for r in straight:
        first = tt.spec_offset(r["global_step"] - 1, 0, 1, 1, 0, 2)
        counts = pol.drawn(0, first, 2)
        assert sum(counts.values()) == 2 and r["telephone_drawn"] == 2 and r["telephone_codec_counts"] == counts
        assert r["noise_drawn"] == 2 and sum(r["speed_factor_counts"]) == 2
    rdir = tmp_path / ("t_" + open(tmp_path / "ids" / "t.txt").read().strip())
    for f in os.listdir(rdir):  # leave the step-1 pair as the run's latest checkpoint
        if "_00000002_" in f:
            os.remove(rdir / f)
    assert sorted(f.split("_")[1] for f in os.listdir(rdir)) == ["00000001", "00000001"]
    resumed = tt.main(common + ["--resume=True"])
    assert [r["global_step"] for r in resumed] == [2]
    print(f"step 2: loss {resumed[0]['train_loss']!r} resumed vs {straight[1]['train_loss']!r} straight; codecs {resumed[0]['telephone_codec_counts']}")
    for k in ("train_loss", "telephone_drawn", "telephone_codec_counts", "noise_drawn", "speed_factor_counts"):
        assert resumed[0][k] == straight[1][k]
    # the channel is heard: the same step without it lands elsewhere; and without the flag the record does not mention the feature
    plain = tt.main(base + ["--train_steps=1", "--exp_name=off"])
    assert "telephone_drawn" not in plain[0] and "telephone_codec_counts" not in plain[0]
    assert plain[0]["train_loss"] != straight[0]["train_loss"]
