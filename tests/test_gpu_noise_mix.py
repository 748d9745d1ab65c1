"""Noise mixing on the device (csrc/noise.hip through ops.noise_mix / augment.NoiseMix): the expected tensors are always the host twin's
(ops.noise_mix_host -- the same rule from the same header, checked against a Python-integer restatement in test_noise_mix_cpu.py), compared
bit for bit: PCM, bank rows, SNRs and gains."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
GUARD = 64
SENTINEL = 0x5EA7
SEEDS = ((0, 0), (7, 3), (2 ** 63 + 5, 2 ** 40))


def clips(B, N, seed, amp=3000):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-amp, amp + 1, (B, N), generator=g, dtype=torch.int64).to(torch.int16)


def i32(v):
    return torch.tensor(v, dtype=torch.int32)


def wide_view(t, lead, pad, fill=0):
    """``t`` [R, C] as a device view at an odd sample offset of a wider buffer: rows at addresses that are only 2-byte aligned, stride above C."""
    buf = torch.full((t.shape[0], lead + t.shape[1] + pad), fill, dtype=torch.int16, device=DEV)
    buf[:, lead:lead + t.shape[1]] = t.to(DEV)
    return buf, buf[:, lead:lead + t.shape[1]]


def assert_same(got, want):
    assert len(got) == len(want) == 4
    for name, g, w in zip(("pcm", "row", "snr", "gain"), got, want):
        assert g.dtype == w.dtype and torch.equal(g.cpu(), w), f"{name} differs from the host twin"


@pytest.mark.parametrize("N", [4096, 4099], ids=["N4096", "N4099_ragged_unaligned_rows"])
@pytest.mark.parametrize("L", [1000, 9000], ids=["L1000_wraps", "L9000"])
def test_equals_the_host_twin(N, L):
    from olmoasr_amd import ops
    B, M = 5, 3
    x = clips(B, N, 100 + N)
    bank = clips(M, L, 7 + L, amp=20000)
    _, xd = wide_view(x, 5, 32)       # 2-byte-aligned rows of a strided input
    _, bd = wide_view(bank, 3, 2)     # a bank row stride above L, rows at odd sample offsets
    seen = set()
    for lens in ([0, 1, 37, N - 1, N], [2047, 2048, 2049, 3000, N]):
        nv = i32(lens)
        for seed, first in SEEDS:
            kw = dict(prob=0.75, snr_db=(-10, 50), seed=seed, first_clip=first)
            want = ops.noise_mix_host(x, nv, bank, **kw)
            assert_same(ops.noise_mix(xd, nv.to(DEV), bd, **kw), want)
            _, out = wide_view(torch.zeros(B, N, dtype=torch.int16), 3, 9)  # ... and 2-byte-aligned output rows on another grid than the input's
            assert_same(ops.noise_mix(xd, nv.to(DEV), bd, out=out, **kw), want)
            seen |= {r >= 0 for r in want[1].tolist()}
    assert seen == {True, False}  # mixed and unmixed rows both occurred


def test_saturating_rows():
    from olmoasr_amd import ops
    B, N, L = 4, 4099, 777
    x = clips(B, N, 3, amp=32767)
    x[0, :N // 2], x[0, N // 2:] = 32767, -32768
    x[1, ::2], x[1, 1::2] = 32767, -32768
    x[2, :] = 32767
    bank = clips(2, L, 4, amp=32767)
    nv = i32([N, N, 3000, N])
    kw = dict(prob=1.0, snr_db=(-10, -5), seed=2, first_clip=8)
    want = ops.noise_mix_host(x, nv, bank, **kw)
    assert all(r >= 0 for r in want[1].tolist())
    assert bool(((want[0] != x) & ((want[0] == 32767) | (want[0] == -32768)))[3].any()), "the planted case never met the clamp"
    assert_same(ops.noise_mix(x.to(DEV), nv.to(DEV), bank.to(DEV), **kw), want)


def test_in_place_equals_out_of_place():
    from olmoasr_amd import augment
    pol = augment.NoiseMix(prob=0.75, snr_db=(0, 30))
    B, N = 6, 4099
    x, bank, nv = clips(B, N, 5).to(DEV), clips(2, 1000, 6).to(DEV), i32([N, 0, 2000, 37, N, 2049]).to(DEV)
    want = pol.apply(x, nv, bank, 3, 1)
    assert {int(r) >= 0 for r in want[1]} == {True, False}
    buf, y = wide_view(x.cpu(), 1, 6)
    got = pol.apply(y, nv, bank, 3, 1, out=y)
    assert got[0].data_ptr() == y.data_ptr()
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    assert bool((buf[:, :1] == 0).all()) and bool((buf[:, 1 + N:] == 0).all())  # nothing outside the rows moved


@pytest.mark.parametrize("N", [4096, 4099])
def test_guard_bands_survive(N):
    from olmoasr_amd import ops
    B = 5
    x, bank = clips(B, N, 21), clips(3, 1000, 22, amp=9000)
    nv = i32([0, 1, 37, N - 1, N])
    for prob in (1.0, 0.0, 0.5):
        kw = dict(prob=prob, snr_db=(0, 10), seed=4, first_clip=9)
        buf, out = wide_view(torch.zeros(B, N, dtype=torch.int16), GUARD, GUARD, fill=SENTINEL)
        got = ops.noise_mix(x.to(DEV), nv.to(DEV), bank.to(DEV), out=out, **kw)
        torch.cuda.synchronize()
        assert got[0].data_ptr() == out.data_ptr()
        host = buf.cpu()
        assert bool((host[:, :GUARD] == SENTINEL).all()) and bool((host[:, GUARD + N:] == SENTINEL).all()), "a guard band of the PCM was written"
        assert_same(got, ops.noise_mix_host(x, nv, bank, **kw))
    # the report arrays, through the entry itself: 64 sentinel elements on either side of each
    from olmoasr_amd import _native as native
    import ctypes
    kw = dict(prob=1.0, snr_db=(0, 10), seed=4, first_clip=9)
    xd, bd, nvd = x.to(DEV), bank.to(DEV), nv.to(DEV)
    out = torch.empty(B, N, dtype=torch.int16, device=DEV)
    row = torch.full((GUARD + B + GUARD,), 77, dtype=torch.int32, device=DEV)
    snr, gain = row.clone(), row.long()
    ws = torch.empty(native.lib().oasr_noise_workspace_bytes(B, N), dtype=torch.uint8, device=DEV)
    a = native.NoiseArgs()
    a.pcm_in, a.pcm_out, a.n_valid, a.bank = xd.data_ptr(), out.data_ptr(), nvd.data_ptr(), bd.data_ptr()
    a.row_out, a.snr_out, a.gain_out = row[GUARD:].data_ptr(), snr[GUARD:].data_ptr(), gain[GUARD:].data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    a.ld_in = a.ld_out = N
    a.ld_bank, a.B, a.N, a.M, a.L = 1000, B, N, 3, 1000
    a.policy, a.seed, a.first_clip = ops.noise_policy(1.0, (0, 10)), 4, 9
    native.call("oasr_noise_mix", ctypes.byref(a), native.STREAM, device=xd.device)
    torch.cuda.synchronize()
    want = ops.noise_mix_host(x, nv, bank, **kw)
    for t, w in ((row, want[1]), (snr, want[2]), (gain, want[3])):
        t = t.cpu()
        assert bool((t[:GUARD] == 77).all()) and bool((t[GUARD + B:] == 77).all()), "a guard band of a report was written"
        assert torch.equal(t[GUARD:GUARD + B], w.to(t.dtype))
    assert torch.equal(out.cpu(), want[0])


@pytest.mark.parametrize("first", [5, 2 ** 32 - 2, M64 - 1])
def test_a_batch_equals_its_clips_one_by_one(first):
    from olmoasr_amd import augment
    pol = augment.NoiseMix(prob=0.75, snr_db=(-5, 40))
    B, N = 4, 4099
    x, bank = clips(B, N, 33).to(DEV), clips(5, 3001, 34).to(DEV)
    nv = i32([4099, 3000, 2000, 1500]).to(DEV)
    batch = pol.apply(x, nv, bank, 17, first)
    for b in range(B):
        single = pol.apply(x[b:b + 1], nv[b:b + 1], bank, 17, (first + b) & M64)
        for got, want in zip(single, batch):
            assert torch.equal(got[0], want[b])
        drawn, m, _, s = pol.plan(17, (first + b) & M64, 5, 3001)
        assert (int(batch[1][b]), int(batch[2][b])) == ((m, s) if drawn else (-1, -128))


@pytest.mark.parametrize("bad", [-1, "N+1", -2 ** 31, 2 ** 31 - 1])
def test_a_length_outside_the_contract_copies_the_row(bad):
    from olmoasr_amd import ops
    N = 4099
    bad = N + 1 if bad == "N+1" else bad
    x, bank = clips(3, N, 41), clips(2, 1000, 42)
    kw = dict(prob=1.0, snr_db=(5, 20), seed=1, first_clip=0)
    got = ops.noise_mix(x.to(DEV), i32([3000, bad, 2000]).to(DEV), bank.to(DEV), **kw)
    torch.cuda.synchronize()
    assert torch.equal(got[0][1].cpu(), x[1]) and (int(got[1][1]), int(got[2][1]), int(got[3][1])) == (-1, -128, 0)
    assert_same(got, ops.noise_mix_host(x, i32([3000, bad, 2000]), bank, **kw))  # the twin copies such a row too; the neighbours are what they would have been
    want = ops.noise_mix_host(x, i32([3000, 0, 2000]), bank, **kw)
    assert_same(got, want)
    assert int(want[1][0]) >= 0 and int(want[1][2]) >= 0


def test_runs_on_the_current_stream():
    from olmoasr_amd import augment, ops
    pol = augment.NoiseMix(prob=1.0, snr_db=(5, 20))
    B, N = 3, 4099
    x, bank, nv = clips(B, N, 51), clips(2, 1500, 52), i32([4000, 3000, 3600])
    xd, bd, nvd = x.to(DEV), bank.to(DEV), nv.to(DEV)
    pol.apply(xd[:1], nvd[:1], bd, 0, 0)  # (the workspace is leased by the first call)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    assert s != torch.cuda.default_stream(DEV)
    with torch.cuda.stream(s):
        a = pol.apply(xd, nvd, bd, 8, 40)
        b = pol.apply(a[0], nvd, bd, 9, 50)  # consumes what the first call wrote: ordered by the stream alone
    s.synchronize()
    wa = ops.noise_mix_host(x, nv, bank, prob=1.0, snr_db=(5, 20), seed=8, first_clip=40)
    wb = ops.noise_mix_host(wa[0], nv, bank, prob=1.0, snr_db=(5, 20), seed=9, first_clip=50)
    assert_same(a, wa)
    assert_same(b, wb)


def test_refusals_come_before_any_launch():
    from olmoasr_amd import augment, ops
    N, L = 4096, 1000
    x = torch.full((2, N), 3, dtype=torch.int16, device=DEV)
    nv = i32([N, 100]).to(DEV)
    out = torch.full((2, N), 5, dtype=torch.int16, device=DEV)
    bank = torch.full((2, L), 7, dtype=torch.int16, device=DEV)
    both = torch.full((2, N + 32), 3, dtype=torch.int16, device=DEV)
    cases = [dict(pcm=x.cpu()), dict(pcm=x.float()), dict(pcm=x[0]), dict(pcm=x.t()), dict(n_valid=nv.cpu()), dict(n_valid=nv.long()), dict(n_valid=nv[:1]),
             dict(bank=bank.cpu()), dict(bank=bank.float()), dict(bank=bank[0]), dict(bank=bank.t()), dict(bank=bank[:0]), dict(bank=bank[:, :0]),
             dict(out=out.cpu()), dict(out=out[:, :N - 1]), dict(out=out.float()), dict(out=both[:, 1:N + 1], pcm=both[:, :N]), dict(out=both[:, 32:], pcm=both[:, :N]),
             dict(out=bank.expand(2, L), pcm=x[:, :L]), dict(seed=-1), dict(first_clip=2 ** 64), dict(prob=-0.5), dict(prob=1.5), dict(prob=None),
             dict(snr_db=(-11, 0)), dict(snr_db=(0, 51)), dict(snr_db=(20, 5)), dict(snr_db=(5.0, 20.0)), dict(snr_db=7)]
    for kw in cases:
        args = dict(pcm=x, n_valid=nv, bank=bank, prob=1.0, snr_db=(5, 20), out=out)
        args.update(kw)
        pcm, n_valid, bk = args.pop("pcm"), args.pop("n_valid"), args.pop("bank")
        with pytest.raises(ValueError):
            ops.noise_mix(pcm, n_valid, bk, **args)
    with pytest.raises(ValueError):
        augment.NoiseMix(snr_db=(6, 5))
    empty = ops.noise_mix(x[:0], nv[:0], bank, prob=1.0, snr_db=(5, 20))  # B = 0: nothing to do, not an error
    assert tuple(empty[0].shape) == (0, N) and empty[1].numel() == 0
    torch.cuda.synchronize()
    assert bool((out == 5).all()) and bool((x == 3).all()) and bool((both == 3).all()) and bool((bank == 7).all())


def test_the_real_shape():
    """B = 2, N = L = 480000: 235 tiles per row, the last one ragged; a drawn row and an undrawn one, chosen through the host plan.  Then one
    clip of 600001 samples: 293 tiles, more partial sums than a workgroup has threads, over a bank row that wraps."""
    from olmoasr_amd import augment, ops
    N = 480000
    pol = augment.NoiseMix(prob=0.5, snr_db=(5, 20))
    x, bank = clips(2, N, 9, amp=12000), clips(2, N, 10, amp=32767)
    nv = i32([400001, 470000])
    seed = next(s for s in range(256) if pol.plan(s, 0, 2, N)[0] and pol.plan(s, 0, 2, N)[2] % 8 and not pol.plan(s, 1, 2, N)[0])
    want = ops.noise_mix_host(x, nv, bank, prob=0.5, snr_db=(5, 20), seed=seed)
    assert want[1].tolist()[0] >= 0 and want[1].tolist()[1] == -1
    assert_same(pol.apply(x.to(DEV), nv.to(DEV), bank.to(DEV), seed), want)
    N = 600001
    x, nv = clips(1, N, 11, amp=12000), i32([N])
    want = ops.noise_mix_host(x, nv, bank, prob=1.0, snr_db=(5, 20), seed=3)
    assert want[1].tolist()[0] >= 0
    assert_same(ops.noise_mix(x.to(DEV), nv.to(DEV), bank.to(DEV), prob=1.0, snr_db=(5, 20), seed=3), want)


# ---- the training script -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tt():
    spec = importlib.util.spec_from_file_location("tt_gpu_noise", os.path.join(ROOT, "scripts", "training", "train_timestamps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TINY = ["--model_variant=tiny", "--eff_batch_size=2", "--train_batch_size=2", "--n_synthetic=4", "--timestamps=True"]


def test_the_run_trains_logs_its_draws_and_resumes_exactly(tt, tmp_path):
    """Two steps with a seeded synthetic bank, --noise_prob 1.0 and speed perturbation on: the run trains, every step's noise_drawn and
    noise_snr_db_mean are the host plan's, and after --resume from the step-1 checkpoint step 2 lands on the same loss and counts, bit for
    bit."""
    from olmoasr_amd import augment
    rng = np.random.default_rng(1234)
    recordings = np.empty(3, dtype=object)
    for i, n in enumerate((16000, 48001, 30000)):
        recordings[i] = np.round(rng.standard_normal(n) * 2000).clip(-32768, 32767).astype(np.int16)
    np.save(tmp_path / "bank.npy", recordings, allow_pickle=True)
    common = TINY + ["--train_steps=2", "--ckpt_freq=1", "--train_log_freq=1", f"--ckpt_dir={tmp_path}", f"--run_id_dir={tmp_path}/ids",
                     "--exp_name=n", "--speed_perturb=3way", f"--noise_bank={tmp_path}/bank.npy", "--noise_prob=1.0", "--noise_snr_db=0,15", "--lr=1e-3"]
    straight = tt.main(common)
    assert [r["global_step"] for r in straight] == [1, 2] and not any(r["found_inf"] for r in straight)
    assert all(math.isfinite(r["train_loss"]) for r in straight)
    pol = augment.NoiseMix(prob=1.0, snr_db=(0, 15))
    for r in straight:
        first = tt.spec_offset(r["global_step"] - 1, 0, 1, 1, 0, 2)
        count, total = pol.drawn(0, first, 2, 3, 48001)
        assert count == 2 and r["noise_drawn"] == 2 and r["noise_snr_db_mean"] == round(total / 2, 3) and 0 <= r["noise_snr_db_mean"] <= 15
        assert sum(r["speed_factor_counts"]) == 2
    rdir = tmp_path / ("n_" + open(tmp_path / "ids" / "n.txt").read().strip())
    for f in os.listdir(rdir):  # leave the step-1 pair as the run's latest checkpoint
        if "_00000002_" in f:
            os.remove(rdir / f)
    assert sorted(f.split("_")[1] for f in os.listdir(rdir)) == ["00000001", "00000001"]
    resumed = tt.main(common + ["--resume=True"])
    assert [r["global_step"] for r in resumed] == [2]
    print(f"step 2: loss {resumed[0]['train_loss']!r} resumed vs {straight[1]['train_loss']!r} straight; SNR mean {resumed[0]['noise_snr_db_mean']}")
    for k in ("train_loss", "noise_drawn", "noise_snr_db_mean", "speed_factor_counts"):
        assert resumed[0][k] == straight[1][k]
    # the noise is heard: the same two steps without it land elsewhere; and without the flag the record does not mention the feature
    plain = tt.main(TINY + ["--train_steps=1", "--ckpt_freq=0", "--train_log_freq=1", f"--ckpt_dir={tmp_path}", f"--run_id_dir={tmp_path}/ids", "--exp_name=off",
                            "--speed_perturb=3way", "--lr=1e-3"])
    assert "noise_drawn" not in plain[0] and "noise_snr_db_mean" not in plain[0]
    assert plain[0]["train_loss"] != straight[0]["train_loss"]
