"""Reverberation on the device (csrc/reverb.hip through ops.reverb / augment.Reverb): the expected tensors are always the host twin's
(ops.reverb_host -- the same rule from the same header, held to two restatements in test_reverb_cpu.py), compared bit for bit.  The kernel
computes the sum on the int8 matrix cores from byte digits, 256 outputs to a tile and 4096 to a workgroup; the cases below are chosen against
that: every tap position of an 81-tap response planted alone (every Toeplitz diagonal, every 16-tap block, the 64-tap k-step boundary), the
accumulators' extremes at 8192 taps, the digit boundaries of x, and lengths around a tile and a workgroup."""
import importlib.util
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reverb_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
SENTINEL = 0x5EA7
TILE, WG = 256, 4096  # outputs of one MFMA tile / of one workgroup (csrc/reverb.hip)


def t16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int16))


def i32(v):
    return torch.tensor(np.asarray(v), dtype=torch.int32)


def wide_view(t, lead, pad, fill=0):
    """``t`` [R, C] as a device view at an odd sample offset of a wider buffer: rows at addresses that are only 2-byte aligned, stride above C."""
    buf = torch.full((t.shape[0], lead + t.shape[1] + pad), fill, dtype=torch.int16, device=DEV)
    buf[:, lead:lead + t.shape[1]] = t.to(DEV)
    return buf, buf[:, lead:lead + t.shape[1]]


def both(x, nv, bank, delay, **kw):
    """(device result on the CPU, host twin's result) for CPU operands."""
    from olmoasr_amd import ops
    x, nv, bank, delay = t16(x), i32(nv), t16(bank), i32(delay)
    want = ops.reverb_host(x, nv, bank, delay, **kw)
    got = ops.reverb(x.to(DEV), nv.to(DEV), bank.to(DEV), delay.to(DEV), **kw)
    return tuple(t.cpu() for t in got), want


def assert_same(got, want):
    assert len(got) == len(want) == 2
    for name, g, w in zip(("pcm", "row"), got, want):
        assert g.dtype == w.dtype and torch.equal(g.cpu(), w), f"{name} differs from the host twin"


@pytest.mark.parametrize("K", [1, 15, 16, 17, 63, 64, 65, 81, 1000, 4096, 8192])
def test_equals_the_host_twin(K):
    B, N, R = 4, 20003, 3
    x = rc.clips(B, N, 100 + K, amp=32767)
    bank, delay = rc.quantized_bank(R, K, 7 + K)
    seen = set()
    for nv, seed, first in (([N, 12345, N - 1, 8192], 0, 0), ([4097, N, 300, N], 2 ** 63 + 5, 2 ** 40)):
        got, want = both(x, nv, bank, delay, prob=0.8, seed=seed, first_clip=first)
        assert_same(got, want)
        seen |= {r >= 0 for r in want[1].tolist()}
    assert True in seen


@pytest.mark.parametrize("value", [32639, -32639, 1])
def test_planted_single_taps(value):
    """K = 81: one tap at each k = 0 .. 80 in turn against an asymmetric ramp: every b - j, every block c, the 64-wide k-step boundary.  The
    81 responses are the rows of one bank; 81 * 6 clips of the same ramp at prob = 1 draw every row (asserted), delays vary by row."""
    from olmoasr_amd import ops
    K, N = 81, 4500  # two workgroups, the second ragged
    bank = np.concatenate([rc.planted(K, k, value) for k in range(K)])
    delay = np.array([(7 * k) % K for k in range(K)], dtype=np.int32)
    B = 6 * K
    x = np.tile(rc.ramp(N), (B, 1))
    got, want = both(x, [N] * B, bank, delay, prob=1.0, seed=11)
    assert set(want[1].tolist()) == set(range(K))
    assert_same(got, want)
    # ... and the twin's answer is the shifted ramp itself, scaled: a planted tap is a pure delay
    r = int(want[1][0])
    shift = int(delay[r]) - r
    n = np.arange(N)
    src = np.where((n + shift >= 0) & (n + shift < N), rc.ramp(N).astype(np.int64)[np.clip(n + shift, 0, N - 1)], 0)
    assert want[0][0].tolist() == np.clip((src * value + 16384) >> 15, -32768, 32767).tolist()


@pytest.mark.parametrize("taps", ["all_max", "alternating"])
def test_accumulator_extremes(taps):
    """K = 8192: all taps 32639 (and +-32639 alternating) against x == -32768, == 32767 and the digit boundaries -129 / 128 / 255: the three
    int32 accumulators at their largest, and the output clamp on both sides."""
    K, N = 8192, 12000
    bank = np.full((1, K), 32639, dtype=np.int16)
    if taps == "alternating":
        bank[0, 1::2] = -32639
    n = np.arange(N)
    x = np.stack([np.full(N, -32768), np.full(N, 32767), np.full(N, -129), np.full(N, 128), np.full(N, 255),
                  np.where(n & 1, -32768, 32767), np.where(n & 1, 32767, -32768), np.where(n & 1, 255, -129)]).astype(np.int16)
    got, want = both(x, [N] * len(x), bank, [K // 2], prob=1.0)
    assert_same(got, want)
    y = want[0]
    if taps == "all_max":
        assert int(y[0].min()) == -32768 and int(y[1].max()) == 32767
    else:
        assert int(y[5].max()) == 32767 and int(y[5].min()) == -32768 and int(y[6].max()) == 32767 and int(y[6].min()) == -32768


def test_contract_clamps():
    from olmoasr_amd import ops
    K, N = 100, 5000
    x = rc.clips(3, N, 5, amp=20000)
    bank, _ = rc.quantized_bank(1, K, 6)
    wild, tame = bank.copy(), bank.copy()
    wild[0, 3], wild[0, 50], wild[0, 99] = 32767, -32768, 32640
    tame[0, 3], tame[0, 50], tame[0, 99] = 32639, -32639, 32639
    for d_wild, d_tame in ((-5, 0), (K + 5, K - 1), (-2 ** 31, 0), (2 ** 31 - 1, K - 1)):
        got, want = both(x, [N, 777, N - 1], wild, [d_wild], prob=1.0, seed=2)
        assert_same(got, want)
        got2, _ = both(x, [N, 777, N - 1], tame, [d_tame], prob=1.0, seed=2)
        assert torch.equal(got[0], got2[0])


@pytest.mark.parametrize("K", [81, 1000])
def test_edges(K):
    """n_valid around a tile and a workgroup, 1 and N; 0, -1 and N + 1 are copies with row -1; delay 0 and K - 1; what lies behind n_valid is
    copied and is not heard."""
    N = 2 * WG + 700
    lens = [1, TILE - 1, TILE, TILE + 1, WG - 1, WG, WG + 1, N, 0, -1, N + 1]
    x = rc.clips(len(lens), N, 40 + K, amp=30000)  # (random samples behind n_valid: garbage that must not reach the output)
    bank, _ = rc.quantized_bank(2, K, 41 + K)
    for delay in ([0, K - 1], [K - 1, 0]):
        got, want = both(x, lens, bank, delay, prob=1.0, seed=9)
        assert_same(got, want)
        assert want[1].tolist()[-3:] == [-1, -1, -1] and min(want[1].tolist()[:-3]) >= 0
        assert torch.equal(got[0][-3:], t16(x)[-3:])
        for b, nv in enumerate(lens[:-3]):
            assert torch.equal(got[0][b, nv:], t16(x)[b, nv:])
        quiet = x.copy()
        for b, nv in enumerate(lens[:-3]):
            quiet[b, nv:] = 0
        got_q, _ = both(quiet, lens, bank, delay, prob=1.0, seed=9)
        for b, nv in enumerate(lens[:-3]):
            assert torch.equal(got[0][b, :nv], got_q[0][b, :nv])


def test_layout_views_and_guard_bands():
    """Rows through views at odd sample offsets with ld > N, input, bank and output each on a grid of its own; the samples around the output
    rows survive."""
    from olmoasr_amd import ops
    B, N, R, K = 3, 4099, 2, 65
    x, (bank, delay) = rc.clips(B, N, 77, amp=25000), rc.quantized_bank(R, K, 78)
    nv = i32([N, 2049, 4097])
    _, xd = wide_view(t16(x), 5, 32, fill=1234)
    _, bd = wide_view(t16(bank), 3, 2, fill=-77)
    for seed, first in ((0, 0), (7, 3), (2 ** 63 + 5, 2 ** 40)):
        kw = dict(prob=0.75, seed=seed, first_clip=first)
        want = ops.reverb_host(t16(x), nv, t16(bank), i32(delay), **kw)
        assert_same(ops.reverb(xd, nv.to(DEV), bd, i32(delay).to(DEV), **kw), want)
        buf, out = wide_view(torch.zeros(B, N, dtype=torch.int16), 3, 9, fill=SENTINEL)
        res = ops.reverb(xd, nv.to(DEV), bd, i32(delay).to(DEV), out=out, **kw)
        assert res[0] is out
        assert_same(res, want)
        assert bool((buf[:, :3] == SENTINEL).all()) and bool((buf[:, 3 + N:] == SENTINEL).all())


@pytest.mark.parametrize("first", [5, 2 ** 32 - 2, M64 - 1])
def test_a_batch_equals_its_clips_one_by_one(first):
    from olmoasr_amd import ops
    B, N, R, K = 6, 5003, 4, 300
    x, (bank, delay) = t16(rc.clips(B, N, 21)).to(DEV), rc.quantized_bank(R, K, 22)
    bank, delay = t16(bank).to(DEV), i32(delay).to(DEV)
    nv = i32([N, 4096, 17, N - 1, 2000, N]).to(DEV)
    seed = next(s for s in range(256) if {ops.reverb_plan(0.6, s, (first + b) & M64, R)[0] for b in range(B)} == {True, False})  # (host plan)
    whole = ops.reverb(x, nv, bank, delay, prob=0.6, seed=seed, first_clip=first)
    for b in range(B):
        one = ops.reverb(x[b:b + 1], nv[b:b + 1], bank, delay, prob=0.6, seed=seed, first_clip=(first + b) & M64)
        assert torch.equal(one[0][0], whole[0][b]) and int(one[1][0]) == int(whole[1][b])
    assert {r >= 0 for r in whole[1].tolist()} == {True, False}


def test_probability_ends_and_the_policy():
    from olmoasr_amd import augment, ops
    B, N = 5, 4500
    x, (bank, delay) = t16(rc.clips(B, N, 31)), rc.quantized_bank(2, 40, 32)
    args = (x.to(DEV), i32([N] * B).to(DEV), t16(bank).to(DEV), i32(delay).to(DEV))
    y, row = augment.Reverb(prob=0.0).apply(*args, seed=3)
    assert row.tolist() == [-1] * B and torch.equal(y.cpu(), x)
    y, row = augment.Reverb(prob=1.0).apply(*args, seed=3, first_clip=8)
    want = ops.reverb_host(x, i32([N] * B), t16(bank), i32(delay), prob=1.0, seed=3, first_clip=8)
    assert_same((y, row), want)
    assert min(row.tolist()) >= 0 and row.tolist() == [augment.Reverb(prob=1.0).plan(3, 8 + b, 2)[1] for b in range(B)]


def test_refusals_come_before_any_launch():
    from olmoasr_amd import ops
    N, K = 4096, 100
    x = torch.full((2, N), 3, dtype=torch.int16, device=DEV)
    nv, delay = i32([N, 100]).to(DEV), i32([0, 5]).to(DEV)
    out = torch.full((2, N), 5, dtype=torch.int16, device=DEV)
    bank = torch.full((2, K), 7, dtype=torch.int16, device=DEV)
    wide = torch.full((2, N + 32), 3, dtype=torch.int16, device=DEV)
    cases = [dict(pcm=x.cpu()), dict(pcm=x.float()), dict(pcm=x[0]), dict(pcm=x.t()), dict(n_valid=nv.cpu()), dict(n_valid=nv.long()), dict(n_valid=nv[:1]),
             dict(delay=delay.cpu()), dict(delay=delay.long()), dict(delay=delay[:1]), dict(bank=bank.cpu()), dict(bank=bank.float()), dict(bank=bank[0]),
             dict(bank=bank.t()), dict(bank=bank[:, :0]), dict(bank=torch.zeros(2, 8193, dtype=torch.int16, device=DEV)),
             dict(out=out.cpu()), dict(out=out[:, :N - 1]), dict(out=out.float()), dict(out=x),  # in place is not offered
             dict(out=wide[:, 1:N + 1], pcm=wide[:, :N]), dict(out=wide[:, 32:], pcm=wide[:, :N]), dict(out=bank.expand(2, K), pcm=x[:, :K]),
             dict(seed=-1), dict(first_clip=2 ** 64), dict(prob=-0.5), dict(prob=1.5), dict(prob=None)]
    for kw in cases:
        args = dict(pcm=x, n_valid=nv, bank=bank, delay=delay, prob=1.0, out=out)
        args.update(kw)
        pcm, n_valid, bk, dl = args.pop("pcm"), args.pop("n_valid"), args.pop("bank"), args.pop("delay")
        with pytest.raises(ValueError):
            ops.reverb(pcm, n_valid, bk, dl, **args)
    empty = ops.reverb(x[:0], nv[:0], bank, delay, prob=1.0)  # B = 0: nothing to do, not an error
    assert tuple(empty[0].shape) == (0, N) and empty[1].numel() == 0
    torch.cuda.synchronize()
    assert bool((out == 5).all()) and bool((x == 3).all()) and bool((wide == 3).all()) and bool((bank == 7).all())


def test_a_bad_workspace_is_refused_before_any_launch():
    """What only the device entry checks: the workspace (null, below oasr_reverb_workspace_bytes, not 16-byte aligned) is OASR_EINVAL."""
    import ctypes
    from olmoasr_amd import _native, ops
    N, K = 4096, 100
    x = torch.full((2, N), 3, dtype=torch.int16, device=DEV)
    out = torch.full((2, N), 5, dtype=torch.int16, device=DEV)
    bank = torch.full((2, K), 7, dtype=torch.int16, device=DEV)
    a, _, row, keep = ops._reverb_args(x, i32([N, 100]).to(DEV), bank, i32([0, 5]).to(DEV), 1.0, 0, 0, out, True)
    row.fill_(99)
    need = _native.lib().oasr_reverb_workspace_bytes(2, K)
    assert need == 16 + 2 * 2 * 2048
    ws = torch.zeros(need + 32, dtype=torch.uint8, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for ptr, size in ((None, need), (ws.data_ptr(), need - 1), (ws.data_ptr() + 8, need), (ws.data_ptr(), 0)):
        a.workspace, a.workspace_bytes = ptr, size
        assert _native.lib().oasr_reverb(ctypes.byref(a), stream) == -1 and "workspace" in _native.lib().oasr_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == 5).all()) and row.tolist() == [99, 99]
    a.workspace, a.workspace_bytes = ws.data_ptr(), need  # ... and exactly enough is enough
    assert _native.lib().oasr_reverb(ctypes.byref(a), stream) == 0
    torch.cuda.synchronize()
    assert min(row.tolist()) >= 0 and bool((ws[need:] == 0).all())


# ---- the training script -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tt():
    spec = importlib.util.spec_from_file_location("tt_gpu_reverb", os.path.join(ROOT, "scripts", "training", "train_timestamps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TINY = ["--model_variant=tiny", "--eff_batch_size=2", "--train_batch_size=2", "--n_synthetic=4", "--timestamps=True"]


def test_the_run_trains_logs_its_draws_and_resumes_exactly(tt, tmp_path):
    """Two steps with speed perturbation, reverberation, noise mixing and SpecAugment together: the run trains, every step's reverb_drawn is
    the host plan's, and after --resume from the step-1 checkpoint step 2 lands on the same loss and counts, bit for bit."""
    from olmoasr_amd import augment
    rng = np.random.default_rng(1234)
    recordings = np.empty(2, dtype=object)
    for i, n in enumerate((16000, 30000)):
        recordings[i] = np.round(rng.standard_normal(n) * 2000).clip(-32768, 32767).astype(np.int16)
    np.save(tmp_path / "noise.npy", recordings, allow_pickle=True)
    rirs = np.empty(3, dtype=object)
    for i, h in enumerate(rc.responses(3, 1600, 5)):
        rirs[i] = h[:1600 - 300 * i]
    np.save(tmp_path / "rir.npy", rirs, allow_pickle=True)
    common = TINY + ["--train_steps=2", "--ckpt_freq=1", "--train_log_freq=1", f"--ckpt_dir={tmp_path}", f"--run_id_dir={tmp_path}/ids",
                     "--exp_name=r", "--speed_perturb=3way", f"--rir_bank={tmp_path}/rir.npy", "--reverb_prob=1.0", f"--noise_bank={tmp_path}/noise.npy",
                     "--noise_prob=1.0", "--noise_snr_db=10,20", "--spec_augment=LB", "--lr=1e-3"]
    straight = tt.main(common)
    assert [r["global_step"] for r in straight] == [1, 2] and not any(r["found_inf"] for r in straight)
    assert all(math.isfinite(r["train_loss"]) for r in straight)
    pol = augment.Reverb(prob=1.0)
    for r in straight:
        first = tt.spec_offset(r["global_step"] - 1, 0, 1, 1, 0, 2)
        assert r["reverb_drawn"] == pol.drawn(0, first, 2, 3) == 2
        assert r["noise_drawn"] == 2 and sum(r["speed_factor_counts"]) == 2 and r["spec_masked_cells"] > 0
    rdir = tmp_path / ("r_" + open(tmp_path / "ids" / "r.txt").read().strip())
    for f in os.listdir(rdir):  # leave the step-1 pair as the run's latest checkpoint
        if "_00000002_" in f:
            os.remove(rdir / f)
    assert sorted(f.split("_")[1] for f in os.listdir(rdir)) == ["00000001", "00000001"]
    resumed = tt.main(common + ["--resume=True"])
    assert [r["global_step"] for r in resumed] == [2]
    print(f"step 2: loss {resumed[0]['train_loss']!r} resumed vs {straight[1]['train_loss']!r} straight")
    for k in ("train_loss", "reverb_drawn", "noise_drawn", "noise_snr_db_mean", "speed_factor_counts", "spec_masked_cells"):
        assert resumed[0][k] == straight[1][k]
    # the room is heard: the same step without it lands elsewhere; and without the flag the record does not mention the feature
    dry = [a for a in common if "rir_bank" not in a and "reverb_prob" not in a and "exp_name" not in a and "train_steps" not in a and "ckpt_freq" not in a]
    plain = tt.main(dry + ["--train_steps=1", "--ckpt_freq=0", "--exp_name=dry"])
    assert "reverb_drawn" not in plain[0]
    assert plain[0]["train_loss"] != straight[0]["train_loss"]
