"""Speed perturbation on the device (csrc/speed.hip through ops.speed_perturb / augment.SpeedPerturb): the expected tensors are always the host
twin's (ops.speed_perturb_host -- the same rule from the same header, checked against a numpy restatement in test_speed_perturb_cpu.py),
compared bit for bit: PCM, lengths, factor indices and both token tensors."""
import importlib.util
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
THREE_WAY = ((9, 10), (1, 1), (11, 10))
FIVE = THREE_WAY + ((2, 1), (1, 2))
GUARD = 64
SENTINEL = 0x5EA7
TS0 = 50363


def noise(B, N, seed):
    """Full-scale int16 noise with runs of +-32767 / -32768 in the first rows, so that the filter's overshoot meets the clamp."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-32768, 32768, (B, N), generator=g, dtype=torch.int64).to(torch.int16)
    x[0, :N // 2], x[0, N // 2:] = 32767, -32768
    if B > 1:
        x[1, ::2], x[1, 1::2] = 32767, -32768
    return x


def token_rows(B, S, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(TS0 - 40, TS0 + 1541, (B, S), generator=g, dtype=torch.int64)
    t[:, 0], t[:, 1], t[:, 2], t[:, -1] = TS0, TS0 + 1500, TS0 + 1501, 51864
    return t


def i32(v):
    return torch.tensor(v, dtype=torch.int32)


def both(x, nv, factors, seed, first, tokens=None):
    """The op on the device and its host twin on the same operands: ((pcm, n_out, factor, tokens...) on the CPU) x 2."""
    from olmoasr_amd import ops
    th = tuple(t.clone() for t in tokens) if tokens else ()
    td = tuple(t.to(DEV) for t in tokens) if tokens else ()
    want = ops.speed_perturb_host(x, nv, factors=factors, seed=seed, first_clip=first, tokens=th)
    got = ops.speed_perturb(x.to(DEV), nv.to(DEV), factors=factors, seed=seed, first_clip=first, tokens=td)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in got + td), tuple(want + th)


def assert_same(got, want):
    assert len(got) == len(want)
    for name, g, w in zip(("pcm", "n_out", "factor", "tokens[0]", "tokens[1]"), got, want):
        assert g.dtype == w.dtype and torch.equal(g, w), f"{name} differs from the host twin"


@pytest.mark.parametrize("N", [4096, 4099], ids=["N4096", "N4099_ragged_unaligned_rows"])
@pytest.mark.parametrize("factors", [THREE_WAY, FIVE, ((2, 1),), ((1, 2), (11, 10))], ids=["3way", "3way+2/1+1/2", "2/1", "1/2+11/10"])
def test_equals_the_host_twin(N, factors):
    B = 5
    x = noise(B, N, 100 + N)
    nv = i32([0, 1, 37, N - 1, N])
    seen = set()
    for seed, first in ((0, 0), (7, 3), (2 ** 63 + 5, 2 ** 40)):
        got, want = both(x, nv, factors, seed, first, tokens=(token_rows(B, 448, 1), token_rows(B, 448, 2)))
        assert_same(got, want)
        seen |= set(want[2].tolist())
    assert len(seen - {-1}) >= min(2, len(factors))  # more than one factor was exercised
    # lengths in the middle of the row: several tiles with audio, a tile that straddles n_out, tiles of zeros
    got, want = both(x, i32([2047, 2048, 2049, 3000, 1861]), factors, 5, 11)
    assert_same(got, want)


def test_the_real_shape():
    """N = 480000, B = 2: 235 tiles per row, the last one ragged; a clip that takes a factor and one that falls back to the copy."""
    from olmoasr_amd import ops
    N = 480000
    x = noise(2, N, 9)
    nv = i32([400000, 470000])
    # (a seed under which the first row resamples -- looked up in the host plan, not on the device)
    seed = next(s for s in range(64) if ops.speed_plan(THREE_WAY, s, 0, 400000, N)[3] in (0, 2) and ops.speed_plan(THREE_WAY, s, 1, 470000, N)[3] == -1)
    got, want = both(x, nv, THREE_WAY, seed, 0, tokens=(token_rows(2, 448, 3),))
    assert want[2].tolist()[1] == -1 and want[2].tolist()[0] in (0, 2)
    assert_same(got, want)
    got, want = both(x[:1], nv[:1], ((11, 10),), 0, 0)
    assert want[1].tolist() == [(400000 * 10) // 11]
    assert_same(got, want)


@pytest.mark.parametrize("N", [4096, 4099])
def test_guard_bands_survive(N):
    from olmoasr_amd import ops
    B = 5
    x = noise(B, N, 21)
    nv = i32([0, 1, 37, N - 1, N])
    for factors in (FIVE, ((1, 1),), ((2, 1),)):
        buf = torch.full((B, GUARD + N + GUARD), SENTINEL, dtype=torch.int16, device=DEV)
        out = buf[:, GUARD:GUARD + N]
        got, n_out, fac = ops.speed_perturb(x.to(DEV), nv.to(DEV), factors=factors, seed=4, first_clip=9, out=out)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr()
        host = buf.cpu()
        assert bool((host[:, :GUARD] == SENTINEL).all()) and bool((host[:, GUARD + N:] == SENTINEL).all()), "a guard band was written"
        want = ops.speed_perturb_host(x, nv, factors=factors, seed=4, first_clip=9)
        assert torch.equal(host[:, GUARD:GUARD + N], want[0]) and torch.equal(n_out.cpu(), want[1]) and torch.equal(fac.cpu(), want[2])
    # a strided INPUT (rows inside a wider buffer, starting at an odd sample) reads the same clips
    wide = torch.zeros(B, N + 37, dtype=torch.int16)
    wide[:, 5:5 + N] = x
    got, _, _ = ops.speed_perturb(wide.to(DEV)[:, 5:5 + N], nv.to(DEV), factors=FIVE, seed=4, first_clip=9)
    assert torch.equal(got.cpu(), ops.speed_perturb_host(x, nv, factors=FIVE, seed=4, first_clip=9)[0])


@pytest.mark.parametrize("first", [5, 2 ** 32 - 2, M64 - 1])
def test_a_batch_equals_its_clips_one_by_one(first):
    from olmoasr_amd import augment
    pol = augment.SpeedPerturb(factors=FIVE)
    B, N = 4, 4099
    x = noise(B, N, 33).to(DEV)
    nv = i32([4099, 3000, 2000, 1500]).to(DEV)
    ta, tb = token_rows(B, 64, 5).to(DEV), token_rows(B, 64, 6).to(DEV)
    one_a, one_b = ta.clone(), tb.clone()
    batch = pol.apply(x, nv, 17, first, tokens=(ta, tb))
    for b in range(B):
        single = pol.apply(x[b:b + 1], nv[b:b + 1], 17, (first + b) & M64, tokens=(one_a[b:b + 1], one_b[b:b + 1]))
        for got, want in zip(single, batch):
            assert torch.equal(got[0], want[b])
        p = pol.plan(17, (first + b) & M64, int(nv[b]), N)
        assert (int(batch[1][b]), int(batch[2][b])) == p[2:]
    assert torch.equal(one_a, ta) and torch.equal(one_b, tb)


@pytest.mark.parametrize("bad", [-1, "N+1", -2 ** 31, 2 ** 31 - 1])
def test_a_length_outside_the_contract_copies_the_row(bad):
    from olmoasr_amd import ops
    N = 4099
    bad = N + 1 if bad == "N+1" else bad
    x = noise(3, N, 41)
    tok = token_rows(3, 32, 8)
    d_tok = tok.to(DEV)
    nv = i32([3000, bad, 2000])
    got, n_out, fac = ops.speed_perturb(x.to(DEV), nv.to(DEV), factors=((11, 10),), seed=1, first_clip=0, tokens=(d_tok,))
    torch.cuda.synchronize()
    assert torch.equal(got[1].cpu(), x[1]) and int(fac[1]) == -1 and int(n_out[1]) == min(max(bad, 0), N)
    assert torch.equal(d_tok[1].cpu(), tok[1])  # its tokens are left alone
    h_tok = tok.clone()
    want = ops.speed_perturb_host(x, i32([3000, 0, 2000]), factors=((11, 10),), seed=1, first_clip=0, tokens=(h_tok,))
    for b in (0, 2):  # the neighbours are what they would have been
        assert torch.equal(got[b].cpu(), want[0][b]) and int(n_out[b]) == int(want[1][b]) and int(fac[b]) == 0
        assert torch.equal(d_tok[b].cpu(), h_tok[b])


def test_runs_on_the_current_stream():
    from olmoasr_amd import augment
    pol = augment.SpeedPerturb.preset("3way")
    B, N = 3, 4099
    x = noise(B, N, 51)
    nv = i32([4000, 3000, 3600])
    xd, nvd = x.to(DEV), nv.to(DEV)
    pol.apply(xd[:1], nvd[:1], 0, 0)  # (the ratios' tables are uploaded by the first call that meets them)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    assert s != torch.cuda.default_stream(DEV)
    with torch.cuda.stream(s):
        a = pol.apply(xd, nvd, 8, 40)
        b = pol.apply(a[0], a[1], 9, 50)  # consumes what the first call wrote: ordered by the stream alone
    s.synchronize()
    from olmoasr_amd import ops
    wa = ops.speed_perturb_host(x, nv, factors=THREE_WAY, seed=8, first_clip=40)
    wb = ops.speed_perturb_host(wa[0], wa[1], factors=THREE_WAY, seed=9, first_clip=50)
    for got, want in zip(a + b, wa + wb):
        assert torch.equal(got.cpu(), want)


def test_refusals_come_before_any_launch():
    from olmoasr_amd import augment, ops
    N = 4096
    x = torch.full((2, N), 3, dtype=torch.int16, device=DEV)
    nv = i32([N, 100]).to(DEV)
    out = torch.full((2, N), 5, dtype=torch.int16, device=DEV)
    tok = torch.full((2, 8), TS0 + 100, dtype=torch.int64, device=DEV)
    cases = [dict(pcm=x.cpu()), dict(pcm=x.float()), dict(pcm=x[0]), dict(pcm=x.t()), dict(n_valid=nv.cpu()), dict(n_valid=nv.long()), dict(n_valid=nv[:1]),
             dict(out=out.cpu()), dict(out=out[:, :N - 1]), dict(out=out.float()), dict(out=x), dict(out=x[:, 1:]), dict(tokens=(tok.int(),)),
             dict(tokens=(tok.cpu(),)), dict(tokens=(tok[:1],)), dict(tokens=(tok, tok, tok)), dict(tokens=(tok, tok[:, :4])), dict(seed=-1),
             dict(first_clip=2 ** 64), dict(ts_max=-1), dict(ts_max=2 ** 24 + 1), dict(ts_begin=-1),
             dict(factors=((4, 6),)), dict(factors=((0, 1),)), dict(factors=((33, 32),)), dict(factors=((1, 33),)), dict(factors=((3, 1),)),
             dict(factors=THREE_WAY * 3), dict(factors=())]
    for kw in cases:
        args = dict(pcm=x, n_valid=nv, factors=THREE_WAY, out=out, tokens=(tok,))
        args.update(kw)
        pcm, n_valid = args.pop("pcm"), args.pop("n_valid")
        with pytest.raises(ValueError):
            ops.speed_perturb(pcm, n_valid, **args)
    with pytest.raises(ValueError):
        augment.SpeedPerturb(factors=((6, 4),))
    empty = ops.speed_perturb(x[:0], nv[:0], factors=THREE_WAY)  # B = 0: nothing to do, not an error
    assert tuple(empty[0].shape) == (0, N) and empty[1].numel() == 0
    torch.cuda.synchronize()
    assert bool((out == 5).all()) and bool((x == 3).all()) and bool((tok == TS0 + 100).all())


# ---- the training script -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tt():
    spec = importlib.util.spec_from_file_location("tt_gpu_speed", os.path.join(ROOT, "scripts", "training", "train_timestamps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TINY = ["--model_variant=tiny", "--eff_batch_size=2", "--train_batch_size=2", "--n_synthetic=4", "--timestamps=True"]


def test_the_run_trains_counts_its_factors_and_resumes_exactly(tt, tmp_path):
    """Two steps with --speed_perturb=3way: the run trains, every step's speed_factor_counts (from the host plan) account for the step's
    clips, and after --resume from the step-1 checkpoint step 2 draws the same factors and lands on the same loss, bit for bit."""
    from olmoasr_amd import augment, synth
    common = TINY + ["--train_steps=2", "--ckpt_freq=1", "--train_log_freq=1", f"--ckpt_dir={tmp_path}", f"--run_id_dir={tmp_path}/ids",
                     "--exp_name=s", "--speed_perturb=3way", "--lr=1e-3"]
    straight = tt.main(common)
    assert [r["global_step"] for r in straight] == [1, 2] and not any(r["found_inf"] for r in straight)
    assert all(math.isfinite(r["train_loss"]) for r in straight)
    pol = augment.SpeedPerturb.preset("3way")
    for r in straight:
        first = tt.spec_offset(r["global_step"] - 1, 0, 1, 1, 0, 2)
        idx = [((r["global_step"] - 1) * 2 + j) % 4 for j in range(2)]  # the sampler's order over --n_synthetic=4
        nv = [synth.n_valid_host(synth.synth_sample(i, True)[0]) for i in idx]
        want = pol.factor_counts(0, first, nv, 480000)
        assert r["speed_factor_counts"] == want and sum(want) == 2 and len(want) == 4
    rdir = tmp_path / ("s_" + open(tmp_path / "ids" / "s.txt").read().strip())
    for f in os.listdir(rdir):  # leave the step-1 pair as the run's latest checkpoint
        if "_00000002_" in f:
            os.remove(rdir / f)
    assert sorted(f.split("_")[1] for f in os.listdir(rdir)) == ["00000001", "00000001"]
    resumed = tt.main(common + ["--resume=True"])
    assert [r["global_step"] for r in resumed] == [2]
    print(f"step 2: loss {resumed[0]['train_loss']!r} resumed vs {straight[1]['train_loss']!r} straight; factors {resumed[0]['speed_factor_counts']}")
    assert resumed[0]["speed_factor_counts"] == straight[1]["speed_factor_counts"]
    assert resumed[0]["train_loss"] == straight[1]["train_loss"]
    # without the flag the record does not mention the feature
    off = tt.main(TINY + ["--train_steps=1", "--ckpt_freq=0", f"--ckpt_dir={tmp_path}", f"--run_id_dir={tmp_path}/ids", "--exp_name=off"])
    assert "speed_factor_counts" not in off[0]
