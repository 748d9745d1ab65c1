"""SpecAugment on the device (csrc/specaug.hip through ops.spec_augment_ / augment.SpecAugment): the expected tensor is always the input with
the host twin's plan applied on the CPU, compared bit for bit -- cells outside the plan as int32 views, so "not written" means bit-identical."""
import importlib.util
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
GUARD = 4096
SENTINEL = 0x5EA7BEEF  # (a finite float; compared as bits)

SHAPES = [(1, 80, 3000), (3, 80, 3000), (4, 80, 257), (2, 80, 37), (2, 5, 1), (1, 1, 1000)]
POLICIES = {"LD": dict(freq_masks=2, freq_width=27, time_masks=2, time_width=100),
            "LB": dict(freq_masks=1, freq_width=27, time_masks=1, time_width=100),
            "none": dict(freq_masks=0, freq_width=27, time_masks=0, time_width=100),
            "wider_than_both_axes": dict(freq_masks=2, freq_width=1000, time_masks=2, time_width=100000),
            "8+8": dict(freq_masks=8, freq_width=27, time_masks=8, time_width=100)}


def bit_patterns(shape, seed):
    """Random 32-bit patterns read as float32 (every exponent, NaNs and infinities among them), with a NaN and a -0.0 planted."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2 ** 31, 2 ** 31, shape, generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
    flat = x.view(-1)
    flat[0] = float("nan")
    flat[flat.numel() // 2] = -0.0
    flat[-1] = float("nan")
    return x


def planned_mask(kw, seed, first_clip, shape):
    from olmoasr_amd import ops
    B, n_mels, T = shape
    mask = torch.zeros(shape, dtype=torch.bool)
    for b in range(B):
        f_iv, t_iv = ops.spec_augment_plan(**kw, seed=seed, clip=(first_clip + b) & M64, n_mels=n_mels, T=T)
        for s, w in f_iv:
            mask[b, s:s + w, :] = True
        for s, w in t_iv:
            mask[b, :, s:s + w] = True
    return mask


def guarded(x, front=GUARD, back=GUARD):
    """x on the device as a slice of a larger buffer with `front` / `back` sentinel floats around it: (buffer, view)."""
    buf = torch.full((front + x.numel() + back,), SENTINEL, dtype=torch.int32)
    buf[front:front + x.numel()] = x.view(torch.int32).reshape(-1)  # (moved as integers: the patterns stay as they are)
    buf = buf.to(DEV).view(torch.float32)
    return buf, buf[front:front + x.numel()].view(x.shape)


def check(x, got_buf, front, mask, fill):
    """got_buf: the guarded buffer after the call, on the CPU."""
    bits = got_buf.view(torch.int32)
    n = x.numel()
    assert bool((bits[:front] == SENTINEL).all()) and bool((bits[front + n:] == SENTINEL).all()), "a guard band was written"
    got = bits[front:front + n].view(x.shape)
    assert torch.equal(got[~mask], x.view(torch.int32)[~mask]), "a cell outside the plan changed"
    want = torch.tensor([fill], dtype=torch.float32).view(torch.int32)
    if math.isnan(fill):
        assert bool(got[mask].view(torch.float32).isnan().all())
    else:
        assert bool((got[mask] == want).all()), "a planned cell is not `fill`"


@pytest.mark.parametrize("policy", list(POLICIES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exactly_the_planned_cells_are_written(shape, policy):
    from olmoasr_amd import ops
    kw = POLICIES[policy]
    k = SHAPES.index(shape)
    seed, first, front = 1000 + k, 3 * k, GUARD + k % 4  # (the tensor starts at every offset from a 16-byte boundary over the shapes)
    x = bit_patterns(shape, seed)
    buf, view = guarded(x, front)
    assert view.data_ptr() % 16 == 4 * (k % 4) and view.is_contiguous()
    out = ops.spec_augment_(view, **kw, seed=seed, first_clip=first)
    assert out is view
    mask = planned_mask(kw, seed, first, shape)
    assert (policy == "none") == (not bool(mask.any()))
    check(x, buf.cpu(), front, mask, 0.0)


@pytest.mark.parametrize("shape", [SHAPES[4], SHAPES[1]], ids=["smallest", "largest"])
def test_guard_bands_survive_a_policy_that_masks_everything(shape):
    """Widths far beyond both axes with 8 + 8 masks: rows and spans reach the first and the last cell of the tensor."""
    from olmoasr_amd import ops
    kw = dict(freq_masks=8, freq_width=2 ** 31 - 1, time_masks=8, time_width=2 ** 31 - 1)
    for front in (GUARD, GUARD + 1, GUARD + 3):
        x = bit_patterns(shape, 5)
        buf, view = guarded(x, front, GUARD + 2)
        ops.spec_augment_(view, **kw, fill=-1.5, seed=9, first_clip=2 ** 64 - 1)  # (row 1 wraps to stream id 0)
        mask = planned_mask(kw, 9, 2 ** 64 - 1, shape)
        assert mask[:, 0, :].any() or mask[:, :, 0].any()
        check(x, buf.cpu(), front, mask, -1.5)


@pytest.mark.parametrize("offset", [5, 2 ** 32 - 2])
def test_a_batch_equals_its_clips_one_by_one(offset):
    from olmoasr_amd import augment
    pol = augment.SpecAugment.preset("LD")
    x = bit_patterns((4, 80, 257), 77)
    whole = pol.apply_(x.to(DEV), 31, first_clip=offset).cpu()
    parts = torch.stack([pol.apply_(x[b].to(DEV), 31, first_clip=offset + b).cpu() for b in range(4)])  # ([n_mels, T] input)
    assert torch.equal(whole.view(torch.int32), parts.view(torch.int32))
    mask = planned_mask(pol.kwargs(257), 31, offset, (4, 80, 257))
    assert torch.equal(whole.view(torch.int32)[~mask], x.view(torch.int32)[~mask]) and bool((whole[mask] == 0).all())
    assert len({mask[b].numpy().tobytes() for b in range(4)}) == 4  # (the four clips drew different masks)
    assert int(mask.sum()) == augment.masked_cells(pol, 31, offset, 4, 80, 257)


def test_the_table_row_of_the_large_seed_on_the_device():
    from olmoasr_amd import augment
    mel = torch.zeros(1, 80, 3000, device=DEV)
    augment.SpecAugment.preset("LD", fill=1.0).apply_(mel, 2 ** 63 + 5, first_clip=2 ** 40 + 3)
    want = torch.zeros(80, 3000)
    for s, w in ((44, 22), (40, 14)):
        want[s:s + w, :] = 1.0
    for s, w in ((300, 67), (2392, 62)):
        want[:, s:s + w] = 1.0
    assert torch.equal(mel.cpu()[0], want)


@pytest.mark.parametrize("fill", [0.0, -1.5, float("nan")], ids=["zero", "minus1.5", "nan"])
def test_fill_values(fill):
    from olmoasr_amd import augment
    pol = augment.SpecAugment.preset("LD", fill=fill)
    x = torch.randn(3, 80, 257, generator=torch.Generator().manual_seed(3))
    got = pol.apply_(x.to(DEV), 11, first_clip=100).cpu()
    mask = planned_mask(pol.kwargs(257), 11, 100, (3, 80, 257))
    assert mask.any() and not mask.all()
    if math.isnan(fill):
        assert torch.equal(got.isnan(), mask)
    else:
        assert bool((got[mask] == fill).all())
    assert torch.equal(got.view(torch.int32)[~mask], x.view(torch.int32)[~mask])


def test_runs_on_the_current_stream():
    from olmoasr_amd import augment
    pol = augment.SpecAugment.preset("LD")
    x = bit_patterns((3, 80, 3000), 21)
    a, b = x.to(DEV), x.to(DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    assert s != torch.cuda.default_stream(DEV)
    with torch.cuda.stream(s):
        pol.apply_(a, 8, first_clip=40)
        pol.apply_(b, 8, first_clip=40)
    s.synchronize()
    mask = planned_mask(pol.kwargs(3000), 8, 40, (3, 80, 3000))
    a, b = a.cpu(), b.cpu()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(a.view(torch.int32)[~mask], x.view(torch.int32)[~mask]) and bool((a[mask] == 0).all())


def test_refusals_come_before_any_launch():
    from olmoasr_amd import _native, augment, ops
    pol = augment.SpecAugment.preset("LD", fill=7.0)
    kw = pol.kwargs(64)
    cpu = torch.zeros(2, 80, 64)
    with pytest.raises(_native.NativeError, match="no CPU fallback"):
        pol.apply_(cpu, 0)
    bf = torch.zeros(2, 80, 64, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(_native.NativeError, match="dtype"):
        pol.apply_(bf, 0)
    base = torch.zeros(2, 64, 80, device=DEV)
    with pytest.raises(ValueError, match="contiguous"):
        pol.apply_(base.transpose(1, 2), 0)
    with pytest.raises(ValueError, match="n_mels, T"):
        ops.spec_augment_(torch.zeros(64, device=DEV), **kw)
    with pytest.raises(ValueError, match="seed"):
        ops.spec_augment_(base, **kw, seed=-1)
    with pytest.raises(ValueError, match="first_clip"):
        ops.spec_augment_(base, **kw, first_clip=2 ** 64)
    with pytest.raises(ValueError, match="masks"):
        ops.spec_augment_(base, **{**kw, "time_masks": 9})
    empty = torch.zeros(0, 80, 64, device=DEV)
    assert pol.apply_(empty, 0) is empty  # B = 0: nothing to do, not an error
    torch.cuda.synchronize()
    assert float(cpu.abs().sum()) == 0 and float(bf.float().abs().sum()) == 0 and float(base.abs().sum()) == 0


# ---- the training script -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tt():
    spec = importlib.util.spec_from_file_location("tt_gpu_spec", os.path.join(ROOT, "scripts", "training", "train_timestamps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TINY = ["--model_variant=tiny", "--eff_batch_size=2", "--train_batch_size=2", "--n_synthetic=4"]


@pytest.mark.parametrize("log_freq", [[], ["--train_log_freq=1"]], ids=["span_step", "plain_step_with_logits"])
def test_masks_reach_the_engine(tt, tmp_path, log_freq):
    """fill = NaN plants NaNs in the engine's input: the step overflows and the loss scaler skips it, on the span path (step 1 under the
    default --train_log_freq) and on the plain path alike; the same line with the default fill trains."""
    common = TINY + ["--train_steps=1", "--ckpt_freq=0", f"--ckpt_dir={tmp_path}", f"--run_id_dir={tmp_path}/ids", "--spec_augment=LD"] + log_freq
    planted = tt.main(common + ["--exp_name=nan", "--spec_fill=nan"])
    assert len(planted) == 1 and planted[0]["global_step"] == 1 and planted[0]["found_inf"] is True
    assert planted[0]["loss_scale"] == 32768.0  # (halved: the step was skipped like any overflow)
    clean = tt.main(common + ["--exp_name=clean"])
    assert len(clean) == 1 and clean[0]["found_inf"] is False and math.isfinite(clean[0]["train_loss"])
    from olmoasr_amd import augment
    cells = augment.masked_cells(augment.SpecAugment.preset("LD"), 0, tt.spec_offset(0, 0, 1, 1, 0, 2), 2, 80, 3000)
    assert clean[0]["spec_masked_cells"] == planted[0]["spec_masked_cells"] == cells > 0
    assert ("train_token_error_rate" in clean[0]) == bool(log_freq)  # (which path step 1 took)


def test_resume_reproduces_the_masks(tt, tmp_path):
    """Steps 3-4 of a 4-step run, and the same two steps after --resume from the step-2 checkpoint: the same masks (from the step counter,
    not from how long the process has lived), hence the same losses to the project's tolerance for two runs over the same samples (2e-4
    relative, tests/test_gpu_data.py; measured on an MI355X: 0 at step 3, 1.0e-5 at step 4)."""
    from olmoasr_amd import augment
    common = TINY + ["--train_steps=4", "--ckpt_freq=2", "--train_log_freq=1", f"--ckpt_dir={tmp_path}", f"--run_id_dir={tmp_path}/ids",
                     "--exp_name=r", "--spec_augment=LD", "--lr=1e-3"]
    straight = tt.main(common)
    assert [r["global_step"] for r in straight] == [1, 2, 3, 4] and not any(r["found_inf"] for r in straight)
    rdir = tmp_path / ("r_" + open(tmp_path / "ids" / "r.txt").read().strip())
    for f in os.listdir(rdir):  # leave the step-2 pair as the run's latest checkpoint
        if "_00000004_" in f:
            os.remove(rdir / f)
    assert sorted(f.split("_")[1] for f in os.listdir(rdir)) == ["00000002", "00000002"]
    resumed = tt.main(common + ["--resume=True"])
    assert [r["global_step"] for r in resumed] == [3, 4]
    pol = augment.SpecAugment.preset("LD")
    for r, s in zip(resumed, straight[2:]):
        want = augment.masked_cells(pol, 0, tt.spec_offset(r["global_step"] - 1, 0, 1, 1, 0, 2), 2, 80, 3000)
        rel = abs(r["train_loss"] - s["train_loss"]) / abs(s["train_loss"])
        print(f"step {r['global_step']}: masked cells {r['spec_masked_cells']} / {s['spec_masked_cells']} / {want}, "
              f"loss {r['train_loss']:.6f} vs {s['train_loss']:.6f} (rel {rel:.2e})")
        assert r["spec_masked_cells"] == s["spec_masked_cells"] == want > 0
        assert rel <= 2e-4
    assert len({r["spec_masked_cells"] for r in straight}) > 1  # (the steps drew different masks)
