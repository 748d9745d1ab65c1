"""CPU half of SpecAugment (csrc/specaug_core.h through its host twin, oasr_spec_augment_plan): known answers, the rule written out again
here in plain Python, the invariants of every interval, the distribution of the widths, the argument checks that fire before any launch, and
the training script's flags and stream-id rule."""
import ctypes
import importlib.util
import math
import os
import random

import pytest

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
def tt():
    spec = importlib.util.spec_from_file_location("tt_spec_cpu", os.path.join(ROOT, "scripts", "training", "train_timestamps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the rule, from the text of include/oasr.h; nothing below is imported from the package --------------------------------------
def mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def rule(seed, clip, freq_masks, freq_width, time_masks, time_width, n_mels, T):
    h = mix(mix(seed) ^ clip)
    out = []
    for kind, n, W, L in ((1, freq_masks, freq_width, n_mels), (2, time_masks, time_width, T)):
        W = min(W, L)
        iv = []
        for i in range(n):
            width = mix(h ^ ((kind << 16) | (i << 1))) % (W + 1)
            start = mix(h ^ ((kind << 16) | (i << 1) | 1)) % (L - width + 1)
            iv.append((start, width))
        out.append(iv)
    return tuple(out)


def cases():
    """(seed, clip, freq_masks, freq_width, time_masks, time_width, time_ratio, n_mels, T): every edge the rule has, then seeded draws."""
    edge_ids = [0, 1, 7, 2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 3, 2 ** 63, 2 ** 63 + 5, 2 ** 64 - 1]
    out = []
    policies = [(2, 27, 2, 100, 1.0), (1, 27, 1, 100, 1.0), (0, 27, 0, 100, 1.0), (2, 0, 2, 0, 1.0), (8, 27, 8, 100, 1.0),
                (3, 1000, 4, 100000, 1.0), (2, 27, 2, 100, 0.1), (2, 27, 2, 100, 0.0), (8, 2 ** 31 - 1, 8, 2 ** 31 - 1, 0.5)]
    shapes = [(1, 1), (1, 3000), (80, 1), (5, 1), (1, 1000), (80, 37), (80, 257), (80, 3000), (128, 3000)]
    for k, (pol, shape) in enumerate((p, s) for p in policies for s in shapes):
        out.append((edge_ids[k % len(edge_ids)], edge_ids[(3 * k + 1) % len(edge_ids)], *pol, *shape))
    for s in edge_ids:
        for c in edge_ids:
            out.append((s, c, 2, 27, 2, 100, 1.0, 80, 3000))
    rng = random.Random(20190418)
    while len(out) < 2400:
        big = rng.random() < 0.3
        seed = rng.getrandbits(64) | (1 << 63) if big else rng.getrandbits(rng.choice((8, 32, 64)))
        clip = rng.choice((rng.getrandbits(64) | (1 << 63), 2 ** 32 + rng.randint(-4, 4), rng.getrandbits(20)))
        n_mels, T = rng.choice((1, 2, 5, 80, 128)), rng.choice((1, 2, 37, 257, 1000, 1500, 3000))
        out.append((seed, clip, rng.randint(0, 8), rng.choice((0, 1, 27, 200)), rng.randint(0, 8), rng.choice((0, 1, 3, 100, 5000)),
                    rng.choice((1.0, 1.0, 0.5, 0.1, 0.0)), n_mels, T))
    return out


def run_case(augment, case):
    seed, clip, fm, fw, tm, tw, ratio, n_mels, T = case
    pol = augment.SpecAugment(freq_masks=fm, freq_width=fw, time_masks=tm, time_width=tw, time_ratio=ratio)
    cap = min(tw, int(math.floor(ratio * T)))
    return augment.plan(pol, seed, clip, n_mels, T), rule(seed, clip, fm, fw, tm, cap, n_mels, T), cap


KNOWN = [  # (seed, clip, policy kwargs, n_mels, T, frequency masks, time masks) as (start, width)
    (0, 0, {}, 80, 3000, [(0, 11), (65, 4)], [(2666, 25), (2253, 54)]),
    (1234, 7, {}, 80, 3000, [(52, 19), (11, 22)], [(2549, 28), (1021, 78)]),
    (2 ** 63 + 5, 2 ** 40 + 3, {}, 80, 3000, [(44, 22), (40, 14)], [(300, 67), (2392, 62)]),
    (0, 0, {"time_width": 3}, 80, 37, [(0, 11), (65, 4)], [(2, 2), (7, 1)]),
]


@pytest.mark.parametrize("row", KNOWN, ids=lambda r: f"seed{r[0]}-clip{r[1]}-T{r[4]}")
def test_known_answers_come_out_of_the_plan(native, row):
    from olmoasr_amd import augment
    seed, clip, over, n_mels, T, freq, time = row
    assert augment.plan(augment.SpecAugment.preset("LD", **over), seed, clip, n_mels, T) == (freq, time)
    assert rule(seed, clip, 2, 27, 2, over.get("time_width", 100), n_mels, T) == (freq, time)  # (the restatement is held to them too)


def test_time_ratio_caps_the_time_width_as_an_integer(native):
    from olmoasr_amd import augment
    pol = augment.SpecAugment.preset("LD", time_ratio=0.1)
    assert pol.time_cap(37) == 3 and pol.time_cap(3000) == 100 and augment.SpecAugment.preset("LD").time_cap(37) == 37
    assert augment.plan(pol, 0, 0, 80, 37) == ([(0, 11), (65, 4)], [(2, 2), (7, 1)])
    lb = augment.SpecAugment.preset("LB")
    assert (lb.freq_masks, lb.freq_width, lb.time_masks, lb.time_width, lb.time_ratio, lb.fill) == (1, 27, 1, 100, 1.0, 0.0)
    assert augment.SpecAugment() == augment.SpecAugment.preset("LD")
    with pytest.raises(ValueError, match="LD"):
        augment.SpecAugment.preset("XL")


def test_python_restatement_equals_the_host_twin_and_intervals_stay_inside(native):
    from olmoasr_amd import augment, ops
    all_cases = cases()
    assert len(all_cases) >= 2000
    seen = {"zero_masks": 0, "full_masks": 0, "wide_freq": 0, "wide_time": 0, "capped": 0, "big_seed": 0, "big_clip": 0, "below_2_32": 0, "above_2_32": 0,
            "one_bin": 0, "one_frame": 0, "width0": 0}
    for case in all_cases:
        seed, clip, fm, fw, tm, tw, ratio, n_mels, T = case
        got, want, cap = run_case(augment, case)
        assert got == want, case
        for iv, W, L in ((got[0], fw, n_mels), (got[1], cap, T)):
            for start, width in iv:
                assert 0 <= start and start + width <= L and 0 <= width <= min(W, L), (case, start, width)
        seen["zero_masks"] += fm == 0 and tm == 0
        seen["full_masks"] += fm == 8 and tm == 8
        # (SpecAugment never hands the library a time width above T -- time_ratio <= 1 -- so that side of min(W, L) is reached through ops)
        raw = ops.spec_augment_plan(freq_masks=fm, freq_width=fw, time_masks=tm, time_width=tw, seed=seed, clip=clip, n_mels=n_mels, T=T)
        assert raw == rule(seed, clip, fm, fw, tm, tw, n_mels, T), case
        assert all(0 <= s_ and s_ + w_ <= T and 0 <= w_ <= min(tw, T) for s_, w_ in raw[1]), case
        seen["wide_freq"] += fw > n_mels and fm > 0
        seen["wide_time"] += tw > T and tm > 0
        seen["capped"] += cap < tw and cap < T
        seen["big_seed"] += seed >= 2 ** 63
        seen["big_clip"] += clip >= 2 ** 63
        seen["below_2_32"] += 2 ** 32 - 8 <= clip < 2 ** 32
        seen["above_2_32"] += 2 ** 32 <= clip < 2 ** 32 + 8
        seen["one_bin"] += n_mels == 1
        seen["one_frame"] += T == 1
        seen["width0"] += (fw == 0 and fm > 0) or (cap == 0 and tm > 0)
    assert all(v > 0 for v in seen.values()), seen


def test_masked_cells_is_the_union_of_rows_and_columns(native):
    from olmoasr_amd import augment
    pol = augment.SpecAugment.preset("LD")
    for seed, first, B, n_mels, T in ((0, 0, 1, 80, 3000), (1234, 5, 3, 80, 257), (7, 2 ** 64 - 2, 4, 5, 37)):
        want = 0
        for b in range(B):
            f_iv, t_iv = rule(seed, (first + b) & M64, 2, 27, 2, min(100, T), n_mels, T)
            rows = {r for s, w in f_iv for r in range(s, s + w)}
            cols = {c for s, w in t_iv for c in range(s, s + w)}
            want += sum(1 for r in range(n_mels) for c in range(T) if r in rows or c in cols)
        assert augment.masked_cells(pol, seed, first, B, n_mels, T) == want
    assert augment.masked_cells(augment.SpecAugment(freq_masks=0, time_masks=0), 3, 0, 4, 80, 3000) == 0


def test_widths_are_uniform(native):
    """Seed 42, clips 0 .. 19999, LD: 40,000 frequency widths, uniform on 0 .. 27 (mean 13.5, sd 8.08: standard error 0.040, bound 6 of
    them; per-value expectation 1428.6, sd 37, bound 6 of them).  Measured on the CPU: mean 13.543, counts 1365 .. 1505."""
    from olmoasr_amd import augment
    pol = augment.SpecAugment.preset("LD")
    widths = [w for clip in range(20000) for _, w in augment.plan(pol, 42, clip)[0]]
    assert len(widths) == 40000
    mean = sum(widths) / len(widths)
    counts = [widths.count(v) for v in range(28)]
    print(f"mean {mean:.3f}, counts {min(counts)} .. {max(counts)}")
    assert abs(mean - 13.5) <= 0.25
    assert sum(counts) == 40000 and all(1200 <= c <= 1660 for c in counts), counts


def test_bad_arguments_are_refused_by_the_library_and_the_binding(native):
    import torch
    from olmoasr_amd import augment, ops
    lib = native.lib()
    assert lib.oasr_version() == 216 == native.ABI_VERSION
    assert ctypes.sizeof(native.SpecAug) == lib.oasr_sizeof_specaug() == 20
    buf = torch.zeros(64, dtype=torch.int32)  # (host memory: every call below must be refused before anything is touched or launched)
    ok = native.SpecAug(2, 27, 2, 100, 0.0)
    bad_policies = [native.SpecAug(-1, 27, 2, 100, 0.0), native.SpecAug(2, -1, 2, 100, 0.0), native.SpecAug(2, 27, -1, 100, 0.0),
                    native.SpecAug(2, 27, 2, -1, 0.0), native.SpecAug(9, 27, 2, 100, 0.0), native.SpecAug(2, 27, 9, 100, 0.0)]

    def refused(rc, *words):
        msg = lib.oasr_last_error().decode()
        return rc == -1 and all(w in msg for w in words)

    for pol in bad_policies:
        assert refused(lib.oasr_spec_augment(native.ptr(buf), 1, 80, 3000, ctypes.byref(pol), 0, 0, None), "oasr_spec_augment:")
        assert refused(lib.oasr_spec_augment_plan(ctypes.byref(pol), 0, 0, 80, 3000, native.ptr(buf), native.ptr(buf)), "oasr_spec_augment_plan:")
    for B, n_mels, T in ((0, 80, 3000), (-1, 80, 3000), (1, 0, 3000), (1, 80, 0), (1, 80, -5)):
        assert refused(lib.oasr_spec_augment(native.ptr(buf), B, n_mels, T, ctypes.byref(ok), 0, 0, None), "oasr_spec_augment:", ">= 1")
    assert refused(lib.oasr_spec_augment(None, 1, 80, 3000, ctypes.byref(ok), 0, 0, None), "null")
    assert refused(lib.oasr_spec_augment(native.ptr(buf), 1, 80, 3000, None, 0, 0, None), "null")
    for n_mels, T in ((0, 3000), (80, 0), (-3, 3000)):
        assert refused(lib.oasr_spec_augment_plan(ctypes.byref(ok), 0, 0, n_mels, T, native.ptr(buf), native.ptr(buf)), ">= 1")
    assert refused(lib.oasr_spec_augment_plan(None, 0, 0, 80, 3000, native.ptr(buf), native.ptr(buf)), "null")
    assert refused(lib.oasr_spec_augment_plan(ctypes.byref(ok), 0, 0, 80, 3000, None, native.ptr(buf)), "null")
    assert refused(lib.oasr_spec_augment_plan(ctypes.byref(ok), 0, 0, 80, 3000, native.ptr(buf), None), "null")
    assert int(buf.abs().sum()) == 0
    assert lib.oasr_spec_augment_plan(ctypes.byref(ok), 0, 0, 80, 3000, native.ptr(buf), native.ptr(buf[8:])) == 0
    assert buf[:4].tolist() == [0, 11, 65, 4] and buf[8:12].tolist() == [2666, 25, 2253, 54]
    # the Python surface says the same with ValueError / NativeError, on tensors that are not even on a GPU
    mel = torch.zeros(2, 80, 100)
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        ops.spec_augment_(mel, freq_masks=2, freq_width=27, time_masks=2, time_width=100)
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        augment.SpecAugment.preset("LD").apply_(mel, 0)
    for kw in (dict(freq_masks=9), dict(time_masks=9), dict(freq_masks=-1), dict(freq_width=-1), dict(time_width=-2), dict(freq_masks=1.5),
               dict(time_ratio=1.5), dict(time_ratio=-0.1)):
        with pytest.raises(ValueError):
            augment.SpecAugment(**kw)
    for kw in (dict(seed=-1), dict(seed=2 ** 64), dict(clip=-1), dict(clip=2 ** 64), dict(n_mels=0), dict(T=0)):
        with pytest.raises(ValueError):
            ops.spec_augment_plan(freq_masks=2, freq_width=27, time_masks=2, time_width=100, **kw)
    assert int((mel != 0).sum()) == 0


def test_cli_flags(tt, native):
    args = tt.parse_args([])
    assert args.spec_augment == "off" and args.spec_policy is None and all(args[f] is None for f in tt.SPEC_OVERRIDES)
    args = tt.parse_args(["--spec_augment=LD", "--spec_time_width=50"])
    p = args.spec_policy
    assert args.spec_augment == "LD" and (p.freq_masks, p.freq_width, p.time_masks, p.time_width, p.time_ratio, p.fill) == (2, 27, 2, 50, 1.0, 0.0)
    p = tt.parse_args(["--spec_augment", "LB", "--spec_fill=nan", "--spec_time_ratio=0.2", "--spec_freq_masks=3", "--spec_freq_width=9",
                       "--spec_time_masks=0"]).spec_policy
    assert (p.freq_masks, p.freq_width, p.time_masks, p.time_width, p.time_ratio) == (3, 9, 0, 100, 0.2) and math.isnan(p.fill)
    with pytest.raises(SystemExit, match="off . LD . LB"):
        tt.parse_args(["--spec_augment=XL"])
    with pytest.raises(SystemExit, match="off . LD . LB"):
        tt.parse_args(["--spec_augment=True"])
    for flag in ("--spec_freq_masks=1", "--spec_freq_width=5", "--spec_time_masks=1", "--spec_time_width=50", "--spec_time_ratio=0.5",
                 "--spec_fill=0.5"):
        with pytest.raises(SystemExit, match="LD . LB"):
            tt.parse_args([flag])
        with pytest.raises(SystemExit, match="LD . LB"):
            tt.parse_args(["--spec_augment=off", flag])
    for flag in ("--spec_freq_masks=9", "--spec_time_width=-1", "--spec_fill=much", "--spec_time_ratio=2"):
        with pytest.raises(SystemExit):
            tt.parse_args(["--spec_augment=LD", flag])


def test_spec_offset_gives_every_micro_batch_its_own_ids(tt):
    world, batch, accum = 8, 4, 4
    offs = sorted(tt.spec_offset(step, micro, accum, world, rank, batch) for step in range(50) for micro in range(accum) for rank in range(world))
    assert len(set(offs)) == 50 * accum * world and offs[0] == 0
    assert all(b - a >= batch for a, b in zip(offs, offs[1:]))  # the ranges [o, o + train_batch_size) do not overlap
    assert tt.spec_offset(3, 2, 4, 8, 5, 4) == ((3 * 4 + 2) * 8 + 5) * 4
