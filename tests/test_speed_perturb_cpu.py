"""CPU half of speed perturbation (csrc/speed_core.h through its host twin: oasr_speed_perturb_host, oasr_speed_plan, oasr_speed_table): the
tap tables against the formula, the resampler against the rule written out again here in numpy, known answers, a quality guard on sines, the
timestamp-token map, the seeded choice of the factor, the argument checks that fire before any launch, the loaders' ``last_n_valid`` and the
training script's flags."""
import ctypes
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
THREE_WAY = ((9, 10), (1, 1), (11, 10))
TABLES = {(11, 10): 19, (9, 10): 17, (3, 2): 26, (2, 3): 17, (32, 31): 18, (1, 2): 17, (2, 1): 34}


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
    spec = importlib.util.spec_from_file_location("tt_speed_cpu", os.path.join(ROOT, "scripts", "training", "train_timestamps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the rule, from the text of include/oasr.h; nothing below is imported from the package --------------------------------------
def mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def half_width(P, Q):
    fc = 0.95 * min(1.0, Q / P)
    return math.floor(16.0 / fc) + 1


def formula_taps(P, Q):
    """float64 [Q, 2H]: c of the header's formula, before quantisation."""
    fc = 0.95 * min(1.0, Q / P)
    Wd = 16.0 / fc
    H = math.floor(Wd) + 1
    k = np.arange(2 * H, dtype=np.float64) - H + 1
    u = k[None, :] - (np.arange(Q, dtype=np.float64) / Q)[:, None]
    c = fc * np.sinc(fc * u) * (0.5 + 0.5 * np.cos(np.pi * u / Wd))  # np.sinc(x) = sin(pi x) / (pi x)
    return np.where(np.abs(u) < Wd, c, 0.0), H


def choice(seed, clip, n_factors):
    return mix(mix(mix(seed) ^ clip) ^ (3 << 16)) % n_factors


def plan(factors, seed, clip, n_valid, N):
    i = choice(seed, clip, len(factors))
    P, Q = factors[i]
    n_out = (n_valid * Q) // P
    if n_out > N:
        return 1, 1, n_valid, -1
    return P, Q, n_out, i


def resample(x, n_valid, N, P, Q, T, H):
    """One row by the header's "Sample" rule, in int64 numpy, with the library's own table T [Q, 2H]."""
    if P == Q:
        return x.copy()
    n_out = (n_valid * Q) // P
    xp = np.zeros(n_valid + 2 * H + (N * P) // Q + 2, dtype=np.int64)
    xp[H:H + n_valid] = x[:n_valid]           # xp[i + H] = x[i], zero outside [0, n_valid)
    n = np.arange(n_out, dtype=np.int64)
    m, r = (n * P) // Q, (n * P) % Q
    idx = m[:, None] + np.arange(2 * H)[None, :] - H + 1 + H
    acc = (xp[idx] * T[r].astype(np.int64)).sum(axis=1)
    y = np.zeros(N, dtype=np.int16)
    y[:n_out] = np.clip((acc + 16384) >> 15, -32768, 32767).astype(np.int16)
    return y


def token_map(t, P, Q, ts_begin=50363, ts_max=1500):
    if not ts_begin <= t <= ts_begin + ts_max:
        return t
    return ts_begin + min(ts_max, (2 * (t - ts_begin) * Q + P) // (2 * P))


def i32(v):
    return torch.tensor(v, dtype=torch.int32)


# ---- the table --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pq", sorted(TABLES))
def test_table_matches_the_formula_and_sums_to_one(ops, pq):
    P, Q = pq
    T, H = ops.speed_table(P, Q)
    assert H == half_width(P, Q) == TABLES[pq] and tuple(T.shape) == (Q, 2 * H) and T.dtype == torch.int32
    T = T.numpy().astype(np.int64)
    assert (T.sum(axis=1) == 32768).all()
    c, _ = formula_taps(P, Q)
    q = np.floor(c * 32768 + 0.5).astype(np.int64)
    fix = 32768 - q.sum(axis=1)               # what the phase's largest tap takes on top
    want = q.copy()
    want[np.arange(Q), q.argmax(axis=1)] += fix  # (argmax: the first of equal maxima)
    assert np.abs(T - want).max() <= 1, "a tap is more than 1 from the restated formula"
    assert np.abs(fix).max() <= 2 * H


def test_absolute_tap_sum_shows_why_32_bits_are_not_enough(ops):
    T, _ = ops.speed_table(9, 10)
    worst = int(T.to(torch.int64).abs().sum(dim=1).max())
    assert worst > 65536 and worst * 32768 > 2 ** 31  # full-scale input overflows a 32-bit sum
    assert worst == 73920


# ---- the resampler against the restatement --------------------------------------------------------------------------------------------
def noise_rows(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-32768, 32768, (B, N), generator=g, dtype=torch.int64).to(torch.int16)
    x[0, :N // 2] = 32767    # full-scale runs: the overshoot of the filter meets the clamp
    x[0, N // 2:] = -32768
    x[1, ::2], x[1, 1::2] = 32767, -32768
    return x


@pytest.mark.parametrize("factors", [THREE_WAY, ((11, 10),), ((9, 10),), ((2, 1), (1, 2)), ((3, 2), (2, 3), (32, 31))], ids=str)
def test_host_twin_equals_the_restatement(ops, factors):
    N = 4096
    H = max(half_width(P, Q) for P, Q in factors if P != Q)
    nv = [0, 1, H, 2999, 4096, 1234, 4095]
    x = noise_rows(len(nv), N, 7)
    clamped = 0
    for seed, first in ((0, 0), (11, 2 ** 32 - 3), (2 ** 63 + 5, M64 - 2)):
        y, n_out, fac = ops.speed_perturb_host(x, i32(nv), factors=factors, seed=seed, first_clip=first)
        for b, n_valid in enumerate(nv):
            P, Q, no, f = plan(factors, seed, (first + b) & M64, n_valid, N)
            assert (int(n_out[b]), int(fac[b])) == (no, f) == ops.speed_plan(factors, seed, (first + b) & M64, n_valid, N)[2:]
            T, Hpq = (ops.speed_table(P, Q) if P != Q else (torch.zeros(1, 2, dtype=torch.int32), 1))
            want = resample(x[b].numpy(), n_valid, N, P, Q, T.numpy(), Hpq)
            assert np.array_equal(y[b].numpy(), want), (b, n_valid, P, Q)
            if P != Q:
                clamped += int((np.abs(want.astype(np.int64)) >= 32767).sum())
    assert clamped > 0  # the full-scale rows met the clamp


def test_known_answers(ops):
    N, nv = 4096, 3000
    g = torch.Generator().manual_seed(3)
    noise = torch.randint(-32768, 32768, (1, N), generator=g, dtype=torch.int64).to(torch.int16)
    y, n_out, fac = ops.speed_perturb_host(noise, i32([nv]), factors=((1, 1),))
    assert torch.equal(y, noise) and n_out.tolist() == [nv] and fac.tolist() == [0]  # the identity is a bit copy of the WHOLE row
    const = torch.zeros(1, N, dtype=torch.int16)
    const[0, :nv] = 12345
    for (P, Q) in ((11, 10), (9, 10)):
        H = half_width(P, Q)
        y, n_out, fac = ops.speed_perturb_host(const, i32([nv]), factors=((P, Q),))
        no = (nv * Q) // P
        assert n_out.tolist() == [no] and fac.tolist() == [0]
        assert bool((y[0, 2 * H:no - 2 * H] == 12345).all()) and bool((y[0, no:] == 0).all())
    # a slow-down that would not fit the row: the copy, factor -1
    y, n_out, fac = ops.speed_perturb_host(noise, i32([3700]), factors=((9, 10),))
    assert (3700 * 10) // 9 > N and torch.equal(y, noise) and n_out.tolist() == [3700] and fac.tolist() == [-1]
    assert ops.speed_plan(((9, 10),), 0, 0, 3700, N) == (1, 1, 3700, -1)
    y, n_out, fac = ops.speed_perturb_host(noise, i32([3686]), factors=((9, 10),))  # 3686 * 10 // 9 = 4095: fits
    assert n_out.tolist() == [4095] and fac.tolist() == [0]
    # out= and row strides: the row gaps of a strided output are not written
    buf = torch.full((2, N + 128), 0x5EA7, dtype=torch.int16)
    two = torch.cat([noise, const])
    got, _, _ = ops.speed_perturb_host(two, i32([nv, nv]), factors=((11, 10),), out=buf[:, 64:64 + N])
    assert got.data_ptr() == buf[:, 64:].data_ptr()
    assert bool((buf[:, :64] == 0x5EA7).all()) and bool((buf[:, 64 + N:] == 0x5EA7).all())
    assert torch.equal(buf[1, 64:64 + N], ops.speed_perturb_host(const, i32([nv]), factors=((11, 10),), first_clip=1)[0][0])


@pytest.mark.parametrize("pq", [(11, 10), (9, 10)])
@pytest.mark.parametrize("freq", [200, 1000, 3000])
def test_quality_guard_on_sines(ops, pq, freq):
    """A sine of amplitude 20000 resampled by P / Q against the sine at the new rate, away from the edges.  The float64 formula with this
    quantisation gives at most 6 LSB here (measured through the host twin, which equals the restatement
    above bit for bit: 1.4 .. 6.0 LSB over these six cases, the worst at 11/10 and 3000 Hz); a wrong phase or tap
    offset lands in the thousands.  16 LSB leaves room for the +-1 ties of the table."""
    P, Q = pq
    N, nv = 8192, 7000
    H = half_width(P, Q)
    n_in = np.arange(N, dtype=np.float64)
    x = np.zeros(N, dtype=np.int16)
    x[:nv] = np.round(20000 * np.sin(2 * np.pi * freq / 16000 * n_in[:nv])).astype(np.int16)
    y, n_out, fac = ops.speed_perturb_host(torch.from_numpy(x)[None], i32([nv]), factors=(pq,))
    no = int(n_out[0])
    assert no == (nv * Q) // P and fac.tolist() == [0]
    n = np.arange(2 * H, no - 2 * H, dtype=np.float64)
    want = 20000 * np.sin(2 * np.pi * freq / 16000 * n * P / Q)
    err = float(np.abs(y[0, 2 * H:no - 2 * H].numpy().astype(np.float64) - want).max())
    T, _ = ops.speed_table(P, Q)
    restated = resample(x, nv, N, P, Q, T.numpy(), H)
    assert np.array_equal(restated, y[0].numpy())
    print(f"{P}/{Q} at {freq} Hz: max error {err:.2f} LSB over {n.size} samples")
    assert err <= 16.0


# ---- tokens -----------------------------------------------------------------------------------------------------------------------------
def test_timestamp_tokens(ops):
    B0 = 50363
    pcm = torch.zeros(1, 4096, dtype=torch.int16)
    for (P, Q), known in (((11, 10), {0: 0, 1: 1, 11: 10, 1500: 1364}), ((9, 10), {9: 10, 0: 0, 1500: 1500, 1400: 1500, 1350: 1500, 1349: 1499})):
        for k, want in known.items():
            assert token_map(B0 + k, P, Q) == B0 + want
        ks = list(range(0, 1501))
        others = [50256, 50257, 50362, 51864, 0, B0 + 1501]
        row = torch.tensor([[B0 + k for k in ks] + others + [B0 + k for k in known]], dtype=torch.int64)
        a, b = row.clone(), row.flip(1).clone()
        ops.speed_perturb_host(pcm, i32([100]), factors=((P, Q),), tokens=(a, b))
        want = torch.tensor([[token_map(int(t), P, Q) for t in row[0]]], dtype=torch.int64)
        assert torch.equal(a, want) and torch.equal(b, want.flip(1))
        mapped = a[0, :len(ks)]
        assert bool((mapped[1:] >= mapped[:-1]).all()) and int(mapped.max()) <= B0 + 1500 and int(mapped.min()) == B0  # monotone, clamped
        assert a[0, len(ks):len(ks) + len(others)].tolist() == others                                                  # the rest untouched
        for i, (k, w) in enumerate(known.items()):
            assert int(a[0, len(ks) + len(others) + i]) == B0 + w
    # other ts_begin / ts_max, one tensor only, and the identity leaves everything alone
    t = torch.tensor([[100, 110, 120, 99, 121]], dtype=torch.int64)
    ops.speed_perturb_host(pcm, i32([100]), factors=((2, 1),), tokens=(t,), ts_begin=100, ts_max=20)
    assert t.tolist() == [[100, 105, 110, 99, 121]]
    t = torch.tensor([[100, 110, 120, 99, 121]], dtype=torch.int64)
    ops.speed_perturb_host(pcm, i32([100]), factors=((1, 2),), tokens=(t,), ts_begin=100, ts_max=20)
    assert t.tolist() == [[100, 120, 120, 99, 121]]
    keep = torch.tensor([[B0 + 7, 50256]], dtype=torch.int64)
    ops.speed_perturb_host(pcm, i32([100]), factors=((1, 1),), tokens=(keep,))
    assert keep.tolist() == [[B0 + 7, 50256]]
    # a row that falls back to the copy keeps its tokens as well
    keep = torch.tensor([[B0 + 700]], dtype=torch.int64)
    _, _, fac = ops.speed_perturb_host(pcm, i32([4000]), factors=((9, 10),), tokens=(keep,))
    assert fac.tolist() == [-1] and keep.tolist() == [[B0 + 700]]


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
def test_plan_is_the_stated_hash(ops):
    ids = [0, 1, 7, 2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 3, 2 ** 63, 2 ** 64 - 2, 2 ** 64 - 1]
    many = ((9, 10), (1, 1), (11, 10), (3, 2), (2, 3), (5, 4), (4, 5), (17, 9))
    for factors in (THREE_WAY, many, ((11, 10),)):
        for seed in ids:
            for clip in ids:
                P, Q, n_out, f = ops.speed_plan(factors, seed, clip, 1000, 4096)
                assert f == choice(seed, clip, len(factors)) and (P, Q) == factors[f] and n_out == (1000 * Q) // P
                assert (P, Q, n_out, f) == plan(factors, seed, clip, 1000, 4096)
    counts = [0, 0, 0]
    for clip in range(30000):
        counts[ops.speed_plan(THREE_WAY, 1234, clip, 1000, 480000)[3]] += 1
    assert sum(counts) == 30000 and all(0.31 * 30000 <= c <= 0.36 * 30000 for c in counts), counts
    # the same h as SpecAugment's, another kind: the factor does not follow from a mask
    h = mix(mix(1234) ^ 5)
    assert choice(1234, 5, 3) == mix(h ^ (3 << 16)) % 3


def test_augment_surface(ops):
    from olmoasr_amd import augment
    pol = augment.SpeedPerturb.preset("3way")
    assert pol.factors == THREE_WAY == augment.SpeedPerturb().factors and (pol.ts_begin, pol.ts_max) == (50363, 1500)
    assert pol.plan(3, 9, 1000, 4096) == ops.speed_plan(THREE_WAY, 3, 9, 1000, 4096) == plan(THREE_WAY, 3, 9, 1000, 4096)
    nv = [1000, 4000, 0, 4096, 3000]
    counts = pol.factor_counts(3, M64 - 1, nv, 4096)  # (stream ids wrap at 2^64)
    want = [0, 0, 0, 0]
    for b, v in enumerate(nv):
        want[plan(THREE_WAY, 3, (M64 - 1 + b) & M64, v, 4096)[3]] += 1
    assert counts == want and sum(counts) == len(nv)
    assert augment.SpeedPerturb(factors=[[3, 2], [2, 3]]).factors == ((3, 2), (2, 3))
    with pytest.raises(ValueError, match="3way"):
        augment.SpeedPerturb.preset("5way")
    for bad in (((4, 6),), ((0, 1),), ((1, 0),), ((33, 32),), ((32, 33),), ((3, 1),), ((1, 3),), (), THREE_WAY * 3, ((1.5, 1),), ((1, 1, 1),), 7):
        with pytest.raises(ValueError):
            augment.SpeedPerturb(factors=bad)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(native, ops):
    lib = native.lib()
    N = 64
    x, y = torch.full((2, N), 3, dtype=torch.int16), torch.full((2, N), 5, dtype=torch.int16)
    nv = i32([N, 10])

    def block(factors=((11, 10),), pcm_in=x, pcm_out=y):
        a = native.SpeedArgs()
        a.pcm_in, a.pcm_out, a.n_valid = pcm_in.data_ptr(), pcm_out.data_ptr(), nv.data_ptr()
        a.ld_in = a.ld_out = N
        a.B, a.N = 2, N
        a.policy.n_factors = len(factors)
        for i, (p, q) in enumerate(factors[:8]):
            a.policy.P[i], a.policy.Q[i] = p, q
        return a

    def refused(rc, what):
        return rc == -1 and what in lib.oasr_last_error().decode()  # OASR_EINVAL

    assert lib.oasr_speed_perturb_host(ctypes.byref(block())) == 0
    y.fill_(5)
    for factors, what in ((((4, 6),), "coprime"), (((0, 1),), "[1, 32]"), (((1, 0),), "[1, 32]"), (((33, 32),), "[1, 32]"), (((32, 33),), "[1, 32]"),
                          (((3, 1),), "ratio"), (((1, 3),), "ratio"), (THREE_WAY * 3, "n_factors"), ((), "n_factors")):
        assert refused(lib.oasr_speed_perturb_host(ctypes.byref(block(factors))), what), factors
        pol = block(factors).policy
        out = [ctypes.c_int(-5) for _ in range(4)]
        assert refused(lib.oasr_speed_plan(ctypes.byref(pol), 0, 0, 10, N, *[ctypes.byref(o) for o in out]), what)
        assert [o.value for o in out] == [-5] * 4
        with pytest.raises(ValueError):
            ops.speed_perturb_host(x, nv, factors=factors)
        with pytest.raises(ValueError):
            ops.speed_plan(factors, 0, 0, 10, N)
    both = torch.full((2, N + 32), 3, dtype=torch.int16)
    assert refused(lib.oasr_speed_perturb_host(ctypes.byref(block(pcm_in=both[:, :N], pcm_out=both[:, 32:]))), "overlap")
    a = block(pcm_in=both[:, :N], pcm_out=both[:, 32:])
    a.ld_in = a.ld_out = N + 32
    assert refused(lib.oasr_speed_perturb_host(ctypes.byref(a)), "overlap")
    assert refused(lib.oasr_speed_perturb_host(ctypes.byref(block(pcm_out=x))), "overlap")
    with pytest.raises(ValueError, match="overlap"):
        ops.speed_perturb_host(both[:, :N], nv, factors=THREE_WAY, out=both[:, 32:])
    with pytest.raises(ValueError, match="overlap"):
        ops.speed_perturb_host(x, nv, factors=THREE_WAY, out=x)
    assert bool((y == 5).all()) and bool((both == 3).all()) and bool((x == 3).all())
    # lengths the host can read are refused; the table of the identity does not exist
    for bad in ([N + 1, 0], [-1, 0]):
        with pytest.raises(ValueError, match="n_valid"):
            ops.speed_perturb_host(x, i32(bad), factors=THREE_WAY)
    a = block()
    bad_len = i32([N + 1, 0])
    a.n_valid = bad_len.data_ptr()
    assert refused(lib.oasr_speed_perturb_host(ctypes.byref(a)), "n_valid")
    with pytest.raises(ValueError):
        ops.speed_table(1, 1)
    with pytest.raises(ValueError):
        ops.speed_table(4, 6)
    # dtypes, shapes, devices
    for kw in (dict(pcm=x.float()), dict(pcm=x[0]), dict(n_valid=nv.long()), dict(n_valid=nv[:1]), dict(tokens=(torch.zeros(2, 4),)),
               dict(tokens=(torch.zeros(3, 4, dtype=torch.int64),)), dict(tokens=(torch.zeros(2, 4, dtype=torch.int64),) * 3),
               dict(tokens=(torch.zeros(2, 4, dtype=torch.int64), torch.zeros(2, 5, dtype=torch.int64))), dict(out=torch.zeros(2, N)),
               dict(out=torch.zeros(2, N + 1, dtype=torch.int16)), dict(seed=-1), dict(first_clip=2 ** 64), dict(ts_max=-1), dict(ts_begin=1.5)):
        args = dict(pcm=x, n_valid=nv, factors=THREE_WAY, tokens=(torch.zeros(2, 4, dtype=torch.int64),))
        args.update(kw)
        pcm, n_valid = args.pop("pcm"), args.pop("n_valid")
        with pytest.raises(ValueError):
            ops.speed_perturb_host(pcm, n_valid, **args)
    with pytest.raises(ValueError, match="GPU"):
        ops.speed_perturb(x, nv, factors=THREE_WAY)  # the device entry takes no CPU tensor, and says so before a launch
    assert bool((y == 5).all())


# ---- the loaders ------------------------------------------------------------------------------------------------------------------------
def last_nonzero_end(row):
    nz = row.numpy().nonzero()[0]
    return int(nz[-1]) + 1 if nz.size else 0


def test_loaders_hand_out_n_valid(tmp_path):
    from olmoasr_amd import data, synth
    order = [[0, 1, 2], [3, 4, 5]]
    ld = synth.SynthLoader(iter(order), "cpu", workers=2, depth=2, timestamps=True)
    assert ld.last_n_valid is None and ld.last_n_valid_host is None
    for idx, (pcm, ti, ty, tl) in zip(order, ld):
        nv = ld.last_n_valid
        assert nv.dtype == torch.int32 and tuple(nv.shape) == (3,) and torch.equal(nv, ld.last_n_valid_host) and not ld.last_n_valid_host.is_cuda
        assert nv.tolist() == [last_nonzero_end(pcm[r]) for r in range(3)]
        assert all(240000 <= v <= 480000 for v in nv.tolist())
    ld.close()
    d = data.write_synthetic_shards(str(tmp_path), 5, per_file=3, timestamps=True)
    shards = data.AudioTextShards(data.load_samples_dicts(d))
    ld = data.ShardLoader(shards, iter([[0, 1, 2], [3, 4]]), "cpu", batch=3, workers=2, depth=2)
    for b, (pcm, ti, ty, tl) in zip((3, 2), ld):
        nv = ld.last_n_valid
        assert nv.dtype == torch.int32 and tuple(nv.shape) == (b,) and torch.equal(nv, ld.last_n_valid_host)
        for r in range(b):  # the loaded clip's own length: nothing but silence behind it
            assert last_nonzero_end(pcm[r]) <= int(nv[r]) <= 480000 and not bool(pcm[r, int(nv[r]):].any())
    ld.close()


# ---- the training script ----------------------------------------------------------------------------------------------------------------
def test_cli_flags(tt, native):
    off = tt.parse_args([])
    assert off.speed_perturb == "off" and off.speed_factors is None and off.speed_policy is None
    assert "speed_perturb" in tt.NATIVE_FLAGS and "speed_factors" in tt.NATIVE_FLAGS
    explicit = tt.parse_args(["--speed_perturb=off"])
    assert dict(explicit) == dict(off)
    on = tt.parse_args(["--speed_perturb=3way"])
    assert on.speed_policy.factors == THREE_WAY
    rest = {k: v for k, v in on.items() if k not in ("speed_perturb", "speed_policy")}
    assert rest == {k: v for k, v in off.items() if k not in ("speed_perturb", "speed_policy")}  # nothing else moves
    p = tt.parse_args(["--speed_perturb", "3way", "--speed_factors=((3,2),(1,1),(2,3),(11,10))"]).speed_policy
    assert p.factors == ((3, 2), (1, 1), (2, 3), (11, 10))
    assert tt.parse_args(["--speed_perturb=3way", "--speed_factors=[[9,10],[11,10]]"]).speed_policy.factors == ((9, 10), (11, 10))
    for bad in ("--speed_perturb=5way", "--speed_perturb=True", "--speed_perturb=on"):
        with pytest.raises(SystemExit, match="off . 3way"):
            tt.parse_args([bad])
    for flag in ("--speed_factors=((9,10),)",):
        with pytest.raises(SystemExit, match="3way"):
            tt.parse_args([flag])
        with pytest.raises(SystemExit, match="3way"):
            tt.parse_args(["--speed_perturb=off", flag])
    for flag in ("--speed_factors=((4,6),)", "--speed_factors=((3,1),)", "--speed_factors=((0,1),)", "--speed_factors=((33,32),)", "--speed_factors=()",
                 "--speed_factors=(9,10)", "--speed_factors=fast", "--speed_factors=1.1", "--speed_factors=((9,10,11),)", "--speed_factors=((1.5,1),)",
                 "--speed_factors=" + repr(THREE_WAY * 3)):
        with pytest.raises(SystemExit):
            tt.parse_args(["--speed_perturb=3way", flag])
