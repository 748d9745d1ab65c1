"""Op-level parity of every HIP kernel against a plain fp32 PyTorch evaluation of the same op on the same
(bf16-rounded) inputs.  Tolerances: a bf16 output carries one rounding (rel 2^-9 = 0.2 %), fp32 accumulation
differences are far below that -> rtol 1e-2 with an absolute floor tied to the output scale."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DEV = "cuda"


def ops():
    from olmoasr_amd import ops as o
    return o


def close(got, ref, rtol=1e-2, atol=None, name=""):
    got, ref = got.float(), ref.float()
    if atol is None:
        atol = 1e-2 * float(ref.abs().mean()) + 1e-6
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bool(bad.any()), f"{name}: {int(bad.sum())}/{bad.numel()} off, max abs err {float(err.max()):.4g}, ref scale {float(ref.abs().max()):.4g}"


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(DEV)


def outdir():
    d = os.path.join(os.environ.get("GRAFT_REPO_ROOT", os.getcwd()), "gpurun_out")
    os.makedirs(d, exist_ok=True)
    return d


# ------------------------------------------------------------------------------------------------------------
def test_probe_tr16_lane_mapping():
    """Pins the ds_read_b64_tr_b16 semantics the GEMM/attention transposed operand reads rely on: within each
    16-lane group, lane c's j-th result is element (c & 3) of the 8 bytes fetched by lane 4j + (c >> 2)."""
    from olmoasr_amd import _native as N
    src = torch.arange(16 * 64, dtype=torch.float32).to(BF).to(DEV)  # value == linear index (exact in bf16 up to 256; use ids)
    ids = torch.arange(16 * 64, dtype=torch.int16).to(DEV)
    dst = torch.zeros(64 * 4, dtype=torch.int16, device=DEV)
    N.check(N.lib().oasr_probe_tr16(N.ptr(ids), N.ptr(dst), N.stream_ptr()), "probe")
    torch.cuda.synchronize()
    got = dst.cpu().view(64, 4).numpy()
    exp = np.zeros((64, 4), dtype=np.int16)
    for l in range(64):
        g, c = l >> 4, l & 15
        for j in range(4):
            src_lane = 4 * j + (c >> 2)
            row = g * 4 + (src_lane >> 2)
            col = (src_lane & 3) * 4 + (c & 3)
            exp[l, j] = row * 64 + col
    with open(os.path.join(outdir(), "probe_tr16.json"), "w") as f:
        json.dump({"got": got.tolist(), "expected": exp.tolist()}, f)
    assert (got == exp).all(), "ds_read_b64_tr_b16 lane mapping differs from the assumed one; see gpurun_out/probe_tr16.json"
    del src


# ------------------------------------------------------------------------------------------------------------
def test_log_mel_matches_oracle():
    from oracle import mel_oracle as me
    from oracle import model_oracle as mo
    pcm, *_ = mo.synthetic_batch([0, 1, 2])
    ref = me.log_mel_batch(pcm.numpy())
    got = ops().log_mel(pcm.to(DEV)).cpu().numpy()
    assert got.shape == (3, 80, 3000)
    err = np.abs(got - ref)
    # fp32 DFT vs float64 oracle: the error is relative to the frame energy; bins near the -8 floor carry the most
    assert err.max() < 2e-3, f"max err {err.max()}"
    assert err.mean() < 2e-5, f"mean err {err.mean()}"
    # float32 waveform input is the same thing as int16/32768
    got_f = ops().log_mel((pcm.float() / 32768.0).to(DEV)).cpu().numpy()
    assert np.array_equal(got_f, got)


def test_log_mel_edge_cases():
    from oracle import mel_oracle as me
    z = torch.zeros(2, 480000, dtype=torch.int16)
    got = ops().log_mel(z.to(DEV)).cpu().numpy()
    assert np.allclose(got, -1.5)  # (log10(1e-10) + 4) / 4
    g = torch.Generator().manual_seed(5)
    short = (torch.randn(1, 16000, generator=g) * 0.3).clamp(-1, 1)
    ref = me.log_mel_spectrogram(short[0].numpy())
    got = ops().log_mel(short.to(DEV)).cpu().numpy()[0]
    assert got.shape == ref.shape == (80, 100)
    assert np.abs(got - ref).max() < 2e-3
    # a pure tone: 80 dB of dynamic range between bins must survive (this is what rules out a bf16 DFT)
    t = torch.arange(480000) / 16000.0
    tone = (0.5 * torch.sin(2 * math.pi * 1000.0 * t))[None]
    ref = me.log_mel_spectrogram(tone[0].numpy())
    got = ops().log_mel(tone.to(DEV)).cpu().numpy()[0]
    assert np.abs(got - ref).max() < 5e-2 and np.abs(got - ref).mean() < 2e-3


# ------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(256, 256, 128), (384, 128, 512), (296, 136, 200), (128, 1024, 64), (1000, 384, 1536), (520, 8, 64),
               (3000, 1152, 384)]


@pytest.fixture(params=[0, 1, 2, 3, 4], ids=["auto", "general", "fast256x128", "fast256x256", "pingpong256"])
def gemm_path(request):
    """Run GEMM tests through both kernels: the direct-to-LDS fast path (where it applies) and the general one."""
    from olmoasr_amd import _native as N
    N.lib().oasr_gemm_force_general(request.param)
    yield request.param
    N.lib().oasr_gemm_force_general(0)


def test_probe_lds_dma_out_of_range_lanes():
    """Records what buffer_load ... lds writes for out-of-range lanes (zeros vs nothing) -- informational, the fast
    GEMM path does not rely on it (it clamps source rows instead)."""
    from olmoasr_amd import _native as N
    src = torch.arange(1, 513, dtype=torch.int16, device=DEV)
    dst = torch.zeros(512, dtype=torch.int16, device=DEV)
    N.check(N.lib().oasr_probe_lds_oob(N.ptr(src), N.ptr(dst), N.stream_ptr()), "probe")
    got = dst.cpu().view(64, 8)
    assert torch.equal(got[:32], src.cpu().view(64, 8)[:32])
    oob = got[32:]
    kind = "zeros" if bool((oob == 0).all()) else ("untouched" if bool((oob == -21846).all()) else "other")
    with open(os.path.join(outdir(), "probe_lds_oob.json"), "w") as f:
        json.dump({"oob_lanes": kind, "sample": oob[0].tolist()}, f)
    assert kind in ("zeros", "untouched")


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
@pytest.mark.parametrize("ta,tb", [(False, False), (False, True), (True, False), (True, True)])
def test_gemm_layouts(M, N, K, ta, tb, gemm_path):
    A = rnd(K, M, seed=1) if ta else rnd(M, K, seed=1)
    B = rnd(K, N, seed=2) if tb else rnd(N, K, seed=2)
    out = torch.full((M, N), float("nan"), device=DEV, dtype=BF)
    ops().gemm(A, B, M, N, K, ta=ta, tb=tb, out=out)
    Af = A.float().t() if ta else A.float()
    Bf = B.float().t() if tb else B.float()
    close(out, Af @ Bf.t(), name=f"gemm {M}x{N}x{K} ta={ta} tb={tb}")


@pytest.mark.parametrize("layout", ["nt_resid", "nt_gelu", "nn", "tn_splitk"])
def test_gemm_pingpong_persistent_launch_matches_plain(layout):
    """Persistent launches of the 256x256 kernel (one workgroup per CU walking the plain launch's grid, next tile's prologue
    issued ahead of the epilogue) must produce the plain launch's bits (fp32 atomic outputs: its values)."""
    from olmoasr_amd import _native as N
    if layout == "tn_splitk":
        M, N_, K = 2048, 2048, 4096   # 64 tiles x 8 K-ranges = 512 virtual blocks
        A, B = rnd(K, M, seed=1), rnd(K, N_, seed=2, scale=0.05)
    else:
        M, N_, K = 256 * 40 + 64, 2048, 512  # 41 x 8 = 328 virtual blocks (uneven rounds, ragged last row panel)
        A = rnd(M, K, seed=1)
        B = rnd(K, N_, seed=2, scale=0.05) if layout == "nn" else rnd(N_, K, seed=2, scale=0.05)
    bias = torch.randn(N_, device=DEV)
    resid = rnd(M, N_, seed=3)
    outs = []
    try:
        N.lib().oasr_gemm_force_general(4)  # force the ping-pong kernel
        for v in (24, 40):                  # default kernels: plain launch / persistent launch
            N.lib().oasr_gemm_set_variant(v)
            if layout == "tn_splitk":
                o = torch.zeros(M, N_, device=DEV)
                ops().gemm(A, B, M, N_, K, ta=True, tb=True, out_f32=o, atomic=True, split_k=8)
                outs.append((o,))
            elif layout == "nt_gelu":
                o = torch.full((M, N_), float("nan"), device=DEV, dtype=BF)
                pre = torch.full((M, N_), float("nan"), device=DEV, dtype=BF)
                ops().gemm(A, B, M, N_, K, bias=bias, act=2, out=o, out_pre=pre)
                outs.append((o, pre))
            else:
                o = torch.full((M, N_), float("nan"), device=DEV, dtype=BF)
                cs = torch.zeros(N_, device=DEV)
                ops().gemm(A, B, M, N_, K, tb=(layout == "nn"), bias=bias, resid=resid, out=o)
                outs.append((o, cs))
    finally:
        N.lib().oasr_gemm_force_general(0)
        N.lib().oasr_gemm_set_variant(-1)
    for a, b in zip(outs[0], outs[1]):
        if layout == "tn_splitk":
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-3)
        else:
            assert torch.equal(a, b)
    if layout == "tn_splitk":
        close(outs[1][0], A.float().t() @ B.float(), name="persistent wgrad")
    elif layout != "nt_gelu":
        Bf = B.float() if layout == "nn" else B.float().t()
        pre = (A.float() @ Bf + bias).bfloat16().float()
        ref = pre + resid.float()
        # one bf16 ulp of the larger addend: where pre and the residual cancel, the fp32 reference product (vendor GEMM, box dependent)
        # may round `pre` to the neighbouring bf16 value
        ulp = torch.maximum(pre.abs(), resid.float().abs()) * 2.0 ** -7
        assert bool(((outs[1][0].float() - ref).abs() <= ulp + 1e-2 * ref.abs() + 1e-3).all()), "persistent " + layout


@pytest.mark.parametrize("M,N_,K", [(2560, 1024, 1024), (520, 512, 320)])  # the second: ragged last row panel, an odd count (5) of K-tiles
@pytest.mark.parametrize("ta,tb", [(False, False), (False, True), (True, True)])
def test_gemm_pingpong_schedules_are_bit_identical(ta, tb, M, N_, K):
    """The 256x256 kernel walks a K-tile in four phases of 8 MFMAs (schedule 2) or in two sections of 16 with part of the direct-to-LDS
    pieces issued between the MFMAs (7, the default without fused column sums); every accumulator receives its K slices in the same
    order in both, so they must produce the same bits."""
    from olmoasr_amd import _native as N
    A = rnd(K, M, seed=1) if ta else rnd(M, K, seed=1)
    B = rnd(K, N_, seed=2, scale=0.05) if tb else rnd(N_, K, seed=2, scale=0.05)
    outs = []
    try:
        N.lib().oasr_gemm_force_general(4)  # force the ping-pong kernel
        for v in (2, 7):
            N.check(N.lib().oasr_gemm_set_variant(v), "variant")
            if ta:  # wgrad layout: fp32 atomic output
                o = torch.zeros(M, N_, device=DEV)
                ops().gemm(A, B, M, N_, K, ta=ta, tb=tb, out_f32=o, atomic=True, split_k=1)
            else:
                o = torch.full((M, N_), float("nan"), device=DEV, dtype=BF)
                ops().gemm(A, B, M, N_, K, ta=ta, tb=tb, out=o)
            outs.append(o)
    finally:
        N.lib().oasr_gemm_force_general(0)
        N.lib().oasr_gemm_set_variant(-1)
    assert torch.equal(outs[0], outs[1])
    Af = A.float().t() if ta else A.float()
    Bf = B.float().t() if tb else B.float()
    close(outs[1], Af @ Bf.t(), name="ping-pong schedule 7")


def test_gemm_epilogues(gemm_path):
    M, N, K = 300, 256, 192
    A, B = rnd(M, K, seed=3), rnd(N, K, seed=4, scale=0.1)
    bias = rnd(N, seed=31).float()  # seeded: an unseeded draw occasionally lands an output on a bf16 rounding tie
    resid = rnd(M, N, seed=5)
    ref = A.float() @ B.float().t() + bias
    out, pre = torch.empty(M, N, device=DEV, dtype=BF), torch.empty(M, N, device=DEV, dtype=BF)
    ops().gemm(A, B, M, N, K, bias=bias, act=1, out=out, out_pre=pre)
    close(pre, ref, name="pre-activation")
    close(out, F.gelu(pre.float()), name="gelu(out_pre)")
    ops().gemm(A, B, M, N, K, bias=bias, resid=resid, out=out)
    close(out, ref.to(BF).float() + resid.float(), name="residual")
    pos = rnd(100, N, seed=32).float()
    ops().gemm(A, B, M, N, K, bias=bias, act=1, pos=pos, pos_period=100, out=out)
    close(out, F.gelu(ref.to(BF).float()).to(BF).float() + pos[torch.arange(M, device=DEV) % 100], name="gelu+pos")
    u = rnd(M, N, seed=6)
    ops().gemm(A, B, M, N, K, dgelu_u=u, out=out)
    uf = u.float().cpu().requires_grad_(True)
    F.gelu(uf).sum().backward()
    close(out, (A.float() @ B.float().t()).to(BF).float() * uf.grad.to(DEV), name="dgelu")
    # act == 2 (training forward of mlp.0): out = gelu(pre), out_pre = gelu'(pre); the dgrad consumes it with dgelu_deriv
    dsave = torch.empty(M, N, device=DEV, dtype=BF)
    ops().gemm(A, B, M, N, K, bias=bias, act=2, out=out, out_pre=dsave)
    pf = pre.float().cpu().requires_grad_(True)
    F.gelu(pf).sum().backward()
    close(out, F.gelu(pre.float()), name="act=2 gelu")
    close(dsave, pf.grad.to(DEV), name="act=2 saved gelu'")
    out2 = torch.empty(M, N, device=DEV, dtype=BF)
    ops().gemm(A, B, M, N, K, dgelu_u=dsave, dgelu_deriv=True, out=out2)
    close(out2, (A.float() @ B.float().t()).to(BF).float() * dsave.float(), name="dgelu from the saved derivative")
    c32 = torch.ones(M, N, device=DEV)
    ops().gemm(A, B, M, N, K, out_f32=c32, beta=1.0)
    close(c32, A.float() @ B.float().t() + 1.0, rtol=1e-4, atol=1e-3, name="f32 beta=1")
    c32.zero_()
    ops().gemm(A, B, M, N, K, out_f32=c32, atomic=True, split_k=3)
    close(c32, A.float() @ B.float().t(), rtol=1e-4, atol=1e-3, name="split-k atomic")


def test_gemm_wgrad_shape(gemm_path):
    """dW[N,K] += dY[M,N]^T X[M,K] with a long ragged token dimension and split-K atomics (TN layout)."""
    Mtok, N, K = 3000, 384, 256
    dY, X = rnd(Mtok, N, seed=7, scale=0.05), rnd(Mtok, K, seed=8)
    dW = torch.zeros(N, K, device=DEV)
    ops().gemm(dY, X, N, K, Mtok, ta=True, tb=True, out_f32=dW, atomic=True, split_k=4)
    close(dW, dY.float().t() @ X.float(), rtol=1e-3, atol=1e-2, name="wgrad")
    for split in (8, 16):  # multiples of 8 take the XCD-owned K-range mapping
        dW.zero_()
        ops().gemm(dY, X, N, K, Mtok, ta=True, tb=True, out_f32=dW, atomic=True, split_k=split)
        close(dW, dY.float().t() @ X.float(), rtol=1e-3, atol=1e-2, name=f"wgrad split {split}")


@pytest.mark.parametrize("which", ["conv1", "conv2"])
def test_gemm_conv_windows(which):
    """Conv1d(k=3,p=1[,s=2]) as a window GEMM over a time-major activation, against F.conv1d."""
    from olmoasr_amd import _native as N_
    o = ops()
    B_ = 2
    if which == "conv1":
        ci, co, T, stride = 80, 128, 3000, 1
    else:
        ci, co, T, stride = 128, 128, 3000, 2
    x = rnd(B_, T, ci, seed=9)  # time-major
    w = (torch.randn(co, ci, 3, generator=torch.Generator().manual_seed(10)) * 0.05).to(BF)
    ldk = 256 if which == "conv1" else 3 * ci
    wp = torch.zeros(co, ldk, dtype=BF)
    wp[:, :3 * ci] = w.permute(0, 2, 1).reshape(co, 3 * ci)  # k = kk*ci + c
    wp = wp.to(DEV)
    Tout = T // stride
    view = N_.Operand(x.data_ptr(), ci * stride, Tout, T * ci, ci, 3 * ci, (2 * ci) if stride == 1 else 3 * ci)
    out = torch.empty(B_ * Tout, co, device=DEV, dtype=BF)
    o.gemm(None, wp, B_ * Tout, co, ldk, a_view=view, out=out)
    ref = F.conv1d(x.float().permute(0, 2, 1), w.float().to(DEV), stride=stride, padding=1).permute(0, 2, 1).reshape(B_ * Tout, co)
    close(out, ref, name=which)
    # wgrad through the same window view: dWp[co, ldk] = dY^T . windows
    dY = rnd(B_ * Tout, co, seed=11, scale=0.1)
    dWp = torch.zeros(co, ldk, device=DEV)
    o.gemm(dY, None, co, ldk, B_ * Tout, ta=True, tb=True, b_view=view, out_f32=dWp, atomic=True, split_k=2)
    xf = x.float().permute(0, 2, 1).detach().requires_grad_(False)
    wf = w.float().to(DEV).requires_grad_(True)
    y = F.conv1d(xf, wf, stride=stride, padding=1)
    y.backward(dY.float().view(B_, Tout, co).permute(0, 2, 1))
    ref_w = wf.grad.permute(0, 2, 1).reshape(co, 3 * ci)
    close(dWp[:, :3 * ci], ref_w, rtol=1e-3, atol=2e-2 * float(ref_w.abs().mean()) + 1e-6, name=which + " wgrad")


# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,d", [(1000, 384), (37, 512), (4096, 1024), (130, 1280)])
def test_layernorm(rows, d):
    x = rnd(rows, d, seed=12, scale=2.0)
    gamma = 1 + 0.1 * rnd(d, seed=33).float()
    beta = 0.1 * rnd(d, seed=34).float()
    y, mean, rstd = ops().layernorm_fwd(x, gamma, beta)
    xf = x.float().detach().requires_grad_(True)
    gf, bf_ = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    ref = F.layer_norm(xf, (d,), gf, bf_, 1e-5)
    close(y, ref, name="ln fwd")
    close(mean, xf.mean(-1), rtol=1e-4, atol=1e-5, name="mean")
    dy, dres = rnd(rows, d, seed=13), rnd(rows, d, seed=14)
    dx, dg, db = ops().layernorm_bwd(dy, x, gamma, mean, rstd, dres)
    ref.backward(dy.float())
    close(dx, xf.grad.to(BF).float() + dres.float(), name="ln dx")
    close(dg, gf.grad, rtol=2e-3, atol=2e-3 * float(gf.grad.abs().mean()) + 1e-4, name="dgamma")
    close(db, bf_.grad, rtol=2e-3, atol=2e-3 * float(bf_.grad.abs().mean()) + 1e-4, name="dbeta")


# ------------------------------------------------------------------------------------------------------------
def ref_attention(q, k, v, kv_len, causal):
    B, Tq, H, D = q.shape
    Tk = k.shape[1]
    qf, kf, vf = (t.float().permute(0, 2, 1, 3) for t in (q, k, v))
    s = qf @ kf.transpose(-1, -2) / 8.0
    mask = torch.zeros(B, 1, Tq, Tk, device=q.device, dtype=torch.bool)
    if causal:
        mask |= torch.ones(Tq, Tk, device=q.device, dtype=torch.bool).triu(1)
    if kv_len is not None:
        mask |= torch.arange(Tk, device=q.device)[None, None, None, :] >= kv_len[:, None, None, None]
    s = s.masked_fill(mask, float("-inf"))
    p = torch.softmax(s, -1)
    o = (p @ vf).permute(0, 2, 1, 3).reshape(B, Tq, H * D)
    return o, torch.logsumexp(s, -1)


ATTN_CASES = [
    dict(B=2, H=3, Tq=1500, Tk=1500, causal=False, kv=False),   # encoder self-attention
    dict(B=3, H=2, Tq=448, Tk=448, causal=True, kv=True),       # decoder self-attention with key padding
    dict(B=2, H=2, Tq=448, Tk=1500, causal=False, kv=False),    # cross-attention
    dict(B=1, H=1, Tq=70, Tk=70, causal=True, kv=False),        # ragged small
    dict(B=2, H=2, Tq=5, Tk=200, causal=False, kv=False),       # decode-like
]


@pytest.fixture(params=[1, 0], ids=["pingpong", "general"])
def attn_path(request):
    """1 = default dispatch (8-wave ping-pong kernels for the unmasked cases), 0 = the general (maskable) kernels for everything."""
    from olmoasr_amd import _native as N
    N.lib().oasr_attention_set_pingpong(request.param)
    yield request.param
    N.lib().oasr_attention_set_pingpong(1)


ATTN_CASES += [
    dict(B=1, H=2, Tq=300, Tk=1000, causal=False, kv=False),    # ragged: 2 query blocks of 256 (one partial), 16 key tiles = 4 ring rounds
    dict(B=2, H=1, Tq=257, Tk=65, causal=False, kv=False),      # one query row in the second block, one key in the second tile
]


@pytest.mark.parametrize("case", ATTN_CASES)
def test_attention_fwd_bwd(case, attn_path):
    if attn_path == 0 and (case["causal"] or case["kv"]):
        pytest.skip("masked cases always run the general kernels")
    B, H, Tq, Tk = case["B"], case["H"], case["Tq"], case["Tk"]
    d = H * 64
    # fused-qkv style strided views, exactly as the engine lays them out
    if Tq == Tk:
        qkv = rnd(B, Tq, 3 * d, seed=15)
        q, k, v = (qkv[:, :, i * d:(i + 1) * d].unflatten(2, (H, 64)) for i in range(3))
    else:
        qb, kvb = rnd(B, Tq, d, seed=16), rnd(B, Tk, 2 * d, seed=17)
        q = qb.unflatten(2, (H, 64))
        k, v = (kvb[:, :, i * d:(i + 1) * d].unflatten(2, (H, 64)) for i in range(2))
    kv_len = None
    if case["kv"]:
        kv_len = torch.tensor([7, 220, 448][:B], dtype=torch.int32, device=DEV)
    o, lse, o_lo = ops().attention_fwd(q, k, v, kv_len, case["causal"], want_o_lo=True)
    o32 = o.float() + o_lo.float()  # O and its bf16 rounding residual: fp32-grade O in 4 bytes per element
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    ro, rlse = ref_attention(qr, kr, vr, kv_len, case["causal"])
    close(o, ro, atol=2e-3 + 1e-2 * float(ro.abs().mean()), name="attn o")
    close(lse, rlse, rtol=1e-3, atol=2e-3, name="lse")
    close(o32, ro, rtol=5e-3, atol=5e-3 * float(ro.abs().max()), name="attn o32")  # only P's bf16 rounding left
    d_o = rnd(B, Tq, d, seed=18, scale=0.5)
    dq, dk, dv = ops().attention_bwd(q, k, v, o, lse, d_o, kv_len, case["causal"], o_lo=o_lo)
    dq2, dk2, dv2 = ops().attention_bwd(q, k, v, o, lse, d_o, kv_len, case["causal"])  # delta from the bf16 O
    # fused query / value bias gradients: column sums of the STORED bf16 dq / dv, accumulated into fp32
    csq, csv = torch.full((d,), 0.25, device=DEV), torch.full((d,), -0.5, device=DEV)
    dq3, _, dv3 = ops().attention_bwd(q, k, v, o, lse, d_o, kv_len, case["causal"], o_lo=o_lo, dq_colsum=csq, dv_colsum=csv)
    assert torch.equal(dq3, dq) and torch.equal(dv3, dv)
    wq, wv = dq.float().sum((0, 1)).reshape(d) + 0.25, dv.float().sum((0, 1)).reshape(d) - 0.5
    close(csq, wq, rtol=1e-4, atol=1e-3 * float(wq.abs().max()) + 1e-4, name="fused dq column sums")
    close(csv, wv, rtol=1e-4, atol=1e-3 * float(wv.abs().max()) + 1e-4, name="fused dv column sums")
    ro.backward(d_o.float())
    for nm, got, ref in (("dq", dq, qr.grad), ("dk", dk, kr.grad), ("dv", dv, vr.grad)):
        # dS/P are rounded to bf16 before the second MFMA: error is relative to the largest entries of a row
        close(got, ref, rtol=2e-2, atol=5e-3 * float(ref.abs().max()) + 1e-3, name=nm)
    close(dq2, qr.grad, rtol=3e-2, atol=1e-2 * float(qr.grad.abs().max()) + 1e-3, name="dq (bf16-O delta)")


@pytest.mark.parametrize("kind", ["decoder-self", "cross", "cross-ragged", "all-zero", "dense"])
def test_attention_bwd_skips_zero_gradient_tiles_exactly(kind, attn_path):
    """d_o rows of decoder positions the loss ignores are exactly zero; with the qtile_flags workspace the dQ kernel records the
    all-zero 64-query tiles, a block of them leaves dQ = 0 without touching K / V, and the dK/dV kernel stops at the last non-zero
    tile.  Must be bit-identical to the run without the workspace (it only removes additions of zero)."""
    B, H = 3, 2
    d = H * 64
    lens = {"decoder-self": [7, 130, 300], "cross": [20, 64, 201], "cross-ragged": [1, 448, 65], "all-zero": [0, 0, 0], "dense": [448, 448, 448]}[kind]
    causal = kind == "decoder-self"
    Tq, Tk = 448, (448 if causal else 1500)
    if causal:
        qkv = rnd(B, Tq, 3 * d, seed=41)
        q, k, v = (qkv[:, :, i * d:(i + 1) * d].unflatten(2, (H, 64)) for i in range(3))
        kv_len = torch.tensor([max(n, 1) for n in lens], dtype=torch.int32, device=DEV)
    else:
        qb, kvb = rnd(B, Tq, d, seed=42), rnd(B, Tk, 2 * d, seed=43)
        q = qb.unflatten(2, (H, 64))
        k, v = (kvb[:, :, i * d:(i + 1) * d].unflatten(2, (H, 64)) for i in range(2))
        kv_len = None
    o, lse, o_lo = ops().attention_fwd(q, k, v, kv_len, causal, want_o_lo=True)
    d_o = rnd(B, Tq, d, seed=44, scale=0.5)
    for b, n in enumerate(lens):
        d_o[b, n:] = 0
    ref = ops().attention_bwd(q, k, v, o, lse, d_o, kv_len, causal, o_lo=o_lo)
    flags = torch.full((B, H, (Tq + 63) // 64), -7, dtype=torch.int32, device=DEV)
    cs, cv = torch.zeros(d, device=DEV), torch.zeros(d, device=DEV)
    got = ops().attention_bwd(q, k, v, o, lse, d_o, kv_len, causal, o_lo=o_lo, dq_colsum=cs, dv_colsum=cv, qtile_flags=flags)
    for name, a_, b_ in zip(("dq", "dk", "dv"), got, ref):
        assert torch.equal(a_, b_), (name, float((a_.float() - b_.float()).abs().max()))
    want = torch.tensor([[[1 if t * 64 < n else 0 for t in range((Tq + 63) // 64)] for _ in range(H)] for n in lens], dtype=torch.int32)
    assert torch.equal(flags.cpu(), want), (flags.cpu(), want)
    close(cs, ref[0].float().sum((0, 1)).reshape(d), rtol=1e-4, atol=1e-3 * float(ref[0].float().abs().max()) + 1e-4, name="dq column sums")
    close(cv, ref[2].float().sum((0, 1)).reshape(d), rtol=1e-4, atol=1e-3 * float(ref[2].float().abs().max()) + 1e-4, name="dv column sums")


def test_attention_bwd_delta_precision():
    """When mean(V) dominates V's variation (LayerNorm'ed encoder output + value bias -- the cross-attention case), dP and
    delta = rowsum(dO*O) nearly cancel; taking delta from the bf16-rounded O then costs several % of dQ/dK.  The
    engine therefore keeps O's bf16 rounding residual next to O for the backward (o + o_lo is fp32-grade); this test pins
    the improvement."""
    B, H, Tq, Tk = 2, 2, 448, 1500
    d = H * 64
    g = torch.Generator().manual_seed(23)
    qb = (torch.randn(B, Tq, d, generator=g) * 0.3).to(BF).to(DEV)
    kv = torch.randn(B, Tk, 2 * d, generator=g) * 0.3
    kv[:, :, d:] += 3.0 * torch.randn(1, 1, d, generator=g)  # strong common component in V
    kvb = kv.to(BF).to(DEV)
    q = qb.unflatten(2, (H, 64))
    k, v = (kvb[:, :, i * d:(i + 1) * d].unflatten(2, (H, 64)) for i in range(2))
    o, lse, o_lo = ops().attention_fwd(q, k, v, None, False, want_o_lo=True)
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    ro, _ = ref_attention(qr, kr, vr, None, False)
    d_o = rnd(B, Tq, d, seed=24, scale=0.5)
    ro.backward(d_o.float())
    rel = {}
    for tag, lo_arg in (("fp32O", o_lo), ("bf16O", None)):
        dq, dk, dv = ops().attention_bwd(q, k, v, o, lse, d_o, None, False, o_lo=lo_arg)
        rel[tag] = [float((a.float() - b).norm() / b.norm()) for a, b in ((dq, qr.grad), (dk, kr.grad), (dv, vr.grad))]
    print("rel L2 err (dq, dk, dv):", rel)
    assert max(rel["fp32O"][:2]) < 0.02
    assert rel["fp32O"][0] < 0.5 * rel["bf16O"][0] or rel["bf16O"][0] < 0.01


# ------------------------------------------------------------------------------------------------------------
def test_cross_entropy():
    rows, V, ld, ignore = 300, 51865, 51968, 51864
    g = torch.Generator().manual_seed(19)
    logits = torch.zeros(rows, ld, dtype=BF)
    logits[:, :V] = (torch.randn(rows, V, generator=g) * 3).to(BF)
    tgt = torch.randint(0, 50257, (rows,), generator=g)
    tgt[::7] = ignore
    tgt[5] = 51863
    lf = logits[:, :V].float().to(DEV).requires_grad_(True)
    ref = F.cross_entropy(lf, tgt.to(DEV), ignore_index=ignore)
    (ref * 4.0).backward()
    lg = logits.to(DEV)
    loss, row_loss = ops().cross_entropy_(lg, V, tgt.to(DEV), ignore, gscale=4.0)
    assert abs(float(loss) - float(ref)) < 1e-4 * abs(float(ref))
    close(lg[:, :V], lf.grad, rtol=1e-2, atol=1e-7, name="dlogits")
    assert float(lg[:, V:].float().abs().max()) == 0.0
    assert float(lg[::7].float().abs().max()) == 0.0


def test_cross_entropy_gradient_is_the_fp32_gradient_rounded_once():
    """d(logits) at ulp level (the end-to-end comparison of the autograd bridge with the fused path allows 2e-2 rel-L2 because the two
    formulas break bf16 ties differently; this pins the fused kernel's own output): every stored bf16 value is within ONE bf16 ulp of
    the float64 gradient (softmax - onehot) * g / n_valid, and all but a handful are its correctly rounded value."""
    rows, V, ld, ignore = 257, 51865, 51968, 51864
    g = torch.Generator().manual_seed(23)
    logits = torch.zeros(rows, ld, dtype=BF)
    logits[:, :V] = (torch.randn(rows, V, generator=g) * 2.5).to(BF)
    tgt = torch.randint(0, 50257, (rows,), generator=g)
    tgt[::5] = ignore
    lg = logits.to(DEV)
    ops().cross_entropy_(lg, V, tgt.to(DEV), ignore, gscale=1024.0)
    got = lg[:, :V].float().cpu().double()
    lf = logits[:, :V].double()
    p = torch.softmax(lf, -1)
    onehot = torch.zeros_like(p)
    valid = tgt != ignore
    onehot[valid, tgt[valid]] = 1.0
    want = (p - onehot) * (1024.0 / int(valid.sum()))
    want[~valid] = 0.0
    want_bf = want.float().to(BF).double()
    # one bf16 ulp of |want| (8 bits of precision: 2^(floor(log2|x|) - 7)); zeros must be exact zeros
    ulp = torch.where(want == 0, torch.zeros_like(want), torch.exp2(torch.floor(torch.log2(want.abs().clamp_min(1e-300))) - 7))
    err = (got - want).abs()
    assert bool((err <= ulp * 1.0001 + 1e-300).all()), f"max error {float((err / ulp.clamp_min(1e-300)).max()):.3f} ulp"
    off = int((got != want_bf).sum())
    assert off <= 2e-3 * got.numel(), f"{off} of {got.numel()} values are not the correctly rounded gradient"
    assert float(got[~valid].abs().max()) == 0.0


@pytest.mark.parametrize("tb", [False, True])
def test_gemm_fused_column_sum(tb, gemm_path):
    """Bias gradient fused into the dgrad epilogue (NN fast path) and its unfused fallback (other layouts / kernels)."""
    M, N, K = 1000, 384, 256
    A = rnd(M, K, seed=31)
    B = rnd(K, N, seed=32, scale=0.1) if tb else rnd(N, K, seed=32, scale=0.1)
    u = rnd(M, N, seed=33)
    out = torch.empty(M, N, device=DEV, dtype=BF)
    cs = torch.full((N,), 0.5, device=DEV)
    ops().gemm(A, B, M, N, K, tb=tb, dgelu_u=u, out=out, colsum=cs)
    close(cs, out.float().sum(0) + 0.5, rtol=1e-4, atol=1e-3, name="fused colsum == column sums of the stored output")


@pytest.mark.parametrize("M,N,K", [(1, 768, 768), (20, 2304, 768), (33, 776, 3072), (64, 51864, 384), (8, 40, 64)])
def test_gemm_skinny_decode_shapes(M, N, K):
    """Decode-sized GEMMs (a few token rows x a whole weight matrix) take the skinny kernel: plain, bias + GELU (+pre),
    bias + residual, and fp32 output, against fp32 torch with the autocast rounding points."""
    A, B = rnd(M, K, seed=11), rnd(N, K, seed=12, scale=0.05)
    bias = rnd(N, seed=35).float()
    ref = A.float() @ B.float().t()
    out = torch.full((M, N), float("nan"), device=DEV, dtype=BF)
    ops().gemm(A, B, M, N, K, out=out)
    close(out, ref, name="skinny plain")
    pre = torch.empty_like(out)
    ops().gemm(A, B, M, N, K, bias=bias, act=1, out=out, out_pre=pre)
    close(pre, ref + bias, name="skinny pre-activation")
    close(out, F.gelu(pre.float()), name="skinny gelu")
    resid = rnd(M, N, seed=13)
    ops().gemm(A, B, M, N, K, bias=bias, resid=resid, out=out)
    close(out, (ref + bias).to(BF).float() + resid.float(), name="skinny residual")
    o32 = torch.full((M, N), float("nan"), device=DEV)
    ops().gemm(A, B, M, N, K, out_f32=o32)
    close(o32, ref, rtol=2e-3, atol=2e-3, name="skinny fp32 out")


@pytest.mark.parametrize("Tk,kv", [(1, False), (37, False), (448, True), (1500, False)])
def test_attention_decode_step_kernel(Tk, kv):
    """Tq == 1 takes the decode-step kernel (one query row per (batch, head), K/V streamed once): strided cache layouts
    (q | k | v interleaved rows, as the KV cache stores them), optional per-sequence lengths."""
    B, H = 3, 4
    d = H * 64
    cache = rnd(B, Tk, 3 * d, seed=41)                      # [q | k | v] per position
    q = cache[:, Tk - 1:Tk, :d].unflatten(2, (H, 64))       # the query lives in the last position's row
    k = cache[:, :, d:2 * d].unflatten(2, (H, 64))
    v = cache[:, :, 2 * d:].unflatten(2, (H, 64))
    kv_len = torch.tensor([Tk, max(1, Tk // 2), max(1, Tk - 3)], dtype=torch.int32, device=DEV) if kv else None
    o, lse = ops().attention_fwd(q, k, v, kv_len, False)
    ro, rlse = ref_attention(q, k, v, kv_len, False)
    close(o, ro, atol=2e-3 + 1e-2 * float(ro.abs().mean()), name=f"decode attn o Tk={Tk}")
    close(lse, rlse, rtol=1e-3, atol=2e-3, name="decode attn lse")


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices")
def test_operands_on_different_devices_are_refused_before_the_launch():
    from olmoasr_amd import _native as N
    x = rnd(8, 64)
    gamma, beta = torch.ones(64, device="cuda:1"), torch.zeros(64, device="cuda:1")
    with pytest.raises(N.NativeError, match="oasr_layernorm_fwd: arguments on cuda:0 and on cuda:1"):
        ops().layernorm_fwd(x, gamma, beta)
