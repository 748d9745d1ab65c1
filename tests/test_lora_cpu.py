"""LoRA adapters without a GPU: target resolution and its refusals, the train script's flags, the adapter parameter table of
oasr_create_ex3 (pure host code), and -- in float64 -- the weight-space identities the engine's adapter gradients rest on
(DESIGN.md section 3c):  dB = s * dW @ A^T,  dA = s * B^T @ dW  with dW = dL/dW of W = W0 + s * B @ A."""
import ctypes as C
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _module_names(n_enc=2, n_dec=2):
    """The module tree of OLMoASR (named_modules() names), built by hand: no device needed."""
    names = ["encoder", "encoder.conv1", "encoder.conv2", "encoder.blocks", "encoder.ln_post", "decoder", "decoder.token_embedding",
             "decoder.blocks", "decoder.ln"]
    for side, n, cross in (("encoder", n_enc, False), ("decoder", n_dec, True)):
        for i in range(n):
            p = f"{side}.blocks.{i}"
            names += [p, f"{p}.attn", f"{p}.attn.query", f"{p}.attn.key", f"{p}.attn.value", f"{p}.attn.out", f"{p}.attn_ln"]
            if cross:
                names += [f"{p}.cross_attn", f"{p}.cross_attn.query", f"{p}.cross_attn.key", f"{p}.cross_attn.value", f"{p}.cross_attn.out",
                          f"{p}.cross_attn_ln"]
            names += [f"{p}.mlp", f"{p}.mlp.0", f"{p}.mlp.2", f"{p}.mlp_ln"]
    return names


def test_resolve_targets_default_patterns():
    from olmoasr_amd.lora import DEFAULT_TARGETS, resolve_targets
    got = resolve_targets(_module_names(), DEFAULT_TARGETS)
    want = [f"{s}.blocks.{i}.attn.{k}" for s in ("encoder", "decoder") for i in range(2) for k in ("query", "value")]
    assert got == want
    assert not any("cross_attn" in n for n in got)  # "*.attn.query" does not reach the cross-attention


def test_resolve_targets_other_patterns():
    from olmoasr_amd.lora import resolve_targets
    names = _module_names()
    assert resolve_targets(names, ["decoder.*.attn.query"]) == ["decoder.blocks.0.attn.query", "decoder.blocks.1.attn.query"]
    assert resolve_targets(names, "*.cross_attn.value") == ["decoder.blocks.0.cross_attn.value", "decoder.blocks.1.cross_attn.value"]
    # a plain name selects like peft's target_modules: itself and every name ending in "." + it (cross_attn.query included)
    q = resolve_targets(names, ["query"])
    assert len(q) == 6 and all(n.endswith(".query") for n in q)
    mlp = resolve_targets(names, ["encoder.blocks.1.mlp.0", "*.mlp.2"])
    assert mlp == ["encoder.blocks.0.mlp.2", "encoder.blocks.1.mlp.0", "encoder.blocks.1.mlp.2", "decoder.blocks.0.mlp.2",
                   "decoder.blocks.1.mlp.2"]  # (in module order)


@pytest.mark.parametrize("pattern", ["decoder.token_embedding", "encoder.conv1", "*.conv2", "*.attn_ln", "*.mlp", "*.blocks.0.attn"])
def test_resolve_targets_refuses_non_block_linears(pattern):
    from olmoasr_amd.lora import resolve_targets
    with pytest.raises(ValueError, match="not a block Linear"):
        resolve_targets(_module_names(), [pattern])


def test_resolve_targets_refuses_unmatched_and_empty():
    from olmoasr_amd.lora import resolve_targets
    with pytest.raises(ValueError, match="match no module"):
        resolve_targets(_module_names(), ["*.attn.query", "*.self_attn.q_proj"])
    with pytest.raises(ValueError):
        resolve_targets(_module_names(), [])


def test_add_lora_refuses_dropout_and_rank_before_touching_the_model():
    from olmoasr_amd.lora import add_lora
    with pytest.raises(ValueError, match="lora_dropout"):
        add_lora(None, r=16, lora_dropout=0.05)
    for r in (0, 65):
        with pytest.raises(ValueError, match="rank"):
            add_lora(None, r=r)


def _train_script():
    spec = importlib.util.spec_from_file_location("tt_lora_cpu", os.path.join(ROOT, "scripts", "training", "train_timestamps.py"))
    tt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tt)
    return tt


def test_train_script_lora_flags():
    tt = _train_script()
    a = tt.parse_args(["--lora_rank=16", "--lora_alpha=32"])
    assert a.lora_rank == 16 and a.lora_alpha == 32 and a.lora_targets == ("*.attn.query", "*.attn.value")
    a = tt.parse_args(["--lora_rank", "8", "--lora_targets", "decoder.*.attn.query,decoder.*.attn.value"])
    assert a.lora_rank == 8 and a.lora_targets == ("decoder.*.attn.query", "decoder.*.attn.value")
    d = tt.parse_args([])
    assert d.lora_rank == 0 and not d.freeze_encoder  # adapters are opt-in; every other default is the reference's / as before
    for k, v in tt.REFERENCE_FLAGS.items():
        if k != "ckpt_file_name":
            assert d[k] == v, k
    with pytest.raises(SystemExit):
        tt.parse_args(["--lora_rank=-1"])


# ---- the adapter parameter table (oasr_create_ex3 is host code: no device needed) ----------------------------------------------
def _lib():
    from olmoasr_amd import _native as N
    try:
        return N, N.lib()
    except N.NativeError as e:  # pragma: no cover
        pytest.fail(f"liboasr.so must be built (__graft_entry__.build()): {e}")


def _table(N, lib, ctx):
    out = []
    for i in range(lib.oasr_param_count(ctx)):
        name = C.create_string_buffer(128)
        off, numel, ndim = C.c_int64(), C.c_int64(), C.c_int()
        shape = (C.c_int64 * 4)()
        N.check(lib.oasr_param_info(ctx, i, name, 128, C.byref(off), C.byref(numel), C.byref(ndim), shape), "param_info")
        out.append((name.value.decode(), off.value, numel.value, tuple(shape[j] for j in range(ndim.value))))
    segs = []
    for i in range(lib.oasr_segment_count(ctx)):
        o, m = C.c_int64(), C.c_int64()
        N.check(lib.oasr_segment_info(ctx, i, C.byref(o), C.byref(m)), "segment_info")
        segs.append((o.value, m.value))
    return out, segs


def _dims(N):
    from oracle import model_oracle as mo
    dm = mo.VARIANTS["tiny"]
    return N.Dims(*[getattr(dm, f[0]) for f in N.Dims._fields_]), dm


def test_adapter_table_layout():
    N, lib = _lib()
    cd, dm = _dims(N)
    base = lib.oasr_create_ex2(C.byref(cd), dm.n_vocab + 1, 0)
    tb, sb = _table(N, lib, base)
    idx = {n: i for i, (n, *_) in enumerate(tb)}
    targets = [idx[f"decoder.blocks.1.attn.query.weight"], idx["encoder.blocks.0.attn.value.weight"], idx["decoder.blocks.0.mlp.2.weight"]]
    r = 12
    arr = (C.c_int32 * 3)(*targets)
    ctx = lib.oasr_create_ex3(C.byref(cd), dm.n_vocab + 1, 0, arr, 3, r, 2.0)
    assert ctx, lib.oasr_last_error()
    try:
        tl, sl = _table(N, lib, ctx)
        assert lib.oasr_lora_count(ctx) == 3
        names = [n for n, *_ in tl]
        d = dm.n_audio_state
        want = [("decoder.blocks.1.attn.query.lora_A", (r, d)), ("decoder.blocks.1.attn.query.lora_B", (d, r)),
                ("encoder.blocks.0.attn.value.lora_A", (r, d)), ("encoder.blocks.0.attn.value.lora_B", (d, r)),
                ("decoder.blocks.0.mlp.2.lora_A", (r, 4 * d)), ("decoder.blocks.0.mlp.2.lora_B", (d, r))]
        ad = [(n, s) for n, _, _, s in tl if ".lora_" in n]
        assert ad == want
        # every base tensor keeps name and shape; the adapters sit between the conv stem and the token embedding (still the arena's end)
        assert [n for n in names if ".lora_" not in n] == [n for n, *_ in tb]
        assert names[-1] == "decoder.token_embedding.weight" and names[-8] == "encoder.conv1.bias"
        assert all(numel % 4 == 0 for n, _, numel, _ in tl if ".lora_" in n)
        offs = [(o, m) for _, o, m, _ in tl]
        assert all(a[0] + a[1] == b[0] for a, b in zip(offs, offs[1:]))  # back to back
        assert lib.oasr_param_numel(ctx) == lib.oasr_param_numel(base) + sum(m for n, _, m, _ in tl if ".lora_" in n)
        # one segment more, the LAST one, covering exactly the adapters; the segments still tile the arena
        assert len(sl) == len(sb) + 1
        lo = min(o for n, o, _, _ in tl if ".lora_" in n)
        assert sl[-1] == (lo, sum(m for n, _, m, _ in tl if ".lora_" in n))
        assert sum(m for _, m in sl) == lib.oasr_param_numel(ctx)
        # an adapted base weight can never be trainable (refused before anything reaches the device)
        mask = (C.c_uint8 * len(tl))(*([1] * len(tl)))
        assert lib.oasr_set_trainable(ctx, mask, len(tl)) != 0
        assert b"LoRA" in lib.oasr_last_error()
    finally:
        lib.oasr_destroy(ctx)
        lib.oasr_destroy(base)
    # no adapters: exactly the ex2 context
    base = lib.oasr_create_ex2(C.byref(cd), dm.n_vocab + 1, 0)
    none = lib.oasr_create_ex3(C.byref(cd), dm.n_vocab + 1, 0, None, 0, 0, 0.0)
    try:
        assert _table(N, lib, none) == (tb, sb) and lib.oasr_lora_count(none) == 0
        assert lib.oasr_shadow_bytes(none) == lib.oasr_shadow_bytes(base)
        assert all(lib.oasr_workspace_bytes(none, 2, 448, m) == lib.oasr_workspace_bytes(base, 2, 448, m) for m in (0, 1))
    finally:
        lib.oasr_destroy(none)
        lib.oasr_destroy(base)


@pytest.mark.parametrize("bad", ["decoder.token_embedding.weight", "encoder.conv1.weight", "decoder.blocks.0.attn.query.bias",
                                 "decoder.blocks.0.mlp_ln.weight", "twice", "rank"])
def test_adapter_table_refusals(bad):
    N, lib = _lib()
    cd, dm = _dims(N)
    base = lib.oasr_create_ex2(C.byref(cd), dm.n_vocab + 1, 0)
    tb, _ = _table(N, lib, base)
    lib.oasr_destroy(base)
    idx = {n: i for i, (n, *_) in enumerate(tb)}
    q = idx["decoder.blocks.0.attn.query.weight"]
    targets, r = ([q, q], 8) if bad == "twice" else ([q], 65) if bad == "rank" else ([idx[bad]], 8)
    arr = (C.c_int32 * len(targets))(*targets)
    ctx = lib.oasr_create_ex3(C.byref(cd), dm.n_vocab + 1, 0, arr, len(targets), r, 1.0)
    assert not ctx
    assert lib.oasr_last_error()


# ---- the weight-space identities, float64 -------------------------------------------------------------------------------------------
def test_weight_space_adapter_gradients_equal_autograd():
    """For W = W0 + s B A: the adapter gradients from dW = dL/dW (the engine's path) equal autograd through (a) the parametrized weight
    (torch.nn.utils.parametrize, minLoRA style) and (b) the activation-side form x W0^T + s (x A^T) B^T -- in float64, to rounding."""
    import torch.nn.utils.parametrize as P
    g = torch.Generator().manual_seed(0)
    out_f, in_f, r, s, n = 24, 40, 4, 32 / 4, 17
    W0 = torch.randn(out_f, in_f, generator=g, dtype=torch.float64)
    A0 = torch.randn(r, in_f, generator=g, dtype=torch.float64) * 0.2
    B0 = torch.randn(out_f, r, generator=g, dtype=torch.float64) * 0.2
    bias = torch.randn(out_f, generator=g, dtype=torch.float64)
    x = torch.randn(n, in_f, generator=g, dtype=torch.float64)
    tgt = torch.randn(n, out_f, generator=g, dtype=torch.float64)

    def loss_of(y):
        return ((torch.tanh(y) - tgt) ** 2).sum()

    # the engine's route: ordinary weight gradient of the effective weight, then the projection
    W = (W0 + s * B0 @ A0).requires_grad_(True)
    loss_of(x @ W.T + bias).backward()
    dW = W.grad
    dB = s * dW @ A0.T
    dA = s * B0.T @ dW

    # (a) parametrized nn.Linear
    class LoRA(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.A = torch.nn.Parameter(A0.clone())
            self.B = torch.nn.Parameter(B0.clone())

        def forward(self, w):
            return w + s * self.B @ self.A

    lin = torch.nn.Linear(in_f, out_f, dtype=torch.float64)
    with torch.no_grad():
        lin.weight.copy_(W0)
        lin.bias.copy_(bias)
    lin.weight.requires_grad_(False)
    P.register_parametrization(lin, "weight", LoRA())
    loss_of(lin(x)).backward()
    par = lin.parametrizations.weight[0]
    assert torch.allclose(par.A.grad, dA, rtol=1e-12, atol=1e-12)
    assert torch.allclose(par.B.grad, dB, rtol=1e-12, atol=1e-12)

    # (b) activation-side form (peft's LoraLayer.forward without dropout)
    A = A0.clone().requires_grad_(True)
    B = B0.clone().requires_grad_(True)
    loss_of(x @ W0.T + bias + s * (x @ A.T) @ B.T).backward()
    assert torch.allclose(A.grad, dA, rtol=1e-12, atol=1e-12)
    assert torch.allclose(B.grad, dB, rtol=1e-12, atol=1e-12)
    # B = 0 (peft's init): dA vanishes, dB does not -- training starts from B
    assert torch.count_nonzero(s * torch.zeros_like(B0).T @ dW) == 0 and float(dB.abs().max()) > 0


def test_accumulated_projection_is_the_projection_of_the_sum():
    """The engine zeroes dW per micro-batch and accumulates the projected dA / dB (linear in dW): sum of projections == projection of the sum."""
    g = torch.Generator().manual_seed(1)
    A = torch.randn(8, 32, generator=g, dtype=torch.float64)
    B = torch.randn(16, 8, generator=g, dtype=torch.float64)
    d1, d2 = torch.randn(16, 32, generator=g, dtype=torch.float64), torch.randn(16, 32, generator=g, dtype=torch.float64)
    s = 2.0
    assert torch.allclose(s * (d1 + d2) @ A.T, s * d1 @ A.T + s * d2 @ A.T)
    assert torch.allclose(s * B.T @ (d1 + d2), s * B.T @ d1 + s * B.T @ d2)
