"""CPU-side checks of the staged autograd entries (ABI 214): the ABI generation, the new exports and their argument
refusals, and the workspace plans -- the fused modes keep exactly the parent's sizes, the stage plans are the fused one cut in two.
No compute: the contexts are only planned (oasr_workspace_bytes is a dry run), the entries are called with null pointers."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("oasr_train_encode", "oasr_train_encode_bwd", "oasr_train_decode", "oasr_train_decode_bwd", "oasr_train_step")
# oasr_workspace_bytes of the library before the stage entries existed (ABI 213), per (variant, compute dtype): (B, S, mode) -> bytes
PINNED = {
    ("tiny", 0): {(2, 448, 0): 170051584, (2, 448, 1): 392684800, (128, 448, 0): 10882373632, (128, 448, 1): 24992949248},
    ("tiny", 1): {(2, 448, 0): 339501824, (2, 448, 1): 781727744, (128, 448, 0): 21727076096, (128, 448, 1): 49891584768},
    ("medium", 0): {(2, 448, 0): 296462592, (2, 448, 1): 4047388672, (128, 448, 0): 18972609792, (128, 448, 1): 258163172608},
    ("medium", 1): {(2, 448, 0): 592132352, (2, 448, 1): 8070762496, (128, 448, 0): 37895280896, (128, 448, 1): 515658903808},
}


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    from olmoasr_amd import _native
    if not os.path.isfile(_native.LIB_PATH):
        g.build()
    return _native


def _ctx(native, variant, cdt=0):
    from oracle import model_oracle as mo
    dims = mo.VARIANTS[variant]
    cd = native.Dims(*[getattr(dims, f[0]) for f in native.Dims._fields_])
    ctx = native.lib().oasr_create_ex2(ctypes.byref(cd), dims.n_vocab + 1, cdt)
    assert ctx
    return ctx


def test_abi_214_and_exports(native):
    lib = native.lib()
    hdr = open(os.path.join(ROOT, "include", "oasr.h")).read()
    assert int(re.search(r"#define\s+OASR_ABI_VERSION\s+(\d+)", hdr).group(1)) == 216  # (215 adds test hooks only; 216 moves the fused step from a given xa into oasr_train_step)
    assert lib.oasr_version() == 216 == native.ABI_VERSION
    for name, val in (("OASR_MODE_TRAIN_ENC", native.MODE_TRAIN_ENC), ("OASR_MODE_TRAIN_DEC", native.MODE_TRAIN_DEC)):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", hdr).group(1)) == val
    for n in ENTRIES:
        assert re.search(rf"\b{n}\s*\(", hdr), n
        assert hasattr(lib, n) and n in native.EXPORTS, n


def test_null_context_and_null_pointers_are_refused(native):
    lib = native.lib()
    step = native.TrainStepArgs(B=2, S=448, loss_scale=1.0, inv_accum=1.0)  # every pointer null
    for call in (lambda c: lib.oasr_train_encode(c, None, 2, None, None, 0, None),
                 lambda c: lib.oasr_train_encode_bwd(c, None, 2, None, None, 0, None),
                 lambda c: lib.oasr_train_decode(c, None, None, None, 2, 448, None, None, 0, None),
                 lambda c: lib.oasr_train_decode_bwd(c, None, None, None, 2, 448, None, None, 0, None),
                 lambda c: lib.oasr_train_step(c, ctypes.byref(step), None, 0, None)):
        assert call(None) != 0
        assert lib.oasr_last_error()
    # a context that is not bound yet is refused before any pointer is looked at; bound to fake (never dereferenced) addresses, the
    # missing pointers are named
    ctx = _ctx(native, "tiny")
    try:
        assert lib.oasr_train_encode(ctx, None, 2, None, None, 0, None) == -3  # OASR_ESTATE: not bound
        fake = ctypes.c_void_p(1 << 40)
        assert lib.oasr_bind(ctx, fake, fake, None, None, fake) == 0
        assert lib.oasr_bind_shadow(ctx, fake) == 0
        assert lib.oasr_train_encode(ctx, None, 2, None, None, 0, None) == -1
        assert b"mel" in lib.oasr_last_error()
        assert lib.oasr_train_encode_bwd(ctx, None, 2, None, None, 0, None) == -1
        assert b"dxa" in lib.oasr_last_error()
        assert lib.oasr_train_decode(ctx, None, None, None, 2, 448, None, None, 0, None) == -1
        assert b"tokens" in lib.oasr_last_error()
        assert lib.oasr_train_decode_bwd(ctx, None, None, None, 2, 448, None, None, 0, None) == -1
        assert b"dlogits" in lib.oasr_last_error()
        assert lib.oasr_train_step(ctx, ctypes.byref(step), None, 0, None) == -1
        assert b"xa" in lib.oasr_last_error()
        assert lib.oasr_train_decode(ctx, fake, fake, fake, 2, 449, fake, fake, 1 << 40, None) == -1  # S > n_text_ctx
    finally:
        lib.oasr_destroy(ctx)


@pytest.mark.parametrize("variant", ["tiny", "medium"])
@pytest.mark.parametrize("cdt", [0, 1])
def test_fused_workspace_sizes_are_unchanged(native, variant, cdt):
    lib = native.lib()
    ctx = _ctx(native, variant, cdt)
    try:
        for (B, S, mode), want in PINNED[(variant, cdt)].items():
            assert lib.oasr_workspace_bytes(ctx, B, S, mode) == want, (variant, cdt, B, S, mode)
        assert lib.oasr_workspace_bytes(ctx, 2, 448, 4) == 0 and lib.oasr_workspace_bytes(ctx, 2, 448, -1) == 0  # unknown modes
    finally:
        lib.oasr_destroy(ctx)


@pytest.mark.parametrize("cdt", [0, 1])
def test_stage_plans_cut_the_fused_plan(native, cdt):
    """medium, B = 128, S = 448: the decoder stage needs well under half of the fused plan (the per-layer cross-attention K / V over the
    encoder rows dominate it: about 0.35), the encoder stage less than the fused plan, the two together at most 10 % more."""
    lib = native.lib()
    ctx = _ctx(native, "medium", cdt)
    try:
        train, enc, dec = (lib.oasr_workspace_bytes(ctx, 128, 448, m) for m in (native.MODE_TRAIN, native.MODE_TRAIN_ENC, native.MODE_TRAIN_DEC))
        assert dec < 0.5 * train
        assert enc < train
        assert enc + dec <= 1.1 * train
        # the encoder stage's plan does not depend on the text context; the decoder's shrinks with it
        assert lib.oasr_workspace_bytes(ctx, 128, 1, native.MODE_TRAIN_ENC) == enc
        assert lib.oasr_workspace_bytes(ctx, 128, 224, native.MODE_TRAIN_DEC) < dec
    finally:
        lib.oasr_destroy(ctx)

