"""CPU-side checks of oasr_train_step's one validation function (include/oasr.h at oasr_train_step_args; csrc/engine_step.hip:
train_step_check): one row per refusal, each with its return code and a word of its message.  No compute: the context is only planned and
bound to fake addresses that are never dereferenced, and every row is refused before anything is launched."""
import ctypes
import os

import pytest

EINVAL, ESTATE = -1, -3
FAKE = 1 << 40  # a "present" pointer
B, S = 2, 448
PRESENT = dict(tokens=FAKE, targets=FAKE, text_len=FAKE, loss_out=FAKE, B=B, S=S, span_forward=1, loss_scale=1.0, inv_accum=1.0)


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    from olmoasr_amd import _native
    if not os.path.isfile(_native.LIB_PATH):
        g.build()
    return _native


def _ctx(native, n_text_ctx=448):
    from oracle import model_oracle as mo
    dims = mo.VARIANTS["tiny"]
    cd = native.Dims(*[n_text_ctx if f[0] == "n_text_ctx" else getattr(dims, f[0]) for f in native.Dims._fields_])
    ctx = native.lib().oasr_create_ex2(ctypes.byref(cd), dims.n_vocab + 1, 0)
    assert ctx, native.lib().oasr_last_error()
    return ctx


def _bound(native, n_text_ctx=448):
    """A planned context bound to fake addresses (default mask: every tensor trainable)."""
    lib = native.lib()
    ctx = _ctx(native, n_text_ctx)
    fake = ctypes.c_void_p(FAKE)
    assert lib.oasr_bind(ctx, fake, fake, None, None, fake) == 0
    assert lib.oasr_bind_shadow(ctx, fake) == 0
    return ctx


@pytest.fixture(scope="module")
def ctx(native):
    c = _bound(native)
    yield c
    native.lib().oasr_destroy(c)


def _step(native, c, ws=FAKE, ws_bytes=1 << 40, **fields):
    lib = native.lib()
    args = native.TrainStepArgs(**{**PRESENT, **fields})
    rc = lib.oasr_train_step(c, ctypes.byref(args), ctypes.c_void_p(ws) if ws else None, ws_bytes, None)
    return rc, lib.oasr_last_error() or b""


def test_null_context_null_args_and_unbound_context(native):
    lib = native.lib()
    rc, msg = _step(native, None, mel=FAKE)
    assert rc == EINVAL and b"null context" in msg
    c = _ctx(native)
    try:
        rc, msg = _step(native, c, mel=FAKE)
        assert rc == ESTATE and b"not fully bound" in msg
    finally:
        lib.oasr_destroy(c)
    c = _bound(native)
    try:
        assert lib.oasr_train_step(c, None, ctypes.c_void_p(FAKE), 1 << 40, None) == EINVAL
        assert b"null args" in lib.oasr_last_error()
    finally:
        lib.oasr_destroy(c)


REFUSED = [  # (id, fields, code, word of the message)
    ("neither_mel_nor_xa", dict(), EINVAL, b"one of mel and xa"),
    ("both_mel_and_xa", dict(mel=FAKE, xa=FAKE), EINVAL, b"one of mel and xa"),
    ("no_tokens", dict(mel=FAKE, tokens=None), EINVAL, b"tokens"),
    ("no_targets", dict(mel=FAKE, targets=None), EINVAL, b"targets"),
    ("no_text_len", dict(mel=FAKE, text_len=None), EINVAL, b"text_len"),
    ("no_loss_out", dict(mel=FAKE, loss_out=None), EINVAL, b"loss_out"),
    ("no_workspace", dict(mel=FAKE, ws=None), EINVAL, b"workspace"),
    ("B_zero", dict(mel=FAKE, B=0), EINVAL, b"B=0"),
    ("S_zero", dict(mel=FAKE, S=0), EINVAL, b"S=0"),
    ("S_past_the_context", dict(xa=FAKE, S=449), EINVAL, b"S=449"),
    ("span_over_a_trimmed_context", dict(mel=FAKE, span_host=FAKE, S=384), EINVAL, b"whole context"),
    ("span_forward_unknown", dict(mel=FAKE, span_host=FAKE, span_forward=2), EINVAL, b"span_forward"),
    ("span_with_logits_out", dict(mel=FAKE, span_host=FAKE, logits_out=FAKE), EINVAL, b"logits_out"),
    ("pred_out_without_span", dict(mel=FAKE, pred_out=FAKE), EINVAL, b"pred_out comes with span_host"),
    ("mel_clip_max_without_span", dict(mel=FAKE, mel_clip_max=FAKE), EINVAL, b"mel_clip_max comes with span_host"),
    ("xa_with_mel_clip_max", dict(xa=FAKE, span_host=FAKE, mel_clip_max=FAKE), EINVAL, b"given xa"),
    ("xa_with_logits_out", dict(xa=FAKE, logits_out=FAKE), EINVAL, b"given xa"),
    ("xa_with_a_trainable_encoder", dict(xa=FAKE), ESTATE, b"encoder tensor is trainable"),
    ("xa_span_pred_with_a_trainable_encoder", dict(xa=FAKE, span_host=FAKE, pred_out=FAKE), ESTATE, b"encoder tensor is trainable"),
]


@pytest.mark.parametrize("fields,code,word", [r[1:] for r in REFUSED], ids=[r[0] for r in REFUSED])
def test_refusals(native, ctx, fields, code, word):
    rc, msg = _step(native, ctx, **fields)
    assert rc == code and word in msg, (rc, msg)


def test_the_argument_checks_come_before_the_workspace_and_the_state(native, ctx):
    rc, msg = _step(native, ctx, xa=FAKE, logits_out=FAKE, ws_bytes=0)  # wrong three times over: the argument is named
    assert rc == EINVAL and b"given xa" in msg
    rc, msg = _step(native, ctx, xa=FAKE, ws_bytes=0)  # wrong twice: the workspace before the trainable encoder
    assert rc == EINVAL and b"workspace too small" in msg


@pytest.mark.parametrize("src,mode", [("mel", 1), ("xa", 3)])
def test_workspace_one_byte_short(native, ctx, src, mode):
    """The size asked for is oasr_workspace_bytes of the step's own mode: OASR_MODE_TRAIN from mel, OASR_MODE_TRAIN_DEC from xa.  From xa the
    exact size passes this check and meets the next one (the all-trainable mask), which pins the threshold from both sides without a launch."""
    need = native.lib().oasr_workspace_bytes(ctx, B, S, mode)
    assert need > 4096
    rc, msg = _step(native, ctx, ws_bytes=need - 1, **{src: FAKE})
    assert rc == EINVAL and b"workspace too small" in msg
    if src == "xa":
        assert native.lib().oasr_workspace_bytes(ctx, B, S, 1) > need  # (the fused plan's size would not tell the two modes apart)
        rc, msg = _step(native, ctx, ws_bytes=need, xa=FAKE)
        assert rc == ESTATE and b"encoder tensor is trainable" in msg


def test_pred_out_on_a_shape_the_row_table_cannot_chunk(native):
    lib = native.lib()
    c = _bound(native, n_text_ctx=100)  # not a multiple of 64
    try:
        rc, msg = _step(native, c, mel=FAKE, span_host=FAKE, pred_out=FAKE, S=100)
        assert rc == EINVAL and b"chunk-row table" in msg and b"n_text_ctx = 100" in msg
    finally:
        lib.oasr_destroy(c)
