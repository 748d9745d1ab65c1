"""CPU-side checks of label smoothing and z-loss in the fused step (include/oasr.h at oasr_train_step_args.label_smoothing; DESIGN.md section
3j): the struct grows at its end under ABI 216, train_step_check refuses bad values before anything is launched or dereferenced (the context is
bound to fake addresses, as in test_train_step_args_cpu.py), the Python surface raises ValueError for the same conditions, and the training
script parses and validates --label_smoothing / --z_loss."""
import ctypes
import importlib.util
import math
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
FAKE = 1 << 40  # a "present" pointer, never dereferenced
B, S = 2, 448
PRESENT = dict(mel=FAKE, tokens=FAKE, targets=FAKE, text_len=FAKE, loss_out=FAKE, B=B, S=S, span_forward=1, loss_scale=1.0, inv_accum=1.0)


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    from olmoasr_amd import _native
    if not os.path.isfile(_native.LIB_PATH):
        g.build()
    return _native


@pytest.fixture(scope="module")
def ctx(native):
    from oracle import model_oracle as mo
    lib = native.lib()
    dims = mo.VARIANTS["tiny"]
    cd = native.Dims(*[getattr(dims, f[0]) for f in native.Dims._fields_])
    c = lib.oasr_create_ex2(ctypes.byref(cd), dims.n_vocab + 1, 0)
    assert c, lib.oasr_last_error()
    fake = ctypes.c_void_p(FAKE)
    assert lib.oasr_bind(c, fake, fake, None, None, fake) == 0
    assert lib.oasr_bind_shadow(c, fake) == 0
    yield c
    lib.oasr_destroy(c)


@pytest.fixture(scope="module")
def tt():
    spec = importlib.util.spec_from_file_location("tt_cli_reg", os.path.join(ROOT, "scripts", "training", "train_timestamps.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_the_struct_grows_at_its_end_under_abi_216(native):
    lib = native.lib()
    assert lib.oasr_version() == 216 == native.ABI_VERSION
    assert lib.oasr_sizeof_train_step_args() == ctypes.sizeof(native.TrainStepArgs)
    names = [f[0] for f in native.TrainStepArgs._fields_]
    assert names[-4:] == ["label_smoothing", "z_loss", "loss_parts_out", "loss_parts_rows"]
    assert names[-6:-4] == ["loss_scale", "inv_accum"]  # what was the end of the struct stays where it was
    assert native.TrainStepArgs.label_smoothing.offset == native.TrainStepArgs.inv_accum.offset + 4
    z = native.TrainStepArgs()
    assert z.label_smoothing == 0.0 and z.z_loss == 0.0 and not z.loss_parts_out and not z.loss_parts_rows  # all-zero = off
    assert hasattr(lib, "oasr_cross_entropy_ex") and "oasr_cross_entropy_ex" in native.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "oasr.h")).read()
    assert "oasr_cross_entropy_ex(" in hdr and "float label_smoothing;" in hdr and "float* loss_parts_rows;" in hdr


def _step(native, c, ws_bytes=1 << 40, **fields):
    lib = native.lib()
    args = native.TrainStepArgs(**{**PRESENT, **fields})
    rc = lib.oasr_train_step(c, ctypes.byref(args), ctypes.c_void_p(FAKE), ws_bytes, None)
    return rc, lib.oasr_last_error() or b""


REFUSED = [  # (id, fields, the field the message names)
    ("eps_one", dict(label_smoothing=1.0), b"label_smoothing"),
    ("eps_negative", dict(label_smoothing=-0.1), b"label_smoothing"),
    ("eps_nan", dict(label_smoothing=math.nan), b"label_smoothing"),
    ("eps_inf", dict(label_smoothing=math.inf), b"label_smoothing"),
    ("z_negative", dict(z_loss=-1.0), b"z_loss"),
    ("z_nan", dict(z_loss=math.nan), b"z_loss"),
    ("z_inf", dict(z_loss=math.inf), b"z_loss"),
    ("parts_without_row_scratch", dict(label_smoothing=0.1, loss_parts_out=FAKE), b"loss_parts_rows"),
]


@pytest.mark.parametrize("fields,word", [r[1:] for r in REFUSED], ids=[r[0] for r in REFUSED])
def test_refusals_name_the_field_and_touch_nothing(native, ctx, fields, word):
    """Every pointer is a fake address: a check that came after a launch or a dereference would fault instead of returning."""
    rc, msg = _step(native, ctx, **fields)
    assert rc == EINVAL and word in msg, (rc, msg)
    # ... and before the workspace check: the value is named even when the workspace is also too small
    rc, msg = _step(native, ctx, ws_bytes=0, **fields)
    assert rc == EINVAL and word in msg, (rc, msg)


def test_good_values_pass_the_value_checks(native, ctx):
    """In-range values reach the next refusal (the workspace size), so the checks above refuse the values and nothing else."""
    for fields in (dict(label_smoothing=0.1, z_loss=1e-4), dict(label_smoothing=0.999, z_loss=10.0),
                   dict(z_loss=1e-4, loss_parts_out=FAKE, loss_parts_rows=FAKE), dict(loss_parts_rows=FAKE)):
        rc, msg = _step(native, ctx, ws_bytes=0, **fields)
        assert rc == EINVAL and b"workspace too small" in msg, (fields, rc, msg)


def test_cross_entropy_ex_refuses_bad_values_before_any_launch(native):
    lib = native.lib()
    fake = ctypes.c_void_p(FAKE)
    for eps, z, word in ((1.0, 0.0, b"label_smoothing"), (-0.1, 0.0, b"label_smoothing"), (math.nan, 0.0, b"label_smoothing"),
                         (0.0, -1.0, b"z_loss"), (0.0, math.nan, b"z_loss")):
        rc = lib.oasr_cross_entropy_ex(fake, 1024, 1000, fake, 4, 999, 1.0, fake, fake, fake, 1, eps, z, None, None)
        assert rc == EINVAL and word in lib.oasr_last_error(), (eps, z, lib.oasr_last_error())


def test_python_value_errors():
    from olmoasr_amd import ops
    from olmoasr_amd.model import OLMoASR
    bad = [dict(label_smoothing=1.0), dict(label_smoothing=-0.1), dict(label_smoothing=float("nan")), dict(z_loss=-1.0),
           dict(z_loss=float("inf")), dict(z_loss=float("nan"))]
    for kw in bad:
        name = next(iter(kw))
        with pytest.raises(ValueError, match=name):  # refused before any argument is looked at
            OLMoASR.loss_and_backward(None, None, None, None, None, **kw)
        with pytest.raises(ValueError, match=name):
            ops.cross_entropy_(None, 1000, None, 999, **kw)
    for parts in (torch.zeros(3), torch.zeros(2, dtype=torch.float64), torch.zeros(2, 1), torch.zeros(4)[::2], [0.0, 0.0]):
        with pytest.raises(ValueError, match="loss_parts_out"):
            OLMoASR.loss_and_backward(None, None, None, None, None, label_smoothing=0.1, loss_parts_out=parts)
    assert ops.check_loss_regularisers(0, 0, "t") == (0.0, 0.0) and ops.check_loss_regularisers(0.1, 1e-4, "t") == (0.1, 1e-4)


def test_cli_flags(tt):
    d = tt.parse_args([])
    assert d.label_smoothing == 0.0 and d.z_loss == 0.0 and isinstance(d.label_smoothing, float) and isinstance(d.z_loss, float)
    a = tt.parse_args(["--label_smoothing=0.1", "--z_loss", "1e-4"])
    assert a.label_smoothing == 0.1 and a.z_loss == 1e-4
    assert tt.parse_args(["--z_loss=0"]).z_loss == 0.0
    # the script's own options, not the reference's flag list
    assert "label_smoothing" in tt.NATIVE_FLAGS and "z_loss" in tt.NATIVE_FLAGS
    assert "label_smoothing" not in tt.REFERENCE_FLAGS and "z_loss" not in tt.REFERENCE_FLAGS
    for argv, word in ((["--label_smoothing=1.0"], "--label_smoothing"), (["--label_smoothing=-0.1"], "--label_smoothing"),
                       (["--label_smoothing=nan"], "--label_smoothing"), (["--label_smoothing=lots"], "--label_smoothing"),
                       (["--label_smoothing=True"], "--label_smoothing"), (["--z_loss=-1"], "--z_loss"), (["--z_loss=inf"], "--z_loss"),
                       (["--z_loss=None"], "--z_loss")):
        with pytest.raises(SystemExit, match=word):
            tt.parse_args(argv)
