"""CPU half of the device-resident beam search: the library's host twin (oasr_beam_update_host: csrc/beam_core.h, the text the device kernel
includes) against the restatement of decoding.py's BeamSearchDecoder.update in tests/beam_cases.py -- every case, every step, every output
with ``==``, the double scores included --, the binding's sizeof / ABI check, the argument checks, and the host twin of the cache reorder
against ``index_select``."""
import ctypes as C
import os

import pytest
import torch

import beam_cases as bc


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    from olmoasr_amd import _native
    if not os.path.isfile(_native.LIB_PATH):
        g.build()
    _native.lib()
    from olmoasr_amd import ops
    return ops


def test_the_restatement_shows_what_each_planted_case_is_about():
    for case in bc.planted_cases():
        snaps = bc.run_ref(case)
        assert case["expect"](snaps), case["name"]
    # patience: C = 2 < B = 4 fills and completes; C = 2 B holds more finished sequences than there are beams
    half = bc.run_ref(bc.patience_cases()[1])
    assert [s["completed"] for s in half].index(True) % 8 != 7 and half[-1] == half[-2] and [len(p) for p in half[-1]["pool"]] == [2]
    double = bc.run_ref(bc.patience_cases()[2])
    assert max(len(p) for p in double[-1]["pool"]) > 3
    # the random runs fill pools, and none of them is short
    runs = [bc.run_ref(c) for c in bc.random_cases()]
    assert len(runs) == 12 and all(len(r) == 12 for r in runs)
    assert not any(any(s["short"]) for r in runs for s in r)
    assert sum(any(r[-1]["pool"]) for r in runs) >= 9


@pytest.mark.parametrize("case", bc.all_cases(), ids=lambda c: c["name"])
def test_host_twin_equals_the_restatement(ops, case):
    bc.check_case(ops, case, "cpu", ops.beam_update_host)


def test_sizeof_and_abi_version(ops):
    from olmoasr_amd import _native as N
    lib = N.lib()
    assert lib.oasr_version() == N.ABI_VERSION == 216
    assert lib.oasr_sizeof_beam_args() == C.sizeof(N.BeamArgs) == 136
    assert ("oasr_sizeof_beam_args", N.BeamArgs) in N.STRUCT_SIZES
    for name in ("oasr_beam_update", "oasr_beam_update_host", "oasr_decode_reorder", "oasr_decode_reorder_host"):
        assert name in N.EXPORTS


def test_bad_arguments_raise_before_anything_runs(ops):
    from olmoasr_amd import _native as N
    with pytest.raises(ValueError):
        ops.beam_state(1, 16, 16, 24, bc.INIT, "cpu")                         # B = 16
    with pytest.raises(ValueError):
        ops.beam_state(1, 0, 1, 24, bc.INIT, "cpu")
    with pytest.raises(ValueError):
        ops.beam_state(1, 2, 0, 24, bc.INIT, "cpu")                           # an empty pool
    st = ops.beam_state(2, 3, 3, 24, bc.INIT, "cpu", fill=bc.FILL, guard=1)
    before = {k: v.clone() for k, v in st.backing.items()}
    lp, tok = torch.zeros(6, 4), torch.zeros(6, 4, dtype=torch.int64)
    for bad_lp, bad_tok in ((lp, tok[:, :3].contiguous()), (lp, tok[:5]), (lp[:, :3].contiguous(), tok), (lp, tok.int()), (lp.double(), tok),
                            (lp, tok.t().contiguous().t())):
        with pytest.raises(ValueError):
            ops.beam_update_host(st, bad_lp, bad_tok, eot=bc.EOT)
    with pytest.raises(ValueError):
        ops.beam_update(st, lp, tok, eot=bc.EOT)                              # a CPU state on the device entry
    assert st.len == 2 and st.cur == 0 and all(torch.equal(v, before[k]) for k, v in st.backing.items())
    # the C side refuses what the wrapper would (the native refusals are the stand-alone host check's: make beam-host-check)
    a = N.BeamArgs()
    with pytest.raises(N.NativeError, match="oasr_beam_update_host"):
        N.call("oasr_beam_update_host", C.byref(a))
    # full rows: no further token fits
    full = ops.beam_state(1, 1, 1, 3, bc.INIT, "cpu")
    ops.beam_update_host(full, torch.zeros(1, 2), torch.tensor([[1, 2]]), eot=bc.EOT)
    with pytest.raises(ValueError):
        ops.beam_update_host(full, torch.zeros(1, 2), torch.tensor([[1, 2]]), eot=bc.EOT)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_host_reorder_equals_index_select_and_refuses_foreign_sources(ops, dtype):
    L, B, n_ctx, d, group = 2, 6, 7, 8, 3
    g = torch.Generator().manual_seed(4)
    rows = torch.randn(L, B, n_ctx, 3 * d, generator=g).to(dtype)
    sources = [0, 0, 1, 5, 3, 3]
    for pos in (0, 1, 5, 7):
        want = rows.clone()
        want[:, :, :pos, d:] = rows[:, sources][:, :, :pos, d:]
        got = ops.kv_reorder_host(rows.clone(), pos, group, sources)
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), pos
    same = ops.kv_reorder_host(rows.clone(), 5, group, list(range(B)))
    assert torch.equal(same.view(torch.uint8), rows.view(torch.uint8))
    held = rows.clone()
    for bad in ([0, 0, 3, 5, 3, 3], [0, 0, 1, 2, 3, 3], [0, 0, 1, 5, 3, 6], [-1, 0, 1, 5, 3, 3]):  # a source outside its window
        with pytest.raises(ValueError):
            ops.kv_reorder_host(held, 5, group, bad)
    with pytest.raises(ValueError):
        ops.kv_reorder_host(held, 5, 4, sources)                              # a group that does not divide B
    with pytest.raises(ValueError):
        ops.kv_reorder_host(held, 8, group, sources)                          # pos past n_ctx
    assert torch.equal(held.view(torch.uint8), rows.view(torch.uint8))


def test_options_default_and_validation():
    from olmoasr_amd.decoding import DecodingOptions
    assert DecodingOptions().beam_backend == "host"
    assert DecodingOptions(beam_size=3, beam_backend="native").beam_backend == "native"
