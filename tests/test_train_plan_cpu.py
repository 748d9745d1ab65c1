"""The training engine's host decisions without a GPU: how Runner::wgrad splits a weight gradient and which sections of a block's backward
run under a trainability mask are plain C++ (csrc/train_plan_host.cpp), exported on plain integers (include/oasr_testing.h:
oasr_train_wgrad_plan_debug, oasr_train_block_needs_debug).  Nothing is launched here.

 1. the weight-gradient plan at recorded answers: the production shapes, both ping-pong thresholds, the view case, the tiny model's shapes;
 2. the block-needs function over every combination of its inputs against the predicates written out again here.
"""
import ctypes
import itertools
import os

import pytest


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    from olmoasr_amd import _native
    if not os.path.isfile(_native.LIB_PATH):
        g.build()
    return _native


def wgrad_plan(native, tokens, N, K, view=0):
    split, pp = ctypes.c_int(-7), ctypes.c_int(-7)
    native.check(native.lib().oasr_train_wgrad_plan_debug(tokens, N, K, view, ctypes.byref(split), ctypes.byref(pp)), "oasr_train_wgrad_plan_debug")
    return split.value, pp.value


# (tokens M, N, K, view) -> (split_k, atomic_on_pp), as the rule answered before it moved out of the runner
WGRAD_TABLE = [
    ((192000, 1024, 1024, 0), (16, 1)), ((192000, 4096, 1024, 0), (8, 1)), ((192000, 1024, 4096, 0), (4, 1)), ((192000, 3072, 1024, 0), (8, 0)),
    ((192000, 2048, 1024, 0), (8, 1)), ((57344, 1024, 1024, 0), (16, 0)), ((57344, 4096, 1024, 0), (4, 1)), ((57344, 1024, 4096, 0), (4, 1)),
    ((57344, 3072, 1024, 0), (8, 0)), ((57344, 51864, 1024, 0), (1, 0)), ((57344, 1, 1024, 0), (24, 0)), ((18688, 1024, 1024, 0), (16, 0)),
    ((18688, 4096, 1024, 0), (4, 0)), ((18688, 1024, 4096, 0), (4, 0)), ((18688, 3072, 1024, 0), (8, 0)), ((150000, 1024, 1024, 0), (16, 1)),
    ((149999, 1024, 1024, 0), (24, 0)), ((40000, 4096, 1024, 0), (4, 1)), ((39999, 4096, 1024, 0), (4, 0)), ((192000, 1024, 4096, 1), (16, 0)),
    ((384000, 1024, 256, 0), (32, 0)), ((192000, 1024, 3072, 0), (8, 0)), ((3000, 384, 384, 0), (4, 0)), ((3000, 384, 1152, 0), (4, 0)),
    ((6000, 384, 256, 0), (8, 0)), ((896, 384, 384, 0), (1, 0)), ((896, 1536, 384, 0), (1, 0)), ((896, 384, 1536, 0), (1, 0)),
    ((896, 1152, 384, 0), (1, 0)), ((64, 384, 384, 0), (1, 0)), ((512, 384, 384, 0), (1, 0)), ((128, 8, 384, 0), (1, 0)),
]


def test_weight_gradient_plan_answers_as_before(native):
    for (M, N, K, view), want in WGRAD_TABLE:
        split, pp = wgrad_plan(native, M, N, K, view)
        assert (split, pp) == want, (M, N, K, view)
        assert split >= 1  # (launch_gemm's condition)
        assert pp in (0, 1) and (not pp or (N % 256 == 0 and K % 256 == 0 and not view)), (M, N, K, view)


def test_weight_gradient_plan_is_legal_off_the_table(native):
    """split_k >= 1, and the ping-pong opt-in only on whole 256 x 256 tiles of a plain operand, around the table's shapes too"""
    for M, N, K, view in itertools.product((1, 63, 64, 513, 18688, 39999, 40000, 149999, 150000, 192000), (1, 8, 255, 256, 1024, 2048, 4096, 51864),
                                           (8, 256, 264, 1024, 4096), (0, 1)):
        split, pp = wgrad_plan(native, M, N, K, view)
        assert split in (1, 2, 4, 8, 16, 24, 32), (M, N, K, view, split)
        assert pp in (0, 1) and (not pp or (N % 256 == 0 and K % 256 == 0 and not view)), (M, N, K, view)
    lib = native.lib()
    split, pp = ctypes.c_int(-7), ctypes.c_int(-7)
    for bad in ((0, 8, 8), (8, 0, 8), (8, 8, 0)):
        assert lib.oasr_train_wgrad_plan_debug(*bad, 0, ctypes.byref(split), ctypes.byref(pp)) != 0
    assert (split.value, pp.value) == (-7, -7)


ASK = ("need_dx_in", "need_xa", "cross", "sa", "ca", "mlp", "cln", "attn_ln", "kv")  # bit order of oasr_train_block_needs_debug's argument
MLP, CA, SA, CA_KV, CA_TAIL, SA_TAIL = 1, 2, 4, 8, 16, 32                            # ... and of its answer


def needs(native, **asked):
    assert set(asked) <= set(ASK)
    got = native.lib().oasr_train_block_needs_debug(sum(1 << i for i, k in enumerate(ASK) if asked.get(k)))
    assert got >= 0
    return got


def expected_needs(need_dx_in, need_xa, cross, sa, ca, mlp, cln, attn_ln, kv):
    """The predicates of the block's backward as they stood inline: what each section needs, and how far the pass gets before the first
    `nothing further is needed`."""
    sa_need = need_dx_in or sa
    ca_need = cross and (sa_need or need_xa or ca)
    mlp_need = (ca_need if cross else sa_need) or mlp
    got = 0
    if not mlp_need:
        return got
    got |= MLP
    if cross:
        if not ca_need:
            return got
        got |= CA
        if kv or need_xa:
            got |= CA_KV
        if not sa_need and not cln:
            return got
        got |= CA_TAIL
    if not sa_need:
        return got
    got |= SA
    if not need_dx_in and not attn_ln:
        return got
    return got | SA_TAIL


def test_block_needs_truth_table(native):
    rows = 0
    for bits in itertools.product((False, True), repeat=len(ASK)):
        asked = dict(zip(ASK, bits))
        got = needs(native, **asked)
        assert got == expected_needs(**asked), asked
        if not asked["cross"]:
            assert not got & (CA | CA_KV | CA_TAIL), asked  # a block without a cross-attention never reports one
        # a section never runs without the ones above it
        assert not got & SA or got & MLP, asked
        assert not got & CA or got & MLP, asked
        assert not (got & SA and asked["cross"]) or got & CA, asked
        rows += 1
    assert rows == 512
    assert native.lib().oasr_train_block_needs_debug(-1) == -1 and native.lib().oasr_train_block_needs_debug(512) == -1


def test_block_needs_properties(native):
    everything = {k: True for k in ASK}
    assert needs(native, **everything) == MLP | CA | SA | CA_KV | CA_TAIL | SA_TAIL
    assert needs(native, **dict(everything, cross=False)) == MLP | SA | SA_TAIL
    # nothing needed: nothing past the mlp.2 weight gradient, with or without a cross-attention
    assert needs(native) == 0 and needs(native, cross=True) == 0
    # d(xa) alone: the MLP and cross sections of a cross block (to reach the key|value side), not its self section, not the LayerNorm tail
    assert needs(native, need_xa=True, cross=True) == MLP | CA | CA_KV
    assert needs(native, need_xa=True) == 0  # (an encoder block is never asked for d(xa); it would change nothing)
    # the input gradient alone runs everything on the data path, but the key|value side only for its own sake
    assert needs(native, need_dx_in=True, cross=True) == MLP | CA | SA | CA_TAIL | SA_TAIL
    assert needs(native, need_dx_in=True) == MLP | SA | SA_TAIL
    # a LayerNorm's own gradient keeps the tail that computes it
    assert needs(native, cross=True, ca=True, cln=True) == MLP | CA | CA_TAIL
    assert needs(native, cross=True, ca=True, kv=True) == MLP | CA | CA_KV
    assert needs(native, sa=True, attn_ln=True) == MLP | SA | SA_TAIL
    assert needs(native, sa=True) == MLP | SA
    assert needs(native, mlp=True, cross=True) == MLP
