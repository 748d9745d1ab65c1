"""The Python binding's own machinery, without a GPU: the workspace slot that knows what it holds (model._Slot), the one native-call
path (_native.call) through a host entry, and the struct-size table lib() holds a library to."""
import ctypes as C
import os
import re

import pytest
import torch


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    from olmoasr_amd import _native
    if not os.path.isfile(_native.LIB_PATH):
        g.build()
    _native.lib()
    return _native


GONE = "activations of this forward are gone"


def test_slot_take_keeps_the_storage_and_voids_older_leases():
    from olmoasr_amd.model import _Slot
    s = _Slot()
    assert s.buf is None
    a = s.take(64, "cpu")
    lease_a = s.gen
    assert a.dtype == torch.uint8 and a.numel() == 64 and a.device.type == "cpu" and s.buf is a
    b = s.take(16, "cpu")  # fits: the same storage, not shrunk
    lease_b = s.gen
    assert b is a and b.numel() == 64 and lease_b != lease_a
    with pytest.raises(RuntimeError, match=r"^model\.encoder backward: .*" + GONE):
        s.redeem(lease_a, "model.encoder")  # every take voids the lease before it
    assert s.gen == lease_b  # a refused redeem consumes nothing
    assert s.redeem(lease_b, "model.encoder") is a  # the newest lease: once
    with pytest.raises(RuntimeError, match=GONE):
        s.redeem(lease_b, "model.encoder")
    c = s.take(4096, "cpu")  # does not fit: grown
    assert c.numel() >= 4096 and s.buf is c
    assert s.take(64, "cpu") is c and c.numel() >= 4096  # and never shrunk again
    leases = set()
    for _ in range(3):
        s.take(1, "cpu")
        leases.add(s.gen)
    assert len(leases) == 3


def test_slot_drop_voids_the_lease():
    from olmoasr_amd.model import _Slot
    s = _Slot()
    s.take(32, "cpu")
    lease = s.gen
    s.drop()
    assert s.buf is None
    with pytest.raises(RuntimeError, match=r"^OLMoASR\.forward backward: .*" + GONE + r".*forward and backward in pairs"):
        s.redeem(lease, "OLMoASR.forward")
    s.take(32, "cpu")  # a new buffer under the old lease's number would be the hole again: the lease stays void
    with pytest.raises(RuntimeError, match=GONE):
        s.redeem(lease, "OLMoASR.forward")
    s.drop()
    with pytest.raises(RuntimeError, match=GONE):
        s.redeem(s.gen, "OLMoASR.forward")  # nothing to redeem from an empty slot, whatever the number


def test_call_passes_tensors_none_and_ctypes_values(native):
    N = native
    H = C.c_int()
    N.call("oasr_speed_table", 3, 2, None, C.byref(H))  # None arrives as NULL: the size query of ops.speed_table
    assert H.value > 0
    T = torch.zeros(2, 2 * H.value, dtype=torch.int32)
    N.call("oasr_speed_table", 3, 2, T, C.byref(H))  # a CPU tensor arrives as its address and names no device
    assert T.sum(1).tolist() == [32768, 32768]
    from olmoasr_amd import ops
    assert torch.equal(ops.speed_table(3, 2)[0], T)


def test_call_raises_under_the_entrys_name_with_the_librarys_text(native):
    N = native
    H = C.c_int()
    with pytest.raises(N.NativeError) as e:
        N.call("oasr_speed_table", 0, 2, None, C.byref(H))
    text = N.lib().oasr_last_error().decode()
    assert text.startswith("oasr_speed_table:") and "P = 0" in text
    assert str(e.value).startswith("oasr_speed_table failed (rc=") and text in str(e.value)
    with pytest.raises(N.NativeError, match="oasr_speed_table failed .*null H"):
        N.call("oasr_speed_table", 3, 2, None, None)  # None arrives as NULL here too
    with pytest.raises(N.NativeError, match="oasr_edit_counts_host failed"):
        N.call("oasr_edit_counts_host", None)
    with pytest.raises(N.NativeError, match="oasr_speed_table: a stream was asked for"):
        N.call("oasr_speed_table", 3, 2, None, N.STREAM)  # no device to take a stream from: refused before the entry runs


def test_struct_size_table_covers_what_the_library_exports(native):
    N = native
    lib = N.lib()
    blob = open(N.LIB_PATH, "rb").read()
    exported = {n.decode() for n in set(re.findall(rb"oasr_sizeof_[a-z0-9_]+", blob))}
    exported = {n for n in exported if hasattr(lib, n)}  # (a name inside a message is no symbol)
    rows = [entry for entry, _ in N.STRUCT_SIZES]
    assert len(exported) >= 7 and sorted(rows) == sorted(exported) and len(set(rows)) == len(rows)
    assert rows[0] == "oasr_sizeof_attn_args"  # the one lib() checks before it declares anything
    for entry, struct in N.STRUCT_SIZES:
        assert entry in N.EXPORTS and issubclass(struct, C.Structure)
        assert getattr(lib, entry)() == C.sizeof(struct), entry


def test_a_wrong_struct_size_is_refused_and_nothing_is_published(native, monkeypatch):
    N = native

    class Grown(C.Structure):
        _fields_ = N.TrainStepArgs._fields_ + [("one_more", C.c_void_p)]
    monkeypatch.setattr(N, "STRUCT_SIZES", N.STRUCT_SIZES[:-1] + [("oasr_sizeof_train_step_args", Grown)])
    monkeypatch.setattr(N, "_lib", None)
    for _ in range(2):
        with pytest.raises(N.NativeError, match=r"oasr_sizeof_train_step_args answers \d+ bytes, this binding's Grown has \d+ -- rebuild"):
            N.lib()
        assert N._lib is None
