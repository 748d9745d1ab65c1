"""GPU half of the token error counts (csrc/editdist.hip): ``ops.edit_counts`` on the case sets of tests/edit_cases.py, compared with
``torch.equal`` against the library's host twin (which tests/test_edit_distance_cpu.py holds against the rule written out independently).
Every output lies in a sentinel-filled buffer with one guard row past B."""
import pytest
import torch

from edit_cases import KNOWN, binary_pairs, length_pairs, pack, random_pairs

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -12345


def run_guarded(ops, packed):
    """edit_counts into rows [0, B) of a sentinel-filled [B + 1, 4] buffer: (the B rows, whether the guard row kept the sentinel)."""
    hyp, hyp_len, ref, ref_len = (t.to(DEV) for t in packed)
    B = hyp.shape[0]
    buf = torch.full((B + 1, 4), SENTINEL, dtype=torch.int32, device=DEV)
    got = ops.edit_counts(hyp, hyp_len, ref, ref_len, out=buf[:B])
    assert got.data_ptr() == buf.data_ptr()
    host = buf.cpu()
    return host[:B], bool((host[B] == SENTINEL).all())


CASE_SETS = {
    "known": lambda: [(h, r) for h, r, _ in KNOWN],
    "binary": binary_pairs,                                   # B = 3969
    "random": random_pairs,                                   # B = 300
    "edge_lengths": length_pairs,                             # 0 .. 1023 on either side, 1023 x 1 and 1 x 1023 among them
    "wave_and_workgroup_boundaries": lambda: length_pairs((511, 512, 513, 1), seed=7),
    "single_pair": lambda: random_pairs(1, seed=11),          # B = 1
}


@pytest.mark.parametrize("name", list(CASE_SETS))
def test_edit_counts_equal_the_host_twin(name):
    from olmoasr_amd import ops
    pairs = CASE_SETS[name]()
    packed = pack(pairs)
    want = ops.edit_counts_host(*packed)
    got, guard_ok = run_guarded(ops, packed)
    assert guard_ok, "the guard row past B was written"
    assert torch.equal(got, want), (name, (got != want).any(dim=1).nonzero().flatten().tolist()[:8])
    assert int(got.min()) >= 0
    if name == "known":
        assert got.tolist() == [list(k) for _, _, k in KNOWN]


def test_row_strides_trailing_tokens_and_int64():
    from olmoasr_amd import ops
    pairs = random_pairs(64, seed=5) + length_pairs((0, 130), seed=3)
    hyp, hyp_len, ref, ref_len = pack(pairs, extra=3)  # tokens past the lengths inside the rows
    want = ops.edit_counts_host(hyp, hyp_len, ref, ref_len)
    B = len(pairs)
    wide_h = torch.full((B, hyp.shape[1] + 5), 9, dtype=torch.int32)
    wide_r = torch.full((B, ref.shape[1] + 11), 9, dtype=torch.int32)
    wide_h[:, :hyp.shape[1]], wide_r[:, :ref.shape[1]] = hyp, ref
    view_h, view_r = wide_h.to(DEV)[:, :hyp.shape[1]], wide_r.to(DEV)[:, :ref.shape[1]]
    assert not view_h.is_contiguous()
    assert torch.equal(ops.edit_counts(view_h, hyp_len.to(DEV), view_r, ref_len.to(DEV)).cpu(), want)
    assert torch.equal(ops.edit_counts(view_h.long(), hyp_len.to(DEV).long(), view_r.long(), ref_len.to(DEV).long()).cpu(), want)


def test_two_launches_on_one_stream_do_not_share_state():
    """Different inputs into two outputs, back to back on the same stream, then the first inputs again."""
    from olmoasr_amd import ops
    a, b = pack(random_pairs(130, seed=21)), pack(length_pairs((3, 200, 449), seed=22))
    want_a, want_b = ops.edit_counts_host(*a), ops.edit_counts_host(*b)
    da, db = [t.to(DEV) for t in a], [t.to(DEV) for t in b]
    out_a = torch.full((want_a.shape[0], 4), SENTINEL, dtype=torch.int32, device=DEV)
    out_b = torch.full((want_b.shape[0], 4), SENTINEL, dtype=torch.int32, device=DEV)
    ops.edit_counts(*da, out=out_a)
    ops.edit_counts(*db, out=out_b)
    again = ops.edit_counts(*da)
    torch.cuda.synchronize()
    assert torch.equal(out_a.cpu(), want_a) and torch.equal(out_b.cpu(), want_b) and torch.equal(again.cpu(), want_a)


def test_lengths_outside_the_contract_mark_their_row_and_bad_shapes_raise():
    """The lengths live on the device, so the launch cannot refuse them: such a pair's row reads (-1, -1, -1, -1), its neighbours are right."""
    from olmoasr_amd import ops
    hyp, hyp_len, ref, ref_len = pack(random_pairs(6, seed=8))
    want = ops.edit_counts_host(hyp, hyp_len, ref, ref_len)
    bad_h, bad_r = hyp_len.clone(), ref_len.clone()
    bad_h[1], bad_r[3], bad_h[4] = hyp.shape[1] + 1, -1, 1024
    got = ops.edit_counts(hyp.to(DEV), bad_h.to(DEV), ref.to(DEV), bad_r.to(DEV)).cpu()
    for b in range(6):
        assert got[b].tolist() == ([-1] * 4 if b in (1, 3, 4) else want[b].tolist()), b
    d = [t.to(DEV) for t in (hyp, hyp_len, ref, ref_len)]
    with pytest.raises(ValueError):
        ops.edit_counts(d[0], d[1], d[2][:5], d[3])          # B mismatch
    with pytest.raises(ValueError):
        ops.edit_counts(d[0], d[1][:5], d[2], d[3])
    with pytest.raises(ValueError):
        ops.edit_counts(hyp, d[1], d[2], d[3])               # a CPU operand
    with pytest.raises(ValueError):
        ops.edit_counts(d[0].float(), d[1], d[2], d[3])
    with pytest.raises(ValueError):
        ops.edit_counts(*d, out=torch.empty(6, 4, dtype=torch.int64, device=DEV))
