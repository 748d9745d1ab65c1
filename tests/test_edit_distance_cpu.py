"""CPU half of the token error counts: the library's host twin (oasr_edit_counts_host: csrc/editdist_core.h, the text the device kernel
includes) against the rule written out again in tests/edit_cases.py, the invariants of every result, the argument checks, the sequence
rules of olmoasr_amd/metrics.py against gen_pred's list rules restated here, and the training script's flag."""
import importlib.util
import os

import pytest
import torch

from edit_cases import EDGE_LENGTHS, KNOWN, binary_pairs, length_pairs, pack, random_pairs, rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOT, IGNORE = 50256, 51864


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    from olmoasr_amd import _native
    if not os.path.isfile(_native.LIB_PATH):
        g.build()
    _native.lib()
    from olmoasr_amd import ops
    return ops


@pytest.fixture(scope="module")
def tt():
    spec = importlib.util.spec_from_file_location("tt_edit_cpu", os.path.join(ROOT, "scripts", "training", "train_timestamps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def check_set(ops, tt, pairs, **pack_args):
    """The twin on one batch against ``rule`` pair by pair, plus the invariants and the training script's own Levenshtein distance."""
    hyp, hyp_len, ref, ref_len = pack(pairs, **pack_args)
    got = ops.edit_counts_host(hyp, hyp_len, ref, ref_len)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(pairs), 4)
    for (h, r), row in zip(pairs, got.tolist()):
        s, d, i, hits = row
        assert tuple(row) == rule(h, r), (h, r, row)
        assert min(row) >= 0 and s + d + hits == len(r) and s + i + hits == len(h), (h, r, row)
        assert s + d + i == tt.token_error_counts([h], [r])[0], (h, r, row)


def test_known_answers(ops, tt):
    pairs = [(h, r) for h, r, _ in KNOWN]
    hyp, hyp_len, ref, ref_len = pack(pairs)
    assert ops.edit_counts_host(hyp, hyp_len, ref, ref_len).tolist() == [list(k) for _, _, k in KNOWN]
    assert [rule(h, r) for h, r in pairs] == [k for _, _, k in KNOWN]  # (the restatement itself)
    check_set(ops, tt, pairs)


def test_every_binary_pair_up_to_length_5(ops, tt):
    pairs = binary_pairs()
    assert len(pairs) == 3969
    check_set(ops, tt, pairs)


def test_seeded_random_pairs(ops, tt):
    pairs = random_pairs()
    assert len(pairs) == 300 and max(len(h) for h, _ in pairs) == 40 and min(len(r) for _, r in pairs) == 0
    check_set(ops, tt, pairs)


def test_edge_lengths_on_either_side(ops, tt):
    pairs = length_pairs()
    assert {(len(h), len(r)) for h, r in pairs} >= {(1023, 1), (1, 1023), (1023, 1023), (0, 1023), (1023, 0), (64, 65), (448, 63)}
    assert len(pairs) == len(EDGE_LENGTHS) ** 2
    check_set(ops, tt, pairs)


def test_row_strides_and_trailing_tokens(ops, tt):
    pairs = random_pairs(40, seed=5)
    check_set(ops, tt, pairs, extra=3)  # tokens past the lengths inside the rows
    hyp, hyp_len, ref, ref_len = pack(pairs, extra=2)
    want = ops.edit_counts_host(hyp, hyp_len, ref, ref_len)
    wide_h, wide_r = torch.full((len(pairs), hyp.shape[1] + 5), 9, dtype=torch.int32), torch.full((len(pairs), ref.shape[1] + 11), 9, dtype=torch.int32)
    wide_h[:, :hyp.shape[1]], wide_r[:, :ref.shape[1]] = hyp, ref
    view_h, view_r = wide_h[:, :hyp.shape[1]], wide_r[:, :ref.shape[1]]
    assert not view_h.is_contiguous() and view_h.stride(0) == hyp.shape[1] + 5
    assert torch.equal(ops.edit_counts_host(view_h, hyp_len, view_r, ref_len), want)
    assert torch.equal(ops.edit_counts_host(view_h.long(), hyp_len.long(), view_r.long(), ref_len.long()), want)  # int64 ids and lengths: plumbing
    assert [tuple(r) for r in want.tolist()] == [rule(h, r) for h, r in pairs]


def test_bad_arguments_raise_before_anything_runs(ops):
    tok = torch.ones(2, 1024, dtype=torch.int32)
    one = torch.ones(2, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.edit_counts_host(tok, torch.tensor([1024, 1], dtype=torch.int32), tok, one)       # past 1023
    with pytest.raises(ValueError):
        ops.edit_counts_host(tok, one, tok, torch.tensor([1, 1024], dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.edit_counts_host(tok[:, :4], torch.tensor([5, 1], dtype=torch.int32), tok, one)   # past the row width
    with pytest.raises(ValueError):
        ops.edit_counts_host(tok, one, tok[:, :4], torch.tensor([1, 5], dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.edit_counts_host(tok, torch.tensor([-1, 1], dtype=torch.int32), tok, one)         # negative
    with pytest.raises(ValueError):
        ops.edit_counts_host(tok, one, tok[:1], one)                                          # B mismatch
    with pytest.raises(ValueError):
        ops.edit_counts_host(tok, one[:1], tok, one)
    with pytest.raises(ValueError):
        ops.edit_counts_host(tok.float(), one, tok, one)
    assert ops.edit_counts_host(tok[:, :1023], torch.tensor([1023, 0], dtype=torch.int32), tok[:, :1023], torch.tensor([1023, 1023], dtype=torch.int32)).tolist() == \
        [[0, 0, 0, 1023], [0, 1023, 0, 0]]


# ---- metrics.train_sequences against gen_pred's list rules (the argmax itself needs the GPU) ------------------------------------------
def gen_pred_lists(pred_rows, target_rows):
    preds, tgts = [], []
    for row in pred_rows:
        if -1 in row:
            row = row[:row.index(-1)]                     # positions the span step did not compute
        preds.append(row[:row.index(EOT) + 1] if EOT in row else row)
    for row in target_rows:
        row = [t for t in row if t != IGNORE]
        tgts.append((row[:row.index(EOT)] if EOT in row else row) + [EOT])
    return preds, tgts


SEQ_PRED = [[5, 6, 7, 8, 9, 10],              # no eot
            [EOT, 6, 7, 8, 9, 10],            # eot at position 0
            [5, 6, -1, EOT, -1, -1],          # -1 before the eot
            [5, 6, EOT, 7, -1, -1],           # eot before the -1
            [-1, -1, -1, -1, -1, -1],         # nothing computed
            [5, 6, 7, EOT, EOT, 3]]           # two eots
SEQ_TGT = [[IGNORE, 5, IGNORE, 6, EOT, IGNORE],   # interior ignore
           [5, 6, 7, 8, 9, 10],                   # no eot, nothing ignored
           [IGNORE] * 6,                          # everything ignored
           [EOT, 5, 6, IGNORE, IGNORE, IGNORE],   # eot first
           [5, IGNORE, IGNORE, EOT, 7, EOT],      # tokens after the first eot
           [IGNORE, IGNORE, IGNORE, IGNORE, IGNORE, 4]]


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_train_sequences_follow_gen_pred(dtype):
    from olmoasr_amd import metrics
    pred, tgt = torch.tensor(SEQ_PRED, dtype=dtype), torch.tensor(SEQ_TGT, dtype=torch.int64)
    hyp, hyp_len, ref, ref_len = metrics.train_sequences(pred, tgt)
    assert hyp.dtype == hyp_len.dtype == ref.dtype == ref_len.dtype == torch.int32
    assert tuple(hyp.shape) == (6, 6) and tuple(ref.shape) == (6, 7)
    preds, tgts = gen_pred_lists(SEQ_PRED, SEQ_TGT)
    assert [hyp[b, :hyp_len[b]].tolist() for b in range(6)] == preds
    assert [ref[b, :ref_len[b]].tolist() for b in range(6)] == tgts
    assert hyp_len.tolist() == [6, 1, 2, 3, 0, 4] and ref_len.tolist() == [3, 7, 1, 1, 2, 2]


def test_error_counter_equals_token_error_rate(ops, tt):
    from olmoasr_amd import metrics
    g = torch.Generator().manual_seed(3)
    counter = metrics.ErrorCounter("cpu")
    all_p, all_t = [], []
    for _ in range(3):  # three micro-batches accumulate
        pred = torch.randint(0, 6, (16, 24), generator=g)
        tgt = torch.randint(0, 6, (16, 24), generator=g)
        pred[pred == 5], tgt[tgt == 5] = EOT, EOT
        tgt[torch.rand(16, 24, generator=g) < 0.3] = IGNORE
        pred[torch.arange(16)[:, None] * 2 < torch.arange(24)[None, :] - 4] = -1  # rows computed to different lengths
        counter.add(pred, tgt)
        p, t = gen_pred_lists(pred.tolist(), tgt.tolist())
        all_p += p
        all_t += t
    s, d, i, h = counter.counts()
    assert metrics.ErrorCounter.fraction((s, d, i, h)) == tt.token_error_counts(all_p, all_t)  # integers: numerator and denominator
    assert s + d + h == sum(len(t) for t in all_t) and s + i + h == sum(len(p) for p in all_p)
    assert counter.rate() == tt.token_error_rate(all_p, all_t)
    counter.reset()
    assert counter.counts() == (0, 0, 0, 0) and counter.rate() == 0.0


def test_train_error_counts_flag(tt):
    assert tt.parse_args([]).train_error_counts == "host"
    assert tt.parse_args(["--train_error_counts=device"]).train_error_counts == "device"
    assert tt.parse_args(["--train_error_counts", "host"]).train_error_counts == "host"
    for bad in ("gpu", "True", "1", ""):
        with pytest.raises(SystemExit):
            tt.parse_args([f"--train_error_counts={bad}"])
    with pytest.raises(SystemExit):  # the predictions come from the span step
        tt.parse_args(["--train_error_counts=device", "--span_backward=False"])
