"""What of the teacher-forced score runs without a GPU: the ABI of the new entries, the host twin of the reduce on the planted reduce cases,
``metrics.ValidationTotals``, the validation flags of the training script, and the stand-alone host check under a host sanitizer."""
import ctypes as C
import importlib.util
import os
import shutil
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_cases as sc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "olmoasr_amd", "csrc")


@pytest.fixture(scope="module")
def tt():
    spec = importlib.util.spec_from_file_location("tt_score_cpu", os.path.join(ROOT, "scripts", "training", "train_timestamps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_abi_version_struct_size_and_null_args():
    from olmoasr_amd import _native as N
    lib = N.lib()
    assert lib.oasr_version() == N.ABI_VERSION == 216
    assert lib.oasr_sizeof_score_args() == C.sizeof(N.ScoreArgs) == 12 * 8 + 2 * 4
    assert ("oasr_sizeof_score_args", N.ScoreArgs) in N.STRUCT_SIZES
    assert lib.oasr_score(None, None, None, 0, None) != 0  # refused: nothing to dereference, nothing launched
    assert b"null" in lib.oasr_last_error()
    header = open(os.path.join(ROOT, "include", "oasr.h")).read()
    assert "#define OASR_ABI_VERSION 216" in header
    for entry in ("oasr_score", "oasr_score_rows", "oasr_score_reduce", "oasr_score_reduce_host", "oasr_sizeof_score_args"):
        assert entry + "(" in header and entry in N.EXPORTS


# ---- the host twin of the reduce --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", sc.REDUCE_S)
def test_reduce_host_on_the_planted_cases(S):
    from olmoasr_amd import ops
    case = sc.reduce_case(S)
    got = ops.score_reduce_host(case["row_nll"], case["pred"], case["targets"], case["span"], V=case["V"], ignore=case["ignore"])
    for name, g, w in zip(("nll_sum", "nll_max", "n_tok", "n_hit"), got, case["want"]):
        assert torch.equal(g, w), (name, g.tolist(), w.tolist())
    for b in (0, 4):  # span 0; a sample with no valid target
        assert int(got[2][b]) == 0 and float(got[0][b]) == 0.0 and float(got[1][b]) == 0.0
    if case["planted"]:
        assert float(got[0][1]) != float(case["row_nll"][1][(case["targets"][1] != case["ignore"]) & (case["targets"][1] >= 0)
                                                            & (case["targets"][1] < case["V"])].sum())  # a float32 sum rounds elsewhere
    # span=None: every row
    full = ops.score_reduce_host(case["row_nll"], case["pred"], case["targets"], V=case["V"], ignore=case["ignore"])
    assert torch.equal(full[2], sc.reduce_expect(case["row_nll"], case["pred"], case["targets"], torch.full((6,), S), case["V"], case["ignore"])[2])


def test_reduce_host_refusals():
    from olmoasr_amd import ops
    nll, pred, tgt = torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(ValueError):
        ops.score_reduce_host(nll, pred.long(), tgt, V=5)
    with pytest.raises(ValueError):
        ops.score_reduce_host(nll[:, :2], pred, tgt, V=5)
    with pytest.raises(ValueError):
        ops.score_reduce_host(nll, pred, tgt, torch.zeros(3, dtype=torch.int32), V=5)
    with pytest.raises(ValueError):
        ops.score_reduce_host(nll, pred, tgt, V=0)
    with pytest.raises(ValueError):
        ops.score_rows(torch.zeros(6, 8), 5, tgt)  # a CPU tensor: there is no CPU fallback of the row kernel


# ---- ValidationTotals ---------------------------------------------------------------------------------------------------------------------------
class _Score:
    def __init__(self, nll_sum, n_tok, n_hit):
        self.nll_sum = torch.tensor(nll_sum, dtype=torch.float32)
        self.n_tok = torch.tensor(n_tok, dtype=torch.int32)
        self.n_hit = torch.tensor(n_hit, dtype=torch.int32)


def test_validation_totals_are_token_weighted():
    from olmoasr_amd.metrics import ValidationTotals
    a, b = _Score([10.0, 2.0], [10, 1], [5, 1]), _Score([300.0], [100], [20])
    t = ValidationTotals().add(a).add(b)
    rec = t.record()
    assert rec == {"val_loss": 312.0 / 111, "val_token_acc": 26 / 111, "val_n_tokens": 111, "val_n_samples": 3}
    mean_of_means = ((12.0 / 11) + 3.0) / 2
    assert abs(rec["val_loss"] - mean_of_means) > 0.5  # not a mean of batch means
    assert t.nll.dtype == torch.float64 and t.counts.dtype == torch.int64
    # merge = having added everything to one instance; any batching of the same samples gives the same record
    m = ValidationTotals().add(a).merge(ValidationTotals().add(b))
    assert m.record() == rec
    split = ValidationTotals().add(_Score([10.0], [10], [5])).add(_Score([2.0, 300.0], [1, 100], [1, 20]))
    assert split.record() == rec
    # the packed form carries the whole state (what the training script all-reduces), and sums like the totals do
    p = ValidationTotals().load_packed(ValidationTotals().add(a).packed() + ValidationTotals().add(b).packed())
    assert p.record() == rec and p.packed().dtype == torch.float64 and p.packed().shape == (4,)
    assert ValidationTotals().record() == {"val_loss": 0.0, "val_token_acc": 0.0, "val_n_tokens": 0, "val_n_samples": 0}
    t.reset()
    assert t.record()["val_n_samples"] == 0
    big = ValidationTotals()  # float64 sums: 2^24 + 1 survives
    big.add(_Score([16777216.0], [1], [0])).add(_Score([1.0], [1], [0]))
    assert big.record()["val_loss"] == 16777217.0 / 2


# ---- the training script's flags ------------------------------------------------------------------------------------------------------------------
def test_validation_flags(tt):
    d = tt.parse_args([])
    assert d.val_freq == 0 and d.val_samples_dicts_dir is None and d.n_val == 256 and d.val_batch_size == d.train_batch_size
    assert all(f in tt.NATIVE_FLAGS for f in ("val_freq", "val_samples_dicts_dir", "n_val", "val_batch_size"))
    a = tt.parse_args(["--val_freq=50", "--n_val=32", "--val_batch_size=16", "--train_batch_size=4"])
    assert (a.val_freq, a.n_val, a.val_batch_size) == (50, 32, 16)
    assert tt.parse_args(["--val_freq=5", "--train_batch_size=4"]).val_batch_size == 4
    for bad in (["--val_freq=-1"], ["--val_freq=1.5"], ["--val_freq=True"], ["--n_val=0", "--val_freq=1"], ["--val_batch_size=0", "--val_freq=1"],
                ["--val_samples_dicts_dir=/tmp/x"], ["--val_samples_dicts_dir=/tmp/x", "--val_freq=0"],
                ["--val_freq=5", "--synthetic=False", "--samples_dicts_dir=/tmp/x"]):
        with pytest.raises(SystemExit):
            tt.parse_args(bad)
    ok = tt.parse_args(["--val_freq=5", "--synthetic=False", "--samples_dicts_dir=/tmp/x", "--val_samples_dicts_dir=/tmp/y"])
    assert ok.val_samples_dicts_dir == "/tmp/y"


def test_synthetic_validation_indices_are_disjoint(tt):
    from olmoasr_amd import ddp
    args = tt.parse_args(["--val_freq=10", "--n_synthetic=512", "--n_val=64"])
    val = tt.val_indices(args)
    assert len(val) == len(set(val)) == 64 and val[0] == 512 + 8
    held_out = {args.n_synthetic + i for i in range(8)}  # evaluate()'s clips (main)
    train = set()
    for rank in range(8):
        train |= set(ddp.shard_indices(args.n_synthetic, rank, 8))
    assert train == set(range(512))
    assert not set(val) & train and not set(val) & held_out


def test_validation_batches_trim_to_the_span():
    from olmoasr_amd import validation
    from olmoasr_amd.synth import supervised_span_host
    pcm, ti, ty, tl = validation.synthetic_batch([520, 521, 522])
    assert pcm.shape == (3, 480000) and pcm.dtype == torch.int16 and ti.shape == ty.shape == (3, 448) and tl.dtype == torch.int32
    span = supervised_span_host(ty, tl)
    S = validation.trimmed_context(span)
    assert S % 64 == 0 and int(span.max()) <= S < int(span.max()) + 64 and bool((ty[:, S:] == 51864).all())
    assert validation.trimmed_context(torch.tensor([1])) == 64 and validation.trimmed_context(torch.tensor([448])) == 448
    assert validation.trimmed_context(torch.tensor([65, 3])) == 128


# ---- the host twin under a sanitizer ------------------------------------------------------------------------------------------------------------
def test_score_host_check_under_sanitizers(tmp_path):
    """Builds csrc/tools/score_host_check.cpp with score_host.cpp under AddressSanitizer + UBSan (host code only, a program of its own) and
    runs it: the twin against the rule written out again, buffers of exactly the size a call may touch."""
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "score_host_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(CSRC, "tools", "score_host_check.cpp"), os.path.join(CSRC, "score_host.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "0 mismatches" in res.stdout and "bad arguments accepted: 0" in res.stdout
