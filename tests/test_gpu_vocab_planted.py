"""The kernels of csrc/loss.hip -- ce_kernel<REG>, count_valid, loss_reduce --, those of csrc/select.hip -- pick / pick_ts / topk_ts /
sample_ts -- and the fp32 engine's ce_f32_kernel on the planted rows of tests/vocab_planted.py, against float64.  The cases, the bounds and the check functions live there
(``check_ce``, ``check_topk``, ``check_sample``); tests/test_vocab_planted_cpu.py shows on the CPU that those checks catch a dropped
register slot, a wave missing from a reduction, a loop bound off by a tile, a truncating store, ties to the wrong side and the like.

Cross-entropy runs through oasr_test_cross_entropy (include/oasr_testing.h: the body of oasr_cross_entropy_ex for bf16 and fp32 logits);
every case also runs with write_grad = 0, which must leave the logits -- poisoned pad included -- bit-identical and give the same row_loss.

Measured on one MI355X (-s prints them): row_loss as err / bound; the gradient as the worst excess over one ulp in units of the slack s_c
(<= 0: inside one ulp; 1 = the bound), for the columns with p < 0.5 and for the confident ones (p >= 0.5); |rne_mean| (bound 0.1).

    class        kernel        row_loss        gradient, p < 0.5    gradient, p >= 0.5    |rne_mean|
    needle       bf16 / reg    0.092 / 0.077   inside one ulp       --                    (flat rows: too few cells)
    needle       fp32 / reg    0.098 / 0.097   inside one ulp       --
    peaked       bf16 / reg    0.092 / 0.095   0.0038 / inside      0.31 / inside         0.0037 / 0.012
    peaked       fp32 / reg    0.092 / 0.077   8e-6 / 0.013         0.35 / inside
    offset       bf16          0.139           inside one ulp       inside one ulp        (too few cells)
    offset       fp32          0.094           inside one ulp       inside one ulp
    shapes       bf16 / reg    0.174 / 0.145   inside one ulp       inside one ulp        0.0079 / 0.011
    shapes       fp32 / reg    0.100 / 0.117   0.0077 / 0.032       0.091 / 0.31
    wave_peaks   bf16, fp32    0 (exact)       4e-13                --
    all_ignored  bf16, fp32    loss 0.0, every stored value bit-zero

Before the fixes that came with this suite the same rows gave: bf16 peaked 37 (p < 0.5, the margin-88 row: v_exp_f32 flushed softmax values
below 2^-126 whose gradients are normal numbers); fp32 peaked / offset / shapes-9x1024 / shapes-5x8 3.2 / 5.4 / 1.8 / 1.9 at the confident
column (exp(x - lse) and an fp32 sum of ~200 terms per thread); pick_tokens NaN for the log-probability of every row without survivors.
The selection kernels and the exact inverse-CDF draws pass without a figure: ids are compared exactly.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vocab_planted as P  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32


# ---- cross-entropy --------------------------------------------------------------------------------------------------------------------------
def _run_ce(case, eps, z, logits_in):
    from olmoasr_amd import ops
    tgt = case["targets"].to(DEV)
    out = {}
    for write_grad in (1, 0):
        lg = logits_in.to(DEV)
        loss, row, nv = ops.cross_entropy_test_(lg, case["V"], tgt, case["ignore"], gscale=P.GSCALE, write_grad=write_grad, label_smoothing=eps,
                                                z_loss=z)
        torch.cuda.synchronize()
        if write_grad:
            out.update(grad=lg.cpu(), row_loss=row.cpu(), loss=loss.cpu()[0], n_valid=int(nv))
        else:
            out.update(nograd_logits=lg.cpu(), nograd_row_loss=row.cpu(), logits_in=logits_in)
    return out


def _ce_params(dtypes):
    for name in P.CE_CASES:
        for reg in ((False, True) if name in P.CE_REG_CASES else (False,)):
            for d in dtypes:
                yield pytest.param(name, reg, d, id=f"{name}-{'reg' if reg else 'plain'}-{d}")


def _check(case, got, eps, z, tag):
    fails, fig = P.check_ce(case, got, eps, z)
    print(f"   {case['name']} eps={eps} z={z} {tag}: " + ", ".join(f"{k} {v:.3g}" for k, v in fig.items()))
    assert fails == [], (case["name"], tag, fails, fig)


@pytest.mark.parametrize("name,reg,dtype", _ce_params(("bf16",)))
def test_cross_entropy_bf16(name, reg, dtype):
    case = P.ce_case(name)
    eps, z = P.REG if reg else (0.0, 0.0)
    got = _run_ce(case, eps, z, case["logits"])
    _check(case, got, eps, z, "bf16")
    if name == "all_ignored":
        assert float(got["loss"]) == 0.0 and not bool(got["grad"].view(torch.int16).any()) and not bool(got["row_loss"].any())


@pytest.mark.parametrize("name,reg,dtype", _ce_params(("fp32-padded", "fp32-ld=V")))
def test_cross_entropy_fp32(name, reg, dtype):
    """ce_f32_kernel, the cross-entropy the fp32 validation engine is trusted for: the same cases and bounds, the bf16-ulp term replaced by
    2^-21 |want|."""
    case = P.ce_case(name)
    eps, z = P.REG if reg else (0.0, 0.0)
    got = _run_ce(case, eps, z, P.ce_f32_logits(case, dtype == "fp32-padded"))
    _check(case, got, eps, z, dtype)
    if name == "all_ignored":
        assert float(got["loss"]) == 0.0 and not bool(got["grad"].view(torch.int32).any())


def test_the_product_entry_is_the_hooks_bf16_path():
    """oasr_cross_entropy_ex (what the training step's unit operator calls) and the hook at bf16 share one body: bit-identical results."""
    from olmoasr_amd import ops
    case = P.ce_case("needle")
    tgt = case["targets"].to(DEV)
    a, b = case["logits"].to(DEV), case["logits"].to(DEV)
    la, ra = ops.cross_entropy_(a, case["V"], tgt, case["ignore"], gscale=P.GSCALE)
    lb, rb, _ = ops.cross_entropy_test_(b, case["V"], tgt, case["ignore"], gscale=P.GSCALE)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(ra, rb) and torch.equal(la, lb)


# ---- selection --------------------------------------------------------------------------------------------------------------------------------
def _gpu_run(case):
    from olmoasr_amd import ops
    V = case["V"]
    if "stored" in case:  # the cdf cases: one stored row and many draws -- 32 copies of the row, the draws in launches of 32
        lg = case["stored"].expand(32, case["ld"]).contiguous().to(DEV)
    else:
        lg = case["logits"].to(DEV)
    view = lg[:, :V]  # row stride ld: the pad lies between the rows
    mask = None if case["mask"] is None else case["mask"].to(DEV)
    r = case["rules"]
    kw = {}
    if r is not None:
        kw = dict(history=r["history"].to(DEV), n_history=r["n_history"], max_initial_index=r["max_initial_index"], **case["ids"])

    def run(kind, K=1, T=1.0, u=None):
        if kind == "pick":
            if r is None:
                tok, lp = ops.pick_tokens(view, mask=mask)
            else:
                tok, lp = ops.pick_tokens_ts(view, kw["history"], kw["n_history"], timestamp_begin=kw["timestamp_begin"], eot=kw["eot"],
                                             no_timestamps=kw["no_timestamps"], max_initial_index=kw["max_initial_index"], mask=mask)
        elif kind == "topk":
            lp, tok = ops.topk_tokens(view, K, mask=mask, **kw)
        elif "stored" in case:
            parts = [ops.sample_tokens(view[:len(uc)], T, uc.to(DEV), mask=mask) for uc in u.split(32)]
            tok, lp = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
        else:
            tok, lp = ops.sample_tokens(view, T, u.to(DEV), mask=mask, **kw)
        torch.cuda.synchronize()
        return tok.cpu(), lp.cpu()
    return run


@pytest.mark.parametrize("V", P.SEL_V)
def test_selection_kernels(V):
    """pick_tokens / pick_tokens_ts, topk_tokens (K = 1, 6, 16) and sample_tokens on every planted case at this vocabulary size: ids exact
    (equal values by ascending id), never >= V, never a column without survivor probability; log-probabilities within 2e-4 of float64,
    1e-6 where the expectation is 0, -inf exactly on a row without survivors -- from all four kernels (kernels.h at launch_pick_tokens)."""
    bad = {}
    for case in P.sel_cases(V):
        f = P.sel_failures(case, _gpu_run(case))
        if f:
            bad[case["name"]] = f
    assert bad == {}, bad


@pytest.mark.parametrize("V", P.SEL_V)
def test_pick_ts_equals_topk_first(V):
    """pick_ts_kernel stores what row_stat computes, and topk_ts_kernel's first entry is taken from the same row_stat: on every planted
    case with rules ops.pick_tokens_ts and ops.topk_tokens(k = 1) give equal ids and log-probabilities that compare == (-inf == -inf on
    the empty rows; a zero of either sign on a row with one survivor)."""
    bad = {}
    n = 0
    for case in P.sel_cases(V):
        if case["rules"] is None:
            continue
        n += 1
        run = _gpu_run(case)
        (tok, lp), (tok1, lp1) = run("pick"), run("topk", K=1)
        rows = [r for r in range(tok.shape[0]) if int(tok[r]) != int(tok1[r, 0]) or not float(lp[r]) == float(lp1[r, 0])]
        if rows:
            bad[case["name"]] = [(r, int(tok[r]), int(tok1[r, 0]), float(lp[r]), float(lp1[r, 0])) for r in rows]
    assert n > 0 or P.sel_ids(V) is None
    assert bad == {}, bad


@pytest.mark.parametrize("k", range(len(P.CDF_EXACT)), ids=[f"V{V}-n{n}" for V, n in P.CDF_EXACT])
def test_sample_inverse_cdf_is_exact_on_unit_masses(k):
    """n survivors of equal logit, all else masked: every mass is 1.0 at any temperature, so u = j / n draws survivor j exactly, u = 0 the
    first, u = 1 - 2^-24 the last -- over range boundaries, thread 255's partial range and runs of empty ranges."""
    case = P.cdf_cases()[k]
    assert P.cdf_failures(case, _gpu_run(case)) == {}
