"""The planted rows of tests/vocab_planted.py see what they claim to see (CPU only).

The check functions tests/test_gpu_vocab_planted.py applies to the kernels are applied here to stand-ins for the kernels written in float32
torch (``emulate_ce`` / ``emulate_sel``).  Unflawed, every case passes -- so the bounds hold for the plain float32 formula before any GPU
run -- and each planted flaw (a dropped register slot, a wave left out of a reduction, a loop bound one tile short, ...) fails the named
case and check.  Run with -s to see the flaw -> case table."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vocab_planted as P  # noqa: E402

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64


# ---- cross-entropy --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.CE_CASES)
def test_ce_case_values_are_exact_and_the_float32_formula_meets_the_bounds(name):
    c = P.ce_case(name)
    V = c["V"]
    assert torch.equal(c["logits"][:, :V].to(F64), c["x"]), "a planted value is not a bf16 value"
    assert torch.equal(P.ce_f32_logits(c, True)[:, :V].to(F64), c["x"])
    if c["ld"] > V:
        pad = c["logits"][:, V:]
        assert bool(torch.isnan(pad[0::2].float()).all()) and bool((pad[1::2].float() > 2.9e38).all())
    assert c["logits"].shape[0] <= 64
    for eps, z in [(0.0, 0.0)] + ([P.REG] if name in P.CE_REG_CASES else []):
        for store, padded in ((BF, True), (F32, True), (F32, False)):
            fails, fig = P.check_ce(c, P.emulate_ce(c, eps, z, store=store, padded=padded), eps, z)
            print(f"   {name} eps={eps} z={z} {'bf16' if store == BF else 'fp32'}: " + ", ".join(f"{k} {v:.3g}" for k, v in fig.items()))
            assert fails == [], (name, eps, z, store, fails)


def test_ce_cases_plant_what_the_issue_lists():
    n = P.ce_case("needle")
    cols = {int(r.argmax()) for r in n["x"]}
    V = n["V"]
    assert cols >= {0, 7, 8, 8191, 8192, 49152, 8 * (V // 8), V - 2, V - 1} | {512 * k for k in range(1, 16)}
    assert n["ignore"] == -100 and set(n["targets"].tolist()) >= {V - 1, 3}
    assert {(int(r.argmax()) // 8) // 1024 for r in n["x"]} == set(range(7))                      # every register slot
    assert {((int(r.argmax()) // 8) % 1024) // 64 for r in P.ce_case("wave_peaks")["x"]} == set(range(16))  # every wave
    p = P.ce_case("peaked")
    assert sorted({int(r.max()) for r in p["x"]}) == list(P.PEAK_MARGINS)
    e = P.ce_expect(p)
    assert float(e["p"].max()) >= 1 - 1e-15 and float(e["row_loss"][e["valid"]].min()) < 1e-30    # lse - x_t far below fp32 resolution
    o = P.ce_case("offset")
    assert float(o["x"].max()) == 72.0 and float(o["x"].min()) >= -80.0 and bool((o["x"] * 2 == torch.round(o["x"] * 2)).all())
    for V, ld in P.CE_SHAPES:
        s = P.ce_case(f"shapes-{V}x{ld}")
        t = s["targets"]
        e = P.ce_expect(s)
        oor = (t != s["ignore"]) & ((t < 0) | (t >= V))
        assert int(oor.sum()) == 2 and int((t == s["ignore"]).sum()) == 4 and e["n_valid"] == 10
        assert {0, V - 1} <= set(t[e["valid"]].tolist())
    a = P.ce_expect(P.ce_case("all_ignored"))
    assert a["n_valid"] == 0 and a["loss"] == 0.0 and not bool(a["grad"].any())


CE_CAUGHT_BY = {  # flaw -> (case, the check that must fail there)
    "slot6": ("needle", "grad"),
    "max_wave": ("wave_peaks", "finite"),
    "sum_wave": ("needle", "row_loss"),
    "pad_kept": ("needle", "finite"),
    "straddle_gt": ("needle", "finite"),
    "onehot_off": ("needle", "grad"),
    "trunc": ("shapes-51865x51968", "rne_mean"),
    "count_oor": ("shapes-51865x51968", "n_valid"),
    "no_max": ("peaked", "finite"),
}


@pytest.mark.parametrize("flaw", P.CE_FLAWS)
def test_each_cross_entropy_flaw_fails_a_named_case(flaw):
    name, check = CE_CAUGHT_BY[flaw]
    c = P.ce_case(name)
    fails, _ = P.check_ce(c, P.emulate_ce(c, flaw=flaw))
    print(f"   {flaw:12s} caught by {name}: {fails}")
    assert check in fails, (flaw, name, fails)


def test_cross_entropy_flaws_that_need_their_own_case():
    """What only one case can see: the truncating store passes every one-ulp bound (the rounding statistic catches it); a wave missing from
    the maximum is invisible to a +8 needle (the sum stays finite) and needs the +120 rows; targets outside [0, V) counted as valid also
    show in all_ignored; a dropped slot 6 also shows at ld = 57344."""
    fails, _ = P.check_ce(P.ce_case("needle"), P.emulate_ce(P.ce_case("needle"), flaw="trunc"))
    assert fails == []
    fails, _ = P.check_ce(P.ce_case("needle"), P.emulate_ce(P.ce_case("needle"), flaw="max_wave"))
    assert fails == []
    c = P.ce_case("all_ignored")
    assert "n_valid" in P.check_ce(c, P.emulate_ce(c, flaw="count_oor"))[0]
    c = P.ce_case("shapes-57344x57344")
    assert "grad" in P.check_ce(c, P.emulate_ce(c, flaw="slot6"))[0]
    c = P.ce_case("shapes-51865x51968")
    assert "rne_mean" in P.check_ce(c, P.emulate_ce(c, *P.REG, flaw="trunc"), *P.REG)[0]


# ---- selection --------------------------------------------------------------------------------------------------------------------------------
def _emu(case, flaw=None):
    return lambda kind, **kw: P.emulate_sel(case, kind, flaw, **kw)


@pytest.mark.parametrize("V", P.SEL_V)
def test_selection_cases_are_exact_and_pass_on_the_stand_in(V):
    for c in P.sel_cases(V):
        x32 = c["logits"][:, :V].to(F64)
        assert torch.equal(x32, c["x"]), c["name"]
        pad = c["logits"][:, V:]
        assert bool(torch.isposinf(pad[0::2]).all()) and bool(torch.isnan(pad[1::2]).all()) and c["ld"] == V + 103
        P.sel_filtered(c)
        if c["rules"] is not None:  # the force decision is an exact tie where one is planted, and nowhere else near fp32's resolution
            m = c["_force_margin"]
            assert bool((~torch.isfinite(m) | (m == 0) | (m.abs() > 5e-4)).all()), (c["name"], m)
        assert P.sel_failures(c, _emu(c)) == {}, c["name"]


@pytest.mark.parametrize("k", range(len(P.CDF_EXACT)))
def test_cdf_exact_cases(k):
    c = P.cdf_cases()[k]
    V, n = P.CDF_EXACT[k]
    pos, per = c["survivors"], (V + 255) // 256
    assert len(pos) == n and (V - 1 in pos or n == 2)
    owners = sorted({p // per for p in pos})
    assert any(p % per == per - 1 and p + 1 in pos for p in pos)            # the last column of a range and the first of the next
    assert owners[-1] == (V - 1) // per                                     # the last, partial range
    assert n == 2 or n > 64 or V < 1000 or max(b - a for a, b in zip(owners, owners[1:])) > 1  # runs of empty ranges
    for T in P.CDF_T:
        want, _, _ = P.sel_expect_draw(c, T, c["u"])
        assert torch.equal(want, c["want_draw"]), (V, n, T)
    assert P.cdf_failures(c, _emu(c)) == {}


def test_selection_expectations_are_the_issues():
    V = 1000
    by = {c["name"]: c for c in P.sel_cases(V)}
    t = by[f"ties-V{V}-plain"]
    tok, lp = P.sel_expect_topk(t, 16)
    assert tok[0].tolist() == list(range(16)) and bool((lp[0] + math.log(V)).abs().max() < 1e-12)
    assert tok[1, :4].tolist() == [0, 1, 64, 256] and tok[2, :4].tolist() == [63, 64, 127, 319]
    tok, lp = P.sel_expect_topk(by[f"ties_masked-V{V}-plain"], 16)
    assert tok[0].tolist() == list(range(3, 19)) and bool((lp[0] + math.log(V - 3)).abs().max() < 1e-12)
    e = by[f"empty_and_single-V{V}-plain"]
    tok, lp = P.sel_expect_topk(e, 4)
    assert tok[0].tolist() == [0, 0, 0, 0] and bool((lp[0] == -math.inf).all())
    assert tok[1].tolist() == [0, 0, 0, 0] and lp[1].tolist() == [0.0] + [-math.inf] * 3     # single@0
    assert tok[-1].tolist() == [V - 1, 0, 0, 0] and lp[-1].tolist() == [0.0] + [-math.inf] * 3
    er = by[f"empty_and_single-V{V}-rules"]
    i = er["labels"].index(f"single@{er['ids']['no_timestamps']}")
    assert P.sel_expect_topk(er, 1)[1][i, 0] == -math.inf                                    # <|notimestamps|> alone: an empty row
    f = by[f"force_edge-V{V}-rules"]
    tok, lp = P.sel_expect_topk(f, 1)
    assert tok[:, 0].tolist() == f["want_pick"]
    assert abs(float(lp[1, 0]) + math.log(2)) < 1e-12 and float(lp[2, 0]) == 0.0
    n = by[f"needle-V{V}-rules"]
    assert n["ids"]["no_timestamps"] not in P.sel_expect_topk(n, 1)[0][:, 0].tolist()
    tr = by[f"ties-V{V}-rules"]
    a, s = tr["ids"]["timestamp_begin"] - 5, tr["ids"]["timestamp_begin"] + 7
    tok, _ = P.sel_expect_topk(tr, 2)
    assert tok[-2].tolist() == [a, s] and tok[-1, 0].item() == s                              # text first unless forced
    o = by[f"offsets-V{V}-plain"]
    w = list(o["winner_always"].items())[0]
    assert P.sel_expect_topk(o, 1)[0][w[0], 0] == w[1] and abs(float(P.sel_expect_topk(o, 1)[1][w[0], 0])) < 1e-12


@pytest.mark.parametrize("V", (51865, 300))
def test_rule_edges_agree_with_the_decoders_own_rules(V):
    """The expectation's rule mask is decoding._timestamp_rules' (pinned to transformers in tests/test_decoding_cpu.py); here the whole
    filtered row -- force step included -- is compared with that function run on a float64 copy of the planted row."""
    cases = [c for c in P.sel_cases(V) if c["kind"].startswith("rule_edges")]
    assert len(cases) == 4
    for c in cases:
        ref = c["x"].clone()
        r = c["rules"]
        with P._decoding_ids(c["ids"]) as D:
            D._timestamp_rules(ref, r["history"][:, :r["n_history"]], 0, r["max_initial_index"])
        assert torch.equal(torch.isinf(ref), torch.isinf(P.sel_filtered(c))), c["name"]
        tok = P.sel_expect_topk(c, 1)[0][:, 0].tolist()
        tb = c["ids"]["timestamp_begin"]
        want = {"rule_edges_first": [tb + 50, tb], "rule_edges_unpaired": [tb + 20, tb + 20],
                "rule_edges_pair": [0, 0, 5], "rule_edges_pair_then_text": [tb + 21, tb + 21]}[c["kind"]]
        assert tok == want, (c["name"], tok, want)


SEL_CAUGHT_BY = {  # flaw -> (V, case name, run, check)
    "stop_256": (51865, "needle-V51865-plain", "pick", "ids"),
    "to_ld": (51865, "needle-V51865-plain", "pick", "id_range"),
    "tie_high": (1000, "ties-V1000-plain", "topk K=16", "ids"),
    "wave_drop": (51865, "needle-V51865-plain", "pick", "ids"),
    "per_floor": (51865, ("cdf", 51865, 64), "sample T=1.0", "ids"),
    "le_run": (51865, ("cdf", 51865, 64), "sample T=1.0", "ids"),
    "force_ge": (300, "force_edge-V300-rules", "pick", "ids"),
    "nots_alive": (51865, "needle-V51865-rules", "pick", "dead_id"),
    "empty_nan": (257, "empty_and_single-V257-plain", "pick", "lp"),
}


@pytest.mark.parametrize("flaw", P.SEL_FLAWS)
def test_each_selection_flaw_fails_a_named_case(flaw):
    V, name, run, check = SEL_CAUGHT_BY[flaw]
    if isinstance(name, tuple):
        c = P.cdf_cases()[P.CDF_EXACT.index(name[1:])]
        fails = P.cdf_failures(c, _emu(c, flaw))
    else:
        c = {c["name"]: c for c in P.sel_cases(V)}[name]
        fails = P.sel_failures(c, _emu(c, flaw))
    print(f"   {flaw:12s} caught by {c['name']}: {fails}")
    assert check in fails.get(run, []), (flaw, name, fails)
