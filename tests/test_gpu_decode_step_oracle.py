"""The KV-cached decoder step's bf16 engines -- multi-launch (csrc/decode_proj.hip), one-XCD team (csrc/decode_xcd.hip), chip-wide
(csrc/decode_wide.hip) -- against the CPU oracle, not against each other: tests/test_gpu_decode_step.py compares HIP with HIP, so a rounding
point misplaced in decode_shared.h (all engines at once) or an error of the chip-wide engine below its 4-ulp envelope passes there.

Every case: one seeded state_dict on both sides, a synthetic encoder output xa [B, Te, d] (N(0, 1), rounded to bf16: identical values on
both sides, and Te is free to vary), random tokens behind <sot>.  Native: per-position logits of kv_cache_begin / _step / _check with the
engine forced (test_gpu_decode_step._steps).  Oracle (oracle/model_oracle.py, TextDecoder.forward without the cache, model.py:688-775; the
causal mask makes row p the cached step p): ``ref`` in fp32 and ``mir`` under the reference's autocast rounding points.  The mirror receives
xa as a bf16 tensor -- what the autocast encoder hands the decoder -- so that model.py:732 rounds the embedded tokens to bf16 and the
residual stream is bf16, as in the reference under autocast and in the engines.

Bounds: the training path's (test_gpu_parity_sizes.py), unchanged --
  * finite logits, a clean kv_cache_check
  * max |native - ref| <= 1.5 max |mir - ref|, the same for the means
  * against the mirror >= 99.9 % of the logits within 2 bf16 ulp of the logit scale, none beyond 4 (tests/bf16_ulp.py)
  * argmax == ref's wherever ref's top-2 gap exceeds 2 max |mir - ref| ("clear" positions); at least half of the (b, p) positions of
    every case are clear -- asserted from ref and mir alone, checked on the CPU before any GPU run
  * B = 1 in modes 5 / -1: the chip-wide engine's flag epoch in the cache tail is non-zero (no silent fallback); a forced team engine
    leaves its barrier counter; a shape the forced engine declines must meet the bounds on the engine it falls back to, with neither trace.

Seed and sharpening: the token embedding is multiplied by SHARPEN = 8 (the ``pair`` fixture of test_gpu_decode_parity.py uses 3 against the
fp32 engine; kaiming init alone gives near-flat distributions).  The top-2 gap and the bf16 envelope both grow with the head's scale, so
the share of clear positions rises only once the tied embedding makes the input token's own logit stand out: about 0.45-0.55 at x 3-6
whatever the seed, 0.6-0.9 at x 8 (largest logit 55-81 against ~48 for the bulk's maximum, so the ulp of the logit scale is still that of
the bulk or one binade above it), 1.0 at x 16 -- where one outlier of 220 would set the ulp and the bound would say little about the rest.
The state_dict seeds (the case lists below) are those of three tried per case whose share is at least 0.625 on the CPU, so that a CPU whose
bf16 matmul sums in another order (the mirror's envelope moves by ~10 % between machines) still has half the positions clear; every test
asserts the share before it looks at the engine.

Shapes, from the sources: the chip-wide engine splits the cross-attention keys of a head over WNS = 8 workgroups of ceil(Te / 8) keys, each
with 72 lane groups x WCK = 3 key slots -- a segment is EMPTY (m = -inf, l = 0 in the merge) as soon as Te < 8, so the smallest Te with an
empty segment is 1 (seven of eight empty; the issue's 5 leaves three), and every key slot is full at Te = 8 x 216 = 1728, not at 1536
(decode_wide_supports accepts up to 1728; at 1536 the third slot of a group is two-thirds full).  The team engine and the multi-launch
attention kernel take the keys in ceil(Te / 768) <= 2 segments: no empty segment exists there, both segments are full at 1536, and the team
engine declines Te = 1728 (-> folded multi-launch step, whose attention then runs the tiled kernel: Tk > 1536).  Both sets of values run.
The team engine also declines d % 256 != 0, so at d = 384 mode 2 is the folded multi-launch step; cases b and c repeat mode 2 at d = 512,
where the team runs.

Measured on an MI355X, all 38 cases inside the bounds: share of logits within 0.5 / 1 / 2 / 4 ulp of the mirror and the largest distance, the
worst of the runs of each (case, d, engine); max |native - ref| was 0.78-1.21 x the mirror's, the mean 0.96-1.01 x.
    case d     engine   0.5      1        2        4       max ulp
    a    384   wide   0.99087  1.00000  1.00000  1.00000  1.25
    a    384   multi  0.99145  1.00000  1.00000  1.00000  1.25
    a    768   wide   0.86520  0.99331  1.00000  1.00000  2.12
    a    768   multi  0.86119  0.99275  1.00000  1.00000  2.12
    a    1280  wide   0.99387  1.00000  1.00000  1.00000  1.00
    a    1280  multi  0.99474  1.00000  1.00000  1.00000  1.00
    b    384   multi  0.88198  0.99457  1.00000  1.00000  2.06
    b    512   team   0.99517  1.00000  1.00000  1.00000  1.00
    c    384   wide   0.83430  0.98537  0.99998  1.00000  2.50
    c    384   multi  0.85924  0.99082  1.00000  1.00000  2.50
    c    512   team   0.85591  0.99103  1.00000  1.00000  2.19
    d    512   wide   0.98904  1.00000  1.00000  1.00000  1.25
    d    512   team   0.98917  1.00000  1.00000  1.00000  1.38
(Rows with 0.83-0.88 within half an ulp are the cases whose largest logit is below 64: their ulp is 0.25, not 0.5.)
What the bounds see and what they do not -- deliberately wrong mirrors against the mirror, on the CPU, cases a (inference layout) and d;
mean distance in ulp, share within 2 ulp, largest distance (the engines themselves: mean 0.155 / 0.308 / 0.148 / 0.166):
    variant                                   a 384              a 768              a 1280             d 512, S = 448
    fp32 accumulation, same rounding points   0.081 1.00000 0.75  0.191 1.00000 1.50  0.107 1.00000 0.75  0.111 1.00000 1.00
    P not rounded to bf16 before P.V          0.157 1.00000 1.38  0.305 1.00000 2.00  0.151 1.00000 1.06  0.162 1.00000 1.25
    residual stream kept in fp32              0.197 1.00000 1.62  0.383 0.99993 3.50  0.203 1.00000 1.56  0.217 1.00000 1.82
    every Linear output TRUNCATED to bf16     0.217 1.00000 1.62  0.447 0.99912 3.25  0.211 1.00000 1.56  0.289 1.00000 2.38
None of the four FAILS the bounds at these shapes (against ref the truncating variant reaches 1.35 x the mirror's mean at S = 448, bound
1.5): with two layers a missing or misplaced rounding point moves a logit by a fraction of an ulp of the logit scale, and ANY other
summation order already decorrelates the bf16 roundings from the mirror's (the engines sit exactly where the P-unrounded variant sits).
What the bounds do hold the engines to: no error above two ulp of the logit scale on more than 0.1 % of the logits, none above four --
a wrong key, a dropped segment, a stale packet, a NaN from an empty segment, a row of the vocabulary assigned twice or not at all, an
engine that silently is not the one asked for -- against a reference that shares no code with the engines.  (On the CPU again, d = 384,
B = 1: a mirror without the last eighth of the cross-attention keys is 1.6 / 3.8 / 5.5 / 13.9 ulp away on average at Te = 1500 / 1536 /
200 / 5 and fails every bound; one that reads every key's neighbour instead is 6.8 / 10.3 / 107 ulp away at most at Te = 1536 / 200 / 5
and fails, but stays inside the bounds at case a's Te = 1500.)  A rounding point misplaced
by less than that needs deeper models than a quick test affords (test_gpu_parity_sizes.py has them for the training path).
"""
import os

import pytest
import torch

from bf16_ulp import bf16_ulp_report
from test_gpu_decode_step import _dims, _steps, _tail

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHARPEN = 8.0
L = 2  # decoder layers everywhere: the packet hand-over between layers needs two


def _build_case(d, H, B, S, Te, inference, seed):
    """State_dict, inputs and the two oracle evaluations of one case (CPU only)."""
    from oracle import model_oracle as mo
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    dims = mo.Dims(80, Te, d, H, 1, 51864, 448, d, H, L)
    sd = mo.init_state_dict(dims, seed=seed, train_vocab_rows=not inference)
    sd["decoder.token_embedding.weight"] = sd["decoder.token_embedding.weight"] * SHARPEN
    g = torch.Generator().manual_seed(1000 + seed)
    xa = torch.randn(B, Te, d, generator=g) * torch.linspace(1.0, 0.8, B)[:, None, None]  # per-row inputs differ in scale as well
    xa = xa.to(torch.bfloat16).float()
    toks = torch.randint(0, 50000, (B, S), generator=g)
    toks[:, 0] = 50257
    with torch.no_grad():
        ref = mo.decoder_forward(sd, dims, toks, xa)
        mir = mo.decoder_forward(sd, dims, toks, xa.to(torch.bfloat16), autocast_bf16=True)
    env = (mir - ref).abs()
    top2 = ref.topk(2, -1).values
    clear = (top2[..., 0] - top2[..., 1]) > 2 * float(env.max())
    return dict(dims=dims, sd=sd, xa=xa, toks=toks, ref=ref, mir=mir, env_max=float(env.max()), env_mean=float(env.mean()), clear=clear,
                inference=inference, key=(d, H, B, S, Te, inference, seed))


_CASES, _NET = {}, {}


def _case(*key):
    if key not in _CASES:
        _CASES[key] = _build_case(*key)
    return _CASES[key]


def _net(c):
    """the case's model on the bf16 engine (one alive at a time: consecutive modes of a case share it)"""
    from olmoasr_amd.model import OLMoASR
    if _NET.get("key") != c["key"]:
        _NET.clear()
        torch.cuda.empty_cache()
        net = OLMoASR(_dims(c["dims"]), device=DEV, seed=0, inference=c["inference"])
        res = net.load_state_dict(c["sd"], strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        _NET.update(key=c["key"], net=net)
    return _NET["net"]


def _engine_of(c, mode):
    """The engine pick_step_engine (csrc/engine_decode.hip) gives this case on a whole MI355X: 'wide', 'team' or 'multi'."""
    from olmoasr_amd import _native as N
    d, H, B, S, Te, inference, _ = c["key"]
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    nwg = 256 if n_cu >= 256 else n_cu & ~3
    rows = 51864 + (0 if inference else 1)
    if mode in (-1, 5) and B == 1 and N.lib().oasr_wide_supports_debug(d, H, Te, 448, L, 1, nwg, rows) == 1:
        return "wide"
    if ((mode == -1 and B == 1) or mode >= 2) and d % 256 == 0 and B <= 4 and Te <= 1536:  # decode_xcd_supports
        return "team"
    return "multi"


def _check(c, mode, tag, must_be=None):
    net = _net(c)
    # ---- the gate, from the oracle alone ----
    share = float(c["clear"].float().mean())
    print(f"[{tag} mode {mode}] mirror envelope max {c['env_max']:.4f} mean {c['env_mean']:.5f}; clear positions {share:.3f}")
    assert share >= 0.5, share
    info = {}
    got = _steps(net, c["xa"].to(DEV), c["toks"].to(DEV), mode, info).cpu()
    assert info["ok"] is True
    assert torch.isfinite(got).all()
    # ---- which engine ran ----
    engine = _engine_of(c, mode)
    tail = _tail(info["state"])
    counter, epoch = int(tail[0]), int(tail[4])
    if c["key"][2] == 1 and mode in (-1, 5):
        assert epoch != 0, f"flag epoch {epoch}: the chip-wide one-launch engine did not run"
    if must_be is not None:
        assert engine == must_be, (engine, must_be)
    assert (epoch != 0) == (engine == "wide") and (counter != 0) == (engine == "team"), (engine, counter, epoch)
    # ---- against the fp32 oracle, within the mirror's own envelope ----
    ref, mir = c["ref"], c["mir"]
    err = (got - ref).abs()
    print(f"   {engine}: vs fp32 oracle max {float(err.max()):.4f} mean {float(err.mean()):.5f} | scale {float(ref.abs().max()):.2f}")
    valid = torch.ones(got.shape[:2], dtype=torch.bool)
    within2, worst_ulp = bf16_ulp_report(got, mir, valid, f"{tag} mode {mode} {engine}")
    assert float(err.max()) <= 1.5 * c["env_max"], (float(err.max()), c["env_max"])
    assert float(err.mean()) <= 1.5 * c["env_mean"], (float(err.mean()), c["env_mean"])
    assert within2 >= 0.999 and worst_ulp <= 4.0, (within2, worst_ulp)
    assert (got.argmax(-1)[c["clear"]] == ref.argmax(-1)[c["clear"]]).all()


# ---- a. the three instantiations of the chip-wide engine at 256 workgroups (R_d = 2, 4, 6), both head layouts ----------------------------
A_CASES = [(384, 6, True, 31), (384, 6, False, 132), (768, 12, True, 33), (768, 12, False, 34), (1280, 20, True, 35), (1280, 20, False, 36)]


@pytest.mark.parametrize("d,H,inference,seed,mode", [a + (m,) for a in A_CASES for m in (5, -1, 1)])
def test_one_sequence_on_every_engine_vs_oracle(d, H, inference, seed, mode):
    """B = 1, S = 12, Te = 1500: the chip-wide engine (forced and as the default) and the multi-launch engine each meet the bound on their own."""
    c = _case(d, H, 1, 12, 1500, inference, seed)
    _check(c, mode, f"a d={d} {'inference' if inference else 'training'} layout", must_be="wide" if mode != 1 else "multi")


# ---- b. the batch rules of pick_step_engine ---------------------------------------------------------------------------------------------
B_CASES = [(384, 6, 3, 2, 41), (384, 6, 3, -1, 41), (384, 6, 5, -1, 42), (384, 6, 17, -1, 43), (512, 8, 3, 2, 144)]


@pytest.mark.parametrize("d,H,B,mode,seed", B_CASES)
def test_batched_step_vs_oracle(d, H, B, mode, seed):
    """B = 3 forced onto the team engine (d = 384: declined, folded multi-launch; d = 512: the team) and by default (folded), B = 5 (folded, no
    team), B = 17 (separate LayerNorm kernels)."""
    c = _case(d, H, B, 12, 1500, True, seed)
    _check(c, mode, f"b d={d} B={B}", must_be="team" if (d, mode) == (512, 2) else "multi")


# ---- c. the cross-attention key split: full, ragged, with empty segments ----------------------------------------------------------------
C_SEEDS = {(1, 1728): 251, (2, 1728): 251, (1, 1536): 252, (2, 1536): 252, (1, 200): 53, (2, 200): 53, (1, 5): 154, (2, 5): 154, (1, 1): 55, (2, 1): 155}
C_CASES = [(384, 6, B, mode, Te, C_SEEDS[B, Te]) for Te in (1728, 1536, 200, 5, 1) for B, mode in ((1, 5), (2, 2))] + \
          [(512, 8, 2, 2, 1536, 61), (512, 8, 2, 2, 200, 262), (512, 8, 2, 2, 5, 263)]


@pytest.mark.parametrize("d,H,B,mode,Te,seed", C_CASES)
def test_cross_attention_key_split_vs_oracle(d, H, B, mode, Te, seed):
    """Te = 1728 / 1536: every key slot of the chip-wide engine / of the team engine's two segments full; 200: ragged; 5 and 1: three and
    seven of the chip-wide engine's eight segments empty (module docstring).  B = 2 in mode 2 at d = 384 is the folded multi-launch step
    (its attention kernel: one segment, the second empty, for Te <= 768; the tiled kernel at 1728); at d = 512 the team engine."""
    c = _case(d, H, B, 12, Te, True, seed)
    _check(c, mode, f"c d={d} B={B} Te={Te}", must_be="wide" if B == 1 else ("team" if d == 512 else "multi"))


# ---- d. the full text context once -----------------------------------------------------------------------------------------------------
D_KEY = (512, 8, 1, 448, 1500, True, 71)


@pytest.fixture(scope="module")
def full_context():
    return _case(*D_KEY)


@pytest.mark.parametrize("mode", [5, 2])
def test_full_text_context_vs_oracle(full_context, mode):
    """All 448 positions, one sequence: self-attention crosses the engines' key-group and 256-key boundaries against an independent
    reference -- the chip-wide engine and the one-XCD team, same bounds over every position."""
    _check(full_context, mode, "d d=512 S=448", must_be="wide" if mode == 5 else "team")
