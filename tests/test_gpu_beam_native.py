"""Device-resident beam search on the GPU: ``ops.beam_update`` against its host twin on the planted cases of tests/beam_cases.py (every
tensor of the state, guard rows and sentinels included), ``kv_cache_reorder_native`` against the existing ``kv_cache_reorder`` byte for byte
on the whole cache buffer, and ``decode(beam_backend="native")`` against ``decode(beam_backend="host")`` (exactly) and the CPU oracle (under
the bounds of tests/test_gpu_decode_parity.py) on the fp32 engine."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_cases as bc  # noqa: E402

DEV = "cuda"
KEEP = [1000, 2000, 3000, 4000, 5000]  # the restricted vocabulary: five text tokens (none of them suppressed or blank) and eot


def _dims(mo_dims):
    from olmoasr_amd.config.model_dims import ModelDimensions
    return ModelDimensions(**{k: getattr(mo_dims, k) for k in ModelDimensions.__dataclass_fields__})


# ---- the operator against its host twin ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bc.all_cases(), ids=lambda c: c["name"])
def test_beam_update_equals_the_host_twin(case):
    from olmoasr_amd import ops
    host = bc.run_state(ops, case, "cpu", ops.beam_update_host)
    for (i, st, tokens_in, before_in, before_out, want), (_, ht, *_rest) in zip(bc.run_state(ops, case, DEV, ops.beam_update), host):
        # every tensor of the state, with its guard rows and whatever the sentinel still covers: token rows behind len + 1, the step's input
        # buffer, the rows of a short window, unused pool slots
        for name, back in st.backing.items():
            assert torch.equal(back.cpu(), ht.backing[name]), (case["name"], i, name)
        assert st.cur == ht.cur and st.len == ht.len
        assert tokens_in.equal(before_in), (case["name"], i, "the step's input buffer was written")
        assert st.tokens[:, st.len:].eq(bc.FILL).all(), (case["name"], i, "written behind len + 1 tokens")
        beam = case["beam"]
        for a, short in enumerate(want["short"]):
            if short:
                assert st.tokens[a * beam:(a + 1) * beam].equal(before_out[a * beam:(a + 1) * beam]), (case["name"], i, "short window written")
        bc.guards_intact(st)
        got = bc.state_snapshot(st, want)  # ... and the restatement itself
        for key in want:
            assert got[key] == want[key], (case["name"], i, key)


def test_beam_update_refuses_before_the_launch():
    from olmoasr_amd import ops
    st = ops.beam_state(2, 3, 3, 24, bc.INIT, DEV, fill=bc.FILL, guard=1)
    before = {k: v.clone() for k, v in st.backing.items()}
    lp, tok = torch.zeros(6, 4, device=DEV), torch.zeros(6, 4, dtype=torch.int64, device=DEV)
    for bad_lp, bad_tok in ((lp, tok[:, :3].contiguous()), (lp[:5], tok), (lp, tok.cpu()), (lp, tok.int())):
        with pytest.raises(ValueError):
            ops.beam_update(st, bad_lp, bad_tok, eot=bc.EOT)
    with pytest.raises(ValueError):
        ops.beam_update_host(st, lp, tok, eot=bc.EOT)
    torch.cuda.synchronize()
    assert all(torch.equal(v, before[k]) for k, v in st.backing.items())


# ---- the cache reorder -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
def test_reorder_native_moves_exactly_what_kv_cache_reorder_moves(dtype):
    from olmoasr_amd import _native as N
    from olmoasr_amd.model import OLMoASR
    from oracle import model_oracle as mo
    dims = mo.Dims(80, 1500, 384, 6, 2, 51864, 448, 384, 6, 2)
    net = OLMoASR(_dims(dims), device=DEV, seed=5, inference=True, compute_dtype=dtype)
    g = torch.Generator().manual_seed(9)
    xa = torch.randn(6, 1500, 384, generator=g).to(DEV)
    state = net.kv_cache_begin(xa)
    sources = [0, 0, 1, 5, 3, 3]  # two windows x beam 3
    src_dev = torch.tensor(sources, dtype=torch.int32, device=DEV)
    ident = torch.arange(6, dtype=torch.int32, device=DEV)
    net.kv_cache_reorder_native(state, src_dev, 3)  # pos = 0: nothing is cached yet
    fed = 0
    for pos in (1, 5):
        while fed < pos:
            net.kv_cache_step(state, torch.randint(0, 50000, (6,), generator=g).to(DEV))
            fed += 1
        assert state["pos"] == pos
        start = state["cache"].clone()
        if pos == 1:  # (pos = 0 above left the buffer as decode_begin + the first step wrote it: that step ran on an untouched cache)
            zero = dict(state, pos=0)
            net.kv_cache_reorder_native(zero, src_dev, 3)
            assert torch.equal(state["cache"], start)
        net.kv_cache_reorder_native(state, ident, 3)
        assert torch.equal(state["cache"], start), "identity sources moved something"
        want = dict(state, cache=start.clone())
        net.kv_cache_reorder(want, sources)
        assert not torch.equal(want["cache"], start)
        net.kv_cache_reorder_native(state, src_dev, 3)
        assert torch.equal(state["cache"], want["cache"]), f"pos {pos}: the whole buffer (self rows, cross K/V, later positions, control tail)"
        # a source outside its window: refused on the host where the index is readable, ignored by the kernel where it is not
        held = state["cache"].clone()
        foreign = torch.tensor([0, 0, 3, 5, 3, 3], dtype=torch.int32)
        with pytest.raises(N.NativeError, match="outside its group"):
            N.call("oasr_decode_reorder", net._ctx, state["cache"], 6, pos, 3, foreign.to(DEV), foreign, N.STREAM)
        net.kv_cache_reorder_native(state, foreign.to(DEV), 3)  # window 0 is skipped, window 1 moves: [5, 3, 3] of the rows as they are now
        part = dict(state, cache=held.clone())
        net.kv_cache_reorder(part, [0, 1, 2, 5, 3, 3])
        assert torch.equal(state["cache"], part["cache"])
    with pytest.raises(ValueError):
        net.kv_cache_reorder_native(state, src_dev.long(), 3)
    with pytest.raises(N.NativeError):
        net.kv_cache_reorder_native(state, src_dev, 4)  # a group that does not divide B


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair(tiny_case):
    """The ``pair`` recipe of tests/test_gpu_decode_parity.py: 2-layer d=384 inference-layout model on both sides, same weights; fp32
    engine.  Three windows (the third a blend of the two seeded ones), and the oracle's encoder output of them, computed once."""
    from olmoasr_amd.model import OLMoASR
    from oracle import model_oracle as mo
    torch.set_num_threads(min(32, len(os.sched_getaffinity(0))))
    dims = mo.Dims(80, 1500, 384, 6, 2, 51864, 448, 384, 6, 2)
    sd = mo.init_state_dict(dims, seed=21, train_vocab_rows=False)
    sd["decoder.token_embedding.weight"] = sd["decoder.token_embedding.weight"] * 3.0
    net = OLMoASR(_dims(dims), device=DEV, seed=0, inference=True, compute_dtype="float32")
    net.load_state_dict(sd)
    mel = tiny_case["mel"]
    mel3 = torch.cat([mel, 0.5 * mel[:1] + 0.5 * mel[1:]])
    return net, sd, dims, mel3, mo.encoder_forward(sd, dims, mel3)


def _oracle(pair, n_windows, monkeypatch, **opts):
    """oracle.decode_oracle.decode on the first ``n_windows`` windows, with the encoder output the fixture already holds."""
    from oracle import decode_oracle as do
    net, sd, dims, mel3, xa = pair
    monkeypatch.setattr(do.mo, "encoder_forward", lambda sd_, dims_, m: xa[: m.shape[0]])
    return do.decode(sd, dims, mel3[:n_windows], do.Options(**opts))


def _same(got, want, what):  # the bounds of tests/test_gpu_decode_parity.py
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g.tokens == w.tokens, f"{what} row {b}: native {g.tokens} vs oracle {w.tokens}"
        assert abs(g.avg_logprob - w.avg_logprob) < 2e-4, (what, b, g.avg_logprob, w.avg_logprob)
        assert abs(g.no_speech_prob - w.no_speech_prob) < 1e-5 + 1e-3 * w.no_speech_prob


def _identical(got, want, what):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g.tokens == w.tokens and g.avg_logprob == w.avg_logprob and g.no_speech_prob == w.no_speech_prob, \
            (what, b, g.tokens, w.tokens, g.avg_logprob, w.avg_logprob)


@pytest.mark.parametrize("without_timestamps", [False, True])
@pytest.mark.parametrize("beam,patience", [(3, None), (2, 2.0), (4, 0.5)])
def test_decode_native_equals_host_and_oracle(pair, monkeypatch, beam, patience, without_timestamps):
    from olmoasr_amd.decoding import DecodingOptions, decode
    net, sd, dims, mel3, _ = pair
    opts = dict(sample_len=6, beam_size=beam, patience=patience, without_timestamps=without_timestamps)
    want = _oracle(pair, 3, monkeypatch, **opts)
    for n_windows in (3, 1):
        mel = mel3[:n_windows].to(DEV)
        for cache in (True, False):
            host = decode(net, mel, DecodingOptions(use_kv_cache=cache, beam_backend="host", **opts))
            native = decode(net, mel, DecodingOptions(use_kv_cache=cache, beam_backend="native", **opts))
            what = f"beam {beam} patience {patience} windows {n_windows} cache {cache}"
            _identical(native, host, what)
            _same(native, want[:n_windows], what)  # (windows decode independently: the oracle's first rows are the 1-window answer)


def test_decode_native_length_penalty_and_single_window_form(pair, monkeypatch):
    from olmoasr_amd.decoding import DecodingOptions, decode
    net, sd, dims, mel3, _ = pair
    opts = dict(sample_len=5, beam_size=3, without_timestamps=True, length_penalty=0.6)
    want = _oracle(pair, 3, monkeypatch, **opts)
    host = decode(net, mel3.to(DEV), DecodingOptions(**opts))
    native = decode(net, mel3.to(DEV), DecodingOptions(beam_backend="native", **opts))
    _identical(native, host, "length penalty")
    _same(native, want, "length penalty")
    one = decode(net, mel3[0].to(DEV), beam_backend="native", **opts)  # [80, 3000] -> one result, options through keywords
    assert one.tokens == native[0].tokens and one.avg_logprob == native[0].avg_logprob


def _restricted_mask(bias):
    from olmoasr_amd.decoding import EOT
    mask = torch.full((51864,), -float("inf"))
    mask[KEEP] = 0.0
    mask[EOT] = bias
    return mask


def _count_calls(monkeypatch, name):
    from olmoasr_amd import ops
    calls, inner = [], getattr(ops, name)

    def counted(*args, **kwargs):
        calls.append(1)
        return inner(*args, **kwargs)
    monkeypatch.setattr(ops, name, counted)
    return calls


EOT_BIAS = 6.0       # with it, on this model, two of the three windows fill their pool before step 16 and one runs to the limit (asserted below)
EOT_BIAS_HALF = 5.5  # patience 0.5: the first window's pool of 2 fills at step 14 of 16, between two polls (asserted below)


def test_restricted_vocabulary_fills_the_pools(pair, monkeypatch):
    """Five text tokens and eot survive the masks, eot with a finite bias: at least K = 4 survivors at every step, so no step is short, and
    sequences really end.  One window at least finishes by eot before the limit and one at least is closed by finalize."""
    from olmoasr_amd.decoding import DecodingOptions, decode
    net, sd, dims, mel3, _ = pair
    opts = dict(sample_len=16, beam_size=3, without_timestamps=True, suppress_mask=_restricted_mask(EOT_BIAS))
    steps = _count_calls(monkeypatch, "topk_tokens")
    per_window = []
    for w in range(3):  # how many steps each window takes alone on the host backend: fewer than 16 = its pool filled
        del steps[:]
        decode(net, mel3[w].to(DEV), DecodingOptions(**opts))
        per_window.append(len(steps))
    print("steps per window:", per_window)
    assert min(per_window) < 16, "no window finishes by eot before the limit: the case has degenerated"
    assert max(per_window) == 16, "no window is closed by finalize: the case has degenerated"
    host = decode(net, mel3.to(DEV), DecodingOptions(**opts))
    native = decode(net, mel3.to(DEV), DecodingOptions(beam_backend="native", **opts))
    _identical(native, host, "restricted vocabulary")
    assert all(set(r.tokens) <= set(KEEP) for r in host)
    want = _oracle(pair, 3, monkeypatch, sample_len=16, beam_size=3, without_timestamps=True, logit_bias=_restricted_mask(EOT_BIAS))
    _same(native, want, "restricted vocabulary")
    for cache in (True, False):
        _identical(decode(net, mel3.to(DEV), DecodingOptions(beam_backend="native", use_kv_cache=cache, **opts)), host, f"cache {cache}")


def test_patience_below_one_completes_between_two_polls(pair, monkeypatch):
    """patience 0.5 (a pool of 2 for 4 beams; finalize closes live beams too): the host path stops at the step that fills the pool, the
    native loop at its next poll -- the latch keeps the live beams of the completing step through the surplus steps."""
    from olmoasr_amd.decoding import DecodingOptions, decode
    net, sd, dims, mel3, _ = pair
    opts = dict(sample_len=16, beam_size=4, patience=0.5, without_timestamps=True, suppress_mask=_restricted_mask(EOT_BIAS_HALF))
    steps = _count_calls(monkeypatch, "topk_tokens")
    host = decode(net, mel3[:1].to(DEV), DecodingOptions(**opts))
    host_steps = len(steps)
    del steps[:]
    native = decode(net, mel3[:1].to(DEV), DecodingOptions(beam_backend="native", **opts))
    native_steps = len(steps)
    print("host steps", host_steps, "native steps", native_steps)
    assert host_steps < 16 and host_steps % 8 != 0, "completion must fall on a step that is no multiple of 8"
    assert native_steps == min(16, (host_steps + 7) // 8 * 8) > host_steps
    _identical(native, host, "patience 0.5")
    want = _oracle(pair, 1, monkeypatch, sample_len=16, beam_size=4, patience=0.5, without_timestamps=True, logit_bias=_restricted_mask(EOT_BIAS_HALF))
    _same(native, want, "patience 0.5")


# ---- options and pass-through ---------------------------------------------------------------------------------------------------------------
def test_beam_backend_option(pair):
    from olmoasr_amd.decoding import DecodingOptions, decode
    net, sd, dims, mel3, _ = pair
    assert DecodingOptions().beam_backend == "host"
    with pytest.raises(ValueError, match="beam_backend"):
        decode(net, mel3[:1].to(DEV), DecodingOptions(sample_len=2, beam_size=3, beam_backend="bogus"))
    # ignored without beam_size
    a = decode(net, mel3[:1].to(DEV), DecodingOptions(sample_len=3, without_timestamps=True, beam_backend="native"))
    b = decode(net, mel3[:1].to(DEV), DecodingOptions(sample_len=3, without_timestamps=True))
    _identical(a, b, "greedy")


def test_transcribe_passes_beam_backend_through(pair):
    from oracle import model_oracle as mo
    net, sd, dims, mel3, _ = pair
    pcm = mo.synthetic_sample(300)[0]
    kw = dict(logprob_threshold=None, no_speech_threshold=None, sample_len=6, beam_size=3)
    host = net.transcribe(pcm, temperature=0.0, beam_backend="host", **kw)
    native = net.transcribe(pcm, temperature=0.0, beam_backend="native", **kw)
    assert host["segments"] and [s["tokens"] for s in native["segments"]] == [s["tokens"] for s in host["segments"]]
    assert [(s["seek"], s["start"], s["end"], s["avg_logprob"]) for s in native["segments"]] == \
        [(s["seek"], s["start"], s["end"], s["avg_logprob"]) for s in host["segments"]]
    with pytest.raises(ValueError, match="beam_backend"):
        net.transcribe(pcm, temperature=0.0, beam_backend="bogus", **kw)
    # temperature fallback: every avg_logprob is below 0, so the beam pass at t = 0 is followed by a sampling pass at t = 0.4, where
    # beam_size is dropped and beam_backend rides along unused
    kw["logprob_threshold"] = 0.0
    fb_host = net.transcribe(pcm, temperature=(0.0, 0.4), beam_backend="host", **kw)
    fb_native = net.transcribe(pcm, temperature=(0.0, 0.4), beam_backend="native", **kw)
    assert [s["tokens"] for s in fb_native["segments"]] == [s["tokens"] for s in fb_host["segments"]]
    assert all(s["temperature"] == 0.4 for s in fb_native["segments"])
