"""GPU half of the native word-timestamp alignment (csrc/align.hip): ``ops.dtw`` bit for bit against ``timing.dtw``, ``ops.alignment_matrix``
against a float64 restatement within a bound taken from the torch path's own fp32 error, and ``find_alignment`` / ``transcribe`` end to end
with ``backend="native"``."""
import numpy as np
import pytest
import torch

from alignment_cases import DTW_FAMILIES, DTW_SHAPES, MATRIX_CASES, deal_out, dtw_cost, dtw_want, matrix_planes, matrix_reference

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -12345


def _paths_equal(got, want):
    return np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy(), want[1])


@pytest.mark.parametrize("family", DTW_FAMILIES)
@pytest.mark.parametrize("N,M", DTW_SHAPES)
def test_dtw_is_bit_identical_to_timing_dtw(N, M, family):
    """Path buffers and workspace pre-filled with a sentinel: the path equals timing.dtw's, the entries past its length are untouched, and a
    second call on the same (now dirty) buffers gives the same path."""
    from olmoasr_amd import _native as native
    from olmoasr_amd import ops
    x = dtw_cost(N, M, family).to(DEV)
    want = dtw_want(N, M, family)
    got = ops.dtw(x)
    assert got[0].dtype == torch.int64 and not got[0].is_cuda and _paths_equal(got, want)
    P = N + M - 1
    path = torch.full((2 * P + 1,), SENTINEL, dtype=torch.int32, device=DEV)
    ws = torch.full((native.lib().oasr_dtw_workspace_bytes(N, M),), 0xA5, dtype=torch.uint8, device=DEV)
    for _ in range(2):
        ops.dtw_device(x, path=path, workspace=ws)
        host = path.cpu().numpy()
        ln = int(host[-1])
        assert ln == len(want[0])
        assert np.array_equal(host[:ln], want[0]) and np.array_equal(host[P:P + ln], want[1])
        assert (host[ln:P] == SENTINEL).all() and (host[P + ln:2 * P] == SENTINEL).all()


@pytest.mark.parametrize("N,M,family", [(65, 63, "randn"), (5, 64, "ties"), (130, 129, "ridge"), (446, 1500, "randn"), (1, 9, "randn"), (7, 1, "ties")])
def test_dtw_negates_and_honours_the_row_stride(N, M, family):
    """negate=True on m is timing.dtw(-m); the input is the row slice [2:-1] of a wider matrix whose other entries are NaN."""
    from olmoasr_amd import ops
    x = dtw_cost(N, M, family)
    big = torch.full((N + 3, M + 5), float("nan"))
    big[2:-1, :M] = x
    view = big.to(DEV)[2:-1, :M]
    assert _paths_equal(ops.dtw(view, negate=True), dtw_want(N, M, family, True))
    assert _paths_equal(ops.dtw(view), dtw_want(N, M, family))


@pytest.mark.parametrize("case", MATRIX_CASES, ids=lambda c: "x".join(map(str, c)))
def test_alignment_matrix_against_float64(case):
    """max |native - float64| <= 8 * max(e32, 2^-24 * max |float64|), e32 = the fp32 torch path's own distance from float64 on the same
    input (the 8: another exp, another summation order over up to 1500 frames and 448 tokens).  Unselected heads and frames >= F are NaN;
    the output lies between guard rows; the native matrix gives the float64 matrix's DTW path; a second call gives the same bits."""
    from olmoasr_amd import ops
    Hsel, n, F, sc = case
    m64, e32, path64 = matrix_reference(case)
    layers, heads = deal_out(matrix_planes(*case), F)
    order = sorted(layers)
    qk = [layers[l].to(DEV) for l in order]
    hpl = [[h for ll, h in heads if ll == l] for l in order]
    guard = torch.full((n + 2, F), float(SENTINEL), device=DEV)
    got = ops.alignment_matrix(qk, hpl, F, out=guard[1:-1])
    assert got.data_ptr() == guard[1:-1].data_ptr()
    assert bool((guard[0] == SENTINEL).all()) and bool((guard[-1] == SENTINEL).all())
    m = got.cpu().numpy()
    assert np.isfinite(m).all()
    err = float(np.abs(m.astype(np.float64) - m64).max())
    floor = 2.0 ** -24 * float(np.abs(m64).max())
    print(f"case {case}: native vs float64 {err:.3e}, torch fp32 vs float64 {e32:.3e}, ratio to the bound's base {err / max(e32, floor):.2f}")
    assert err <= 8 * max(e32, floor), (err, e32, floor)
    assert _paths_equal(ops.dtw(got[2:-1], negate=True), path64)
    again = ops.alignment_matrix(qk, hpl, F)
    assert torch.equal(again, got)


def test_alignment_matrix_widths_one_and_three_and_a_generic_one():
    """medfilt_width 1 (no filter), 3 and 5 (the generic network) against the float64 restatement at that width, by the same bound."""
    from alignment_cases import matrix_float64
    from olmoasr_amd import ops, timing
    case = (6, 8, 130, 2)
    qk = matrix_planes(*case)
    layers, heads = deal_out(qk, case[2])
    order = sorted(layers)
    dev = [layers[l].to(DEV) for l in order]
    hpl = [[h for ll, h in heads if ll == l] for l in order]
    for w in (1, 3, 5):
        m64 = matrix_float64(qk, case[2], width=w)
        m32 = timing.alignment_matrix_torch({0: qk}, [(0, s) for s in range(case[0])], case[2], w, 1.0).numpy()
        e32 = float(np.abs(m32 - m64).max())
        got = ops.alignment_matrix(dev, hpl, case[2], medfilt_width=w).cpu().numpy()
        err = float(np.abs(got - m64).max())
        assert err <= 8 * max(e32, 2.0 ** -24 * float(np.abs(m64).max())), (w, err, e32)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
class WordTok:
    """Scripted tokenizer with whisper's attribute names: every text token is one word."""
    eot, sot_sequence, no_timestamps, timestamp_begin = 50256, (50257,), 50362, 50363

    def decode(self, ids):
        return "".join(f" w{int(i)}" for i in ids if i < self.eot)

    def encode(self, s):
        return [int(x[1:]) for x in s.split()]

    def split_to_word_tokens(self, tokens):
        return [f" w{t}" if t < self.eot else "<|eot|>" for t in tokens], [[t] for t in tokens]


@pytest.fixture(scope="module")
def net(tiny_case):
    from olmoasr_amd.config.model_dims import ModelDimensions
    from olmoasr_amd.model import OLMoASR
    dims = tiny_case["dims"]
    model = OLMoASR(ModelDimensions(**{k: getattr(dims, k) for k in ModelDimensions.__dataclass_fields__}), device=DEV, seed=0)
    model.load_state_dict(tiny_case["sd"])
    return model


def test_find_alignment_native_backend(net, tiny_case):
    """One WordTiming per word, the same words and tokens as the torch backend, monotone times inside the window; the window's encoder
    output given as ``audio_features`` changes nothing.  (Equal word TIMES across the backends are not asserted on a random-weight model: a
    1e-7 difference may legitimately move a tie; the planted matrices above carry that check.)"""
    from olmoasr_amd import timing
    mel = tiny_case["mel"][:1].to(DEV)
    text = [1000, 2000, 3000, 4000, 5000]
    ref = timing.find_alignment(net, WordTok(), text, mel[0], 3000, backend="torch")
    words = timing.find_alignment(net, WordTok(), text, mel[0], 3000, backend="native")
    assert [w.word for w in words] == [w.word for w in ref] == [f" w{t}" for t in text]
    assert [w.tokens for w in words] == [w.tokens for w in ref] == [[t] for t in text]
    assert [w.probability for w in words] == [w.probability for w in ref]
    times = [(w.start, w.end) for w in words]
    assert all(0.0 <= s <= e <= 30.0 for s, e in times) and all(a[1] <= b[0] + 1e-9 for a, b in zip(times, times[1:]))
    xa = net.embed_audio(mel)
    assert timing.find_alignment(net, WordTok(), text, None, 3000, backend="native", audio_features=xa) == words
    assert timing.find_alignment(net, WordTok(), text, None, 3000, backend="native", audio_features=xa[0]) == words
    assert timing.find_alignment(net, WordTok(), text, None, 3000, backend="torch", audio_features=xa) == ref
    short = timing.find_alignment(net, WordTok(), text, mel[0], 4, backend="native")  # 2 frames: the last window of a short clip, filter skipped
    assert [w.word for w in short] == [f" w{t}" for t in text] and all(0.0 <= w.start <= w.end <= 0.04 + 1e-9 for w in short)
    assert timing.find_alignment(net, WordTok(), [], mel[0], 3000, backend="native") == []
    with pytest.raises(ValueError, match="backend"):
        timing.find_alignment(net, WordTok(), text, mel[0], 3000, backend="bogus")


def test_transcribe_with_the_native_alignment_backend(net, tiny_case):
    pcm = tiny_case["pcm"][0].float() / 32768.0
    kw = dict(tokenizer=WordTok(), word_timestamps=True, temperature=0.0, logprob_threshold=None, no_speech_threshold=None,
              compression_ratio_threshold=None, sample_len=12)
    out = net.transcribe(pcm, alignment_backend="native", **kw)
    assert out["segments"]
    seen = 0
    for s in out["segments"]:
        assert "words" in s
        if any(t < WordTok.eot for t in s["tokens"]):
            assert len(s["words"]) > 0
        for w in s["words"]:
            assert set(w) == {"word", "start", "end", "probability"} and 0.0 <= w["start"] <= w["end"] <= 31.0
            seen += 1
    assert seen > 0
    # the same windows, segments, words and tokens as the torch backend (which encodes each window itself): the encoder output handed over is
    # the aligned window's own
    ref = net.transcribe(pcm, alignment_backend="torch", **kw)
    assert [(s["seek"], s["tokens"]) for s in ref["segments"]] == [(s["seek"], s["tokens"]) for s in out["segments"]]
    assert [[w["word"] for w in s["words"]] for s in ref["segments"]] == [[w["word"] for w in s["words"]] for s in out["segments"]]
    assert [[w["probability"] for w in s["words"]] for s in ref["segments"]] == [[w["probability"] for w in s["words"]] for s in out["segments"]]
    with pytest.raises(ValueError, match="backend"):
        net.transcribe(pcm, alignment_backend="bogus", **kw)
