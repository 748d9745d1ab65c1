"""Planted cases for csrc/score.hip beyond the cross-entropy rows of tests/vocab_planted.py: argmax rows (where a tie, the last column or the
padding can fool a one-pass argmax that shares its registers with the softmax statistics) and per-sample reduce cases (which rows count, the
order and the rounding of the sum).  Plain torch / numpy on the CPU; the expectations are computed here, once per case.

``score_rows_kernel`` runs 1024 threads; a bf16 thread t owns the 16-byte pieces t, t + 1024, ... (8 columns each: chunk c of thread t covers
columns 8 (t + 1024 c) .. + 7), an fp32 thread pieces of 4 columns; wave w = t // 64; the column-by-column path gives thread t the columns
t, t + 1024, ...  The planted columns below are taken modulo V, so every shape gets every row."""
import functools

import numpy as np
import torch

NINF = -float("inf")
POISON = 1.0e30  # columns [V, ld): larger than every logit
ARGMAX_SHAPES = ((51865, 51968), (57337, 57344), (8193, 8200), (9, 1024), (5, 8), (1, 8))
REDUCE_S = (1, 63, 64, 448)
IGNORE = 51864


@functools.lru_cache(maxsize=None)
def argmax_case(V, ld):
    """dict(x f32 [rows, ld] of bf16-representable values with POISON in [V, ld), want int64 [rows], labels)."""
    g = torch.Generator().manual_seed(V)
    rows, want, labels = [], [], []

    def flat(base, planted):
        r = torch.full((V,), float(base))
        for c, v in planted.items():
            r[c % V] = v
        return r

    def add(label, r, w=None):
        rows.append(r)
        want.append(int(torch.argmax(r)) if w is None else w % V)
        labels.append(label)

    ties = {"one piece": (8, 9), "two threads": (16, 8), "two waves": (8 * 64 * 3 + 1, 8 * 64 * 9), "two chunks": (8 * 1024 * 2 + 40, 40),
            "fp32 pieces": (4, 7), "thread 1023 and 0": (8 * 1023, 8 * 1024), "last column and first": (V - 1, 0),
            "three": (V - 1, 30001, 7)}
    for name, cols in ties.items():
        add(f"equal maxima: {name} {cols}", flat(-1.0, {c: 6.0 for c in cols}), min(c % V for c in cols))
    add("maximum at V - 1", flat(0.5, {V - 1: 3.0}), V - 1)
    add("maximum at V - 2 over a random row", torch.randn(V, generator=g).to(torch.bfloat16).float().index_fill_(0, torch.tensor([max(V - 2, 0)]), 40.0),
        max(V - 2, 0))
    add("all equal", torch.full((V,), 0.25), 0)
    add("all -inf", torch.full((V,), NINF), 0)
    add("-inf except one", flat(NINF, {V // 2: -7.0}), V // 2)
    add("negative row, maximum -2.5", flat(-3.0, {12345: -2.5}), 12345)
    add("random", torch.randn(V, generator=g).to(torch.bfloat16).float())
    x = torch.full((len(rows), ld), POISON)
    x[:, :V] = torch.stack(rows)
    w = torch.tensor(want, dtype=torch.int64)
    assert torch.equal(w, torch.argmax(x[:, :V], dim=1)), "torch.argmax returns the lowest index among equal maxima"
    return dict(V=V, ld=ld, x=x, want=w, labels=labels)


def reduce_expect(row_nll, pred, targets, span, V, ignore):
    """The rule of include/oasr.h at oasr_score_reduce in numpy: (nll_sum f32, nll_max f32, n_tok i32, n_hit i32), the sum a SEQUENTIAL float64
    cumsum of the counted rows rounded once."""
    nll, pred, tgt, span = (np.asarray(t) for t in (row_nll, pred, targets, span))
    B, S = nll.shape
    out = (np.zeros(B, np.float32), np.zeros(B, np.float32), np.zeros(B, np.int32), np.zeros(B, np.int32))
    for b in range(B):
        n = min(max(int(span[b]), 0), S)
        t = tgt[b, :n]
        counted = (t != ignore) & (t >= 0) & (t < V)
        vals = nll[b, :n][counted].astype(np.float64)
        if vals.size:
            out[0][b] = np.float32(np.cumsum(vals)[-1])
            out[1][b] = vals.max()
        out[2][b] = int(counted.sum())
        out[3][b] = int((pred[b, :n][counted] == t[counted]).sum())
    return tuple(torch.from_numpy(o) for o in out)


@functools.lru_cache(maxsize=None)
def reduce_case(S, V=51865, ignore=IGNORE):
    """B = 6 samples of S rows: span 0, the planted sample (span S), a span past S, a random span, a sample whose targets are all ignored or
    out of range (no valid target), a full random one.  Magnitudes are spread over 12 binades so that a float32 running sum (or a tree sum)
    rounds differently from the sequential double sum.  The planted sample starts 2^24, 1, 1 where S >= 3: float32 accumulation stays at 2^24,
    the double sum rounds to 2^24 + 2."""
    g = torch.Generator().manual_seed(1000 + S)
    B = 6
    nll = torch.ldexp(torch.randint(0, 1 << 20, (B, S), generator=g).float(), torch.randint(-17, -5, (B, S), generator=g))
    kind = torch.randint(0, 8, (B, S), generator=g)
    tgt = torch.randint(0, V, (B, S), generator=g)
    tgt = torch.where(kind == 0, torch.full_like(tgt, ignore), tgt)
    tgt = torch.where(kind == 1, torch.full_like(tgt, V + 2), tgt)
    tgt = torch.where(kind == 2, torch.full_like(tgt, -1), tgt)
    pred = torch.where(torch.rand(B, S, generator=g) < 0.5, tgt, torch.randint(0, V, (B, S), generator=g)).to(torch.int32)
    span = torch.tensor([0, S, S + 5, int(torch.randint(0, S + 1, (1,), generator=g)), S, S], dtype=torch.int32)
    tgt[4] = torch.where(torch.arange(S) % 2 == 0, torch.full((S,), ignore), torch.full((S,), V))  # no valid target
    planted = S >= 3
    if planted:
        nll[1, :3] = torch.tensor([16777216.0, 1.0, 1.0])
        tgt[1, :3] = 3
    want = reduce_expect(nll, pred, tgt, span, V, ignore)
    if planted:  # the plant is what it claims: sequential float32 and double sums of the sample differ
        c = ((tgt[1] != ignore) & (tgt[1] >= 0) & (tgt[1] < V)).numpy()
        f32 = np.float32(0)
        for v in nll[1].numpy()[c]:
            f32 = np.float32(f32 + v)
        assert f32 != want[0][1].numpy(), "planted sample: float32 and double accumulation agree"
    return dict(S=S, V=V, ignore=ignore, row_nll=nll, pred=pred, targets=tgt, span=span, want=want, planted=planted)
