"""Planted rows for the kernels of csrc/loss.hip and csrc/select.hip (and the fp32 cross-entropy of csrc/fp32ref.hip): case builders, float64 expectations, the
check functions the GPU suite applies, and stand-ins for the kernels with one deliberate flaw at a time (plain torch, no GPU needed).

Seeded Gaussian rows at the full vocabulary say little about where these kernels can go wrong: which thread, register slot and wave owns a
column, the chunk that straddles V, the columns past V, ids outside [0, V), ties, empty rows, decision edges.  Every case here plants a
value at such a place, so a kernel that mishandles it gives a visibly different answer.

Cross-entropy (``ce_case(name)``, names in ``CE_CASES``): a case is a dict of ``logits`` bf16 [rows, ld] (columns [V, ld) hold NaN 0x7FC0 in even rows and bf16(3e38) in
odd rows: the header promises only that the first V entries are valid), ``targets``, ``ignore``, ``V``, ``ld``, ``x`` (the planted values,
float64 [rows, V], each exactly representable in bf16) and the float64 expectation of the plain objective (``row_loss``, ``loss``, ``grad``,
``lse``, ``p``); ``ce_expect(case, eps, z)`` gives the expectation for label smoothing eps and z-loss z (the formulae:
tests/test_gpu_loss_regularisers.py).  gscale = 1024, at most 64 rows per case.  ``ce_kernel`` runs 1024 threads x 7 register slots x 8
columns: thread t, slot c own columns 8 (t + 1024 c) .. + 7, wave w = t // 64, and 16 wave results are combined through LDS.

Selection (``sel_cases(V)``, ``cdf_cases()``): ``logits`` fp32 [rows, ld = V + 103], the pad +inf in even rows and NaN in odd rows; the kernels get the view
[:, :V].  ``rules`` is None (masks only) or the history the timestamp rules are evaluated from.  The expectation is the float64 row after
the rules (``decoding._timestamp_rules`` gives the rule mask; the "timestamp mass beats every text token" decision is taken in float64 on
the planted values), ordered by (value descending, id ascending).

``check_*`` return the names of the checks that failed; ``emulate_ce`` / ``emulate_sel`` follow the kernels' ownership schedules in
float32 torch and take ``flaw=`` (``CE_FLAWS`` / ``SEL_FLAWS``).  tests/test_vocab_planted_cpu.py shows that the checks pass on the
unflawed stand-ins and that each flaw fails a named case.
"""
import contextlib
import functools
import math

import torch

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
I64 = torch.int64
NINF = -float("inf")
GSCALE = 1024.0
REG = (0.1, 1e-2)  # (label smoothing eps, z-loss z) of the regularised runs
BIG = 3.0e38
V_HEAD, LD_HEAD = 51865, 51968
CE_THREADS, CE_CHUNKS = 1024, 7
CE_SHAPES = ((51865, 51968), (51864, 51968), (57344, 57344), (57337, 57344), (8193, 8200), (9, 1024), (8, 8), (5, 8), (1, 8))
SEL_PAD = 103
SEL_V = (51865, 51864, 1, 255, 256, 257, 300, 1000)

CE_FLAWS = ("slot6", "max_wave", "sum_wave", "pad_kept", "straddle_gt", "onehot_off", "trunc", "count_oor", "no_max")
SEL_FLAWS = ("stop_256", "to_ld", "tie_high", "wave_drop", "per_floor", "le_run", "force_ge", "nots_alive", "empty_nan")


# ================================================ cross-entropy ======================================================================
def _bf(x):
    return x.to(BF).to(F64)


def _poison(t, V, even, odd):
    if t.shape[1] > V:
        t[0::2, V:] = even
        t[1::2, V:] = odd
    return t


def ce_expect(case, eps=0.0, z=0.0):
    """float64 expectation of a case under (eps, z); computed once per (case, eps, z)."""
    cache = case.setdefault("_expect", {})
    if (eps, z) not in cache:
        x, V, t = case["x"], case["V"], case["targets"]
        valid = (t != case["ignore"]) & (t >= 0) & (t < V)
        n = int(valid.sum())
        rows = x.shape[0]
        lse = torch.logsumexp(x, -1)
        p = torch.exp(x - lse[:, None])
        tt = torch.where(valid, t, torch.zeros_like(t))
        xt = x.gather(1, tt[:, None])[:, 0]
        row = lse - (1 - eps) * xt - eps / V * x.sum(-1) + z * lse ** 2
        row = torch.where(valid, row, torch.zeros_like(row))
        g = GSCALE / max(1, n)
        grad = g * ((1 + 2 * z * lse[:, None]) * p - eps / V)
        grad[torch.arange(rows), tt] -= g * (1 - eps)
        grad[~valid] = 0.0
        cache[(eps, z)] = dict(row_loss=row, loss=float(row.sum() / max(1, n)), grad=grad, lse=lse, p=p, valid=valid, n_valid=n, g=g,
                               xmax=x.max(-1).values, xt=xt)
    return cache[(eps, z)]


def _ce_case(name, x, V, ld, targets, ignore, labels):
    x = x.to(F64)
    rows = x.shape[0]
    assert rows <= 64 and x.shape[1] == V and V <= ld and ld % 8 == 0 and ld <= CE_THREADS * CE_CHUNKS * 8 and len(labels) == rows
    logits = torch.zeros(rows, ld, dtype=BF)
    logits[:, :V] = x.to(BF)
    if ld > V:
        logits.view(torch.int16)[0::2, V:] = 0x7FC0
        logits[1::2, V:] = BIG
    case = dict(name=name, logits=logits, targets=torch.as_tensor(targets, dtype=I64), ignore=ignore, V=V, ld=ld, x=x, labels=labels)
    e = ce_expect(case)
    case.update({k: e[k] for k in ("row_loss", "loss", "grad", "lse", "p")})
    return case


def ce_f32_logits(case, padded):
    """The same planted values as fp32 logits, with the poisoned pad (``padded``) or ld == V."""
    V = case["V"]
    ld = case["ld"] if padded else V
    lg = torch.zeros(case["x"].shape[0], ld, dtype=F32)
    lg[:, :V] = case["x"].to(F32)
    return _poison(lg, V, float("nan"), BIG)


def needle_columns(V=V_HEAD):
    cols = {0, 7, 8, 8191, 8192, 49152, 8 * (V // 8), V - 2, V - 1} | {512 * k for k in range(1, 16)} | {8192 * c for c in range(2, 6)}
    return sorted(c for c in cols if 0 <= c < V)


def _peaked_base(V, g, half_steps=False):
    b = torch.randn(V, generator=g, dtype=F64) * 2.5
    b = (torch.round(b * 2) / 2).clamp(-8, 8) if half_steps else _bf(b)
    return b - b.max() if half_steps else _bf(b - b.max())


PEAK_MARGINS = (4, 8, 16, 24, 40, 88, 120)


def _build_needle():
    V, ld = V_HEAD, LD_HEAD
    rows, tg, lab = [], [], []
    for c in needle_columns(V):
        for t in (c, 3):
            r = torch.full((V,), -2.0, dtype=F64)
            r[c] = 8.0
            rows.append(r)
            tg.append(t)
            lab.append(f"needle@{c} target@{t}")
    return _ce_case("needle", torch.stack(rows), V, ld, tg, -100, lab)


def _build_peaked():
    V, ld = V_HEAD, LD_HEAD
    g = torch.Generator().manual_seed(11)
    rows, tg, lab = [], [], []
    for i, m in enumerate(PEAK_MARGINS):
        base = _peaked_base(V, g)
        peak = (7001 * (i + 1) + 5) % V  # spread over the register slots
        base[peak] = float(m)
        for t in (peak, (peak + 1000) % V):
            rows.append(base)
            tg.append(t)
            lab.append(f"margin {m} peak@{peak} target@{t}")
    return _ce_case("peaked", torch.stack(rows), V, ld, tg, -100, lab)


def _build_wave_peaks():
    """Not in the issue's list: flat 0.0 rows with +120 in wave k of slot 0, one row per wave -- exp(120) overflows fp32, so a wave that
    misses the maximum reduction cannot hide behind a sum that is still finite (a +8 needle can)."""
    V, ld = V_HEAD, LD_HEAD
    rows, tg, lab = [], [], []
    for k in range(16):
        c = 512 * k + 8 * k + 1
        r = torch.zeros(V, dtype=F64)
        r[c] = 120.0
        rows.append(r)
        tg.append(c)
        lab.append(f"+120@{c} (wave {k})")
    return _ce_case("wave_peaks", torch.stack(rows), V, ld, tg, -100, lab)


def _build_offset():
    V, ld = V_HEAD, LD_HEAD
    g = torch.Generator().manual_seed(12)
    needle = torch.full((V,), -2.0, dtype=F64)
    needle[8191] = 8.0
    peaked = _peaked_base(V, g, half_steps=True)
    peaked[20011] = 8.0
    rows, tg, lab = [], [], []
    for nm, r, c in (("needle", needle, 8191), ("peaked", peaked, 20011)):
        for off in (64.0, -64.0):
            for t in (c, 3):
                rows.append(r + off)
                tg.append(t)
                lab.append(f"{nm} {off:+.0f} target@{t}")
    return _ce_case("offset", torch.stack(rows), V, ld, tg, -100, lab)


def _build_shapes(V, ld, k):
    g = torch.Generator().manual_seed(100 + k)
    rows = 16
    off = torch.linspace(-30, 30, rows, dtype=F64)[torch.randperm(rows, generator=g)][:, None]
    x = _bf(torch.randn(rows, V, generator=g, dtype=F64) * 2.5 + off)
    ignore = -100
    m8 = 8 * ((V - 1) // 8)
    planted = [0, V - 1, V - 2, m8, m8 - 1, None, V // 2, V // 3, 7, 8, 1, V - 3]  # None: the row's argmax
    oor = [t for t in (V, ld - 1, -1, 2 ** 40) if t < 0 or t >= V]
    tg, lab, j = [], [], 0
    for r in range(rows):
        if r % 4 == 3:
            tg.append(ignore)
            lab.append("ignored")
        elif r in (5, 10):
            tg.append(oor[(k + r) % len(oor)])
            lab.append(f"out of range {tg[-1]}")
        else:
            t = planted[j % len(planted)]
            j += 1
            t = int(x[r].argmax()) if t is None else min(max(t, 0), V - 1)
            tg.append(t)
            lab.append(f"target@{t}")
    return _ce_case(f"shapes-{V}x{ld}", x, V, ld, tg, ignore, lab)


def _build_all_ignored():
    V, ld = V_HEAD, LD_HEAD
    g = torch.Generator().manual_seed(13)
    x = _bf(torch.randn(8, V, generator=g, dtype=F64) * 2.5)
    ignore = V - 1  # the training layout's pad id: inside [0, V)
    tg = [ignore, V, ignore, ld - 1, -1, ignore, 2 ** 40, ignore]
    return _ce_case("all_ignored", x, V, ld, tg, ignore, [f"target {t}" for t in tg])


@functools.lru_cache(maxsize=None)
def ce_case(name):
    if name.startswith("shapes-"):
        V, ld = (int(v) for v in name[7:].split("x"))
        return _build_shapes(V, ld, CE_SHAPES.index((V, ld)))
    return {"needle": _build_needle, "peaked": _build_peaked, "wave_peaks": _build_wave_peaks, "offset": _build_offset,
            "all_ignored": _build_all_ignored}[name]()


CE_CASES = ("needle", "peaked", "wave_peaks", "offset", "all_ignored") + tuple(f"shapes-{V}x{ld}" for V, ld in CE_SHAPES)
CE_REG_CASES = ("needle", "peaked") + tuple(f"shapes-{V}x{ld}" for V, ld in CE_SHAPES)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def check_ce(case, got, eps=0.0, z=0.0):
    """``got``: grad (the logits tensor after the run, [rows, ld], bf16 or fp32, CPU), row_loss f32 [rows], loss, n_valid; optionally
    nograd_logits / nograd_row_loss (the write_grad = 0 run) with ``logits_in`` (what that run was given).  Returns (names of the failed
    checks, figures): the bounds are the issue's, stated once here.

      row_loss   |got - want| <= 2^-21 max(1, |x_max|, |x_t|) + 1e-6 |want|; exactly 0 for ignored / out-of-range rows
      loss       within 1e-6 relative of the float64 mean of the kernel's own row_loss (loss_reduce accumulates in double), and within
                 1e-4 relative or 2^-21 absolute of the float64 loss
      gradient   |got - want| <= u 1.0001 + s_c + 2^-126; u = one bf16 ulp of want (fp32 logits: 2^-21 |want|); s_c = 2^-17 g (p_c + eps / V)
                 where p_c < 0.5, 2^-22 g where p_c >= 0.5 (the cancellation at a confident column); 2^-126 admits flush-to-zero
      rne_mean   (bf16, added here) over the columns of a case with p_c < 0.5 and |want| >= 2^-60, when there are at least 4096 of them in at
                 least 256 distinct bf16 cells [k u, (k + 1) u): the mean over the cells of the cell's mean (|got| - |want|) / u lies in
                 [-0.1, 0.1].  Round-to-nearest-even leaves 0 +- 0.29 / sqrt(cells) <= 0.02, truncation -0.5; the fp32 error of the value
                 (2^-17 relative) is 2^-9 of u.  (Per cell, because a flat row puts every column into one cell, whose one rounding error
                 says nothing.)
      pad columns and ignored rows bit-zero, n_valid, nothing non-finite."""
    e = ce_expect(case, eps, z)
    V, valid, n, g = case["V"], e["valid"], e["n_valid"], e["g"]
    fails, fig = [], {}
    grad, rl, loss = got["grad"], got["row_loss"].to(F64), float(got["loss"])
    is_bf = grad.dtype == BF
    if not (bool(torch.isfinite(rl).all()) and bool(torch.isfinite(grad.float()).all()) and math.isfinite(loss)):
        fails.append("finite")
    if int(got["n_valid"]) != n:
        fails.append("n_valid")
    # row loss
    mag = torch.maximum(torch.maximum(e["xmax"].abs(), e["xt"].abs()), torch.ones_like(e["xt"]))
    bound = 2.0 ** -21 * mag + 1e-6 * e["row_loss"].abs()
    err = (rl - e["row_loss"]).abs()
    if n and not bool((err <= bound)[valid].all()):
        fails.append("row_loss")
    fig["row_loss"] = float((err / bound)[valid].max()) if n else 0.0
    if not bool((rl[~valid] == 0).all()):
        fails.append("ignored_rows")
    # loss
    own = float(rl.sum() / max(1, n))
    if not abs(loss - own) <= 1e-6 * abs(own):
        fails.append("loss_reduce")
    if not abs(loss - e["loss"]) <= max(1e-4 * abs(e["loss"]), 2.0 ** -21):
        fails.append("loss")
    if n == 0 and loss != 0.0:
        fails.append("loss")
    # gradient
    want = e["grad"]
    gg = grad[:, :V].to(F64)
    if is_bf:
        ulp = torch.where(want == 0, torch.zeros_like(want), torch.exp2(torch.floor(torch.log2(want.abs().clamp_min(1e-300))) - 7))
    else:
        ulp = 2.0 ** -21 * want.abs()
    conf = e["p"] >= 0.5
    slack = torch.where(conf, torch.full_like(want, 2.0 ** -22 * g), 2.0 ** -17 * g * (e["p"] + eps / V)) + 2.0 ** -126
    gerr = (gg - want).abs()
    if n and not bool((gerr <= ulp * 1.0001 + slack)[valid].all()):
        fails.append("grad")
    if n:
        exc = ((gerr - ulp * 1.0001) / slack)[valid]
        cv = conf[valid]
        fig["grad_excess"] = float(exc[~cv].max()) if bool((~cv).any()) else 0.0
        fig["grad_excess_confident"] = float(exc[cv].max()) if bool(cv.any()) else 0.0
    if is_bf and n:
        sel = (~conf) & (want.abs() >= 2.0 ** -60) & valid[:, None]
        if int(sel.sum()) >= 4096:
            w, u = want.abs()[sel], ulp[sel]
            cell, inv = torch.unique(torch.floor(w / u).to(I64) + 256 * torch.log2(u).to(I64), return_inverse=True)
            if cell.numel() >= 256:
                r = (gg.abs()[sel] - w) / u
                per_cell = torch.zeros(cell.numel(), dtype=F64).scatter_add_(0, inv, r) / torch.bincount(inv, minlength=cell.numel())
                fig["rne_mean"] = float(per_cell.mean())
                if not abs(fig["rne_mean"]) <= 0.1:
                    fails.append("rne_mean")
    if bool(_bits(grad[:, V:]).any()):
        fails.append("pad_zero")
    if bool(_bits(grad[~valid]).any()):
        fails.append("ignored_rows")
    if "nograd_logits" in got:
        if not torch.equal(_bits(got["nograd_logits"]), _bits(got["logits_in"])):
            fails.append("nograd_logits")
        if not torch.equal(_bits(got["nograd_row_loss"]), _bits(got["row_loss"])):
            fails.append("nograd_row_loss")
    return sorted(set(fails)), fig


def emulate_ce(case, eps=0.0, z=0.0, flaw=None, store=BF, padded=True):
    """``ce_kernel`` in float32 torch, following its ownership schedule (chunk = col // 8, thread = chunk % 1024, slot = chunk // 1024,
    wave = thread // 64) with the formula written the plain way: exp(x - max) g / sum - onehot g.  ``store`` = fp32: the same on fp32
    logits, stored unrounded (the float32 formula the fp32 kernel is held to).  Flaws: see CE_FLAWS."""
    assert flaw is None or flaw in CE_FLAWS
    V, t, ignore = case["V"], case["targets"], case["ignore"]
    lg = case["logits"] if store == BF else ce_f32_logits(case, padded)
    rows, ld = lg.shape
    reg = eps != 0.0 or z != 0.0
    col = torch.arange(ld)
    ch = col // 8
    slot, wave = ch // CE_THREADS, (ch % CE_THREADS) // 64
    valid = (t != ignore) & (t >= 0) & (t < V)
    n = int((t != ignore).sum()) if flaw == "count_oor" else int(valid.sum())
    x = lg.to(F32).clone()
    dead = col >= V
    if flaw == "pad_kept":
        dead = torch.zeros_like(dead)
    if flaw == "straddle_gt":
        dead = col > V
    x[:, dead] = NINF
    loaded = slot != 6 if flaw == "slot6" else torch.ones(ld, dtype=torch.bool)
    x[:, ~loaded] = NINF
    in_max = loaded & (wave != 5) if flaw == "max_wave" else loaded
    in_sum = loaded & (wave != 5) if flaw == "sum_wave" else loaded
    mx = x[:, in_max].max(-1).values.clamp_min(-3.0e38) if bool(in_max.any()) else torch.full((rows,), -3.0e38)
    if flaw == "no_max":
        mx = torch.zeros(rows)
    ex = torch.exp(x - mx[:, None])
    s = ex[:, in_sum].sum(-1)
    lse = mx + torch.log(s)
    tt = torch.where(valid, t, torch.zeros_like(t))
    ar = torch.arange(rows)
    xt = lg[ar, tt].to(F32)
    nll = lse - xt
    row = nll
    g = torch.tensor(GSCALE, dtype=F32) / max(1, n)
    sg = g / s
    if reg:
        ev = torch.tensor(eps, dtype=F32) / V
        xs = torch.where(((col < V) & loaded)[None, :], x, torch.zeros(1)).sum(-1)
        row = nll + eps * xt - ev * xs + z * lse * lse
        sg = g * (1 + 2 * z * lse) / s
    grad = ex * sg[:, None]
    if reg:
        grad = grad - g * ev
        grad[:, col >= V] = 0.0
    tcol = (tt + 1).clamp_max(ld - 1) if flaw == "onehot_off" else tt
    grad[ar, tcol] -= g * (1 - eps) if reg else g
    if store == BF:
        out = (grad.view(torch.int32) & -65536).view(F32).to(BF) if flaw == "trunc" else grad.to(BF)
    else:
        out = grad
    out[:, ~loaded] = lg[:, ~loaded]
    out[~valid] = 0
    row = torch.where(valid, row, torch.zeros_like(row))
    loss = (row.to(F64).sum() / max(1, n)).to(F32)
    return dict(grad=out, row_loss=row, loss=loss, n_valid=n)


# ================================================ selection ==========================================================================
def sel_ids(V):
    """The real ids at the model's head, scaled ones elsewhere (None for V < 12: rule-free modes only)."""
    if V in (51865, 51864):
        from olmoasr_amd import decoding as D
        return dict(timestamp_begin=D.TIMESTAMP_BEGIN, eot=D.EOT, no_timestamps=D.NO_TIMESTAMPS)
    if V < 12:
        return None
    return dict(timestamp_begin=V // 2 + 4, eot=V // 2, no_timestamps=V // 2 + 2)


@contextlib.contextmanager
def _decoding_ids(ids):
    from olmoasr_amd import decoding as D
    old = (D.TIMESTAMP_BEGIN, D.EOT, D.NO_TIMESTAMPS)
    D.TIMESTAMP_BEGIN, D.EOT, D.NO_TIMESTAMPS = ids["timestamp_begin"], ids["eot"], ids["no_timestamps"]
    try:
        yield D
    finally:
        D.TIMESTAMP_BEGIN, D.EOT, D.NO_TIMESTAMPS = old


def _sel_case(name, V, x, labels, rules=None, mask=None, **extra):
    """rules: None, or dict(history int64 [rows, H], n_history, max_initial_index)."""
    x = torch.stack(x) if isinstance(x, (list, tuple)) else x
    x = x.to(F64)
    rows = x.shape[0]
    assert x.shape[1] == V and len(labels) == rows
    ld = V + SEL_PAD
    lg = torch.zeros(rows, ld, dtype=F32)
    lg[:, :V] = x.to(F32)
    _poison(lg, V, float("inf"), float("nan"))
    ids = sel_ids(V)
    assert rules is None or ids is not None
    return dict(name=f"{name}-V{V}-{'rules' if rules else 'plain'}", kind=name, V=V, ld=ld, logits=lg, x=x, labels=labels, rules=rules, mask=mask,
                ids=ids, **extra)


def sel_rule_mask(case):
    """bool [rows, V]: the columns ``decoding._timestamp_rules`` masks before its last step (they do not depend on the values): the module's
    own function on a row whose text columns sit far above the timestamp mass, so its last step removes nothing more."""
    rows, V = case["x"].shape
    r = case["rules"]
    if r is None:
        return torch.zeros(rows, V, dtype=torch.bool)
    with _decoding_ids(case["ids"]) as D:
        probe = torch.zeros(rows, V, dtype=F64)
        probe[:, :case["ids"]["timestamp_begin"]] = 1000.0
        D._timestamp_rules(probe, r["history"][:, :r["n_history"]], 0, r["max_initial_index"])
    return torch.isinf(probe)


def sel_filtered(case):
    """float64 [rows, V]: the row the kernels pick from (-inf = not a survivor), the force rule decided in float64."""
    if "_filtered" not in case:
        f = case["x"].clone()
        if case["mask"] is not None:
            f = f + case["mask"].to(F64)[None, :]
        f[sel_rule_mask(case)] = NINF
        f[~(f > NINF)] = NINF
        if case["rules"] is not None:
            tb = case["ids"]["timestamp_begin"]
            stamp, text = torch.logsumexp(f[:, tb:], -1), f[:, :tb].max(-1).values
            case["_force_margin"] = stamp - text
            force = (stamp > NINF) & ((text == NINF) | (stamp > text))
            f[:, :tb] = torch.where(force[:, None], torch.full_like(f[:, :tb], NINF), f[:, :tb])
        case["_filtered"] = f
    return case["_filtered"]


def sel_expect_topk(case, K):
    """(ids int64 [rows, K], lp float64 [rows, K]) by a stable sort on (value descending, id ascending); past the survivors (0, -inf)."""
    f = sel_filtered(case)
    if "_order" not in case:
        case["_order"] = torch.sort(-f, dim=-1, stable=True).indices[:, :16]
    order = case["_order"][:, :K]
    val = f.gather(1, order)
    lse = torch.logsumexp(f, -1)
    alive = val > NINF
    lp = torch.where(alive, val - lse[:, None], torch.full_like(val, NINF))
    return torch.where(alive, order, torch.zeros_like(order)), lp


def _lp_fails(got, want):
    got, want = got.to(F64).reshape(-1), want.reshape(-1)
    dead = want == NINF
    ok = torch.where(dead, got == NINF, (got - want).abs() <= torch.where(want.abs() <= 1e-12, 1e-6, 2e-4))
    return [] if bool(ok.all()) else ["lp"]


def check_topk(case, K, tok, lp):
    """ids exact (ties by ascending id), below V and survivors; log-probabilities within 2e-4 (1e-6 where the expectation is 0), -inf exactly
    where there is no survivor.  ``pick`` is K = 1."""
    want_tok, want_lp = sel_expect_topk(case, K)
    tok = tok.reshape(want_tok.shape).to(I64)
    fails = []
    if not bool(((tok >= 0) & (tok < case["V"])).all()):
        fails.append("id_range")
    elif not bool(((sel_filtered(case).gather(1, tok) > NINF) | (want_lp == NINF)).all()):
        fails.append("dead_id")
    if not torch.equal(tok, want_tok):
        fails.append("ids")
    return sorted(set(fails + _lp_fails(lp, want_lp)))


def check_pick(case, tok, lp):
    return check_topk(case, 1, tok, lp)


def sel_expect_draw(case, T, u):
    """The inverse-CDF draw in float64: the first survivor whose cumulative mass exceeds u total (the last survivor when none does)."""
    f = sel_filtered(case)
    m = torch.exp((f - f.max(-1, keepdim=True).values.clamp_min(-1e300)) / T)
    m = torch.where(f > NINF, m, torch.zeros_like(m))
    cum = torch.cumsum(m, -1)
    hit = cum > (u.to(F64) * cum[:, -1])[:, None]
    first = hit.int().argmax(-1)
    last = (m > 0).int().cumsum(-1).argmax(-1)
    return torch.where(hit.any(-1), first, last), m, cum


def check_sample(case, T, u, tok, lp, exact):
    """A draw is below V, a survivor, and sits where the inverse CDF puts it: ``exact`` (the cdf_exact rows, all masses 1.0) the float64 draw
    itself; otherwise cum_before(tok) - tol <= u total <= cum_through(tok) + tol with tol = 1e-5 total (fp32 masses summed in another
    order).  ``winner_always`` rows (T <= 1): the planted winner for every u.  lp: the draw's log_softmax at temperature 1."""
    f = sel_filtered(case)
    V = case["V"]
    tok = tok.to(I64).reshape(-1)
    empty = ~(f > NINF).any(-1)
    fails = []
    if not bool(((tok >= 0) & (tok < V)).all()):
        return ["id_range"]
    ft = f.gather(1, tok[:, None])[:, 0]
    if not bool(((ft > NINF) | empty).all()):
        fails.append("dead_id")
    want, m, cum = sel_expect_draw(case, T, u)
    if exact:
        if not torch.equal(torch.where(empty, torch.zeros_like(want), want), tok):
            fails.append("ids")
    else:
        total = cum[:, -1]
        target, tol = u.to(F64) * total, 1e-5 * total
        through = cum.gather(1, tok[:, None])[:, 0]
        before = through - m.gather(1, tok[:, None])[:, 0]
        if not bool((((before - tol <= target) & (target <= through + tol)) | empty).all()):
            fails.append("cdf")
        if not bool((tok[empty] == 0).all()):
            fails.append("ids")
    for r, c in case.get("winner_always", {}).items() if T <= 1.0 else ():  # (T = 2: exp(-100) is still a mass in fp32)
        if int(tok[r]) != c:
            fails.append("ids")
    lse = torch.logsumexp(f, -1)
    want_lp = torch.where(empty | ~(ft > NINF), torch.full_like(lse, NINF), ft - lse)
    return sorted(set(fails + _lp_fails(lp, want_lp)))


# ---- builders -----------------------------------------------------------------------------------------------------------------------
def _per(V):
    return (V + 255) // 256


def _neutral_rules(rows, V):
    """Rules on with one text token sampled: only <|notimestamps|> and the force rule act."""
    return dict(history=torch.full((rows, 1), 3, dtype=I64), n_history=1, max_initial_index=None)


def sel_needle_columns(V):
    ids, per = sel_ids(V), _per(V)
    cols = {0, 255, 256, V - 256, V - 1}
    if ids:
        cols |= {ids["timestamp_begin"] - 1, ids["timestamp_begin"], ids["eot"], ids["no_timestamps"]}
    for t in (0, 1, 254, 255):
        if t * per < V:
            cols |= {t * per, min(V, (t + 1) * per) - 1}
    return sorted(c for c in cols if 0 <= c < V)


def _flat_with(V, base, planted):
    r = torch.full((V,), float(base), dtype=F64)
    for c, v in planted.items():
        r[c] = v
    return r


def _needle(V, rules):
    cols = sel_needle_columns(V)
    x, lab = [_flat_with(V, 0.0, {c: 5.0}) for c in cols], [f"+5@{c}" for c in cols]
    if rules:  # (on a flat row the timestamp mass can take the whole text part away, <|notimestamps|> with it: one row where it cannot)
        ids = sel_ids(V)
        x.append(_flat_with(V, NINF, {ids["no_timestamps"]: 5.0, 1: 0.0, ids["timestamp_begin"] + 1: -1.0}))
        lab.append("+5@<|notimestamps|>, one text and one timestamp survivor")
    return _sel_case("needle", V, x, lab, _neutral_rules(len(x), V) if rules else None)


def _tie_sets(V):
    out = []
    for c in (0, 63, 191, V - 257):
        s = sorted({k for k in (c, c + 1, c + 64, c + 256) if 0 <= k < V})
        if c >= 0 and len(s) >= 2 and s not in out:
            out.append(s)
    return out


def _ties(V, rules):
    x, lab = [torch.zeros(V, dtype=F64)], ["all equal"]
    for s in _tie_sets(V):
        x.append(_flat_with(V, 0.0, {k: 3.0 for k in s}))
        lab.append(f"+3@{s}")
    if rules:
        ids = sel_ids(V)
        a, s = ids["timestamp_begin"] - 5, ids["timestamp_begin"] + 7
        x.append(_flat_with(V, NINF, {a: 9.0, s: 9.0, 1: 2.0}))  # one timestamp at the text maximum: not forced, the text id first
        lab.append(f"text {a} = stamp {s}, alone")
        x.append(_flat_with(V, 0.0, {a: 6.0, s: 6.0}))  # the other timestamps add mass: forced
        lab.append(f"text {a} = stamp {s}, flat rest")
    return _sel_case("ties", V, x, lab, _neutral_rules(len(x), V) if rules else None)


def _ties_masked(V, rules):
    mask = torch.zeros(V, dtype=F32)
    mask[:3] = NINF
    return _sel_case("ties_masked", V, [torch.zeros(V, dtype=F64)], ["all equal, columns 0..2 masked"], _neutral_rules(1, V) if rules else None, mask)


def _empty_and_single(V, rules):
    ids = sel_ids(V)
    singles = sorted({0, V - 1, V // 3} | ({ids["timestamp_begin"], ids["no_timestamps"], ids["eot"]} if ids else set()))
    x, lab = [torch.full((V,), NINF, dtype=F64)], ["empty"]
    for c in singles:
        x.append(_flat_with(V, NINF, {c: 1.5}))
        lab.append(f"single@{c}")
    return _sel_case("empty_and_single", V, x, lab, _neutral_rules(len(x), V) if rules else None)


def _empty_by_mask(V, rules):
    g = torch.Generator().manual_seed(V)
    x = torch.randn(2, V, generator=g, dtype=F64)
    return _sel_case("empty_by_mask", V, x.to(F32), ["masked out", "masked out"], _neutral_rules(2, V) if rules else None,
                     torch.full((V,), NINF, dtype=F32))


def _force_edge(V):
    ids = sel_ids(V)
    tb, eot = ids["timestamp_begin"], ids["eot"]
    a, b, s1, s2 = eot - 3, 2, tb + 2, min(V - 1, tb + 9)
    x = [_flat_with(V, NINF, {a: 1.0, b: 0.0, s1: 1.0}),                  # (a) equal: strict >, not forced
         _flat_with(V, NINF, {a: 1.0, b: 0.0, s1: 1.0, s2: 1.0}),         # (b) two timestamps: forced, the lower id, lp = -ln 2
         _flat_with(V, NINF, {a: 1.0, b: 0.0, s1: 1.0 + 2.0 ** -10})]      # (c) one timestamp just above: forced
    return _sel_case("force_edge", V, x, ["(a) one stamp at the text maximum", "(b) two stamps at it", "(c) one stamp 2^-10 above"],
                     _neutral_rules(3, V), want_pick=[a, s1, s1])


def _rule_edges(V):
    ids = sel_ids(V)
    tb = ids["timestamp_begin"]
    s = tb + 20
    out = []

    def case(tag, hist, mii, needles):
        x = [_flat_with(V, 0.0, {c: 5.0}) for c in needles]
        h = torch.tensor([hist] * len(x), dtype=I64).reshape(len(x), len(hist))
        out.append(_sel_case(f"rule_edges_{tag}", V, x, [f"+5@{c}" for c in needles], dict(history=h, n_history=len(hist), max_initial_index=mii)))
    case("first", [], 50, [tb + 50, tb + 51])
    case("unpaired", [3, s], None, [s, s - 1])
    case("pair", [s, s], None, [s, s + 1, 5])
    case("pair_then_text", [s, s, 3], None, [s, s + 1])
    return out


def _offsets(V, rules):
    c = min(256, V - 1)
    x, lab = [_flat_with(V, 0.0, {c: 5.0}) + 1e4], [f"+5@{c}, all +1e4"]
    ts = _tie_sets(V)
    if ts:
        x.append(_flat_with(V, 0.0, {k: 3.0 for k in ts[0]}) + 1e4)
        lab.append(f"+3@{ts[0]}, all +1e4")
    w = V // 3
    winner_row = len(x)
    x.append(_flat_with(V, 0.0, {w: 200.0}))
    lab.append(f"+200@{w}")
    r = torch.tensor([0.0, float(torch.tensor(-1e30, dtype=F32)), NINF, 1.0, 0.5], dtype=F64).repeat(V // 5 + 1)[:V].clone()
    r[V // 2 + 1 if V > 2 else 0] = 2.0
    x.append(r)
    lab.append("fp32(-1e30) and -inf among ordinary entries")
    return _sel_case("offsets", V, x, lab, _neutral_rules(len(x), V) if rules else None, winner_always={winner_row: w})


def cdf_positions(V, n):
    """n survivor columns: thread 255's (or the last non-empty thread's) partial range, then the last column of a range and the first of the
    next, with runs of empty ranges between the pairs."""
    per = _per(V)
    last_owner = (V - 1) // per
    cand = [last_owner * per - 1, last_owner * per, V - 1]
    step = max(1, min(254, last_owner) // max(1, n // 2))
    for t in list(range(1, last_owner + 1, step)) + list(range(1, last_owner + 1)):
        cand += [t * per - 1, t * per]
    pos = []
    for c in cand + list(range(V)):
        if 0 <= c < V and c not in pos:
            pos.append(c)
        if len(pos) == n:
            break
    assert len(pos) == n
    return sorted(pos)


def _cdf_exact(V, n, k):
    """One stored row under the draws u = j / n (j = 0 .. n - 1), 0 and 1 - 2^-24 (``logits`` is that row expanded, one per draw; the launchers
    want a row stride >= V, so the GPU test runs copies of ``stored`` in batches)."""
    pos = cdf_positions(V, n)
    row = _flat_with(V, NINF, {c: 0.0 for c in pos})
    u = torch.cat([torch.arange(n, dtype=F32) / n, torch.tensor([0.0, 1.0 - 2.0 ** -24], dtype=F32)])
    c = _sel_case(f"cdf_exact_n{n}", V, [row, row], ["", ""], None, u=u, survivors=pos)
    c["stored"] = c["logits"][k % 2:k % 2 + 1]  # [1, ld]: the +inf pad or the NaN pad
    c["logits"] = c["stored"].expand(u.numel(), c["ld"])
    c["x"] = c["x"][:1].expand(u.numel(), V)
    c["labels"] = [f"u={float(v):.6g}" for v in u]
    c["want_draw"] = torch.tensor(pos + [pos[0], pos[-1]], dtype=I64)
    return c


CDF_EXACT = tuple((V, n) for V in (51865, 1000, 257) for n in (2, 64, 256))
CDF_T = (0.5, 1.0, 2.0)


@functools.lru_cache(maxsize=None)
def sel_cases(V):
    """Every planted selection case at vocabulary size V (cdf_exact: ``cdf_cases``)."""
    out = []
    for rules in ((False, True) if sel_ids(V) else (False,)):
        out += [_needle(V, rules), _ties(V, rules), _ties_masked(V, rules), _empty_and_single(V, rules), _empty_by_mask(V, rules), _offsets(V, rules)]
    if sel_ids(V):
        out.append(_force_edge(V))
        if V >= 255:
            out += _rule_edges(V)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cdf_cases():
    return tuple(_cdf_exact(V, n, k) for k, (V, n) in enumerate(CDF_EXACT))


def topk_ks(V):
    return [k for k in (1, 6, 16) if k <= V]


def sample_uniforms(case):
    """The draws a general case is sampled with: seeded uniforms, all 0, all 1 - 2^-24."""
    rows = case["x"].shape[0]
    g = torch.Generator().manual_seed(rows + case["V"])
    return [torch.rand(rows, generator=g, dtype=F32), torch.zeros(rows, dtype=F32), torch.full((rows,), 1.0 - 2.0 ** -24, dtype=F32)]


def sel_failures(case, run):
    """Every applicable kernel on a case: ``run(kind, K=, T=, u=)`` -> (tok, lp) with kind "pick" (ops.pick_tokens on a rule-free case,
    ops.pick_tokens_ts on one with rules), "topk", "sample".  Returns {run: failed checks}, empty when all pass."""
    out = {"pick": check_pick(case, *run("pick"))}
    for K in topk_ks(case["V"]):
        out[f"topk K={K}"] = check_topk(case, K, *run("topk", K=K))
    for T in (1.0, 2.0):
        for i, u in enumerate(sample_uniforms(case)):
            out[f"sample T={T} u#{i}"] = check_sample(case, T, u, *run("sample", T=T, u=u), exact=False)
    return {k: v for k, v in out.items() if v}


def cdf_failures(case, run):
    out = {f"sample T={T}": check_sample(case, T, case["u"], *run("sample", T=T, u=case["u"]), exact=True) for T in CDF_T}
    return {k: v for k, v in out.items() if v}


# ---- the kernels' schedule in float32 torch ---------------------------------------------------------------------------------------------
def _emu_filtered(case, flaw, use_rules):
    """fp32 [rows, ncol] after masks and rules (no force step yet), -inf = dropped; ncol = ld when the column loop runs past V."""
    V, ld = case["V"], case["ld"]
    ncol = ld if flaw == "to_ld" else V
    x = case["logits"][:, :ncol].clone()
    if case["mask"] is not None:
        x[:, :V] += case["mask"][None, :]
    dead = torch.zeros(x.shape, dtype=torch.bool)
    if use_rules and case["rules"] is not None:
        dead[:, :V] = sel_rule_mask(case)
        if flaw == "nots_alive":
            dead[:, case["ids"]["no_timestamps"]] = False
    col = torch.arange(ncol)
    if flaw == "stop_256":
        dead[:, col >= V - V % 256] = True
    if flaw == "wave_drop":
        dead[:, (col % 256) // 64 == 2] = True
    return x, dead


def _emu_rowstat(case, flaw, pick_kernel=False):
    """filtered fp32 row with the force step applied, as pick_ts / row_stat take it (pick_kernel: no filter, NaN and +inf go through)."""
    x, dead = _emu_filtered(case, flaw, not pick_kernel)
    if pick_kernel:
        return torch.where(dead, torch.full_like(x, NINF), x)
    f = torch.where(dead | ~(x > NINF), torch.full_like(x, NINF), x)
    if case["rules"] is not None:
        tb = case["ids"]["timestamp_begin"]
        M = f.max(-1, keepdim=True).values.clamp_min(-3.0e38)  # (relative to the row maximum, as the kernels work)
        stamp, text = torch.logsumexp(f[:, tb:] - M, -1), (f[:, :tb] - M).max(-1).values
        beats = stamp >= text if flaw == "force_ge" else stamp > text
        force = (stamp > NINF) & ((text == NINF) | beats)
        f[:, :tb] = torch.where(force[:, None], torch.full_like(f[:, :tb], NINF), f[:, :tb])
    return f


def emulate_sel(case, kind, flaw=None, K=1, T=1.0, u=None):
    """kind: "pick" (pick_kernel: rule-free cases; pick_ts_kernel: cases with rules), "topk", "sample".  Returns (tok, lp) as ops does."""
    assert flaw is None or flaw in SEL_FLAWS
    f = _emu_rowstat(case, flaw, pick_kernel=(kind == "pick" and case["rules"] is None))
    rows, ncol = f.shape
    V = case["V"]
    fa = torch.where(f != f, torch.full_like(f, NINF), f)  # the comparisons drop NaN; the sum below keeps it
    M = fa.max(-1, keepdim=True).values.clamp_min(-3.0e38)
    lse = torch.logsumexp(f - M, -1)  # of x - max, as row_stat keeps it
    empty = ~(fa > NINF).any(-1)
    empty_lp = float("nan") if flaw == "empty_nan" else NINF
    if kind in ("pick", "topk"):
        key = -fa.flip(-1) if flaw == "tie_high" else -fa
        order = torch.sort(key, dim=-1, stable=True).indices[:, :K]
        order = ncol - 1 - order if flaw == "tie_high" else order
        val = fa.gather(1, order)
        alive = val > NINF
        lp = torch.where(alive, (val - M) - lse[:, None], torch.full_like(val, NINF))
        lp = torch.where(empty[:, None], torch.full_like(lp, empty_lp), lp)
        tok = torch.where(alive, order, torch.zeros_like(order))
        return (tok[:, 0], lp[:, 0]) if kind == "pick" else (tok, lp)
    per = V // 256 if flaw == "per_floor" else _per(V)
    m = torch.where(fa > NINF, torch.exp((fa - M) * (1.0 / T)), torch.zeros_like(fa))[:, :V]
    owned = torch.zeros(rows, 256 * max(per, 1), dtype=F32)
    w = min(V, 256 * per)
    owned[:, :w] = m[:, :w]  # (per = floor: the columns past 256 per belong to nobody)
    part = owned.view(rows, 256, max(per, 1)).sum(-1)
    total = part.cumsum(-1)[:, -1]
    target = (u * total)[:, None]
    cum = owned.cumsum(-1)
    hit = (owned > 0) & (target <= cum if flaw == "le_run" else target < cum)
    first = hit.int().argmax(-1)
    last = (owned > 0).int().cumsum(-1).argmax(-1)
    tok = torch.where(hit.any(-1), first, last)
    tok = torch.where(empty | ~(owned > 0).any(-1), torch.zeros_like(tok), tok)
    ft = fa.gather(1, tok[:, None])[:, 0]
    lp = torch.where(ft > NINF, (ft - M[:, 0]) - lse, torch.full_like(ft, NINF))
    lp = torch.where(empty, torch.full_like(lp, empty_lp), lp)
    return tok, lp
