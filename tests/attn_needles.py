"""Attention inputs with planted scores, a float64 reference and rounding-point error bounds (plain torch, no GPU needed).

Every attention test used to feed q, k ~ N(0, 1): scaled scores of ordinary size, where a leaked key carries too little weight to
show and the forward's lazy rescale never fires after the first tile.  The cases built here plant the scores instead.

Planting.  q, k, v are bf16 [B, T, H, 64] strided views laid out like the engine's (self-attention: one fused q | k | v buffer of
token stride 3 H 64; cross-attention: q [B, Tq, H 64] and a fused k | v buffer).  Channel 0 carries the planted score exactly:
q[i, 0] = 8 r_i and k[j, 0] = t_j are bf16 values, so q[i, 0] k[j, 0] / 8 = r_i t_j with no rounding anywhere (a product of two
bf16 values is exact in fp32).  Channels 1..63 carry uniform noise of amplitude aq (q) and ak (k), both powers of two, so the noise
moves any score by at most ``noise_bound = 63 aq ak / 8`` nats (``Case.noise_bound``, computed from the stored values).

Scenarios (``SCENARIOS``):
  masked   keys at masked positions dominate: without causality every key j >= kv_len[b] scores +60 nats over the real keys,
           which sit at 0 +- 2; with causality the planted score is a strictly increasing ramp over the keys (r = 128, t_j the
           j-th bf16 value above 1.0: steps of 1, 2, 4 and 8 nats), so for query i every key j > i outscores every key it may see,
           and the keys past kv_len outscore all of them.  V rows at j >= kv_len hold +-64: any leak moves O by O(64).
  phantom  every real key at -40 nats (+- 2): a zero-score phantom key from the zero-filled tail of the last 64-key tile would take
           essentially all the mass (e^40 against Tk e^0).
  plateau  1000-odd keys at level 0, then ONE later 64-key tile [960, 1024) stepped up: +6 nats in the even rows of even 32-row
           waves -- over the forward's rescale threshold (8 in log2 units = 5.55 nats), so the wave raises its maximum mid-row and
           rescales O and l -- and +5 nats in every other row, under it: an odd wave never rescales and packs P up to e^5 = 2^7.2
           to bf16.  V is +1 +- 0.5 on the plateau and -1 +- 0.5 on the step, and the mass before the step is 3.6 % (even rows)
           or 9.5 % (odd rows) of the total, so a rescale that forgets O or l is off by O(1).  Noise <= 0.06 nats keeps every row
           on its side of the threshold.
  onehot   one key per (b, h) at 0 nats, every other real key at -40, masked keys at +60 with +-64 rows: O = V[peak].  The peak
           moves with (b, h) over 0, 63, 64, 127, 128, 255, 256, Tk - 1, kv_len - 1 (where they exist).
  uniform  every score exactly -30 nats (no noise): O = mean(V[:kv_len]), lse = -30 + log(kv_len).
  offset   N(0, 1) scores (noise channels only) shifted by -80 nats through channel 0: the softmax must not move.

Reference: float64 softmax attention per (b, h) slice: O, lse and the backward (dQ, dK, dV from P, dP and delta), plus per-element
bounds derived from the kernels' rounding points (``fwd_bounds`` / ``bwd_bounds``, documented there).  ``emulate`` is a float64
stand-in for the kernels with one deliberate flaw at a time; the CPU power test shows each flaw misses these bounds by >= 10x.
"""
import math
from dataclasses import dataclass, field
from typing import List, Optional

import torch

BF = torch.bfloat16
F64 = torch.float64
SCALE = 0.125
LOG2E = 1.4426950408889634
RESCALE_THR = 8.0            # attention_fwd.hip: the forward's lazy-rescale threshold (log2 units)
EPS_BF = 2.0 ** -8           # unit roundoff of bf16: 8 significant bits, round to nearest (half an ulp of [1, 2) is 2^-8)
EPS_F32 = 2.0 ** -24
SCENARIOS = ("masked", "phantom", "plateau", "onehot", "uniform", "offset")
STEP0 = 960                  # plateau: first key of the stepped tile
ONEHOT_PEAKS = (0, 63, 64, 127, 128, 255, 256)


@dataclass
class Case:
    scenario: str
    q: torch.Tensor              # bf16 [B, Tq, H, 64] strided view
    k: torch.Tensor              # bf16 [B, Tk, H, 64] strided view
    v: torch.Tensor
    kv_len: Optional[List[int]]  # per-sample key length (None: all Tk keys)
    causal: bool
    noise_bound: float           # max |score contribution of channels 1..63| in nats
    r: torch.Tensor              # float64 [B, H, Tq]: planted query factor (q[..., 0] / 8)
    t: torch.Tensor              # float64 [B, H, Tk]: planted key factor (k[..., 0])
    peak: Optional[torch.Tensor] = None  # onehot: int [B, H] peak key
    meta: dict = field(default_factory=dict)

    @property
    def shape(self):
        B, Tq, H, _ = self.q.shape
        return B, H, Tq, self.k.shape[1]

    def lens(self):
        B, H, Tq, Tk = self.shape
        return [min(Tk, n) for n in self.kv_len] if self.kv_len is not None else [Tk] * B

    def kv_len_tensor(self, device):
        return None if self.kv_len is None else torch.tensor(self.kv_len, dtype=torch.int32, device=device)


def bf16_ramp(n, start=1.0):
    """n strictly increasing bf16 values: start and its n - 1 bf16 successors."""
    bits = torch.tensor([start], dtype=BF).view(torch.int16).item()
    return torch.arange(bits, bits + n, dtype=torch.int32).to(torch.int16).view(BF).double()


def _bf(x):
    return x.to(BF)


def _noise(shape, amp, g):
    return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * amp)


def make(scenario, B, H, Tq, Tk, *, causal=False, kv_len=None, seed=0, noise=True):
    """Builds one case.  ``noise=False`` zeroes channels 1..63 (scores are then exactly r_i t_j)."""
    assert scenario in SCENARIOS and (not causal or Tq == Tk)
    g = torch.Generator().manual_seed(seed * 1009 + Tq * 7 + Tk)
    lens = [min(Tk, n) for n in kv_len] if kv_len is not None else [Tk] * B
    assert min(lens) >= 1
    r = torch.ones(B, H, Tq, dtype=F64)
    t = torch.zeros(B, H, Tk, dtype=F64)
    vv = torch.randn(B, Tk, H, 64, generator=g, dtype=F64)
    aq, ak = 2.0 ** -2, 1.0
    jj = torch.arange(Tk)
    masked_key = torch.stack([jj >= n for n in lens])[:, None, :].expand(B, H, Tk)  # [B, H, Tk]
    big_v = 64.0 * torch.sign(torch.randn(B, Tk, H, 64, generator=g, dtype=F64))
    peak = None
    if scenario == "masked":
        assert causal or kv_len is not None, "the masked needle needs a mask"
        if causal:
            r.fill_(128.0)
            t[:] = bf16_ramp(Tk)
            aq, ak = 2.0 ** -3, 2.0 ** -2
        else:
            t[masked_key] = 60.0
    elif scenario == "phantom":
        t.fill_(-40.0)
    elif scenario == "plateau":
        assert Tk >= STEP0 + 64 and not causal
        i = torch.arange(Tq)
        even = ((i // 32) % 2 == 0) & (i % 2 == 0)
        r[:] = torch.where(even, 6.0, 5.0).double()
        t[:, :, STEP0:STEP0 + 64] = 1.0
        aq, ak = 2.0 ** -4, 2.0 ** -3
        vv = 1.0 + 0.5 * vv
        vv[:, STEP0:STEP0 + 64] -= 2.0
    elif scenario == "onehot":
        t.fill_(-40.0)
        peak = torch.zeros(B, H, dtype=torch.long)
        for b in range(B):
            cands = sorted({p for p in ONEHOT_PEAKS + (Tk - 1, lens[b] - 1) if p < lens[b]})
            for h in range(H):
                peak[b, h] = cands[(b * H + h + seed) % len(cands)]
                t[b, h, peak[b, h]] = 0.0
        t[masked_key] = 60.0
    elif scenario == "uniform":
        t.fill_(-30.0)
        aq = ak = 0.0
        vv = 1.0 + 0.5 * vv
    elif scenario == "offset":
        t.fill_(-80.0)
        aq = ak = None  # N(0, 1) noise scores
    if not noise:
        aq = ak = 0.0
    vv = torch.where(masked_key.permute(0, 2, 1)[..., None], big_v, vv)

    q = torch.zeros(B, Tq, H, 64, dtype=F64)
    k = torch.zeros(B, Tk, H, 64, dtype=F64)
    q[..., 0] = 8.0 * r.permute(0, 2, 1)
    k[..., 0] = t.permute(0, 2, 1)
    if aq is None:  # q_c, k_c ~ N(0, 1): sum of 63 products / 8 ~ N(0, 63 / 64)
        q[..., 1:] = torch.randn(B, Tq, H, 63, generator=g, dtype=F64)
        k[..., 1:] = torch.randn(B, Tk, H, 63, generator=g, dtype=F64)
    elif aq > 0:
        q[..., 1:] = _noise((B, Tq, H, 63), aq, g)
        k[..., 1:] = _noise((B, Tk, H, 63), ak, g)
    qb, kb, vb = _bf(q), _bf(k), _bf(vv)
    # the planted factors survive bf16 rounding unchanged
    assert torch.equal(qb[..., 0].double(), q[..., 0]) and torch.equal(kb[..., 0].double(), k[..., 0])
    qv, kv_, vv_ = _engine_layout(qb, kb, vb)
    nb = 63 * float(qb[..., 1:].double().abs().max()) * float(kb[..., 1:].double().abs().max()) / 8 if qb.shape[-1] > 1 else 0.0
    return Case(scenario, qv, kv_, vv_, list(kv_len) if kv_len is not None else None, causal, nb, r, t, peak,
                meta=dict(seed=seed, aq=aq, ak=ak))


def _engine_layout(q, k, v):
    """bf16 [B, T, H, 64] tensors -> strided views as the engine holds them (fused q | k | v when Tq == Tk, else q and fused k | v)."""
    B, Tq, H, _ = q.shape
    Tk = k.shape[1]
    d = H * 64
    if Tq == Tk:
        buf = torch.empty(B, Tq, 3 * d, dtype=BF)
        for i, x in enumerate((q, k, v)):
            buf[:, :, i * d:(i + 1) * d] = x.reshape(B, Tq, d)
        return tuple(buf[:, :, i * d:(i + 1) * d].unflatten(2, (H, 64)) for i in range(3))
    qb = q.reshape(B, Tq, d).clone()
    kvb = torch.empty(B, Tk, 2 * d, dtype=BF)
    kvb[:, :, :d] = k.reshape(B, Tk, d)
    kvb[:, :, d:] = v.reshape(B, Tk, d)
    return qb.unflatten(2, (H, 64)), kvb[:, :, :d].unflatten(2, (H, 64)), kvb[:, :, d:].unflatten(2, (H, 64))


def to_device(case, device):
    """The same case with its operands (same strided layout) on ``device``."""
    q, k, v = case.q, case.k, case.v
    if q.shape[1] == k.shape[1]:
        base = q._base if q._base is not None else q
        buf = base.to(device)
        d = q.shape[2] * 64
        q, k, v = (buf[:, :, i * d:(i + 1) * d].unflatten(2, (q.shape[2], 64)) for i in range(3))
    else:
        qb = (q._base if q._base is not None else q).to(device)
        kvb = (k._base if k._base is not None else k).to(device)
        H = q.shape[2]
        d = H * 64
        q = qb.reshape(q.shape[0], q.shape[1], d).unflatten(2, (H, 64))
        k, v = (kvb[:, :, i * d:(i + 1) * d].unflatten(2, (H, 64)) for i in range(2))
    c = Case(**{**case.__dict__})
    c.q, c.k, c.v = q, k, v
    return c


# ---- float64 reference ------------------------------------------------------------------------------------------------------
def _mask(case, b, Tq, Tk, diag_shift=0, extra_key=0):
    n = min(Tk, case.lens()[b] + extra_key)
    m = torch.arange(Tk)[None, :] < n
    m = m.expand(Tq, Tk).clone()
    if case.causal:
        m &= torch.arange(Tk)[None, :] <= torch.arange(Tq)[:, None] + diag_shift
    return m


def _slices(case):
    B, H, Tq, Tk = case.shape
    for b in range(B):
        for h in range(H):
            yield b, h, case.q[b, :, h].double(), case.k[b, :, h].double(), case.v[b, :, h].double()


def reference(case, d_o=None, q_rows=None):
    """float64 O [B, Tq, H, 64], lse [B, H, Tq], the row weights A = sum_j p_ij |V_j| and the slice statistics the bounds need;
    with ``d_o`` ([B, Tq, H * 64]) also dQ, dK, dV (same shapes as q, k, v) from P, dP = dO V^T, delta = rowsum(dO * O)."""
    B, H, Tq, Tk = case.shape
    out = {n: torch.zeros(B, Tq, H, 64, dtype=F64) for n in ("o", "A")}
    out["lse"] = torch.zeros(B, H, Tq, dtype=F64)
    out["s_abs"] = torch.zeros(B, H, Tq, dtype=F64)
    out["s_max"] = torch.zeros(B, H, Tq, dtype=F64)
    if d_o is not None:
        dO_all = d_o.double().reshape(B, Tq, H, 64)
        for n in ("dq", "dq_bound"):
            out[n] = torch.zeros(B, Tq, H, 64, dtype=F64)
        for n in ("dk", "dv", "dk_bound", "dv_bound"):
            out[n] = torch.zeros(B, Tk, H, 64, dtype=F64)
    for b, h, q, k, v in _slices(case):
        s = (q @ k.T) * SCALE
        ok = _mask(case, b, Tq, Tk)
        s = s.masked_fill(~ok, -math.inf)
        lse = torch.logsumexp(s, -1)
        p = torch.exp(s - lse[:, None])
        o = p @ v
        out["o"][b, :, h] = o
        out["lse"][b, h] = lse
        out["A"][b, :, h] = p @ v.abs()
        sab = ((q.abs() @ k.abs().T) * SCALE).masked_fill(~ok, 0.0)
        out["s_abs"][b, h] = sab.max(-1).values
        out["s_max"][b, h] = s.max(-1).values
        if d_o is None:
            continue
        dO = dO_all[b, :, h]
        dp = dO @ v.T
        delta = (dO * o).sum(-1)
        ds = p * (dp - delta[:, None])
        out["dv"][b, :, h] = p.T @ dO
        out["dq"][b, :, h] = SCALE * ds @ k
        out["dk"][b, :, h] = SCALE * ds.T @ q
        # ---- backward bounds (see bwd_bounds) ----
        eps_s = _eps_score(sab.max(-1).values)
        tol_lse = _lse_tol(lse, s.max(-1).values, eps_s, Tk)
        eps_p = eps_s + tol_lse + 2.0 ** -22 + 2.0 ** -23 * lse.abs()                    # relative error of the kernel's P
        tol_o = (2 * EPS_BF + 2 * eps_s[:, None] + Tk * EPS_F32) * (p @ v.abs())
        e_delta = dO.abs().mul(tol_o).sum(-1) + 2.0 ** -18 * (dO * o).abs().sum(-1)      # delta from the kernel's O (+ residual)
        e_dp = 2.0 ** -18 * (dO.abs() @ v.abs().T)                                       # 64-term fp32 sum of exact products
        E = p * ((eps_p[:, None] + EPS_BF + 2.0 ** -22) * (dp - delta[:, None]).abs() + e_dp + e_delta[:, None])
        out["dv_bound"][b, :, h] = (p * (EPS_BF + eps_p[:, None] + Tq * EPS_F32)).T @ dO.abs() + EPS_BF * out["dv"][b, :, h].abs()
        out["dk_bound"][b, :, h] = SCALE * (E.T @ q.abs() + Tq * EPS_F32 * ds.abs().T @ q.abs()) + EPS_BF * out["dk"][b, :, h].abs()
        out["dq_bound"][b, :, h] = SCALE * (E @ k.abs() + Tk * EPS_F32 * ds.abs() @ k.abs()) + EPS_BF * out["dq"][b, :, h].abs()
    return out


def _eps_score(s_abs):
    """fp32 error of a scaled score (nats): 64 exact bf16 products summed in fp32, worst case one rounding of the running
    sum per product: 64 * 2^-24 * sum_c |q_c k_c| / 8."""
    return 64 * EPS_F32 * s_abs


def _lse_tol(lse, s_max, eps_s, Tk):
    """lse = (m + log2 l) ln 2 in fp32: the score error, the rounding of the running maximum m (log2 units) and of the final product,
    l summed in fp32 over Tk keys (each exp2 within 2^-22), log2 within 2^-21."""
    return 2 * eps_s + 2.0 ** -21 * (lse.abs() + s_max.abs()) + Tk * EPS_F32 + 2.0 ** -20


def fwd_bounds(case, ref):
    """Per-element bound for O and per-row bound for lse.

    O: the kernels round exactly twice -- P to bf16 before the PV MFMA (rel u = 2^-8 per key, so at most u sum_j p_j |V_j| = u A)
    and O itself to bf16 (rel u, |O| <= A).  On top: the fp32 score error eps_s (a relative error of each P), and fp32 sums over
    Tk keys (Tk 2^-24 A).  tol_O = (2u + 2 eps_s + Tk 2^-24) A.
    lse: see _lse_tol; it is fp32 throughout, no bf16 rounding touches it."""
    B, H, Tq, Tk = case.shape
    eps_s = _eps_score(ref["s_abs"])                                   # [B, H, Tq]
    tol_o = (2 * EPS_BF + 2 * eps_s.permute(0, 2, 1)[..., None] + Tk * EPS_F32) * ref["A"] + 1e-30
    tol_lse = _lse_tol(ref["lse"], ref["s_max"], eps_s, Tk)
    return tol_o, tol_lse


def bwd_bounds(ref):
    """u = 2^-8, the unit roundoff of bf16.
    dV = sum_i bf16(P_ij) dO_i, rounded: (u + eps_P + Tq 2^-24) sum_i P_ij |dO_i| + u |dV|, with eps_P the relative error
    of the kernel's P = exp2(s log2e / 8 - lse log2e): score error + lse error + exp2.
    dK, dQ: dS = P (dP - delta) is rounded to bf16 before its MFMA; its error E_ij = P_ij [(eps_P + u) |dP - delta| + err(dP) +
    err(delta)], err(delta) from the kernel's O (within tol_O) and a 64-term fp32 sum; then tol_dK = (sum_i E_ij |Q_i| + Tq 2^-24
    sum_i |dS_ij| |Q_i|) / 8 + u |dK| (one rounding of dK), tol_dQ alike over keys."""
    return ref["dq_bound"] + 1e-30, ref["dk_bound"] + 1e-30, ref["dv_bound"] + 1e-30


def margin(got, want, tol):
    """max |got - want| / tol (< 1: within the bound).  NaN anywhere counts as infinitely far."""
    err = (got.double() - want.double()).abs() / tol
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    return float(err.max())


# ---- float64 emulation of the kernels with one deliberate flaw ------------------------------------------------------------
FLAWS = ("kv_len_admitted", "phantom_admitted", "diagonal_shifted", "rescale_forgets_o", "rescale_forgets_l")


def emulate(case, flaw=None):
    """O [B, Tq, H, 64] and lse [B, H, Tq] the way the forward kernel computes them -- 64-key tiles, a running maximum per row in
    log2 units raised only when some row of the 32-row wave grows past it by more than RESCALE_THR -- in float64, with at most
    one flaw:
      kv_len_admitted    the key at kv_len[b] passes the mask (key <= kv_len instead of key < kv_len);
      phantom_admitted   the zero rows that fill the last 64-key tile past Tk pass the mask (score 0, V = 0);
      diagonal_shifted   the causal mask admits key i + 1 for query i;
      rescale_forgets_o  a raised maximum rescales l but not O;
      rescale_forgets_l  a raised maximum rescales O but not l."""
    assert flaw in (None,) + FLAWS
    B, H, Tq, Tk = case.shape
    o_out = torch.zeros(B, Tq, H, 64, dtype=F64)
    lse_out = torch.zeros(B, H, Tq, dtype=F64)
    for b, h, q, k, v in _slices(case):
        n_keys = Tk
        if flaw == "phantom_admitted":
            n_keys = (Tk + 63) // 64 * 64
            k = torch.cat([k, k.new_zeros(n_keys - Tk, 64)])
            v = torch.cat([v, v.new_zeros(n_keys - Tk, 64)])
        s = (q @ k.T) * SCALE * LOG2E
        ok = _mask(case, b, Tq, n_keys, diag_shift=1 if flaw == "diagonal_shifted" else 0,
                   extra_key=1 if flaw == "kv_len_admitted" else 0)
        if flaw == "phantom_admitted":
            ok[:, Tk:] = True
            if case.causal:
                ok[:, Tk:] = False  # (causal: the diagonal masks tail rows anyway)
        s = s.masked_fill(~ok, -math.inf)
        m = torch.full((Tq,), -math.inf, dtype=F64)
        l = torch.zeros(Tq, dtype=F64)
        o = torch.zeros(Tq, 64, dtype=F64)
        for t0 in range(0, n_keys, 64):
            st = s[:, t0:t0 + 64]
            m_c = st.max(-1).values
            grow = (m_c > m + RESCALE_THR) | torch.isinf(m) & torch.isfinite(m_c)
            wave_grow = torch.zeros(Tq, dtype=torch.bool)  # the branch is wave-uniform: 32 query rows per wave
            for w0 in range(0, Tq, 32):
                wave_grow[w0:w0 + 32] = grow[w0:w0 + 32].any()
            m_new = torch.where(wave_grow, torch.maximum(m, m_c), m)
            alpha = torch.where(torch.isinf(m) & torch.isinf(m_new), torch.ones_like(m), torch.exp2(m - m_new))
            alpha = torch.where(wave_grow, alpha, torch.ones_like(alpha))
            if flaw != "rescale_forgets_l":
                l = l * alpha
            if flaw != "rescale_forgets_o":
                o = o * alpha[:, None]
            m = m_new
            p = torch.exp2(st - m[:, None]).nan_to_num(0.0)
            l = l + p.sum(-1)
            o = o + p @ v[t0:t0 + 64]
        o_out[b, :, h] = o / l[:, None]
        lse_out[b, h] = (m + torch.log2(l)) / LOG2E
    return o_out, lse_out


def applicable_flaws(case):
    """The flaws a scenario is built to expose (the power test requires a >= 10x miss for each)."""
    B, H, Tq, Tk = case.shape
    f = []
    if case.kv_len is not None and any(n < Tk for n in case.lens()) and case.scenario in ("masked", "onehot"):
        f.append("kv_len_admitted")
    if case.causal and case.scenario == "masked":
        f.append("diagonal_shifted")
    if Tk % 64 and not case.causal and case.scenario in ("phantom", "onehot", "uniform", "offset"):
        f.append("phantom_admitted")
    if case.scenario in ("plateau", "onehot"):
        f += ["rescale_forgets_o", "rescale_forgets_l"]
    return f
