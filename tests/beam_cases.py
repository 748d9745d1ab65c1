"""Planted cases for the device-resident beam search (``ops.beam_update`` / ``ops.beam_update_host``; the rule: csrc/beam_core.h), and a
literal restatement of ``BeamSearchDecoder.update`` as ``olmoasr_amd/decoding.py`` runs it on the host -- dicts of tuples over plain Python
lists -- extended by the two rules the operator adds: a SHORT step (fewer than ``beam`` continuations: nothing of the window is written, the
window is skipped from then on) and the completion LATCH (once every pool is full, a step only writes identity sources).

A case is ``dict(name, n_audio, beam, patience, steps, ...)``: ``steps`` is a list of ``(top_lp, top_tok)`` with ``n_audio * beam`` rows of
``beam + 1`` entries each -- what ``ops.topk_tokens`` returns, log-probabilities descending, ``(-inf, 0)`` repeated when fewer survive.  The
sampled vocabulary is 0..7 with ``EOT`` = 7.  Not collected by pytest."""
import random
import struct

EOT = 7
INIT = [100, 101]  # the sot sequence
NINF = -float("inf")
FILL = -7  # the sentinel the states of the tests are filled with


def f32(x):
    """x rounded to float32, as a Python float (what ``torch.tensor(list_of_floats)`` stores)."""
    return struct.unpack("f", struct.pack("f", x))[0] if x == x and abs(x) != float("inf") else x


def max_candidates(case):
    return max(1, round(case["beam"] * (case.get("patience") or 1.0)))


class Ref:
    """The host path's state over plain lists."""

    def __init__(self, case):
        self.n_audio, self.beam, self.C = case["n_audio"], case["beam"], max_candidates(case)
        n = self.n_audio * self.beam
        self.tokens = [list(r) for r in case["init_rows"]] if "init_rows" in case else [list(INIT) for _ in range(n)]
        self.sums = [f32(s) for s in case.get("init_sums", [0.0] * n)]
        self.sources = list(range(n))
        self.last = [INIT[-1]] * n
        self.finished = [dict() for _ in range(self.n_audio)]
        self.short = [False] * self.n_audio

    def completed(self):
        return all(len(f) >= self.C for f in self.finished)

    def step(self, top_lp, top_tok):
        beam, n = self.beam, self.n_audio * self.beam
        if self.completed():  # the latch: identity sources, nothing else
            for a in range(self.n_audio):
                if not self.short[a]:
                    self.sources[a * beam:(a + 1) * beam] = range(a * beam, (a + 1) * beam)
            return
        tok_cpu, prev_sum = [list(r) for r in self.tokens], list(self.sums)
        for a in range(self.n_audio):
            if self.short[a]:
                continue
            next_tokens, new_sum, sources = [], [], []
            # ---- decoding.py, BeamSearchDecoder.update, one audio window ----
            scores, newly, origin = {}, {}, {}
            for j in range(beam):
                idx = a * beam + j
                prefix = tok_cpu[idx]
                for lp, t in zip(top_lp[idx], top_tok[idx]):
                    seq = tuple(prefix + [t])
                    scores[seq] = float(prev_sum[idx]) + lp
                    origin[seq] = idx
            saved = 0
            for seq in sorted(scores, key=scores.get, reverse=True):
                if seq[-1] == EOT:
                    newly[seq] = scores[seq]
                else:
                    new_sum.append(scores[seq])
                    next_tokens.append(list(seq))
                    sources.append(origin[seq])
                    saved += 1
                    if saved == beam:
                        break
            if saved < beam:  # the host path fails here (a ragged tensor); the operator flags the window and writes nothing
                self.short[a] = True
                continue
            for seq in sorted(newly, key=newly.get, reverse=True):
                if len(self.finished[a]) >= self.C:
                    break
                self.finished[a][seq] = newly[seq]
            # ---- end ----
            for m in range(beam):
                r = a * beam + m
                self.tokens[r], self.sums[r], self.sources[r], self.last[r] = next_tokens[m], f32(new_sum[m]), sources[m], next_tokens[m][-1]

    def snapshot(self):
        return dict(tokens=[list(r) for r in self.tokens], sums=list(self.sums), sources=list(self.sources), last=list(self.last),
                    pool=[[(list(seq), sc) for seq, sc in f.items()] for f in self.finished], short=list(self.short), completed=self.completed())


def run_ref(case):
    """The snapshots after every step of the case."""
    ref, out = Ref(case), []
    for top_lp, top_tok in case["steps"]:
        ref.step(top_lp, top_tok)
        out.append(ref.snapshot())
    return out


# ---- the same steps through ops.beam_update / ops.beam_update_host ------------------------------------------------------------------------
def make_state(ops, case, device, guard=2):
    import torch
    n_ctx = case.get("n_ctx", 24)
    st = ops.beam_state(case["n_audio"], case["beam"], max_candidates(case), n_ctx, INIT, device, fill=FILL, guard=guard)
    if "init_rows" in case:
        st.buffers[0][:, :len(INIT)] = torch.tensor(case["init_rows"], dtype=torch.int64, device=st.device)
    if "init_sums" in case:
        st.sums.copy_(torch.tensor(case["init_sums"], dtype=torch.float32))
    return st


def step_tensors(step, device):
    import torch
    top_lp, top_tok = step
    return torch.tensor(top_lp, dtype=torch.float32, device=device), torch.tensor(top_tok, dtype=torch.int64, device=device)


def state_snapshot(st, want):
    """The state in the shape of ``Ref.snapshot``: a live row is read up to the length the restatement says it has (``want``), and everything
    behind it must still be the sentinel; a short window's rows are reported as the restatement has them (they are checked apart)."""
    beam = st.beam
    count, full_len, short = st.status.cpu().tolist()
    toks, rows = st.tokens.cpu(), []
    for r, ref_row in enumerate(want["tokens"]):
        if short[r // beam]:
            rows.append(list(ref_row))
            continue
        assert toks[r, len(ref_row):].eq(FILL).all(), f"row {r}: something was written behind token {len(ref_row)}"
        rows.append(toks[r, :len(ref_row)].tolist())
    pool_tok, pool_len, pool_score = st.pool_tokens.cpu(), st.pool_len.cpu().tolist(), st.pool_score.cpu().tolist()
    pool = []
    for a in range(st.n_audio):
        pool.append([(pool_tok[a, k, :pool_len[a][k]].tolist(), pool_score[a][k]) for k in range(count[a])])
        for k in range(st.max_candidates):
            used = pool_len[a][k] if k < count[a] else 0
            assert pool_tok[a, k, used:].eq(FILL).all(), f"window {a}: pool slot {k} written behind its length"
    return dict(tokens=rows, sums=st.sums.cpu().tolist(), sources=st.sources.cpu().tolist(), last=st.last_token.cpu().tolist(), pool=pool,
                short=[bool(s) for s in short], completed=all(f != 0x7fffffff for f in full_len))


def guards_intact(st):
    """Every tensor of the state was allocated with guard rows of the sentinel on either side: they must still hold it."""
    g = st.guard
    for name, back in st.backing.items():
        assert g > 0 and back[:g].eq(FILL).all() and back[-g:].eq(FILL).all(), f"{name}: a guard row was written"


def run_state(ops, case, device, update):
    """Runs the case on a fresh state with ``update`` (ops.beam_update or ops.beam_update_host); yields (step, state, the buffer that was
    the step's input, its clone from before the step, the restatement's snapshot) after every step."""
    st = make_state(ops, case, device)
    for i, (step, want) in enumerate(zip(case["steps"], run_ref(case))):
        top_lp, top_tok = step_tensors(step, st.device)
        tokens_in, before_in, before_out = st.buffers[st.cur], st.buffers[st.cur].clone(), st.buffers[1 - st.cur].clone()
        update(st, top_lp, top_tok, eot=EOT)
        yield i, st, tokens_in, before_in, before_out, want


def check_case(ops, case, device, update):
    """``update`` against the restatement on every step and every output, with ``==``; plus what no step may write."""
    beam = case["beam"]
    for i, st, tokens_in, before_in, before_out, want in run_state(ops, case, device, update):
        got = state_snapshot(st, want)
        for key in want:
            assert got[key] == want[key], (case["name"], i, key, got[key], want[key])
        assert tokens_in.equal(before_in), (case["name"], i, "the step's input buffer was written")
        for a, short in enumerate(want["short"]):
            if short:  # a short window: neither buffer's rows moved
                assert st.tokens[a * beam:(a + 1) * beam].equal(before_out[a * beam:(a + 1) * beam]), (case["name"], i, "short window written")
        guards_intact(st)
    return want


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def pad(entries, K):
    """A row of the top-K: the given (logprob, token) pairs, then (-inf, 0) up to K entries."""
    entries = list(entries) + [(NINF, 0)] * (K - len(entries))
    return [f32(lp) for lp, _ in entries], [t for _, t in entries]


def steps_from(rows_per_step, K):
    out = []
    for rows in rows_per_step:
        padded = [pad(r, K) for r in rows]
        out.append(([p[0] for p in padded], [p[1] for p in padded]))
    return out


def split_step(B, K=None):
    """A first step that gives the B rows of ONE window B distinct prefixes: every row offers tokens 1..B at -0.1, -0.2, ..."""
    return [[(-0.1 * (k + 1), k + 1) for k in range(B)] for _ in range(B)]


def planted_cases():
    cases = []
    # 1. identical prefixes at step 0: the rows' candidates collapse, at the first row's position with the LAST row's score and origin
    cases.append(dict(name="identical prefixes", n_audio=1, beam=3, steps=steps_from([
        [[(-0.1, 1), (-0.5, 2), (-1.0, 3), (-2.0, 4)], [(-0.2, 1), (-0.4, 2), (-1.1, 3), (-2.5, 5)], [(-0.3, 1), (-0.6, 2), (-0.9, 3), (-3.0, EOT)]],
        [[(-0.1, 4), (-0.2, 5), (-0.3, 6), (-0.4, 1)], [(-0.1, 4), (-0.2, 5), (-0.3, 6), (-0.4, 1)], [(-0.1, 4), (-0.2, 5), (-0.3, 6), (-0.4, 1)]]], 4),
        expect=lambda snaps: snaps[0]["sources"] == [2, 2, 2] and snaps[0]["sums"] == [f32(-0.3), f32(-0.6), f32(-0.9)]))
    # 2. a row with 2 survivors of K = 4: (-inf, 0) twice
    cases.append(dict(name="few survivors", n_audio=1, beam=3, steps=steps_from([
        split_step(3),
        [[(-0.1, 1), (-0.2, 2)], [(-0.3, 3), (-0.4, 4), (-0.5, 5), (-0.6, 6)], [(-0.2, 1), (-0.9, 2)]],
        [[(-0.1, 1), (-0.2, 2)], [(-0.1, 1)], [(-0.5, 5), (-0.6, 6), (-0.7, 2), (-0.8, 3)]]], 4),
        expect=lambda snaps: not any(s["short"][0] for s in snaps) and all(x > NINF for x in snaps[-1]["sums"])))
    # 3. eot inside the first B continuations is pooled; eot behind the B-th continuation is dropped
    cases.append(dict(name="eot ranking", n_audio=1, beam=2, steps=steps_from([
        split_step(2),
        [[(-0.1, 1), (-0.2, EOT), (-3.0, 2)], [(-0.5, 3), (-4.0, 4), (-5.0, EOT)]]], 3),
        expect=lambda snaps: [p[0] for p in snaps[1]["pool"][0]] == [INIT + [1, EOT]] and not snaps[1]["completed"]))
    # 4. the pool cap (C = round(3 * 0.67) = 2) is reached in the middle of a step's finished list; later steps add none.  Window 1 never
    # finishes, so window 0 is not latched and goes on refusing
    eots = [[(-0.1 * (j + 1), EOT), (-1.0, 1), (-1.1, 2), (-1.2, 3)] for j in range(3)]
    plain = [[(-0.3, 1), (-0.4, 2), (-0.5, 3), (-0.6, 4)] for _ in range(3)]
    cases.append(dict(name="pool cap", n_audio=2, beam=3, patience=0.67, steps=steps_from([
        split_step(3) + split_step(3), eots + plain, eots + plain, plain + plain], 4),
        expect=lambda snaps: [len(p) for p in snaps[1]["pool"]] == [2, 0] and snaps[3]["pool"] == snaps[1]["pool"] and not snaps[3]["completed"]
        and [p[1] for p in snaps[1]["pool"][0]] == [f32(-0.1) + f32(-0.1), f32(-0.2) + f32(-0.2)]))
    # 5. equal double scores from different rows: insertion order decides who continues
    cases.append(dict(name="equal scores", n_audio=1, beam=2, steps=steps_from([
        [[(-0.5, 1), (-0.5, 2), (-9.0, 3)], [(-0.5, 1), (-0.5, 2), (-9.0, 3)]],
        [[(-1.0, 3), (-1.0, 4), (-3.0, 5)], [(-1.0, 4), (-2.0, 3), (-3.0, 5)]]], 3),
        expect=lambda snaps: snaps[0]["tokens"] == [INIT + [1], INIT + [2]] and snaps[1]["tokens"] == [INIT + [1, 3], INIT + [1, 4]]))
    # 6. equal in fp32, different in double: the double order decides, the stored sum is the rounded one
    cases.append(dict(name="fp32 versus double", n_audio=1, beam=2, init_sums=[-16777216.0, -16777216.0], steps=steps_from([
        [[(-1.0, 1), (-2.0, 3), (-3.0, 4)], [(-0.5, 2), (-2.5, 5), (-3.5, 6)]]], 3),
        expect=lambda snaps: snaps[0]["tokens"] == [INIT + [2], INIT + [1]] and snaps[0]["sums"] == [-16777216.0, -16777216.0]
        and snaps[0]["sources"] == [1, 0]))
    # 9. a short step: window 0 is left with one continuation of three; window 1 goes on
    cases.append(dict(name="short step", n_audio=2, beam=3, steps=steps_from([
        [[(-0.1, EOT)]] * 3 + split_step(3), plain + plain, plain + plain], 4),
        expect=lambda snaps: all(s["short"] == [True, False] for s in snaps) and snaps[2]["tokens"][0] == INIT and len(snaps[2]["tokens"][3]) == 5))
    # 8. three windows complete at steps 1, 2 and 4; two further updates after the latch change nothing but write identity sources
    B = 2
    rows = []
    for i in range(7):
        step = []
        for a, at in enumerate((1, 2, 4)):
            for j in range(B):
                if i == 0:
                    step.append([(-0.1, 1), (-0.2, 2), (-9.0, 3)])
                elif i == at:
                    step.append([(-0.1, EOT), (-0.5 - 0.1 * j, 3), (-0.9, 4)])
                else:
                    step.append([(-0.2 - 0.1 * j, 1 + (i + j) % 5), (-0.6, 6), (-2.0 + 0.5 * j, 2 - j)])  # (row 1 is ranked first now and then)
        rows.append(step)
    cases.append(dict(name="latch", n_audio=3, beam=B, steps=steps_from(rows, 3),
                      expect=lambda snaps: [s["completed"] for s in snaps] == [False] * 4 + [True] * 3 and snaps[5]["sources"] == list(range(6))
                      and all({k: v for k, v in s.items() if k != "sources"} == {k: v for k, v in snaps[4].items() if k != "sources"} for s in snaps[5:])
                      and any(s["sources"] != list(range(6)) for s in snaps[1:5])))
    return cases


def random_case(beam, seed, patience=None, n_audio=2, n_steps=12, distinct=None):
    """Seeded random log-probabilities over the 8-token vocabulary: every row offers min(K, survivors) distinct tokens (eot among them three
    times in ten), the rest is (-inf, 0).  ``distinct`` rows start from different prefixes (15 rows of one prefix over 8 tokens are short)."""
    rng = random.Random(1000 * beam + seed)
    K, n = beam + 1, n_audio * beam
    steps = []
    for _ in range(n_steps):
        rows = []
        for _ in range(n):
            vocab = [t for t in range(8) if t != EOT or rng.random() < 0.3]
            picks = rng.sample(vocab, min(K, rng.randint(max(1, len(vocab) - 3), len(vocab))))
            lps = sorted((f32(-rng.random() * 4.0) for _ in picks), reverse=True)
            rows.append(list(zip(lps, picks)))
        steps.append(rows)
    case = dict(name=f"random beam {beam} seed {seed} patience {patience}", n_audio=n_audio, beam=beam, patience=patience, steps=steps_from(steps, K))
    if distinct if distinct is not None else beam > 5:
        case["init_rows"] = [[100 + r, 101] for r in range(n)]
    return case


def patience_cases():
    # 7. C = 2 < B = 4 and C = 2 B
    return [random_case(4, 0, patience=0.5), random_case(4, 1, patience=0.5, n_audio=1), random_case(3, 0, patience=2.0),
            random_case(2, 1, patience=2.0, n_audio=3)]


def random_cases():
    # 10.
    return [random_case(beam, seed) for beam in (1, 2, 5, 15) for seed in (0, 1, 2)]


def all_cases():
    return planted_cases() + patience_cases() + random_cases()
