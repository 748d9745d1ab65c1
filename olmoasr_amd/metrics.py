"""Token error counts of a training or evaluation step without a host loop: the sequences ``gen_pred`` scores
(scripts/training/train_timestamps.py, after the reference's gen_pred / calc_pred_wer, train_timestamps.py:1077-1180) cut out of the
prediction and target matrices by index arithmetic on their own device, and ``ops.edit_counts`` on them.  Nothing here reads the device
except ``ErrorCounter.counts()`` and ``ValidationTotals.record()``."""
import torch

from . import ops

EOT, IGNORE = 50256, 51864


def train_sequences(pred, targets, eot=EOT, ignore=IGNORE):
    """``gen_pred``'s rules as tensors: ``pred`` int [B, S] (``loss_and_backward(pred_out=...)``: -1 where nothing was computed), ``targets``
    int [B, S] -> (hyp int32 [B, S], hyp_len int32 [B], ref int32 [B, S + 1], ref_len int32 [B]).

      hyp row  ``pred`` cut after its first ``eot`` (inclusive) or before its first -1, whichever comes first
      ref row  ``targets`` with ``ignore`` removed (order kept), cut before the first ``eot``, then ``eot`` appended

    Entries past a length are unspecified (``ops.edit_counts`` never reads them).  Torch index plumbing on the operands' device -- no host
    synchronisation; CPU tensors work too."""
    if pred.dim() != 2 or targets.dim() != 2 or pred.shape[0] != targets.shape[0]:
        raise ValueError(f"train_sequences: pred [B, S] and targets [B, S'], got {tuple(pred.shape)} and {tuple(targets.shape)}")
    B, S = pred.shape
    St = targets.shape[1]
    dev = pred.device
    pos = torch.arange(S, device=dev).expand(B, S)
    after_eot = torch.where(pred == eot, pos + 1, S).amin(dim=1) if S else torch.zeros(B, dtype=torch.int64, device=dev)
    before_neg = torch.where(pred < 0, pos, S).amin(dim=1) if S else torch.zeros(B, dtype=torch.int64, device=dev)
    hyp_len = torch.minimum(after_eot, before_neg).to(torch.int32)
    # stable compaction of the kept targets: token k of the kept ones goes to column k, the ignored ones to a dump column past the row
    keep = targets != ignore
    dest = torch.where(keep, keep.cumsum(dim=1) - 1, St + 1)
    buf = torch.zeros(B, St + 2, dtype=targets.dtype, device=dev).scatter_(1, dest, targets)
    n_keep = keep.sum(dim=1, keepdim=True)
    tpos = torch.arange(St + 1, device=dev).expand(B, St + 1)
    cut = torch.where((buf[:, :St + 1] == eot) & (tpos < n_keep), tpos, n_keep).amin(dim=1, keepdim=True)  # first kept eot, or every kept token
    ref = buf[:, :St + 1].scatter_(1, cut, eot).to(torch.int32)
    return pred.to(torch.int32), hyp_len, ref, (cut.squeeze(1) + 1).to(torch.int32)


def pad_sequences(seqs, device="cpu"):
    """Python id lists -> (int32 [B, L] zero padded, int32 [B] lengths) on ``device`` (the operands of ``ops.edit_counts``)."""
    L = max([len(s) for s in seqs] + [1])
    tok = torch.zeros(len(seqs), L, dtype=torch.int32)
    for b, s in enumerate(seqs):
        tok[b, :len(s)] = torch.as_tensor(s, dtype=torch.int32)
    return tok.to(device), torch.tensor([len(s) for s in seqs], dtype=torch.int32).to(device)


class ErrorCounter:
    """Running (substitutions, deletions, insertions, hits) over the pairs it is fed, kept in an int64 [4] tensor on ``device``: ``add`` /
    ``add_sequences`` launch ``ops.edit_counts`` (``ops.edit_counts_host`` for CPU tensors) and sum its rows on the device; ``counts()`` is the
    only host read.  ``rate()`` = (S + D + I) / max(1, S + D + H), the token error rate of the same sequences."""

    def __init__(self, device="cpu", eot=EOT, ignore=IGNORE):
        self.total = torch.zeros(4, dtype=torch.int64, device=device)
        self.eot, self.ignore = eot, ignore

    def reset(self):
        self.total.zero_()

    def add_sequences(self, hyp, hyp_len, ref, ref_len):
        fn = ops.edit_counts if hyp.is_cuda else ops.edit_counts_host
        self.total += fn(hyp, hyp_len, ref, ref_len).sum(dim=0)

    def add(self, pred, targets):
        """One micro-batch: ``pred`` / ``targets`` [B, S] as ``train_sequences`` takes them."""
        self.add_sequences(*train_sequences(pred, targets, self.eot, self.ignore))

    def counts(self):
        """(S, D, I, H) as Python ints: the one device-to-host copy."""
        return tuple(int(v) for v in self.total.cpu().tolist())

    @staticmethod
    def fraction(counts):
        """(errors, reference tokens) = (S + D + I, S + D + H) of a (S, D, I, H) tuple."""
        s, d, i, h = counts
        return s + d + i, s + d + h

    def rate(self):
        errs, n = self.fraction(self.counts())
        return errs / max(1, n)


class ValidationTotals:
    """Running totals of ``OLMoASR.score`` results over a held-out set, kept on ``device``: ``nll`` float64 [1] (the sum of nll_sum) and
    ``counts`` int64 [3] = (tokens, hits, samples).  ``add`` sums a batch on the device, ``merge`` adds another instance's totals,
    ``packed()`` / ``load_packed()`` carry the whole state as ONE float64 [4] tensor for an all-reduce (the counts are far below 2^53, so
    float64 holds them exactly), and ``record()`` is the only host read.  ``val_loss`` is the token-weighted mean, sum nll_sum / sum n_tok: it
    does not depend on how the set was cut into batches (a mean of per-batch means would)."""

    def __init__(self, device="cpu"):
        self.nll = torch.zeros(1, dtype=torch.float64, device=device)
        self.counts = torch.zeros(3, dtype=torch.int64, device=device)

    def reset(self):
        self.nll.zero_()
        self.counts.zero_()

    def add(self, score):
        """One batch: a ``Score`` (or anything with ``nll_sum``, ``n_tok`` and ``n_hit`` tensors [B])."""
        dev = self.nll.device
        self.nll += score.nll_sum.to(torch.float64).sum().to(dev)
        self.counts[:2] += torch.stack([score.n_tok.to(torch.int64).sum(), score.n_hit.to(torch.int64).sum()]).to(dev)
        self.counts[2] += score.n_tok.numel()
        return self

    def merge(self, other):
        self.nll += other.nll.to(self.nll.device)
        self.counts += other.counts.to(self.counts.device)
        return self

    def packed(self):
        return torch.cat([self.nll, self.counts.to(torch.float64)])

    def load_packed(self, t):
        self.nll.copy_(t[:1])
        self.counts.copy_(t[1:].round().to(torch.int64))
        return self

    def record(self):
        """{"val_loss", "val_token_acc", "val_n_tokens", "val_n_samples"} as Python numbers: the one device-to-host copy."""
        nll, tok, hit, n = self.packed().cpu().tolist()
        tok, hit, n = int(round(tok)), int(round(hit)), int(round(n))
        return {"val_loss": nll / max(1, tok), "val_token_acc": hit / max(1, tok), "val_n_tokens": tok, "val_n_samples": n}
