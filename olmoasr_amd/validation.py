"""Held-out scoring loops over ``OLMoASR.score``: host batches of clips that are never augmented (seeded synthetic indices, or shard
samples through ``data.AudioTextShards``), each trimmed to its own supervised span, scored on the device.  The token rows are built on the
host (as every loader here does), so the trim needs no device read; nothing in the loop synchronises with the device."""
import torch

from . import ops
from .synth import N_SAMPLES, N_TEXT_CTX, PAD_ID, supervised_span_host, synth_sample


def synthetic_batch(indices, timestamps=False):
    """HOST (pcm int16 [b, 480000], text_input i64 [b, 448], text_y i64 [b, 448], text_len i32 [b]) of the seeded synthetic samples."""
    items = [synth_sample(int(i), timestamps) for i in indices]
    return (torch.stack([it[0] for it in items]), torch.stack([it[1] for it in items]), torch.stack([it[2] for it in items]),
            torch.tensor([it[3] for it in items], dtype=torch.int32))


def shard_batch(shards, indices):
    """The same from ``data.AudioTextShards`` samples (clips zero-padded to 30 s, as ``ShardLoader`` pads them)."""
    b = len(indices)
    pcm = torch.zeros(b, N_SAMPLES, dtype=torch.int16)
    ti = torch.full((b, N_TEXT_CTX), PAD_ID, dtype=torch.int64)
    ty = torch.full((b, N_TEXT_CTX), PAD_ID, dtype=torch.int64)
    tl = torch.zeros(b, dtype=torch.int32)
    for r, i in enumerate(indices):
        clip, ti[r], ty[r], n = shards.load(int(i))
        pcm[r, :clip.shape[0]] = torch.from_numpy(clip.copy())
        tl[r] = int(n)
    return pcm, ti, ty, tl


def trimmed_context(span_host, n_text_ctx=N_TEXT_CTX):
    """The decoder context a batch needs: its largest span rounded up to 64 (at least 64, at most n_text_ctx)."""
    top = int(span_host.max()) if span_host.numel() else 0
    return max(64, min(n_text_ctx, (top + 63) // 64 * 64))


def score_batch(net, batch, device, trim=True):
    """One host batch through ``net.score``: returns (Score, targets on the device [b, S]) with S = ``trimmed_context`` of the batch
    (``trim=False``: the full context)."""
    pcm, ti, ty, tl = batch
    span = supervised_span_host(ty, tl)
    S = trimmed_context(span, net.dims.n_text_ctx) if trim else net.dims.n_text_ctx
    mel = ops.log_mel(pcm.to(device, non_blocking=True))
    ty_d = ty[:, :S].to(device, non_blocking=True)
    sc = net.score(mel, ti[:, :S].to(device, non_blocking=True), ty_d, tl.to(device, non_blocking=True), span=span.to(device, non_blocking=True))
    return sc, ty_d


def score_set(net, n, fetch, device, batch, totals=None, counter=None, trim=True):
    """Scores samples 0 .. n - 1 in order, ``batch`` at a time; ``fetch(list of positions)`` returns a host batch.  Feeds ``totals``
    (``metrics.ValidationTotals``) and ``counter`` (``metrics.ErrorCounter``, from the teacher-forced predictions) when given and yields each
    batch's ``Score``."""
    for i in range(0, n, batch):
        sc, ty_d = score_batch(net, fetch(list(range(i, min(n, i + batch)))), device, trim)
        if totals is not None:
            totals.add(sc)
        if counter is not None:
            counter.add(sc.pred, ty_d)
        yield sc
