"""Frozen parameters on the host side: the data-parallel reducers communicate the trainable ranges of the gradient arena only (torch
DDP leaves requires_grad=False parameters out of its buckets), and ZeRO-1 refuses a partly frozen model."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from olmoasr_amd import ddp


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


N = 1000
SEGMENTS = [(0, 100), (100, 300), (400, 350), (750, 250)]  # completion order == arena order here
TRAINABLE = [(0, 60), (160, 200), (900, 100)]                # frozen: [60, 160), [360, 900)


def test_trainable_pieces_and_buckets():
    pieces = ddp.trainable_pieces(SEGMENTS, TRAINABLE)
    assert pieces == [(0, 60, 0), (160, 200, 1), (900, 100, 3)]
    red = ddp.GradReducer(torch.zeros(N), SEGMENTS, trainable=TRAINABLE)
    assert sum(n for _, n, _ in red.buckets) == 360
    for off, n, _ in red.buckets:
        assert any(lo <= off and off + n <= lo + m for lo, m in TRAINABLE)


class _ArenaModule(torch.nn.Module):
    def __init__(self, rank):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(N))
        self.flat_params = self.w.data
        self.flat_grads = torch.full((N,), float("nan"))  # frozen ranges: never written by the backward; must not be touched
        for lo, m in TRAINABLE:
            self.flat_grads[lo:lo + m] = 0.0
        self.grad_segments = list(SEGMENTS)

    def trainable_ranges(self):
        return list(TRAINABLE)

    def refresh_shadow(self):
        pass

    def forward(self, x):
        return x

    def fake_backward(self, g):
        for lo, m in TRAINABLE:
            self.flat_grads[lo:lo + m] += g[lo:lo + m]
        post = getattr(self, "_autograd_post_backward", None)
        if post is not None:
            post()


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g = [torch.randn(N, generator=torch.Generator().manual_seed(7 * r + 1)) for r in range(world)]
        # DistributedDataParallel: mean over ranks on the trainable ranges; the frozen ranges (NaN here) are never sent or received
        base = _ArenaModule(rank)
        model = ddp.DistributedDataParallel(base, device_ids=[rank])
        model(torch.zeros(1))
        base.fake_backward(g[rank])
        mean = sum(g) / world
        for lo, m in TRAINABLE:
            assert torch.allclose(base.flat_grads[lo:lo + m], mean[lo:lo + m], atol=1e-6)
        frozen = torch.ones(N, dtype=torch.bool)
        for lo, m in TRAINABLE:
            frozen[lo:lo + m] = False
        assert torch.isnan(base.flat_grads[frozen]).all()
        # GradReducer (fused path): SUM over ranks == one rank accumulating both ranks' micro-batches
        flat = torch.full((N,), float("nan"))
        for lo, m in TRAINABLE:
            flat[lo:lo + m] = g[rank][lo:lo + m]
        red = ddp.GradReducer(flat, SEGMENTS, trainable=TRAINABLE, force=True)
        red.reduce()
        acc = torch.zeros(N)
        for r in range(world):
            acc += g[r]
        for lo, m in TRAINABLE:
            assert torch.allclose(flat[lo:lo + m], acc[lo:lo + m], atol=1e-6)
        assert torch.isnan(flat[frozen]).all()
        q.put((rank, "ok"))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_reducers_skip_frozen_ranges_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(60)
    assert all(r[1] == "ok" for r in res), res


def test_zero1_refuses_a_partly_frozen_model():
    from olmoasr_amd import _native as N_
    from olmoasr_amd import zero

    class _Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Parameter(torch.zeros(4))
            self.b = torch.nn.Parameter(torch.zeros(4))
            self.flat_params = torch.zeros(8)

    net = _Net()
    net.b.requires_grad_(False)
    with pytest.raises(N_.NativeError, match="frozen"):
        zero.NativeBackend(net)


def test_freeze_encoder_flag_parses():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("tt_cli_freeze", os.path.join(root, "scripts", "training", "train_timestamps.py"))
    tt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tt)
    assert tt.parse_args([]).freeze_encoder is False
    assert tt.parse_args(["--freeze_encoder", "True"]).freeze_encoder is True
    assert tt.parse_args(["--freeze_encoder=False"]).freeze_encoder is False
    assert tt.parse_args(["--freeze_encoder"]).freeze_encoder is True


def test_finetuning_state_dict_adds_the_pad_row():
    import math
    from types import SimpleNamespace
    from olmoasr_amd import hub
    dims = dict(n_mels=80, n_audio_ctx=1500, n_audio_state=384, n_audio_head=6, n_audio_layer=1, n_vocab=51864, n_text_ctx=448,
                n_text_state=384, n_text_head=6, n_text_layer=1)
    emb = torch.randn(51864, 384)
    ck = {"dims": dims, "model_state_dict": {"decoder.token_embedding.weight": emb, "decoder.ln.weight": torch.ones(384)}}
    d, sd = hub.finetuning_state_dict(ck, seed=3)
    e = sd["decoder.token_embedding.weight"]
    assert d.n_vocab == 51864 and e.shape == (51865, 384) and torch.equal(e[:-1], emb)
    want = torch.empty(1, 384).normal_(0.0, math.sqrt(2.0 / 384), generator=torch.Generator().manual_seed(3))
    assert torch.equal(e[-1:], want)  # kaiming normal (fan_in = n_state), as a fresh model draws the embedding
    assert not torch.equal(hub.finetuning_state_dict(ck, seed=4)[1]["decoder.token_embedding.weight"][-1], e[-1])
    # a training checkpoint (module. prefix, n_vocab + 1 rows) passes through unchanged
    ck2 = {"dims": SimpleNamespace(**dims), "model_state_dict": {"module.decoder.token_embedding.weight": e}}
    assert torch.equal(hub.finetuning_state_dict(ck2)[1]["decoder.token_embedding.weight"], e)
    with pytest.raises(ValueError):
        hub.finetuning_state_dict({"dims": dims, "model_state_dict": {"decoder.token_embedding.weight": torch.zeros(10, 384)}})
