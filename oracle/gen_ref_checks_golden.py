"""Writes tests/golden/ref_checks.npz and tests/golden/ref_checks.json: reference outputs for the checks that used to run the
UNMODIFIED reference live, captured once so that the tests need nothing outside the repository.  Run it where the reference
tree is readable (``OLMOASR_REFERENCE`` names it): ``python -m oracle.gen_ref_checks_golden``.  TEST INFRASTRUCTURE ONLY.

  ref_checks.npz   the reference olmoasr.model.OLMoASR (tiny, CPU fp32) on the B=2 synthetic batch with init_state_dict(seed 0):
                   its logits at LOGIT_SAMPLE seeded (sample, position, vocabulary) entries
  ref_checks.json  "transcribe_clip": the reference's transcribe() on the scripted case TRANSCRIBE_CLIP_CASE (clip_timestamps with
                   a closed and an open-ended clip, a three-step temperature ladder); "ckpt_state_dict": key -> shape of the
                   reference OLMoASR's state_dict at CKPT_DIMS (what its load_state_dict(strict=True) accepts)
"""
import json
import os

import numpy as np
import torch

from oracle import mel_oracle as me
from oracle import model_oracle as mo
from oracle import ref_import
from oracle import ref_transcribe_harness as H

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
LOGIT_SAMPLE = 16384
TRANSCRIBE_CLIP_CASE = dict(seed=99, content_frames=45000, kw=dict(temperature=(0.0, 0.4, 0.8), logprob_threshold=-0.8,
                                                                     no_speech_threshold=0.5, clip_timestamps=[3.0, 200.0, 210.5]))
CKPT_DIMS = mo.Dims(80, 1500, 64, 1, 1, 51864, 448, 64, 1, 1)


def logit_sample_index(shape):
    """(sample, position, vocabulary) indices of the stored logits: a torch CPU generator with seed 0."""
    g = torch.Generator().manual_seed(0)
    return tuple(torch.randint(0, n, (LOGIT_SAMPLE,), generator=g) for n in shape)


def main():
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    ref_model, _, ref_dims = ref_import.load()
    dims = mo.VARIANTS["tiny"]
    sd = mo.init_state_dict(dims, seed=0)
    pcm, ti, ty, tl = mo.synthetic_batch([0, 1])
    mel = torch.from_numpy(me.log_mel_batch(pcm.numpy(), dtype=np.float32))
    net = ref_model.OLMoASR(ref_dims.VARIANT_TO_DIMS["tiny"])
    net.load_state_dict(sd, strict=True)
    with torch.no_grad():
        lg = net(mel, ti, mo.build_padding_mask(tl))
    b, p, v = logit_sample_index(lg.shape)
    np.savez_compressed(os.path.join(OUT, "ref_checks.npz"), logit_shape=np.array(lg.shape, dtype=np.int64),
                        logit_value=lg[b, p, v].numpy().astype(np.float32))

    c = TRANSCRIBE_CLIP_CASE
    clip = H.comparable(H.run_reference(H.scripted_decode(c["seed"]), H.index_mel(c["content_frames"]), **dict(c["kw"])))
    ck = ref_model.OLMoASR(dims=ref_dims.ModelDimensions(**CKPT_DIMS.__dict__))
    shapes = {k: list(t.shape) for k, t in ck.state_dict().items()}
    with open(os.path.join(OUT, "ref_checks.json"), "w") as f:
        json.dump({"transcribe_clip": clip, "ckpt_state_dict": shapes}, f, separators=(",", ":"))
    print("ref_checks.npz / ref_checks.json written:", len(clip["segments"]), "segments,", len(shapes), "state_dict entries")


if __name__ == "__main__":
    main()
