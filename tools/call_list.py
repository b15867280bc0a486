"""The library calls of one step, in order: ``python tools/call_list.py fp32|bf16|fp16x3|eval`` prints, for every pcaa_*
call, the entry point, its integer and float arguments and the ordinal (by first appearance) of the stream it went to.
Pointers are not recorded, so two trees that launch the same work print the same list -- the check of a refactor of the
Python layer.  ``fp32`` / ``bf16`` / ``fp16x3``: one eager PCAATrainer step at B=4, N=32, C=4, K=4; ``eval``: one eval-mode
encoder_forward(want_bwd=True) + encoder_backward(need_dx=True).  One process per list; no profiler."""
import ctypes
import os
import re
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opensetgaitrecognition_pcaa_amd import _lib, constants, functional as F, models, synthetic as syn  # noqa: E402
from opensetgaitrecognition_pcaa_amd.train import PCAATrainer  # noqa: E402
from oracle import pcaa_oracle as O  # noqa: E402

NUMBERS = (ctypes.c_int, ctypes.c_long, ctypes.c_size_t, ctypes.c_float, ctypes.c_double)


class Recorder:
    def __init__(self, lib):
        self.lib, self.calls, self.streams = lib, [], {}
        with open(_lib.HEADER) as f:           # the entry points whose last parameter is the stream
            self.streamed = set(re.findall(r"\b(pcaa_\w+)\s*\([^)]*\bstream\s*\)", f.read()))

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("pcaa_"):
            return fn

        def call(*args):
            nums = [a for a, t in zip(args, fn.argtypes) if t in NUMBERS]
            st = self.streams.setdefault(args[-1], len(self.streams)) if name in self.streamed else "-"
            self.calls.append(f"{name} {nums} stream {st}")
            return fn(*args)
        return call


def main(what):
    B, N, C, K, T = 4, 32, 4, 4, constants.NSTEPS
    constants.NFEATURES = C
    rec = _lib._lib = Recorder(_lib.load())
    x = syn.synthetic_pcs(B, T, N, C, seed=1).to("cuda:0").permute(0, 3, 1, 2)
    if what == "eval":
        enc = models.CGEncoder(K, nmax_points=N, use_projection_head=True).float()
        syn.deterministic_fill_(enc, 0)
        enc = enc.to("cuda:0").eval()
        logits, fv, st = F.encoder_forward(enc, x, False, mode="fp32", want_bwd=True)
        F.encoder_backward(enc, st, torch.ones_like(logits), torch.ones_like(fv), need_dx=True)
    else:
        cfg = dict(constants.CONFIG, NMAX=N, TRAIN_CLASSES=list(range(K)), BATCH_SIZE=B)
        tr = PCAATrainer(cfg, device="cuda:0", precision=what)
        for i, m in enumerate((tr.encoder, tr.decoder, tr.discriminator, tr.decoder_projection_head,
                               tr.discriminator_projection_head)):
            syn.deterministic_fill_(m, 30 + i)
        tr.set_prior_means(O.sample_distant_points(32, K, 10, 10).float())
        tr.finalize()
        tr.train()
        tr.step(x, syn.synthetic_labels(B, K, seed=2).to("cuda:0"), syn.synthetic_z0(B, 32, seed=3).to("cuda:0"),
                syn.synthetic_alphas(B, seed=4).to("cuda:0"))
    torch.cuda.synchronize()
    print("\n".join(rec.calls))


if __name__ == "__main__":
    main(sys.argv[1])
