"""A/B of the OR-CED step's triplet route on one MI355X: eager ``orced_losses`` + backward + fused Adam with
``triplet="aten"`` (the torch restatement: sorts, cdist, boolean gathers, host synchronisations) against
``triplet="hip"`` (pcaa_orced_triplet), in one process, the routes alternating.

    python tools/orced_triplet_ab.py [--B 64 --N 128 --K 6 --warmup 5 --steps 20 --repeats 3] [--out FILE]
    python tools/orced_triplet_ab.py --route hip --warmup 0 --steps 10      # one route only: for a kernel trace

Prints (and appends to --out) one line per repeat and the medians; times are host clock around synchronised windows.
Launch counts come from two traced runs of one route with different --steps (their difference over the difference of
the step counts), e.g.  rocprofv3 --kernel-trace --stats -d DIR -- python tools/orced_triplet_ab.py --route hip --steps 10"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from opensetgaitrecognition_pcaa_amd import constants, models, orced, synthetic as syn  # noqa: E402
from opensetgaitrecognition_pcaa_amd.train import FlatBuffer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--K", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--route", choices=("both", "aten", "hip"), default="both")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("orced_triplet_ab: needs the GPU (there is no CPU path to time)")
    dev, C, T = "cuda", 4, constants.NSTEPS
    constants.NFEATURES = C
    enc = models.ORCEDEncoder(a.K, nmax_points=a.N).float()
    dec = models.ORCEDDecoder(nmax_points=a.N).float()
    gml = models.GaussianMeanLearner(a.K).float()
    for i, m in enumerate((enc, dec, gml)):
        syn.deterministic_fill_(m, 80 + i)
        m.to(dev).train()
    named = [("E." + n, p) for n, p in enc.named_parameters()]
    named += [("G." + n, p) for n, p in dec.named_parameters() if n.startswith("dense")]
    named += [("ML." + n, p) for n, p in gml.named_parameters()]
    flat = FlatBuffer(named, dev)
    for name, p in named:
        p.grad = flat.grad_views[name]
    pcs = syn.synthetic_pcs(a.B, T, a.N, C, seed=140).to(dev).permute(0, 3, 1, 2)
    gt = syn.synthetic_labels(a.B, a.K, seed=240).to(dev)
    cfg = dict(TRAIN_CLASSES=list(range(a.K)), REC_W=1.0, CE_W=1.0, KL_W=1.0, TRIPLET_W=1.0, TRIPLET_MARGIN=0.5)
    chamfer = orced.SeqChamferLoss()

    def step(route):
        out = orced.orced_losses(enc, dec, gml, pcs, gt, cfg, 0.5, chamfer, triplet=route)
        out["tot"].backward()
        flat.adam(1e-4, 0.9, 0.9)
        flat.g.zero_()
        return out

    def window(route):
        for _ in range(a.warmup):
            step(route)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            out = step(route)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps * 1e3, float(out["trip"].detach())

    routes = ("aten", "hip") if a.route == "both" else (a.route,)
    lines = [f"orced_triplet_ab B={a.B} N={a.N} K={a.K} warmup={a.warmup} steps={a.steps} repeats={a.repeats} "
             f"device={torch.cuda.get_device_name(0)}"]
    ms = {r: [] for r in routes}
    for rep in range(a.repeats):
        for r in routes:
            t, trip = window(r)
            ms[r].append(t)
            lines.append(f"repeat {rep} {r:4s} {t:8.3f} ms/step  trip {trip:.6f}")
    for r in routes:
        lines.append(f"median {r:4s} {statistics.median(ms[r]):8.3f} ms/step  spread (max - min) {max(ms[r]) - min(ms[r]):.3f} ms")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
