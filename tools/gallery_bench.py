"""What run-time enrolment costs a live tick: one MultiStreamScorer.push at 64 streams with and without a gallery.

    python tools/gallery_bench.py [--out profiles/gallery.txt]

N = 128, C = 4, K = 8, bf16 mode, ``hop`` = 6 new frames per stream per tick, every stream warmed until it emits one window
per tick (the bed of tools/multi_stream_bench.py).  Four scorers on the same encoder and the same frames:
  none    no gallery: the route before galleries existed (pcaa_stream_score), the baseline
  empty   a gallery with no identity, history = 8 (pcaa_stream_score_gallery scans no slot)
  64      a gallery of 64 identities, history = 8
  1024    a gallery of 1 024 identities, history = 8
alternated in one process: WINDOWS windows of TICKS ticks each, per window the time between two device events and the host
wall time to a synchronise, both per tick; medians and spreads ((max - min) / median over the windows); the ratio of each
configuration's median to the baseline's.  Then ``ops.gallery_score`` alone at B = 1 024 windows for 0, 64 and 1 024 slots
against ``inference.joint_likelihood`` on the same windows, alternated in the same way.  The identities are centroids of
random embeddings near the prior means; recognition accuracy is not measured here (the data set is not available).
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opensetgaitrecognition_pcaa_amd import constants, functional as F_hip, inference, models, ops, synthetic as syn  # noqa: E402
from opensetgaitrecognition_pcaa_amd.gallery import Gallery  # noqa: E402

S, N, C, K, KVOTE, D, HIST = 64, 128, 4, 8, 4, 32, 8
SLOTS = (0, 64, 1024)
B_SCORE = 1024


def make_encoder():
    constants.NFEATURES = C
    enc = models.CGEncoder(K, nmax_points=N, use_projection_head=True).float()
    syn.deterministic_fill_(enc, 0)
    enc = enc.cuda().eval()
    means = (torch.randn(K, D, generator=torch.Generator().manual_seed(1)) * 3).cuda()
    return enc, means


def make_gallery(means, slots):
    """``slots`` identities, each enrolled from four embeddings around a point near a prior mean"""
    g = Gallery(D, max(slots, 1), "cuda")
    gen = torch.Generator().manual_seed(7 + slots)
    for e in range(slots):
        centre = means[e % K].cpu() + 2.0 * torch.randn(D, generator=gen)
        g.enrol((centre + 0.3 * torch.randn(4, D, generator=gen)).cuda().contiguous())
    assert len(g) == slots and g.high_water == slots
    return g


class Bed:
    """the four scorers over the same S tracks, all warmed to one window per stream per tick"""

    def __init__(self, enc, means, n_ticks):
        T, hop = constants.NSTEPS, constants.CROP_STEP
        self.hop, self.warm = hop, T + hop * 3
        F = self.warm + hop * n_ticks
        gen = torch.Generator().manual_seed(100 + S)
        base = syn.synthetic_pcs(1, F, N, C, seed=5)[0]
        tracks = [(base.roll(7 * s, 0) + 0.01 * torch.randn(base.shape, generator=gen)).contiguous().cuda() for s in range(S)]
        self.ticks = [torch.cat([t[p:p + hop] for t in tracks]) for p in range(self.warm, F, hop)]
        self.scorers, self.pos = {}, {}
        for name in ("none",) + tuple("empty" if n == 0 else str(n) for n in SLOTS):
            kw = {} if name == "none" else dict(gallery=make_gallery(means, 0 if name == "empty" else int(name)), history=HIST)
            ms = inference.MultiStreamScorer(enc, means, 0.0, KVOTE, K, max_streams=S, **kw)
            self.sids = [ms.open() for _ in range(S)]
            for a in range(0, self.warm, 32):
                b = min(a + 32, self.warm)
                ms.push(self.sids, [b - a] * S, torch.cat([t[a:b] for t in tracks]))
            self.scorers[name], self.pos[name] = ms, 0

    def tick(self, name):
        out = self.scorers[name].push(self.sids, [self.hop] * S, self.ticks[self.pos[name]])
        self.pos[name] += 1
        return out


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, (time.perf_counter() - t0) * 1e3 / reps, out


def report(say, names, rec, base, unit):
    med = {}
    for name in names:
        for kind, vals in zip(("device events", "host wall"), rec[name]):
            m = statistics.median(vals)
            med[name, kind] = m
            say(f"  {name:>5s} {kind:13s}: " + " ".join(f"{v:.4f}" for v in vals)
                + f"   median {m:.4f} {unit}  spread {100 * (max(vals) - min(vals)) / m:.1f} %")
    for name in names:
        if name != base:
            say(f"  {name:>5s} / {base}: device events {med[name, 'device events'] / med[base, 'device events']:.3f}x, "
                f"host wall {med[name, 'host wall'] / med[base, 'host wall']:.3f}x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gallery_bench: needs the GPU; nothing is measured without one")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    enc, means = make_encoder()
    F_hip.set_precision("bf16")
    say(f"gallery_bench: one MultiStreamScorer.push at S={S} streams, N={N} C={C} K={K} bf16, {constants.CROP_STEP} new frames "
        f"per stream per tick (one new window per stream), history={HIST} with a gallery, {torch.cuda.get_device_name(0)}")
    say(f"configurations alternated in one process, {args.windows} windows of {args.ticks} ticks, ms per tick; spread = "
        "(max - min) / median over the windows")
    bed = Bed(enc, means, 4 + args.windows * args.ticks)
    names = list(bed.scorers)
    for _ in range(4):                                        # every shape warmed; the last warm tick is compared
        outs = {name: bed.tick(name) for name in names}
    base = outs["none"]
    same = torch.equal(outs["empty"].lik, base.lik) and torch.equal(outs["empty"].preds, base.preds) and \
        torch.equal(outs["empty"].votes, base.votes)
    say(f"empty gallery against no gallery on the same tick: {'the same bits' if same else 'DIFFERENT'}")
    for name in names[2:]:
        moved = (outs[name].preds != base.preds).float().mean().item()
        say(f"gallery of {name}: {100 * moved:.1f} % of the tick's windows carry an enrolled identity's label")
    rec = {name: ([], []) for name in names}
    for _ in range(args.windows):
        for name in names:
            d, h, _ = timed(lambda: bed.tick(name), args.ticks)
            rec[name][0].append(d)
            rec[name][1].append(h)
    report(say, names, rec, "none", "ms")
    assert all(ms.scatter_err.item() == 0 for ms in bed.scorers.values())

    say(f"ops.gallery_score alone, B={B_SCORE} windows, D={D}, Kc={K}, against inference.joint_likelihood (us per call, "
        f"{args.windows} windows of {10 * args.ticks} calls)")
    gen = torch.Generator().manual_seed(3)
    x = (means[torch.arange(B_SCORE) % K].cpu() + torch.randn(B_SCORE, D, generator=gen)).cuda().contiguous()
    preds = (torch.arange(B_SCORE) % K).cuda()
    fns = {"jl": lambda: inference.joint_likelihood(x, means)}
    for n in SLOTS:
        g = make_gallery(means, n)
        fns[str(n)] = (lambda g: lambda: g.score(x, preds, means, K))(g)
    for fn in fns.values():
        for _ in range(5):
            fn()
    rec = {name: ([], []) for name in fns}
    for _ in range(args.windows):
        for name, fn in fns.items():
            d, h, _ = timed(fn, 10 * args.ticks)
            rec[name][0].append(1e3 * d)
            rec[name][1].append(1e3 * h)
    report(say, list(fns), rec, "jl", "us")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
