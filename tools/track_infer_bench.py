"""Open-set inference on one long track: the crop path against the frame-deduplicated paths.

    python tools/track_infer_bench.py [--out profiles/track_infer.txt]

N = 128, C = 4, K = 8, bf16 mode, one synthetic track of 6 168 frames = 1 024 aligned windows of 30 frames with a hop of 6
(the inference leg's configuration with real overlap), resident in HBM.  Three paths, alternated in one process:
  (a) OpenSetScorer.embed on the 1 024 materialised crops              -- the baseline, every crop frame encoded
  (b) OpenSetScorer.embed(dedup_frames=True) on the same crops         -- overlap detection and planning included
  (c) OpenSetScorer.embed_track on the track (drop_last_aligned=False: the same 1 024 windows)
Device events around CALLS calls that end in a synchronise; 2 warm-up rounds, then WINDOWS windows per path; medians and
the spread of (a) over its windows.  Then the per-push latency of StreamingScorer for 6 new frames (one new window).
Derived bound: (c) does (30 + 6 * 1023) / (30 * 1024) = 0.2008 of (a)'s per-point arithmetic, so at most 4.98x.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opensetgaitrecognition_pcaa_amd import constants, functional as F_hip, inference, models, synthetic as syn  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--pushes", type=int, default=200)
    ap.add_argument("--n-windows", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, C, K, T, hop, W = 128, 4, 8, constants.NSTEPS, constants.CROP_STEP, args.n_windows
    F = T + hop * (W - 1)
    dev = "cuda"
    constants.NFEATURES = C
    enc = models.CGEncoder(K, nmax_points=N, use_projection_head=True).float()
    syn.deterministic_fill_(enc, 0)
    enc = enc.to(dev).eval()
    means = (torch.randn(K, 32, generator=torch.Generator().manual_seed(1)) * 3).to(dev)
    track = syn.synthetic_pcs(1, F, N, C, seed=5)[0].contiguous().to(dev)
    crops = torch.stack([track[s:s + T] for s in range(0, F - T + 1, hop)]).permute(0, 3, 1, 2)     # [W,C,T,N] view
    assert crops.shape[0] == W
    F_hip.set_precision("bf16")
    scorer = inference.OpenSetScorer(enc, means, batch_size=1024)
    paths = {"a": lambda: scorer.embed(crops),
             "b": lambda: scorer.embed(crops, dedup_frames=True),
             "c": lambda: scorer.embed_track(track, drop_last_aligned=False)}
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"track_infer_bench: N={N} C={C} K={K} bf16, track of {F} frames = {W} windows (T={T}, hop={hop}), "
        f"{torch.cuda.get_device_name(0)}")
    ref = paths["a"]()
    for name in ("b", "c"):
        got = paths[name]()
        agree = (got[0] == ref[0]).float().mean().item()
        err = ((got[1] - ref[1]).abs().max() / ref[1].abs().max()).item()
        say(f"  ({name}) against (a): labels agree {agree:.4f}, embedding difference {err:.2e} of scale, "
            f"frames encoded {scorer.last_frames_encoded} of {W * T}")
    for _ in range(2):
        for fn in paths.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for _ in range(args.windows):
        for name, fn in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.calls)
    med = {k: statistics.median(v) for k, v in ms.items()}
    for name in paths:
        say(f"  ({name}) ms per call, {args.windows} windows of {args.calls} calls: "
            + " ".join(f"{v:.3f}" for v in ms[name]) + f"   median {med[name]:.3f}")
    spread = (max(ms["a"]) - min(ms["a"])) / med["a"]
    say(f"  spread of (a) over its windows: {100 * spread:.2f} % of its median")
    bound = (W * T) / (T + hop * (W - 1))
    say(f"  (a)/(b) = {med['a'] / med['b']:.2f}x   (a)/(c) = {med['a'] / med['c']:.2f}x   derived bound {bound:.2f}x "
        f"(work ratio {1 / bound:.4f})")
    say(f"  windows per second: (a) {W / med['a'] * 1e3:.0f}  (b) {W / med['b'] * 1e3:.0f}  (c) {W / med['c'] * 1e3:.0f}")

    # ---- streaming: 6 new frames = one new window per push
    stream = inference.StreamingScorer(enc, means, 0.0, 4, K)
    stream.push(track[:T + 6 * 8])
    pos = T + 6 * 8
    dev_ms, host_ms = [], []
    for i in range(args.pushes):
        chunk = track[pos:pos + hop]
        pos = pos + hop if pos + 2 * hop <= F else 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = stream.push(chunk)
        e1.record()
        torch.cuda.synchronize()
        host_ms.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(e0.elapsed_time(e1))
        assert out[0].shape[0] == 1
    say(f"  StreamingScorer.push of {hop} frames (one new window), median of {args.pushes}: "
        f"{statistics.median(dev_ms):.3f} ms between device events, {statistics.median(host_ms):.3f} ms host wall time "
        f"to the synchronise")
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            stream.push(track[:hop])
            torch.cuda.synchronize()
        n = sum(e.count for e in prof.key_averages() if getattr(e, "device_type", None) is not None
                and "cuda" in str(e.device_type).lower())
        say(f"  launches per push (device activities the profiler saw, copies included): {n}")
    except Exception as exc:       # the count is a convenience; the timings above do not depend on it
        say(f"  launches per push: not counted ({type(exc).__name__}: {exc})")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
