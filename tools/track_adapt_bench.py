"""One adaptation step of the frozen-BatchNorm encoder (``params="all"``) on the same walks, three ways:

  (a) crops   -- the walks' hop-6 crops written out, through ``adapt.finetune_frozen_bn``: every frame encoded once per
                 window it lies in (NSTEPS / hop = 5 times), every repeated detection once per copy;
  (b) tracks  -- ``adapt.finetune_frozen_bn_tracks``: every frame once, the walks in one PointNet pass and one temporal
                 pass, the window gradients overlap-added;
  (c) tracks, ``dedup_points=True`` -- every frame's DISTINCT detections once, pooled with their multiplicities.

    python tools/track_adapt_bench.py [--out profiles/track_backward.txt]

N = 128, C = 4, K = 8, bf16 and fp32.  Walks: synthetic raw tracks of FRAMES = 150 frames with 3 .. 40 and 3 .. 150
detections per frame, padded on the host as ``process_track`` pads them; 1 and 4 walks per step (a single walk shows the
launch-bound end).  A step is forward, loss, backward and one Adam update with lr = 0 (the parameters keep their bits, so
every call does the same work).  5 warm-up calls per leg, then REPS (>= 20) rounds in which every leg is timed once
(alternated: drift hits all legs alike), each call between two HIP events and, around them, the host wall time to the
call's end (the call ends with the loss on the host); medians and the spread ((max - min) / median).  Next to each leg:
the point rows its PointNet block runs per step, and what one step launches: the calls into the HIP library, and the
device activities (kernels, memsets, copies) torch's profiler records for one step, where it records any.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from multi_stream_bench import C, K, N, make_encoder  # noqa: E402
from opensetgaitrecognition_pcaa_amd import _lib, adapt, constants, datasets, functional as F_hip, ops, synthetic as syn  # noqa: E402

FRAMES = 150
WARMUP = 5
MAX_POINTS = (40, 150)
WALKS = (1, 4)


def make_walks(n, max_points):
    """-> (tracks [F, N, C] on the device, their crops [W_total, C, T, N], window labels, walk labels, detections / frame)"""
    T, hop = constants.NSTEPS, constants.CROP_STEP
    tracks, crops, cards_all = [], [], []
    for i in range(n):
        raw = syn.synthetic_raw_track(9000 + 10 * max_points + i, FRAMES, max_points=max_points)
        cards = np.array([len(fr["z_coord"]) for fr in raw])
        np.random.seed(max_points + i)
        track = torch.from_numpy(datasets.frames_from_picks(raw, datasets.draw_picks(cards, N), C).astype(np.float32)).cuda()
        W, _ = F_hip.track_windows(FRAMES, T, hop)
        idx = (hop * torch.arange(W, device="cuda"))[:, None] + torch.arange(T, device="cuda")[None, :]
        tracks.append(track)
        crops.append(track[idx])
        cards_all.append(cards)
    walk_labels = torch.arange(n, device="cuda") % K
    W = crops[0].shape[0]
    crops = torch.cat(crops).contiguous().permute(0, 3, 1, 2)              # point-major [W_total, T, N, C] storage
    return tracks, crops, walk_labels.repeat_interleave(W).contiguous(), walk_labels, np.concatenate(cards_all)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


class LibraryCalls:
    """counts the calls into libpcaa_hip.so while it is active (a call is one launch, a few of them two)"""

    def __init__(self):
        self.lib, self.n, self.saved = _lib.load(), 0, {}

    def __enter__(self):
        for name in _lib.parse_header():
            fn = getattr(self.lib, name)
            self.saved[name] = fn

            def counted(*a, _fn=fn):
                self.n += 1
                return _fn(*a)

            setattr(self.lib, name, counted)
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.lib, name, fn)
        return False


def device_activities(fn):
    """kernels + memsets + copies torch's profiler records for one call; None where it records nothing"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception:                                        # a profiler that is not there is no reason to lose the timings
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("--reps: the median of at least 20")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    T, hop = constants.NSTEPS, constants.CROP_STEP
    enc, _ = make_encoder()
    W, U = F_hip.track_windows(FRAMES, T, hop)
    say(f"track_adapt_bench: one params='all' adaptation step (forward, loss, backward, Adam with lr = 0), N={N} C={C} K={K}, "
        f"{torch.cuda.get_device_name(0)}; walks of {FRAMES} frames = {W} hop-{hop} windows over {U} frames each; {WARMUP} "
        f"warm-up calls, then the median of {args.reps} calls, the legs alternated; spread = (max - min) / median; device = "
        "between two HIP events, wall = host time to the end of the call")
    say("ratio: time of leg (a) / time of the leg; rows: point rows through the PointNet block per step")
    for mode in ("bf16", "fp32"):
        F_hip.set_precision(mode)
        for max_points in MAX_POINTS:
            for n in WALKS:
                tracks, crops, win_labels, walk_labels, cards = make_walks(n, max_points)
                distinct = sum(ops.unique_chunk_rows(int(ops.frames_unique_offsets(t[:U])[-1])) for t in tracks)
                rows = {"a crops": n * W * T * N, "b tracks": n * U * N, "c tracks dedup_points": distinct}
                legs = {"a crops": lambda: adapt.finetune_frozen_bn(enc, crops, win_labels, 1, 0.0, params="all"),
                        "b tracks": lambda: adapt.finetune_frozen_bn_tracks(enc, tracks, walk_labels, 1, 0.0, params="all"),
                        "c tracks dedup_points": lambda: adapt.finetune_frozen_bn_tracks(
                            enc, tracks, walk_labels, 1, 0.0, params="all", dedup_points=True)}
                say(f"{mode}, 3..{max_points} detections per frame (mean {cards.mean():.1f}; N / min(card, N) = "
                    f"{N / np.minimum(cards, N).mean():.2f}), {n} walk(s) = {n * W} windows per step:")
                losses, calls, acts = {}, {}, {}
                for name, fn in legs.items():
                    for _ in range(WARMUP):
                        losses[name] = fn()[0]
                    with LibraryCalls() as lc:
                        fn()
                    calls[name] = lc.n
                    acts[name] = device_activities(fn)
                rec = {name: [] for name in legs}
                for _ in range(args.reps):
                    for name, fn in legs.items():
                        rec[name].append(timed(fn))
                med = {name: (statistics.median(d for d, _ in v), statistics.median(w for _, w in v)) for name, v in rec.items()}
                for name, v in rec.items():
                    dev = [d for d, _ in v]
                    say(f"  leg [{mode} | 3..{max_points} | {n} walks | {name}] device {med[name][0]:.3f} ms  spread "
                        f"{100 * (max(dev) - min(dev)) / med[name][0]:.1f} %  min {min(dev):.3f}  wall {med[name][1]:.3f} ms  "
                        f"ratio {med['a crops'][0] / med[name][0]:.2f}x  rows {rows[name]} ({rows['a crops'] / rows[name]:.2f}x "
                        f"fewer)  library calls {calls[name]}  device activities "
                        f"{acts[name] if acts[name] is not None else 'n/a'}  loss {losses[name]:.6f}")
                say(f"  device memory held after the legs: {torch.cuda.memory_allocated() / 2 ** 30:.2f} GiB")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
