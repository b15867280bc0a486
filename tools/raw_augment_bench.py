"""What the augmentation stage of csrc/raw_frames.hip (``augment=``) costs where it runs: in a training batch built by
``RawTrackBatcher.batch`` and in ``OpenSetScorer.embed_raw_track`` of a long track.

    python tools/raw_augment_bench.py [--out profiles/raw_augment.txt]

GPU only.  Three configurations, alternated sample by sample in one process: ``none`` (no ``augment``: the entry points
and kernels without the stage), ``all`` (yaw, mirror, scale, speed and noise on every column) and ``noise`` (noise on
every column, nothing else).  A sample is CALLS calls between two HIP events, after WARM warm-up calls of every leg; the
median and the spread (max - min) / median of SAMPLES samples are reported.
  1. ``RawTrackBatcher.batch(idx)`` (two row gathers and the one ``pcaa_crops_from_raw[_aug]`` launch) at B = 64, N = 128
     and B = 16, N = 150, C = 4, T = 30, on the synthetic store of tools/raw_batcher_bench.py (64 tracks x 240 frames of
     3 .. 200 detections), random crop indices;
  2. ``embed_raw_track`` of one track of 1 024 windows (N = 128, C = 4, K = 8, bf16 mode), padded and ``dedup_points``.
The measurements replace everything from the line "== measurements" on in ``--out``; what stands before it (the kernels'
resource listing) is kept."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from opensetgaitrecognition_pcaa_amd import batcher, constants, datasets, functional as F_hip, inference, synthetic as syn  # noqa: E402
from opensetgaitrecognition_pcaa_amd.constants import SPLIT  # noqa: E402

SHAPES = ((64, 128), (16, 150))
C, T = 4, constants.NSTEPS
TRACKS, FRAMES, MAX_POINTS = 64, 240, 200                 # the store of tools/raw_batcher_bench.py
WARM, SAMPLES, CALLS, CALLS_TRACK = 20, 12, 200, 200
WINDOWS = 1024
MARK = "== measurements"
NOISE = [0.02, 0.02, 0.03, 0.1, 1.0]
CONFIGS = {"none": None,
           "all": {"yaw": 0.5, "mirror": True, "scale": (0.9, 1.1), "speed": (0.8, 1.25), "noise": NOISE},
           "noise": {"noise": NOISE}}


def samples(legs, calls):
    """{name: fn} -> {name: [ms per call of each sample]}: WARM calls of every leg, then the legs alternated sample by sample"""
    for fn in legs.values():
        for _ in range(WARM):
            fn()
    out = {name: [] for name in legs}
    for _ in range(SAMPLES):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) / calls)
    return out


def report(say, res, unit="ms"):
    med = {k: statistics.median(v) for k, v in res.items()}
    for name, ms in res.items():
        say(f"  {name:<6s} median {med[name]:9.4f} {unit}  spread {100 * (max(ms) - min(ms)) / med[name]:5.1f} %  min {min(ms):9.4f}"
            + ("" if name == "none" else f"  / none = {med[name] / med['none']:.3f}x ({med[name] - med['none']:+.4f} {unit})"))


def batches(say):
    tracks = [syn.synthetic_raw_track(100 + i, FRAMES, max_points=MAX_POINTS) for i in range(TRACKS)]
    store = datasets.RawTrackStore(tracks, [i % 8 for i in range(TRACKS)], ["free_walk"] * TRACKS,
                                   [str(i) for i in range(TRACKS)], splits=["train"] * TRACKS).to_device("cuda")
    cards = store.cards()
    say(f"part 1: RawTrackBatcher.batch(idx), a store of {TRACKS} tracks x {FRAMES} frames, {int(cards.sum())} detections "
        f"({cards.min()} .. {cards.max()} a frame), C = {C}, T = {T}; ms a batch")
    for B, N in SHAPES:
        view = store.crops(SPLIT.TRAIN, N, C)
        idx = torch.randint(0, len(view), (B,), generator=torch.Generator().manual_seed(B)).cuda()
        loaders = {name: batcher.RawTrackBatcher(view, B, seed=1, augment=aug) for name, aug in CONFIGS.items()}
        res = samples({name: (lambda ld=ld: ld.batch(idx)) for name, ld in loaders.items()}, CALLS)
        for ld in loaders.values():
            ld.check()
        say(f" B = {B}, N = {N}: a batch is {B * T} frames = {B * T * N * C * 4 / 2 ** 20:.2f} MiB")
        report(say, res)


def tracks(say):
    from multi_stream_bench import K, N, make_encoder
    F_hip.set_precision("bf16")
    enc, means = make_encoder()
    F = T + constants.CROP_STEP * WINDOWS
    while inference.window_count(F) > WINDOWS:
        F -= 1
    while inference.window_count(F) < WINDOWS:
        F += 1
    raw = syn.synthetic_raw_track(77, F, max_points=MAX_POINTS)
    points, offsets = datasets.pack_raw_frames(raw)
    points, offsets = points.cuda(), offsets.cuda()
    sc = inference.OpenSetScorer(enc, means)
    say(f"part 2: OpenSetScorer.embed_raw_track, one track of {F} frames = {inference.window_count(F)} windows, "
        f"{points.shape[0]} detections, N = {N}, C = {C}, K = {K}, bf16 mode; ms a track")
    for dedup in (False, True):
        legs = {name: (lambda aug=aug: sc.embed_raw_track(points, offsets, seed=3, track_key=5, dedup_points=dedup, augment=aug))
                for name, aug in CONFIGS.items()}
        res = samples(legs, CALLS_TRACK)
        assert int(sc.raw_err.item()) == 0
        say(f" {'dedup_points' if dedup else 'padded'}:")
        report(say, res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw_augment.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("raw_augment_bench: needs the GPU; there is nothing to measure without it")
    constants.NFEATURES = C
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(MARK)
    say(f"tools/raw_augment_bench.py on {torch.cuda.get_device_name(0)}: none / all / noise alternated in one process; {WARM} "
        f"warm-up calls a leg, then {SAMPLES} samples of {CALLS} calls (tracks: {CALLS_TRACK}) between HIP events; median, spread = "
        f"(max - min) / median, min")
    batches(say)
    tracks(say)
    head = ""
    if os.path.exists(args.out):
        with open(args.out) as f:
            head = f.read().split(MARK)[0]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(head + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
