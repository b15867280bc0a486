"""Thinned raw frames (``keep`` / ``keep_points``): what the stage costs in the kernels and what a sweep point costs.

    python tools/point_sweep_bench.py [--out profiles/point_sweep.txt]

N = 128, C = 4, K = 8, bf16 mode, raw frames of 3 .. 200 detections.  HIP events around each call, 5 warm-up calls, medians
of 20 calls, the legs of a comparison alternated in one process; spread = (max - min) / median.
  1. the three kernels alone (``ops.frames_from_raw``, ``crops_from_raw``, ``frames_from_raw_unique``) on a store of 64
     tracks x 240 frames at keep 0 (the entry points without the stage), 10, 20, 50, both rules;
  2. ``MultiStreamScorer.push_raw`` at 64 streams, 6 new frames per stream per tick, keep_points 0 / 20, padded and
     ``dedup_points``;
  3. ``inference.point_sweep`` over keep 10, 20, 50, 100, N on a store of 10 subjects x 10 tracks of 60 frames, with and
     without ``dedup_points`` (one k, so the time is the embedding's).
The keep = 0 calls against the parent commit are measured by ``tools/raw_ingest_bench.py`` / ``tools/raw_batcher_bench.py``
run on both commits in one job; this tool does not build the parent."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from multi_stream_bench import C, K, KVOTE, N, make_encoder  # noqa: E402
from opensetgaitrecognition_pcaa_amd import constants, datasets, functional as F_hip, inference, ops, synthetic as syn  # noqa: E402
from opensetgaitrecognition_pcaa_amd.constants import SPLIT  # noqa: E402

MAX_POINTS = 200
WARM, CALLS = 5, 20
KEEPS = (0, 10, 20, 50)
RULES = ("first", "random")


def timed(legs):
    """legs: {name: callable} -> {name: (median ms, spread)}: WARM untimed rounds, then CALLS rounds, the legs alternated"""
    ms = {name: [] for name in legs}
    for r in range(WARM + CALLS):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= WARM:
                ms[name].append(a.elapsed_time(b))
    return {name: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for name, v in ms.items()}


def kernels(lines):
    tracks = [syn.synthetic_raw_track(5000 + i, 240, max_points=MAX_POINTS) for i in range(64)]
    st = datasets.RawTrackStore(tracks, [i % 8 for i in range(64)], ["free_walk"] * 64, [str(i) for i in range(64)]).to_device()
    F, P = st.n_frames, st.points.shape[0]
    start = torch.from_numpy(np.random.default_rng(0).integers(0, F - constants.NSTEPS, 64).astype(np.int32)).cuda()
    lines.append(f"part 1: the kernels alone, a store of 64 tracks x 240 frames, {P} detections (3 .. {MAX_POINTS} a frame), N = {N}, "
                 f"C = {C}; frames / unique: all {F} frames, crops: B = 64 x T = {constants.NSTEPS}; ms, median of {CALLS} (spread)")
    raw = (st.points_dev, st.offsets_dev)
    for rule in RULES:
        legs = {}
        for keep in KEEPS:
            kw = dict(seed=3, frame_key=st.frame_key_dev, keep=keep, keep_rule=rule)
            legs[("frames", keep)] = lambda kw=kw: ops.frames_from_raw(*raw, N, C, **kw)
            legs[("crops", keep)] = lambda kw=kw: ops.crops_from_raw(*raw, start, constants.NSTEPS, N, C, **kw)
            legs[("unique", keep)] = lambda kw=kw: ops.frames_from_raw_unique(*raw, N, C, **kw)
        res = timed(legs)
        for what in ("frames", "crops", "unique"):
            lines.append(f"  {rule:6s} {what:6s} " + "  ".join(
                f"keep {keep:3d}: {res[(what, keep)][0]:7.3f} ({res[(what, keep)][1]:4.0%})" for keep in KEEPS))


def ticks(lines, enc, means):
    S, hop, T = 64, constants.CROP_STEP, constants.NSTEPS
    warm = T + 3 * hop
    tracks = [syn.synthetic_raw_track(7000 + s, warm + hop, max_points=MAX_POINTS) for s in range(S)]
    lines.append(f"part 2: MultiStreamScorer.push_raw, {S} streams x {hop} new frames a tick, every stream emitting one window; "
                 f"ms a tick, median of {CALLS} (spread); the tick is replayed on a copy of the warmed state's counters")
    legs = {}
    for keep in (0, 20):
        for dedup in (False, True):
            ms = inference.MultiStreamScorer(enc, means, 0.0, KVOTE, K, max_streams=S, seed=1, dedup_points=dedup,
                                             keep_points=keep, keep_rule="random")
            sids = [ms.open() for _ in range(S)]
            for a in range(0, warm, 32):
                b = min(a + 32, warm)
                p, o = datasets.pack_raw_frames([fr for t in tracks for fr in t[a:b]])
                ms.push_raw(sids, [b - a] * S, p.cuda(), o.cuda())
            p, o = datasets.pack_raw_frames([fr for t in tracks for fr in t[warm:warm + hop]])
            p, o = p.cuda(), o.cuda()
            state = (ms.n_frames.copy(), ms.n_windows.copy())

            def tick(ms=ms, sids=sids, p=p, o=o, state=state):
                ms.n_frames[:], ms.n_windows[:] = state
                ms.push_raw(sids, [hop] * S, p, o)
            legs[(keep, dedup)] = tick
    res = timed(legs)
    for (keep, dedup), (med, spread) in res.items():
        lines.append(f"  keep_points {keep:3d} {'dedup_points' if dedup else 'padded      '}: {med:7.3f} ({spread:4.0%})")


def sweep(lines, enc, means):
    tracks, subj, names = [], [], []
    for s in range(10):
        for t in range(10):
            tracks.append(syn.synthetic_raw_track(9000 + 10 * s + t, 60, max_points=MAX_POINTS))
            subj.append(s)
            names.append(f"{t}{s}")
    st = datasets.RawTrackStore(tracks, subj, ["hands_in_pockets"] * 100, names)
    st.assign_like_generate_splits(list(range(K)), seed=0).to_device()
    lines.append(f"part 3: inference.point_sweep, 10 subjects x 10 tracks of 60 frames (3 .. {MAX_POINTS} detections), {K} known "
                 f"subjects, one k; ms per keep (TEST + UNSEEN crops built and embedded once), median of {CALLS} (spread)")
    keeps = (10, 20, 50, 100, N)
    legs = {(keep, dedup): (lambda keep=keep, dedup=dedup: inference.point_sweep(enc, means, st, [keep], [2], N, dedup_points=dedup))
            for keep in keeps for dedup in (False, True)}
    res = timed(legs)
    for dedup in (False, True):
        lines.append(f"  {'dedup_points' if dedup else 'padded      '} " + "  ".join(
            f"keep {keep:3d}: {res[(keep, dedup)][0]:7.2f} ({res[(keep, dedup)][1]:4.0%})" for keep in keeps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_sweep.txt"))
    args = ap.parse_args()
    F_hip.set_precision("bf16")
    constants.NFEATURES = C
    enc, means = make_encoder()
    lines = [f"tools/point_sweep_bench.py on {torch.cuda.get_device_name(0)}: thinned raw frames; HIP events, {WARM} warm-up calls, "
             f"medians of {CALLS}, legs alternated"]
    kernels(lines)
    ticks(lines, enc, means)
    sweep(lines, enc, means)
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
