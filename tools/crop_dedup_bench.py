"""Scoring STORED crops and processed tracks without their padding: ``dedup_points`` of ``OpenSetScorer.embed`` /
``embed_track`` against the padded path, with and without ``dedup_frames``.

    python tools/crop_dedup_bench.py [--out profiles/frame_unique.txt] [--parent FILE]
    python tools/crop_dedup_bench.py --legs off --out FILE       # only code the parent commit has: run it on a checkout of it

N = 128, C = 4, K = 8.  Data sets:
  * ``raw P``: one synthetic raw track (``synthetic_raw_track(..., max_points=P)``, P = 40, 100, 250) of NSTEPS + 6 * 1 024
    frames, padded on the host as ``process_track`` pads it (``datasets.draw_picks`` / ``frames_from_picks``), its 1 024
    hop-6 crops materialised on the device.  P = 40 is the case the evaluation meets (a few dozen detections, N = 128);
    100 and 250 bracket the break-even;
  * ``no duplicates``: ``synthetic_pcs`` crops and a ``synthetic_pcs`` track: every row distinct, no frame shared.  It
    prices the option where it cannot pay: the count pass, the copy of the offsets, the unfused pool.
Legs, in bf16 and fp32: ``embed`` of the crops under the four combinations of ``dedup_frames`` x ``dedup_points``,
``embed_track`` of the track with ``dedup_points`` off and on.  5 warm-up calls per leg, then REPS (>= 20) rounds in which
every leg is timed once (alternated: drift hits all legs alike), each call between two HIP events; the median and the spread
((max - min) / median).  Next to each time: the rows the PointNet block ran against frames x N.  The offsets pass with its
copy and the write pass are also timed alone.  ``--parent FILE`` (the ``--legs off`` output of the parent commit) adds each
leg's ratio to the PARENT's padded path; without it the ratio is to this build's.  The break-even duplicate share of a mode is
interpolated linearly in the duplicate share between the two measured data sets around it.
"""
import argparse
import os
import re
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from multi_stream_bench import C, K, N, make_encoder  # noqa: E402
from opensetgaitrecognition_pcaa_amd import constants, datasets, functional as F_hip, inference, ops, synthetic as syn  # noqa: E402

CROPS = 1024
WARMUP = 5
RAW_MAX_POINTS = (40, 100, 250)


def raw_data(max_points):
    """-> (name, track [F, N, C] on the device, its CROPS hop-6 crops [CROPS, C, T, N], duplicate share of the track's rows)"""
    T, hop = constants.NSTEPS, constants.CROP_STEP
    F = T + hop * CROPS
    raw = syn.synthetic_raw_track(4242, F, max_points=max_points)
    cards = np.array([len(fr["z_coord"]) for fr in raw])
    np.random.seed(max_points)
    picks = datasets.draw_picks(cards, N)
    track = torch.from_numpy(datasets.frames_from_picks(raw, picks, C).astype(np.float32)).cuda()
    assert inference.window_count(F) == CROPS
    idx = (hop * torch.arange(CROPS, device="cuda"))[:, None] + torch.arange(T, device="cuda")[None, :]
    crops = track[idx].contiguous().permute(0, 3, 1, 2)                   # point-major [CROPS, T, N, C] storage
    U = (CROPS - 1) * hop + T
    return f"raw {max_points}", track, crops, 1.0 - float(np.minimum(cards[:U], N).sum()) / (U * N)


def distinct_data():
    T, hop = constants.NSTEPS, constants.CROP_STEP
    crops = syn.synthetic_pcs(CROPS, T, N, C, seed=7).cuda().permute(0, 3, 1, 2)
    track = syn.synthetic_pcs(1, T + hop * CROPS, N, C, seed=8)[0].cuda().contiguous()
    return "no duplicates", track, crops, 0.0


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def run_legs(legs, reps):
    """{name: callable} -> {name: [ms] * reps}: WARMUP calls each, then every leg once per round"""
    for fn in legs.values():
        for _ in range(WARMUP):
            fn()
    rec = {name: [] for name in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            rec[name].append(event_ms(fn))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--legs", choices=("all", "off"), default="all")
    ap.add_argument("--parent", default=None, metavar="FILE", help="the --legs off output of the parent commit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("--reps: the median of at least 20")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    parent = {}
    if args.parent:
        for line in open(args.parent):
            m = re.match(r"\s*leg \[(.+?)\] median ([0-9.]+) ms", line)
            if m:
                parent[m.group(1)] = float(m.group(2))
    on = args.legs == "all"
    enc, means = make_encoder()
    sc = inference.OpenSetScorer(enc, means)
    T, hop = constants.NSTEPS, constants.CROP_STEP
    say(f"crop_dedup_bench --legs {args.legs}: N={N} C={C} K={K}, {torch.cuda.get_device_name(0)}; {CROPS} hop-{hop} crops "
        f"of one track ({CROPS * T} crop frames, {(CROPS - 1) * hop + T} track frames); {WARMUP} warm-up calls, then the "
        f"median of {args.reps} calls between HIP events, the legs alternated; spread = (max - min) / median")
    say("ratio: time of the " + ("PARENT commit's" if parent else "this build's") + " padded path (embed: dedup_frames "
        "off, dedup_points off; embed_track: dedup_points off) / time of the leg; rows: what the PointNet block ran")
    data = [raw_data(p) for p in RAW_MAX_POINTS] + [distinct_data()]
    points = {}                                               # (mode, entry, frames option) -> [(duplicate share, t_off, t_on)]
    for mode in ("bf16", "fp32"):
        F_hip.set_precision(mode)
        for name, track, crops, share in data:
            say(f"{mode}, {name} (duplicate share of the rows {100 * share:.1f} %):")
            legs, rows = {}, {}
            for frames_opt in (False, True):
                for points_opt in ((False, True) if on else (False,)):
                    key = f"{mode} | {name} | embed dedup_frames={int(frames_opt)} dedup_points={int(points_opt)}"
                    if points_opt:
                        legs[key] = lambda f=frames_opt: sc.embed(crops, dedup_frames=f, dedup_points=True)
                    else:                                     # as the parent commit is called
                        legs[key] = lambda f=frames_opt: sc.embed(crops, dedup_frames=f)
            for points_opt in ((False, True) if on else (False,)):
                key = f"{mode} | {name} | embed_track dedup_points={int(points_opt)}"
                legs[key] = (lambda: sc.embed_track(track, dedup_points=True)) if points_opt else (lambda: sc.embed_track(track))
            for key, fn in legs.items():                      # the rows each leg runs (and one more warm-up)
                sc.last_rows_encoded = sc.last_frames_encoded = None
                fn()
                if "dedup_points=1" in key:
                    rows[key] = sc.last_rows_encoded
                else:
                    rows[key] = (CROPS * T if sc.last_frames_encoded is None else sc.last_frames_encoded) * N
            rec = run_legs(legs, args.reps)
            med = {key: statistics.median(v) for key, v in rec.items()}
            for key, v in rec.items():
                base_key = re.sub(r"dedup_(frames|points)=1", r"dedup_\1=0", key)
                base = parent.get(base_key, med[base_key])
                padded_rows = rows[base_key]
                say(f"  leg [{key}] median {med[key]:.3f} ms  spread {100 * (max(v) - min(v)) / med[key]:.1f} %  min "
                    f"{min(v):.3f}  ratio {base / med[key]:.2f}x  rows {rows[key]} of {padded_rows} "
                    f"({padded_rows / rows[key]:.2f}x fewer)")
            if on:
                for entry, off_key, on_key in (
                        ("embed", "embed dedup_frames=0 dedup_points=0", "embed dedup_frames=0 dedup_points=1"),
                        ("embed + dedup_frames", "embed dedup_frames=1 dedup_points=0", "embed dedup_frames=1 dedup_points=1"),
                        ("embed_track", "embed_track dedup_points=0", "embed_track dedup_points=1")):
                    points.setdefault((mode, entry), []).append(
                        (share, med[f"{mode} | {name} | {off_key}"], med[f"{mode} | {name} | {on_key}"]))
                # the two passes of the front alone, on the crops' frames and on the track's
                for what, frames in (("crop frames", F_hip._point_major(crops).view(CROPS * T, N, C)),
                                     ("track frames", track[:(CROPS - 1) * hop + T])):
                    u_off = ops.frames_unique_offsets(frames)
                    M = ops.unique_chunk_rows(int(u_off[-1]))
                    out = (torch.empty((M, C), device="cuda"), torch.empty(M, device="cuda"))
                    alone = run_legs({"offsets + copy": lambda: ops.frames_unique_offsets(frames).cpu(),
                                      "offsets": lambda: ops.frames_unique_offsets(frames),
                                      "write": lambda: ops.frames_unique(frames, u_off, M=M, out=out)}, args.reps)
                    say(f"  front alone, {frames.shape[0]} {what} -> {int(u_off[-1])} rows: " + ", ".join(
                        f"{k} {statistics.median(v):.3f} ms" for k, v in alone.items())
                        + f"; a rank scratch would hold {frames.shape[0] * N * 4 / 2 ** 20:.1f} MiB")
    if on:
        say("break-even: the smallest duplicate share at which dedup_points=True is faster than the same call without it "
            "(linear in the share between the two measured data sets around the crossing):")
        for (mode, entry), pts in points.items():
            pts.sort()
            gains = [(s, t_off / t_on) for s, t_off, t_on in pts]
            text = ", ".join(f"{100 * s:.0f} %: {g:.2f}x" for s, g in gains)
            cross = None
            for (s0, g0), (s1, g1) in zip(gains, gains[1:]):
                if g0 < 1.0 <= g1:
                    cross = s0 + (1.0 - g0) * (s1 - s0) / (g1 - g0)
            verdict = ("wins at every measured share" if gains[0][1] >= 1.0 else
                       "loses at every measured share" if cross is None else f"break-even at about {100 * cross:.0f} %")
            say(f"  {mode} {entry}: off / on at duplicate share {text} -> {verdict}")
    assert sc.unique_err.item() == 0 if on else True
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
