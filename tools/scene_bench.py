"""What splitting scene frames into people costs a live tick: ``SceneSplitter.push`` beside ``MultiStreamScorer.push_raw``
of the same people pre-separated.

    python tools/scene_bench.py [--out profiles/scene_split.txt]

N = 128, C = 4, K = 8, bf16 mode, 6 scene frames a tick, 1, 4 and 16 people in view (``synthetic.synthetic_scene``: 8 - 20
detections per person and frame, 4 clutter detections per frame), every stream warmed until it emits one window per tick.
Per number of people, seven measurements alternated in one process -- WINDOWS windows of TICKS ticks each, medians and
spreads ((max - min) / median over the windows):
  cluster   ``ops.scene_cluster(zero_fill=False)``, the launch the live path makes, on the tick's scene frames: device
            events per call (the launch and the allocation of its six outputs; no fill kernels)
  wait      clustering, the packed copy of the cluster tables and the ONE host wait (``SceneFront.cluster``) on an idle
            device: host wall
  behind    the same while a tick of the second scorer is in flight on the current stream and no ``ready`` event is
            given: the wait covers what is left of that tick (host wall of the wait alone, the tick's enqueue excluded)
  ready     the same with the ``ready`` event of an upload stream: the side stream does not wait for the tick in flight
  associate ``scene.associate`` alone on the tick's cluster tables: host wall, no device work
  push      the whole ``SceneSplitter.push``: device events and host wall to a synchronise, per tick
  push_raw  ``MultiStreamScorer.push_raw`` of the same people's own frames, on a second scorer: the same two clocks
and the ratio push / push_raw.  The last warm tick of the two scorers is compared bit for bit first.
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

from opensetgaitrecognition_pcaa_amd import constants, datasets, functional as F_hip, inference, models, ops, scene  # noqa: E402
from opensetgaitrecognition_pcaa_amd import synthetic as syn  # noqa: E402

N, C, K, KVOTE, D, TICK, EPS, CLUTTER = 128, 4, 8, 4, 32, 6, 0.5, 4
PEOPLE = (1, 4, 16)


def make_encoder():
    constants.NFEATURES = C
    enc = models.CGEncoder(K, nmax_points=N, use_projection_head=True).float()
    syn.deterministic_fill_(enc, 0)
    enc = enc.cuda().eval()
    means = (torch.randn(K, D, generator=torch.Generator().manual_seed(1)) * 3).cuda()
    return enc, means


def dev(raw):
    points, offsets = datasets.pack_raw_frames(raw, torch.float32)
    return points.cuda(), offsets.cuda()


class Bed:
    """a splitter over one scorer and a second scorer fed the people's own frames, both warmed to one window per stream
    per tick; the ticks are resident on the device"""

    def __init__(self, enc, means, people, n_ticks):
        T, hop = constants.NSTEPS, constants.CROP_STEP
        warm = -(-(T + 3 * hop) // TICK)
        scn, persons = syn.synthetic_scene(40 + people, (warm + n_ticks) * TICK, people, CLUTTER, EPS)
        mk = lambda: inference.MultiStreamScorer(enc, means, 0.0, KVOTE, K, max_streams=people, max_push=TICK, seed=3)
        self.ms, self.mf = mk(), mk()
        self.sp = scene.SceneSplitter(self.ms, eps=EPS, min_points=3, confirm=1)
        self.scene_ticks, self.own_ticks, self.pos = [], [], {"push": warm, "push_raw": warm}
        person_of = None
        for t in range(warm + n_ticks):
            frames = scn[t * TICK:(t + 1) * TICK]
            self.scene_ticks.append(dev(frames))
            if t == 0:                                          # which person each track is: by its lane
                st = self.sp.push(*self.scene_ticks[0])
                person_of = {tid: int(round(y / (3.5 * EPS))) for tid, (x, y) in st.positions.items()}
                assert sorted(person_of.values()) == list(range(people)) and st.opened == [(i, i) for i in range(people)]
                self.sids = [self.mf.open() for _ in range(people)]
                self.order = [person_of[tid] for tid in range(people)]
            self.own_ticks.append(dev([fr for k in self.order for fr in persons[k][t * TICK:(t + 1) * TICK]]))
        last = None
        for t in range(warm):
            a = self.sp.push(*self.scene_ticks[t]) if t else st
            b = self.mf.push_raw(self.sids, [TICK] * people, *self.own_ticks[t])
            last = (a.tick, b)
        self.same = all(torch.equal(getattr(last[0], n), getattr(last[1], n)) for n in ("preds", "sup_fv", "lik", "votes"))
        self.windows = len(last[1])
        self.front = scene.SceneFront("cuda", EPS, 3, 0.1, 0.0, 16, self.sp.front.params)
        self.people = people
        # a third scorer that replays one warm tick for the in-flight measurements
        self.replay, self.upload = mk(), torch.cuda.Stream()
        for _ in range(people):
            self.replay.open()
        for t in range(warm - 1):
            self.replay.push_raw(self.sids, [TICK] * people, *self.own_ticks[t])
        self.replay_state = (self.replay.n_frames.copy(), self.replay.n_windows.copy())      # before its last warm tick
        self.replay_tick = self.own_ticks[warm - 1]

    def tick(self, name):
        t = self.pos[name]
        self.pos[name] += 1
        if name == "push":
            return self.sp.push(*self.scene_ticks[t])
        return self.mf.push_raw(self.sids, [TICK] * self.people, *self.own_ticks[t])

    def cluster(self, t):
        p, o = self.scene_ticks[t]
        return ops.scene_cluster(p, o, self.front.eps2, self.front.wz2, self.front.wv2, 3, 16, self.front.err, zero_fill=False)

    def wait(self, t):
        return self.front.cluster(*self.scene_ticks[t])

    def wait_in_flight(self, t, with_ready):
        """host wall (ms) of the front end's wait alone, entered right after a tick of the second scorer was enqueued.
        The scene frames are resident; ``ready`` is an event on the otherwise idle upload stream.  The scorer's tick is
        the last warm tick, replayed by a third scorer whose counters are put back first: one window per stream, as in
        the measured ticks."""
        self.replay.n_frames[:], self.replay.n_windows[:] = self.replay_state
        ready = None
        if with_ready:
            ready = torch.cuda.Event()
            ready.record(self.upload)
        torch.cuda.synchronize()
        self.replay.push_raw(self.sids, [TICK] * self.people, *self.replay_tick)
        t0 = time.perf_counter()
        self.front.cluster(*self.scene_ticks[t], ready=ready)
        dt = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        return dt

    def tables(self, t):
        _, _, count, cen, _ = self.front.cluster(*self.scene_ticks[t])
        return count.copy(), cen.copy()


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, (time.perf_counter() - t0) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scene_bench: needs the GPU; nothing is measured without one")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    enc, means = make_encoder()
    F_hip.set_precision("bf16")
    say(f"scene_bench: SceneSplitter.push beside MultiStreamScorer.push_raw of the same people pre-separated, N={N} C={C} K={K} "
        f"bf16, {TICK} scene frames a tick, {CLUTTER} clutter detections a frame, {torch.cuda.get_device_name(0)}")
    say(f"measurements alternated in one process, {args.windows} windows of {args.ticks} ticks, ms per tick (cluster: per "
        "launch); spread = (max - min) / median over the windows")
    for people in PEOPLE:
        bed = Bed(enc, means, people, args.windows * args.ticks)
        card = float(np.mean([int(p.shape[0]) for p, _ in bed.scene_ticks])) / TICK
        say(f"{people} people ({card:.0f} detections a scene frame, {bed.windows} windows a tick): last warm tick of the two "
            f"scorers: {'the same bits' if bed.same else 'DIFFERENT'}")
        names = ("cluster", "wait", "behind", "ready", "associate", "push", "push_raw")
        rec = {n: ([], []) for n in names}
        first = bed.pos["push"]
        for w in range(args.windows):
            t0 = first + w * args.ticks
            it = iter(range(t0, t0 + args.ticks))
            d, h = timed(lambda: bed.cluster(next(it)), args.ticks)
            rec["cluster"][0].append(d), rec["cluster"][1].append(h)
            it = iter(range(t0, t0 + args.ticks))
            d, h = timed(lambda: bed.wait(next(it)), args.ticks)
            rec["wait"][0].append(d), rec["wait"][1].append(h)
            for name, flag in (("behind", False), ("ready", True)):
                vals = [bed.wait_in_flight(t, flag) for t in range(t0, t0 + args.ticks)]
                rec[name][0].append(float("nan")), rec[name][1].append(statistics.median(vals))
            tabs = [bed.tables(t) for t in range(t0, t0 + args.ticks)]
            state = bed.sp.front.state
            c0 = time.perf_counter()
            for count, cen in tabs:             # chained: every tick continues the state the one before left
                state = scene.associate(state, count, cen, bed.sp.front.params)[0]
            rec["associate"][0].append(float("nan")), rec["associate"][1].append((time.perf_counter() - c0) * 1e3 / len(tabs))
            for name in ("push", "push_raw"):
                d, h = timed(lambda: bed.tick(name), args.ticks)
                rec[name][0].append(d), rec[name][1].append(h)
        med = {}
        for name in names:
            for kind, vals in zip(("device events", "host wall"), rec[name]):
                if vals[0] != vals[0]:              # (no device clock for this row)
                    continue
                m = statistics.median(vals)
                med[name, kind] = m
                say(f"  {name:>8s} {kind:13s}: " + " ".join(f"{v:.4f}" for v in vals)
                    + f"   median {m:.4f} ms  spread {100 * (max(vals) - min(vals)) / m:.1f} %")
        say(f"  push / push_raw: device events {med['push', 'device events'] / med['push_raw', 'device events']:.3f}x, host wall "
            f"{med['push', 'host wall'] / med['push_raw', 'host wall']:.3f}x")
        assert int(bed.sp.err) == 0 and int(bed.ms.raw_err) == 0 and int(bed.mf.raw_err) == 0
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
