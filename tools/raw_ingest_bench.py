"""From the radar's detections to a scored tick: frame preparation on the host against ``MultiStreamScorer.push_raw``.

    python tools/raw_ingest_bench.py [--out profiles/raw_ingest.txt]                           # timings, one process
    rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d DIR -- \\
        python tools/raw_ingest_bench.py --trace-segments                                      # a run of its own
    python tools/raw_ingest_bench.py --count-trace DIR [--out profiles/raw_ingest.txt]         # appends the counts
    python tools/raw_ingest_bench.py --dedup [--out profiles/raw_unique.txt]                   # push_raw padded against dedup_points

N = 128, C = 4, K = 8, bf16 mode, ``hop`` = 6 new frames per stream per tick, every stream warmed until it emits one window
per tick; raw frames of 3 .. MAX_POINTS detections (both the repeat-pad and the subsample branch at N = 128).  For S in 1, 4,
16, 64, three legs, each on a MultiStreamScorer of its own:
  (a) what there was before ``push_raw``: ``datasets.process_track`` on the tick's new raw frames on the host, cast to fp32,
      upload, ``push``;
  (b) ``datasets.pack_raw_frames`` of the same raw frames, upload, ``push_raw`` (picks drawn on the device);
  (c) ``push`` alone on frames that were prepared and uploaded before the clock started: the floor.
Alternated in one process: WINDOWS windows of TICKS ticks each; per window the host wall time to a synchronise and the part
of it spent preparing frames on the host ((a): process_track + cast; (b): pack_raw_frames; (c): nothing), both per tick;
medians and spreads ((max - min) / median over the windows).

``--dedup`` measures ``dedup_points=True`` (the frames' distinct points through the PointNet block once, pooled with their
multiplicities) against the padded ``push_raw``, the detections of every tick on the device before the clock starts, the two
legs alternated in one process as above: ticks at every S, and ``OpenSetScorer.embed_raw_track`` of one track of 1 024 windows;
N = 128, raw frames of 3 .. 40 and of 3 .. 150 detections, bf16 and fp32.  Next to each time: the rows the PointNet block ran
(padded: frames x N; dedup: the compact table, and of it the rows that hold a distinct point).

``--trace-segments`` runs, at every S, TRACE_TICKS ticks of (c), of (b) with the packed detections already on the device
(as (c)'s frames are: the comparison of what the two entry points launch) and of (b) as timed (pack + two uploads per
tick) between two launches of a marker kernel; ``--count-trace`` counts the device activities between the markers.
"""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from multi_stream_bench import C, K, KVOTE, MARKER, N, STREAMS, TRACE_TICKS, make_encoder, marker  # noqa: E402
from opensetgaitrecognition_pcaa_amd import constants, datasets, functional as F_hip, inference, ops, synthetic as syn  # noqa: E402

MAX_POINTS = 200
LEGS = ("a", "b", "c")


class Bed:
    """S raw tracks and one warmed MultiStreamScorer per leg"""

    def __init__(self, enc, means, S, n_ticks):
        T, hop = constants.NSTEPS, constants.CROP_STEP
        self.S, self.hop = S, hop
        self.warm = T + hop * 3
        F = self.warm + hop * n_ticks
        self.tracks = [syn.synthetic_raw_track(900 + 64 * S + s, F, max_points=MAX_POINTS) for s in range(S)]
        np.random.seed(S)
        ready = [torch.from_numpy(datasets.process_track(t, nmax=N, nfeatures=C)).float() for t in self.tracks]
        self.multi = {leg: inference.MultiStreamScorer(enc, means, 0.0, KVOTE, K, max_streams=S, seed=S) for leg in LEGS}
        self.sids = [self.multi["a"].open() for _ in range(S)]
        for leg in LEGS[1:]:
            assert [self.multi[leg].open() for _ in range(S)] == self.sids
        self.counts = [hop] * S
        for a in range(0, self.warm, 32):
            b = min(a + 32, self.warm)
            frames = torch.cat([t[a:b] for t in ready]).cuda()
            for leg in LEGS:
                self.multi[leg].push(self.sids, [b - a] * S, frames)
        self.pos = {leg: self.warm for leg in LEGS + ("b_dev",)}
        self.prep = {leg: 0.0 for leg in LEGS}
        # (c): the tick's frames as a tracker that keeps processed frames on the device would hand them over
        self.ticks_c = [torch.cat([t[p:p + hop] for t in ready]).cuda() for p in range(self.warm, F, hop)]
        self.ticks_b_dev = None

    def _new_raw(self, leg):
        p = self.pos[leg]
        self.pos[leg] = p + self.hop
        return [fr for t in self.tracks for fr in t[p:p + self.hop]]

    def tick_a(self):
        raw = self._new_raw("a")
        t0 = time.perf_counter()
        frames = torch.from_numpy(datasets.process_track(raw, nmax=N, nfeatures=C).astype(np.float32))
        self.prep["a"] += time.perf_counter() - t0
        return self.multi["a"].push(self.sids, self.counts, frames.cuda())

    def tick_b(self):
        raw = self._new_raw("b")
        t0 = time.perf_counter()
        points, offsets = datasets.pack_raw_frames(raw, torch.float32)
        self.prep["b"] += time.perf_counter() - t0
        return self.multi["b"].push_raw(self.sids, self.counts, points.cuda(non_blocking=True), offsets.cuda(non_blocking=True))

    def tick_c(self):
        i = (self.pos["c"] - self.warm) // self.hop
        self.pos["c"] += self.hop
        return self.multi["c"].push(self.sids, self.counts, self.ticks_c[i])

    def stage_b_dev(self, n_ticks):
        """the packed detections of the next ``n_ticks`` ticks of leg (b), on the device before the segment starts"""
        p0 = self.pos["b"]
        self.ticks_b_dev = []
        for p in range(p0, p0 + n_ticks * self.hop, self.hop):
            points, offsets = datasets.pack_raw_frames([fr for t in self.tracks for fr in t[p:p + self.hop]], torch.float32)
            self.ticks_b_dev.append((points.cuda(), offsets.cuda()))
        torch.cuda.synchronize()

    def tick_b_dev(self):
        points, offsets = self.ticks_b_dev.pop(0)
        self.pos["b"] += self.hop
        return self.multi["b"].push_raw(self.sids, self.counts, points, offsets)


def timed(bed, leg, ticks):
    fn = getattr(bed, "tick_" + leg)
    bed.prep[leg] = 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ticks):
        fn()
    host = (time.perf_counter() - t0) * 1e3 / ticks
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / ticks, host, bed.prep[leg] * 1e3 / ticks


SEGMENTS = (("c", "tick_c", "push, frames on the device"), ("b", "tick_b_dev", "push_raw, detections on the device"),
            ("b+", "tick_b", "pack_raw_frames, two uploads, push_raw"))


def trace_segments():
    enc, means = make_encoder()
    F_hip.set_precision("bf16")
    scratch = torch.zeros((2, 2, 4, 4), device="cuda")
    for S in STREAMS:
        bed = Bed(enc, means, S, 3 * (3 + TRACE_TICKS) + 2)
        for name, fn, _ in SEGMENTS:
            if fn == "tick_b_dev":
                bed.stage_b_dev(3 + TRACE_TICKS)
            for _ in range(3):                     # every shape warmed before its traced segment
                getattr(bed, fn)()
            torch.cuda.synchronize()
            marker(scratch)
            for _ in range(TRACE_TICKS):
                getattr(bed, fn)()
            marker(scratch)
            torch.cuda.synchronize()
            print(f"segment ({name}) S={S}: {TRACE_TICKS} ticks between two markers", flush=True)
        assert bed.multi["b"].raw_err.item() == 0


def count_trace(folder, say):
    rows = []
    for f in glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), "kernel", r["Kernel_Name"]) for r in csv.DictReader(open(f))]
    for f in glob.glob(os.path.join(folder, "**", "*memory_copy_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), "copy", r.get("Direction", "copy")) for r in csv.DictReader(open(f))]
    rows.sort()
    marks = [i for i, r in enumerate(rows) if r[1] == "kernel" and MARKER in r[2]]
    names = [(name, what, S) for S in STREAMS for name, _, what in SEGMENTS]
    if len(marks) != 2 * len(names):
        raise SystemExit(f"expected {2 * len(names)} marker kernels in the trace, found {len(marks)}")
    say(f"device activities per tick (rocprofv3 kernel and memory-copy traces, a run of its own, {TRACE_TICKS} ticks "
        "between two marker kernels):")
    per_tick = {}
    for (name, what, S), lo, hi in zip(names, marks[0::2], marks[1::2]):
        seg = rows[lo + 1:hi]
        kernels = sum(r[1] == "kernel" for r in seg)
        per_tick[name, S] = len(seg) / TRACE_TICKS
        say(f"  ({name:2s}) S={S:<2d}: {len(seg) / TRACE_TICKS:g} per tick = {kernels / TRACE_TICKS:g} kernels + "
            f"{(len(seg) - kernels) / TRACE_TICKS:g} copies   [{what}]")
        if S == STREAMS[0] and name in ("b", "c"):
            per = {}
            for r in seg:
                key = r[2].replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0].split("<")[0][:70]
                per[key] = per.get(key, 0) + 1
            for key, n in sorted(per.items(), key=lambda kv: -kv[1]):
                say(f"        {n / TRACE_TICKS:5g}  {key}")
    extra = {S: per_tick["b", S] - per_tick["c", S] for S in STREAMS}
    say("  (b) - (c), activities per tick: " + ", ".join(f"S={S}: {extra[S]:+g}" for S in STREAMS)
        + f" -> {'one more at every S' if all(v == 1 for v in extra.values()) else 'NOT one more at every S'}")


class DedupBed:
    """S raw tracks, the detections of every tick staged on the device, a warmed padded and a warmed dedup scorer"""

    def __init__(self, enc, means, S, n_ticks, max_points):
        T, hop = constants.NSTEPS, constants.CROP_STEP
        self.S, self.hop = S, hop
        warm = T + hop * 3
        tracks = [syn.synthetic_raw_track(1700 + 64 * S + s, warm + hop * n_ticks, max_points=max_points) for s in range(S)]
        self.multi = {leg: inference.MultiStreamScorer(enc, means, 0.0, KVOTE, K, max_streams=S, seed=S, dedup_points=leg == "u")
                      for leg in ("p", "u")}
        self.sids = [self.multi["p"].open() for _ in range(S)]
        assert [self.multi["u"].open() for _ in range(S)] == self.sids
        for a in range(0, warm, 32):
            b = min(a + 32, warm)
            points, offsets = datasets.pack_raw_frames([fr for t in tracks for fr in t[a:b]], torch.float32)
            for leg in ("p", "u"):
                self.multi[leg].push_raw(self.sids, [b - a] * S, points.cuda(), offsets.cuda())
        self.staged, self.distinct_rows, self.table_rows = [], 0, 0
        for p in range(warm, warm + hop * n_ticks, hop):
            raw = [fr for t in tracks for fr in t[p:p + hop]]
            points, offsets = datasets.pack_raw_frames(raw, torch.float32)
            self.staged.append((points.cuda(), offsets.cuda()))
            cards = np.array([len(fr["z_coord"]) for fr in raw])
            self.distinct_rows += int(np.minimum(cards, N).sum())
            self.table_rows += ops.unique_table_rows(points.shape[0], len(raw), N)
        self.n_ticks = n_ticks
        self.at = {"p": 0, "u": 0}
        torch.cuda.synchronize()

    def tick(self, leg):
        points, offsets = self.staged[self.at[leg]]
        self.at[leg] += 1
        return self.multi[leg].push_raw(self.sids, [self.hop] * self.S, points, offsets)


def _wall(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def _line(say, head, rec):
    med = {leg: statistics.median(v) for leg, v in rec.items()}
    for leg, name in (("p", "padded"), ("u", "dedup ")):
        v = rec[leg]
        say(f"  {head} {name}: " + " ".join(f"{x:.3f}" for x in v)
            + f"   median {med[leg]:.3f}  spread {100 * (max(v) - min(v)) / max(med[leg], 1e-9):.1f} %")
    return med


def dedup_legs(args, say):
    enc, means = make_encoder()
    hop, T = constants.CROP_STEP, constants.NSTEPS
    say(f"raw_ingest_bench --dedup: N={N} C={C} K={K}, {torch.cuda.get_device_name(0)}; push_raw with the padded frames "
        "(padded) against dedup_points=True (dedup), detections on the device before the clock starts; alternated, "
        f"{args.windows} windows of {args.ticks} ticks, wall ms per tick to a device synchronise; spread = (max - min) / median")
    say("rows: what the PointNet block ran -- padded: frames x N (to whole tiles); dedup: the compact table "
        "min(P + n, n N) to whole 256-row tiles, of which 'distinct' hold a point (sum of min(card, N))")
    for mode in ("bf16", "fp32"):
        F_hip.set_precision(mode)
        for max_points in (40, 150):
            say(f"{mode}, raw frames of 3..{max_points} detections:")
            for S in STREAMS:
                n_ticks = 2 + args.windows * args.ticks
                bed = DedupBed(enc, means, S, n_ticks, max_points)
                for leg in ("p", "u"):
                    for _ in range(2):
                        bed.tick(leg)
                rec = {"p": [], "u": []}
                for _ in range(args.windows):
                    for leg in ("p", "u"):
                        rec[leg].append(_wall(lambda: bed.tick(leg), args.ticks))
                for leg in ("p", "u"):
                    assert bed.multi[leg].scatter_err.item() == 0 and bed.multi[leg].raw_err.item() == 0
                q = F_hip.frame_pad_quantum(N)
                padded_rows = -(-S * hop // q) * q * N
                med = _line(say, f"S={S:<2d}", rec)
                say(f"  S={S:<2d} rows per tick: padded {padded_rows}, dedup table {bed.table_rows / n_ticks:.0f} (distinct "
                    f"{bed.distinct_rows / n_ticks:.0f}); rows padded / table {padded_rows * n_ticks / bed.table_rows:.2f}x, "
                    f"time padded / dedup {med['p'] / med['u']:.2f}x")
            # one long track: 1 024 windows
            F = T + hop * 1024
            raw = syn.synthetic_raw_track(4242, F, max_points=max_points)
            points, offsets = datasets.pack_raw_frames(raw, torch.float32)
            points, offsets = points.cuda(), offsets.cuda()
            sc = inference.OpenSetScorer(enc, means)
            run = {"p": lambda: sc.embed_raw_track(points, offsets, seed=3), "u": lambda: sc.embed_raw_track(points, offsets, seed=3, dedup_points=True)}
            for leg in ("p", "u"):
                run[leg]()
            table = sc.last_rows_encoded
            rec = {"p": [], "u": []}
            for _ in range(args.windows):
                for leg in ("p", "u"):
                    rec[leg].append(_wall(run[leg], 3))
            assert sc.raw_err.item() == 0
            cards = np.array([len(fr["z_coord"]) for fr in raw])
            U = sc.last_frames_encoded
            med = _line(say, f"embed_raw_track, {inference.window_count(F)} windows ({U} frames)", rec)
            say(f"  embed_raw_track rows: padded {U * N}, dedup table {table} (distinct {int(np.minimum(cards[:U], N).sum())}); "
                f"rows padded / table {U * N / table:.2f}x, time padded / dedup {med['p'] / med['u']:.2f}x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-segments", action="store_true")
    ap.add_argument("--count-trace", default=None, metavar="DIR")
    ap.add_argument("--dedup", action="store_true")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def write(mode):
        if args.out:
            with open(args.out, mode) as f:
                f.write("\n".join(lines) + "\n")

    if args.count_trace:
        count_trace(args.count_trace, say)
        return write("a")
    if args.trace_segments:
        return trace_segments()
    if args.dedup:
        dedup_legs(args, say)
        return write("w")
    enc, means = make_encoder()
    F_hip.set_precision("bf16")
    hop = constants.CROP_STEP
    say(f"raw_ingest_bench: N={N} C={C} K={K} bf16, {hop} new raw frames per stream per tick (3..{MAX_POINTS} detections "
        f"each, one new window per stream), {torch.cuda.get_device_name(0)}")
    say("(a) process_track on the host + cast + upload + push, (b) pack_raw_frames + upload + push_raw, (c) push of frames "
        f"already on the device; alternated, {args.windows} windows of {args.ticks} ticks, ms per tick; spread = (max - min) / "
        "median over the windows")
    say("wall: to a device synchronise; host: until the last tick's calls have returned; prep: of that, preparing the frames "
        "on the host ((a) process_track + cast, (b) pack_raw_frames)")
    result = {}
    for S in STREAMS:
        bed = Bed(enc, means, S, 2 + 2 + args.windows * args.ticks)
        for _ in range(2):
            for leg in LEGS:
                getattr(bed, "tick_" + leg)()
        rec = {leg: ([], [], []) for leg in LEGS}
        for _ in range(args.windows):
            for leg in LEGS:
                for store, v in zip(rec[leg], timed(bed, leg, args.ticks)):
                    store.append(v)
        for leg in LEGS:
            assert bed.multi[leg].scatter_err.item() == 0 and bed.multi[leg].raw_err.item() == 0
        say(f"S={S} ({S * hop} frames per tick):")
        med = {}
        for leg in LEGS:
            for kind, vals in zip(("wall", "host", "prep"), rec[leg]):
                m = statistics.median(vals)
                med[leg, kind] = m
                if kind == "prep" and leg == "c":
                    continue
                say(f"  ({leg}) {kind:4s}: " + " ".join(f"{v:.3f}" for v in vals)
                    + f"   median {m:.3f}  spread {100 * (max(vals) - min(vals)) / max(m, 1e-9):.1f} %")
        say(f"  (a) prep share of wall {100 * med['a', 'prep'] / med['a', 'wall']:.0f} %, {1e3 * med['a', 'prep'] / (S * hop):.1f} us "
            f"per frame; (b) prep share of wall {100 * med['b', 'prep'] / med['b', 'wall']:.0f} %, "
            f"{1e3 * med['b', 'prep'] / (S * hop):.1f} us per frame")
        say(f"  wall (a)/(b) {med['a', 'wall'] / med['b', 'wall']:.2f}x   (b)/(c) {med['b', 'wall'] / med['c', 'wall']:.2f}x   "
            f"(b) - (c) {med['b', 'wall'] - med['c', 'wall']:+.3f} ms")
        result[S] = med
    say("host time per tick against S (does (b) grow the way (a) does?):")
    for leg in ("a", "b", "c"):
        say(f"  ({leg}) host: " + "  ".join(f"S={S}: {result[S][leg, 'host']:.3f}" for S in STREAMS)
            + f"   S=64 / S=1 = {result[STREAMS[-1]][leg, 'host'] / result[STREAMS[0]][leg, 'host']:.1f}x")
    write("w")


if __name__ == "__main__":
    main()
