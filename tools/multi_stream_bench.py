"""S concurrent live tracks: S StreamingScorers pushed one after the other against one MultiStreamScorer tick.

    python tools/multi_stream_bench.py [--out profiles/multi_stream.txt]                       # timings, one process
    rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d DIR -- \\
        python tools/multi_stream_bench.py --trace-segments                                    # a run of its own
    python tools/multi_stream_bench.py --count-trace DIR [--out profiles/multi_stream.txt]     # appends the counts

N = 128, C = 4, K = 8, bf16 mode, ``hop`` = 6 new frames per stream per tick, every stream warmed until it emits one window
per tick.  For S in 1, 4, 16, 64:
  (a) S StreamingScorer objects pushed one after the other   -- the only way before MultiStreamScorer existed
  (b) one MultiStreamScorer.push of the same 6 * S frames
alternated in one process: WINDOWS windows of TICKS ticks each, per window the time between two device events and the host
wall time to a synchronise, both per tick; medians and spreads ((max - min) / median over the windows).  The outputs of the
last tick of (a) and (b) are compared in the same run.

``--trace-segments`` runs, for (a) at S = 1 and (b) at every S, TRACE_TICKS ticks between two launches of a marker kernel
(pcaa_crop_overlap, which no tick uses); ``--count-trace`` reads the profiler's kernel and memory-copy traces of that run
and counts the device activities between the markers, per tick.
"""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opensetgaitrecognition_pcaa_amd import constants, functional as F_hip, inference, models, ops, synthetic as syn  # noqa: E402

STREAMS = (1, 4, 16, 64)
MARKER = "crop_overlap_kernel"
TRACE_TICKS = 10
N, C, K, KVOTE = 128, 4, 8, 4


class Bed:
    """S tracks, S StreamingScorers and one MultiStreamScorer on the same encoder, all warmed to one window per tick"""

    def __init__(self, enc, means, S, n_ticks):
        T, hop = constants.NSTEPS, constants.CROP_STEP
        self.S, self.hop = S, hop
        self.warm = T + hop * 3
        F = self.warm + hop * n_ticks
        gen = torch.Generator().manual_seed(100 + S)
        base = syn.synthetic_pcs(1, F, N, C, seed=5)[0]
        # S tracks: the seeded track, each stream shifted and jittered (distinct frames, same statistics)
        self.tracks = [(base.roll(7 * s, 0) + 0.01 * torch.randn(base.shape, generator=gen)).contiguous().cuda()
                       for s in range(S)]
        self.single = [inference.StreamingScorer(enc, means, 0.0, KVOTE, K) for _ in range(S)]
        self.multi = inference.MultiStreamScorer(enc, means, 0.0, KVOTE, K, max_streams=max(S, 1))
        self.sids = [self.multi.open() for _ in range(S)]
        for s in range(S):
            self.single[s].push(self.tracks[s][:self.warm])
        for a in range(0, self.warm, 32):
            b = min(a + 32, self.warm)
            self.multi.push(self.sids, [b - a] * S, torch.cat([t[a:b] for t in self.tracks]))
        self.pos_a = self.pos_b = self.warm
        # the tick's frames as the tracker would hand them over: one tensor per tick for (b), one view per stream for (a)
        self.ticks_b = [torch.cat([t[p:p + hop] for t in self.tracks])
                        for p in range(self.warm, F, hop)]

    def tick_a(self):
        p = self.pos_a
        out = [sc.push(t[p:p + self.hop]) for sc, t in zip(self.single, self.tracks)]
        self.pos_a = p + self.hop
        return out

    def tick_b(self):
        i = (self.pos_b - self.warm) // self.hop
        out = self.multi.push(self.sids, [self.hop] * self.S, self.ticks_b[i])
        self.pos_b += self.hop
        return out


def timed(fn, ticks):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(ticks):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ticks, (time.perf_counter() - t0) * 1e3 / ticks, out


def make_encoder():
    constants.NFEATURES = C
    enc = models.CGEncoder(K, nmax_points=N, use_projection_head=True).float()
    syn.deterministic_fill_(enc, 0)
    enc = enc.cuda().eval()
    means = (torch.randn(K, 32, generator=torch.Generator().manual_seed(1)) * 3).cuda()
    return enc, means


def marker(scratch):
    ops.crop_overlap(scratch, 1)


def trace_segments():
    enc, means = make_encoder()
    F_hip.set_precision("bf16")
    scratch = torch.zeros((2, 2, 4, 4), device="cuda")
    beds = [(S, Bed(enc, means, S, 3 + TRACE_TICKS)) for S in STREAMS]
    segments = [("a", 1, beds[0][1].tick_a)] + [("b", S, bed.tick_b) for S, bed in beds]
    for _, _, fn in segments:                  # every shape warmed before its traced segment
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for name, S, fn in segments:
        marker(scratch)
        for _ in range(TRACE_TICKS):
            fn()
        marker(scratch)
        torch.cuda.synchronize()
        print(f"segment ({name}) S={S}: {TRACE_TICKS} ticks between two markers", flush=True)


def count_trace(folder, say):
    rows = []
    for f in glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), "kernel", r["Kernel_Name"]) for r in csv.DictReader(open(f))]
    for f in glob.glob(os.path.join(folder, "**", "*memory_copy_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), "copy", r.get("Direction", "copy")) for r in csv.DictReader(open(f))]
    rows.sort()
    marks = [i for i, r in enumerate(rows) if r[1] == "kernel" and MARKER in r[2]]
    names = [("a", 1)] + [("b", S) for S in STREAMS]
    if len(marks) != 2 * len(names):
        raise SystemExit(f"expected {2 * len(names)} marker kernels in the trace, found {len(marks)}")
    say(f"device activities per tick (rocprofv3 kernel and memory-copy traces, a run of its own, {TRACE_TICKS} ticks "
        "between two marker kernels):")
    for (name, S), lo, hi in zip(names, marks[0::2], marks[1::2]):
        seg = rows[lo + 1:hi]
        kernels = sum(r[1] == "kernel" for r in seg)
        copies = len(seg) - kernels
        say(f"  ({name}) S={S:<2d}: {len(seg) / TRACE_TICKS:g} per tick = {kernels / TRACE_TICKS:g} kernels + "
            f"{copies / TRACE_TICKS:g} copies")
        if name == "b" and S == 1 or name == "a":
            per = {}
            for r in seg:
                key = r[2].replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0].split("<")[0][:70]
                per[key] = per.get(key, 0) + 1
            for key, n in sorted(per.items(), key=lambda kv: -kv[1]):
                say(f"        {n / TRACE_TICKS:5g}  {key}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-segments", action="store_true")
    ap.add_argument("--count-trace", default=None, metavar="DIR")
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
    enc, means = make_encoder()
    F_hip.set_precision("bf16")
    say(f"multi_stream_bench: N={N} C={C} K={K} bf16, {constants.CROP_STEP} new frames per stream per tick (one new window "
        f"per stream), {torch.cuda.get_device_name(0)}")
    say(f"(a) S StreamingScorers pushed one after the other, (b) one MultiStreamScorer tick; alternated, {args.windows} "
        f"windows of {args.ticks} ticks, ms per tick; spread = (max - min) / median over the windows")
    result = {}
    for S in STREAMS:
        bed = Bed(enc, means, S, 2 + 2 + args.windows * args.ticks)
        for _ in range(2):
            out_a, out_b = bed.tick_a(), bed.tick_b()
        # same frames through both: compare what they return
        pa, fa = torch.cat([o[0] for o in out_a]), torch.cat([o[1] for o in out_a])
        agree = (pa == out_b.preds).float().mean().item()
        err = ((fa - out_b.sup_fv).abs().max() / fa.abs().max()).item()
        assert len(out_b) == S and out_b.stream.tolist() == bed.sids
        for _ in range(2):
            bed.tick_a(), bed.tick_b()
        rec = {"a": ([], []), "b": ([], [])}
        for _ in range(args.windows):
            for name, fn in (("a", bed.tick_a), ("b", bed.tick_b)):
                d, h, _ = timed(fn, args.ticks)
                rec[name][0].append(d)
                rec[name][1].append(h)
        assert bed.multi.scatter_err.item() == 0
        say(f"S={S}: outputs of (b) against (a) on the same tick: labels agree {agree:.4f}, embedding difference {err:.2e} "
            "of scale")
        med = {}
        for name in ("a", "b"):
            for kind, vals in zip(("device events", "host wall"), rec[name]):
                m = statistics.median(vals)
                med[name, kind] = (m, (max(vals) - min(vals)) / m)
                say(f"  ({name}) {kind:13s}: " + " ".join(f"{v:.3f}" for v in vals)
                    + f"   median {m:.3f}  spread {100 * med[name, kind][1]:.1f} %")
        for kind in ("device events", "host wall"):
            a, b = med["a", kind], med["b", kind]
            say(f"  (a)/(b) {kind}: {a[0] / b[0]:.2f}x   ((a) per stream {a[0] / S:.3f} ms, (b) per stream {b[0] / S:.3f} ms)")
        result[S] = med
    say("conditions:")
    a1, b1 = result[1]["a", "device events"], result[1]["b", "device events"]
    ok3 = b1[0] <= a1[0] * (1 + a1[1])
    say(f"  3. (b) at S=1 not slower than (a) at S=1 by more than (a)'s spread: (b) {b1[0]:.3f} ms, (a) {a1[0]:.3f} ms, "
        f"spread {100 * a1[1]:.1f} % -> {'holds' if ok3 else 'FAILS'}")
    for S in (16, 64):
        a, b = result[S]["a", "device events"], result[S]["b", "device events"]
        ok4 = b[0] < a[0] * (1 - a[1])
        say(f"  4. (b) faster than (a) at S={S} by more than (a)'s spread: (a)/(b) = {a[0] / b[0]:.2f}x, spread "
            f"{100 * a[1]:.1f} % -> {'holds' if ok4 else 'FAILS'}")
    write("w")


if __name__ == "__main__":
    main()
