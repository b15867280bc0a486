"""Training batches built from raw detections on the device (``batcher.RawTrackBatcher``) against batches gathered from
stored crops (``batcher.DeviceBatcher``), next to the train step they feed; and what it costs to get each store into HBM.

    python tools/raw_batcher_bench.py [--out profiles/raw_batcher.txt]

Part 1, for (B, N) in (64, 128) and (16, 150), C = 4, T = 30, a store of TRACKS tracks of FRAMES frames with 3 .. MAX_POINTS
detections a frame (both the repeat-pad and the subsample branch at either N), random crop indices, bf16 mode.  Legs,
alternated in one process, WARM warm-up calls and then the median of WINDOWS windows between HIP events, CALLS calls a
window for the legs with a step and CALLS_SHORT for the three without (they take tens of microseconds a call: a short
window of them times the clock and the queue), spread = (max - min) / median over the windows:
  raw kernel   the one ``pcaa_crops_from_raw`` launch of a batch inside an epoch (starts and labels are slices of the
               epoch's permuted tables);
  raw batch()  ``RawTrackBatcher.batch(idx)``: two 4-byte-row gathers (starts, labels) and that launch;
  dev batch()  ``DeviceBatcher.batch(idx)`` over the same crops written out once: two row gathers and a label copy;
  step         ``PCAATrainer.step`` on one resident batch (this step is the parent commit's: nothing in it changed);
  raw + step / dev + step   a batch from either batcher and the step on it.
Part 2, a synthetic set of 10 subjects x 3 scenarios x SET_TRACKS tracks of SET_FRAMES frames written as pickles, once with
3 .. 40 and once with 3 .. MAX_POINTS detections a frame: host wall time, ending in a device synchronise, of
  raw store    ``split_track_files`` + reading the pickles + ``RawTrackStore`` (packs) + ``to_device`` + listing the crops of
               the four splits: serves every N;
  crop store   ``generate_splits`` at ONE N (reads the pickles, ``process_track``, writes the crop files) + ``pack_split`` +
               ``PackedCrops.to_device`` of the four splits;
and the bytes each keeps on disk and in HBM."""
import argparse
import os
import pickle
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opensetgaitrecognition_pcaa_amd import batcher, constants, datasets, functional as F_hip, synthetic as syn  # noqa: E402
from opensetgaitrecognition_pcaa_amd.constants import SPLIT  # noqa: E402

SHAPES = ((64, 128), (16, 150))
C, K, T = 4, 8, constants.NSTEPS
TRACKS, FRAMES, MAX_POINTS = 64, 240, 200
WARM, WINDOWS, CALLS = 5, 20, 20
CALLS_SHORT = 400        # calls per window of the legs without a step: tens of microseconds each, 20 of them time the clock
SET_TRACKS, SET_FRAMES, SET_N = 10, 60, 128


def event_windows(legs):
    """{name: (fn, calls per window)} -> {name: [ms per call of each window]}, the legs alternated window by window"""
    for fn, _ in legs.values():
        for _ in range(WARM):
            fn()
    out = {name: [] for name in legs}
    for _ in range(WINDOWS):
        for name, (fn, calls) in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) / calls)
    return out


def line(name, ms):
    med = statistics.median(ms)
    return f"  {name:<12s} median {med:8.4f} ms  spread {100 * (max(ms) - min(ms)) / med:5.1f} %  min {min(ms):8.4f}"


def build_trainer(B, N):
    from opensetgaitrecognition_pcaa_amd.train import PCAATrainer
    from opensetgaitrecognition_pcaa_amd.utils import sample_distant_points
    cfg = dict(constants.CONFIG)
    cfg.update(NMAX=N, TRAIN_CLASSES=list(range(K)), BATCH_SIZE=B)
    tr = PCAATrainer(cfg, device=torch.device("cuda"), precision="bf16")
    for i, m in enumerate((tr.encoder, tr.decoder, tr.discriminator, tr.decoder_projection_head,
                           tr.discriminator_projection_head)):
        syn.deterministic_fill_(m, i)
    tr.set_prior_means(sample_distant_points(32, K, 10, 10))
    tr.finalize()
    tr.train()
    return tr


def part1(say):
    tracks = [syn.synthetic_raw_track(100 + i, FRAMES, max_points=MAX_POINTS) for i in range(TRACKS)]
    store = datasets.RawTrackStore(tracks, [i % K for i in range(TRACKS)], ["free_walk"] * TRACKS,
                                   [str(i) for i in range(TRACKS)], splits=["train"] * TRACKS).to_device("cuda")
    cards = store.cards()
    say(f"part 1: a store of {TRACKS} tracks x {FRAMES} frames, {int(cards.sum())} detections ({cards.min()} .. {cards.max()} a "
        f"frame, {store.points.numel() * 4 / 2 ** 20:.1f} MiB as fp32 [P,5]); {WARM} warm-up calls, median of {WINDOWS} windows "
        f"between HIP events, {CALLS} calls a window with a step and {CALLS_SHORT} without, legs alternated; spread = (max - min) "
        f"/ median")
    for B, N in SHAPES:
        view = store.crops(SPLIT.TRAIN, N, C)
        raw = batcher.RawTrackBatcher(view, B, seed=1)
        crops, labels = view.materialize(seed=1)
        dev = batcher.DeviceBatcher(crops.permute(0, 2, 3, 1).contiguous(), labels, B)
        g = torch.Generator().manual_seed(B)
        idx = torch.randint(0, len(view), (B,), generator=g).cuda()
        p_raw, l_raw = raw.batch(idx)
        p_dev, l_dev = dev.batch(idx)
        assert torch.equal(p_raw, p_dev) and torch.equal(l_raw, l_dev), "the two batchers disagree"
        start = raw._starts[idx].contiguous()
        tr = build_trainer(B, N)
        z0, al = syn.synthetic_z0(B, 32).cuda(), syn.synthetic_alphas(B).cuda()
        step = lambda p, l: tr.step(p, l, z0, al)                                    # noqa: E731
        res = event_windows({
            "raw kernel": (lambda: raw._crops(start), CALLS_SHORT),
            "raw batch()": (lambda: raw.batch(idx), CALLS_SHORT),
            "dev batch()": (lambda: dev.batch(idx), CALLS_SHORT),
            "step": (lambda: step(p_dev, l_dev), CALLS),
            "raw + step": (lambda: step(*raw.batch(idx)), CALLS),
            "dev + step": (lambda: step(*dev.batch(idx)), CALLS),
        })
        raw.check(), dev.check(), tr.check()
        say(f"B = {B}, N = {N}: {len(view)} crops; a batch is {B * T} frames = {B * T * N * C * 4 / 2 ** 20:.2f} MiB; the "
            f"written-out crops hold {crops.numel() * 4 / 2 ** 20:.0f} MiB in HBM")
        for name, ms in res.items():
            say(line(name, ms))
        m = {k: statistics.median(v) for k, v in res.items()}
        say(f"  raw batch() / dev batch() = {m['raw batch()'] / m['dev batch()']:.2f}x; raw batch() / step = "
            f"{100 * m['raw batch()'] / m['step']:.2f} %; (raw + step) / (dev + step) = {m['raw + step'] / m['dev + step']:.3f}x")
        del tr


def tree_bytes(d):
    return sum(os.path.getsize(os.path.join(r, f)) for r, _, fs in os.walk(d) for f in fs)


def part2(say, max_points):
    import sklearn.model_selection  # noqa: F401  (its import, about a second, belongs to neither leg)
    with tempfile.TemporaryDirectory() as tmp:
        data, gen = os.path.join(tmp, "raw"), os.path.join(tmp, "gen")
        for subj in range(10):
            for si, scen in enumerate(("free_walk", "hands_in_pockets", "smartphone")):
                d = os.path.join(data, f"target{subj}", scen)
                os.makedirs(d)
                for t in range(SET_TRACKS):
                    with open(os.path.join(d, f"pc_tr{t}{si}.obj"), "wb") as f:
                        pickle.dump(syn.synthetic_raw_track(5000 + subj * 100 + si * 10 + t, SET_FRAMES, max_points=max_points), f)
        constants.DATA_PATH, constants.GEN_DATA_PATH = data, gen
        classes = [0, 1, 2, 3, 4, 5]
        torch.empty(1 << 20).pin_memory()                      # the first pinned allocation of the process
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        files = datasets.split_track_files(classes, (0.8, 0.1, 0.1), 0)
        tracks = []
        for path, _, _, _ in files:
            with open(path, "rb") as f:
                tracks.append(pickle.load(f))
        t1 = time.perf_counter()
        store = datasets.RawTrackStore(tracks, [f[1] for f in files], [f[2] for f in files],
                                       [datasets.track_file_index(f[0]) for f in files], splits=[f[3] for f in files])
        t2 = time.perf_counter()
        store.to_device("cuda")
        views = [store.crops(split, SET_N, C) for split in SPLIT]
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        np.random.seed(0)
        stats = datasets.generate_splits(train_classes=classes, seed=0, nmax_points=SET_N, verbose=False)
        t4 = time.perf_counter()
        held = 0
        for split in SPLIT:
            batcher.pack_split(datasets.MSRadarDataset(split), os.path.join(gen, split.value + "_packed"))
        t5 = time.perf_counter()
        for split in SPLIT:
            crops, _ = batcher.PackedCrops(os.path.join(gen, split.value + "_packed")).to_device("cuda")
            held += crops.numel() * 4
        torch.cuda.synchronize()
        t6 = time.perf_counter()
        assert [len(v) for v in views] == [stats[s.value] for s in SPLIT]
        raw_hbm = store.points.numel() * 4 + store.offsets.numel() * 4 + store.frame_key.numel() * 4
        crop_files = sum(os.path.getsize(os.path.join(gen, s.value, f)) for s in SPLIT for f in os.listdir(os.path.join(gen, s.value)))
        ms = lambda a, b: 1e3 * (b - a)                                                  # noqa: E731
        say(f"part 2, 3 .. {max_points} detections a frame: 10 subjects x 3 scenarios x {SET_TRACKS} tracks x {SET_FRAMES} frames "
            f"({store.n_frames} frames, {store.points.shape[0]} detections), {sum(stats.values())} crops at N = {SET_N}; host wall "
            f"time of ONE run each, ending in a device synchronise; sklearn imported and a pinned buffer allocated beforehand")
        say(f"  raw store   split + read pickles {ms(t0, t1):8.1f} ms, pack {ms(t1, t2):8.1f} ms, upload + list crops {ms(t2, t3):7.1f} ms, "
            f"total {ms(t0, t3):8.1f} ms; pickles {tree_bytes(data) / 2 ** 20:.1f} MiB on disk, {raw_hbm / 2 ** 20:.1f} MiB in HBM; "
            f"serves every N")
        say(f"  crop store  generate_splits {ms(t3, t4):8.1f} ms ({1e3 * ms(t3, t4) / store.n_frames:.1f} us a frame), pack_split "
            f"{ms(t4, t5):8.1f} ms, upload {ms(t5, t6):7.1f} ms, total {ms(t3, t6):8.1f} ms; crop files {crop_files / 2 ** 20:.1f} MiB + "
            f"packed {held / 2 ** 20:.1f} MiB on disk, {held / 2 ** 20:.1f} MiB in HBM; for N = {SET_N} alone")
        say(f"  crop store / raw store: time {(t6 - t3) / (t3 - t0):.2f}x, HBM {held / raw_hbm:.2f}x, disk beside the pickles "
            f"{(crop_files + held) / 2 ** 20:.0f} MiB against none")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("raw_batcher_bench: needs the GPU; there is nothing to measure without it")
    F_hip.set_precision("bf16")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"raw_batcher_bench: {torch.cuda.get_device_name(0)}, C = {C}, T = {T}, K = {K}, bf16 mode")
    part1(say)
    for max_points in (40, MAX_POINTS):
        part2(say, max_points)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
