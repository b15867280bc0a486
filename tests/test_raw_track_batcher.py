"""``batcher.RawTrackBatcher`` on the device: batches built from the raw detections of a ``datasets.RawTrackStore`` by one
``pcaa_crops_from_raw`` launch each, against a ``DeviceBatcher`` over the same crops written out once, and through the
train loop.  B = 4, N = 32, T = 30, tracks of 40 - 60 frames with 3 - 60 detections a frame (both sides of N)."""
import numpy as np
import pytest
import torch

from opensetgaitrecognition_pcaa_amd import batcher, constants, datasets, synthetic as syn
from opensetgaitrecognition_pcaa_amd.constants import SPLIT

pytestmark = pytest.mark.gpu

B, N, C, T = 4, 32, 4, constants.NSTEPS
LENGTHS = (40, 47, 53, 60, 44)


@pytest.fixture(scope="module")
def store():
    tracks = [syn.synthetic_raw_track(700 + i, F, max_points=60) for i, F in enumerate(LENGTHS)]
    st = datasets.RawTrackStore(tracks, [0, 1, 2, 0, 1], ["free_walk"] * 5, ["3", "10", "4", "21", "7"], splits=["train"] * 5,
                                serials=[11, 5, 8, 2, 30])
    return st.to_device("cuda")


def _epochs(loader, n, seed):
    torch.manual_seed(seed)
    out = []
    for _ in range(n):
        out.append([(p.clone(), l.clone()) for p, l in loader])
    return out, torch.rand(2)


def test_fixed_redraw_is_a_device_batcher_over_the_written_out_crops(store):
    from opensetgaitrecognition_pcaa_amd import ops
    view = store.crops(SPLIT.TRAIN, N, C)
    assert len(view) == sum((F - 1 - T) // constants.CROP_STEP + 1 for F in LENGTHS) == 17
    frames = ops.frames_from_raw(store.points_dev, store.offsets_dev, N, C, seed=9, frame_key=store.frame_key_dev)
    crops = torch.stack([frames[s:s + T] for s in view.start.tolist()])                  # [M,T,N,C]
    labels = torch.from_numpy(view.labels).cuda()
    for shuffle, drop_last in ((True, True), (False, False)):
        raw = batcher.RawTrackBatcher(view, B, shuffle=shuffle, drop_last=drop_last, seed=9)
        ref = batcher.DeviceBatcher(crops, labels, B, shuffle=shuffle, drop_last=drop_last)
        assert len(raw) == len(ref) == (4 if drop_last else 5)
        got, after_got = _epochs(raw, 2, 123)
        want, after_want = _epochs(ref, 2, 123)
        assert torch.equal(after_got, after_want), "the same consumption of torch's global RNG"
        for e in range(2):
            assert len(got[e]) == len(want[e]) == len(raw)
            for (p, l), (pw, lw) in zip(got[e], want[e]):
                assert p.shape == pw.shape and p.shape[1:] == (C, T, N) and p.stride() == pw.stride()
                assert l.dtype == torch.int64 and torch.equal(l, lw) and torch.equal(p, pw)
        raw.check()
        # .batch(idx): the same crops by index
        idx = torch.tensor([16, 0, 5, 5], device="cuda")
        p, l = raw.batch(idx)
        pw, lw = ref.batch(idx)
        assert torch.equal(p, pw) and torch.equal(l, lw)
    # the deployment route draws the same frames: track serial 8 (track 2) under the same seed
    a, b = int(store.track_first[2]), int(store.track_first[3])
    off = store.offsets_dev[a:b + 1]
    keys = torch.from_numpy(np.stack([np.full(b - a, 8), np.arange(b - a)], axis=1).astype(np.int32)).cuda()
    assert torch.equal(store.frame_key_dev[a:b], keys)
    alone = ops.frames_from_raw(store.points_dev, off, N, C, seed=9, frame_key=keys)
    assert torch.equal(alone, frames[a:b])


def test_host_picks_give_the_reference_route(store):
    """with a host-drawn pick table the batches are ``frames_from_raw(pick=...)`` of the same frames: the parity route"""
    from opensetgaitrecognition_pcaa_amd import ops
    view = store.crops(SPLIT.TRAIN, N, C)
    np.random.seed(4)
    picks = datasets.draw_picks(store.cards(), N)
    frames = ops.frames_from_raw(store.points_dev, store.offsets_dev, N, C, pick=torch.from_numpy(picks).cuda())
    crops = torch.stack([frames[s:s + T] for s in view.start.tolist()])
    raw = batcher.RawTrackBatcher(view, B, shuffle=False, picks=picks, redraw="epoch", seed=1)
    for _ in range(2):                                      # supplied picks: the epoch's seed draws nothing
        for k, (p, l) in enumerate(raw):
            assert torch.equal(p.permute(0, 2, 3, 1), crops[k * B:(k + 1) * B])
    raw.check()


def test_epoch_redraw_resamples_the_drawn_part_only(store):
    view = store.crops(SPLIT.TRAIN, N, C)
    cards = store.cards()

    def run():
        ld = batcher.RawTrackBatcher(view, B, shuffle=False, drop_last=False, seed=9, redraw="epoch")
        eps, _ = _epochs(ld, 2, 5)
        ld.check()
        assert ld.seed_of(0) == datasets.epoch_draw_seed(9, 0) != ld.seed_of(1)
        return [torch.cat([p for p, _ in ep]).permute(0, 2, 3, 1).cpu().double().numpy() for ep in eps]   # [M,T,N,C]

    e0, e1 = run()
    again0, again1 = run()
    assert np.array_equal(e0, again0) and np.array_equal(e1, again1), "reproducible from (seed, epoch)"
    differ = n_pad = n_sub = 0
    for i, s in enumerate(view.start.tolist()):
        for t in range(T):
            card = int(cards[s + t])
            a, b = e0[i, t], e1[i, t]
            if card != N and not np.array_equal(a, b):
                differ += 1
            if card == N:
                continue
            if card < N:
                # rows 0 .. card - 1 are the frame's own detections in both epochs; only the mean they are centred by
                # moved.  Each value is rounded to fp32 once (2^-24 relative), so differences of rows agree to
                # 2^-24 (|a_p| + |a_0| + |b_p| + |b_0|) (1 + 2^-20: the bound is formed from the rounded values), plus
                # the 1e-12 s of the fp64 work that the gate of test_raw_frames.py allows (s <= 10 here)
                n_pad += 1
                da, db = a[:card] - a[:1], b[:card] - b[:1]
                tol = 2.0 ** -24 * (np.abs(a[:card]) + np.abs(a[:1]) + np.abs(b[:card]) + np.abs(b[:1])) * (1 + 2.0 ** -20) + 1e-11
                assert (np.abs(da - db) <= tol).all(), (i, t, card)
            else:
                n_sub += 1
    assert differ > 0 and n_pad > 50 and n_sub > 50
    # the fixed draws are another seed's: epoch 0 of "epoch" is not the fixed batcher's epoch
    fixed = batcher.RawTrackBatcher(view, B, shuffle=False, drop_last=False, seed=9)
    f0 = torch.cat([p for p, _ in fixed]).permute(0, 2, 3, 1).cpu().double().numpy()
    assert not np.array_equal(f0, e0)


def test_jitter_moves_whole_tracks_inside_themselves(store):
    from opensetgaitrecognition_pcaa_amd import ops
    view = store.crops(SPLIT.TRAIN, N, C)
    frames = ops.frames_from_raw(store.points_dev, store.offsets_dev, N, C, seed=9, frame_key=store.frame_key_dev)
    ld = batcher.RawTrackBatcher(view, B, shuffle=False, drop_last=False, seed=9, jitter=True)
    moved = 0
    for epoch in range(3):
        starts = view.starts(9, epoch, True)
        assert np.array_equal(ld.starts_of(epoch), starts)
        moved += int((starts != view.start).sum())
        got = torch.cat([p for p, _ in ld]).permute(0, 2, 3, 1)
        assert torch.equal(got, torch.stack([frames[s:s + T] for s in starts.tolist()])), epoch
    ld.check()
    assert moved > 0


def test_an_index_outside_the_view_is_refused_not_faulted(store):
    view = store.crops(SPLIT.TRAIN, N, C)
    ld = batcher.RawTrackBatcher(view, B, seed=9)
    good, _ = ld.batch(torch.tensor([0, 1, 2, 3], device="cuda"))
    ld.check()
    p, l = ld.batch(torch.tensor([0, len(view) + 5, -1, 3], device="cuda"))
    assert torch.equal(p[[0, 3]], good[[0, 3]])
    with pytest.raises(IndexError):
        ld.check()
    # a crop outside the store is refused by the batch kernel itself
    ld2 = batcher.RawTrackBatcher(view, B, seed=9)
    ld2._device()
    ld2._starts = ld2._starts.clone()
    ld2._starts[1] = store.n_frames - T + 1
    p, _ = ld2.batch(torch.tensor([0, 1, 2, 3], device="cuda"))
    assert not p[1].any() and torch.equal(p[[0, 2, 3]], good[[0, 2, 3]])
    with pytest.raises(IndexError):
        ld2.check()


@pytest.mark.timeout(300)
def test_run_loop_and_the_sequential_procedure_from_a_store(tmp_path, monkeypatch):
    """one epoch of variant 4 fed by ``store.crops`` through ``batcher_for`` (N = 32, B = 4), then the open-set procedure on
    the store's sequential TEST / UNSEEN crops: no crop file is written"""
    from opensetgaitrecognition_pcaa_amd import inference
    from opensetgaitrecognition_pcaa_amd.train import train_variant4
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(constants, "NFEATURES", 4)
    plan = ([(0, "train"), (1, "train")] * 2 + [(0, "valid"), (1, "valid"), (0, "test"), (1, "test"), (2, "unseen"),
            (3, "unseen"), (4, "unseen")])
    tracks = [syn.synthetic_raw_track(900 + i, 48 + (i % 3) * 6, max_points=60) for i in range(len(plan))]
    st = datasets.RawTrackStore(tracks, [p[0] for p in plan], ["smartphone"] * len(plan), [str(i) for i in range(len(plan))],
                                splits=[p[1] for p in plan])
    made = []

    def factory(split):
        view = st.crops(split, N, C)
        if split == SPLIT.TRAIN:
            view.batcher_options = dict(seed=3, redraw="epoch", jitter=True)
        made.append(view)
        return view

    cfg = dict(constants.CONFIG)
    cfg.update(MODEL_NAME="raw_V4", TRAIN_CLASSES=[0, 1], NMAX=N, BATCH_SIZE=B, EPOCHS=1, CHECKPOINT_FREQUENCY=1, NOTES="")
    torch.manual_seed(0)
    np.random.seed(0)
    timing = []
    trainer, hist = train_variant4(cfg, wandb_mode="disabled", dataset_factory=factory, timing=timing)
    assert len(hist) == 1 and all(np.isfinite(v) for v in hist[0].values()), hist
    assert timing[0]["train_steps"] == len(made[0]) // B >= 3 and timing[0]["valid_batches"] == len(made[1]) // B >= 1
    assert isinstance(batcher.batcher_for(made[0], B, "cuda", True), batcher.RawTrackBatcher)
    valid = batcher.batcher_for(made[1], B, "cuda", False)
    assert valid.redraw == "fixed" and not valid.jitter and not valid.shuffle
    enc, means = trainer.encoder.eval(), trainer.discriminator_means
    known, known_labels = st.crops(SPLIT.TEST, N, C, order="sequential").materialize()
    unseen, unseen_labels = st.crops(SPLIT.UNSEEN, N, C, order="sequential").materialize()
    assert known.shape[1:] == (C, T, N) and unseen.shape[1:] == (C, T, N)
    preds, labels, thr = inference.naive_sequential_procedure_tensors(2, enc, means, known, known_labels, unseen, unseen_labels)
    assert len(preds) == len(labels) > 0 and np.isfinite(thr) and preds.min() >= 0 and preds.max() <= 2
    assert not list(tmp_path.rglob("crop*.npy")), "no crop files"


@pytest.mark.timeout(300)
def test_the_studies_run_from_a_store_without_crop_files(tmp_path, monkeypatch):
    """``train_pointsubsampling(raw_store=...)`` cut down to one class count, one subset and two NMAX, and
    ``CGAAE_inference(raw_store=...)``: the result files of the file route, no ``generate_splits``, no crop files"""
    import json
    import os
    from opensetgaitrecognition_pcaa_amd import inference
    from opensetgaitrecognition_pcaa_amd.train import train_pointsubsampling
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(constants, "NFEATURES", 4)
    monkeypatch.setattr(constants, "GEN_DATA_PATH", str(tmp_path / "gen"))

    def refuse(*a, **k):
        raise AssertionError("generate_splits was called")

    monkeypatch.setattr(datasets, "generate_splits", refuse)
    tracks, subj, scen, names = [], [], [], []
    for s in range(10):
        for t in range(10):
            tracks.append(syn.synthetic_raw_track(3000 + 10 * s + t, 42 + (t % 2) * 6, max_points=24))
            subj.append(s); scen.append("hands_in_pockets"); names.append(f"{t}{s}")
    st = datasets.RawTrackStore(tracks, subj, scen, names)
    base = dict(constants.CONFIG)
    base.update(EPOCHS=1, BATCH_SIZE=8, CHECKPOINT_FREQUENCY=1, NOTES="", SUBSAMPLE_FACTOR=1.0)
    torch.manual_seed(0)
    res = train_pointsubsampling(n_training_classes=(4,), n_points_subs=(12, 20), n_tests=1, ks=(2,), config=base,
                                 model_name_base="raw_sweep_V4_", raw_store=st)
    assert set(res) == {"raw_sweep_V4_12.4.1", "raw_sweep_V4_20.4.1"}
    for name, log in res.items():
        assert 0.0 <= log[2]["f1_macro"] <= 1.0 and os.path.exists(f"models/{name}/final_preds_2.npy")
        with open(f"models/{name}/naive_seq_log_2.json") as f:
            assert json.load(f)["n_steps"] == 2
    counts = {sp: st.split.count(sp) for sp in SPLIT}
    assert counts == {SPLIT.TRAIN: 32, SPLIT.VALID: 4, SPLIT.TEST: 4, SPLIT.UNSEEN: 60}
    out = inference.CGAAE_inference(["raw_sweep_V4_20.4.1"], ks=[2, 4], variation="V4", raw_store=st)
    assert set(out) == {2, 4} and np.array_equal(np.load("models/raw_sweep_V4_20.4.1/final_labels_2.npy").max(), 4)
    with pytest.raises(ValueError):
        inference.CGAAE_inference(["raw_sweep_V4_20.4.1"], ks=[2], variation="V4", raw_store=st, force_pc_subsampling=10)
    assert not list(tmp_path.rglob("crop*.npy")) and not (tmp_path / "gen").exists()


@pytest.mark.parametrize("drop_last", [True, False])
def test_two_ranks_assemble_the_halves_of_each_global_batch(store, monkeypatch, drop_last):
    """world = 2 in one process (the broadcast of rank 0's order replaced by nothing: both ranks draw it from the same torch
    seed): rank r's batches are rows [r B / 2, (r + 1) B / 2) of the single-process batches, the ragged last one left out"""
    import torch.distributed as dist
    monkeypatch.setattr(dist, "broadcast", lambda tensor, src=0, group=None: None)
    view = store.crops(SPLIT.TRAIN, N, C)
    whole, _ = _epochs(batcher.RawTrackBatcher(view, B, drop_last=drop_last, seed=9, redraw="epoch"), 2, 31)
    ranks = [_epochs(batcher.RawTrackBatcher(view, B, drop_last=drop_last, seed=9, redraw="epoch", rank=r, world=2), 2, 31)[0]
             for r in range(2)]
    for e in range(2):
        full = [b for b in whole[e] if b[0].shape[0] == B]
        assert len(ranks[0][e]) == len(ranks[1][e]) == len(full) == 4
        for (p, l), (p0, l0), (p1, l1) in zip(full, ranks[0][e], ranks[1][e]):
            assert torch.equal(torch.cat([p0, p1]), p) and torch.equal(torch.cat([l0, l1]), l)
