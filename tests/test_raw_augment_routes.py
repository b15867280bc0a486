"""``augment=`` through every raw route on the device: ``RawTrackBatcher`` draws under the epoch's seed, ``embed_raw_track``
equals ``embed_track`` of the augmented frames (and its ``dedup_points`` route agrees within the gates of
tests/raw_unique_ref.py, as the thinned route does in test_raw_keep_scorers.py), ``perturbation_sweep`` is the sibling of
``point_sweep``, and one epoch of variant 4 trains from an augmenting batcher.  N = 32, C = 4, K = 4."""
import numpy as np
import pytest
import torch

import raw_unique_ref as R
from helpers import T
from test_raw_keep_scorers import _dev, _keys, _setup, _track
from opensetgaitrecognition_pcaa_amd import batcher, constants, datasets, synthetic as syn
from opensetgaitrecognition_pcaa_amd.constants import SPLIT

pytestmark = pytest.mark.gpu

K, N, C, B, HOP = 4, 32, 4, 4, constants.CROP_STEP
AUG = {"yaw": 0.8, "mirror": True, "scale": (0.85, 1.15), "speed": (0.8, 1.2), "noise": [0.03, 0.03, 0.04, 0.15]}
LENGTHS = (40, 47, 53, 60, 44, 51)


@pytest.fixture(scope="module")
def store():
    tracks = [syn.synthetic_raw_track(800 + i, F, max_points=60) for i, F in enumerate(LENGTHS)]
    st = datasets.RawTrackStore(tracks, [0, 1, 2, 0, 1, 2], ["free_walk"] * 6, ["3", "10", "4", "21", "7", "9"],
                                splits=["train"] * 6, serials=[11, 5, 8, 2, 30, 17])
    return st.to_device("cuda")


def _all(loader):
    return torch.cat([p for p, _ in loader]).permute(0, 2, 3, 1)                  # [M, T, N, C]


def test_batcher_augments_under_the_epochs_seed(store):
    from opensetgaitrecognition_pcaa_amd import ops
    view = store.crops(SPLIT.TRAIN, N, C)
    start = torch.from_numpy(view.start.astype(np.int32)).cuda()
    ld = batcher.RawTrackBatcher(view, B, shuffle=False, drop_last=False, seed=9, redraw="epoch", augment=AUG)
    twin = batcher.RawTrackBatcher(view, B, shuffle=False, drop_last=False, seed=9, redraw="epoch", augment=AUG)
    epochs = []
    for epoch in range(2):
        want = ops.crops_from_raw(store.points_dev, store.offsets_dev, start, T, N, C, seed=ld.seed_of(epoch),
                                  frame_key=store.frame_key_dev, augment=AUG)
        got = _all(ld)
        assert torch.equal(got, want), epoch
        assert torch.equal(_all(twin), got), "the same (seed, epoch): the same bits"
        epochs.append(got)
    ld.check()
    assert not torch.equal(epochs[0], epochs[1]), "the draws are renewed per epoch"
    plain = _all(batcher.RawTrackBatcher(view, B, shuffle=False, drop_last=False, seed=9, redraw="epoch"))
    assert not torch.equal(plain, epochs[0])
    # all windows of a track share its draws: overlapping windows hold the same frames
    hop = view.hop
    same_track = [(a, b) for a in range(len(view)) for b in range(len(view))
                  if view.track[a] == view.track[b] and view.start[b] - view.start[a] == hop]
    assert same_track
    for a, b in same_track:
        assert torch.equal(epochs[0][a, hop:], epochs[0][b, :T - hop])
    # fixed: every epoch the same
    fixed = batcher.RawTrackBatcher(view, B, shuffle=False, drop_last=False, seed=9, redraw="fixed", augment=AUG)
    first = _all(fixed)
    assert torch.equal(_all(fixed), first) and not torch.equal(first, plain)
    # with supplied picks and with keep_points
    picks = torch.from_numpy(datasets.device_picks_host(4, store.frame_key.numpy(), store.cards(), N)).cuda()
    for kw, okw in ((dict(picks=picks), dict(pick=picks)), (dict(keep_points=(4, 12), keep_rule="random"),
                                                            dict(keep=(4, 12), keep_rule="random"))):
        ld2 = batcher.RawTrackBatcher(view, B, shuffle=False, drop_last=False, seed=9, augment=AUG, **kw)
        want = ops.crops_from_raw(store.points_dev, store.offsets_dev, start, T, N, C, seed=9, frame_key=store.frame_key_dev,
                                  augment=AUG, **okw)
        assert torch.equal(_all(ld2), want)
        ld2.check()
    # batcher_for: the validation loader is not augmented
    view.batcher_options = dict(seed=9, redraw="epoch", augment=AUG)
    try:
        train, valid = batcher.batcher_for(view, B, "cuda", True), batcher.batcher_for(view, B, "cuda", False)
        assert train.augment is not None and valid.augment is None
        bare = batcher.RawTrackBatcher(view, B, shuffle=False, seed=9)
        assert torch.equal(_all(valid), _all(bare))
    finally:
        view.batcher_options = {}


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_embed_raw_track_is_embed_track_of_the_augmented_frames(mode):
    from opensetgaitrecognition_pcaa_amd import functional as F_hip, inference, ops
    F_hip.set_precision(mode)
    enc, means = _setup()
    raw = _track(41, 48)
    points, offsets = _dev(raw)
    sc = inference.OpenSetScorer(enc, means)
    frames = ops.frames_from_raw(points, offsets, N, C, seed=5, frame_key=_keys(7, 0, 48), augment=AUG)
    want = sc.embed_track(frames)
    off = sc.embed_raw_track(points, offsets, seed=5, track_key=7, augment=AUG)
    assert off[0].numel() == inference.window_count(48) > 0
    for g, w in zip(off, want):
        assert torch.equal(g, w)
    plain = sc.embed_raw_track(points, offsets, seed=5, track_key=7)
    assert not torch.equal(plain[1], off[1])
    for g, w in zip(sc.embed_raw_track(points, offsets, seed=5, track_key=7, augment={"scale": 1.0}), plain):
        assert torch.equal(g, w), "a neutral augment is today's call"
    # supplied picks: the keys are formed from track_key all the same
    picks = torch.from_numpy(datasets.device_picks_host(3, _keys(7, 0, 48).cpu().numpy(), R.cards_of(raw), N)).cuda()
    got = sc.embed_raw_track(points, offsets, pick=picks, seed=5, track_key=7, augment=AUG)
    want = sc.embed_track(ops.frames_from_raw(points, offsets, N, C, pick=picks, seed=5, frame_key=_keys(7, 0, 48), augment=AUG))
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    # dedup_points: the comparison of test_raw_keep_scorers.test_dedup_points_agrees_with_the_padded_thinned_route
    on = sc.embed_raw_track(points, offsets, seed=5, track_key=7, dedup_points=True, augment=AUG)
    keys = np.stack([np.full(48, 7), np.arange(48)], axis=1)
    frames64 = datasets.frames_from_picks(raw, datasets.device_picks_host(5, keys, R.cards_of(raw), N), C, augment=AUG, seed=5,
                                          keys=keys)
    sd = R.sd64(enc)
    logits = R.oracle_window_logits(sd, R.oracle_frame_features(sd, frames64), T, HOP, True)
    safe = R.safe_windows(logits, mode)[:inference.window_count(48)]
    gate = R.MODE_GATE[mode]
    fv_on, fv_off = on[1].cpu().numpy(), off[1].cpu().numpy()
    scale = np.abs(fv_off).max()
    e_fv = np.abs(fv_on - fv_off).max() / scale
    print(f"[augment dedup] {mode}: sup_fv difference {e_fv:.2e} of scale (gate {gate:.0e}); {int((~safe).sum())} of {safe.size} "
          "windows excluded")
    assert on[0].numel() == off[0].numel() == safe.size
    assert e_fv <= gate
    assert (~safe).sum() <= R.MAX_EXCLUDED * safe.size
    assert np.array_equal(on[0].cpu().numpy()[safe], off[0].cpu().numpy()[safe])
    assert sc.raw_err.item() == 0


@pytest.mark.timeout(300)
def test_perturbation_sweep(tmp_path, monkeypatch):
    from opensetgaitrecognition_pcaa_amd import functional as F_hip, inference
    F_hip.set_precision("fp32")
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(constants, "NFEATURES", C)
    tracks, subj, names = [], [], []
    for s in range(10):
        for t in range(10):
            tracks.append(_track(3000 + 10 * s + t, 42 + (t % 2) * 6))
            subj.append(s)
            names.append(f"{t}{s}")
    st = datasets.RawTrackStore(tracks, subj, ["hands_in_pockets"] * 100, names)
    st.assign_like_generate_splits([0, 1, 2, 3]).to_device("cuda")
    enc, means = _setup()
    ks = [2, 4]
    noisy = {"noise": {"x": 0.5, "y": 0.5, "doppler": 1.0}, "yaw": 1.0}
    augments = {"clean": None, "also clean": {"scale": 1.0}, "noisy": noisy}
    refit = inference.perturbation_sweep(enc, means, st, augments, ks, N, refit=True)
    points = inference.point_sweep(enc, means, st, [0], ks, N)
    assert list(refit) == list(augments) and all(set(refit[n]) == set(ks) for n in augments)
    assert refit["clean"] == points[0] and refit["also clean"] == points[0]
    assert all(0.0 <= refit["noisy"][k]["accuracy"] <= 1.0 for k in ks)
    # refit=False: the clean threshold meets the degraded crops
    deployed = inference.perturbation_sweep(enc, means, st, augments, ks, N)
    assert deployed["clean"] == points[0], "on the crops it was fitted on, the clean threshold is the refit one"
    scorer = inference.OpenSetScorer(enc, means)
    sets = {}
    for name in ("clean", "noisy"):
        sets[name] = []
        for split in (SPLIT.TEST, SPLIT.UNSEEN):
            pcs, labels = inference._sequential_split_from_store(st, split, constants.TRAIN_SCENARIOS, N,
                                                                 augment=augments[name], seed=0)
            preds, _, lik = scorer.embed(pcs, dedup_frames=True, dedup_points=True)
            sets[name] += [(preds, lik), labels]
    clean_thr = inference._sequential_votes(ks[0], scorer, *sets["clean"])[2]
    noisy_thr = inference._sequential_votes(ks[0], scorer, *sets["noisy"])[2]
    for k in ks:
        preds, labels, thr = inference._sequential_votes(k, scorer, *sets["noisy"], threshold=clean_thr)
        assert thr == clean_thr and scorer.threshold == clean_thr
        assert deployed["noisy"][k] == inference._metrics(k, preds, labels.astype(int))
    print(f"[perturbation sweep] thresholds clean {clean_thr:.3e} noisy {noisy_thr:.3e}; accuracy clean "
          f"{deployed['clean'][2]['accuracy']:.3f} deployed {deployed['noisy'][2]['accuracy']:.3f} refit {refit['noisy'][2]['accuracy']:.3f}")
    assert not list(tmp_path.rglob("*.json")) and not list(tmp_path.rglob("*.npy")), "writes no file"


@pytest.mark.timeout(300)
def test_one_epoch_of_variant_4_from_an_augmenting_batcher(tmp_path, monkeypatch):
    from opensetgaitrecognition_pcaa_amd.train import train_variant4
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(constants, "NFEATURES", C)
    plan = [(0, "train"), (1, "train")] * 2 + [(0, "valid"), (1, "valid")]
    tracks = [syn.synthetic_raw_track(900 + i, 48 + (i % 3) * 6, max_points=60) for i in range(len(plan))]
    st = datasets.RawTrackStore(tracks, [p[0] for p in plan], ["smartphone"] * len(plan), [str(i) for i in range(len(plan))],
                                splits=[p[1] for p in plan])

    def factory(split):
        view = st.crops(split, N, C)
        view.batcher_options = dict(seed=1, redraw="epoch", augment=AUG)
        return view

    made = []
    real = batcher.batcher_for

    def recording(*a, **k):
        made.append(real(*a, **k))
        return made[-1]

    monkeypatch.setattr(batcher, "batcher_for", recording)
    cfg = dict(constants.CONFIG)
    cfg.update(MODEL_NAME="aug_V4", TRAIN_CLASSES=[0, 1], NMAX=N, BATCH_SIZE=B, EPOCHS=1, CHECKPOINT_FREQUENCY=1, NOTES="")
    torch.manual_seed(0)
    np.random.seed(0)
    trainer, hist = train_variant4(cfg, wandb_mode="disabled", dataset_factory=factory)
    assert len(hist) == 1 and all(np.isfinite(v) for v in hist[0].values()), hist
    assert len(made) == 2 and made[0].augment == datasets.augment_arguments(AUG) and made[0].redraw == "epoch"
    assert made[1].augment is None and made[1].redraw == "fixed", "the validation loader sees the frames as measured"
    for ld in made:
        ld.check()
