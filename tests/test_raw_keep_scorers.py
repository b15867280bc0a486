"""``keep_points`` through every raw route on the device: the thinned raw routes equal the frame routes on the frames
``ops.frames_from_raw(keep=...)`` wrote, a keep no frame reaches changes nothing, ``dedup_points`` agrees with the padded
thinned route within the gates of tests/raw_unique_ref.py, ``RawTrackBatcher`` thins its batches under the epoch's seed,
and ``CGAAE_inference`` / ``point_sweep`` run the sweep from one resident store.  N = 32, C = 4, K = 4, tracks of 40 - 48
frames with 1 - 40 detections, keep 6 and (4, 12)."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import raw_unique_ref as R
from helpers import T, load_golden, make_encoder
from opensetgaitrecognition_pcaa_amd import batcher, constants, datasets, synthetic as syn
from opensetgaitrecognition_pcaa_amd.constants import SPLIT

K, N, C, HOP = 4, 32, 4, constants.CROP_STEP
KEEPS = [6, (4, 12)]
THRESHOLD = 1e-30


def _track(seed, F):
    """F raw frames of 1 - 40 detections"""
    rng = np.random.default_rng(seed)
    return [R.make_frame(rng, int(n)) for n in rng.integers(1, 41, F)]


def _dev(raw, dtype=torch.float32):
    points, offsets = datasets.pack_raw_frames(raw, dtype)
    return points.cuda(), offsets.cuda()


def _keys(serial, first, n):
    return torch.from_numpy(np.stack([np.full(n, serial), first + np.arange(n)], axis=1).astype(np.int32)).cuda()


def _setup():
    enc = make_encoder(K, N, C, True, seed=0).cuda().eval()
    means = torch.from_numpy(load_golden("misc")[0]["means_K4"]).float()
    return enc, means


def _hi(keep):
    return keep[1] if isinstance(keep, tuple) else keep


@pytest.mark.gpu
@pytest.mark.parametrize("keep", KEEPS, ids=str)
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_thinned_raw_routes_equal_the_frame_routes(mode, keep):
    from opensetgaitrecognition_pcaa_amd import functional as F_hip, inference, ops
    F_hip.set_precision(mode)
    enc, means = _setup()
    raw = _track(41, 48)
    points, offsets = _dev(raw)
    kw = dict(keep=keep, keep_rule="random")
    # the whole track
    sc = inference.OpenSetScorer(enc, means)
    got = sc.embed_raw_track(points, offsets, seed=5, track_key=7, keep_points=keep, keep_rule="random")
    frames = ops.frames_from_raw(points, offsets, N, C, seed=5, frame_key=_keys(7, 0, 48), **kw)
    want = sc.embed_track(frames)
    assert got[0].numel() == inference.window_count(48) > 0
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    plain = ops.frames_from_raw(points, offsets, N, C, seed=5, frame_key=_keys(7, 0, 48))
    assert not torch.equal(frames, plain), "the keep thins something"
    # a keep no frame reaches is no keep at all
    for noop in (40, (40, 64), 1024):
        same = sc.embed_raw_track(points, offsets, seed=5, track_key=7, keep_points=noop, keep_rule="random")
        for g, w in zip(same, sc.embed_raw_track(points, offsets, seed=5, track_key=7)):
            assert torch.equal(g, w), noop
    # a live track, a few frames at a time
    a = inference.StreamingScorer(enc, means, THRESHOLD, 3, K, max_push=16, seed=5, keep_points=keep, keep_rule="random")
    b = inference.StreamingScorer(enc, means, THRESHOLD, 3, K, max_push=16)
    pos = 0
    for n in (7, 20, 0, 21):
        p, o = _dev(raw[pos:pos + n])
        got = a.push_raw(p, o)
        want = b.push(ops.frames_from_raw(p, o, N, C, seed=5, frame_key=_keys(a.serial, pos, n), **kw))
        for g, w in zip(got, want):
            assert torch.equal(g, w), pos
        pos += n
    assert a.n_windows == b.n_windows == (48 - T) // HOP + 1 and torch.equal(a.votes(), b.votes())
    # two live tracks in one tick
    tracks = [raw, _track(42, 44)]
    ms = inference.MultiStreamScorer(enc, means, THRESHOLD, 2, K, max_streams=2, max_push=8, seed=9, keep_points=keep,
                                     keep_rule="random")
    mf = inference.MultiStreamScorer(enc, means, THRESHOLD, 2, K, max_streams=2, max_push=8)
    sids = [ms.open(), ms.open()]
    assert [mf.open(), mf.open()] == sids
    at, windows = [0, 0], 0
    while at[1] < 44:
        counts = [min(8, 48 - at[0]), min(7, 44 - at[1])]
        chunk = [fr for s in range(2) for fr in tracks[s][at[s]:at[s] + counts[s]]]
        keys = torch.cat([_keys(ms.track_serial[sids[s]], at[s], counts[s]) for s in range(2)])
        p, o = _dev(chunk)
        got = ms.push_raw(sids, counts, p, o)
        want = mf.push(sids, counts, ops.frames_from_raw(p, o, N, C, seed=9, frame_key=keys, **kw))
        assert np.array_equal(got.stream, want.stream) and np.array_equal(got.window, want.window)
        for name in ("preds", "sup_fv", "lik", "votes"):
            assert torch.equal(getattr(got, name), getattr(want, name)), (name, at)
        windows += len(got)
        at = [at[s] + counts[s] for s in range(2)]
    assert windows >= 6 and ms.raw_err.item() == 0 and a.raw_err.item() == 0 and sc.raw_err.item() == 0
    with pytest.raises(ValueError, match="supplied picks"):
        sc.embed_raw_track(points, offsets, pick=torch.zeros((48, N), dtype=torch.int32, device="cuda"), keep_points=keep)


def _thinned_frames64(raw, serial, seed, keep, rule):
    """the thinned padded frames in fp64 on the host: the restated picks, the arithmetic of frames_from_picks"""
    keys = np.stack([np.full(len(raw), serial), np.arange(len(raw))], axis=1)
    picks = datasets.device_picks_host(seed, keys, R.cards_of(raw), N, keep=keep, keep_rule=rule)
    return datasets.frames_from_picks(raw, picks, C)


_LOGITS = {}


def _oracle_safe(enc, raw, serial, seed, keep, rule, mode):
    """the margin rule of the fp64 oracle on the track's eager windows (the logits are computed once per keep)"""
    tag = (serial, seed, keep, rule, len(raw))
    if tag not in _LOGITS:
        sd = R.sd64(enc)
        _LOGITS[tag] = R.oracle_window_logits(sd, R.oracle_frame_features(sd, _thinned_frames64(raw, serial, seed, keep, rule)),
                                              T, HOP, True)
    return R.safe_windows(_LOGITS[tag], mode)


def test_the_oracle_alone_excludes_few_windows():
    """no GPU work: the fp64 oracle's margin rule on the thinned track of the test below leaves at least 90 % of its
    windows to compare labels on, in both modes and for both keeps"""
    enc = make_encoder(K, N, C, True, seed=0).eval()
    raw = _track(41, 48)
    for keep in KEEPS:
        for mode in ("fp32", "bf16"):
            safe = _oracle_safe(enc, raw, 7, 5, keep, "first", mode)
            assert safe.size == (48 - T) // HOP + 1 and (~safe).sum() <= R.MAX_EXCLUDED * safe.size, (keep, mode, safe)
            assert (~safe[:3]).sum() <= R.MAX_EXCLUDED * 3                     # ... and of the 3 that embed_raw_track scores


@pytest.mark.gpu
@pytest.mark.parametrize("keep", KEEPS, ids=str)
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_dedup_points_agrees_with_the_padded_thinned_route(mode, keep):
    from opensetgaitrecognition_pcaa_amd import functional as F_hip, inference, ops
    F_hip.set_precision(mode)
    enc, means = _setup()
    raw = _track(41, 48)
    points, offsets = _dev(raw)
    sc = inference.OpenSetScorer(enc, means)
    on = sc.embed_raw_track(points, offsets, seed=5, track_key=7, dedup_points=True, keep_points=keep)
    rows_run, frames_run = sc.last_rows_encoded, sc.last_frames_encoded
    off = sc.embed_raw_track(points, offsets, seed=5, track_key=7, keep_points=keep)
    sc.embed_raw_track(points, offsets, seed=5, track_key=7, dedup_points=True)
    rows_plain = sc.last_rows_encoded
    # the table holds at most frames * min(keep, N) rows, in whole GEMM tiles (ops.UNIQUE_ROW_QUANTUM)
    assert rows_run == ops.unique_table_rows(points.shape[0], frames_run, N, _hi(keep))
    assert rows_run <= ops.unique_chunk_rows(frames_run * min(_hi(keep), N)) and rows_run < rows_plain
    eager = _oracle_safe(enc, raw, 7, 5, keep, "first", mode)
    W = inference.window_count(48)                                             # the reference's rule drops the aligned last one
    safe = eager[:W]
    gate = R.MODE_GATE[mode]
    fv_on, fv_off = on[1].cpu().numpy(), off[1].cpu().numpy()
    scale = np.abs(fv_off).max()
    e_fv = np.abs(fv_on - fv_off).max() / scale
    excluded = int((~safe).sum())
    print(f"[keep dedup] {mode} keep={keep}: sup_fv difference {e_fv:.2e} of scale (gate {gate:.0e}); {excluded} of {safe.size} "
          f"windows excluded; rows {rows_run} against {rows_plain} without keep")
    assert on[0].numel() == off[0].numel() == safe.size
    assert e_fv <= gate
    assert excluded <= R.MAX_EXCLUDED * safe.size
    assert np.array_equal(on[0].cpu().numpy()[safe], off[0].cpu().numpy()[safe])
    lik_on, lik_off = on[2].cpu().numpy(), off[2].cpu().numpy()
    room = R.lik_rel_bound(fv_off, means.numpy(), gate * scale) * np.where(lik_off > 0, lik_off, 0.0)
    assert (np.abs(lik_on - lik_off) <= np.nan_to_num(room, nan=0.0, posinf=np.inf)).all()
    # the live scorers take the two options together
    a = inference.StreamingScorer(enc, means, THRESHOLD, 3, K, max_push=16, seed=5, dedup_points=True, keep_points=keep)
    ms = inference.MultiStreamScorer(enc, means, THRESHOLD, 2, K, max_streams=1, max_push=48, seed=5, dedup_points=True,
                                     keep_points=keep)
    a.serial = 7
    sid = ms.open()
    ms.track_serial[sid] = 7
    live = a.push_raw(points, offsets)
    tick = ms.push_raw([sid], [48], points, offsets)
    for got in (live[1], tick.sup_fv):                                         # eager: one window more, the first W the same
        assert got.shape[0] == eager.size and np.abs(got[:W].cpu().numpy() - fv_off).max() / scale <= gate
    assert sc.raw_err.item() == 0 and a.raw_err.item() == 0 and ms.raw_err.item() == 0


@pytest.fixture(scope="module")
def store():
    tracks = [_track(700 + i, F) for i, F in enumerate((40, 47, 44, 48, 42))]
    st = datasets.RawTrackStore(tracks, [0, 1, 2, 0, 1], ["free_walk"] * 5, ["3", "10", "4", "21", "7"], splits=["train"] * 5,
                                serials=[11, 5, 8, 2, 30])
    return st.to_device("cuda")


@pytest.mark.gpu
def test_batcher_thins_under_the_epochs_seed_and_a_train_step_runs(store):
    from opensetgaitrecognition_pcaa_amd import ops
    from opensetgaitrecognition_pcaa_amd.train import PCAATrainer
    B = 4
    view = store.crops(SPLIT.TRAIN, N, C)
    ld = batcher.RawTrackBatcher(view, B, shuffle=False, drop_last=False, seed=9, redraw="epoch", keep_points=(4, 12),
                                 keep_rule="random")
    epochs = []
    for epoch in range(2):
        frames = ops.frames_from_raw(store.points_dev, store.offsets_dev, N, C, seed=ld.seed_of(epoch),
                                     frame_key=store.frame_key_dev, keep=(4, 12), keep_rule="random")
        got = torch.cat([p for p, _ in ld]).permute(0, 2, 3, 1)
        assert torch.equal(got, torch.stack([frames[s:s + T] for s in view.start.tolist()])), epoch
        epochs.append(got)
    ld.check()
    assert not torch.equal(epochs[0], epochs[1]), "counts and sets are re-drawn per epoch"
    whole = torch.cat([p for p, _ in batcher.RawTrackBatcher(view, B, shuffle=False, drop_last=False, seed=9)])
    distinct = lambda x: len(np.unique(x[0, 0].cpu().numpy(), axis=0))                      # rows of crop 0, frame 0
    assert distinct(epochs[0]) <= 12 and not torch.equal(epochs[0], whole.permute(0, 2, 3, 1))
    # batcher_for: the options travel with the view; the validation loader sees the frames whole
    view.batcher_options = dict(seed=9, redraw="epoch", keep_points=(4, 12), keep_rule="random")
    train, valid = batcher.batcher_for(view, B, "cuda", True), batcher.batcher_for(view, B, "cuda", False)
    assert train.keep_points == (4, 12) and train.keep_rule == "random" and valid.keep_points == 0
    view.batcher_options = {}
    # one train step on a thinned batch
    constants.NFEATURES = C
    cfg = dict(constants.CONFIG)
    cfg.update(NMAX=N, TRAIN_CLASSES=list(range(3)), BATCH_SIZE=B)
    tr = PCAATrainer(cfg)
    for i, m in enumerate((tr.encoder, tr.decoder, tr.discriminator, tr.decoder_projection_head, tr.discriminator_projection_head)):
        syn.deterministic_fill_(m, 50 + i)
    tr.sample_prior_means()
    tr.finalize()
    tr.train()
    pcs, labels = next(iter(train))
    out = tr.step(pcs, labels, syn.synthetic_z0(B, 32, seed=80).cuda(), syn.synthetic_alphas(B, seed=90).cuda())
    torch.cuda.synchronize()
    assert all(np.isfinite(out[k].item()) for k in ("d_loss", "rec_loss", "sup_loss", "tot_loss")), out


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_the_sweep_runs_from_one_resident_store(tmp_path, monkeypatch):
    """``CGAAE_inference(raw_store=..., keep_points=6)`` writes the reference's ``_subsampled6`` files; ``point_sweep``
    returns one entry per keep, and where no frame reaches the keep it is the plain evaluation; no crop file anywhere"""
    from opensetgaitrecognition_pcaa_amd import functional as F_hip, inference
    F_hip.set_precision("fp32")
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(constants, "NFEATURES", C)
    monkeypatch.setattr(constants, "GEN_DATA_PATH", str(tmp_path / "gen"))

    def refuse(*a, **k):
        raise AssertionError("generate_splits was called")

    monkeypatch.setattr(datasets, "generate_splits", refuse)
    tracks, subj, names = [], [], []
    for s in range(10):
        for t in range(10):
            tracks.append(_track(3000 + 10 * s + t, 42 + (t % 2) * 6))
            subj.append(s)
            names.append(f"{t}{s}")
    st = datasets.RawTrackStore(tracks, subj, ["hands_in_pockets"] * 100, names)
    name = "keep_V4"
    os.makedirs(f"models/{name}")
    enc = make_encoder(K, N, C, True, seed=0)
    torch.save(enc.state_dict(), f"models/{name}/{name}_E.pt")
    torch.save(torch.from_numpy(load_golden("misc")[0]["means_K4"]).float(), f"models/{name}/discriminator_means.pt")
    with open(f"models/{name}/config.pkl", "wb") as f:
        pickle.dump({"TRAIN_CLASSES": [0, 1, 2, 3], "NMAX": N}, f)
    ks = [2, 4]
    out = inference.CGAAE_inference([name], ks=ks, variation="V4", raw_store=st, keep_points=6, dedup_frames=True)
    assert set(out) == {2, 4}
    with open(f"models/{name}/naive_seq_log_2_subsampled6.json") as f:
        log6 = json.load(f)
    assert log6["n_steps"] == 2 and 0.0 <= log6["accuracy"] <= 1.0
    assert os.path.exists(f"models/{name}/final_preds_2_subsampled6.npy") and os.path.exists(f"models/{name}/naive_seq_log_subsampled6.json")
    assert np.load(f"models/{name}/final_labels_4_subsampled6.npy").max() == 4
    plain = inference.CGAAE_inference([name], ks=ks, variation="V4", raw_store=st, dedup_frames=True)
    with open(f"models/{name}/naive_seq_log_2.json") as f:
        log_plain = json.load(f)
    enc, means = inference.CGAAE_inference_setup(name, 32, "V4", generate_dataset=False, device="cuda")
    keeps = [6, (4, 12), 40]
    sweep = inference.point_sweep(enc, means, st, keeps, ks, N, dedup_points=False)
    assert list(sweep) == keeps and all(set(sweep[k]) == {2, 4} for k in keeps)
    assert sweep[6][2] == log6 and sweep[40][2] == log_plain                  # keep >= every card: the plain evaluation
    assert {m: sweep[40][4][m] for m in plain[4]} == plain[4]
    dedup = inference.point_sweep(enc, means, st, [6], ks, N)                  # dedup_points: the same curve within votes
    assert set(dedup[6]) == {2, 4} and all(0.0 <= dedup[6][k]["accuracy"] <= 1.0 for k in ks)
    assert not list(tmp_path.rglob("crop*.npy")) and not (tmp_path / "gen").exists()
