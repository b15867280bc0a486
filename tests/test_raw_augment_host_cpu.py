"""The host side of the raw-track augmentation stage (csrc/raw_frames.hip, the ``_aug`` entry points): argument handling,
the numpy restatement of its draws and of its arithmetic (``datasets.augment_arguments``, ``augment_draws_host``,
``device_noise_host``, ``frames_from_picks(augment=)``) and the option handling of ``RawTrackBatcher``.  No device.

Draw statistics are held to five standard errors of an ideal generator: for n standard normal values the mean has
standard error 1/sqrt(n) and the sample variance sqrt(2/n); the correlation of two independent columns of ``rows`` rows
1/sqrt(rows); a uniform word's mean sqrt(1/(12 n)) and a fair bit's share 0.5/sqrt(n)."""
import math

import numpy as np
import pytest
import torch

from opensetgaitrecognition_pcaa_amd import batcher, datasets, synthetic as syn

FULL = {"yaw": 0.6, "mirror": True, "scale": (0.9, 1.1), "speed": (0.8, 1.25), "noise": [0.02, 0.02, 0.03, 0.1, 1.0]}


# ------------------------------------------------------------------------------------------------- augment_arguments
def test_augment_arguments_spellings():
    A = datasets.augment_arguments
    assert A(FULL) == (0.6, 1.0, 0.9, 1.1, 0.8, 1.25, 0.02, 0.02, 0.03, 0.1, 1.0)
    assert len(A(FULL)) == datasets.AUG_PARAMS == 11
    assert A({"scale": 1.2}) == (0.0, 0.0, 1.2, 1.2, 1.0, 1.0, 0, 0, 0, 0, 0)
    assert A({"speed": [0.5, 2]}) == (0.0, 0.0, 1.0, 1.0, 0.5, 2.0, 0, 0, 0, 0, 0)
    assert A({"noise": (0.1, 0.2)}) == (0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0.1, 0.2, 0, 0, 0)
    assert A({"noise": {"doppler": 0.3, "power": 2}}) == (0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0, 0, 0, 0.3, 2.0)
    assert A({"yaw": math.pi, "mirror": 1})[:2] == (math.pi, 1.0)
    assert A(A(FULL)) == A(FULL), "the parameter form passes through"


@pytest.mark.parametrize("neutral", [None, {}, {"yaw": 0}, {"mirror": False}, {"scale": 1}, {"scale": (1, 1), "speed": 1.0},
                                     {"noise": []}, {"noise": [0, 0, 0, 0, 0]}, {"noise": {"x": 0.0}},
                                     {"yaw": 0.0, "mirror": False, "scale": (1.0, 1.0), "speed": (1, 1), "noise": {}}])
def test_augment_arguments_neutral_is_none(neutral):
    assert datasets.augment_arguments(neutral) is None


@pytest.mark.parametrize("bad", [{"yaw": -0.1}, {"yaw": 3.2}, {"yaw": float("nan")}, {"yaw": float("inf")},
                                 {"scale": 0}, {"scale": (0.0, 1.0)}, {"scale": (-1, 1)}, {"scale": (1.2, 1.1)},
                                 {"scale": (1, float("inf"))}, {"scale": (1, 2, 3)},
                                 {"speed": 0}, {"speed": (-0.5, 1)}, {"speed": (2, 1)}, {"speed": float("nan")},
                                 {"noise": [-0.1]}, {"noise": [0, float("inf")]}, {"noise": {"z": float("nan")}},
                                 {"noise": [0] * 6}, {"noise": {"range": 1.0}}, {"rotate": 0.1}, {"yaw": 0.1, "jitter": 1},
                                 [1.0, 2.0], "yaw"])
def test_augment_arguments_refusals(bad):
    with pytest.raises(ValueError):
        datasets.augment_arguments(bad, "test")


def test_rotation_needs_two_columns():
    raw = syn.synthetic_raw_track(1, 3)
    picks = np.zeros((3, 4), dtype=np.int32)
    with pytest.raises(ValueError):
        datasets.frames_from_picks(raw, picks, 1, augment={"yaw": 0.2}, seed=0, keys=np.zeros((3, 2), dtype=np.int32))
    with pytest.raises(ValueError):
        datasets.frames_from_picks(raw, picks, 4, augment={"yaw": 0.2}, seed=0)            # no keys


# ------------------------------------------------------------------------------------------------ augment_draws_host
def test_track_draws_are_shared_by_a_tracks_frames_and_stay_in_range():
    serials = np.array([5, 5, 6, -3, 2 ** 31 - 1, 5])
    d = datasets.augment_draws_host(11, serials, FULL)
    for name in ("yaw", "mirror", "scale", "speed"):
        assert d[name].shape == (6,)
        assert d[name][0] == d[name][1] == d[name][5], "two frames of one serial: one draw"
    many = datasets.augment_draws_host(11, np.arange(-500, 1500), FULL)
    assert (np.abs(many["yaw"]) < 0.6).all() and (many["scale"] >= 0.9).all() and (many["scale"] <= 1.1).all()
    assert (many["speed"] >= 0.8).all() and (many["speed"] <= 1.25).all() and many["mirror"].dtype == bool
    assert 0 < many["mirror"].sum() < 2000 and len(np.unique(many["yaw"])) == 2000
    # another seed, another serial: another draw
    other = datasets.augment_draws_host(12, serials, FULL)
    assert other["yaw"][0] != d["yaw"][0] and other["scale"][0] != d["scale"][0]
    assert d["yaw"][0] != d["yaw"][2] and d["speed"][0] != d["speed"][2]
    assert datasets.augment_draws_host(11 + 2 ** 32, serials, FULL)["yaw"][0] != d["yaw"][0], "the seed's high word counts"
    # neutral parameters give neutral draws
    n = datasets.augment_draws_host(11, serials, None)
    assert not n["yaw"].any() and not n["mirror"].any() and (n["scale"] == 1).all() and (n["speed"] == 1).all()
    assert not datasets.augment_draws_host(11, serials, {"yaw": 0.3})["mirror"].any()


def test_track_draws_do_not_depend_on_the_frame_number():
    """key[1] is not absorbed: frames_from_picks gives frames (7, 0) and (7, 33) of equal content the same geometry"""
    rng = np.random.default_rng(0)
    fr = {"cardinality": np.array([9]), "elements": rng.standard_normal((9, 2)), "z_coord": rng.standard_normal(9),
          "dopplers": rng.standard_normal(9), "powers": np.exp(rng.standard_normal(9))}
    picks = np.tile(np.arange(9, dtype=np.int32), (2, 1))
    aug = {"yaw": 1.0, "mirror": True, "scale": (0.5, 2.0), "speed": (0.5, 2.0)}
    out = datasets.frames_from_picks([fr, fr], picks, 5, augment=aug, seed=4, keys=[(7, 0), (7, 33)])
    assert np.array_equal(out[0], out[1])
    out = datasets.frames_from_picks([fr, fr], picks, 5, augment=aug, seed=4, keys=[(7, 0), (8, 0)])
    assert not np.array_equal(out[0], out[1])


# --------------------------------------------------------------------------------------------------- draw statistics
@pytest.mark.parametrize("seed", [0, 7, 0x1234567890ab])
def test_gaussian_draw_statistics(seed):
    keys = [(t, f) for t in range(4) for f in range(10)]
    g = np.concatenate(datasets.device_noise_host(seed, keys, [1024] * len(keys), 5))
    rows, n = g.shape[0], g.size
    assert g.shape == (40960, 5) and n == 204800
    corr = np.corrcoef(g, rowvar=False)
    off = np.abs(corr - np.eye(5)).max()
    print(f"[augment draws] seed {seed}: mean {g.mean():.2e} / {5 / math.sqrt(n):.2e}, var - 1 {g.var() - 1:.2e} / "
          f"{5 * math.sqrt(2 / n):.2e}, corr {off:.2e} / {5 / math.sqrt(rows):.2e}, max |g| {np.abs(g).max():.2f}")
    assert abs(g.mean()) <= 5 / math.sqrt(n)
    assert abs(g.var() - 1) <= 5 * math.sqrt(2 / n)
    assert off <= 5 / math.sqrt(rows)
    assert np.isfinite(g).all() and np.abs(g).max() < 7


def test_noise_is_keyed_by_frame_and_raw_index():
    a = datasets.device_noise_host(3, [(1, 2), (1, 3), (1, 2)], [50, 50, 20], 4)
    assert [x.shape for x in a] == [(50, 4), (50, 4), (20, 4)]
    assert np.array_equal(a[0][:20], a[2]) and not np.array_equal(a[0], a[1])
    assert np.array_equal(datasets.device_noise_host(3, [(1, 2)], [50], 2)[0], a[0][:, :2]), "column c does not depend on C"
    assert not np.array_equal(datasets.device_noise_host(4, [(1, 2)], [50], 4)[0], a[0])


def test_uniform_word_statistics():
    n = 20000
    serials = np.arange(n)
    aug = {"yaw": 1.0, "mirror": True, "scale": (1.0, 2.0), "speed": (1.0, 2.0)}
    d = datasets.augment_draws_host(3, serials, aug)
    r = {"r0": (d["yaw"] / 1.0 + 1) / 2, "r2": d["scale"] - 1.0, "r3": d["speed"] - 1.0}
    bound = 5 * math.sqrt(1 / (12 * n))
    for name, v in r.items():
        print(f"[augment draws] {name}: mean - 0.5 = {v.mean() - 0.5:.2e} / {bound:.2e}")
        assert abs(v.mean() - 0.5) <= bound and 0 < v.min() and v.max() < 1
    # r_1 itself: through the restated chain (mirror uses only its top bit)
    seed = 3
    s0 = datasets._absorb32(datasets._absorb32(np.uint64(0x9E3779B9), np.uint64(seed)), np.uint64(0))
    u = datasets._absorb32(datasets._absorb32(s0, serials.astype(np.uint64)), np.uint64(0x6175676D))
    w1 = datasets._absorb32(u, np.uint64(1))
    assert abs(datasets._unit(w1).mean() - 0.5) <= bound
    assert np.array_equal((w1 >> np.uint64(31)) != 0, d["mirror"])
    share = d["mirror"].mean()
    print(f"[augment draws] mirror share - 0.5 = {share - 0.5:.2e} / {5 * 0.5 / math.sqrt(n):.2e}")
    assert abs(share - 0.5) <= 5 * 0.5 / math.sqrt(n)


# --------------------------------------------------------------------------------------- frames_from_picks(augment=)
def _setup(n=12, N=40, seed=5):
    raw = syn.synthetic_raw_track(seed, n)
    cards = [len(fr["z_coord"]) for fr in raw]
    keys = np.array([(f // 4, f) for f in range(n)], dtype=np.int32)
    picks = datasets.device_picks_host(9, keys, cards, N)
    return raw, keys, picks


@pytest.mark.parametrize("div", [False, True])
def test_neutral_augment_is_the_function_without(div):
    raw, keys, picks = _setup()
    plain = datasets.frames_from_picks(raw, picks, 5, div)
    for neutral in (None, {}, {"yaw": 0.0, "scale": (1, 1), "noise": [0, 0]}):
        assert np.array_equal(datasets.frames_from_picks(raw, picks, 5, div, augment=neutral, seed=9, keys=keys), plain)


def test_yaw_only_is_a_rotation_of_xy():
    raw, keys, picks = _setup()
    plain = datasets.frames_from_picks(raw, picks, 5)
    turned = datasets.frames_from_picks(raw, picks, 5, augment={"yaw": 2.5}, seed=9, keys=keys)
    assert np.array_equal(turned[:, :, 2:], plain[:, :, 2:]), "z, Doppler and power are bit-equal"
    assert not np.array_equal(turned[:, :, :2], plain[:, :, :2])
    theta = datasets.augment_draws_host(9, keys[:, 0], {"yaw": 2.5})["yaw"]
    for f, fr in enumerate(raw):
        s = np.abs(fr["elements"][picks[f]]).max()                      # the largest uncentred magnitude
        d0 = np.linalg.norm(plain[f, :, None, :2] - plain[f, None, :, :2], axis=-1)
        d1 = np.linalg.norm(turned[f, :, None, :2] - turned[f, None, :, :2], axis=-1)
        assert np.abs(d1 - d0).max() <= 1e-12 * s, f
        # and it is the rotation by the track's angle, of the centred frame as well (the mean turns with the points)
        c, sn = math.cos(theta[f]), math.sin(theta[f])
        want = np.stack([plain[f, :, 0] * c - plain[f, :, 1] * sn, plain[f, :, 0] * sn + plain[f, :, 1] * c], axis=1)
        assert np.abs(turned[f, :, :2] - want).max() <= 1e-12 * s


def test_order_of_the_steps():
    """noise -> scale / speed -> mirror -> rotation, on the dB columns, before the picks and the centring"""
    raw, keys, picks = _setup(n=4, N=16)
    aug = {"yaw": 1.0, "mirror": True, "scale": (0.7, 1.4), "speed": (0.6, 1.5), "noise": [0.1, 0.2, 0.3, 0.4, 0.5]}
    got = datasets.frames_from_picks(raw, picks, 5, True, augment=aug, seed=21, keys=keys)
    d = datasets.augment_draws_host(21, keys[:, 0], aug)
    g = datasets.device_noise_host(21, keys, [len(fr["z_coord"]) for fr in raw], 5)
    for f, fr in enumerate(raw):
        arr = datasets._raw_columns(fr)
        arr[:, 4] = 10 * np.log10(arr[:, 4] + 1e-8)
        arr = arr + np.array([0.1, 0.2, 0.3, 0.4, 0.5]) * g[f]
        arr[:, :3] *= d["scale"][f]
        arr[:, 3] *= d["speed"][f]
        if d["mirror"][f]:
            arr[:, 0] = -arr[:, 0]
        x, y = arr[:, 0].copy(), arr[:, 1].copy()
        arr[:, 0] = x * math.cos(d["yaw"][f]) - y * math.sin(d["yaw"][f])
        arr[:, 1] = x * math.sin(d["yaw"][f]) + y * math.cos(d["yaw"][f])
        v = arr[picks[f]]
        want = (v - v.mean(axis=0)) / (v.std(axis=0) + 1e-8)
        assert np.abs(got[f] - want).max() <= 1e-12 * np.abs(want).max(), f
    # duplicates of a detection stay equal rows: the noise is keyed by the raw index
    for f in range(len(raw)):
        _, first, inverse = np.unique(picks[f], return_index=True, return_inverse=True)
        assert np.array_equal(got[f], got[f][first][inverse])


# ------------------------------------------------------------------------------------------ RawTrackBatcher options
def _view():
    tracks = [syn.synthetic_raw_track(40 + i, 44, max_points=30) for i in range(4)]
    store = datasets.RawTrackStore(tracks, [0, 1, 0, 1], ["lin"] * 4, [str(i) for i in range(4)], splits=["train"] * 4)
    store.to_device = lambda device="cuda": store                 # batcher_for uploads the store; nothing here has a device
    return store.crops("train", N=16, C=4, scenarios=["lin"])


def test_batcher_for_keeps_augment_for_training_and_drops_it_for_validation():
    view = _view()
    assert len(view) > 0
    view.batcher_options = dict(seed=5, redraw="epoch", augment=FULL, keep_points=8)
    train = batcher.batcher_for(view, 2, "cuda", True)
    valid = batcher.batcher_for(view, 2, "cuda", False)
    assert train.augment == datasets.augment_arguments(FULL) and train.redraw == "epoch" and train.keep_points == 8
    assert valid.augment is None and valid.redraw == "fixed" and valid.keep_points == 0
    assert batcher.RawTrackBatcher(view, 2, augment={"scale": 1}).augment is None
    with pytest.raises(ValueError):
        batcher.RawTrackBatcher(view, 2, augment={"yaw": 4.0})
    with pytest.raises(ValueError):
        batcher.RawTrackBatcher(view, 2, augment={"spin": 1.0})
    # together with supplied picks it is allowed (keep_points is not)
    picks = np.zeros((view.store.n_frames, 16), dtype=np.int32)
    assert batcher.RawTrackBatcher(view, 2, picks=picks, augment=FULL).augment is not None


@pytest.mark.parametrize("redraw", ["fixed", "epoch"])
def test_the_augmented_launch_receives_the_epochs_seed(redraw, monkeypatch):
    view = _view()
    b = batcher.RawTrackBatcher(view, 2, shuffle=False, seed=77, redraw=redraw, augment=FULL)
    seen = []

    def fake(points, offsets, start, T, N, C, **kw):             # stands in for the launch: records what it is given
        seen.append((kw["seed"], kw["prep"].augment))
        return torch.zeros((1, T, N, C))

    monkeypatch.setattr(batcher.ops, "crops_from_raw", fake)
    for epoch in range(3):
        b._set_epoch(epoch)
        b._crops(None)
        assert seen[-1] == (b.seed_of(epoch), datasets.augment_arguments(FULL))
    seeds = [s for s, _ in seen]
    if redraw == "fixed":
        assert seeds == [77, 77, 77]
    else:
        assert seeds == [datasets.epoch_draw_seed(77, e) for e in range(3)] and len(set(seeds)) == 3
