"""The host pieces of raw-frame preparation (no GPU): ``datasets.draw_picks`` + ``frames_from_picks`` against the
reference's own ``process_track`` output (tests/golden/datagen.npz, float64 bit for bit), the numpy restatement of the
device's pick draw (``device_picks_host``), ``pack_raw_frames``, the tick plan's frame keys, the new export."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import T
from opensetgaitrecognition_pcaa_amd import _lib, constants, datasets, synthetic as syn

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "datagen.npz"))
META = json.loads(str(G["meta"]))
TAGS = ("plain", "force10", "divstd")


@pytest.mark.parametrize("tag", TAGS)
def test_draw_picks_and_frames_from_picks_reproduce_the_reference(tag):
    c = META[tag]
    raw = syn.synthetic_raw_track(c["seed"], c["n_frames"])
    cards = [int(fr["cardinality"][0]) for fr in raw]
    assert min(cards) < c["nmax"] <= max(cards), "both the pad and the subsample branch"
    np.random.seed(c["np_seed"])
    picks = datasets.draw_picks(cards, c["nmax"], c["force"])
    assert picks.dtype == np.int32 and picks.shape == (len(raw), c["nmax"])
    assert all(0 <= picks[f].min() and picks[f].max() < cards[f] for f in range(len(raw)))
    got = datasets.frames_from_picks(raw, picks, 4, divide_by_std=c["div"])
    assert got.dtype == np.float64
    assert np.array_equal(got, G[f"{tag}.track"]), tag
    # the same generator calls as process_track: after either, numpy's global generator is in the same state
    after = np.random.random()
    np.random.seed(c["np_seed"])
    want = datasets.process_track(raw, divide_by_std=c["div"], force_pc_subsampling=c["force"], nmax=c["nmax"], nfeatures=4)
    assert np.array_equal(got, want) and after == np.random.random()


def test_frames_from_picks_five_features_equal_process_track():
    raw = syn.synthetic_raw_track(77, 12)
    cards = [int(fr["cardinality"][0]) for fr in raw]
    for div in (False, True):
        np.random.seed(5)
        picks = datasets.draw_picks(cards, 20)
        np.random.seed(5)
        want = datasets.process_track(raw, divide_by_std=div, nmax=20, nfeatures=5)
        assert np.array_equal(datasets.frames_from_picks(raw, picks, 5, divide_by_std=div), want)


def _within_5_sigma(counts, trials, prob):
    sd = np.sqrt(trials * prob * (1 - prob))
    return np.abs(counts - trials * prob).max() <= 5 * sd


def test_device_picks_host():
    n, N = 4000, 24
    keys = np.stack([np.full(n, 3), np.arange(n)], axis=1)
    # pad: card 10 -> N 24: the identity, then 14 draws with replacement per frame
    pad = datasets.device_picks_host(11, keys, np.full(n, 10), N)
    assert pad.dtype == np.int32 and pad.shape == (n, N)
    assert (pad[:, :10] == np.arange(10)).all() and pad.min() >= 0 and pad.max() < 10
    counts = np.bincount(pad[:, 10:].reshape(-1), minlength=10)
    assert _within_5_sigma(counts, n * 14, 1 / 10), counts
    # subsample: card 40 -> N 24 distinct indices per frame, every index kept with probability 24 / 40 ...
    sub = datasets.device_picks_host(11, keys, np.full(n, 40), N)
    assert sub.min() >= 0 and sub.max() < 40
    assert all(len(set(row)) == N for row in sub.tolist())
    counts = np.bincount(sub.reshape(-1), minlength=40)
    assert _within_5_sigma(counts, n, N / 40), counts
    # ... and in random order: the first output point is uniform over the 40
    assert _within_5_sigma(np.bincount(sub[:, 0], minlength=40), n, 1 / 40)
    # card == N is the subsample branch: a permutation
    perm = datasets.device_picks_host(11, keys[:50], np.full(50, N), N)
    assert (np.sort(perm, axis=1) == np.arange(N)).all() and (perm != np.arange(N)).any()
    # the key and the seed both matter; equal (seed, key, card) give equal picks wherever the frame stands
    for cards in (np.full(n, 10), np.full(n, 40)):
        base = datasets.device_picks_host(11, keys, cards, N)
        assert (datasets.device_picks_host(12, keys, cards, N) != base).any(axis=1).mean() > 0.99
        assert (datasets.device_picks_host(11, keys + [1, 0], cards, N) != base).any(axis=1).mean() > 0.99
        assert (datasets.device_picks_host(11, keys + [0, 1], cards, N) != base).any(axis=1).mean() > 0.99
        assert np.array_equal(datasets.device_picks_host(11, keys[100:103][::-1], cards[:3], N), base[100:103][::-1])
    # 64-bit and negative seeds: the low and the high word both enter
    one = datasets.device_picks_host(5, keys[:20], np.full(20, 40), N)
    assert (datasets.device_picks_host(5 + (1 << 32), keys[:20], np.full(20, 40), N) != one).any()
    assert np.array_equal(datasets.device_picks_host(-1, keys[:20], np.full(20, 40), N),
                          datasets.device_picks_host((1 << 64) - 1, keys[:20], np.full(20, 40), N))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_pack_raw_frames_round_trips(dtype):
    raw = syn.synthetic_raw_track(3, 9)
    points, offsets = datasets.pack_raw_frames(raw, dtype)
    cards = [int(fr["cardinality"][0]) for fr in raw]
    assert points.dtype == dtype and tuple(points.shape) == (sum(cards), 5) and points.is_contiguous()
    assert offsets.dtype == torch.int32 and offsets.tolist() == [0] + np.cumsum(cards).tolist()
    np_dtype = np.float32 if dtype == torch.float32 else np.float64
    for f, fr in enumerate(raw):
        rows = points[offsets[f]:offsets[f + 1]].numpy()
        assert np.array_equal(rows[:, :2], fr["elements"].astype(np_dtype))
        for col, name in ((2, "z_coord"), (3, "dopplers"), (4, "powers")):
            assert np.array_equal(rows[:, col], fr[name].astype(np_dtype)), name
    empty_p, empty_o = datasets.pack_raw_frames([], dtype)
    assert tuple(empty_p.shape) == (0, 5) and empty_o.tolist() == [0]
    with pytest.raises(TypeError):
        datasets.pack_raw_frames(raw, torch.float16)


def test_plan_tick_frame_keys_are_additive():
    from opensetgaitrecognition_pcaa_amd.inference import plan_tick
    nf, nw = np.array([40, 0, 7], np.int64), np.array([2, 0, 0], np.int64)
    serials = np.array([5, 9, 6])
    args = (nf, nw, [2, 0, 1], [3, 0, 2], T, constants.CROP_STEP, 4, 47, 4)
    old, new = plan_tick(*args), plan_tick(*args, serials=serials)
    assert old.frame_key is None and "frame_key" not in old.offsets
    assert new.frame_key.dtype == np.int32
    assert new.frame_key.tolist() == [[6, 7], [6, 8], [6, 9], [9, 0], [9, 1]]        # (serial, index in its track)
    for name, (a, b) in old.offsets.items():                                          # everything else as it was
        assert new.offsets[name] == (a, b) and np.array_equal(new.packed[a:b], old.packed[a:b])
    a, b = new.offsets["frame_key"]
    assert a == old.packed.size and b == new.packed.size
    assert np.array_equal(new.packed[a:b].reshape(-1, 2), new.frame_key)
    assert plan_tick(nf, nw, [], [], T, constants.CROP_STEP, 4, 47, 4, serials=serials).frame_key.shape == (0, 2)
    with pytest.raises(ValueError):
        plan_tick(*args, serials=serials[:2])


def test_library_exports_frames_from_raw():
    protos = _lib.parse_header()
    lib = _lib.load()
    assert "pcaa_frames_from_raw" in protos and hasattr(lib, "pcaa_frames_from_raw")
    assert lib.pcaa_abi_version() >= 20
    # argument checks run on the host: N above the cap, C out of range, no picks and no keys
    ok = dict(points=None, f64=0, P=0, offsets=None, n=0, pick=None, key=None, seed=0, N=8, C=4, st=1, div=0, out=None,
              n_out=1, pick_out=None, err=None, stream=None)
    for change in ({"N": 1025}, {"C": 6}, {"C": 0}, {"n_out": 0}, {"n": 2}):
        assert lib.pcaa_frames_from_raw(*{**ok, **change}.values()) != 0, change
