"""The host side of thinning raw frames (no GPU): the rule of csrc/raw_frames.hip as ``datasets.device_picks_host(keep=...)``
restates it -- its properties on the families the kernels are tested on --, the table size with ``keep``, the three
``_thin`` exports with their argument checks (they return before any launch), and the refusals of the Python surface."""
import ctypes

import numpy as np
import pytest
import torch

from opensetgaitrecognition_pcaa_amd import _lib, batcher, datasets, inference, ops, synthetic as syn
from opensetgaitrecognition_pcaa_amd.constants import SPLIT

N_FRAMES = 400
SEED = 5
NS = (8, 150, 300)
RULES = ("first", "random")


def _family():
    rng = np.random.default_rng(0)
    cards = rng.integers(1, 60, N_FRAMES)
    cards[:6] = [1, 2, 1024, 150, 151, 149]
    return cards, np.stack([np.full(N_FRAMES, 7), np.arange(N_FRAMES)], axis=1)


CARDS, KEYS = _family()
BASE = {N: datasets.device_picks_host(SEED, KEYS, CARDS, N) for N in NS}      # today's picks, drawn once


def _keeps(N):
    return (1, 5, 20, (5, 20), N, N + 7, 1024)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("N", NS)
def test_the_rule_on_every_family(N, rule):
    for keep in _keeps(N):
        picks = datasets.device_picks_host(SEED, KEYS, CARDS, N, keep=keep, keep_rule=rule)
        kept = datasets.device_keep_host(SEED, KEYS, CARDS, keep, keep_rule=rule)
        lo, hi = keep if isinstance(keep, tuple) else (keep, keep)
        lens = np.array([len(k) for k in kept])
        assert picks.dtype == np.int32 and picks.shape == (N_FRAMES, N)
        assert (lens <= np.minimum(CARDS, hi)).all() and (lens >= np.minimum(CARDS, lo)).all(), keep
        untouched = lens == CARDS                                  # k_f >= card: today's integers
        assert np.array_equal(picks[untouched], BASE[N][untouched]), keep
        if hi == 1024:
            assert untouched.all()
        for f in range(N_FRAMES):
            support, mine = set(picks[f].tolist()), set(kept[f].tolist())
            assert support <= mine and max(mine) < CARDS[f], (keep, f)           # every pick lies in the kept set
            if N >= lens[f]:
                assert support == mine, (keep, f)                                # every kept index is picked
            else:
                assert len(support) == N, (keep, f)                              # a subset without replacement
            if rule == "first":
                assert mine == set(range(lens[f]))


def test_default_arguments_are_todays_integers():
    for N in NS:
        assert np.array_equal(datasets.device_picks_host(SEED, KEYS, CARDS, N, 0, None, "first"), BASE[N])
        assert np.array_equal(datasets.device_picks_host(SEED, KEYS, CARDS, N, keep=None, keep_rule="random"), BASE[N])
    # ... and what they were before the keyword existed: the chain written out for one pad and one subsample frame
    A = datasets._absorb32
    s = np.uint64(0x9E3779B9)
    for w in (SEED, 0, 7, 3):
        s = A(s, np.uint64(w))
    card, N = int(CARDS[3]), 8
    h = A(s, np.arange(card, dtype=np.uint64))
    assert card >= N and np.array_equal(BASE[N][3], np.lexsort((np.arange(card), h))[:N])
    s = A(A(A(A(np.uint64(0x9E3779B9), np.uint64(SEED)), np.uint64(0)), np.uint64(7)), np.uint64(1))
    want = np.concatenate([np.arange(2), (A(s, np.arange(2, 8, dtype=np.uint64)) * np.uint64(2)) >> np.uint64(32)])
    assert CARDS[1] == 2 and np.array_equal(BASE[8][1], want)


def test_first_has_the_support_of_the_references_quirk():
    np.random.seed(3)
    ref = datasets.draw_picks(CARDS, 150, force_pc_subsampling=20)
    got = datasets.device_picks_host(SEED, KEYS, CARDS, 150, keep=20, keep_rule="first")
    assert all(set(ref[f].tolist()) == set(got[f].tolist()) for f in range(N_FRAMES))


def test_random_keeps_every_detection_about_equally_often_and_counts_cover_their_range():
    m = 4000
    keys = np.stack([np.full(m, 9), np.arange(m)], axis=1)
    share = np.zeros(40)
    for k in datasets.device_keep_host(1, keys, np.full(m, 40), 10, keep_rule="random"):
        assert len(k) == len(set(k.tolist())) == 10
        share[k] += 1
    share /= m
    # 10 of 40 kept: p = 0.25, sd of a share over 4000 frames = sqrt(p (1 - p) / m) = 0.0068; five sd
    assert (np.abs(share - 0.25) < 5 * np.sqrt(0.25 * 0.75 / m)).all(), (share.min(), share.max())
    counts = np.array([len(k) for k in datasets.device_keep_host(1, keys, np.full(m, 40), (5, 20), keep_rule="random")])
    assert counts.min() == 5 and counts.max() == 20 and set(counts.tolist()) == set(range(5, 21))
    # uniform on 16 values: mean 12.5, sd of the mean = sqrt((16^2 - 1) / 12 / m) = 0.073; five sd
    assert abs(counts.mean() - 12.5) < 5 * np.sqrt(255 / 12 / m), counts.mean()
    # the count of a frame does not depend on the rule, and an epoch seed draws other counts and other sets
    first = np.array([len(k) for k in datasets.device_keep_host(1, keys, np.full(m, 40), (5, 20), keep_rule="first")])
    assert np.array_equal(first, counts)
    other = np.array([len(k) for k in datasets.device_keep_host(2, keys, np.full(m, 40), (5, 20))])
    assert (other != counts).mean() > 0.8


def test_keep_arguments():
    ka = datasets.keep_arguments
    assert ka(0) == ka(None) == (0, 0, 0) and ka(6) == (6, 6, 0) and ka((4, 12), keep_rule="random") == (12, 4, 1)
    assert ka(12, 4, 1) == (12, 4, 1) and ka(1024) == (1024, 1024, 0)
    for bad in (dict(keep=-1), dict(keep=1025), dict(keep=(0, 4)), dict(keep=(5, 4)), dict(keep=4, keep_min=5),
                dict(keep=4, keep_rule="last"), dict(keep=4, keep_rule=2), dict(keep=(1, 2), keep_min=1),
                dict(keep=0, keep_min=3), dict(keep=(1, 2, 3))):
        with pytest.raises(ValueError):
            ka(**bad)


def test_unique_table_rows_with_keep():
    q = ops.UNIQUE_ROW_QUANTUM
    assert ops.unique_table_rows(10 ** 6, 100, 128) == 100 * 128                    # as it was
    assert ops.unique_table_rows(10 ** 6, 100, 128, keep=0) == 100 * 128
    assert ops.unique_table_rows(10 ** 6, 100, 128, keep=10) == ops.unique_chunk_rows(1000) == 4 * q
    assert ops.unique_table_rows(10 ** 6, 100, 128, keep=500) == 100 * 128          # min(N, keep)
    assert ops.unique_table_rows(300, 100, 128, keep=10) == ops.unique_chunk_rows(400)     # min(P + n, ...)
    assert ops.unique_table_rows(0, 0, 128, keep=10) == q


BASE_ARGS = {
    "pcaa_frames_from_raw_thin": dict(points=None, f64=0, P=0, offsets=None, n=0, pick=None, key=None, seed=0, N=8, C=4,
                                      st=1, div=0, out=None, n_out=1, pick_out=None, err=None, stream=None),
    "pcaa_crops_from_raw_thin": dict(points=None, f64=0, P=0, offsets=None, n=0, start=None, B=1, T=1, pick=None, key=None,
                                     seed=0, N=8, C=4, st=1, div=0, out=None, err=None, stream=None),
    "pcaa_frames_from_raw_unique_thin": dict(points=None, f64=0, P=0, offsets=None, n=0, pick=None, key=None, seed=0, N=8,
                                             C=4, st=1, div=0, rows=None, weight=None, u_off=None, M=256, pick_out=None,
                                             err=None, stream=None),
}


@pytest.mark.parametrize("name", sorted(BASE_ARGS))
def test_thin_exports_and_their_argument_checks(name):
    protos, lib = _lib.parse_header(), _lib.load()
    plain = name[:-len("_thin")]
    assert name in protos and hasattr(lib, name)
    assert protos[name][1] == protos[plain][1] + [ctypes.c_int] * 3        # the neighbour's arguments, then three ints
    # added under the header's version, as pcaa_crops_from_raw was: the loader refuses a library without them by name
    assert lib.pcaa_abi_version() == _lib.ABI_VERSION >= 29
    fn, base = getattr(lib, name), BASE_ARGS[name]
    word = (ctypes.c_int * 4)()
    ptr = ctypes.cast(word, ctypes.c_void_p)

    def refused(change, keep, said):
        rc = fn(*{**base, **change}.values(), *keep)
        msg = lib.pcaa_last_error().decode()
        assert rc != 0 and name in msg and said in msg, (change, keep, msg)

    # every output pointer is NULL: a call that got past its checks would have to launch on nothing
    refused({}, (0, 0, 0), "keep_min <= keep")                              # keep >= 1: 0 is the plain entry point's
    refused({}, (-3, 1, 0), "keep_min <= keep")
    refused({}, (4, 0, 0), "keep_min <= keep")                              # 1 <= keep_min
    refused({}, (4, 5, 0), "keep_min <= keep")                              # keep_min <= keep
    refused({}, (1025, 1, 0), "keep_min <= keep")                           # keep <= PCAA_RAW_MAX_CARD
    refused({}, (4, 4, 2), "keep_rule")
    refused({}, (4, 4, -1), "keep_rule")
    refused({"pick": ptr}, (4, 4, 0), "pick must be NULL")                  # supplied picks decide by themselves
    refused({"n": 2, "offsets": ptr, "pick": None, "key": None}, (4, 2, 1), "frame_key")
    refused({}, (4, 2, 1), "null")                                          # good keep: the neighbour's checks answer
    # the neighbours are as they were: no keep arguments, the same refusal
    assert getattr(lib, plain)(*base.values()) != 0 and plain in lib.pcaa_last_error().decode()


@pytest.fixture(scope="module")
def store():
    tracks = [syn.synthetic_raw_track(40 + i, 40, max_points=12) for i in range(4)]
    st = datasets.RawTrackStore(tracks, [0, 0, 1, 1], ["free_walk"] * 4, [str(i) for i in range(4)])
    return st.assign(["train", "train", "train", "train"])


def test_batcher_refusals_and_options(store):
    view = store.crops(SPLIT.TRAIN, 8, 4, scenarios=["free_walk"])
    assert len(view) > 0
    b = batcher.RawTrackBatcher(view, 2, keep_points=(4, 12), keep_rule="random", redraw="epoch")
    assert b.keep_points == (4, 12) and b.keep_rule == "random" and b.seed_of(0) != b.seed_of(1)
    assert batcher.RawTrackBatcher(view, 2).keep_points == 0
    picks = np.zeros((store.n_frames, 8), np.int32)
    for bad in (dict(keep_points=4, picks=picks), dict(keep_points=(5, 4)), dict(keep_points=2000),
                dict(keep_points=4, keep_rule="nearest")):
        with pytest.raises(ValueError):
            batcher.RawTrackBatcher(view, 2, **bad)
    assert batcher.RawTrackBatcher(view, 2, picks=picks, keep_points=0).picks is not None


def test_ops_refuse_keep_with_picks_and_bad_ranges():
    points, offsets = datasets.pack_raw_frames(syn.synthetic_raw_track(3, 2))
    pick = torch.zeros((2, 8), dtype=torch.int32)
    key = torch.zeros((2, 2), dtype=torch.int32)
    start = torch.zeros(1, dtype=torch.int32)
    for call in (lambda **kw: ops.frames_from_raw(points, offsets, 8, 4, **kw),
                 lambda **kw: ops.frames_from_raw_unique(points, offsets, 8, 4, **kw),
                 lambda **kw: ops.crops_from_raw(points, offsets, start, 2, 8, 4, **kw)):
        with pytest.raises(ValueError, match="supplied picks"):
            call(pick=pick, keep=4)
        for bad in (dict(keep=1025), dict(keep=(0, 3)), dict(keep=4, keep_min=5), dict(keep=4, keep_rule="x")):
            with pytest.raises(ValueError):
                call(frame_key=key, **bad)


def test_inference_refusals(store):
    with pytest.raises(ValueError, match="raw_store"):
        inference.CGAAE_inference(["none"], ks=[2], keep_points=6)
    for bad in (dict(keep_points=6, scenarios_list=[list(inference.constants.TRAIN_SCENARIOS)[0]] * 2),
                dict(keep_points=(4, 12)), dict(keep_points=6, force_pc_subsampling=6), dict(keep_points=6, keep_rule="x"),
                dict(keep_points=2000), dict(force_pc_subsampling=10)):
        with pytest.raises(ValueError):
            inference.CGAAE_inference(["none"], ks=[2], raw_store=store, **bad)
    with pytest.raises(RuntimeError, match="to_device"):
        inference.point_sweep(None, None, store, [6], [2], 8)
