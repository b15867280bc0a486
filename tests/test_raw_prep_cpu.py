"""``datasets.RawPrep`` (no GPU): it holds what ``keep_arguments`` and ``augment_arguments`` return, its suffix and tail are the
ones the header declares for every raw entry point, its cross-rules refuse what they should, the ``prep=`` keyword of the three
ops functions excludes the keywords it is built from, and the batcher and the scorers build one and hold it.
(``MultiStreamScorer`` cannot be constructed without a device: here its constructor is shown to reach the preparation
before the device, tests/test_raw_prep_routes.py looks at the object it holds.)"""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from helpers import load_golden, make_encoder
from opensetgaitrecognition_pcaa_amd import _lib, batcher, datasets, inference, ops, synthetic as syn
from opensetgaitrecognition_pcaa_amd.constants import SPLIT
from opensetgaitrecognition_pcaa_amd.datasets import RawPrep

FULL = {"yaw": 0.6, "mirror": True, "scale": (0.9, 1.1), "speed": (0.8, 1.25), "noise": [0.02, 0.02, 0.03, 0.1, 1.0]}
# the grid of test_keep_arguments, the forms of test_raw_augment_host_cpu.py: dict, 11-tuple, neutral, None
KEEPS = [dict(keep=0), dict(keep=None), dict(keep=6), dict(keep=(4, 12), keep_rule="random"),
         dict(keep=12, keep_min=4, keep_rule=1), dict(keep=1024)]
BAD_KEEPS = [dict(keep=-1), dict(keep=1025), dict(keep=(0, 4)), dict(keep=(5, 4)), dict(keep=4, keep_min=5),
             dict(keep=4, keep_rule="last"), dict(keep=4, keep_rule=2), dict(keep=(1, 2), keep_min=1),
             dict(keep=0, keep_min=3), dict(keep=(1, 2, 3))]
AUGMENTS = [FULL, datasets.augment_arguments(FULL), {"noise": {"doppler": 0.3}}, {"scale": 1}, {}, None]


@pytest.mark.parametrize("aug", AUGMENTS, ids=str)
@pytest.mark.parametrize("keep", KEEPS, ids=str)
def test_of_holds_what_the_normalisers_return(keep, aug):
    prep = RawPrep.of(**keep, augment=aug, who="test")
    thin, vals = datasets.keep_arguments(**keep), datasets.augment_arguments(aug)
    assert (prep.keep, prep.keep_min, prep.rule) == thin and prep.augment == vals
    assert all(type(v) is int for v in thin)
    # suffix and tail: neutral, keep alone, augment with or without keep
    if vals is not None:
        assert prep.suffix == "_aug" and prep.tail[:3] == thin and len(prep.tail) == 4
        assert isinstance(prep.tail[3], ctypes.c_double * datasets.AUG_PARAMS) and tuple(prep.tail[3]) == vals
    elif thin[0]:
        assert prep.suffix == "_thin" and prep.tail == thin
    else:
        assert prep.suffix == "" and prep.tail == () and prep == RawPrep()
    with pytest.raises(dataclasses.FrozenInstanceError):
        prep.keep = 3


def test_of_raises_the_normalisers_errors_under_who():
    for bad in BAD_KEEPS:
        with pytest.raises(ValueError, match="somebody"):
            RawPrep.of(**bad, who="somebody")
    for bad in ({"yaw": 4.0}, {"spin": 1.0}, [1.0, 2.0], "yaw"):
        with pytest.raises(ValueError, match="somebody"):
            RawPrep.of(augment=bad, who="somebody")


@pytest.mark.parametrize("base", ["frames_from_raw", "crops_from_raw", "frames_from_raw_unique"])
def test_suffix_and_tail_against_the_header(base):
    protos = _lib.parse_header()
    ctype = {int: ctypes.c_int, ctypes.c_double * datasets.AUG_PARAMS: ctypes.c_void_p}       # const double* in the header
    seen = set()
    for prep in (RawPrep.of(), RawPrep.of(6), RawPrep.of((4, 12), keep_rule="random"), RawPrep.of(augment=FULL),
                 RawPrep.of(6, augment=FULL)):
        seen.add(prep.suffix)
        assert protos["pcaa_" + base + prep.suffix][1] == protos["pcaa_" + base][1] + [ctype[type(v)] for v in prep.tail]
    assert seen == {"", "_thin", "_aug"}


def test_cross_rules():
    pick = np.zeros((2, 8), np.int32)
    thin, aug, both, none = RawPrep.of(4), RawPrep.of(augment=FULL), RawPrep.of(4, augment=FULL), RawPrep.of()
    for prep in (thin, both):
        with pytest.raises(ValueError, match="supplied picks"):
            prep.check("who", pick, 4)
        prep.check("who", None, 4)
    for prep in (aug, both):
        with pytest.raises(ValueError, match="C >= 2"):
            prep.check("who", None, 1)
    aug.check("who", pick, 2)
    RawPrep.of(augment={"mirror": True, "noise": [0.1]}).check("who", pick, 1)      # no yaw: one column will do
    none.check("who", pick, 1)
    # keys: when the device draws the picks, or when there is augmentation
    assert [p.needs_keys(None) for p in (none, thin, aug, both)] == [True] * 4
    assert [p.needs_keys(pick) for p in (none, aug)] == [False, True]


def _calls():
    points, offsets = datasets.pack_raw_frames(syn.synthetic_raw_track(3, 2))
    start = torch.zeros(1, dtype=torch.int32)
    return (lambda **kw: ops.frames_from_raw(points, offsets, 8, 4, **kw),
            lambda **kw: ops.frames_from_raw_unique(points, offsets, 8, 4, **kw),
            lambda **kw: ops.crops_from_raw(points, offsets, start, 2, 8, 4, **kw))


def test_prep_keyword_excludes_the_keywords_it_is_built_from():
    key = torch.zeros((2, 2), dtype=torch.int32)
    prep = RawPrep.of((4, 12), keep_rule="random", augment=FULL)
    for call in _calls():
        for kw in (dict(keep=4), dict(keep=(4, 12)), dict(keep_min=2), dict(keep_rule="random"), dict(augment=FULL),
                   dict(augment={})):
            with pytest.raises(ValueError, match="prep="):
                call(frame_key=key, prep=prep, **kw)
        for good in (prep, RawPrep.of(), None):
            with pytest.raises(RuntimeError, match="HIP device"):       # past the argument checks, at the CPU tensors
                call(frame_key=key, prep=good)
        with pytest.raises(ValueError, match="supplied picks"):         # the cross-rules hold for a built one too
            call(pick=torch.zeros((2, 8), dtype=torch.int32), prep=prep)


@pytest.fixture(scope="module")
def view():
    tracks = [syn.synthetic_raw_track(40 + i, 40, max_points=12) for i in range(4)]
    st = datasets.RawTrackStore(tracks, [0, 0, 1, 1], ["free_walk"] * 4, [str(i) for i in range(4)])
    return st.assign(["train"] * 4).crops(SPLIT.TRAIN, 8, 4, scenarios=["free_walk"])


def test_the_batcher_holds_one_prep(view):
    b = batcher.RawTrackBatcher(view, 2, keep_points=(4, 12), keep_rule="random", augment=FULL)
    assert b.prep == dataclasses.replace(RawPrep.of((4, 12), keep_rule="random", augment=FULL), tail=b.prep.tail)
    assert tuple(b.prep.tail[3]) == b.augment == datasets.augment_arguments(FULL)
    assert b.keep_points == (4, 12) and b.keep_rule == "random"
    assert batcher.RawTrackBatcher(view, 2).prep == RawPrep()
    picks = np.zeros((view.store.n_frames, 8), np.int32)
    for bad in (dict(keep_points=4, picks=picks), dict(keep_points=(5, 4)), dict(keep_points=2000),
                dict(keep_points=4, keep_rule="nearest")):                 # the list of test_batcher_refusals_and_options
        with pytest.raises(ValueError):
            batcher.RawTrackBatcher(view, 2, **bad)
    with pytest.raises(ValueError, match="supplied picks"):
        batcher.RawTrackBatcher(view, 2, keep_points=4, picks=picks)
    with pytest.raises(ValueError, match="C >= 2"):
        batcher.RawTrackBatcher(view.store.crops(SPLIT.TRAIN, 8, 1, scenarios=["free_walk"]), 2, augment={"yaw": 0.3})
    assert batcher.RawTrackBatcher(view, 2, picks=picks, augment=FULL).prep.suffix == "_aug"


def test_the_scorers_build_their_prep_in_the_constructor():
    K = 4
    enc = make_encoder(K, 8, 4, True, seed=0).eval()
    means = torch.from_numpy(load_golden("misc")[0]["means_K4"]).float()
    st = inference.StreamingScorer(enc, means, 1e-30, 2, K, max_push=8, keep_points=(4, 12), keep_rule="random")
    assert st.prep == RawPrep.of((4, 12), keep_rule="random") and st.keep_points == (4, 12) and st.keep_rule == "random"
    assert inference.StreamingScorer(enc, means, 1e-30, 2, K, max_push=8).prep == RawPrep()
    for scorer in (inference.StreamingScorer, inference.MultiStreamScorer):
        with pytest.raises(ValueError, match=scorer.__name__):
            scorer(enc, means, 1e-30, 2, K, max_push=8, keep_points=(5, 4))
    with pytest.raises(RuntimeError, match="HIP device"):                  # a good keep: the next refusal is the device's
        inference.MultiStreamScorer(enc, means, 1e-30, 2, K, max_push=8, keep_points=(4, 12), keep_rule="random")
