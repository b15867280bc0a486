"""A prebuilt ``datasets.RawPrep`` passed as ``prep=`` gives every raw entry point the bits its keywords give it: the store of
tests/test_raw_keep_host_cpu.py (4 synthetic tracks of 40 frames, 1 - 12 detections), N = 8 (cards on both sides of it),
C = 4, crops of T = 2; no preparation, ``keep=(4, 12)`` "random", the "all" augment of tools/raw_augment_bench.py, and both."""
import pytest
import torch

from helpers import load_golden, make_encoder
from opensetgaitrecognition_pcaa_amd import datasets, synthetic as syn
from opensetgaitrecognition_pcaa_amd.datasets import RawPrep

N, C, T, SEED = 8, 4, 2, 5
KEEP = dict(keep=(4, 12), keep_rule="random")
ALL = {"yaw": 0.5, "mirror": True, "scale": (0.9, 1.1), "speed": (0.8, 1.25), "noise": [0.02, 0.02, 0.03, 0.1, 1.0]}
CONFIGS = {"none": {}, "keep": KEEP, "all": dict(augment=ALL), "both": dict(augment=ALL, **KEEP)}


def _state(prep):
    return (prep.keep, prep.keep_min, prep.rule, prep.augment, prep.suffix, prep.tail[:3], [tuple(a) for a in prep.tail[3:]])


@pytest.mark.gpu
def test_prep_and_keywords_give_the_same_bits():
    from opensetgaitrecognition_pcaa_amd import inference, ops
    store = datasets.RawTrackStore([syn.synthetic_raw_track(40 + i, 40, max_points=12) for i in range(4)], [0, 0, 1, 1],
                                   ["free_walk"] * 4, [str(i) for i in range(4)]).to_device("cuda")
    cards = store.cards()
    assert cards.min() < N < cards.max()
    points, offsets, keys = store.points_dev, store.offsets_dev, store.frame_key_dev
    F = store.n_frames
    start = torch.arange(0, F - T, 7, dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    outs = {}
    for name, kw in CONFIGS.items():
        prep = RawPrep.of(**kw, who="test")
        before = _state(prep)
        for how in (kw, dict(prep=prep), dict(prep=prep)):                 # the keywords; the one object, reused
            pick_out = torch.full((F, N), -1, dtype=torch.int32, device="cuda")
            upick = torch.full((F, N), -1, dtype=torch.int32, device="cuda")
            got = (ops.frames_from_raw(points, offsets, N, C, seed=SEED, frame_key=keys, pick_out=pick_out, err_flag=err, **how),
                   pick_out,
                   ops.crops_from_raw(points, offsets, start, T, N, C, seed=SEED, frame_key=keys, err_flag=err, **how),
                   *ops.frames_from_raw_unique(points, offsets, N, C, seed=SEED, frame_key=keys, pick_out=upick, err_flag=err,
                                               **how),
                   upick)
            want = outs.setdefault(name, got)
            assert len(got) == 7 and all(torch.equal(g, w) for g, w in zip(got, want)), name
        assert _state(prep) == before, name
        assert int(got[1].min()) >= 0 and int(got[6].min()) >= 0, "the picks used were written"
    assert err.item() == 0
    frames = [outs[name][0] for name in CONFIGS]                           # four different preparations
    assert all(not torch.equal(frames[i], frames[j]) for i in range(4) for j in range(i))
    # the live scorers hold the object their constructor built (MultiStreamScorer needs the device for it)
    enc = make_encoder(4, N, C, True, seed=0).cuda().eval()
    means = torch.from_numpy(load_golden("misc")[0]["means_K4"]).float()
    ms = inference.MultiStreamScorer(enc, means, 1e-30, 2, 4, max_streams=2, max_push=8, keep_points=(4, 12),
                                     keep_rule="random")
    assert ms.prep == RawPrep.of(**KEEP) and ms.keep_points == (4, 12) and ms.keep_rule == "random"
