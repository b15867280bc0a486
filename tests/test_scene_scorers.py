"""``scene.SceneSplitter`` over a ``MultiStreamScorer`` on the device: scene frames in, the SAME ticks out as a second scorer
that is fed the people's own frames through ``push_raw`` -- same seed, streams opened in the same order -- so every
comparison is ``torch.equal``.  ``synthetic.synthetic_scene``: people on lanes, clutter, a random detection order per
frame; N = 32, C = 4, K = 4, the small synthetic encoder of the other scorer tests, ticks of 6 frames."""
import numpy as np
import pytest
import torch

from helpers import T, load_golden, make_encoder
from opensetgaitrecognition_pcaa_amd import constants, datasets, scene, synthetic as syn

pytestmark = pytest.mark.gpu

K, N, C, HOP = 4, 32, 4, constants.CROP_STEP
EPS, TICK, THRESHOLD = 0.5, 6, 1e-30
LANE = 3.5 * EPS                                    # synthetic_scene puts person k on the line y = k * LANE


def _setup():
    enc = make_encoder(K, N, C, True, seed=0).cuda().eval()
    means = torch.from_numpy(load_golden("misc")[0]["means_K4"]).float()
    return enc, means


def _dev(raw):
    points, offsets = datasets.pack_raw_frames(raw, torch.float32)
    return points.cuda(), offsets.cuda()


def _pair(enc, means, max_streams=3, **kw):
    from opensetgaitrecognition_pcaa_amd import inference
    mk = lambda: inference.MultiStreamScorer(enc, means, THRESHOLD, 2, K, max_streams=max_streams, max_push=8, seed=9)
    ms, mf = mk(), mk()
    return scene.SceneSplitter(ms, eps=EPS, min_points=3, **kw), ms, mf


def _run(sp, mf, scn, persons, n_frames, upload_stream=None):
    """push the scene tick by tick; mirror every tick on ``mf`` with the people's own frames -> the SceneTicks, and which
    person every track was (by the lane its position lies on).  ``upload_stream``: the scene frames go up on that stream
    and ``push`` gets the event recorded behind them (``ready``)"""
    person_of, ticks, windows = {}, [], 0
    for a in range(0, n_frames, TICK):
        if upload_stream is None:
            st = sp.push(*_dev(scn[a:a + TICK]))
        else:
            with torch.cuda.stream(upload_stream):
                p, o = _dev(scn[a:a + TICK])
                ready = torch.cuda.Event()
                ready.record(upload_stream)
            st = sp.push(p, o, ready=ready)
        for tid, (x, y) in st.positions.items():
            person_of.setdefault(tid, int(round(y / LANE)))
        early = [sid for tid, sid in st.closed if tid not in st.tids]
        for sid in early:
            mf.close(sid)
        for tid, sid in st.opened:
            assert mf.open() == sid, "the second scorer opens its streams in the same order"
        own = [[fr for fr in persons[person_of[tid]][a:a + TICK] if fr is not None] for tid in st.tids]
        assert [len(f) for f in own] == st.counts, (a, st.counts)
        if st.sids:
            want = mf.push_raw(st.sids, st.counts, *_dev([fr for f in own for fr in f]))
            assert np.array_equal(st.tick.stream, want.stream) and np.array_equal(st.tick.window, want.window)
            assert np.array_equal(st.tick.vote_stream, want.vote_stream)
            for name in ("preds", "sup_fv", "lik", "votes"):
                assert torch.equal(getattr(st.tick, name), getattr(want, name)), (name, a)
            windows += len(want)
        else:
            assert len(st.tick) == 0
        for tid, sid in st.closed:
            if tid in st.tids:                       # it still received frames in the tick it died in
                mf.close(sid)
        ticks.append(st)
    assert int(sp.err) == 0 and int(sp.front.gather_err) == 0 and int(sp.ms.raw_err) == 0 and int(mf.raw_err) == 0
    return ticks, person_of, windows


def test_two_people_equal_the_pre_separated_streams():
    enc, means = _setup()
    F = 36
    scn, persons = syn.synthetic_scene(11, F, 2, 3, EPS)
    sp, ms, mf = _pair(enc, means, confirm=1)
    ticks, person_of, windows = _run(sp, mf, scn, persons, F)
    assert sorted(person_of.values()) == [0, 1] and sorted(person_of) == [0, 1], "two tracks, one per person"
    assert ticks[0].opened == [(0, 0), (1, 1)] and all(not t.opened and not t.closed for t in ticks[1:])
    assert all(t.counts == [TICK, TICK] and t.noise == 3 * TICK for t in ticks)
    assert windows == 2 * ((F - T) // HOP + 1) > 0 and ticks[-1].tick.votes.numel() == 2
    # where the tracks are: on their lanes, inside the scene
    for tid, (x, y) in ticks[-1].positions.items():
        assert abs(y - person_of[tid] * LANE) < EPS / 2


def test_a_person_leaves_another_arrives_in_the_middle_of_a_tick():
    enc, means = _setup()
    F = 54
    scn, persons = syn.synthetic_scene(12, F, [(0, F), (0, 14), (20, F)], 2, EPS)
    sp, ms, mf = _pair(enc, means, confirm=1, max_missed=2)
    ticks, person_of, windows = _run(sp, mf, scn, persons, F)
    assert person_of[2] == 2 and sorted(person_of[t] for t in (0, 1)) == [0, 1]
    left = next(t for t in (0, 1) if person_of[t] == 1)
    stays = 1 - left
    # person 1 is seen in frames 12 and 13 of tick 2, missed in 14, 15 and 16: more than max_missed, closed in that tick
    assert ticks[2].closed == [(left, left)] and sorted(ticks[2].counts) == [2, TICK]
    assert all(not t.closed for i, t in enumerate(ticks) if i != 2)
    # person 2 arrives in frame 20, the third frame of tick 3, and takes the slot that was freed
    assert ticks[3].opened == [(2, left)] and ticks[3].tids == [stays, 2] and ticks[3].sids == [stays, left]
    assert dict(zip(ticks[3].sids, ticks[3].counts)) == {stays: TICK, left: 4}, "the counts differ per stream"
    assert ticks[-1].stream_of_track == {stays: stays, 2: left} and ticks[-1].track_of_stream == {stays: stays, left: 2}
    assert windows == ((F - T) // HOP + 1) + ((F - 20 - T) // HOP + 1)
    assert mf._open.tolist() == ms._open.tolist()


def test_more_people_than_streams():
    """three people, two slots: the third confirmation is refused tick after tick (reported, nothing raised, the two
    streams keep scoring) until a person leaves; then the one who waited is born into the freed slot.  The scene frames go
    up on a stream of their own and ``push`` is given the event behind them."""
    enc, means = _setup()
    F = 54
    scn, persons = syn.synthetic_scene(15, F, [(0, F), (0, 14), (0, F)], 2, EPS)
    sp, ms, mf = _pair(enc, means, max_streams=2, confirm=1, max_missed=2)
    ticks, person_of, windows = _run(sp, mf, scn, persons, F, upload_stream=torch.cuda.Stream())
    assert [t.refused for t in ticks[:3]] == [[2], [3], [4]] and all(t.refused == [] for t in ticks[3:])
    assert all(sorted(t.tids) == [0, 1] and len(t.sids) == 2 for t in ticks[:3])
    waited = ({0, 1, 2} - {person_of[0], person_of[1]}).pop()
    left = next(t for t in (0, 1) if person_of[t] == 1)
    assert waited != 1, "the person who leaves had a stream"
    # the refused person's detections went to no stream: more noise than the clutter alone
    assert all(t.noise > 2 * TICK for t in ticks[:3]) and all(t.noise == 2 * TICK for t in ticks[4:])
    # tick 2: the leaver was still fed, so the slot frees after the tick and the waiting person is refused once more;
    # tick 3: born into the freed slot, all six frames
    assert ticks[2].closed == [(left, left)] and ticks[3].opened == [(5, left)] and person_of[5] == waited
    assert dict(zip(ticks[3].tids, ticks[3].counts)) == {1 - left: TICK, 5: TICK}
    assert windows == ((F - T) // HOP + 1) + ((F - 18 - T) // HOP + 1)
    assert mf._open.tolist() == ms._open.tolist() == [True, True]


def test_empty_scene_ticks():
    enc, means = _setup()
    scn, _ = syn.synthetic_scene(13, TICK, 0, 4, EPS)
    sp, ms, mf = _pair(enc, means, confirm=1)
    st = sp.push(*_dev(scn))
    assert len(st.tick) == 0 and st.tick.preds.numel() == 0 and st.tick.votes.numel() == 0 and st.tick.sup_fv.shape == (0, 32)
    assert st.sids == [] and st.opened == [] and st.closed == [] and st.noise == 4 * TICK and st.positions == {}
    assert not ms._open.any() and not ms.n_frames.any(), "no stream was opened, no frame reached the scorer"
    p, o = _dev(scn)
    st = sp.push(p[:0], o[:1])                                           # no frame at all
    assert len(st.tick) == 0 and st.noise == 0
    with pytest.raises(ValueError):
        sp.push(*_dev(scn + scn))                                        # 12 frames > max_push = 8
    with pytest.raises(ValueError):
        scene.SceneSplitter(ms, eps=EPS, max_clusters=65)
    assert int(sp.err) == 0


def test_split_recording_then_embed_raw_track():
    from opensetgaitrecognition_pcaa_amd import inference
    enc, means = _setup()
    F = 40
    scn, persons = syn.synthetic_scene(14, F, [(0, F), (4, F)], 3, EPS)
    out = scene.split_recording(*_dev(scn), eps=EPS, min_points=3, confirm=1, chunk=16)
    assert sorted(out) == [0, 1]
    sc = inference.OpenSetScorer(enc, means)
    firsts = set()
    for tid, (points, offsets, first) in out.items():
        k = 0 if first == 0 else 1
        firsts.add(first)
        own_p, own_o = _dev([fr for fr in persons[k] if fr is not None])
        assert torch.equal(points, own_p) and torch.equal(offsets, own_o), "the person's own detections, bit for bit"
        got, want = sc.embed_raw_track(points, offsets, seed=3, track_key=tid), sc.embed_raw_track(own_p, own_o, seed=3, track_key=tid)
        assert got[0].numel() == inference.window_count(F - first) > 0
        for g, w in zip(got, want):
            assert torch.equal(g, w)
    assert firsts == {0, 4} and int(sc.raw_err) == 0
