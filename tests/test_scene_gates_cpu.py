"""The scene front end on the CPU: the case list of tests/scene_ref.py meets its own input conditions, every planted
defect is caught by at least one case, ``scene.cluster_host`` equals the independent reference on all of them, and
``scene.associate`` does what its docstring says on hand-written tables.  No GPU, no tolerance."""
import numpy as np
import pytest

import scene_ref as R
from opensetgaitrecognition_pcaa_amd import _lib, scene, synthetic as syn

_REFS = {}


def _ref(run):
    case, dt = run
    key = (case.name, dt)
    if key not in _REFS:
        _REFS[key] = R.cluster_ref(case.points(dt), case.offsets, *case.args())
    return _REFS[key]


@pytest.mark.parametrize("run", R.RUNS, ids=R.run_id)
def test_case_conditions_and_host_restatement(run):
    case, dt = run
    R.check_conditions(case, dt)
    ref = _ref(run)
    got = scene.cluster_host(case.points(dt), case.offsets, *case.args())
    for k in R.OUTPUTS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        assert np.array_equal(got[k].view(np.uint8), ref[k].view(np.uint8)), (R.run_id(run), k)
    assert got["err"] == ref["err"]


def test_the_cases_cover_what_they_claim():
    by = {c.name: c for c in R.CASES}
    cards = sorted(int(d) for c in R.CASES for d in np.diff(c.offsets) if d >= 0)
    assert {0, 1, 2, 63, 64, 65, 257, 1024, 1025} <= set(cards)
    assert len(by["mixed7"].offsets) == 8 and len(by["chain1024"].offsets) == 2
    chain = _ref((by["chain1024"], "float64"))
    assert chain["n_clusters"].tolist() == [1] and (chain["label"] == 0).all(), "one component through 1023 links"
    lab, c, d2, core = R.frame_ref(by["chain1024"].points("float64"), *by["chain1024"].args())
    assert (~core).sum() == 2 and ((d2 <= 0.25).sum(axis=1)[core] == 3).all()
    for name in ("bridge", "border_tie"):
        ref = _ref((by[name], "float64"))
        lab, c, d2, core = R.frame_ref(by[name].points("float64"), *by[name].args())
        x = 9                                                           # the point between the two 3 x 3 clusters
        assert c == 2 and not core[x] and core[:9].all() and core[10:].all()
        assert (d2[x, :9] <= 0.25).any() and (d2[x, 10:] <= 0.25).any(), "it sees cores of both"
        assert ref["label"][x] == (1 if name == "bridge" else 0)
        assert ref["cluster_count"][0, :2].tolist() == ([9, 10] if name == "bridge" else [10, 9])
    assert _ref((by["all_noise"], "float32"))["n_clusters"].tolist() == [0]
    assert _ref((by["too_many"], "float32"))["err"] == 2 and _ref((by["too_many"], "float32"))["n_clusters"][0] == 4
    assert _ref((by["card1025"], "float32"))["err"] == 1 and _ref((by["bad_offsets"], "float64"))["err"] == 1
    assert _ref((by["backwards"], "float64"))["n_clusters"].tolist() == [1, 0, 0]
    assert _ref((by["min_points_1"], "float64"))["label"].min() == 0, "min_points = 1: no noise"
    nz = _ref((by["neg_zero"], "float32"))["centroid"][0, 0]
    assert nz[0] == 0 and np.signbit(nz[0]) and np.signbit(nz[3]) and not np.signbit(nz[1]), "-0.0 where every member is -0.0"
    dup = by["duplicates"].points("float64")
    assert len(np.unique(dup[:, :2], axis=0)) < len(dup)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_planted_defect_is_caught(defect):
    caught = [R.run_id(run) for run in R.RUNS
              if not R.same(_ref(run), R.cluster_ref(run[0].points(run[1]), run[0].offsets, *run[0].args(), defect=defect))]
    print(f"[scene] {defect}: caught by {caught}")
    assert caught, defect


def test_gather_ref_and_header():
    src = np.arange(50.0).reshape(10, 5)
    out, err = R.gather_ref(src, [2, 9, 0], [0, 3, 5, 5], 5)
    assert err == 1 and np.array_equal(out[:3], src[2:5]) and not out[3:].any()
    protos = _lib.parse_header()
    assert len(protos["pcaa_scene_cluster"][1]) == 18 and len(protos["pcaa_gather_segments"][1]) == 10
    assert _lib.ABI_VERSION == 29, "the entry points were added without a new version number"


# ------------------------------------------------------------------------------------------------------ associate
def _tables(frames, Cmax=4):
    """[[(x, y, count), ...] per frame] -> counts [n, Cmax], centroids [n, Cmax, 4]"""
    n = len(frames)
    counts, cen = np.zeros((n, Cmax), np.int32), np.zeros((n, Cmax, 4), np.float32)
    for f, clusters in enumerate(frames):
        for c, (x, y, k) in enumerate(clusters):
            counts[f, c], cen[f, c, :2] = k, (x, y)
    return counts, cen


P = scene.AssocParams(gate=1.0, confirm=2, max_missed=1, birth_points=5, alpha=0.5, beta=0.25)


def test_associate_birth_confirm_and_dropped_frames():
    st, plan = scene.associate(scene.AssocState(), *_tables([[(0, 0, 6)], [(0.2, 0, 6)], [(0.4, 0, 6)]]), P)
    assert plan.births == [(0, 0)] and plan.confirmed == [(0, 1)] and plan.deaths == []
    assert plan.segments == {0: [(1, 0), (2, 0)]}, "the frame before the confirmation is dropped"
    assert [t.id for t in st.tracks] == [0] and st.next_id == 1 and st.tracks[0].confirmed
    # alpha-beta by hand: frame 1: pred (0, 0), r = 0.2 -> p = 0.1, v = 0.05; frame 2: pred 0.15, r = 0.25 -> p = 0.275, v = 0.1125
    assert np.allclose(st.tracks[0].p, [0.275, 0.0], atol=1e-6) and np.allclose(st.tracks[0].v, [0.1125, 0.0], atol=1e-6)
    assert np.allclose(plan.positions[0], (0.275, 0.0), atol=1e-6)
    # a cluster below birth_points starts nothing; confirm = 1 emits the birth frame itself
    st2, plan2 = scene.associate(scene.AssocState(), *_tables([[(0, 0, 4)], [(0, 0, 5)]]), P._replace(confirm=1))
    assert plan2.births == [(0, 1)] and plan2.confirmed == [(0, 1)] and plan2.segments == {0: [(1, 0)]}
    # the state passed in is not modified, and a second tick continues it
    st3, plan3 = scene.associate(st, *_tables([[(0.5, 0, 6)]]), P)
    assert st.tracks[0].hits == 3 and st3.tracks[0].hits == 4 and np.allclose(st.tracks[0].p, [0.275, 0.0], atol=1e-6)
    assert plan3.segments == {0: [(0, 0)]} and plan3.births == [] and plan3.confirmed == []


def test_associate_gate_and_greedy_order():
    two = P._replace(confirm=1)
    st, _ = scene.associate(scene.AssocState(), *_tables([[(0, 0, 6), (3, 0, 6)]]), two)
    # outside the gate: the track coasts and the cluster starts a new track
    st_g, plan_g = scene.associate(st, *_tables([[(1.01, 0, 6), (3, 0, 6)]]), two)
    assert plan_g.segments == {0: [], 1: [(0, 1)], 2: [(0, 0)]} and plan_g.births == [(2, 0)]
    # exactly on the gate: inside
    _, plan_e = scene.associate(st, *_tables([[(1.0, 0, 6), (3, 0, 6)]]), two)
    assert plan_e.segments == {0: [(0, 0)], 1: [(0, 1)]} and plan_e.births == []
    # greedy by distance: cluster 0 at 1.4 is 0.6 from track 1... the closest pair goes first, the loser takes what is left
    wide = two._replace(gate=2.0)
    _, plan = scene.associate(st, *_tables([[(1.6, 0, 6), (0.9, 0, 6)]]), wide)
    # pairs: (t0, c1) 0.9, (t1, c0) 1.4, (t0, c0) 1.6 -- (t1, c1) 2.1 is outside the gate
    assert plan.segments == {0: [(0, 1)], 1: [(0, 0)]}
    # equal distances: the lower track id, then the lower cluster id
    _, plan_t = scene.associate(st, *_tables([[(1.5, 0, 6)]]), wide)
    assert plan_t.segments == {0: [(0, 0)], 1: []}
    st_one, _ = scene.associate(scene.AssocState(), *_tables([[(0, 0, 6)]]), two)
    _, plan_c = scene.associate(st_one, *_tables([[(0.5, 0, 6), (-0.5, 0, 6)]]), wide)
    assert plan_c.segments == {0: [(0, 0)], 1: [(0, 1)]}, "the lower cluster id wins the tie; the other one is born"


def test_associate_coast_and_death():
    one = P._replace(confirm=1, max_missed=2)
    st, _ = scene.associate(scene.AssocState(), *_tables([[(0, 0, 6)], [(0.3, 0, 6)]]), one)
    v = st.tracks[0].v.copy()
    assert v[0] > 0
    # two misses: coasting along its velocity, still alive; it is found again where it coasted to
    st2, plan2 = scene.associate(st, *_tables([[], []]), one)
    assert plan2.deaths == [] and st2.tracks[0].missed == 2 and np.allclose(st2.tracks[0].p, st.tracks[0].p + 2 * v)
    st3, plan3 = scene.associate(st2, *_tables([[(float(st2.tracks[0].p[0] + v[0]), 0, 6)]]), one)
    assert plan3.segments == {0: [(0, 0)]} and st3.tracks[0].missed == 0
    # a third miss in a row: more than max_missed, dead in that frame; the plan still lists what it received before
    st4, plan4 = scene.associate(st, *_tables([[(0.45, 0, 6)], [], [], [], [(0.45, 0, 6)]]), one)
    assert plan4.deaths == [(0, 3)] and plan4.segments == {0: [(0, 0)], 1: [(4, 0)]} and plan4.births == [(1, 4)]
    assert [t.id for t in st4.tracks] == [1] and list(plan4.positions) == [1]
    # a tentative track loses its consecutive hits on a miss
    two = P._replace(confirm=2, max_missed=2)
    _, plan5 = scene.associate(scene.AssocState(), *_tables([[(0, 0, 6)], [], [(0, 0, 6)], [(0, 0, 6)]]), two)
    assert plan5.births == [(0, 0)] and plan5.confirmed == [(0, 3)] and plan5.segments == {0: [(3, 0)]}


def test_refuse_takes_a_confirmed_track_out_again():
    """what the splitter does with a track it has no stream for: gone from state and plan, reborn from the next frame"""
    one = P._replace(confirm=1)
    tables = _tables([[(0, 0, 6), (3, 0, 6), (6, 0, 6)], [(0, 0, 6), (3, 0, 6), (6, 0, 6)]])
    st, plan = scene.associate(scene.AssocState(), *tables, one)
    assert [t for t, _ in plan.confirmed] == [0, 1, 2] and plan.refused == []
    st, plan = scene.refuse(st, plan, [2])
    assert [t.id for t in st.tracks] == [0, 1] and st.next_id == 3 and plan.refused == [2]
    assert plan.segments == {0: [(0, 0), (1, 0)], 1: [(0, 1), (1, 1)]} and sorted(plan.positions) == [0, 1]
    assert plan.births == [(0, 0), (1, 0)] and plan.confirmed == [(0, 0), (1, 0)]
    st2, plan2 = scene.associate(st, *_tables([[(0, 0, 6), (3, 0, 6), (6, 0, 6)]]), one)
    assert plan2.births == [(3, 0)] and plan2.segments == {0: [(0, 0)], 1: [(0, 1)], 3: [(0, 2)]}, "born anew under a new id"
    # a refused track that also died in the tick leaves the deaths too
    st3, plan3 = scene.associate(scene.AssocState(), *_tables([[(0, 0, 6)], [], []]), one._replace(max_missed=1))
    assert plan3.deaths == [(0, 2)] and plan3.segments == {0: [(0, 0)]}
    st3, plan3 = scene.refuse(st3, plan3, [0])
    assert plan3.deaths == [] and plan3.segments == {} and plan3.confirmed == [] and plan3.refused == [0]


def test_associate_two_tracks_crossing():
    """two people walk towards each other on lines 0.5 m apart and pass; the velocity prediction keeps each track on its
    own person although the clusters swap their order in the frame"""
    one = P._replace(confirm=1, gate=0.7)
    frames = []
    for f in range(12):
        a, b = (-1.1 + 0.2 * f, 0.0, 8), (1.1 - 0.2 * f, 0.5, 8)
        frames.append([a, b] if f % 2 == 0 else [b, a])                 # the cluster ids alternate
    st, plan = scene.associate(scene.AssocState(), *_tables(frames), one)
    assert plan.births == [(0, 0), (1, 0)] and plan.deaths == []
    assert plan.segments[0] == [(f, f % 2) for f in range(12)] and plan.segments[1] == [(f, 1 - f % 2) for f in range(12)]
    assert st.tracks[0].p[0] > 0.8 and st.tracks[1].p[0] < -0.8 and st.tracks[0].v[0] > 0.15 and st.tracks[1].v[0] < -0.15


def test_synthetic_scene_is_what_it_says():
    eps = 0.5
    scn, persons = syn.synthetic_scene(7, 12, [(0, 12), (3, 9)], 3, eps)
    assert len(scn) == 12 and [p is not None for p in persons[1]] == [3 <= f < 9 for f in range(12)]
    e2, wz2, wv2 = scene.metric(eps, 0.1, 0.0)
    for f, fr in enumerate(scn):
        rows = np.column_stack([fr["elements"], fr["z_coord"], fr["dopplers"], fr["powers"]]).astype(np.float32)
        lab, c = scene.cluster_frame_host(rows, e2, wz2, wv2, 3, 16)
        live = [k for k in range(2) if persons[k][f] is not None]
        assert c == len(live) and (lab < 0).sum() == 3, "one cluster per person, the clutter is noise"
        for k in live:
            mine = np.column_stack([persons[k][f]["elements"], persons[k][f]["z_coord"]]).astype(np.float32)
            ids = {int(l) for l, r in zip(lab, rows) if any((r[:3] == m).all() for m in mine)}
            assert len(ids) == 1 and -1 not in ids
            d2 = scene.pair_d2(np.column_stack([mine, np.zeros(len(mine))]), wz2, 0.0)
            assert d2.max() <= e2, "inside a ball of radius eps / 2"
