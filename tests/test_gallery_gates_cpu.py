"""The gates, input conditions and planted defects of tests/gallery_ref.py, the host bookkeeping of ``gallery.Gallery`` and
the ring rows of ``MultiStreamScorer.enrol_stream``, on the CPU (no GPU needed).

    test_inputs_meet_the_conditions     every case of gallery_ref.CASES: distances apart or planted ties, what the rows cover
    test_wide_and_fsum_agree            the two arithmetics of the reference agree within a fraction of the gate
    test_defects_move_what_they_touch   each planted defect moves >= 80 % of what it touches by > 10 gates or changes the integer
    test_vote_*                         the vote reference against oracle.k_vote on trained labels; its defect
    test_centroid_ref_*                 the host expression: continuing sums, order, skipped rows
    test_gallery_bookkeeping, test_gallery_refusals, test_state_dict_round_trip
    test_ring_rows_*                    against a brute-force replay, including the wrap
    test_header_declares_the_entry_points
"""
import ctypes

import numpy as np
import pytest
import torch

import critic_loss_ref as R
import gallery_ref as G
from opensetgaitrecognition_pcaa_amd import _lib, gallery, inference, ops
from opensetgaitrecognition_pcaa_amd.gallery import Gallery

_REFS = {}


def _ref(case):
    if case not in _REFS:
        c = G.gallery_case(*case)
        _REFS[case] = (c, G.gallery_score_ref(c["x"], c["preds"], c["means"], c["centroids"], c["counts"], c["E"], c["n_labels"]))
    return _REFS[case]


@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_inputs_meet_the_conditions(case):
    B, Kc, D, E, empty = case
    c, ref = _ref(case)
    tie = G.check_separation(ref, c["tie_pairs"])
    lik, near = ref["lik"], ref["near"]
    counts = c["counts"].numpy()
    assert (near < Kc + E).all() and all(n < Kc or counts[n - Kc] > 0 for n in near)
    if B >= 8:
        tiny = np.finfo(np.float64).tiny
        assert (lik == 0).any() and ((lik > 0) & (lik < tiny)).any() and (lik > tiny).any()
        thr = G.mid_threshold(lik)
        G.check_threshold(lik, ref["gate"], thr)
    if B > 1:
        assert (near >= Kc).any() and (near < Kc).any()
    if c["mid_row"] is not None:
        assert tie[c["mid_row"]] and near[c["mid_row"]] == Kc - 1, "midway between a prior mean and a centroid: the prior mode wins"
    if len(c["tie_pairs"]) == 2:
        twins = max(c["tie_pairs"])
        assert (near[tie] == twins[0]).sum() >= 2, "rows on the twin centroids: the lower slot wins"
    assert tie.sum() >= len(c["tie_pairs"])
    if empty:
        assert (counts[:E] == 0).sum() == E // 3


@pytest.mark.parametrize("case", [G.CASES[1], G.CASES[3]], ids=G.case_id)
def test_wide_and_fsum_agree(case):
    c, ref = _ref(case)
    other = G.gallery_score_ref(c["x"], c["preds"], c["means"], c["centroids"], c["counts"], c["E"], c["n_labels"],
                                wide=not R.WIDE)
    assert (np.abs(other["lik"] - ref["lik"]) <= 0.5 * ref["gate"]).all()
    assert np.array_equal(other["near"], ref["near"]) and np.array_equal(other["labels"], ref["labels"])


def _wave_order_f64(c):
    """the likelihood in plain double in the kernel's order: sequential |x - m|^2, the prior terms added one by one, lane l
    of 64 adding slots l, l + 64, ... and the 64 partials meeting in an xor butterfly"""
    x, mu = c["x"].numpy().astype(np.float64), c["means"].numpy().astype(np.float64)
    E, D, Kc = c["E"], x.shape[1], mu.shape[0]
    cent, cnt = c["centroids"].numpy().astype(np.float64)[:E], c["counts"].numpy()[:E]

    def terms(m):
        maha = np.cumsum((x[:, None, :] - m[None]) ** 2, axis=-1)[..., -1]
        return np.exp(-0.5 * (D * R.LOG2PI + maha))
    prior = np.cumsum(terms(mu), axis=1)[:, -1]
    lanes = np.zeros((x.shape[0], 64))
    if E:
        t = np.where(cnt[None] > 0, terms(cent), 0.0)
        for e in range(E):
            lanes[:, e % 64] += t[:, e]
    o = 32
    while o:
        lanes = lanes + lanes[:, np.arange(64) ^ o]
        o >>= 1
    return (prior + lanes[:, 0]) / Kc


@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_a_double_evaluation_in_the_kernels_order_sits_inside_the_gate(case):
    c, ref = _ref(case)
    r = float((np.abs(_wave_order_f64(c) - ref["lik"]) / ref["gate"]).max())
    print(f"[gallery] {G.case_id(case)}: fp64 evaluation in wavefront order, worst |err| / gate = {r:.4f}")
    assert r <= 0.5


@pytest.mark.parametrize("k", G.STREAM_KS)
def test_the_stream_scenario_meets_the_conditions(k):
    S = G.stream_scenario(k)                 # (asserts separation, the distance to the threshold, what the labels cover)
    assert S["n"] == 3 * k + 2 + 2 * S["H"] + 1 and S["m"] == S["H"] and S["after"][2] == 2
    assert (S["votes"] > S["n_labels"]).any(), "a group elects an enrolled identity"


def _moved(ref, bad, mask=None):
    """(touched rows, of them moved): a row is touched when the defect changes its double or an integer, moved when its
    likelihood moves by more than 10 gates or an integer changes"""
    ints = (bad["near"] != ref["near"]) | (bad["labels"] != ref["labels"])
    touched = (bad["lik"] != ref["lik"]) | ints
    if mask is not None:
        touched &= mask
    hit = (np.abs(bad["lik"] - ref["lik"]) > 10 * ref["gate"]) | ints
    return int(touched.sum()), int((hit & touched).sum())


@pytest.mark.parametrize("defect", G.GALLERY_DEFECTS)
def test_defects_move_what_they_touch(defect):
    touched = moved = 0
    for case in G.CASES:
        c, ref = _ref(case)
        bad = G.gallery_score_ref(c["x"], c["preds"], c["means"], c["centroids"], c["counts"], c["E"], c["n_labels"],
                                  defect=defect)
        # (fp32 distance: a row that sits on its mode has |x - m|^2 = 0 in either precision, and a denormal result is a
        # few hundred units of 2^-1074, too coarse to show a relative 1e-5; as in test_critic_loss_gates_cpu.py the
        # downgrade is judged where the nearest distance is not 0 and the result is normal)
        mask = (ref["lik"] > 1e-290) & (ref["d2"].min(1) > 0) if defect == "fp32_distance" else None
        t, m = _moved(ref, bad, mask)
        touched, moved = touched + t, moved + m
    print(f"[gallery] {defect}: touches {touched} rows, moves {moved}")
    assert touched >= 4 and moved >= 0.8 * touched, (defect, touched, moved)


def test_vote_equals_the_oracle_on_trained_labels_and_its_defect_shows():
    thr, nl = 0.5, 3
    for k, (lik, preds) in R.kvote_exhaustive().items():
        assert np.array_equal(G.gallery_vote_ref(lik, preds, thr, k, nl), R.kvote_ref(lik, preds, thr, k, nl))
    for k, (lik, labels) in G.vote_exhaustive((0, 1, nl + 1, nl + 2)).items():
        want = G.gallery_vote_ref(lik, labels, thr, k, nl)
        bad = G.gallery_vote_ref(lik, labels, thr, k, nl, defect="vote_below_n_classes", n_classes=nl)
        assert (lik == thr).any() and len(want) == 8 ** k
        # an integer output: a touched group is a changed one; every group that elects an enrolled identity must change
        assert (want > nl).any() and (bad[want > nl] != want[want > nl]).all()
        assert np.array_equal(bad[want < nl], want[want < nl]) or k > 1


def test_centroid_ref_continues_and_skips():
    fv = G.accumulate_inputs(70, 5)
    c_all, s_all, n_all = G.centroid_ref(fv)
    c1, s1, n1 = G.centroid_ref(fv[:33])
    c2, s2, n2 = G.centroid_ref(fv[33:], None, s1, n1)
    assert n2 == n_all == 70 and np.array_equal(s2, s_all) and np.array_equal(c2, c_all) and c_all.dtype == np.float32
    rev = G.centroid_ref(fv, np.arange(69, -1, -1))[1]
    assert (rev != s_all).any(), "the inputs must make the order of the sum visible"
    c3, _, n3 = G.centroid_ref(fv, [3, -1, 70, 4])
    assert n3 == 2 and np.array_equal(c3, np.float32((fv[3].double() + fv[4].double()).numpy() / 2))


# ------------------------------------------------------------------------------------------------ Gallery on the host
@pytest.fixture
def host_gallery(monkeypatch):
    monkeypatch.setattr(ops, "gallery_accumulate", G.accumulate_host)
    return Gallery(4, 3, "cpu")


def test_gallery_bookkeeping(host_gallery):
    g = host_gallery
    fv = G.accumulate_inputs(6, 4)
    assert g.identities() == [] and len(g) == 0 and g.high_water == 0
    assert g.enrol(fv[:2]) == 0 and g.enrol(fv, rows=[5, 4]) == 1 and g.identities() == [0, 1] and g.high_water == 2
    assert np.array_equal(g.centroids[1].numpy(), G.centroid_ref(fv, [5, 4])[0])
    assert g.enrol(fv[2:3], ident=0) == 0 and int(g.counts[0]) == 3, "a live identity is refined"
    assert np.array_equal(g.centroids[0].numpy(), G.centroid_ref(fv[:3])[0])
    assert g.enrol(fv, ident=2, rows=torch.tensor([1], dtype=torch.int32)) == 2 and len(g) == 3
    assert g.label_of(1, 7) == 9 and g.ident_of(9, 7) == 1 and g.ident_of(7, 7) is None and g.ident_of(2, 7) is None
    g.remove(1)
    assert g.identities() == [0, 2] and int(g.counts[1]) == 0 and not g.sums[1].any() and 1 not in g and g.high_water == 3
    assert g.enrol(fv[3:5]) == 1, "the lowest free slot is taken again"
    assert np.array_equal(g.centroids[1].numpy(), G.centroid_ref(fv[3:5])[0]), "and starts from zero"
    g.enrol(fv, ident=0, rows=[0, 99])
    assert int(g.err) == 1 and int(g.counts[0]) == 4


def test_gallery_refusals(host_gallery):
    g = host_gallery
    fv = G.accumulate_inputs(6, 4)
    for bad in (lambda: Gallery(0, 3, "cpu"), lambda: Gallery(4, 0, "cpu"),
                lambda: g.enrol(G.accumulate_inputs(6, 5)),                 # width mismatch
                lambda: g.enrol(fv[:0]), lambda: g.enrol(fv, rows=[]),      # zero rows
                lambda: g.enrol(fv, rows=[[0]]), lambda: g.enrol(fv, rows=[0.5]),
                lambda: g.enrol(fv, ident=3), lambda: g.enrol(fv, ident=-1), lambda: g.enrol(fv, ident=True),
                lambda: g.remove(0), lambda: g.label_of(0, 4), lambda: g.ident_of(5, 4)):   # unknown identity
        with pytest.raises(ValueError):
            bad()
    assert g.identities() == [] and g.high_water == 0, "a refused call leaves no trace"
    for _ in range(3):
        g.enrol(fv)
    with pytest.raises(ValueError, match="in use"):
        g.enrol(fv)
    with pytest.raises(ValueError):
        inference._Rule(torch.zeros(2, 4), None, 2, g, "x")
    with pytest.raises(ValueError):
        inference._Rule(torch.zeros(2, 5), 3, 2, g, "x")
    assert inference._Rule(torch.zeros(2, 4), 3, 2, g, "x").gallery is g
    assert inference._Rule(torch.zeros(2, 4), None, 2, None, "x").gallery is None


def test_state_dict_round_trip(host_gallery):
    g = host_gallery
    fv = G.accumulate_inputs(6, 4)
    g.enrol(fv[:2]), g.enrol(fv[2:]), g.remove(0)
    state = g.state_dict()
    g.enrol(fv)                                        # the snapshot does not follow later changes
    h = Gallery(4, 3, "cpu")
    h.load_state_dict(state)
    assert h.identities() == [1] and h.high_water == 2 and int(h.counts[1]) == 4 and int(h.counts[0]) == 0
    assert torch.equal(h.sums, state["sums"]) and torch.equal(h.centroids, state["centroids"])
    assert h.enrol(fv[:1]) == 0
    with pytest.raises(ValueError):
        Gallery(5, 3, "cpu").load_state_dict(state)
    with pytest.raises(ValueError):
        Gallery(4, 2, "cpu").load_state_dict(state)
    with pytest.raises(ValueError):
        h.load_state_dict(dict(state, high_water=1))


# ------------------------------------------------------------------------------------------------ enrol_stream's rows
@pytest.mark.parametrize("H,ticks", [(3, [2, 1, 4]), (3, [7]), (5, [1, 1, 1]), (4, [4, 4]), (1, [3])])
def test_ring_rows_against_a_replay(H, ticks):
    total = sum(ticks)
    for m in range(1, min(H, total) + 1):
        got = gallery.ring_rows(total, H, m, stream=6)
        assert got.dtype == np.int32 and got.tolist() == G.ring_rows_brute(ticks, H, m, 6)
    for m in (0, min(H, total) + 1):
        with pytest.raises(ValueError):
            gallery.ring_rows(total, H, m, 6)
    if total > H:
        assert gallery.ring_rows(total, H, H, 0).tolist() != sorted(gallery.ring_rows(total, H, H, 0).tolist()) or total % H == 0


def test_plan_enrolment_is_the_draw_of_sequential_votes():
    lab = np.repeat(np.arange(10, 20), [5, 3, 8, 2, 9, 4, 6, 7, 1, 5])
    val, idents, rows, keep = inference.plan_enrolment(lab, 3, seed=0, unseen_valid_ratio=0.2, enrol_ratio=0.5)
    rng = np.random.default_rng(0)
    assert np.array_equal(val, rng.choice(np.unique(lab), size=2, replace=False))
    assert len(idents) <= 4 and not set(idents) & set(val.tolist()) and list(idents.values()) == list(range(len(idents)))
    assert sorted(idents) == list(idents)
    for s, r in rows.items():
        assert np.array_equal(r, np.flatnonzero(lab == s)[:3]) and (lab == s).sum() > 3 and not keep[r].any()
    assert keep.sum() == len(lab) - 3 * len(idents)
    for shots in (0, 100):
        _, idents, rows, keep = inference.plan_enrolment(lab, shots)
        assert not idents and not rows and keep.all()


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("unknown", [False, True])
def test_voted_windows_is_the_loop_of_the_sequential_procedure(k, unknown):
    """``_voted_windows`` against the loop as ``_sequential_votes`` and ``enrolment_sweep`` each carried it before they
    shared it, copied here: 31 crops of 4 subjects (a trailing partial group at k = 2 and 3), groups that straddle two
    subjects, one validation subject, one enrolled subject"""
    lab = np.repeat([12, 10, 13, 11], [9, 7, 8, 7])
    val_subjects, idents, n_labels = np.array([13]), {10: 0}, 5
    n = (len(lab) // k) * k
    all_votes = np.arange(100, 100 + n // k)
    label_of = (lambda s: n_labels + 1 + idents[s] if s in idents else n_labels) if unknown else (lambda s: s)
    seen = []

    def vote(m):
        seen.append(m)
        return torch.from_numpy(all_votes)
    want_preds, want_labels = [], []
    for w in range(n // k):
        seg = lab[w * k:(w + 1) * k]
        if len(np.unique(seg)) != 1:
            continue
        if unknown and seg[0] in val_subjects:
            continue
        want_preds.append(int(all_votes[w]))
        want_labels.append(int(seg[0]) if not unknown else
                           n_labels + 1 + idents[int(seg[0])] if int(seg[0]) in idents else n_labels)
    got_preds, got_labels = inference._voted_windows(k, lab, vote, val_subjects, unknown, label_of)
    assert seen == [n] and got_preds == want_preds and got_labels == want_labels
    assert all(type(x) is int for x in got_preds + got_labels)
    straddling = sum(len(np.unique(lab[w * k:(w + 1) * k])) != 1 for w in range(n // k))
    assert (straddling > 0) == (k > 1), "the case must hold a window that straddles two subjects"
    assert (13 in [int(lab[w * k]) for w in range(n // k)]) and (unknown or 13 in got_labels)


def test_validation_subjects_is_the_first_draw():
    lab = np.repeat(np.arange(10, 20), [5, 3, 8, 2, 9, 4, 6, 7, 1, 5])
    for seed, ratio in ((0, 0.2), (3, 0.35), (1, 0.0)):
        subjects = np.unique(lab)
        want = np.random.default_rng(seed).choice(subjects, size=int(np.ceil(ratio * len(subjects))), replace=False)
        assert np.array_equal(inference._validation_subjects(lab, np.random.default_rng(seed), ratio), want)
        assert np.array_equal(inference.plan_enrolment(lab, 3, seed=seed, unseen_valid_ratio=ratio)[0], want)


def test_header_declares_the_entry_points():
    protos = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in (("pcaa_gallery_accumulate", 12), ("pcaa_gallery_score", 14), ("pcaa_gallery_kvote", 8),
                         ("pcaa_stream_score_gallery", 29)):
        assert hasattr(lib, name), name
        assert len(protos[name][1]) == n_args, name
    assert lib.pcaa_abi_version() == _lib.ABI_VERSION
