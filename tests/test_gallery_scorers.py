"""Run-time enrolment through the three scorers and ``enrolment_sweep`` on the device.  N = 32, C = 4, K = 4, a synthetic
encoder, tracks of 60 frames (6 eager windows), fp32 and bf16 modes.  The reference (tests/gallery_ref.py) is applied to
the scorer's OWN ``sup_fv`` and to the predictions the same scorer makes without a gallery: the likelihood inside the
gate, labels and votes equal; the threshold is the midpoint of two adjacent reference likelihoods."""
import numpy as np
import pytest
import torch

import gallery_ref as G
from helpers import T, load_golden, make_encoder
from opensetgaitrecognition_pcaa_amd import constants, datasets, synthetic as syn
from opensetgaitrecognition_pcaa_amd.gallery import Gallery

pytestmark = pytest.mark.gpu

K, N, C, D, F, HOP = 4, 32, 4, 32, 60, constants.CROP_STEP
W = (F - T) // HOP + 1                      # eager windows of one track
KV = 2                                      # windows per vote


def _setup(mode):
    from opensetgaitrecognition_pcaa_amd import functional as F_hip
    F_hip.set_precision(mode)
    enc = make_encoder(K, N, C, True, seed=0).cuda().eval()
    means = torch.from_numpy(load_golden("misc")[0]["means_K4"]).float()
    tracks = [syn.synthetic_pcs(1, F, N, C, seed=61 + i)[0].contiguous().cuda() for i in range(2)]
    # the synthetic encoder puts every window far from the golden means: a gallery mode would be the nearest for all of
    # them.  The prior means of this test are four of track 0's own embeddings, where a trained critic would have placed them.
    from opensetgaitrecognition_pcaa_amd import inference
    fv0 = inference.OpenSetScorer(enc, means).embed_track(tracks[0], drop_last_aligned=False)[1]
    return enc, fv0[[0, 2, 4, 5]].clone().contiguous(), tracks


def _same(a, b, what=""):
    for x, y in zip(a, b):
        assert torch.equal(x, y), what


def _against_ref(got, plain_preds, means, gal, what):
    """(labels, sup_fv, lik) of a scorer with gallery ``gal`` against the reference on its own sup_fv -> the reference"""
    labels, fv, lik = got
    ref = G.gallery_score_ref(fv, plain_preds, means, gal.centroids, gal.counts, gal.high_water, K)
    G.check_separation(ref)
    r = float((np.abs(lik.cpu().numpy() - ref["lik"]) / ref["gate"]).max())
    print(f"[gallery] {what}: worst |err| / gate = {r:.3f}; labels {ref['labels'].tolist()}")
    assert r <= 1.0, (what, r)
    assert np.array_equal(labels.cpu().numpy(), ref["labels"]), what
    return ref


def _ticks(ms, tracks, parts):
    """push two tracks through slots 0 and 1 in ticks of ``parts`` frames each -> per stream (labels, sup_fv, lik), votes"""
    sids = [ms.open(), ms.open()]
    out, votes, pos = {s: [] for s in sids}, {s: {} for s in sids}, 0
    for n in parts:
        counts = [n, n]
        frames = torch.cat([t[pos:pos + n] for t in tracks])
        tick = ms.push(sids, counts, frames)
        pos += n
        for s in sids:
            m = torch.from_numpy(tick.stream == s).cuda()
            out[s].append((tick.preds[m], tick.sup_fv[m], tick.lik[m]))
        for v, s, g in zip(tick.votes.tolist(), tick.vote_stream.tolist(), tick.vote_group.tolist()):
            votes[s][g] = v
    assert pos == F
    cat = {s: tuple(torch.cat([o[i] for o in out[s]]) for i in range(3)) for s in sids}
    return sids, cat, {s: [votes[s][g] for g in range(W // KV)] for s in sids}


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_the_three_scorers(mode):
    from opensetgaitrecognition_pcaa_amd import inference
    enc, means, tracks = _setup(mode)
    chunks, parts_a, parts_b = (7, 29, 0, 24), (30, 6, 6, 6, 6, 6), (36, 12, 12)
    thr0 = 1e-30

    # ---- an empty gallery: the bits of the scorers without one
    plain = inference.OpenSetScorer(enc, means)
    plain.threshold = thr0
    want = [plain.embed_track(t, drop_last_aligned=False) for t in tracks]
    assert want[0][0].numel() == W
    gal = Gallery(D, 4, "cuda")
    sg = inference.OpenSetScorer(enc, means, gallery=gal, n_labels=K)
    sg.threshold = thr0
    for t, w in zip(tracks, want):
        got = sg.embed_track(t, drop_last_aligned=False)
        _same(got, w, "OpenSetScorer, empty gallery")
        assert torch.equal(sg.last_preds, w[0])
        assert torch.equal(sg.vote(got[2], got[0], KV, K), plain.vote(w[2], w[0], KV, K))
    live_plain = inference.StreamingScorer(enc, means, thr0, KV, K, max_push=32)
    live_empty = inference.StreamingScorer(enc, means, thr0, KV, K, max_push=32, gallery=gal)
    pos = 0
    for n in chunks:
        a, b = live_plain.push(tracks[0][pos:pos + n]), live_empty.push(tracks[0][pos:pos + n])
        _same(a, b, "StreamingScorer, empty gallery")
        pos += n
    assert live_plain.n_windows == W and torch.equal(live_plain.votes(), live_empty.votes())
    mk = lambda **kw: inference.MultiStreamScorer(enc, means, thr0, KV, K, max_streams=2, max_push=36, **kw)
    sids, plain_ticks, plain_votes = _ticks(mk(), tracks, parts_a)
    for kw in (dict(gallery=gal), dict(gallery=gal, history=3)):
        _, got, votes = _ticks(mk(**kw), tracks, parts_a)
        for s in sids:
            _same(got[s], plain_ticks[s], "MultiStreamScorer, empty gallery")
        assert votes == plain_votes

    # ---- enrol the person of track 1 from its first three windows
    ident = sg.enrol_track(tracks[1], windows=[0, 1, 2], drop_last_aligned=False)
    assert ident == 0 and gal.identities() == [0] and int(gal.counts[0]) == 3 and int(gal.err) == 0
    assert np.array_equal(gal.centroids[0].cpu().numpy(), G.centroid_ref(want[1][1][:3])[0])
    got = [sg.embed_track(t, drop_last_aligned=False) for t in tracks]
    refs = [_against_ref(g, w[0], means, gal, f"OpenSetScorer track {i}") for i, (g, w) in enumerate(zip(got, want))]
    assert (refs[1]["labels"] == gal.label_of(0, K)).any(), "the enrolled person is recognised in their own track"
    assert (refs[0]["labels"] < K).any(), "and a window on a prior mode keeps the classifier's label"
    for i in range(2):
        assert torch.equal(got[i][1], want[i][1])
    all_lik = np.concatenate([r["lik"] for r in refs])
    thr = G.mid_threshold(all_lik)
    G.check_threshold(all_lik, np.concatenate([r["gate"] for r in refs]), thr)
    sg.threshold = thr
    both = set()
    for g, r in zip(got, refs):
        want_votes = G.gallery_vote_ref(r["lik"], r["labels"], thr, KV, K)
        assert np.array_equal(sg.vote(g[2], g[0], KV, K).cpu().numpy(), want_votes)
        both |= set((want_votes == K).tolist())
    assert both == {True, False}, "known and unknown votes both occur"

    # ---- a live track
    live = inference.StreamingScorer(enc, means, thr, KV, K, max_push=32, gallery=gal)
    pos, out = 0, []
    for n in chunks:
        out.append(live.push(tracks[1][pos:pos + n]))
        pos += n
    out = tuple(torch.cat([o[i] for o in out]) for i in range(3))
    live_plain.reset()
    pos, pp = 0, []
    for n in chunks:
        pp.append(live_plain.push(tracks[1][pos:pos + n])[0])
        pos += n
    r = _against_ref(out, torch.cat(pp), means, gal, "StreamingScorer")
    G.check_threshold(r["lik"], r["gate"], thr)
    assert np.array_equal(live.votes().cpu().numpy(), G.gallery_vote_ref(r["lik"], r["labels"], thr, KV, K))

    # ---- many live tracks: two partitions of the same streams, the reference on each one's own embeddings
    results = []
    for parts in (parts_a, parts_b):
        ms = inference.MultiStreamScorer(enc, means, thr, KV, K, max_streams=2, max_push=36, gallery=gal, history=3)
        sids, got_t, votes = _ticks(ms, tracks, parts)
        _, plain_t, _ = _ticks(inference.MultiStreamScorer(enc, means, thr, KV, K, max_streams=2, max_push=36), tracks, parts)
        for s in sids:
            r = _against_ref(got_t[s], plain_t[s][0], means, gal, f"MultiStreamScorer {parts} stream {s}")
            G.check_threshold(r["lik"], r["gate"], thr)
            assert votes[s] == G.gallery_vote_ref(r["lik"], r["labels"], thr, KV, K).tolist()
        results.append((ms, got_t, votes))
    (ms, got_a, votes_a), (_, got_b, votes_b) = results
    for s in sids:                                     # the same Tick whatever the partition
        assert torch.equal(got_a[s][0], got_b[s][0]) and votes_a[s] == votes_b[s]

    # ---- enrol_stream: the stream's last windows from the device ring, against Gallery.enrol on the ticks' sup_fv
    own = Gallery(D, 4, "cuda")
    own.load_state_dict(gal.state_dict())
    ms.gallery = own
    ident = ms.enrol_stream(sids[0], windows=3)
    assert ident == 1 and own.identities() == [0, 1]
    by_hand = Gallery(D, 4, "cuda")
    by_hand.enrol(got_a[sids[0]][1][-3:].contiguous(), ident=1)
    assert torch.equal(own.centroids[1], by_hand.centroids[1]) and torch.equal(own.sums[1], by_hand.sums[1])
    assert int(own.counts[1]) == 3 and int(own.err) == 0 and torch.equal(own.centroids[0], gal.centroids[0])
    for bad in (0, 4, W + 1):
        with pytest.raises(ValueError):
            ms.enrol_stream(sids[0], windows=bad)
    with pytest.raises(RuntimeError):
        inference.MultiStreamScorer(enc, means, thr, KV, K, gallery=gal).enrol_stream(0, 1)
    with pytest.raises(ValueError):
        inference.MultiStreamScorer(enc, means, thr, KV, K, history=3)              # a history needs a gallery
    with pytest.raises(RuntimeError):
        plain.enrol_track(tracks[0])


def test_enrolment_sweep(monkeypatch):
    """a synthetic ``RawTrackStore`` as tests/test_raw_keep_scorers.py sets one up for ``point_sweep``: with ``shots`` such
    that nobody is enrolled an entry is ``point_sweep``'s record for ``keep = 0``; with three shots the enrolled subjects'
    windows are labelled ``n_labels + 1 + identity``"""
    from opensetgaitrecognition_pcaa_amd import inference
    monkeypatch.setattr(constants, "NFEATURES", C)
    enc = make_encoder(K, N, C, True, seed=0).cuda().eval()
    means = torch.from_numpy(load_golden("misc")[0]["means_K4"]).float()
    tracks, subj, names, splits = [], [], [], []
    for s in range(9):
        for t in range(3):
            tracks.append(syn.synthetic_raw_track(4000 + 10 * s + t, 48 + 6 * (t % 2)))
            subj.append(s)
            names.append(f"{t}{s}")
            splits.append("test" if s < 4 else "unseen")
    st = datasets.RawTrackStore(tracks, subj, ["hands_in_pockets"] * len(tracks), names, splits=splits).to_device("cuda")
    ks = [2]
    point = inference.point_sweep(enc, means, st, [0], ks, N)
    sweep = inference.enrolment_sweep(enc, means, st, [0, 3, 1000], ks, N)
    assert list(sweep) == [0, 3, 1000] and all(set(v) == {2} for v in sweep.values())
    assert sweep[0][2] == point[0][2] and sweep[1000][2] == point[0][2], "nobody enrolled: the plain evaluation"
    assert sweep[3][2]["n_steps"] == 2 and 0.0 <= sweep[3][2]["accuracy"] <= 1.0
    # what the sweep enrolled: the plan on the same labels
    u_lab = st.crops(constants.SPLIT.UNSEEN, N=N, C=C, order="sequential",
                     scenarios=constants.TRAIN_SCENARIOS).materialize(seed=0)[1].cpu().numpy()
    val, idents, rows, keep = inference.plan_enrolment(u_lab, 3)
    assert len(val) == 1 and len(idents) == 2 and keep.sum() == len(u_lab) - 6
