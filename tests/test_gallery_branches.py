"""Every branch of csrc/gallery.hip through the C ABI against the wide-arithmetic restatement of tests/gallery_ref.py (its
gates, input conditions and planted defects are shown on the CPU by tests/test_gallery_gates_cpu.py).

    test_score[case]                    lik inside the gate, near and labels equal: B across the 4-window workgroup, Kc = 1,
                                        D = 1 and 33, E = 0 / 1 / 63 / 64 / 65 (the lanes' stride) / 300 with empty slots /
                                        1 024; rows at distance 0, 50, the denormal boundary, 1 600; the planted ties
    test_empty_gallery_is_the_parent    no live slot: the bits of pcaa_joint_likelihood and pcaa_kvote
    test_whole_split_and_stream_agree   one call, two calls and the stream tick give the same bits
    test_accumulate[m]                  the host expression bit for bit; two calls against one; a rows list; a bad row
    test_vote_exhaustive                every pattern over {0, 1, n_labels + 1, n_labels + 2}, k = 1 .. 4; pcaa_kvote's on trained labels
    test_stream[k]                      ticks of k + 1 and 2k + 1 windows, history across launches, an enrolment between two
                                        ticks (stored labels stay), H = 3 over 2H + 1 windows
    test_refusals                       the invalid-argument status of each entry point, nothing launched
"""
import ctypes

import numpy as np
import pytest
import torch

import critic_loss_ref as R
import gallery_ref as G
from opensetgaitrecognition_pcaa_amd import _lib, inference, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
_CASES = {}


def _case(case):
    """inputs on the device, the reference (computed once, shared, never written)"""
    if case not in _CASES:
        c = G.gallery_case(*case, device=DEV)
        ref = G.gallery_score_ref(c["x"], c["preds"], c["means"], c["centroids"], c["counts"], c["E"], c["n_labels"])
        G.check_separation(ref, c["tie_pairs"])
        _CASES[case] = (c, ref)
    return _CASES[case]


def _score_abi(x, preds, means, cent, counts, E, n_labels):
    B, D = x.shape
    lik = torch.full((B,), float("nan"), dtype=torch.float64, device=DEV)
    labels = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    near = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    rc = _lib.load().pcaa_gallery_score(x.data_ptr(), preds.data_ptr(), means.data_ptr(), B, means.shape[0], D,
                                        cent.data_ptr() if E else None, counts.data_ptr() if E else None, E, n_labels,
                                        lik.data_ptr(), labels.data_ptr(), near.data_ptr(), ops._s())
    assert rc == 0, _lib.load().pcaa_last_error()
    return lik, labels, near


@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_score(case):
    c, ref = _case(case)
    lik, labels, near = _score_abi(c["x"], c["preds"], c["means"], c["centroids"], c["counts"], c["E"], c["n_labels"])
    got = lik.cpu().numpy()
    r = float((np.abs(got - ref["lik"]) / ref["gate"]).max())
    print(f"[gallery] score {G.case_id(case)}: worst |err| / gate = {r:.3f}")
    assert np.isfinite(got).all() and r <= 1.0, r
    assert np.array_equal(near.cpu().numpy(), ref["near"])
    assert np.array_equal(labels.cpu().numpy(), ref["labels"])
    # the wrapper is the same launch
    lik2, labels2, near2 = ops.gallery_score(c["x"], c["preds"], c["means"], c["centroids"], c["counts"], c["E"], c["n_labels"])
    assert torch.equal(lik2, lik) and torch.equal(labels2, labels) and torch.equal(near2, near)


@pytest.mark.parametrize("case", [G.CASES[0], G.CASES[3], G.CASES[5]], ids=G.case_id)
def test_empty_gallery_is_the_parent(case):
    c, _ = _case(case)
    want = inference.joint_likelihood(c["x"], c["means"])
    empty = torch.zeros_like(c["counts"])
    for E in sorted({0, c["E"]}):                       # no slot at all; every slot scanned and found empty
        lik, labels, near = _score_abi(c["x"], c["preds"], c["means"], c["centroids"], empty, E, c["n_labels"])
        assert torch.equal(lik, want), "bit-equal to pcaa_joint_likelihood"
        assert torch.equal(labels, c["preds"]) and bool((near < c["means"].shape[0]).all())
    # the vote on trained labels is pcaa_kvote's
    for k, (lk, pr) in R.kvote_exhaustive().items():
        lk, pr = torch.from_numpy(lk).to(DEV), torch.from_numpy(pr).to(DEV)
        assert torch.equal(ops.gallery_vote(lk, pr, 0.5, k, 3), inference.k_vote(lk, pr, 0.5, k, 3))


def _tick_args(n_frames, n_windows, sids, counts, k, ring=4096):
    plan = inference.plan_tick(n_frames, n_windows, sids, counts, 1, 1, k, ring, 1)     # T = hop = 1: one window per frame
    dev = [torch.from_numpy(a).to(DEV) for a in (plan.run_start, plan.win_stream, plan.win_j, plan.vote_pos)]
    return plan, dev


@pytest.mark.parametrize("case", [G.CASES[4], G.CASES[5], G.CASES[6]], ids=G.case_id)
def test_whole_split_and_stream_agree(case):
    c, _ = _case(case)
    B, Kc = c["x"].shape[0], c["means"].shape[0]
    args = (c["means"], c["centroids"], c["counts"], c["E"], c["n_labels"])
    whole = ops.gallery_score(c["x"], c["preds"], *args)
    cut = B // 3 + 1
    parts = [ops.gallery_score(c["x"][a:b].contiguous(), c["preds"][a:b].contiguous(), *args) for a, b in ((0, cut), (cut, B))]
    for w, a, b in zip(whole, *parts):
        assert torch.equal(w, torch.cat([a, b])), "a window's outputs do not depend on the batch or its position"
    # the stream tick: one-hot logits make the argmax the same preds; two streams share the windows
    logits = torch.nn.functional.one_hot(c["preds"], Kc).float().contiguous()
    k, n0 = 3, B // 2
    plan, dev = _tick_args(np.zeros(2, np.int64), np.zeros(2, np.int64), [1, 0], [n0, B - n0], k)
    hist_lik = torch.zeros((2, k), dtype=torch.float64, device=DEV)
    hist_label = torch.zeros((2, k), dtype=torch.int64, device=DEV)
    labels, lik, near, votes = ops.stream_score_gallery(logits, c["x"], c["means"], *dev, plan.vote_group.size, 0.0, k,
                                                        c["n_labels"], c["centroids"], c["counts"], c["E"], hist_lik, hist_label)
    assert torch.equal(lik, whole[0]) and torch.equal(labels, whole[1]) and torch.equal(near, whole[2])


@pytest.mark.parametrize("m", G.ACC_M)
def test_accumulate(m):
    D, E_max, slot = 32, 5, 3
    fv = G.accumulate_inputs(m + 3, D, seed=10 + m, device=DEV)

    def fresh():
        return (torch.zeros((E_max, D), dtype=torch.float64, device=DEV), torch.zeros(E_max, dtype=torch.int32, device=DEV),
                torch.full((E_max, D), 9.0, dtype=torch.float32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV))

    def same(bufs, want):
        c, s, n = want
        sums, counts, cent, _ = bufs
        assert int(counts[slot]) == n and counts.sum().item() == n
        assert np.array_equal(sums[slot].cpu().numpy(), s), "the running fp64 sum, bit for bit"
        assert np.array_equal(cent[slot].cpu().numpy(), c), "np.float32(cumsum_in_float64[-1] / count), bit for bit"
        other = [e for e in range(E_max) if e != slot]
        assert bool((cent[other] == 9.0).all()) and not sums[other].any()

    one = fresh()                                                       # rows 0 .. m - 1 in one call
    ops.gallery_accumulate(fv[:m].contiguous(), slot, *one[:3], err_flag=one[3])
    same(one, G.centroid_ref(fv[:m]))
    assert int(one[3]) == 0
    if m > 1:                                                           # two calls continue the running sum
        two = fresh()
        ops.gallery_accumulate(fv[:m // 2].contiguous(), slot, *two[:3], err_flag=two[3])
        ops.gallery_accumulate(fv[m // 2:m].contiguous(), slot, *two[:3], err_flag=two[3])
        for a, b in zip(one, two):
            assert torch.equal(a, b)
    rows = np.arange(m + 3)[::-1][:m].copy()                            # a rows list, another order
    lst = fresh()
    ops.gallery_accumulate(fv, slot, *lst[:3], rows=torch.from_numpy(rows.astype(np.int32)).to(DEV), err_flag=lst[3])
    same(lst, G.centroid_ref(fv, rows))
    assert int(lst[3]) == 0
    bad_rows = np.concatenate([rows[:m // 2], [m + 3], rows[m // 2:], [-1]])     # out of range: skipped, flagged
    bad = fresh()
    ops.gallery_accumulate(fv, slot, *bad[:3], rows=torch.from_numpy(bad_rows.astype(np.int32)).to(DEV), err_flag=bad[3])
    same(bad, G.centroid_ref(fv, rows))
    assert int(bad[3]) == 1


def test_vote_exhaustive():
    thr, nl = 0.5, 3
    for k, (lik, labels) in G.vote_exhaustive((0, 1, nl + 1, nl + 2)).items():
        want = G.gallery_vote_ref(lik, labels, thr, k, nl)
        assert (lik == thr).any() and len(want) == 8 ** k and (want > nl).any() and (want == nl).any() and (want < nl).any()
        got = ops.gallery_vote(torch.from_numpy(lik).to(DEV), torch.from_numpy(labels).to(DEV), thr, k, nl)
        bad = int((got.cpu().numpy() != want).sum())
        print(f"[gallery] vote k={k}: {len(want)} groups, {bad} differ")
        assert bad == 0
    lik, labels = G.vote_exhaustive((0, nl + 2), ks=(3,))[3]
    lik, labels = np.concatenate([lik, [9.0, 9.0]]), np.concatenate([labels, [5, 5]])       # a trailing partial group
    got = ops.gallery_vote(torch.from_numpy(lik).to(DEV), torch.from_numpy(labels).to(DEV), thr, 3, nl)
    assert np.array_equal(got.cpu().numpy(), G.gallery_vote_ref(lik, labels, thr, 3, nl))


@pytest.mark.parametrize("k", G.STREAM_KS)
def test_stream(k):
    """the scenario of gallery_ref.stream_scenario: ticks of k + 1, 2k + 1, 0 and 2H + 1 windows of one stream, history
    across launches, an enrolment from the ring between two ticks, H = 3"""
    from opensetgaitrecognition_pcaa_amd.gallery import ring_rows
    S = G.stream_scenario(k, DEV)
    D, H, nl, n, ticks = S["D"], S["H"], S["n_labels"], S["n"], S["ticks"]
    fv, logits, means = S["fv"], S["logits"], S["means"]
    sums = torch.zeros((2, D), dtype=torch.float64, device=DEV)
    counts = torch.zeros(2, dtype=torch.int32, device=DEV)
    cent = torch.zeros((2, D), dtype=torch.float32, device=DEV)
    hist_lik = torch.full((S["n_slots"], k), float("nan"), dtype=torch.float64, device=DEV)
    hist_label = torch.full((S["n_slots"], k), -7, dtype=torch.int64, device=DEV)
    fv_hist = torch.full((S["n_slots"] * H, D), float("nan"), dtype=torch.float32, device=DEV)
    ops.gallery_accumulate(S["person"][:1].contiguous(), 0, sums, counts, cent)    # identity 0 is there from the start
    assert np.array_equal(cent.cpu().numpy(), S["before"][0])
    E = 1
    nf, nw = np.zeros(S["n_slots"], np.int64), np.zeros(S["n_slots"], np.int64)
    got_lik, got_lab, got_votes = [], [], {}
    a = 0
    for t, cnt in enumerate(ticks):
        if a == S["enrol_after"] and E == 1:                            # between two ticks: enrol person 1 from the ring
            rows = ring_rows(int(nw[2]), H, S["m"], 2)
            ops.gallery_accumulate(fv_hist, 1, sums, counts, cent, rows=torch.from_numpy(rows).to(DEV))
            E = 2
            assert np.array_equal(cent.cpu().numpy(), S["after"][0]), "the stream's last m windows, oldest first"
            assert counts.tolist() == S["after"][1].tolist()
        ride = {0: (0, 2), 3: (2, 5)}.get(t)                            # slot 0 rides along in the first and the last tick
        sids, cs = ([0, 2], [ride[1] - ride[0], cnt]) if ride else ([2], [cnt])
        lg, x = logits[a:a + cnt], fv[a:a + cnt]
        if ride:
            lg, x = torch.cat([S["other_logits"][ride[0]:ride[1]], lg]), torch.cat([S["other"][ride[0]:ride[1]], x])
        plan, dev = _tick_args(nf, nw, sids, cs, k)
        nf[sids], nw[sids] = plan.n_frames, plan.n_windows
        a += cnt
        if plan.win_row.size == 0:
            continue
        labels, lik, near, votes = ops.stream_score_gallery(lg.contiguous(), x.contiguous(), means, *dev, plan.vote_group.size,
                                                            S["thr"], k, nl, cent, counts, E, hist_lik, hist_label, fv_hist)
        mine = torch.from_numpy(plan.win_stream == 2).to(DEV)
        got_lik.append(lik[mine]), got_lab.append(labels[mine])
        for v, s, g in zip(votes.tolist(), plan.vote_stream.tolist(), plan.vote_group.tolist()):
            if s == 2:
                assert g not in got_votes
                got_votes[g] = v
    got_lik, got_lab = torch.cat(got_lik).cpu().numpy(), torch.cat(got_lab).cpu().numpy()
    r = float((np.abs(got_lik - S["lik"]) / S["gate"]).max())
    print(f"[gallery] stream k={k}: {n} windows, worst |err| / gate = {r:.3f}")
    assert r <= 1.0
    assert np.array_equal(got_lab, S["labels"])
    assert [got_votes.get(g) for g in range(n // k)] == S["votes"].tolist()
    # the ring after 2H + 1 more windows: window j in row 2 * H + j % H, the later one where two share a row
    for j in range(n - H, n):
        assert torch.equal(fv_hist[2 * H + j % H], fv[j])
    assert torch.isnan(fv_hist[H:2 * H]).all() and torch.isnan(hist_lik[1]).all(), "a stream that is in no tick keeps its state"
    for j in range(n - k, n):                                           # the vote history holds the labels as stored
        assert int(hist_label[2, j % k]) == S["labels"][j] and float(hist_lik[2, j % k]) == got_lik[j]


def test_refusals():
    lib = _lib.load()
    c, _ = _case(G.CASES[1])
    x, preds, means, cent, counts = c["x"], c["preds"], c["means"], c["centroids"], c["counts"]
    out = torch.zeros(8, dtype=torch.float64, device=DEV)
    p = [t.data_ptr() for t in (x, preds, means, cent, counts)]
    o = out.data_ptr()
    bad = [
        lib.pcaa_gallery_score(p[0], p[1], p[2], 0, 4, 32, p[3], p[4], 1, 4, o, o, o, ops._s()),
        lib.pcaa_gallery_score(p[0], p[1], p[2], 1, 4, 32, None, p[4], 1, 4, o, o, o, ops._s()),
        lib.pcaa_gallery_score(p[0], p[1], p[2], 1, 4, 32, p[3], p[4], -1, 4, o, o, o, ops._s()),
        lib.pcaa_gallery_score(p[0], None, p[2], 1, 4, 32, p[3], p[4], 1, 4, o, o, o, ops._s()),
        lib.pcaa_gallery_accumulate(p[0], 1, 32, None, 1, 1, 1, o, p[4], p[3], None, ops._s()),        # slot == E_max
        lib.pcaa_gallery_accumulate(p[0], 1, 32, None, 2, 0, 1, o, p[4], p[3], None, ops._s()),        # m > n_rows, no list
        lib.pcaa_gallery_accumulate(p[0], 1, 32, None, 0, 0, 1, o, p[4], p[3], None, ops._s()),
        lib.pcaa_gallery_kvote(o, p[1], ctypes.c_double(0.5), 0, 4, 1, o, ops._s()),
    ]
    assert all(rc == 1 for rc in bad), bad
    assert b"pcaa_gallery_kvote" in lib.pcaa_last_error()
    torch.cuda.synchronize()
    assert not out.any(), "nothing was launched"
    with pytest.raises(ValueError):
        ops.gallery_score(x, preds, means, cent, counts, 2, 4)                     # E beyond the buffers
    with pytest.raises(ValueError):
        ops.gallery_accumulate(x, 1, torch.zeros((1, 32), dtype=torch.float64, device=DEV), counts, cent)
    with pytest.raises(TypeError):
        ops.gallery_vote(out, preds.int(), 0.5, 1, 4)
    with pytest.raises(ValueError):
        ops.stream_score_gallery(x, x, means, torch.zeros(2, dtype=torch.int32, device=DEV),
                                 *(torch.zeros(1, dtype=torch.int32, device=DEV),) * 3, 0, 0.5, 1, 4, cent,
                                 counts, 1, torch.zeros((1, 1), dtype=torch.float64, device=DEV),
                                 torch.zeros((1, 1), dtype=torch.int64, device=DEV),
                                 torch.zeros((3, 31), dtype=torch.float32, device=DEV))   # fv_hist of another width
