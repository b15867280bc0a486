"""The thinning stage of csrc/raw_frames.hip (the ``_thin`` entry points) on every branch, against its numpy restatement:

(a) ``pick_out`` equals ``datasets.device_picks_host(keep=...)`` integer for integer;
(b) the values pass the gate of tests/test_raw_frames.py (restated below: |err| <= 2^-23 |want| + 1e-12 scale) against
    ``datasets.frames_from_picks`` on those picks;
(c) frames with k_f >= card are ``torch.equal`` to what the entry point without thinning writes, picks included;
(d) ``crops_from_raw(keep...)[b, t]`` is ``torch.equal`` to the frame of store frame ``start[b] + t``;
(e) the compact table: ``u_off == cumsum(min(card, k_f, N))``, rows in first-occurrence order bit-equal to the padded
    rows, weights the multiplicities, unused rows zero with weight 0;
(f) bad frames are zeros, flagged, and leave their neighbours alone.

Shapes: N = 8 (a frame is one partial pass of the 256 threads), 150 with C = 5 (150 * 5 is no multiple of 4: the scalar
store path), 300 (> 256 threads: the strided loops); cards on both sides of every keep and of N, 300 and the cap 1024."""
import numpy as np
import pytest
import torch

import raw_unique_ref as R
from opensetgaitrecognition_pcaa_amd import datasets

pytestmark = pytest.mark.gpu

SEED = 12345678901234
RANGE = (5, 20)


def _keeps(N):
    return (1, 5, N, N + 7, 1024, RANGE)


def _cards(N):
    cards = {1, 2, N - 1, N, N + 1, 300, 1024}
    for k in (1, 5, N, N + 7, 1024) + RANGE:
        cards |= {k - 1, k, k + 1}
    return sorted(c for c in cards if 1 <= c <= 1024)


_FRAMES = {}


def _frames(N):
    """the raw frames of the family for N, their keys and cards: made once, shared, never changed"""
    if N not in _FRAMES:
        rng = np.random.default_rng(100 + N)
        cards = _cards(N)
        raw = [R.make_frame(rng, n) for n in cards]
        keys = np.stack([rng.integers(-2 ** 31, 2 ** 31, len(raw)), np.arange(len(raw))], axis=1).astype(np.int32)
        raw32 = [{k: (v if k == "cardinality" else v.astype(np.float32).astype(np.float64)) for k, v in fr.items()}
                 for fr in raw]
        _FRAMES[N] = (raw, raw32, keys, np.array(cards))
    return _FRAMES[N]


def _dev(raw, dtype):
    points, offsets = datasets.pack_raw_frames(raw, dtype)
    return points.cuda(), offsets.cuda()


def _assert_gate(got, want, raw, picks, what):
    """tests/test_raw_frames.py::_assert_gate, restated: |err| <= 2^-23 |want| + 1e-12 scale, scale the column's largest
    picked |value| (frames not divided by their std)"""
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    C = want.shape[2]
    scale = np.empty((len(raw), 1, C))
    for f, fr in enumerate(raw):
        arr = datasets._raw_columns(fr)
        arr[:, 4] = 10 * np.log10(arr[:, 4] + 1e-8)
        scale[f, 0] = np.abs(arr[:, :C][picks[f]]).max(axis=0)
    err = np.abs(got.astype(np.float64) - want)
    bound = 2.0 ** -23 * np.abs(want) + 1e-12 * scale
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"[raw keep] {what}: largest error / bound = {worst:.3f}")
    assert (err <= bound).all(), (what, worst)


def _k_f(keys, keep):
    """the count of every frame (it does not depend on the rule): what is kept of a frame larger than any count"""
    return np.array([len(k) for k in datasets.device_keep_host(SEED, keys, np.full(len(keys), 2000), keep)])


@pytest.mark.parametrize("rule", ["first", "random"])
@pytest.mark.parametrize("N", [8, 150, 300])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("C", [4, 5])
def test_thinned_frames_crops_and_compact_table(C, dtype, N, rule):
    from opensetgaitrecognition_pcaa_amd import ops
    raw, raw32, keys, cards = _frames(N)
    src = raw if dtype == torch.float64 else raw32
    n = len(raw)
    points, offsets = _dev(raw, dtype)
    P = points.shape[0]
    keys_dev = torch.from_numpy(keys).cuda()
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    plain_picks = torch.empty((n, N), dtype=torch.int32, device="cuda")
    plain = ops.frames_from_raw(points, offsets, N, C, seed=SEED, frame_key=keys_dev, pick_out=plain_picks, err_flag=err)
    rng = np.random.default_rng(N)
    T = 3
    start_host = np.concatenate([[0, 0, n - T, 1], rng.integers(0, n - T + 1, 4)]).astype(np.int32)   # overlapping, repeated
    start = torch.from_numpy(start_host).cuda()
    for keep in _keeps(N):
        what = f"C={C} {dtype} N={N} {rule} keep={keep}"
        kw = dict(seed=SEED, frame_key=keys_dev, keep=keep, keep_rule=rule, err_flag=err)
        pick_out = torch.full((n, N), -5, dtype=torch.int32, device="cuda")
        got = ops.frames_from_raw(points, offsets, N, C, pick_out=pick_out, **kw)
        # (a)
        want_picks = datasets.device_picks_host(SEED, keys, cards, N, keep=keep, keep_rule=rule)
        assert np.array_equal(pick_out.cpu().numpy(), want_picks), what
        # (b)
        _assert_gate(got, datasets.frames_from_picks(src, want_picks, C), src, want_picks, what)
        # (c)
        k_f = _k_f(keys, keep)
        lo, hi = keep if isinstance(keep, tuple) else (keep, keep)
        assert k_f.min() >= lo and k_f.max() <= hi
        same = torch.from_numpy(k_f >= cards).cuda()
        assert same.any() and (keep == 1024 or not same.all()), what
        assert torch.equal(got[same], plain[same]) and torch.equal(pick_out[same], plain_picks[same]), what
        assert same.all() or not torch.equal(got[~same], plain[~same])
        # (d)
        crops = ops.crops_from_raw(points, offsets, start, T, N, C, **kw)
        index = torch.from_numpy(start_host[:, None] + np.arange(T)[None, :]).cuda().long()
        assert torch.equal(crops, got[index]), what
        # (e)
        M = ops.unique_table_rows(P, n, N, hi)
        upicks = torch.full((n, N), -5, dtype=torch.int32, device="cuda")
        rows, weight, u_off = ops.frames_from_raw_unique(points, offsets, N, C, pick_out=upicks, **kw)
        assert rows.shape == (M, C) and torch.equal(upicks, pick_out)
        want_off = np.concatenate([[0], np.cumsum(np.minimum(np.minimum(cards, k_f), N))])
        assert np.array_equal(u_off.cpu().numpy(), want_off), what
        want_w, src_row = np.zeros(M, np.float32), np.full(M, -1, np.int64)
        for f in range(n):
            first, mult = R.unique_first(want_picks[f])
            assert first.size <= want_off[f + 1] - want_off[f]
            want_w[want_off[f]:want_off[f] + first.size] = mult
            src_row[want_off[f]:want_off[f] + first.size] = f * N + first
        assert np.array_equal(weight.cpu().numpy(), want_w), what
        want_rows = R.gather_rows(got.cpu().numpy(), src_row)
        assert np.array_equal(rows.cpu().numpy().view(np.uint32), want_rows.view(np.uint32)), what
    assert err.item() == 0


@pytest.mark.parametrize("rule", ["first", "random"])
def test_bad_frames_are_zeroed_flagged_and_leave_their_neighbours_alone(rule):
    """a frame without detections, one above the cap, offsets that leave the points: zeros (one zero row of weight N in
    the compact table), pick_out -1, the flag set; the other frames have the bits of a clean launch"""
    from opensetgaitrecognition_pcaa_amd import ops
    rng = np.random.default_rng(8)
    N, C, keep = 24, 4, (3, 9)
    good = [R.make_frame(rng, n) for n in (5, 30, 17, 40, 9)]
    keys = torch.from_numpy(np.stack([np.full(7, 2), np.arange(7)], axis=1).astype(np.int32)).cuda()
    empty = {"cardinality": np.array([0]), "elements": np.zeros((0, 2)), "z_coord": np.zeros(0), "dopplers": np.zeros(0),
             "powers": np.zeros(0)}

    def run(raw, k, points_rows=None, off0=None):
        points, offsets = _dev(raw, torch.float32)
        if points_rows is not None:
            points = points[:points_rows].contiguous()
        if off0 is not None:
            offsets = offsets.clone()
            offsets[0] = off0
        err = torch.zeros(2, dtype=torch.int32, device="cuda")
        po = torch.full((len(raw), N), -5, dtype=torch.int32, device="cuda")
        kw = dict(seed=1, frame_key=k.contiguous(), keep=keep, keep_rule=rule)
        out = ops.frames_from_raw(points, offsets, N, C, n_out=8, pick_out=po, err_flag=err[:1], **kw)
        rows, weight, u_off = ops.frames_from_raw_unique(points, offsets, N, C, err_flag=err[1:], **kw)
        start = torch.arange(len(raw) - 1, dtype=torch.int32, device="cuda")
        crops = ops.crops_from_raw(points, offsets, start, 2, N, C, **kw)
        assert torch.equal(crops[:, 0], out[:len(raw) - 1]) and torch.equal(crops[:, 1], out[1:len(raw)])
        return out, po, err.tolist(), rows, weight, u_off.cpu().numpy()

    clean, clean_picks, flags, c_rows, c_weight, c_off = run(good, keys[:5])
    assert flags == [0, 0] and clean[:5].abs().sum(dim=(1, 2)).min() > 0 and not clean[5:].any()
    for bad in (empty, R.make_frame(rng, ops.RAW_MAX_CARD + 1)):
        raw = [good[0], bad, good[1], good[2], good[3], good[4]]
        out, po, flags, rows, weight, u_off = run(raw, keys[[0, 6, 1, 2, 3, 4]])
        others = [0, 2, 3, 4, 5]
        assert flags == [1, 1] and not out[1].any() and (po[1] == -1).all() and not out[6:].any()
        assert torch.equal(out[others], clean[:5]) and torch.equal(po[others], clean_picks)
        assert u_off[2] - u_off[1] == 1 and weight[u_off[1]].item() == N and not rows[u_off[1]].any()     # a bad frame counts 1
        for f, g in zip(others, range(5)):
            a, b = u_off[f], u_off[f + 1]
            assert b - a == c_off[g + 1] - c_off[g]
            assert torch.equal(rows[a:b], c_rows[c_off[g]:c_off[g + 1]]) and torch.equal(weight[a:b], c_weight[c_off[g]:c_off[g + 1]])
    total = int(R.cards_of(good).sum())
    out, po, flags, *_ = run(good, keys[:5], points_rows=total - 2)                 # the last frame's rows are not all there
    assert flags == [1, 1] and not out[4].any() and (po[4] == -1).all() and torch.equal(out[:4], clean[:4])
    out, po, flags, *_ = run(good, keys[:5], off0=-3)                               # a negative offset
    assert flags == [1, 1] and not out[0].any() and torch.equal(out[1:5], clean[1:5])
