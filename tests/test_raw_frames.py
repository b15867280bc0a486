"""Raw radar detections -> frames on the device (``ops.frames_from_raw``, csrc/raw_frames.hip) and the scorers' raw entries.

The arithmetic gate, wherever device frames are compared with a float64 host result ``want``:

    |got - want| <= 2^-23 |want| + 1e-12 s

``s``: the largest uncentred magnitude of that column in that frame (divided by ``std + 1e-8`` under ``divide_by_std``).
One fp32 rounding is 2^-24 relative, and a differently rounded last double bit can move the result to the neighbouring
fp32 value; the fp64 work (log10 to a few double ulps, an N-term sum to N 2^-53 s, about 1.7e-14 s at N = 150) sits two
orders under 1e-12 s.  Every comparison also prints how many elements are not bit-identical to ``fp32(want)``: reported,
not gated."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import T, load_golden, make_encoder
from opensetgaitrecognition_pcaa_amd import constants, datasets, synthetic as syn

pytestmark = pytest.mark.gpu

HOP = constants.CROP_STEP
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "datagen.npz"))
META = json.loads(str(G["meta"]))


def _frame(rng, n):
    """one raw frame of n detections, the layout of synthetic.synthetic_raw_track"""
    return {"cardinality": np.array([n]), "elements": rng.standard_normal((n, 2)) * 0.4 + rng.standard_normal(2),
            "z_coord": rng.standard_normal(n) * 0.5 + 1.0, "dopplers": rng.standard_normal(n) * 0.8,
            "powers": np.exp(rng.standard_normal(n) * 1.5)}


def _cards(raw):
    return np.array([len(fr["z_coord"]) for fr in raw])


def _to_f32_values(raw):
    """the same frames with every value rounded to fp32 (held as float64)"""
    return [{k: (v if k == "cardinality" else v.astype(np.float32).astype(np.float64)) for k, v in fr.items()} for fr in raw]


def _dev(raw, dtype):
    points, offsets = datasets.pack_raw_frames(raw, dtype)
    return points.cuda(), offsets.cuda()


def _scale(raw, picks, C, div):
    """s of the gate: [n, 1, C]"""
    s = np.empty((len(raw), 1, C))
    for f, fr in enumerate(raw):
        arr = datasets._raw_columns(fr)
        arr[:, 4] = 10 * np.log10(arr[:, 4] + 1e-8)
        vals = arr[:, :C][picks[f]]
        s[f, 0] = np.abs(vals).max(axis=0) / ((vals.std(axis=0) + 1e-8) if div else 1.0)
    return s


def _assert_gate(got, want, raw, picks, div, what):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    C = want.shape[2]
    err = np.abs(got.astype(np.float64) - want)
    bound = 2.0 ** -23 * np.abs(want) + 1e-12 * _scale(raw, np.asarray(picks), C, div)
    differ = int((got != want.astype(np.float32)).sum())
    print(f"[raw frames] {what}: {differ} of {got.size} elements are not bit-identical to fp32(want); "
          f"largest error / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert (err <= bound).all(), (what, float((err / np.maximum(bound, 1e-300)).max()))


# ------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("tag", ["plain", "force10", "divstd"])
def test_host_picks_fp64_against_the_reference(tag):
    """the reference's own process_track output (tests/golden/datagen.npz), its picks redrawn by draw_picks"""
    from opensetgaitrecognition_pcaa_amd import ops
    c = META[tag]
    raw = syn.synthetic_raw_track(c["seed"], c["n_frames"])
    np.random.seed(c["np_seed"])
    picks = datasets.draw_picks(_cards(raw), c["nmax"], c["force"])
    points, offsets = _dev(raw, torch.float64)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = ops.frames_from_raw(points, offsets, c["nmax"], 4, pick=torch.from_numpy(picks).cuda(), divide_by_std=c["div"],
                              err_flag=err)
    assert err.item() == 0
    _assert_gate(got, G[f"{tag}.track"], raw, picks, c["div"], tag)


@pytest.mark.parametrize("div", [False, True])
def test_five_features_power_to_db(div):
    """The goldens were made with 4 features and cannot reach the power column: C = 5 is compared against this package's
    ``process_track(nfeatures=5)`` (whose first four columns the goldens pin), under the same gate."""
    from opensetgaitrecognition_pcaa_amd import ops
    raw = syn.synthetic_raw_track(31, 40)
    np.random.seed(9)
    picks = datasets.draw_picks(_cards(raw), 24)
    np.random.seed(9)
    want = datasets.process_track(raw, divide_by_std=div, nmax=24, nfeatures=5)
    points, offsets = _dev(raw, torch.float64)
    got = ops.frames_from_raw(points, offsets, 24, 5, pick=torch.from_numpy(picks).cuda(), divide_by_std=div)
    _assert_gate(got, want, raw, picks, div, f"C=5 div={div}")
    # without standardisation: the gathered values themselves (dB in the last column), rounded once
    plain = ops.frames_from_raw(points, offsets, 24, 5, pick=torch.from_numpy(picks).cuda(), standardize=False)
    vals = np.stack([np.concatenate([datasets._raw_columns(fr)[:, :4],
                                     10 * np.log10(fr["powers"][:, None] + 1e-8)], axis=1)[picks[f]] for f, fr in enumerate(raw)])
    _assert_gate(plain, vals, raw, picks, False, "C=5 not standardised")


@pytest.mark.parametrize("C,div", [(4, False), (5, True), (3, False)])
def test_fp32_input(C, div):
    """fp32 detections are exact values: against frames_from_picks fed the same values rounded to fp32 first"""
    from opensetgaitrecognition_pcaa_amd import ops
    raw = syn.synthetic_raw_track(32, 30)
    raw32 = _to_f32_values(raw)
    np.random.seed(2)
    picks = datasets.draw_picks(_cards(raw), 20)
    points, offsets = _dev(raw, torch.float32)
    got = ops.frames_from_raw(points, offsets, 20, C, pick=torch.from_numpy(picks).cuda(), divide_by_std=div)
    _assert_gate(got, datasets.frames_from_picks(raw32, picks, C, div), raw32, picks, div, f"fp32 input C={C}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_device_picks_equal_their_host_restatement(dtype):
    from opensetgaitrecognition_pcaa_amd import ops
    rng = np.random.default_rng(4)
    N = 150
    cards = [1, 2, 149, 150, 151, 300, 1023, 1024] + [int(c) for c in rng.integers(3, 400, 24)]
    raw = [_frame(rng, n) for n in cards]
    keys = np.stack([rng.integers(-2 ** 31, 2 ** 31, len(raw)), np.arange(len(raw))], axis=1).astype(np.int32)
    points, offsets = _dev(raw, dtype)
    for seed in (0, 12345678901234, -7):
        pick_out = torch.full((len(raw), N), -5, dtype=torch.int32, device="cuda")
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        got = ops.frames_from_raw(points, offsets, N, 5, seed=seed, frame_key=torch.from_numpy(keys).cuda(),
                                  pick_out=pick_out, err_flag=err)
        assert err.item() == 0
        want_picks = datasets.device_picks_host(seed, keys, cards, N)
        assert np.array_equal(pick_out.cpu().numpy(), want_picks), seed
        src = raw if dtype == torch.float64 else _to_f32_values(raw)
        _assert_gate(got, datasets.frames_from_picks(src, want_picks, 5), src, want_picks, False, f"device picks seed={seed}")


@pytest.mark.parametrize("host_picks", [False, True])
def test_a_frame_depends_on_nothing_but_itself(host_picks):
    """the 6 frames of one stream: alone or in one launch with 15 other streams' frames; as one call or as calls of 2 and 4;
    with n_out == n or padded -- the same bits"""
    from opensetgaitrecognition_pcaa_amd import ops
    S, n, N, C = 16, 6, 32, 5
    tracks = [syn.synthetic_raw_track(200 + s, n, max_points=70) for s in range(S)]
    every = [fr for tr in tracks for fr in tr]
    keys = np.array([(s, f) for s in range(S) for f in range(n)], dtype=np.int32)
    np.random.seed(1)
    picks = datasets.draw_picks(_cards(every), N)

    def run(lo, hi, n_out=None, dtype=torch.float64, div=True):
        points, offsets = _dev(every[lo:hi], dtype)
        kw = (dict(pick=torch.from_numpy(picks[lo:hi]).cuda()) if host_picks else
              dict(seed=3, frame_key=torch.from_numpy(keys[lo:hi]).cuda()))
        return ops.frames_from_raw(points, offsets, N, C, divide_by_std=div, n_out=n_out, **kw)

    for dtype in (torch.float64, torch.float32):
        together = run(0, S * n, dtype=dtype)
        for s in (0, 5, 15):
            alone = run(s * n, (s + 1) * n, dtype=dtype)
            assert torch.equal(alone, together[s * n:(s + 1) * n]), (s, dtype)
            split = torch.cat([run(s * n, s * n + 2, dtype=dtype), run(s * n + 2, (s + 1) * n, dtype=dtype)])
            assert torch.equal(split, alone)
            padded = run(s * n, (s + 1) * n, n_out=8, dtype=dtype)
            assert padded.shape == (8, N, C) and torch.equal(padded[:n], alone) and not padded[n:].any()
    # one launch over a view into a larger packing (absolute offsets): the same frames again
    points, offsets = _dev(every, torch.float64)
    kw = (dict(pick=torch.from_numpy(picks[12:18]).cuda()) if host_picks else
          dict(seed=3, frame_key=torch.from_numpy(keys[12:18]).cuda()))
    view = ops.frames_from_raw(points, offsets[12:19], N, C, divide_by_std=True, **kw)
    assert torch.equal(view, run(12, 18))


def test_bad_frames_are_zeroed_and_flagged():
    """a zero-cardinality frame, one above the cap, an out-of-range supplied pick, offsets beyond the points: each sets
    err_flag and zeroes that frame only; ordinary in-bounds inputs, nothing faults"""
    from opensetgaitrecognition_pcaa_amd import ops
    rng = np.random.default_rng(8)
    N, C = 24, 4
    good = [_frame(rng, n) for n in (5, 30, 17, 40, 9)]
    keys = torch.from_numpy(np.stack([np.full(7, 2), np.arange(7)], axis=1).astype(np.int32)).cuda()

    def run(raw, n_keys, pick=None, points_rows=None, n_out=None):
        points, offsets = _dev(raw, torch.float32)
        if points_rows is not None:
            points = points[:points_rows].contiguous()
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        pick_out = torch.full((len(raw), N), -5, dtype=torch.int32, device="cuda")
        out = ops.frames_from_raw(points, offsets, N, C, pick=pick, seed=1, frame_key=None if pick is not None else keys[:n_keys],
                                  n_out=n_out, pick_out=pick_out, err_flag=err)
        return out, int(err.item()), pick_out

    clean, flag, clean_picks = run(good, 5, n_out=8)
    assert flag == 0 and clean[:5].abs().sum(dim=(1, 2)).min() > 0 and not clean[5:].any(), "padding rows are zero"
    # frames 1 and 3 of seven: no detections at all, and one more than the cap
    empty = {"cardinality": np.array([0]), "elements": np.zeros((0, 2)), "z_coord": np.zeros(0), "dopplers": np.zeros(0),
             "powers": np.zeros(0)}
    assert ops.RAW_MAX_CARD == 1024
    for bad in (empty, _frame(rng, ops.RAW_MAX_CARD + 1)):
        raw = [good[0], bad, good[1], good[2], good[3], good[4]]
        # the keys of the good frames as in the clean run, so that their picks (and bits) must be the same
        k = keys[[0, 6, 1, 2, 3, 4]].contiguous()
        points, offsets = _dev(raw, torch.float32)
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        pick_out = torch.full((6, N), -5, dtype=torch.int32, device="cuda")
        out = ops.frames_from_raw(points, offsets, N, C, seed=1, frame_key=k, n_out=8, pick_out=pick_out, err_flag=err)
        assert err.item() == 1
        assert not out[1].any() and (pick_out[1] == -1).all() and not out[6:].any()
        assert torch.equal(out[[0, 2, 3, 4, 5]], clean[:5]) and torch.equal(pick_out[[0, 2, 3, 4, 5]], clean_picks)
        # the same with supplied picks
        hp = torch.zeros((6, N), dtype=torch.int32, device="cuda")
        hp[[0, 2, 3, 4, 5]] = clean_picks
        err.zero_()
        out = ops.frames_from_raw(points, offsets, N, C, pick=hp, err_flag=err)
        assert err.item() == 1 and not out[1].any() and torch.equal(out[[0, 2, 3, 4, 5]], clean[:5])
    # a supplied pick outside [0, card): one too large, one negative
    for value, frame in ((17, 2), (-1, 4), (2 ** 31 - 1, 0)):
        hp = clean_picks.clone()
        hp[frame, 3] = value
        out, flag, po = run(good, 5, pick=hp)
        keep = [f for f in range(5) if f != frame]
        assert flag == 1 and not out[frame].any() and (po[frame] == -1).all()
        assert torch.equal(out[keep], clean[keep]) and torch.equal(po[keep], clean_picks[keep])
    # offsets that leave the points: the last frame's rows are not all there
    total = int(_cards(good).sum())
    out, flag, _ = run(good, 5, points_rows=total - 2)
    assert flag == 1 and not out[4].any() and torch.equal(out[:4], clean[:4])
    # negative and descending offsets
    points, offsets = _dev(good, torch.float32)
    off = offsets.clone()
    off[0] = -3
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = ops.frames_from_raw(points, off, N, C, seed=1, frame_key=keys[:5], err_flag=err)
    assert err.item() == 1 and not out[0].any() and torch.equal(out[1:], clean[1:5])
    # refusals on the host
    with pytest.raises(RuntimeError):
        ops.frames_from_raw(points.cpu(), offsets, N, C, seed=1, frame_key=keys[:5])
    with pytest.raises(ValueError):
        ops.frames_from_raw(points, offsets, N, C)                       # neither picks nor keys
    with pytest.raises(ValueError):
        ops.frames_from_raw(points, offsets, ops.RAW_MAX_POINTS + 1, C, seed=1, frame_key=keys[:5])
    with pytest.raises(ValueError):
        ops.frames_from_raw(points, offsets, N, 6, seed=1, frame_key=keys[:5])
    with pytest.raises(TypeError):
        ops.frames_from_raw(points.half(), offsets, N, C, seed=1, frame_key=keys[:5])


# ------------------------------------------------------------------------------------------------------- the scorers
def _track_setup():
    """tests/test_track_inference.py::_track_setup"""
    K, N, C = 4, 32, 4
    enc = make_encoder(K, N, C, True, seed=0).cuda().eval()
    means = torch.from_numpy(load_golden("misc")[0]["means_K4"]).float()
    return K, N, C, enc, means


def _assert_same_tick(a, b, what):
    assert np.array_equal(a.stream, b.stream) and np.array_equal(a.window, b.window), what
    assert np.array_equal(a.vote_stream, b.vote_stream) and np.array_equal(a.vote_group, b.vote_group), what
    for name in ("preds", "sup_fv", "lik", "votes"):
        assert torch.equal(getattr(a, name), getattr(b, name)), (what, name)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_multi_stream_push_raw_equals_push_of_the_same_frames(mode):
    """4 tracks through 3 slots (one slot closed and handed out again), ragged counts including 0, device picks on most
    ticks and host picks on every third: ``push_raw`` returns the Tick ``push(ops.frames_from_raw(same arguments))`` returns"""
    from opensetgaitrecognition_pcaa_amd import functional as F_hip, inference, ops
    F_hip.set_precision(mode)
    K, N, C, enc, means = _track_setup()
    lengths = (75, 44, 70, 52)
    tracks = [syn.synthetic_raw_track(300 + i, F, max_points=60) for i, F in enumerate(lengths)]
    a = inference.MultiStreamScorer(enc, means, 1e-30, 2, K, max_streams=3, max_push=8, seed=99)
    b = inference.MultiStreamScorer(enc, means, 1e-30, 2, K, max_streams=3, max_push=8)
    rng = np.random.default_rng(6)
    slot_of, pos = {}, [0] * 4
    for t in (0, 1, 2):
        slot_of[t] = a.open()
        assert b.open() == slot_of[t]
    n_ticks = n_windows = n_votes = n_padded = 0
    while slot_of:
        live = [int(t) for t in rng.permutation(list(slot_of))]
        counts = [int(min(rng.integers(0, 9), lengths[t] - pos[t])) for t in live]
        if n_ticks % 5 == 1:
            counts[0] = 0
        sids = [slot_of[t] for t in live]
        raw = [fr for t, c in zip(live, counts) for fr in tracks[t][pos[t]:pos[t] + c]]
        keys = np.array([(a.track_serial[slot_of[t]], pos[t] + j) for t, c in zip(live, counts) for j in range(c)],
                        dtype=np.int32).reshape(-1, 2)
        points, offsets = _dev(raw, torch.float32)
        pick = None
        if n_ticks % 3 == 2:
            pick = torch.from_numpy(datasets.draw_picks(_cards(raw), N)).cuda()
        got = a.push_raw(sids, counts, points, offsets, pick=pick)
        frames = ops.frames_from_raw(points, offsets, N, C, pick=pick, seed=99,
                                     frame_key=None if pick is not None else torch.from_numpy(keys).cuda())
        want = b.push(sids, counts, frames)
        _assert_same_tick(got, want, (mode, n_ticks))
        n_ticks += 1
        n_windows += len(got)
        n_votes += got.votes.numel()
        n_padded += bool(sum(counts) % F_hip.frame_pad_quantum(N))
        for t, c in zip(live, counts):
            pos[t] += c
        for t in live:
            if pos[t] == lengths[t]:
                a.close(slot_of[t])
                b.close(slot_of.pop(t))
                if t == 1:                                       # track 3 takes the slot track 1 leaves: a new serial
                    slot_of[3] = a.open()
                    assert b.open() == slot_of[3] == 1 and a.track_serial[1] == 3
    assert n_windows > 20 and n_votes > 8 and pos == list(lengths)
    assert n_padded > 0 or mode == "fp32"
    assert a.raw_err.item() == 0 and a.scatter_err.item() == 0
    assert np.array_equal(a.n_frames, b.n_frames) and np.array_equal(a.n_windows, b.n_windows)
    # refusals leave the state alone
    sid = a.open()
    points, offsets = _dev(tracks[0][:2], torch.float32)
    with pytest.raises(RuntimeError):
        a.push_raw([sid], [2], points.cpu(), offsets)
    with pytest.raises(ValueError):
        a.push_raw([sid], [3], points, offsets)
    with pytest.raises(ValueError):
        a.push_raw([sid], [2], points, offsets.long())
    with pytest.raises(ValueError):
        a.push_raw([sid], [2], points, offsets, pick=torch.zeros((2, N + 1), dtype=torch.int32, device="cuda"))
    assert a.n_frames[sid] == 0
    assert len(a.push_raw([sid], [0], points[:0], offsets[:1])) == 0


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_streaming_push_raw_and_embed_raw_track_equal_their_frame_forms(mode):
    from opensetgaitrecognition_pcaa_amd import functional as F_hip, inference, ops
    F_hip.set_precision(mode)
    K, N, C, enc, means = _track_setup()
    raw = syn.synthetic_raw_track(41, 131, max_points=60)
    a = inference.StreamingScorer(enc, means, 1e-30, 3, K, max_push=16, seed=5)
    b = inference.StreamingScorer(enc, means, 1e-30, 3, K, max_push=16)
    for track in range(2):                                  # the second track after reset(): another serial
        pos = 0
        for i, n in enumerate((7, 40, 3, 0, 33, 48)):
            chunk = raw[pos:pos + n]
            points, offsets = _dev(chunk, torch.float64)
            pick = torch.from_numpy(datasets.draw_picks(_cards(chunk), N)).cuda() if i == 2 else None
            keys = torch.from_numpy(np.stack([np.full(n, a.serial), pos + np.arange(n)], axis=1).astype(np.int32)).cuda()
            got = a.push_raw(points, offsets, pick=pick)
            want = b.push(ops.frames_from_raw(points, offsets, N, C, pick=pick, seed=5,
                                              frame_key=None if pick is not None else keys))
            for g, w in zip(got, want):
                assert torch.equal(g, w), (mode, track, i)
            pos += n
        assert a.n_windows == b.n_windows == (pos - T) // HOP + 1 and torch.equal(a.votes(), b.votes())
        a.reset()
        b.reset()
        assert a.serial == track + 1
    assert a.raw_err.item() == 0
    # the whole track at once
    sc = inference.OpenSetScorer(enc, means)
    points, offsets = _dev(raw, torch.float64)
    keys = torch.from_numpy(np.stack([np.full(len(raw), 7), np.arange(len(raw))], axis=1).astype(np.int32)).cuda()
    for pick in (None, torch.from_numpy(datasets.draw_picks(_cards(raw), N)).cuda()):
        got = sc.embed_raw_track(points, offsets, pick=pick, seed=5, track_key=7)
        want = sc.embed_track(ops.frames_from_raw(points, offsets, N, C, pick=pick, seed=5,
                                                  frame_key=None if pick is not None else keys))
        assert got[0].numel() == inference.window_count(len(raw)) > 0
        for g, w in zip(got, want):
            assert torch.equal(g, w), mode
    assert sc.raw_err.item() == 0
    empty = sc.embed_raw_track(points[:0], offsets[:1])
    assert empty[0].numel() == 0


def test_raw_entries_against_host_prepared_frames_fp32():
    """The frames prepared on the host by ``process_track`` (fp32 mode, host picks: the same draws) through ``embed_track``
    against the raw entries, under the fp32-parity gates of DESIGN.md section 2: embeddings within 1e-4 of scale, labels
    equal wherever the reference's top-2 logit margin is not inside that gate."""
    from opensetgaitrecognition_pcaa_amd import functional as F_hip, inference
    K, N, C, enc, means = _track_setup()
    raw = syn.synthetic_raw_track(52, 120, max_points=60)
    np.random.seed(13)
    picks = datasets.draw_picks(_cards(raw), N)
    np.random.seed(13)
    host = torch.from_numpy(datasets.process_track(raw, nmax=N, nfeatures=C)).float().cuda().contiguous()
    sc = inference.OpenSetScorer(enc, means)
    want = sc.embed_track(host, drop_last_aligned=False)
    W = want[0].numel()
    assert W == (len(raw) - T) // HOP + 1
    with torch.no_grad():
        crops = torch.stack([host[j * HOP:j * HOP + T] for j in range(W)]).permute(0, 3, 1, 2)
        logits = F_hip.encoder_forward(enc, crops, False)[0]
    top2 = logits.topk(2, dim=1).values
    tied = (top2[:, 0] - top2[:, 1]) <= 1e-4 * logits.abs().max()
    scale = want[1].abs().max().item()

    def gates(got, what):
        err = (got[1] - want[1]).abs().max().item()
        differ = int((got[0] != want[0]).sum())
        print(f"[raw vs host frames] {what}: embedding difference {err / scale:.2e} of scale; {int(tied.sum())} of {W} windows "
              f"with a top-2 margin inside the gate, {differ} labels differ")
        assert err <= 1e-4 * scale, (what, err / scale)
        assert torch.equal(got[0][~tied], want[0][~tied]), what

    dev_picks = torch.from_numpy(picks).cuda()
    for dtype in (torch.float64, torch.float32):
        points, offsets = _dev(raw, dtype)
        gates(sc.embed_raw_track(points, offsets, pick=dev_picks, drop_last_aligned=False), f"embed_raw_track {dtype}")
        ms = inference.MultiStreamScorer(enc, means, 1e-30, 2, K, max_streams=2, max_push=8)
        ms.open()
        sid = ms.open()
        ticks = []
        for p in range(0, len(raw), 8):
            q = min(p + 8, len(raw))
            ticks.append(ms.push_raw([sid], [q - p], points[offsets[p]:offsets[q]].contiguous(),
                                     (offsets[p:q + 1] - offsets[p]).contiguous(), pick=dev_picks[p:q]))
        gates((torch.cat([t.preds for t in ticks]), torch.cat([t.sup_fv for t in ticks])), f"push_raw {dtype}")
        assert ms.raw_err.item() == 0
