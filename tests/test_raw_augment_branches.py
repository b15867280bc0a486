"""The augmentation stage of csrc/raw_frames.hip on every branch of its kernels (``ops.frames_from_raw(augment=)``,
``crops_from_raw``, ``frames_from_raw_unique``), against ``datasets.frames_from_picks(augment=)`` in float64.

The gate is that of test_raw_frames.py, ``|got - want| <= 2^-23 |want| + 1e-12 s``, with ``s`` the largest uncentred
magnitude of the AUGMENTED column in the frame (divided by ``std + 1e-8`` under ``divide_by_std``).  It holds for the
reason derived there: the stage adds fp64 ``sin``, ``cos``, ``log`` and ``sqrt``, each accurate to a few double ulps, on
draws with ``|g| < 7``, which stays orders below ``1e-12 s``; the one rounding to fp32 is unchanged.

The exact properties (mirror, power-of-two scale, untouched columns) carry no tolerance: negation and doubling commute
with every rounding of the mean and of the centring."""
import ctypes

import numpy as np
import pytest
import torch

from test_raw_frames import _cards, _dev, _frame, _to_f32_values
from opensetgaitrecognition_pcaa_amd import datasets

pytestmark = pytest.mark.gpu

CARDS = [1, 4, 5, 6, 31, 32, 33, 149, 150, 151, 300, 1024, 2, 77]
FULL = {"yaw": 1.1, "mirror": True, "scale": (0.8, 1.25), "speed": (0.7, 1.3), "noise": [0.05, 0.04, 0.06, 0.2, 1.5]}
SEED = 0x1234567890ab


def _frames():
    rng = np.random.default_rng(12)
    raw = [_frame(rng, n) for n in CARDS]
    serial = rng.integers(-2 ** 31, 2 ** 31, 5)[[0, 1, 0, 2, 2, 3, 0, 1, 4, 4, 3, 2, 1, 0]]     # frames share serials
    keys = np.stack([serial, rng.integers(-2 ** 31, 2 ** 31, len(CARDS))], axis=1).astype(np.int32)
    return raw, keys


RAW, KEYS = _frames()


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gate(got, want, cols, picks, div, what):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    s = np.empty((len(cols), 1, want.shape[2]))
    for f, arr in enumerate(cols):
        vals = arr[picks[f]]
        s[f, 0] = np.abs(vals).max(axis=0) / ((vals.std(axis=0) + 1e-8) if div else 1.0)
    err = np.abs(got.astype(np.float64) - want)
    bound = 2.0 ** -23 * np.abs(want) + 1e-12 * s
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"[raw augment] {what}: {int((got != want.astype(np.float32)).sum())} of {got.size} elements are not bit-identical "
          f"to fp32(want); largest error / bound = {ratio:.3f}")
    assert (err <= bound).all(), (what, ratio)


MODES = ["device", "supplied", "first20", "random3_40"]


def _mode(mode, N):
    """-> (kwargs of the ops call, the picks the host expects)"""
    if mode == "supplied":
        picks = datasets.device_picks_host(99, KEYS, CARDS, N)
        return dict(pick=_cuda(picks)), picks
    keep = {"device": {}, "first20": dict(keep=20, keep_rule="first"), "random3_40": dict(keep=(3, 40), keep_rule="random")}[mode]
    return dict(keep), datasets.device_picks_host(SEED, KEYS, CARDS, N, **keep)


@pytest.mark.parametrize("C", [2, 4, 5])
@pytest.mark.parametrize("N", [5, 32, 150, 300])
def test_augmented_frames_against_fp64(N, C):
    """vector and scalar stores (N C % 4), pad and subsample, N above one pass of 256 threads; fp32 and fp64 points;
    divide_by_std on and off; device picks, supplied picks, thinned first / random"""
    from opensetgaitrecognition_pcaa_amd import ops
    keys = _cuda(KEYS)
    for dtype in (torch.float64, torch.float32):
        src = RAW if dtype == torch.float64 else _to_f32_values(RAW)
        points, offsets = _dev(RAW, dtype)
        cols = datasets.augmented_columns(src, C, FULL, SEED, KEYS)
        for mode in MODES:
            kw, picks = _mode(mode, N)
            for div in (False, True):
                err = torch.zeros(1, dtype=torch.int32, device="cuda")
                pick_out = torch.full((len(RAW), N), -5, dtype=torch.int32, device="cuda")
                got = ops.frames_from_raw(points, offsets, N, C, seed=SEED, frame_key=keys, divide_by_std=div, augment=FULL,
                                          pick_out=pick_out, err_flag=err, **kw)
                assert err.item() == 0
                assert np.array_equal(pick_out.cpu().numpy(), picks), (mode, "the stage does not touch the picks")
                want = datasets.frames_from_picks(src, picks, C, div, augment=FULL, seed=SEED, keys=KEYS)
                _gate(got, want, cols, picks, div, f"N={N} C={C} {dtype} {mode} div={div}")


def test_noise_alone_and_geometry_alone_against_fp64():
    """the skipped-step branches: each group of steps with the others neutral"""
    from opensetgaitrecognition_pcaa_amd import ops
    points, offsets = _dev(RAW, torch.float64)
    keys = _cuda(KEYS)
    N, C = 32, 5
    picks = datasets.device_picks_host(SEED, KEYS, CARDS, N)
    for aug in ({"noise": FULL["noise"]}, {"noise": {"power": 2.0}}, {"yaw": 3.0}, {"mirror": True}, {"scale": (0.5, 0.6)},
                {"speed": 1.7}, {"yaw": 0.2, "noise": {"x": 0.1}}):
        got = ops.frames_from_raw(points, offsets, N, C, seed=SEED, frame_key=keys, augment=aug)
        want = datasets.frames_from_picks(RAW, picks, C, augment=aug, seed=SEED, keys=KEYS)
        _gate(got, want, datasets.augmented_columns(RAW, C, aug, SEED, KEYS), picks, False, f"{aug}")
    plain = ops.frames_from_raw(points, offsets, N, C, seed=SEED, frame_key=keys)
    assert torch.equal(ops.frames_from_raw(points, offsets, N, C, seed=SEED, frame_key=keys, augment={"scale": 1}), plain)


def test_crops_are_the_frames_bit_for_bit():
    from opensetgaitrecognition_pcaa_amd import ops
    points, offsets = _dev(RAW, torch.float32)
    keys = _cuda(KEYS)
    T = 4
    start = torch.tensor([0, 2, 2], dtype=torch.int32, device="cuda")             # overlapping, repeated
    for N, C in ((32, 4), (150, 5), (5, 2)):
        for kw in ({}, dict(keep=(3, 40), keep_rule="random"), dict(pick=_cuda(datasets.device_picks_host(99, KEYS, CARDS, N)))):
            for div in (False, True):
                err = torch.zeros(1, dtype=torch.int32, device="cuda")
                frames = ops.frames_from_raw(points, offsets, N, C, seed=SEED, frame_key=keys, divide_by_std=div,
                                             augment=FULL, err_flag=err, **kw)
                crops = ops.crops_from_raw(points, offsets, start, T, N, C, seed=SEED, frame_key=keys, divide_by_std=div,
                                           augment=FULL, err_flag=err, **kw)
                assert err.item() == 0 and crops.shape == (3, T, N, C)
                for b, s in enumerate(start.tolist()):
                    assert torch.equal(crops[b], frames[s:s + T]), (N, C, b)


def test_compact_rows_are_the_padded_rows_and_the_table_is_unchanged():
    from opensetgaitrecognition_pcaa_amd import ops
    points, offsets = _dev(RAW, torch.float32)
    keys = _cuda(KEYS)
    for N, C in ((32, 4), (150, 5), (300, 2), (5, 4)):
        for kw in ({}, dict(keep=20), dict(keep=(3, 40), keep_rule="random"),
                   dict(pick=_cuda(datasets.device_picks_host(99, KEYS, CARDS, N)))):
            for div in (False, True):
                common = dict(seed=SEED, frame_key=keys, divide_by_std=div, **kw)
                pick_out = torch.full((len(RAW), N), -5, dtype=torch.int32, device="cuda")
                err = torch.zeros(1, dtype=torch.int32, device="cuda")
                padded = ops.frames_from_raw(points, offsets, N, C, augment=FULL, pick_out=pick_out, err_flag=err, **common)
                rows, weight, u_off = ops.frames_from_raw_unique(points, offsets, N, C, augment=FULL, err_flag=err, **common)
                _, weight0, u_off0 = ops.frames_from_raw_unique(points, offsets, N, C, err_flag=err, **common)
                assert err.item() == 0
                assert torch.equal(u_off, u_off0) and torch.equal(weight, weight0), "noise by detection: the same table"
                picks, u, rows, weight, padded = pick_out.cpu().numpy(), u_off.cpu().numpy(), rows.cpu(), weight.cpu(), padded.cpu()
                for f in range(len(RAW)):
                    uniq, first, counts = np.unique(picks[f], return_index=True, return_counts=True)
                    order = np.argsort(first)                                     # order of first occurrence
                    n = len(uniq)
                    assert n <= u[f + 1] - u[f]
                    assert torch.equal(rows[u[f]:u[f] + n], padded[f][first[order]]), (N, C, f)
                    assert np.array_equal(weight[u[f]:u[f] + n].numpy(), counts[order].astype(np.float32))
                    assert not rows[u[f] + n:u[f + 1]].any() and not weight[u[f] + n:u[f + 1]].any()


# ----------------------------------------------------------------------------------------------------- exact properties
def _pair(aug, N=32, C=5, dtype=torch.float32):
    from opensetgaitrecognition_pcaa_amd import ops
    points, offsets = _dev(RAW, dtype)
    keys = _cuda(KEYS)
    plain = ops.frames_from_raw(points, offsets, N, C, seed=SEED, frame_key=keys)
    moved = ops.frames_from_raw(points, offsets, N, C, seed=SEED, frame_key=keys, augment=aug)
    return plain, moved


@pytest.mark.parametrize("N", [32, 300])
def test_mirror_only(N):
    plain, moved = _pair({"mirror": True}, N)
    assert torch.equal(moved[:, :, 1:], plain[:, :, 1:]), "y, z, Doppler, power"
    flip = datasets.augment_draws_host(SEED, KEYS[:, 0], {"mirror": True})["mirror"]
    assert flip.any() and not flip.all()
    for f in range(len(RAW)):
        assert torch.equal(moved[f, :, 0], -plain[f, :, 0] if flip[f] else plain[f, :, 0]), f


@pytest.mark.parametrize("N", [32, 300])
def test_scale_two_doubles_the_coordinates(N):
    plain, moved = _pair({"scale": (2, 2)}, N)
    assert torch.equal(moved[:, :, :3], 2 * plain[:, :, :3]) and torch.equal(moved[:, :, 3:], plain[:, :, 3:])


def test_doppler_noise_leaves_the_coordinates():
    plain, moved = _pair({"noise": {"doppler": 0.5}})
    assert torch.equal(moved[:, :, :3], plain[:, :, :3]) and torch.equal(moved[:, :, 4], plain[:, :, 4])
    assert not torch.equal(moved[:, :, 3], plain[:, :, 3])


@pytest.mark.parametrize("N", [32, 300])
def test_yaw_only_keeps_z_doppler_and_distances(N):
    """pairwise xy distances inside a frame agree within 8 * 2^-24 * (largest centred |coordinate| of the un-augmented
    frame): two fp32 roundings per coordinate per version, both versions.  A point moves by at most sqrt(2) 2^-24 b under
    its rounding, b the version's largest |coordinate|, a distance by twice that; the turned frame's b is at most sqrt(2)
    times the other's: 2 sqrt(2) (1 + sqrt(2)) = 6.9 <= 8."""
    plain, moved = _pair({"yaw": 3.0}, N)
    assert torch.equal(moved[:, :, 2:], plain[:, :, 2:])
    assert not torch.equal(moved[:, :, :2], plain[:, :, :2])
    p, m = plain[:, :, :2].double(), moved[:, :, :2].double()
    d0, d1 = torch.cdist(p, p), torch.cdist(m, m)
    big = p.abs().amax(dim=(1, 2))
    ratio = ((d1 - d0).abs().amax(dim=(1, 2)) / (8 * 2.0 ** -24 * big).clamp_min(1e-300))
    print(f"[raw augment] yaw only N={N}: largest distance change / bound = {ratio.max().item():.3f}")
    assert ((d1 - d0).abs().amax(dim=(1, 2)) <= 8 * 2.0 ** -24 * big).all()


def test_a_frame_depends_on_nothing_but_itself():
    """written alone, inside a longer launch, through a view of the packing, and in a crop: the same bits"""
    from opensetgaitrecognition_pcaa_amd import ops
    N, C = 32, 5
    points, offsets = _dev(RAW, torch.float64)
    keys = _cuda(KEYS)
    together = ops.frames_from_raw(points, offsets, N, C, seed=SEED, frame_key=keys, divide_by_std=True, augment=FULL)
    for f in (0, 7, 11, 13):
        p1, o1 = _dev(RAW[f:f + 1], torch.float64)
        alone = ops.frames_from_raw(p1, o1, N, C, seed=SEED, frame_key=keys[f:f + 1], divide_by_std=True, augment=FULL,
                                    n_out=3)
        assert torch.equal(alone[0], together[f]) and not alone[1:].any(), f
        view = ops.frames_from_raw(points, offsets[f:f + 2], N, C, seed=SEED, frame_key=keys[f:f + 1], divide_by_std=True,
                                   augment=FULL)
        assert torch.equal(view[0], together[f])
        crop = ops.crops_from_raw(points, offsets, torch.tensor([f], dtype=torch.int32, device="cuda"), 1, N, C, seed=SEED,
                                  frame_key=keys, divide_by_std=True, augment=FULL)
        assert torch.equal(crop[0, 0], together[f])
    other = ops.frames_from_raw(points, offsets, N, C, seed=SEED + 1, frame_key=keys, divide_by_std=True, augment=FULL)
    assert not torch.equal(other, together)


def test_bad_frames_are_zeroed_and_flagged():
    """card 0, card 1025, offsets outside the points, a supplied pick out of range: zeros, the flag, neighbours unchanged"""
    from opensetgaitrecognition_pcaa_amd import ops
    rng = np.random.default_rng(8)
    N, C = 24, 4
    good = [_frame(rng, n) for n in (5, 30, 17, 40, 9)]
    keys = _cuda(np.stack([np.full(7, 2), np.arange(7)], axis=1).astype(np.int32))
    points, offsets = _dev(good, torch.float32)
    clean_picks = torch.full((5, N), -5, dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    clean = ops.frames_from_raw(points, offsets, N, C, seed=1, frame_key=keys[:5], augment=FULL, pick_out=clean_picks,
                                err_flag=err, n_out=8)
    assert err.item() == 0 and clean[:5].abs().sum(dim=(1, 2)).min() > 0 and not clean[5:].any()
    empty = {"cardinality": np.array([0]), "elements": np.zeros((0, 2)), "z_coord": np.zeros(0), "dopplers": np.zeros(0),
             "powers": np.zeros(0)}
    for bad in (empty, _frame(rng, ops.RAW_MAX_CARD + 1)):
        raw = [good[0], bad, good[1], good[2], good[3], good[4]]
        k = keys[[0, 6, 1, 2, 3, 4]].contiguous()
        p, o = _dev(raw, torch.float32)
        for route in ("frames", "unique", "crops"):
            err.zero_()
            if route == "frames":
                pick_out = torch.full((6, N), -5, dtype=torch.int32, device="cuda")
                out = ops.frames_from_raw(p, o, N, C, seed=1, frame_key=k, augment=FULL, pick_out=pick_out, err_flag=err)
                assert (pick_out[1] == -1).all() and torch.equal(pick_out[[0, 2, 3, 4, 5]], clean_picks)
            elif route == "crops":
                out = ops.crops_from_raw(p, o, torch.tensor([0, 3], dtype=torch.int32, device="cuda"), 3, N, C, seed=1,
                                         frame_key=k, augment=FULL, err_flag=err).reshape(6, N, C)
            else:
                rows, weight, u_off = ops.frames_from_raw_unique(p, o, N, C, seed=1, frame_key=k, augment=FULL, err_flag=err)
                u = u_off.cpu().numpy()
                assert err.item() == 1 and u[2] - u[1] == 1 and not rows[u[1]].any() and weight[u[1]].item() == N
                continue
            assert err.item() == 1 and not out[1].any()
            assert torch.equal(out[[0, 2, 3, 4, 5]], clean[:5])
    # a supplied pick outside [0, card)
    for value, frame in ((17, 2), (-1, 4), (2 ** 31 - 1, 0)):
        hp = clean_picks.clone()
        hp[frame, 3] = value
        err.zero_()
        out = ops.frames_from_raw(points, offsets, N, C, pick=hp, seed=1, frame_key=keys[:5], augment=FULL, err_flag=err)
        rest = [f for f in range(5) if f != frame]
        assert err.item() == 1 and not out[frame].any() and torch.equal(out[rest], clean[rest])
    # offsets that leave the points
    err.zero_()
    total = int(_cards(good).sum())
    out = ops.frames_from_raw(points[:total - 2].contiguous(), offsets, N, C, seed=1, frame_key=keys[:5], augment=FULL,
                              err_flag=err)
    assert err.item() == 1 and not out[4].any() and torch.equal(out[:4], clean[:4])
    off = offsets.clone()
    off[0] = -3
    err.zero_()
    out = ops.frames_from_raw(points, off, N, C, seed=1, frame_key=keys[:5], augment=FULL, err_flag=err)
    assert err.item() == 1 and not out[0].any() and torch.equal(out[1:], clean[1:5])


def test_argument_errors_are_refused_before_any_launch():
    from opensetgaitrecognition_pcaa_amd import _lib, ops
    points, offsets = _dev(RAW, torch.float32)
    keys = _cuda(KEYS)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    N = 16
    bad = [{"yaw": -0.1}, {"yaw": 3.2}, {"scale": (0.0, 1.0)}, {"scale": (1.2, 1.1)}, {"speed": (0.0, 1.0)},
           {"speed": (2.0, 1.0)}, {"noise": [-1.0]}, {"noise": [float("inf")]}, {"noise": {"z": float("nan")}}, {"spin": 1}]
    for aug in bad:
        for call in (lambda: ops.frames_from_raw(points, offsets, N, 4, seed=1, frame_key=keys, augment=aug, err_flag=err),
                     lambda: ops.frames_from_raw_unique(points, offsets, N, 4, seed=1, frame_key=keys, augment=aug, err_flag=err),
                     lambda: ops.crops_from_raw(points, offsets, offsets[:1], 2, N, 4, seed=1, frame_key=keys, augment=aug,
                                                err_flag=err)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        ops.frames_from_raw(points, offsets, N, 1, seed=1, frame_key=keys, augment={"yaw": 0.5}, err_flag=err)   # C < 2
    picks = _cuda(datasets.device_picks_host(1, KEYS, CARDS, N))
    with pytest.raises(ValueError):
        ops.frames_from_raw(points, offsets, N, 4, pick=picks, augment=FULL, err_flag=err)                       # no keys
    with pytest.raises(ValueError):
        ops.frames_from_raw(points, offsets, N, 4, pick=picks, frame_key=keys, keep=5, augment=FULL, err_flag=err)
    # the library's own refusals: the same parameters handed to the entry point directly
    lib = _lib.load()
    out = torch.full((len(RAW), N, 4), 7.0, device="cuda")

    def direct(vals, C=4, keep=(0, 0, 0), pick=None, frame_key=keys):
        a = (ctypes.c_double * 11)(*vals)
        return lib.pcaa_frames_from_raw_aug(points.data_ptr(), 0, points.shape[0], offsets.data_ptr(), len(RAW),
                                            None if pick is None else pick.data_ptr(),
                                            None if frame_key is None else frame_key.data_ptr(), 1, N, C, 1, 0,
                                            out.data_ptr(), len(RAW), None, err.data_ptr(), None, *keep, a)

    ok = list(datasets.augment_arguments(FULL))
    pi = float(np.pi)
    for at, value in ((0, -0.1), (0, np.nextafter(pi, 4.0)), (0, float("nan")), (2, 0.0), (2, -1.0), (2, 1.3), (4, 0.0),
                      (4, 1.4), (3, float("inf")), (5, float("nan")), (6, -0.01), (8, float("inf")), (10, float("nan"))):
        vals = list(ok)
        vals[at] = value
        assert direct(vals) != 0, (at, value)
    assert direct(ok, C=1) != 0, "yaw with C < 2"
    assert direct(ok, frame_key=None) != 0 and direct(ok, pick=picks, frame_key=None) != 0
    assert direct(ok, keep=(5, 5, 0), pick=picks) != 0, "picks with keep"
    assert direct(ok, keep=(5, 6, 0)) != 0 and direct(ok, keep=(5, 5, 2)) != 0 and direct(ok, keep=(-1, 0, 0)) != 0
    torch.cuda.synchronize()
    assert err.item() == 0 and (out == 7.0).all(), "nothing was launched"
    no_yaw = list(ok)
    no_yaw[0] = 0.0
    assert direct(no_yaw, C=1) == 0 and direct(ok, pick=picks) == 0 and direct(ok, keep=(5, 5, 1)) == 0
    assert err.item() == 0 and not (out == 7.0).any()
