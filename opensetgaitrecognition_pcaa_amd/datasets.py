"""Batch sources for the PCAA loops.

``MSRadarDataset`` keeps the item contract of the reference's dataset
(``datasets.py:381-482``): crop files ``crop{i}_subj{s}_{scenario}_track{t}.npy``
holding float64 ``[T, N, C]``; ``__getitem__`` -> (``[C,T,N]`` float32, int64
label re-indexed densely over the subjects present).  Difference on purpose:
the file list is sorted (the reference uses raw ``os.listdir`` order, which is
file-system dependent).

Dataset *generation* from raw radar tracks: ``crop_with_step``,
``process_track`` and ``generate_splits`` restate ``datasets.py:16-25, 79-161, 183-379`` with the
SAME calls to numpy's global RNG in the same order, so that under one ``np.random.seed`` the crops are
bit-identical to the reference's (golden: ``tests/golden/datagen.npz``).  Built differently: frames go
into one preallocated array (the reference re-concatenates the whole sequence per frame: O(frames^2))
and the repeat-padding is one fancy-index instead of a Python loop per point.

``RawTrackStore`` / ``RawCrops`` keep the raw tracks themselves, packed once, and list a split's windows as indices: what
``batcher.RawTrackBatcher`` builds training batches from on the device, with no crop files (``split_track_files`` is the
part of ``generate_splits`` that decides which track goes to which split).

``SyntheticGaitDataset`` produces mmGait10-shaped crops from a seed; items are
permuted views of point-major ``[T,N,C]`` storage.
"""
import ctypes
import dataclasses
import math
import os

import numpy as np
import torch

from . import constants
from .constants import SCENARIO, SPLIT


def filename2crop(filename):
    return int(filename.split("_")[0][4:])


def filename2subj(filename):
    return int(filename.split("_")[1][4:])


def filename2track(filename):
    return filename.split("_")[-1][5:].split(".")[0]


def filename2scenario(filename):
    return "_".join(filename.split("_")[2:-1])


def crop_with_step(sequence, crop_len, step):
    """Sliding windows ``sequence[i:i+crop_len]`` for ``i in arange(len - crop_len, step=step)``
    (reference ``datasets.py:16-25``: the window starting at ``len - crop_len`` itself is NOT taken)."""
    idxs = np.arange(len(sequence) - crop_len, step=step)
    if len(idxs) == 0:
        return np.array([])
    return np.stack([sequence[i:i + crop_len] for i in idxs])


def process_track(track, standardize_point_cloud=True, divide_by_std=False, force_pc_subsampling=0,
                  nmax=None, nfeatures=None):
    """Raw track (path of a pickle, or the loaded list of frame dicts) -> ``[n_frames, nmax, nfeatures]``
    float64 (reference ``MSRadarDataset.process_track``, ``datasets.py:79-161``): powers to dB
    (``10 log10(p + 1e-8)``), features ``[x, y, z, doppler, power_dB][:nfeatures]``, repeat-pad with
    ``np.random.choice(card, nmax - card)`` or subsample with ``np.random.choice(card, nmax,
    replace=False)`` (numpy's GLOBAL generator, as there), per-frame centring (and optional division by
    ``std + 1e-8``).  Reference quirk kept: with ``force_pc_subsampling = k`` the frame keeps a random
    ORDER of its FIRST k points (the cardinality is overwritten before ``default_rng(0).choice``, ``:107-115``)."""
    import pickle
    nmax = constants.NMAX if nmax is None else nmax
    nf = constants.NFEATURES if nfeatures is None else nfeatures
    frames = track
    if isinstance(track, (str, os.PathLike)):
        with open(track, "rb") as f:
            frames = pickle.load(f)
    sub_rng = np.random.default_rng(0)
    out = np.empty((len(frames), nmax, nf), dtype=np.float64)
    for fi, frame in enumerate(frames):
        card = int(frame["cardinality"][0])
        elements = frame["elements"]
        zs = frame["z_coord"][:, np.newaxis]
        dop = frame["dopplers"][:, np.newaxis]
        pw = frame["powers"][:, np.newaxis]
        if 0 < force_pc_subsampling < card:
            card = force_pc_subsampling
            keep = sub_rng.choice(card, force_pc_subsampling, replace=False)
            elements, zs, dop, pw = elements[keep], zs[keep], dop[keep], pw[keep]
        pw = 10 * np.log10(pw + 1e-8)
        arr = np.concatenate([elements, zs, dop, pw], axis=1)[:, :nf]
        if card < nmax:
            pick = np.random.choice(card, nmax - card)
            final = np.concatenate([arr, arr[pick]], axis=0)
        else:
            pick = np.random.choice(card, nmax, replace=False)
            final = arr[pick, :]
        if standardize_point_cloud:
            mean = final.mean(axis=0)
            std = final.std(axis=0)
            final = final - mean
            if divide_by_std:
                final = final / (std + 1e-8)
        out[fi] = final
    return out


# ---------------------------------------------------------------------------------------------------------------------
# process_track in two halves -- which raw point goes where (the only part that draws random numbers), and the
# arithmetic on the picked points -- so that the second half can run on the device (ops.frames_from_raw) with the picks
# of the first: draw_picks + frames_from_picks == process_track bit for bit.

def draw_picks(cards, nmax, force_pc_subsampling=0):
    """The picks ``process_track`` makes for frames of the cardinalities ``cards`` -> int32 ``[n, nmax]``: output point p
    of frame f is raw point ``picks[f, p]`` of that frame.  Same calls to numpy's GLOBAL generator (and to
    ``default_rng(0)`` for the forced-subsampling quirk) in the same order as ``process_track``: repeat-pad gives
    ``concat(arange(card), choice(card, nmax - card))``, subsampling ``choice(card, nmax, replace=False)``; with
    ``force_pc_subsampling`` the indices go through ``keep`` so that they address the frame's ORIGINAL points."""
    sub_rng = np.random.default_rng(0)
    cards = np.asarray(cards).reshape(-1)
    picks = np.empty((cards.size, int(nmax)), dtype=np.int32)
    for fi, card in enumerate(cards.tolist()):
        keep = None
        if 0 < force_pc_subsampling < card:
            card = force_pc_subsampling
            keep = sub_rng.choice(card, force_pc_subsampling, replace=False)
        if card < nmax:
            idx = np.concatenate([np.arange(card), np.random.choice(card, nmax - card)])
        else:
            idx = np.random.choice(card, nmax, replace=False)
        picks[fi] = idx if keep is None else keep[idx]
    return picks


def _raw_columns(frame):
    """a raw frame dict -> float64 [card, 5]: x, y, z, doppler, LINEAR power"""
    return np.concatenate([frame["elements"], frame["z_coord"][:, np.newaxis], frame["dopplers"][:, np.newaxis],
                           frame["powers"][:, np.newaxis]], axis=1).astype(np.float64, copy=False)


def augmented_columns(raw_frames, nfeatures, augment=None, seed=0, keys=None):
    """What the frames' detections are before they are picked and centred -> a list with one float64 ``[card,
    nfeatures]`` array per frame: x, y, z, doppler, power in dB, and with ``augment`` (``augment_arguments``; ``seed`` and
    ``keys`` int ``[n, 2]``) moved by the augmentation stage of csrc/raw_frames.hip, restated in fp64 in its order: noise
    by raw index, scale / speed, mirror, rotation; a neutral step is skipped."""
    nfeatures = int(nfeatures)
    aug = augment_arguments(augment, "augmented_columns")
    if aug is not None:
        if keys is None:
            raise ValueError("augmented_columns: augment needs the frames' keys")
        keys = np.asarray(keys).reshape(-1, 2)
        if aug[0] != 0 and nfeatures < 2:
            raise ValueError("augmented_columns: a rotation needs the x and y columns")
        cards = [len(fr["z_coord"]) for fr in raw_frames]
        sigma = np.asarray(aug[6:6 + nfeatures])
        noise = device_noise_host(seed, keys, cards, nfeatures) if sigma.any() else None
        draws = augment_draws_host(seed, keys[:, 0], aug)
    out = []
    for fi, frame in enumerate(raw_frames):
        arr = _raw_columns(frame)
        arr[:, 4] = 10 * np.log10(arr[:, 4] + 1e-8)
        arr = arr[:, :nfeatures]
        if aug is not None:
            for c in range(nfeatures):
                if sigma[c] != 0:
                    arr[:, c] = arr[:, c] + sigma[c] * noise[fi][:, c]
            if not (aug[2] == 1 and aug[3] == 1):
                arr[:, :3] = arr[:, :3] * draws["scale"][fi]
            if nfeatures > 3 and not (aug[4] == 1 and aug[5] == 1):
                arr[:, 3] = arr[:, 3] * draws["speed"][fi]
            if draws["mirror"][fi]:
                arr[:, 0] = -arr[:, 0]
            if aug[0] != 0:
                ct, st = np.cos(draws["yaw"][fi]), np.sin(draws["yaw"][fi])
                x, y = arr[:, 0].copy(), arr[:, 1].copy()
                arr[:, 0] = x * ct - y * st
                arr[:, 1] = x * st + y * ct
        out.append(arr)
    return out


def frames_from_picks(raw_frames, picks, nfeatures, divide_by_std=False, augment=None, seed=0, keys=None):
    """The arithmetic half of ``process_track`` on given picks (``draw_picks``, ``device_picks_host``, or the ``pick_out``
    of ``ops.frames_from_raw``): powers to dB, the first ``nfeatures`` columns, ``arr[picks[f]]``, per-frame centring
    (and division by ``std + 1e-8``) -> float64 ``[n, nmax, nfeatures]``.  ``augment`` with ``seed`` and ``keys``: the
    detections moved first (``augmented_columns``), what the ``augment=`` of ``ops.frames_from_raw`` computes."""
    picks = np.asarray(picks)
    out = np.empty((len(raw_frames), picks.shape[1], int(nfeatures)), dtype=np.float64)
    for fi, arr in enumerate(augmented_columns(raw_frames, nfeatures, augment, seed, keys)):
        final = arr[picks[fi], :]
        mean = final.mean(axis=0)
        std = final.std(axis=0)
        final = final - mean
        if divide_by_std:
            final = final / (std + 1e-8)
        out[fi] = final
    return out


_M32 = np.uint64(0xFFFFFFFF)


def _mix32(x):
    """the 32-bit mixer of csrc/raw_frames.hip ("lowbias32") on uint64 arrays holding 32-bit values"""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    return x ^ (x >> np.uint64(16))


def _absorb32(s, w):
    return _mix32(((s ^ w) + np.uint64(0x9E3779B9)) & _M32)


def _chain_state(seed, key):
    """the chain state of csrc/raw_frames.hip after the words seed_lo, seed_hi, key[0], key[1]"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    s0 = _absorb32(_absorb32(np.uint64(0x9E3779B9), np.uint64(seed & 0xFFFFFFFF)), np.uint64(seed >> 32))
    return _absorb32(_absorb32(s0, np.uint64(int(key[0]) & 0xFFFFFFFF)), np.uint64(int(key[1]) & 0xFFFFFFFF))


_KEEP_WORD = np.uint64(0x6B656570)            # "keep": the tag of the thinning stage's chain
KEEP_RULES = ("first", "random")              # PCAA_RAW_KEEP_FIRST / PCAA_RAW_KEEP_RANDOM of include/pcaa_hip.h


def keep_arguments(keep, keep_min=None, keep_rule="first", who="keep"):
    """The thinning parameters as every raw entry point takes them -> ``(keep, keep_min, rule index)`` ints, (0, 0, 0) for
    no thinning.  ``keep``: 0 / None (off), an int K >= 1, or a pair ``(lo, hi)`` = (keep_min, keep): a count per frame
    drawn in ``lo .. hi``; ``keep_min`` defaults to K; ``keep_rule`` "first" / "random" (or 0 / 1)."""
    if isinstance(keep, (tuple, list)):
        if len(keep) != 2 or keep_min is not None:
            raise ValueError(f"{who}: a range is (lo, hi), without a separate keep_min; got {keep!r}, keep_min={keep_min!r}")
        keep_min, keep = keep
    keep = 0 if keep is None else int(keep)
    rule = KEEP_RULES.index(keep_rule) if keep_rule in KEEP_RULES else keep_rule
    if isinstance(rule, bool) or rule not in (0, 1):
        raise ValueError(f"{who}: keep_rule must be 'first' or 'random', got {keep_rule!r}")
    if keep == 0:
        if keep_min not in (None, 0):
            raise ValueError(f"{who}: keep_min={keep_min!r} without keep")
        return 0, 0, 0
    keep_min = keep if keep_min is None else int(keep_min)
    if not 1 <= keep_min <= keep <= 1024:
        raise ValueError(f"{who}: needs 1 <= keep_min <= keep <= 1024 (a frame's detections), got keep_min={keep_min}, keep={keep}")
    return keep, keep_min, int(rule)


def device_keep_host(seed, keys, cards, keep, keep_min=None, keep_rule="first"):
    """The thinning stage of csrc/raw_frames.hip restated in numpy -> a list with one int array per frame: the raw indices
    it keeps, in the order stage 2 numbers them (``arange(card)`` for a frame it leaves alone: k_f >= card, or keep = 0)."""
    keep, keep_min, rule = keep_arguments(keep, keep_min, keep_rule, "device_keep_host")
    keys = np.asarray(keys).reshape(-1, 2)
    kept = []
    for key, card in zip(keys, np.asarray(cards).reshape(-1).tolist()):
        if keep == 0:
            kept.append(np.arange(card))
            continue
        t = _absorb32(_chain_state(seed, key), _KEEP_WORD)
        k = keep
        if keep_min < keep:
            k = keep_min + ((int(_absorb32(t, np.uint64(0xFFFFFFFF))) * (keep - keep_min + 1)) >> 32)
        if k >= card:
            kept.append(np.arange(card))
        elif rule == 0:
            kept.append(np.arange(k))
        else:
            h = _absorb32(t, np.arange(card, dtype=np.uint64))
            kept.append(np.lexsort((np.arange(card), h))[:k])      # the k smallest (h, i), in rank order
    return kept


def device_picks_host(seed, keys, cards, N, keep=0, keep_min=None, keep_rule="first"):
    """What ``pcaa_frames_from_raw`` draws when it is given no picks, restated in numpy, integer for integer -> int32
    ``[n, N]``.  ``keys`` int ``[n, 2]``, ``cards`` ``[n]`` (1 <= card), ``seed`` any Python int (its low 64 bits).
    ``keep`` / ``keep_min`` / ``keep_rule`` (``keep_arguments``): the draws of the ``_thin`` entry points -- the same draw
    over the ``min(card, k_f)`` detections ``device_keep_host`` keeps, mapped through its lists to raw indices."""
    keys = np.asarray(keys).reshape(-1, 2)
    cards = np.asarray(cards).reshape(-1)
    N = int(N)
    kept = None
    if keep_arguments(keep, keep_min, keep_rule, "device_picks_host")[0]:
        kept = device_keep_host(seed, keys, cards, keep, keep_min, keep_rule)
        cards = np.array([len(k) for k in kept], dtype=np.int64)
    picks = np.empty((cards.size, N), dtype=np.int32)
    for fi, card in enumerate(cards.tolist()):
        s = _chain_state(seed, keys[fi])
        if card < N:
            h = _absorb32(s, np.arange(card, N, dtype=np.uint64))
            picks[fi, :card] = np.arange(card)
            picks[fi, card:] = (h * np.uint64(card)) >> np.uint64(32)
        else:
            h = _absorb32(s, np.arange(card, dtype=np.uint64))
            picks[fi] = np.lexsort((np.arange(card), h))[:N]         # rank by (h, i): the N smallest, in key order
        if kept is not None:
            picks[fi] = kept[fi][picks[fi]]
    return picks


_AUG_WORD = np.uint64(0x6175676D)             # "augm": the tag of a track's augmentation draws
_NOISE_WORD = np.uint64(0x6E6F6973)           # "nois": the tag of a frame's noise chain
AUG_PARAMS = 11                               # PCAA_RAW_AUG_PARAMS of include/pcaa_hip.h: yaw, mirror, scale lo / hi,
AUG_COLUMNS = ("x", "y", "z", "doppler", "power")                           # speed lo / hi, sigma[5] over these columns
_AUG_NEUTRAL = (0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def augment_arguments(augment, who="augment"):
    """The augmentation parameters as every raw entry point takes them -> a tuple of the ``AUG_PARAMS`` doubles of
    ``pcaa_*_aug`` (yaw, mirror, scale_lo, scale_hi, speed_lo, speed_hi, sigma x / y / z / doppler / power), or None when
    every step is neutral (None, an empty dict, or neutral values): the caller then makes the call it makes without
    augmentation.  ``augment`` is a dict with any of ``yaw`` (radians, 0 .. pi: each track is turned by an angle uniform in
    (-yaw, yaw) about the radar's vertical axis), ``mirror`` (bool: each track is mirrored across boresight with
    probability 1/2), ``scale`` and ``speed`` (``(lo, hi)`` or one factor, > 0: x, y, z resp. the Doppler times a factor
    uniform in the range, per track) and ``noise`` (up to 5 sigmas in column order, or a dict over ``AUG_COLUMNS``: Gaussian
    noise per detection, in metres, m/s and dB).  A tuple of ``AUG_PARAMS`` numbers (what this returns) passes through
    the same checks."""
    if augment is None:
        return None
    if isinstance(augment, (tuple, list, np.ndarray)):
        vals = [float(v) for v in np.asarray(augment, dtype=np.float64).reshape(-1)]
        if len(vals) != AUG_PARAMS:
            raise ValueError(f"{who}: the parameter form of augment has {AUG_PARAMS} numbers, got {len(vals)}")
    elif isinstance(augment, dict):
        unknown = set(augment) - {"yaw", "mirror", "scale", "speed", "noise"}
        if unknown:
            raise ValueError(f"{who}: unknown augment keys {sorted(unknown)}; known: yaw, mirror, scale, speed, noise")
        vals = list(_AUG_NEUTRAL)
        vals[0] = float(augment.get("yaw", 0.0))
        vals[1] = 1.0 if augment.get("mirror", False) else 0.0
        for at, name in ((2, "scale"), (4, "speed")):
            r = augment.get(name, 1.0)
            if isinstance(r, (tuple, list, np.ndarray)):
                if len(r) != 2:
                    raise ValueError(f"{who}: {name} is one factor or (lo, hi), got {r!r}")
                vals[at], vals[at + 1] = float(r[0]), float(r[1])
            else:
                vals[at] = vals[at + 1] = float(r)
        noise = augment.get("noise", ())
        if isinstance(noise, dict):
            unknown = set(noise) - set(AUG_COLUMNS)
            if unknown:
                raise ValueError(f"{who}: unknown noise columns {sorted(unknown)}; known: {', '.join(AUG_COLUMNS)}")
            for c, name in enumerate(AUG_COLUMNS):
                vals[6 + c] = float(noise.get(name, 0.0))
        else:
            noise = [float(v) for v in np.asarray(noise, dtype=np.float64).reshape(-1)]
            if len(noise) > 5:
                raise ValueError(f"{who}: noise has at most 5 sigmas ({', '.join(AUG_COLUMNS)}), got {len(noise)}")
            vals[6:6 + len(noise)] = noise
    else:
        raise ValueError(f"{who}: augment is a dict (yaw, mirror, scale, speed, noise) or None, got {type(augment).__name__}")
    yaw, _, s0, s1, v0, v1 = vals[:6]
    if not 0.0 <= yaw <= math.pi:                          # a NaN fails too
        raise ValueError(f"{who}: yaw must lie in [0, pi] radians, got {yaw}")
    for name, lo, hi in (("scale", s0, s1), ("speed", v0, v1)):
        if not (0.0 < lo <= hi and math.isfinite(hi)):
            raise ValueError(f"{who}: {name} needs 0 < lo <= hi, finite; got ({lo}, {hi})")
    if not all(s >= 0.0 and math.isfinite(s) for s in vals[6:]):
        raise ValueError(f"{who}: the noise sigmas must be finite and >= 0, got {vals[6:]}")
    vals[1] = 1.0 if vals[1] != 0.0 else 0.0
    return None if tuple(vals) == _AUG_NEUTRAL else tuple(vals)


@dataclasses.dataclass(frozen=True)
class RawPrep:
    """How a raw frame is prepared on its way to ``[N, C]``, decided once: what every raw route (``ops.frames_from_raw``,
    ``crops_from_raw``, ``frames_from_raw_unique`` and all that call them) takes as ``prep=``, or builds from its keywords.

    ``keep`` (k, or ``(lo, hi)`` for a count drawn per frame; ``keep_min`` = lo) and ``keep_rule`` ("first" / "random"):
    the frame keeps at most that many of its detections before its picks are drawn (the ``_thin`` entry points;
    device-drawn picks only, the picks are raw indices); a frame with no more detections than its count has the bits it
    has without ``keep`` (``keep_arguments``; ``device_picks_host(keep=)`` restates the draw).  ``augment`` (yaw, mirror,
    scale, speed, noise: ``augment_arguments``): the picked detections are moved in fp64 before the frame is centred,
    per track and per detection under the call's seed and frame keys -- which it needs with supplied picks too -- in the
    same launch (the ``_aug`` entry points; ``frames_from_picks(augment=)`` restates it).  Neutral values: the plain call.

    Holds the three thinning ints, the ``AUG_PARAMS`` doubles (None when neutral), and what a call needs of them: the
    entry point's ``suffix`` ("", "_thin", "_aug") and its trailing C arguments ``tail``."""
    keep: int = 0
    keep_min: int = 0
    rule: int = 0
    augment: tuple = None
    suffix: str = ""
    tail: tuple = ()

    @classmethod
    def of(cls, keep=0, keep_min=None, keep_rule="first", augment=None, who="RawPrep", prep=None):
        """The keywords of a raw route normalised (``keep_arguments``, ``augment_arguments``: their errors, under ``who``);
        ``prep``: one built earlier, returned as it is -- then the keywords must be at their defaults."""
        if prep is not None:
            if keep or keep_min is not None or keep_rule != "first" or augment is not None:
                raise ValueError(f"{who}: prep= already says how the frames are prepared; give it or keep / keep_min / "
                                 "keep_rule / augment, not both")
            return prep
        thin = keep_arguments(keep, keep_min, keep_rule, who)
        aug = augment_arguments(augment, who)
        if aug is not None:
            return cls(*thin, aug, "_aug", thin + ((ctypes.c_double * AUG_PARAMS)(*aug),))
        return cls(*thin, None, "_thin", thin) if thin[0] else cls()

    def check(self, who, pick, C):
        """the rules between the preparation and the call it serves (the C library checks them again)"""
        if self.keep and pick is not None:
            raise ValueError(f"{who}: keep thins the frames before the device draws their picks; supplied picks decide by "
                             "themselves (datasets.draw_picks(force_pc_subsampling=k) for the reference's)")
        if self.augment is not None and self.augment[0] != 0 and int(C) < 2:
            raise ValueError(f"{who}: a rotation (yaw) needs the x and y columns, C >= 2; got C={int(C)}")

    def needs_keys(self, pick):
        """whether the frames' keys are read: by the device's own draw of the picks, and by the augmentation's draws"""
        return pick is None or self.augment is not None


def _unit(w):
    """a 32-bit hash word as a number in (0, 1): (w + 0.5) 2^-32, exact in fp64"""
    return (np.asarray(w).astype(np.float64) + 0.5) * 2.0 ** -32


def augment_draws_host(seed, serials, augment):
    """The per-track draws of the augmentation stage of csrc/raw_frames.hip, restated -> a dict of arrays, one entry per
    element of ``serials`` (``key[0]`` of the frames; the frame number is not part of the chain, so all frames of a track
    share them): ``yaw`` (theta, radians), ``mirror`` (bool), ``scale``, ``speed``."""
    aug = augment_arguments(augment, "augment_draws_host") or _AUG_NEUTRAL
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    serials = np.asarray(serials, dtype=np.int64).reshape(-1).astype(np.uint64) & _M32
    s0 = _absorb32(_absorb32(np.uint64(0x9E3779B9), np.uint64(seed & 0xFFFFFFFF)), np.uint64(seed >> 32))
    u = _absorb32(_absorb32(s0, serials), _AUG_WORD)
    w = [_absorb32(u, np.uint64(j)) for j in range(4)]
    r = [_unit(x) for x in w]
    return {"yaw": aug[0] * (2.0 * r[0] - 1.0),
            "mirror": ((w[1] >> np.uint64(31)) != 0) & (aug[1] != 0),
            "scale": aug[2] + (aug[3] - aug[2]) * r[2],
            "speed": aug[4] + (aug[5] - aug[4]) * r[3]}


def device_noise_host(seed, keys, cards, C):
    """The standard normal draws g(i, c) of the augmentation stage, restated -> a list with one float64 ``[card, C]`` array
    per frame: row i belongs to the frame's RAW detection i, whichever padded rows it lands in."""
    keys = np.asarray(keys).reshape(-1, 2)
    out = []
    for key, card in zip(keys, np.asarray(cards).reshape(-1).tolist()):
        q = _absorb32(_absorb32(_chain_state(seed, key), _NOISE_WORD), np.arange(card, dtype=np.uint64))
        g = np.empty((card, int(C)), dtype=np.float64)
        for c in range(int(C)):
            r1, r2 = _unit(_absorb32(q, np.uint64(2 * c))), _unit(_absorb32(q, np.uint64(2 * c + 1)))
            g[:, c] = np.sqrt(-2.0 * np.log(r1)) * np.cos(6.283185307179586 * r2)
        out.append(g)
    return out


def pack_raw_frames(raw_frames, dtype=torch.float32):
    """A list of raw frame dicts -> ``(points [P, 5] dtype, offsets [n + 1] int32)``: the layout ``ops.frames_from_raw``
    and the scorers' ``push_raw`` take -- columns x, y, z, doppler, linear power, frame f in rows ``offsets[f] ..
    offsets[f + 1] - 1``.  Host tensors, pinned where there is a device to copy them to (``.cuda(non_blocking=True)``)."""
    if dtype not in (torch.float32, torch.float64):
        raise TypeError(f"pack_raw_frames: float32 or float64, got {dtype}")
    cards = np.array([len(fr["z_coord"]) for fr in raw_frames], dtype=np.int64)
    total = int(cards.sum())
    if total >= 2 ** 31:
        raise ValueError("pack_raw_frames: the offsets do not fit 32 bits")
    pin = torch.cuda.is_available()
    points = torch.empty((total, 5), dtype=dtype, pin_memory=pin)
    offsets = torch.empty(len(raw_frames) + 1, dtype=torch.int32, pin_memory=pin)
    off = offsets.numpy()
    off[0] = 0
    np.cumsum(cards, out=off[1:])
    if raw_frames:
        pts = points.numpy()
        pts[:, :2] = np.concatenate([fr["elements"] for fr in raw_frames])
        for col, name in ((2, "z_coord"), (3, "dopplers"), (4, "powers")):
            pts[:, col] = np.concatenate([fr[name] for fr in raw_frames])
    return points, offsets


LABEL_DICT = {i: f"target{i}" for i in range(10)}        # reference datasets.py:51-62


def split_track_files(train_classes=(), ratios=(0.8, 0.1, 0.1), seed=0, listdir=None):
    """Which raw track file ``generate_splits`` sends where -> a list of ``(path, subject, scenario, split)`` with split in
    "train" / "valid" / "test" / "unseen", in the order ``generate_splits`` processes them (the order in which it consumes
    numpy's global RNG): per training subject and scenario sklearn's ``train_test_split(random_state=seed)`` twice, then
    every track of the other subjects.  As there, an empty ``train_classes`` trains on all ten subjects AND lists every
    track a second time as unseen (the unseen subjects are worked out before the default is filled in).  Draws nothing from a global generator.  ``listdir`` as in ``generate_splits``."""
    from sklearn.model_selection import train_test_split
    ls = listdir or (lambda d: sorted(os.listdir(d)))
    train_ratio, valid_ratio, test_ratio = ratios
    assert train_ratio + valid_ratio + test_ratio == 1.0
    train_classes = list(train_classes)
    unseen_classes = np.setdiff1d(list(LABEL_DICT.keys()), train_classes).tolist()
    if not train_classes:
        train_classes = list(LABEL_DICT.keys())
    files = []
    for subj in train_classes:
        subject_dir = os.path.join(constants.DATA_PATH, LABEL_DICT[subj])
        for scenario in ls(subject_dir):
            tracks = ls(os.path.join(subject_dir, scenario))
            if not all(t[:2] == "pc" for t in tracks):
                raise ValueError(f"invalid file in {os.path.join(subject_dir, scenario)}")
            tr, vt = train_test_split(tracks, train_size=train_ratio, random_state=seed)
            va, te = train_test_split(vt, train_size=valid_ratio / (valid_ratio + test_ratio), random_state=seed)
            for group, key in ((tr, "train"), (va, "valid"), (te, "test")):
                files += [(os.path.join(subject_dir, scenario, t), subj, scenario, key) for t in group]
    for subj in unseen_classes:
        subject_dir = os.path.join(constants.DATA_PATH, LABEL_DICT[subj])
        for scenario in ls(subject_dir):
            files += [(os.path.join(subject_dir, scenario, t), subj, scenario, "unseen")
                      for t in ls(os.path.join(subject_dir, scenario))]
    return files


def track_file_index(pc_file):
    """the track name ``generate_splits`` puts into a crop's file name: ``.../pc_tr12.obj`` -> ``"12"``"""
    return pc_file.split("/")[-1][5:].split(".")[0]


def epoch_draw_seed(seed, epoch):
    """The seed of the device draws of epoch ``epoch`` under ``RawTrackBatcher(redraw="epoch")``: the words seed_lo,
    seed_hi, epoch absorbed with the mixer of csrc/raw_frames.hip (``_absorb32``) from 0x9e3779b9 -> a 32-bit int."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    s = _absorb32(_absorb32(np.uint64(0x9E3779B9), np.uint64(seed & 0xFFFFFFFF)), np.uint64(seed >> 32))
    return int(_absorb32(s, np.uint64(int(epoch) & 0xFFFFFFFF)))


_JITTER_WORD = np.uint64(0x6A697474)          # "jitt": keeps the phase draws apart from the epoch seed's chain


def jitter_phases(seed, epoch, serials, limits):
    """The phase ``RawTrackBatcher(jitter=True)`` adds to all starts of a track in epoch ``epoch``: for track serial ``r``
    and limit ``m`` (>= 1), ``(uint64(h) * m) >> 32`` with ``h`` = the words seed_lo, seed_hi, epoch, _JITTER_WORD, r
    absorbed with the same mixer -> int64 array in ``[0, m)``."""
    s = _absorb32(np.uint64(epoch_draw_seed(seed, epoch)), _JITTER_WORD)
    h = _absorb32(s, np.asarray(serials, dtype=np.int64).astype(np.uint64) & _M32)
    return ((h * np.asarray(limits, dtype=np.uint64)) >> np.uint64(32)).astype(np.int64)


class RawTrackStore:
    """The raw detections of many tracks, packed once: what training reads instead of crop files.  A track is a list of
    frame dicts (``synthetic.synthetic_raw_track``, the reference's pickles).  Host tensors, pinned where there is a device:

    * ``points`` [P, 5] / ``offsets`` int32 [F + 1]: every frame of every track back to back (``pack_raw_frames``);
    * ``track_first`` int64 [n_tracks + 1]: track i owns store frames ``track_first[i] .. track_first[i + 1] - 1``;
    * per track ``subject``, ``scenario``, ``name`` (what ``generate_splits`` writes after ``_track``), ``serial``
      (default: its index) and ``split`` (a ``SPLIT`` value or None), the latter set by ``assign``;
    * ``frame_key`` int32 [F, 2] = (serial, frame in track), as ``frame_table.frame_keys`` forms it: the keys under which
      ``embed_raw_track(track_key=serial)`` / ``push_raw`` draw the same frames' picks.

    ``to_device`` uploads the tables once; ``crops`` lists a split's windows for ``batcher.RawTrackBatcher``."""

    def __init__(self, tracks, subjects, scenarios, names, splits=None, serials=None, dtype=torch.float32):
        n = len(tracks)
        if not (len(subjects) == len(scenarios) == len(names) == n):
            raise ValueError("RawTrackStore: one subject, scenario and name per track")
        self.subject = [int(s) for s in subjects]
        self.scenario = [getattr(s, "value", s) for s in scenarios]
        self.name = [str(t) for t in names]
        self.serial = np.arange(n, dtype=np.int64) if serials is None else np.asarray(serials, dtype=np.int64)
        if self.serial.shape != (n,) or (n and (self.serial.min() < -2 ** 31 or self.serial.max() >= 2 ** 31)):
            raise ValueError("RawTrackStore: one serial per track, each an int32 (it is a word of the frames' draw keys)")
        self.split = [None] * n
        lengths = np.array([len(t) for t in tracks], dtype=np.int64)
        self.track_first = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        if int(self.track_first[-1]) >= 2 ** 31:
            raise ValueError("RawTrackStore: the frame indices do not fit 32 bits")
        self.points, self.offsets = pack_raw_frames([fr for t in tracks for fr in t], dtype)
        F = int(self.track_first[-1])
        self.frame_key = torch.empty((F, 2), dtype=torch.int32, pin_memory=torch.cuda.is_available())
        k = self.frame_key.numpy()
        k[:, 0] = np.repeat(self.serial, lengths).astype(np.int32)
        k[:, 1] = (np.arange(F, dtype=np.int64) - np.repeat(self.track_first[:-1], lengths)).astype(np.int32)
        self.device = None
        self.points_dev = self.offsets_dev = self.frame_key_dev = None
        if splits is not None:
            self.assign(splits)

    @classmethod
    def from_files(cls, files, dtype=torch.float32):
        """From the list ``split_track_files`` returns: every pickle is read once, the splits are assigned."""
        import pickle
        tracks = []
        for path, _, _, _ in files:
            with open(path, "rb") as f:
                tracks.append(pickle.load(f))
        return cls(tracks, [f[1] for f in files], [f[2] for f in files], [track_file_index(f[0]) for f in files],
                   splits=[f[3] for f in files], dtype=dtype)

    # ------------------------------------------------------------------------------------------------ split assignment
    def path(self, i):
        """where ``generate_splits`` would look for track i under ``constants.DATA_PATH``"""
        return os.path.join(constants.DATA_PATH, LABEL_DICT[self.subject[i]], self.scenario[i], f"pc_tr{self.name[i]}.obj")

    def listdir(self, d):
        """``listdir`` for ``split_track_files`` over the tracks held here (no file system): sorted names"""
        names = set()
        for i in range(len(self.name)):
            rel = os.path.relpath(self.path(i), d)
            if not rel.startswith(os.pardir):
                names.add(rel.split(os.sep)[0])
        return sorted(names)

    def assign(self, splits):
        """Set every track's split: a list with one "train" / "valid" / "test" / "unseen" / ``SPLIT`` / None per track, or
        the list of ``split_track_files`` (matched by path; tracks it does not name get None; a track it names twice keeps
        the first split).  -> self"""
        splits = list(splits)
        if splits and isinstance(splits[0], tuple):
            by_path = {}
            for f in splits:
                by_path.setdefault(f[0], f[3])           # listed twice (empty train_classes: also as unseen): the first
            splits = [by_path.get(self.path(i)) for i in range(len(self.name))]
        if len(splits) != len(self.name):
            raise ValueError("RawTrackStore.assign: one split per track")
        self.split = [None if s is None else SPLIT(getattr(s, "value", s)) for s in splits]
        return self

    def assign_like_generate_splits(self, train_classes=(), ratios=(0.8, 0.1, 0.1), seed=0):
        """the assignment ``generate_splits(train_classes, *ratios, seed)`` makes for these tracks"""
        return self.assign(split_track_files(train_classes, ratios, seed, listdir=self.listdir))

    # ---------------------------------------------------------------------------------------------------------- device
    def to_device(self, device="cuda"):
        """Upload points, offsets and frame keys once (pinned sources, one copy each).  -> self"""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("RawTrackStore.to_device: batches are built on the HIP device; there is no CPU path")
        if self.device != device:
            self.points_dev = self.points.to(device, non_blocking=True)
            self.offsets_dev = self.offsets.to(device, non_blocking=True)
            self.frame_key_dev = self.frame_key.to(device, non_blocking=True)
            self.device = device
        return self

    @property
    def n_frames(self):
        return int(self.track_first[-1])

    def cards(self):
        """detections per store frame, int64 [F]"""
        return np.diff(self.offsets.numpy().astype(np.int64))

    def crops(self, split, N=None, C=None, hop=None, order="filenames", T=None, scenarios=None):
        """The crops of the split's tracks -> :class:`RawCrops` (see there)."""
        return RawCrops(self, split, N, C, hop, order, T, scenarios)


class RawCrops:
    """The windows ``generate_splits`` would have cut from the tracks of one split of a :class:`RawTrackStore`, as indices:
    per track of F frames the starts ``range(0, F - T, hop)`` (``frame_table.track_windows``: the reference's count; a
    track with ``F <= T`` has none), ``N`` points per frame and the first ``C`` features.  Per crop: ``track`` (index into
    the store), ``crop`` (index in its track), ``start`` (store frame of its first frame), ``filenames`` (the name
    ``generate_splits`` would have written), ``original_labels`` and ``labels`` (dense over the subjects present, as
    ``MSRadarDataset``); per listed track ``slack`` = F - T - hop (count - 1) >= 1, the room ``RawTrackBatcher``'s jitter has.
    ``order="filenames"``: sorted by file name, the item order of ``MSRadarDataset(split)``; ``"sequential"``: by
    (subject, track name, crop) on top of it, the order of ``MSRadarDataset(split, sequential=True)``.  ``scenarios``
    (default ``constants.TRAIN_SCENARIOS``) filters as there.  Nothing here touches the device."""

    def __init__(self, store, split, N=None, C=None, hop=None, order="filenames", T=None, scenarios=None):
        from .frame_table import track_windows
        if order not in ("filenames", "sequential"):
            raise ValueError(f"RawCrops: order must be 'filenames' or 'sequential', got {order!r}")
        self.store, self.split, self.order = store, SPLIT(getattr(split, "value", split)), order
        self.N = constants.NMAX if N is None else int(N)
        self.C = constants.NFEATURES if C is None else int(C)
        self.T = constants.NSTEPS if T is None else int(T)
        self.hop = constants.CROP_STEP if hop is None else int(hop)
        wanted = {getattr(s, "value", s) for s in (constants.TRAIN_SCENARIOS if scenarios is None else scenarios)}
        items = []                                        # (file name, track, crop)
        for i, sp in enumerate(store.split):
            if sp != self.split or store.scenario[i] not in wanted:
                continue
            W, _ = track_windows(int(store.track_first[i + 1] - store.track_first[i]), self.T, self.hop)
            items += [(f"crop{ci}_subj{store.subject[i]}_{store.scenario[i]}_track{store.name[i]}.npy", i, ci)
                      for ci in range(W)]
        items.sort(key=lambda it: it[0])
        if order == "sequential":
            items.sort(key=lambda it: (filename2subj(it[0]), filename2track(it[0]), filename2crop(it[0])))
        self.filenames = [it[0] for it in items]
        self.track = np.array([it[1] for it in items], dtype=np.int64)
        self.crop = np.array([it[2] for it in items], dtype=np.int64)
        self.start = store.track_first[self.track] + self.hop * self.crop if items else np.zeros(0, np.int64)
        self.original_labels = [store.subject[i] for i in self.track]
        dense = {c: i for i, c in enumerate(sorted(set(self.original_labels)))}
        self.labels = np.array([dense[j] for j in self.original_labels], dtype=np.int64)
        length = store.track_first[self.track + 1] - store.track_first[self.track] if items else np.zeros(0, np.int64)
        count = np.array([track_windows(int(n), self.T, self.hop)[0] for n in length], dtype=np.int64)
        self.slack = length - self.T - self.hop * (count - 1)             # per crop: its track's
        # seed / redraw / jitter / picks / keep_points / keep_rule of the RawTrackBatcher that batcher_for builds
        self.batcher_options = {}

    def __len__(self):
        return len(self.filenames)

    def starts(self, seed=0, epoch=0, jitter=False):
        """store frame of every crop's first frame, int32 [M]; with ``jitter`` each track's starts are shifted by its phase
        of (seed, epoch, serial) in ``[0, min(hop, slack))`` (``jitter_phases``): every window stays inside its track"""
        start = self.start
        if jitter and len(self):
            start = start + jitter_phases(seed, epoch, self.store.serial[self.track], np.minimum(self.hop, self.slack))
        return start.astype(np.int32)

    def materialize(self, seed=0, picks=None, epoch=0, jitter=False, keep_points=0, keep_rule="first", augment=None,
                    prep=None):
        """All crops written out by the batch kernel, one launch -> ``(pcs [M, C, T, N] view of point-major storage,
        labels int64 [M])`` on the store's device: what the evaluation procedures take.  ``keep_points`` / ``keep_rule`` /
        ``augment``, or ``prep`` built from them: how every frame is prepared (:class:`RawPrep`), drawn under ``seed``."""
        from . import ops
        st = self.store
        if st.device is None:
            raise RuntimeError("RawCrops.materialize: call store.to_device() first; there is no CPU path")
        if not len(self):
            raise ValueError(f"RawCrops.materialize: the {self.split.value} split has no crops")
        err = torch.zeros(1, dtype=torch.int32, device=st.device)
        start = torch.from_numpy(self.starts(seed, epoch, jitter)).to(st.device)
        pm = ops.crops_from_raw(st.points_dev, st.offsets_dev, start, self.T, self.N, self.C, pick=picks, seed=seed,
                                frame_key=st.frame_key_dev, err_flag=err, keep=keep_points, keep_rule=keep_rule,
                                augment=augment, prep=prep)
        if int(err.item()):
            raise ValueError("RawCrops.materialize: a frame of the store cannot be processed (no detections, more than "
                             f"{ops.RAW_MAX_CARD}, or a pick outside its frame)")
        return pm.permute(0, 3, 1, 2), torch.from_numpy(self.labels).to(st.device)


def generate_splits(train_classes=(), train_ratio=0.8, valid_ratio=0.1, test_ratio=0.1, seed=0,
                    force_pc_subsampling=0, nmax_points=None, listdir=None, verbose=True):
    """Train/valid/test/unseen crop files under ``constants.GEN_DATA_PATH`` from the raw tracks under
    ``constants.DATA_PATH/target<i>/<scenario>/pc_tr*.obj`` (reference ``generate_splits``,
    ``datasets.py:183-379``): per subject and scenario the tracks are split with sklearn's
    ``train_test_split(random_state=seed)`` twice, every track goes through ``process_track``
    (centred, not divided by std) and ``crop_with_step(NSTEPS, CROP_STEP)``, crops are saved as
    ``crop{i}_subj{s}_{scenario}_track{t}.npy`` (float64 ``[T,N,C]``).  ``listdir`` (default: sorted
    ``os.listdir``) fixes the traversal order and with it the consumption of numpy's global RNG; the
    reference uses raw ``os.listdir`` (file-system order) and asks for ENTER first (``safe_mode``)."""
    nmax_points = constants.NMAX if nmax_points is None else nmax_points
    assert train_ratio + valid_ratio + test_ratio == 1.0
    dirs = {k: os.path.join(constants.GEN_DATA_PATH, k) for k in ("train", "valid", "test", "unseen")}
    for d in dirs.values():
        os.makedirs(d, exist_ok=True)
        for f in os.listdir(d):
            os.remove(os.path.join(d, f))
    train_classes = list(train_classes)
    files = split_track_files(train_classes, (train_ratio, valid_ratio, test_ratio), seed, listdir)   # (the classes as given)
    unseen_classes = np.setdiff1d(list(LABEL_DICT.keys()), train_classes).tolist()
    if not train_classes:
        train_classes = list(LABEL_DICT.keys())

    for pc_file, subj, scenario, key in files:
        arr = process_track(pc_file, standardize_point_cloud=True, divide_by_std=False,
                            force_pc_subsampling=force_pc_subsampling, nmax=nmax_points)
        crops = crop_with_step(arr, crop_len=constants.NSTEPS, step=constants.CROP_STEP)
        for ci in range(len(crops)):
            np.save(os.path.join(dirs[key], f"crop{ci}_subj{subj}_{scenario}_track{track_file_index(pc_file)}.npy"), crops[ci])
    stats = {k: len(os.listdir(d)) for k, d in dirs.items()}
    if verbose:
        from .utils import openness
        print(f"-> sizes {stats}; training classes {train_classes}; unseen {unseen_classes}; "
              f"openness {openness(len(train_classes), len(LABEL_DICT)) * 100:.3f}%")
    return stats


class MSRadarDataset(torch.utils.data.Dataset):
    label_dict = LABEL_DICT
    process_track = staticmethod(process_track)
    generate_splits = staticmethod(generate_splits)

    def __init__(self, split: SPLIT, scenarios=None, sequential=False, subsample_factor=1.0):
        scenarios = constants.TRAIN_SCENARIOS if scenarios is None else scenarios
        self.dataset_dir = os.path.join(constants.GEN_DATA_PATH, split.value)
        self.sequential = sequential
        names = sorted(os.listdir(self.dataset_dir))
        if sequential:
            # group by (subject, track), crops in temporal order
            names.sort(key=lambda f: (filename2subj(f), filename2track(f), filename2crop(f)))
        wanted = {s.value for s in scenarios}
        names = [f for f in names if filename2scenario(f) in wanted]
        if subsample_factor < 1.0:
            names = list(np.random.choice(names, int(len(names) * subsample_factor), replace=False))
        self.filenames = names
        self.original_labels = [filename2subj(f) for f in names]
        dense = {c: i for i, c in enumerate(sorted(set(self.original_labels)))}
        self.labels = np.array([dense[j] for j in self.original_labels], dtype=np.int64)

    def __len__(self):
        return len(self.filenames)

    def __getitem__(self, idx):
        arr = np.load(os.path.join(self.dataset_dir, self.filenames[idx]), allow_pickle=True)
        pc_seq = torch.from_numpy(arr).to(torch.float)      # [T, N, C] point-major
        return pc_seq.permute(2, 0, 1), torch.tensor(self.labels[idx]).type(torch.LongTensor)


class SyntheticGaitDataset(torch.utils.data.Dataset):
    """``n_items`` random crops [T,N,C] (per-frame centred), labels uniform in [0,K)."""

    def __init__(self, n_items, K, N=None, C=None, T=None, seed=0):
        from .synthetic import synthetic_labels, synthetic_pcs
        N = constants.NMAX if N is None else N
        C = constants.NFEATURES if C is None else C
        T = constants.NSTEPS if T is None else T
        self.pcs = synthetic_pcs(n_items, T, N, C, seed=seed)          # [M,T,N,C]
        self.labels = synthetic_labels(n_items, K, seed=seed + 1)

    def __len__(self):
        return self.pcs.shape[0]

    def __getitem__(self, idx):
        return self.pcs[idx].permute(2, 0, 1), self.labels[idx]
