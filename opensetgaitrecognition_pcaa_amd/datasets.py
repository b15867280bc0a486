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

``SyntheticGaitDataset`` produces mmGait10-shaped crops from a seed; items are
permuted views of point-major ``[T,N,C]`` storage.
"""
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


def frames_from_picks(raw_frames, picks, nfeatures, divide_by_std=False):
    """The arithmetic half of ``process_track`` on given picks (``draw_picks``, ``device_picks_host``, or the ``pick_out``
    of ``ops.frames_from_raw``): powers to dB, the first ``nfeatures`` columns, ``arr[picks[f]]``, per-frame centring
    (and division by ``std + 1e-8``) -> float64 ``[n, nmax, nfeatures]``."""
    picks = np.asarray(picks)
    out = np.empty((len(raw_frames), picks.shape[1], int(nfeatures)), dtype=np.float64)
    for fi, frame in enumerate(raw_frames):
        arr = _raw_columns(frame)
        arr[:, 4] = 10 * np.log10(arr[:, 4] + 1e-8)
        final = arr[:, :nfeatures][picks[fi], :]
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


def device_picks_host(seed, keys, cards, N):
    """What ``pcaa_frames_from_raw`` draws when it is given no picks, restated in numpy, integer for integer -> int32
    ``[n, N]``.  ``keys`` int ``[n, 2]``, ``cards`` ``[n]`` (1 <= card), ``seed`` any Python int (its low 64 bits)."""
    keys = np.asarray(keys).reshape(-1, 2)
    cards = np.asarray(cards).reshape(-1)
    N, seed = int(N), int(seed) & 0xFFFFFFFFFFFFFFFF
    picks = np.empty((cards.size, N), dtype=np.int32)
    s0 = _absorb32(_absorb32(np.uint64(0x9E3779B9), np.uint64(seed & 0xFFFFFFFF)), np.uint64(seed >> 32))
    for fi, card in enumerate(cards.tolist()):
        s = _absorb32(_absorb32(s0, np.uint64(int(keys[fi, 0]) & 0xFFFFFFFF)), np.uint64(int(keys[fi, 1]) & 0xFFFFFFFF))
        if card < N:
            h = _absorb32(s, np.arange(card, N, dtype=np.uint64))
            picks[fi, :card] = np.arange(card)
            picks[fi, card:] = (h * np.uint64(card)) >> np.uint64(32)
        else:
            h = _absorb32(s, np.arange(card, dtype=np.uint64))
            picks[fi] = np.lexsort((np.arange(card), h))[:N]         # rank by (h, i): the N smallest, in key order
    return picks


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
    from sklearn.model_selection import train_test_split
    ls = listdir or (lambda d: sorted(os.listdir(d)))
    nmax_points = constants.NMAX if nmax_points is None else nmax_points
    assert train_ratio + valid_ratio + test_ratio == 1.0
    dirs = {k: os.path.join(constants.GEN_DATA_PATH, k) for k in ("train", "valid", "test", "unseen")}
    for d in dirs.values():
        os.makedirs(d, exist_ok=True)
        for f in os.listdir(d):
            os.remove(os.path.join(d, f))
    train_classes = list(train_classes)
    unseen_classes = np.setdiff1d(list(LABEL_DICT.keys()), train_classes).tolist()
    if not train_classes:
        train_classes = list(LABEL_DICT.keys())

    def emit(pc_file, subj, scenario, target_dir):
        arr = process_track(pc_file, standardize_point_cloud=True, divide_by_std=False,
                            force_pc_subsampling=force_pc_subsampling, nmax=nmax_points)
        crops = crop_with_step(arr, crop_len=constants.NSTEPS, step=constants.CROP_STEP)
        track_index = pc_file.split("/")[-1][5:].split(".")[0]
        for ci in range(len(crops)):
            np.save(os.path.join(target_dir, f"crop{ci}_subj{subj}_{scenario}_track{track_index}.npy"), crops[ci])

    for subj in train_classes:
        subject_dir = os.path.join(constants.DATA_PATH, LABEL_DICT[subj])
        for scenario in ls(subject_dir):
            tracks = ls(os.path.join(subject_dir, scenario))
            if not all(t[:2] == "pc" for t in tracks):
                raise ValueError(f"invalid file in {os.path.join(subject_dir, scenario)}")
            tr, vt = train_test_split(tracks, train_size=train_ratio, random_state=seed)
            va, te = train_test_split(vt, train_size=valid_ratio / (valid_ratio + test_ratio), random_state=seed)
            for group, key in ((tr, "train"), (va, "valid"), (te, "test")):
                for t in group:
                    emit(os.path.join(subject_dir, scenario, t), subj, scenario, dirs[key])
    for subj in unseen_classes:
        subject_dir = os.path.join(constants.DATA_PATH, LABEL_DICT[subj])
        for scenario in ls(subject_dir):
            for t in ls(os.path.join(subject_dir, scenario)):
                emit(os.path.join(subject_dir, scenario, t), subj, scenario, dirs["unseen"])
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
