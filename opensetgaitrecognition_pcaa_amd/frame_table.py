"""The host-side rules that every route from frames to a frame-feature table to windows shares (the scorers of
inference.py, the track routes of functional.py, adapt.py), each written once: which windows a track has, where they start
in the table of several tracks, how a chunk of frames is padded to whole GEMM row tiles, what the entry points refuse, how
raw detections become frames.  No autograd, no kernel sequencing beyond the two ``ops`` calls ``raw_frames`` chooses between."""
import collections

import numpy as np
import torch

from . import constants, ops


# ---------------------------------------------------------------------------------------------------- the window rule
def eager_window_count(n_frames, T, hop):
    """Windows of T frames, one every ``hop``, that n_frames frames hold: ``0 if n < T else (n - T) // hop + 1``, on a Python
    int (plain arithmetic: every live push calls it) or elementwise on an integer array.  The live scorers emit by this rule."""
    w = (n_frames - T) // hop + 1
    return w * (w > 0)


def track_windows(n_frames, T=constants.NSTEPS, hop=constants.CROP_STEP, drop_last_aligned=True):
    """-> (W, U): the windows of a track of ``n_frames`` frames and the frames they use.  The reference's ``crop_with_step``
    (datasets.py:16-25, 297-302: a crop per start in ``arange(n_frames - T, step=hop)``) drops the last aligned window when
    ``(n_frames - T) % hop == 0``: the eager count of a track one frame shorter; ``drop_last_aligned=False``: the eager count."""
    n_frames, T, hop = int(n_frames), int(T), int(hop)
    if hop < 1:
        raise ValueError(f"track_windows: hop must be >= 1, got {hop}")
    W = eager_window_count(n_frames - bool(drop_last_aligned), T, hop)
    return W, ((W - 1) * hop + T if W else 0)


TrackPlan = collections.namedtuple("TrackPlan", "counts used starts U")


def plan_track_windows(n_frames, T, hop, drop_last_aligned=True, who="plan_track_windows", allow_empty=False):
    """Tracks of ``n_frames[i]`` frames -> per track its windows ``counts[i]`` and the frames they use ``used[i]``; ``starts``
    int64 [sum counts]: every window's first row in the table of the tracks' used frames back to back (a window never leaves
    its track's rows); ``U``: that table's rows.  A track without a window: ValueError, unless ``allow_empty`` (the scorers)."""
    counts, used = [], []
    for i, n in enumerate(n_frames):
        W, U = track_windows(n, T, hop, drop_last_aligned)
        if W == 0 and not allow_empty:
            raise ValueError(f"{who}: track {i} of {int(n)} frames has no window of {int(T)} frames (hop {int(hop)})")
        counts.append(W)
        used.append(U)
    base = np.cumsum([0] + used)
    starts = [b + int(hop) * np.arange(W, dtype=np.int64) for b, W in zip(base, counts)]
    return TrackPlan(counts, used, np.concatenate(starts) if starts else np.zeros(0, np.int64), int(base[-1]))


# --------------------------------------------------------------------------------------------------- the padding rule
def pad_chunk(src, a, b, q):
    """Frames a .. b - 1 of ``src`` [F, ...] in a chunk of a multiple of ``q`` frames (``functional.frame_pad_quantum``: whole
    GEMM row tiles) -> ``(chunk, lo)``, ``chunk[lo:lo + b - a]`` the frames asked for (the caller drops the others' features).
    The padding: neighbouring frames of ``src`` -- the trailing ones, else the leading ones: a view -- else zeros (one ``cat``)."""
    pad = (a - b) % q
    if b + pad <= src.shape[0]:
        return src[a:b + pad], 0
    if a >= pad:
        return src[a - pad:b], pad
    return torch.cat([src[a:b], src.new_zeros((pad,) + tuple(src.shape[1:]))]), 0


def join_rows(parts):
    """the chunks of a table -> the table (no copy when there is one chunk)"""
    return parts[0] if len(parts) == 1 else torch.cat(parts)


# ------------------------------------------------------------------------------------------------------- the refusals
def _on_device(t, who, name, empty_ok=True):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{who}: {name} must live on the HIP device; this package has no CPU path")
    if not empty_ok and t.numel() == 0:
        raise ValueError(f"{who}: empty {name} {tuple(t.shape)}")


def check_frames(frames, who, empty_ok=True):
    """what every entry point that takes frames refuses: a host tensor, anything but contiguous fp32 [n,N,C]"""
    _on_device(frames, who, "frames", empty_ok)
    if frames.dim() != 3 or frames.dtype != torch.float32 or not frames.is_contiguous():
        raise ValueError(f"{who} expects contiguous fp32 [n,N,C], got {tuple(frames.shape)} {frames.dtype}")


def check_crops(pcs, who, empty_ok=True):
    """what every entry point that takes crops refuses: a host tensor, anything but [M,C,T,N]"""
    _on_device(pcs, who, "input", empty_ok)
    if pcs.dim() != 4:
        raise ValueError(f"{who} expects [B,C,T,N], got {tuple(pcs.shape)}")


def check_raw(points, offsets, pick, N, who):
    """what every entry point that takes raw detections refuses before it touches its state -> the number of frames"""
    _on_device(points, who, "points")
    _on_device(offsets, who, "offsets")
    if points.dim() != 2 or points.shape[1] != 5 or points.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{who} expects points fp32 or fp64 [P,5], got {tuple(points.shape)} {points.dtype}")
    if offsets.dim() != 1 or offsets.dtype != torch.int32 or offsets.numel() < 1:
        raise ValueError(f"{who} expects offsets int32 [n + 1], got {tuple(offsets.shape)} {offsets.dtype}")
    n = offsets.numel() - 1
    if pick is not None:
        _on_device(pick, who, "pick")
        if pick.dtype != torch.int32 or tuple(pick.shape) != (n, N):
            raise ValueError(f"{who} expects pick int32 [{n}, {N}], got {tuple(pick.shape)} {pick.dtype}")
    return n


def check_ragged(rows, weight, u_off, n, N, who):
    """what the entry points that take a compact table refuse: ``rows`` contiguous fp32 [M, C] (not empty), ``weight``
    fp32 [M], ``u_off`` int32 [n + 1], all on the device -> (M, C)"""
    _on_device(rows, who, "rows", empty_ok=False)
    if rows.dim() != 2 or rows.dtype != torch.float32 or not rows.is_contiguous():
        raise ValueError(f"{who} expects contiguous fp32 rows [M,C], got {tuple(rows.shape)} {rows.dtype}")
    M, C = rows.shape
    _on_device(weight, who, "weight")
    _on_device(u_off, who, "u_off")
    if weight.dtype != torch.float32 or tuple(weight.shape) != (M,):
        raise ValueError(f"{who}: weight must be fp32 [{M}], got {tuple(weight.shape)} {weight.dtype}")
    if u_off.dtype != torch.int32 or tuple(u_off.shape) != (int(n) + 1,):
        raise ValueError(f"{who}: u_off must be int32 [{int(n) + 1}], got {tuple(u_off.shape)} {u_off.dtype}")
    return M, C


# ------------------------------------------------------------------------------------------------------ raw detections
def frame_keys(serial, first, n, dev):
    """the keys (track serial, frame index) of frames first .. first + n - 1 of one track, under which their picks are
    drawn on the device: int32 [n, 2], one pinned copy that the host does not wait for"""
    host = torch.empty((n, 2), dtype=torch.int32, pin_memory=True)
    k = host.numpy()
    k[:, 0] = np.int64(serial).astype(np.int32)
    k[:, 1] = (np.arange(n, dtype=np.int64) + int(first)).astype(np.int32)
    return host.to(dev, non_blocking=True)


def raw_frames(points, offsets, N, C, pick, seed, keys, err_flag, a=0, b=None, dedup_points=False, n_out=None, prep=None):
    """Raw detections -> the padded frames [n_out or n, N, C] (``ops.frames_from_raw``) or, with ``dedup_points``, their
    distinct points ``(rows, weight, u_off)`` (``ops.frames_from_raw_unique``), one launch.  ``b``: of frames a .. b - 1 only
    (``offsets``, ``pick``, ``keys``: the whole track's).  ``err_flag``, the caller's, is set by a frame that cannot be processed.
    ``prep`` (``datasets.RawPrep``; None: the frames as they are): how the scorers' frames are thinned and moved first."""
    if b is not None:
        offsets = offsets[a:b + 1]
        pick = None if pick is None else pick[a:b]
        keys = None if keys is None else keys[a:b]
    if dedup_points:
        return ops.frames_from_raw_unique(points, offsets, N, C, pick=pick, seed=seed, frame_key=keys, err_flag=err_flag,
                                          prep=prep)
    return ops.frames_from_raw(points, offsets, N, C, pick=pick, seed=seed, frame_key=keys, n_out=n_out, err_flag=err_flag,
                               prep=prep)
