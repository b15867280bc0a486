"""Deterministic synthetic inputs and weight fills shared by tests, bench and
the golden-vector generator.

Everything here is numpy ``default_rng`` based so that the GPU box can
regenerate bit-identical weights and batches from a seed: decoder weights are
39 MB - 2.5 GB, so fixtures carry seed + formula + outputs, never weights.
"""
import math

import numpy as np
import torch


_BIG_FILLS = {}                      # (shape, seed, index) -> array, insertion-ordered: oldest evicted first
_BIG_FILL_MIN = 1 << 22              # floats
import os as _os

# floats kept in total (default 4 GB of host memory per process; PCAA_FILL_CACHE_FLOATS=0 turns the cache off, e.g. in
# the rank processes of a multi-GPU bench)
_BIG_FILL_BUDGET = int(_os.environ.get("PCAA_FILL_CACHE_FLOATS", 1 << 30))


def fill_tensor_like(name: str, shape, seed: int, index: int) -> np.ndarray:
    """Documented fill formula.  ``index`` is the position in state_dict order.

    * ``num_batches_tracked``            -> 0
    * ``running_var``                    -> U(0.5, 1.5)
    * ``running_mean``                   -> 0.1 * N(0,1)
    * 1-D ``weight`` (BatchNorm gamma)   -> 1 + 0.1 * N(0,1)
    * 1-D ``bias``                       -> 0.05 * N(0,1)
    * >=2-D ``weight``                   -> N(0,1) / sqrt(fan_in), fan_in = prod(shape[1:])
    """
    rng = np.random.default_rng([int(seed), int(index)])
    shape = tuple(int(s) for s in shape)
    if name.endswith("num_batches_tracked"):
        return np.zeros(shape, dtype=np.int64)
    if name.endswith("running_var"):
        return (0.5 + rng.random(shape)).astype(np.float32)
    if name.endswith("running_mean"):
        return (0.1 * rng.standard_normal(shape)).astype(np.float32)
    if len(shape) == 1:
        if name.endswith("weight"):
            return (1.0 + 0.1 * rng.standard_normal(shape)).astype(np.float32)
        return (0.05 * rng.standard_normal(shape)).astype(np.float32)
    fan_in = int(np.prod(shape[1:]))
    key = (shape, int(seed), int(index))
    hit = _BIG_FILLS.get(key)
    if hit is not None:
        return hit
    out = rng.standard_normal(shape, dtype=np.float32)
    out *= np.float32(1.0 / math.sqrt(fan_in))
    n = out.size
    if n >= _BIG_FILL_MIN and n <= _BIG_FILL_BUDGET:
        # the wide decoder matrices (up to 470 M floats, seconds of draws each) are asked for again and again by tests and
        # bench legs that build the same architecture from the same seeds: keep the most recent ones -- READ-ONLY: the array
        # itself is handed out again, so an in-place edit by one caller would corrupt every later fill (numpy enforces it)
        out.setflags(write=False)
        _BIG_FILLS[key] = out
        while sum(v.size for v in _BIG_FILLS.values()) > _BIG_FILL_BUDGET and len(_BIG_FILLS) > 1:
            _BIG_FILLS.pop(next(iter(_BIG_FILLS)))
    return out


@torch.no_grad()
def deterministic_fill_(module_or_state_dict, seed: int):
    """In-place fill of every entry of a module's ``state_dict`` (reference
    modules and this package's drop-in modules share key order, so the same
    seed gives the same weights on both sides)."""
    sd = module_or_state_dict
    if isinstance(sd, torch.nn.Module):
        sd = sd.state_dict()
    import warnings
    for i, (name, t) in enumerate(sd.items()):
        v = fill_tensor_like(name, t.shape, seed, i)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)       # (cached fills are read-only arrays; they are only read here)
            src = torch.from_numpy(v)
        t.copy_(src.to(t.dtype).reshape(t.shape))
    return module_or_state_dict


FEATURE_SCALE = (1.0, 1.0, 0.5, 1.0, 10.0)


def synthetic_pcs(B, T, N, C, seed=1234) -> torch.Tensor:
    """Point-major ``[B,T,N,C]`` float32 batch: standard normal, scaled per
    feature, centred per frame over the N points (mimics the reference's
    per-frame centring, ``datasets.py:142-146``).  Modules consume the
    zero-copy ``permute(0,3,1,2)`` view ``[B,C,T,N]``."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, N, C), dtype=np.float32)
    x *= np.asarray(FEATURE_SCALE[:C], dtype=np.float32)
    x -= x.mean(axis=2, keepdims=True)
    return torch.from_numpy(x)


def synthetic_labels(B, K, seed=1235) -> torch.Tensor:
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(0, K, size=(B,), dtype=np.int64))


def synthetic_z0(B, D=32, seed=1236) -> torch.Tensor:
    """Stand-in for the reference's host ``np.random.normal`` draw
    (``PCAA_ablation.py:915-925``): float64 normal cast to float32."""
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.normal(0.0, 1.0, (B, D))).float()


def synthetic_alphas(B, seed=1237) -> torch.Tensor:
    """Stand-in for ``torch.rand((B,1))`` (``PCAA_ablation.py:944``)."""
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.random((B, 1), dtype=np.float32))


def checksum(t: torch.Tensor, nsample: int = 16) -> dict:
    """sum / L2 / first-and-strided samples of a tensor, float64."""
    f = t.detach().double().reshape(-1).cpu()
    n = f.numel()
    k = min(nsample, n)
    idx = (torch.arange(k, dtype=torch.int64) * (n - 1)) // max(k - 1, 1)
    return {
        "sum": float(f.sum()),
        "l2": float(f.norm()),
        "samples": f[idx].numpy().copy(),
        "sample_idx": idx.numpy().copy(),
    }


def synthetic_raw_track(seed: int, n_frames: int, max_points: int = 40) -> list:
    """A raw radar track in the reference's on-disk format (``datasets.py:95-103``: a pickled list of
    per-frame dicts ``cardinality [1]``, ``elements [n,2]``, ``z_coord [n]``, ``dopplers [n]``,
    ``powers [n]`` (linear, positive)), with per-frame cardinalities on both sides of typical NMAX values."""
    rng = np.random.default_rng(seed)
    frames = []
    for _ in range(n_frames):
        n = int(rng.integers(3, max_points + 1))
        frames.append({
            "cardinality": np.array([n]),
            "elements": rng.standard_normal((n, 2)) * 0.4 + rng.standard_normal(2),
            "z_coord": rng.standard_normal(n) * 0.5 + 1.0,
            "dopplers": rng.standard_normal(n) * 0.8,
            "powers": np.exp(rng.standard_normal(n) * 1.5),
        })
    return frames


def _as_raw_frame(p):
    """rows (x, y, z, doppler, power) -> a raw frame dict of ``synthetic_raw_track``'s format"""
    return {"cardinality": np.array([len(p)]), "elements": p[:, :2].copy(), "z_coord": p[:, 2].copy(),
            "dopplers": p[:, 3].copy(), "powers": p[:, 4].copy()}


def synthetic_scene(seed: int, n_frames: int, people, clutter: int, eps: float, z_weight: float = 0.1,
                    doppler_weight: float = 0.0, min_card: int = 8, max_card: int = 20):
    """Scene frames for ``scene.SceneSplitter`` with the people that went into them -> ``(scene, persons)``: ``scene`` a
    list of ``n_frames`` raw frame dicts (the format of ``synthetic_raw_track``), ``persons[k]`` a list of ``n_frames``
    entries, person k's own frame dict or None where they are not in view.  ``people``: their number, or a list of
    ``(first, last)`` frame spans (``last`` exclusive).  Under the metric ``dx^2 + dy^2 + z_weight dz^2 + doppler_weight
    dv^2``:

    * person k walks along x at constant velocity (0.05 - 0.15 m per frame) in a lane of their own, the lanes ``3.5 eps``
      apart: centres stay >= 3 eps apart;
    * a person's ``min_card .. max_card`` detections lie inside a ball of radius ``eps / 2`` around the centre (drawn
      within ``0.49 eps``, so that rounding to fp32 keeps them inside): all of them within ``eps`` of each other, one
      cluster whatever ``min_points <= min_card``;
    * ``clutter`` detections per frame sit on a lattice of pitch ``2 eps`` at least ``3 eps`` from every lane: isolated by
      more than ``eps`` from everything.

    A scene frame holds its people's and the clutter's detections in a random order; a person's own frame lists theirs in
    the order they have in the scene frame (what a stable regrouping of the scene frame gives back), bit for bit."""
    rng = np.random.default_rng(seed)
    eps = float(eps)
    spans = [(0, n_frames)] * people if isinstance(people, int) else [tuple(int(v) for v in s) for s in people]
    K = len(spans)
    x0 = rng.uniform(-1.0, 1.0, K)
    vx = rng.uniform(0.05, 0.15, K) * rng.choice([-1.0, 1.0], K)
    lane = 3.5 * eps * np.arange(K)
    sz, sv = np.sqrt(z_weight), np.sqrt(doppler_weight)
    slots = [(2.0 * eps * i, -3.0 * eps - 2.0 * eps * j) for i in range(-8, 9) for j in range(4)]
    scene, persons = [], [[None] * n_frames for _ in range(K)]
    for f in range(n_frames):
        rows, owner = [], []
        for k, (a, b) in enumerate(spans):
            if not a <= f < b:
                continue
            n = int(rng.integers(min_card, max_card + 1))
            u = rng.standard_normal((n, 4))
            u *= (0.49 * eps * rng.random(n) ** 0.25 / np.linalg.norm(u, axis=1))[:, None]      # inside the metric's ball
            pts = np.empty((n, 5))
            pts[:, 0] = x0[k] + vx[k] * f + u[:, 0]
            pts[:, 1] = lane[k] + u[:, 1]
            pts[:, 2] = 1.0 + (u[:, 2] / sz if sz > 0 else rng.standard_normal(n) * 0.4)
            pts[:, 3] = vx[k] * 10.0 + (u[:, 3] / sv if sv > 0 else rng.standard_normal(n) * 0.5)
            pts[:, 4] = np.exp(rng.standard_normal(n) * 1.5)
            rows.append(pts)
            owner += [k] * n
        if clutter:
            where = rng.choice(len(slots), size=clutter, replace=False)
            pts = np.empty((clutter, 5))
            pts[:, :2] = np.array(slots)[where]
            pts[:, 2] = rng.uniform(0.0, 2.0, clutter)
            pts[:, 3] = rng.standard_normal(clutter)
            pts[:, 4] = np.exp(rng.standard_normal(clutter))
            rows.append(pts)
            owner += [-1] * clutter
        allp = np.concatenate(rows) if rows else np.zeros((0, 5))
        owner = np.array(owner, dtype=np.int64)
        order = rng.permutation(len(owner))
        allp, owner = allp[order], owner[order]

        scene.append(_as_raw_frame(allp))
        for k in range(K):
            if (owner == k).any():
                persons[k][f] = _as_raw_frame(allp[owner == k])
    return scene, persons
