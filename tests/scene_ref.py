"""An independent reference of the scene clustering rule (csrc/scene.hip, scene.cluster_host), the case list, the input
conditions and the planted defects.  Plain O(m^2) numpy per frame, union-find for the components; nothing here is shared
with the package's own restatement.

The rule: d2(i, j) = dx*dx + dy*dy + wz2*dz*dz + wv2*dv*dv in float64 from the stored values; neighbours iff d2 <= eps2,
self included; core iff >= min_points neighbours; clusters = components of the core points; a non-core point with a core
neighbour joins the cluster of its nearest core neighbour (smallest d2, lowest index on ties) and links nothing; the rest
is noise (-1); ids by ascending lowest core index; ids >= Cmax are noise (err bit 1).  A frame of more than 1024
detections is all noise, a frame with offsets outside the points is not touched (err bit 0).

No tolerance anywhere: every output is an integer, a copy, or np.float32(cumsum64[-1] / count).
"""
import numpy as np

MAX_CARD = 1024
EPS = 0.5
DEFECTS = ("border_merges", "count_excludes_self", "highest_index_on_ties", "ids_by_size", "fp32_distance",
           "strict_less", "grouped_not_stable")


def _find(parent, i):
    while parent[i] != i:
        parent[i] = parent[parent[i]]
        i = parent[i]
    return i


def _d2(rows, wz2, wv2, defect):
    x = rows[:, :4].astype(np.float32 if defect == "fp32_distance" else np.float64)
    t = x.dtype.type
    d = x[:, None, :] - x[None, :, :]
    with np.errstate(invalid="ignore", over="ignore"):
        return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + t(wz2) * d[..., 2] * d[..., 2] + t(wv2) * d[..., 3] * d[..., 3]


def frame_ref(rows, eps2, wz2, wv2, min_points, Cmax, defect=None):
    """one frame -> (labels int32 [m], clusters found, d2, core)"""
    m = len(rows)
    d2 = _d2(rows, wz2, wv2, defect)
    with np.errstate(invalid="ignore"):
        nb = (d2 < d2.dtype.type(eps2)) if defect == "strict_less" else (d2 <= d2.dtype.type(eps2))
    cnt = nb.sum(axis=1) - (np.diag(nb) if defect == "count_excludes_self" else 0)
    core = cnt >= min_points
    parent = list(range(m))
    linkers = np.ones(m, bool) if defect == "border_merges" else core
    for i, j in np.argwhere(np.triu(nb, 1)):
        if (core[i] or core[j]) and linkers[i] and linkers[j]:
            a, b = _find(parent, int(i)), _find(parent, int(j))
            if a != b:
                parent[max(a, b)] = min(a, b)
    comp = np.full(m, -1, np.int64)
    for i in range(m):
        if core[i]:
            comp[i] = _find(parent, i)
    for i in range(m):
        if core[i]:
            continue
        best, bj = None, -1
        for j in range(m):
            if not core[j] or not nb[i, j]:
                continue
            better = best is None or d2[i, j] < best or (defect == "highest_index_on_ties" and d2[i, j] == best)
            if better:
                best, bj = d2[i, j], j
        if bj >= 0:
            comp[i] = comp[bj]
    roots = sorted({int(c) for c, k in zip(comp, core) if k})          # the lowest core index of every component
    if defect == "ids_by_size":
        roots.sort(key=lambda r: (-int((comp == r).sum()), r))
    ids = {r: k for k, r in enumerate(roots)}
    lab = np.array([ids.get(int(c), -1) for c in comp], dtype=np.int32).reshape(m)
    lab[lab >= Cmax] = -1
    return lab, len(roots), d2, core


def cluster_ref(points, offsets, eps2, wz2, wv2, min_points, Cmax, defect=None):
    """the launch's outputs (numpy) and the err bits, by the rule above"""
    P, n = len(points), len(offsets) - 1
    out = dict(label=np.full(P, -1, np.int32), n_clusters=np.zeros(n, np.int32), cluster_count=np.zeros((n, Cmax), np.int32),
               centroid=np.zeros((n, Cmax, 4), np.float32), grouped=np.zeros_like(points),
               seg_off=np.zeros((n, Cmax + 1), np.int32), err=0)
    for f in range(n):
        a, b = int(offsets[f]), int(offsets[f + 1])
        if a < 0 or b > P or b < a:
            out["err"] |= 1
            continue
        out["seg_off"][f] = a
        if b - a > MAX_CARD:
            out["err"] |= 1
            out["grouped"][a:b] = points[a:b]
            continue
        if b == a:
            continue
        rows = points[a:b]
        lab, c, _, _ = frame_ref(rows, eps2, wz2, wv2, min_points, Cmax, defect)
        if c > Cmax:
            out["err"] |= 2
        nc = min(c, Cmax)
        out["label"][a:b] = lab
        out["n_clusters"][f] = nc
        at = a
        for k in list(range(nc)) + [-1]:
            idx = [i for i in range(b - a) if lab[i] == k]
            if defect == "grouped_not_stable":
                idx = idx[::-1]
            if k >= 0:
                out["seg_off"][f, k] = at
                out["cluster_count"][f, k] = len(idx)
                s = np.cumsum(rows[idx, :4].astype(np.float64), axis=0)[-1]
                out["centroid"][f, k] = np.float32(s / len(idx))
            else:
                out["seg_off"][f, nc:] = at
            out["grouped"][at:at + len(idx)] = rows[idx]
            at += len(idx)
    return out


OUTPUTS = ("label", "n_clusters", "cluster_count", "centroid", "grouped", "seg_off")


def same(a, b):
    """every output equal as bits (centroids and rows compared as their integer images)"""
    return a["err"] == b["err"] and all(
        np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) and
        a[k].shape == b[k].shape and a[k].dtype == b[k].dtype for k in OUTPUTS)


# ----------------------------------------------------------------------------------------------------------- the cases
def _rows(xy, rng, z=None, v=None):
    m = len(xy)
    out = np.empty((m, 5))
    out[:, :2] = xy
    out[:, 2] = 1.0 if z is None else z
    out[:, 3] = 0.0 if v is None else v
    out[:, 4] = np.exp(rng.standard_normal(m))
    return out


def _blobs(rng, m, spread=0.17):
    """m detections around centres 4 eps apart, a tenth of them scattered: core, border and noise points"""
    k = max(1, m // 24)
    centres = np.stack([4 * EPS * (np.arange(k) % 8), 4 * EPS * (np.arange(k) // 8)], axis=1)
    xy = centres[rng.integers(0, k, m)] + rng.standard_normal((m, 2)) * spread
    far = rng.random(m) < 0.1
    xy[far] += rng.uniform(-2 * EPS, 2 * EPS, (int(far.sum()), 2))
    return _rows(xy, rng, z=1.0 + rng.standard_normal(m) * 0.3, v=rng.standard_normal(m))


def _grid3(x0, pitch=0.0625):
    return np.array([(x0 + pitch * i, pitch * j) for i in range(3) for j in range(3)])


class Case:
    def __init__(self, name, frames, min_points, Cmax=16, wz2=0.25, wv2=0.0, eps2=EPS * EPS, grid=False, tie=False,
                 dtypes=("float32", "float64"), offsets=None, note=""):
        self.name, self.frames, self.min_points, self.Cmax = name, frames, int(min_points), int(Cmax)
        self.wz2, self.wv2, self.eps2, self.grid, self.tie, self.dtypes, self.note = wz2, wv2, eps2, grid, tie, dtypes, note
        self.points64 = np.concatenate(frames) if frames else np.zeros((0, 5))
        cards = [len(f) for f in frames]
        self.offsets = np.concatenate([[0], np.cumsum(cards)]).astype(np.int32) if offsets is None else np.asarray(offsets, np.int32)

    def points(self, dtype):
        return np.ascontiguousarray(self.points64.astype(dtype))

    def args(self):
        return self.eps2, self.wz2, self.wv2, self.min_points, self.Cmax


def _make_cases():
    rng = np.random.default_rng(2024)
    cases = []
    mixed = [_blobs(rng, m) for m in (0, 1, 2, 63, 64, 65, 257)]
    cases.append(Case("mixed7", mixed, 4, wv2=0.01, note="n = 7, cardinalities 0, 1, 2, 63, 64, 65, 257; the doppler term"))
    cases.append(Case("blobs1024", [_blobs(rng, 1024, spread=0.3)], 5, Cmax=64, note="n = 1, the largest frame"))
    # a 1024-point chain spaced just under eps, in a random index order: the longest propagation; the end points are border
    s = 511.0 / 1024.0
    chain = np.stack([s * np.arange(1024), np.zeros(1024)], axis=1)[rng.permutation(1024)]
    cases.append(Case("chain1024", [_rows(chain, rng)], 3, grid=True, note="interior points have exactly min_points neighbours"))
    ang = 2 * np.pi * rng.permutation(200) / 200
    cases.append(Case("ring", [_rows(7.0 * np.stack([np.cos(ang), np.sin(ang)], axis=1), rng)], 3))
    # two 3 x 3 clusters and one point between them that sees cores of both without being core
    # (pitch 1/16; the point sees one column of three cores on either side and nothing else: 7 neighbours with itself)
    a, x = _grid3(0.0), [[0.59375, 0.0625]]
    cases.append(Case("bridge", [_rows(np.concatenate([a, x, _grid3(1.046875)]), rng)], 8, grid=True,
                      note="the border point is nearer to the second cluster; its count stays below min_points"))
    cases.append(Case("border_tie", [_rows(np.concatenate([a, x, _grid3(1.0625)]), rng)], 8, grid=True, tie=True,
                      note="the border point is exactly as far from a core of each cluster: the lowest index wins"))
    dup = np.repeat(rng.standard_normal((6, 2)) * 2.0, 5, axis=0)[rng.permutation(30)]
    cases.append(Case("duplicates", [_rows(np.concatenate([dup, rng.standard_normal((10, 2)) * 3.0]), rng)], 4))
    cases.append(Case("min_points_1", [_blobs(rng, 40), _rows(rng.standard_normal((9, 2)) * 6.0, rng)], 1, Cmax=64))
    cases.append(Case("all_noise", [_rows(np.stack([2.0 * np.arange(30), np.zeros(30)], axis=1), rng)], 3))
    pairs = np.repeat(np.stack([3.0 * np.arange(20), np.zeros(20)], axis=1), 2, axis=0) + np.tile([[0.0, 0.0], [0.125, 0.0]], (20, 1))
    cases.append(Case("too_many", [_rows(pairs, rng), _blobs(rng, 30)], 2, Cmax=4, grid=False, note="20 clusters, Cmax = 4: err bit 1"))
    cases.append(Case("card1025", [_blobs(rng, 1025), _blobs(rng, 30)], 4, note="err bit 0, the frame all noise"))
    ok = [_blobs(rng, 10), _blobs(rng, 10), _blobs(rng, 10)]
    cases.append(Case("bad_offsets", ok, 3, offsets=[-2, 10, 20, 33], note="frames 0 and 2 leave [0, P]: err bit 0, untouched"))
    cases.append(Case("backwards", ok, 3, offsets=[0, 10, 10, 5], note="a frame that runs backwards, after an empty one"))
    # d2 == eps2 exactly (0.5 apart on the grid), and d2 a relative 2^-30 above eps2 (fp64 input only)
    edge = np.array([(0.0, 0.0), (0.5, 0.0), (1.0, 0.0), (5.0, 0.0), (5.5 + 2.0 ** -32, 0.0), (6.0 + 2.0 ** -31, 0.0)])
    cases.append(Case("grid_edge", [_rows(edge[:3], rng)], 2, grid=True, note="d2 == eps2: neighbours"))
    cases.append(Case("near_eps", [_rows(edge, rng)], 2, grid=True, dtypes=("float64",),
                      note="d2 = eps2 (1 + 2^-30): not neighbours in fp64, neighbours if the distance were formed in fp32"))
    # a cluster whose x and doppler are all -0.0: the sum starts from the first member (cumsum), so the centroid is -0.0
    nz = _rows(np.stack([np.full(5, -0.0), 0.125 * np.arange(5)], axis=1), rng, v=np.full(5, -0.0))
    cases.append(Case("neg_zero", [nz], 3, grid=True, note="centroid -0.0 in x and doppler, as np.cumsum gives it"))
    return cases


CASES = _make_cases()
RUNS = [(c, dt) for c in CASES for dt in c.dtypes]


def run_id(run):
    return f"{run[0].name}-{run[1]}"


def check_conditions(case, dtype):
    """the input conditions, on the reference: no pair's d2 within 2^-40 relative of eps2 unless it sits there exactly on
    a power-of-two grid; nearest-core ties only where planted"""
    pts = case.points(dtype)
    P = len(pts)
    for f in range(len(case.offsets) - 1):
        a, b = int(case.offsets[f]), int(case.offsets[f + 1])
        if a < 0 or b > P or b <= a or b - a > MAX_CARD:
            continue
        rows = pts[a:b]
        _, _, d2, core = frame_ref(rows, *case.args())
        rel = np.abs(d2 - case.eps2) / case.eps2
        close = rel < 2.0 ** -40
        if close.any():
            assert case.grid and (d2[close] == case.eps2).all(), (case.name, f, "a d2 within 2^-40 of eps2")
            assert (rows[:, :4] * 2.0 ** 40 == np.round(rows[:, :4] * 2.0 ** 40)).all(), (case.name, "not on a grid")
        for i in np.flatnonzero(~core):
            cand = np.flatnonzero(core & (d2[i] <= case.eps2))
            if cand.size and (d2[i, cand] == d2[i, cand].min()).sum() > 1:
                assert case.tie, (case.name, f, int(i), "an unplanted nearest-core tie")


# ------------------------------------------------------------------------------------------------- gather_segments
def gather_ref(src, seg_start, out_off, rows):
    """-> (out [rows, 5], err)"""
    out, err = np.zeros((rows, 5), src.dtype), 0
    for o in range(len(seg_start)):
        a, b, s = int(out_off[o]), int(out_off[o + 1]), int(seg_start[o])
        if a < 0 or b < a or b > rows or s < 0 or s + (b - a) > len(src):
            err = 1
            continue
        out[a:b] = src[s:s + b - a]
    return out, err
