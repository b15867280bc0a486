"""Scene frames -> people: the front end of the raw chain.

A radar delivers one point cloud per frame with everybody in view plus clutter.  ``ops.scene_cluster`` splits every frame
of a tick into density clusters on the device and regroups its detections cluster by cluster; ``associate`` (numpy, over
the few KB that come back) follows the clusters from frame to frame and owns stream birth and death;
``ops.gather_segments`` lays the chosen segments out as the ``(points, offsets)`` that ``MultiStreamScorer.push_raw``
takes.  ``SceneSplitter`` ties the three to a scorer, ``split_recording`` runs the same code over a stored recording.

``cluster_host`` restates the kernel's rule in numpy, bit for bit (as ``datasets.device_picks_host`` restates the pick
draws): the documentation of the rule that can be executed.
"""
import collections

import numpy as np
import torch

from . import ops

RAW_MAX_CARD = ops.RAW_MAX_CARD
ERR_BAD_FRAME, ERR_TOO_MANY_CLUSTERS = 1, 2        # the bits of the device flag ``err``


def metric(eps, z_weight, doppler_weight):
    """the kernel's three doubles ``(eps2, wz2, wv2)``: ``d2 = dx*dx + dy*dy + z_weight*dz*dz + doppler_weight*dv*dv``,
    neighbours iff ``d2 <= eps*eps``"""
    eps, wz2, wv2 = float(eps), float(z_weight), float(doppler_weight)
    if not (0.0 <= eps < np.inf and 0.0 <= wz2 < np.inf and 0.0 <= wv2 < np.inf):
        raise ValueError(f"scene: eps, z_weight and doppler_weight must be finite and >= 0, got {eps}, {wz2}, {wv2}")
    return eps * eps, wz2, wv2


def pair_d2(cols, wz2, wv2):
    """``d2(i, j)`` of one frame, float64 [m, m], from its columns x, y, z, doppler (``cols`` [m, >= 4], any float type:
    the stored values widened): the kernel's expression, in its order -- numpy rounds every product and sum, as the kernel
    does with contraction off"""
    c = np.asarray(cols)[:, :4].astype(np.float64)
    dx, dy = c[:, None, 0] - c[None, :, 0], c[:, None, 1] - c[None, :, 1]
    dz, dv = c[:, None, 2] - c[None, :, 2], c[:, None, 3] - c[None, :, 3]
    with np.errstate(invalid="ignore", over="ignore"):
        return dx * dx + dy * dy + np.float64(wz2) * dz * dz + np.float64(wv2) * dv * dv


def cluster_frame_host(cols, eps2, wz2, wv2, min_points, max_clusters):
    """The rule for ONE frame -> ``(label int32 [m], c)``: c clusters found (before the cap), labels ``0 .. min(c,
    max_clusters) - 1`` or -1.

    * ``i`` and ``j`` are neighbours iff ``d2(i, j) <= eps2`` (``pair_d2``); self counts;
    * ``i`` is core iff it has ``>= min_points`` neighbours;
    * clusters are the connected components of the core points under the neighbour relation;
    * a non-core point with at least one core neighbour joins the cluster of its nearest core neighbour (smallest d2,
      lowest index on exact ties) and links nothing;
    * the rest is noise (-1);
    * ids ascend with each cluster's lowest core index; ids ``>= max_clusters`` become noise."""
    m = len(cols)
    if m == 0:
        return np.zeros(0, np.int32), 0
    d2 = pair_d2(cols, wz2, wv2)
    with np.errstate(invalid="ignore"):
        nb = d2 <= np.float64(eps2)
    core = nb.sum(axis=1) >= int(min_points)
    big = m
    lab = np.where(core, np.arange(m), big)
    link = nb & core[None, :] & core[:, None]
    while True:                                    # the lowest label among a core point's core neighbours, to its root
        new = np.where(link, lab[None, :], big).min(axis=1)
        new = np.minimum(new, lab)
        while True:
            up = np.where(new < big, np.append(new, big)[new], big)
            if np.array_equal(up, new):
                break
            new = up
        if np.array_equal(new, lab):
            break
        lab = new
    to_core = np.where(nb & core[None, :], d2, np.inf)
    nearest = to_core.argmin(axis=1)               # (the first minimum: the lowest index on exact ties)
    border = ~core & np.isfinite(to_core.min(axis=1))
    lab = np.where(border, lab[nearest], lab)
    roots = np.flatnonzero(core & (lab == np.arange(m)))
    cid = np.full(m + 1, -1, np.int64)
    cid[roots] = np.arange(roots.size)
    out = cid[lab]
    out[out >= int(max_clusters)] = -1
    return out.astype(np.int32), int(roots.size)


def cluster_host(points, offsets, eps2, wz2, wv2, min_points, max_clusters):
    """``ops.scene_cluster`` on the host, bit for bit: ``points`` [P, 5] float32 / float64 and ``offsets`` [n + 1] (numpy) ->
    a dict of ``label``, ``n_clusters``, ``cluster_count``, ``centroid``, ``grouped``, ``seg_off`` and ``err`` (the bits
    the launch would set).  Rows that no frame owns are zero (``label``: -1), as the wrapper leaves them."""
    points = np.asarray(points)
    offsets = np.asarray(offsets, dtype=np.int64)
    P, n, Cmax = points.shape[0], offsets.size - 1, int(max_clusters)
    label = np.full(P, -1, np.int32)
    grouped = np.zeros_like(points)
    n_clusters = np.zeros(n, np.int32)
    count = np.zeros((n, Cmax), np.int32)
    centroid = np.zeros((n, Cmax, 4), np.float32)
    seg_off = np.zeros((n, Cmax + 1), np.int32)
    err = 0
    for f in range(n):
        a, b = int(offsets[f]), int(offsets[f + 1])
        if a < 0 or b > P or b < a:                # the frame's rows are not touched
            err |= ERR_BAD_FRAME
            continue
        seg_off[f] = a
        if b - a > RAW_MAX_CARD:                   # all noise, the rows as they are
            err |= ERR_BAD_FRAME
            grouped[a:b] = points[a:b]
            continue
        rows = points[a:b]
        lab, c = cluster_frame_host(rows, eps2, wz2, wv2, min_points, Cmax)
        if c > Cmax:
            err |= ERR_TOO_MANY_CLUSTERS
        nc = min(c, Cmax)
        label[a:b] = lab
        n_clusters[f] = nc
        key = np.where(lab < 0, Cmax, lab)
        order = np.argsort(key, kind="stable")     # cluster 0, 1, ..., then noise; ascending detection order inside
        grouped[a:b] = rows[order]
        sizes = np.bincount(key, minlength=Cmax + 1)
        count[f] = sizes[:Cmax]
        seg_off[f] = a + np.cumsum(sizes) - sizes
        for k in range(nc):
            s = np.cumsum(rows[lab == k, :4].astype(np.float64), axis=0)[-1]      # ascending detection order, from the first member
            centroid[f, k] = (s / np.float64(sizes[k])).astype(np.float32)
    return dict(label=label, n_clusters=n_clusters, cluster_count=count, centroid=centroid, grouped=grouped,
                seg_off=seg_off, err=err)


# --------------------------------------------------------------------------------------------------------- association
AssocParams = collections.namedtuple("AssocParams", "gate confirm max_missed birth_points alpha beta")
AssocParams.__doc__ = """``gate``: metres in the plane between a track's prediction and a cluster's centroid; ``confirm``:
consecutive hits that confirm a track; ``max_missed``: a track dies after MORE consecutive misses than this;
``birth_points``: detections an unassigned cluster needs to start a track; ``alpha`` / ``beta``: the filter's fixed gains."""


class Track:
    """one track of ``AssocState``: ``p`` / ``v`` float64 [2] (metres, metres per frame), ``hits`` consecutive hits while
    tentative, ``missed`` consecutive misses"""
    __slots__ = ("id", "p", "v", "hits", "missed", "confirmed")

    def __init__(self, id, p):
        self.id, self.p, self.v = int(id), np.array(p, np.float64), np.zeros(2, np.float64)
        self.hits, self.missed, self.confirmed = 0, 0, False

    def copy(self):
        t = Track(self.id, self.p)
        t.v, t.hits, t.missed, t.confirmed = self.v.copy(), self.hits, self.missed, self.confirmed
        return t


class AssocState:
    """the tracks alive between two ticks, in track-id order, and the next id"""
    __slots__ = ("tracks", "next_id")

    def __init__(self, tracks=(), next_id=0):
        self.tracks, self.next_id = list(tracks), int(next_id)


class AssocPlan:
    """What ``associate`` decided for one tick.  ``segments``: ``{track id: [(frame, cluster), ...]}`` in track-id order,
    an entry for every confirmed track that lived in the tick (possibly empty), frames ascending; ``births`` / ``confirmed``
    / ``deaths``: ``[(track id, frame)]`` in the order they happened; ``positions``: ``{track id: (x, y)}`` of the tracks
    alive after the tick; ``refused``: the track ids ``refuse`` took out again (no stream was free for them)."""
    __slots__ = ("segments", "births", "confirmed", "deaths", "positions", "refused")


def associate(state, counts, centroids, params):
    """One tick of the association step, a pure function (numpy only): ``state`` (``AssocState``; not modified),
    ``counts`` int [n, Cmax] and ``centroids`` [n, Cmax, >= 2] of the tick's n scene frames in time order (what
    ``ops.scene_cluster`` returned: frame f's clusters are the leading entries with ``counts > 0``), ``params``
    (``AssocParams``) -> ``(state', plan)``.  Per frame:

    1. every track predicts ``p + v``;
    2. the pairs (track, cluster) with planar distance ``<= gate`` are sorted by (distance, track id, cluster id) and
       assigned greedily; an assigned track takes ``p = pred + alpha r``, ``v += beta r`` with ``r = centroid - pred``,
       counts a hit and forgets its misses; a tentative track with ``confirm`` consecutive hits is confirmed, and from that
       frame on its clusters are emitted (earlier frames are dropped);
    3. an unassigned track coasts (``p = pred``), loses its consecutive hits, and dies after MORE than ``max_missed``
       consecutive misses;
    4. an unassigned cluster with ``count >= birth_points`` starts a tentative track at its centroid (its first hit), ids
       in cluster order."""
    counts = np.asarray(counts)
    centroids = np.asarray(centroids, dtype=np.float64)
    tracks = [t.copy() for t in state.tracks]
    next_id = state.next_id
    plan = AssocPlan()
    plan.births, plan.confirmed, plan.deaths, plan.refused = [], [], [], []
    segments = {t.id: [] for t in tracks if t.confirmed}

    def hit(t, f, c):
        t.hits += 1
        t.missed = 0
        if not t.confirmed and t.hits >= params.confirm:
            t.confirmed = True
            plan.confirmed.append((t.id, f))
            segments[t.id] = []
        if t.confirmed:
            segments[t.id].append((f, c))

    for f in range(counts.shape[0]):
        nc = int(np.count_nonzero(counts[f] > 0))
        z = centroids[f, :nc, :2]
        pred = {t.id: t.p + t.v for t in tracks}
        cand = []
        if tracks and nc:                           # every (track, cluster) distance at once; the pairs inside the gate
            pp = np.stack([pred[t.id] for t in tracks])
            dist = np.hypot(z[None, :, 0] - pp[:, None, 0], z[None, :, 1] - pp[:, None, 1])
            ti, ci = np.nonzero(dist <= params.gate)
            cand = sorted(zip(dist[ti, ci].tolist(), [tracks[i].id for i in ti.tolist()], ci.tolist()))
        got, taken = {}, set()
        for d, tid, c in cand:
            if tid in got or c in taken:
                continue
            got[tid] = c
            taken.add(c)
        alive = []
        for t in tracks:
            if t.id in got:
                r = z[got[t.id]] - pred[t.id]
                t.p = pred[t.id] + params.alpha * r
                t.v = t.v + params.beta * r
                hit(t, f, got[t.id])
            else:
                t.p = pred[t.id]
                t.missed += 1
                if not t.confirmed:
                    t.hits = 0
                if t.missed > params.max_missed:
                    plan.deaths.append((t.id, f))
                    continue
            alive.append(t)
        tracks = alive
        for c in range(nc):
            if c in taken or counts[f, c] < params.birth_points:
                continue
            t = Track(next_id, z[c])
            next_id += 1
            plan.births.append((t.id, f))
            tracks.append(t)
            hit(t, f, c)
    plan.segments = dict(sorted(segments.items()))
    plan.positions = {t.id: (float(t.p[0]), float(t.p[1])) for t in tracks}
    return AssocState(tracks, next_id), plan


def refuse(state, plan, tids):
    """Take the tracks ``tids`` -- confirmed in this tick -- out of ``associate``'s result again, in place: out of the
    state, and out of the plan's segments, births, confirmations, deaths and positions; they are listed in
    ``plan.refused``.  What a caller does when it has no stream for them: their detections go to no stream in this tick,
    and a person who is still in view starts a new track in the next frame that is clustered, so the birth is deferred
    until a stream is free.  -> ``(state, plan)``"""
    gone = set(tids)
    state.tracks = [t for t in state.tracks if t.id not in gone]
    for t in gone:
        plan.segments.pop(t, None)
        plan.positions.pop(t, None)
    for name in ("births", "confirmed", "deaths"):
        setattr(plan, name, [(t, f) for t, f in getattr(plan, name) if t not in gone])
    plan.refused += [t for t in tids]
    return state, plan


# ------------------------------------------------------------------------------------------------------- the front end
class SceneFront:
    """Steps 1 - 6 of ``SceneSplitter.push`` without a scorer: cluster on a side stream (behind ``ready``, see there), ONE
    host wait for the few KB of cluster tables, ``associate``, one pinned upload of the segment table, one gather on the
    current stream."""

    def __init__(self, device, eps, min_points, z_weight, doppler_weight, max_clusters, params):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("scene: the front end runs on the HIP device; this package has no CPU path")
        self.eps2, self.wz2, self.wv2 = metric(eps, z_weight, doppler_weight)
        self.min_points, self.max_clusters, self.params = int(min_points), int(max_clusters), params
        if self.min_points < 1 or not 1 <= self.max_clusters <= ops.SCENE_MAX_CLUSTERS:
            raise ValueError(f"scene: needs min_points >= 1 and 1 <= max_clusters <= {ops.SCENE_MAX_CLUSTERS}")
        if params.confirm < 1 or params.max_missed < 0 or params.birth_points < 1 or not params.gate >= 0.0:
            raise ValueError(f"scene: needs confirm >= 1, max_missed >= 0, birth_points >= 1, gate >= 0; got {params}")
        self.err = torch.zeros(1, dtype=torch.int32, device=self.device)     # bits: ERR_BAD_FRAME, ERR_TOO_MANY_CLUSTERS
        self.gather_err = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.side = torch.cuda.Stream(device=self.device)
        self.state = AssocState()

    def cluster(self, points, offsets, ready=None):
        """steps 1 and 2 -> (grouped on the device, the host copies of n_clusters, cluster_count, centroid, seg_off).
        ``ready``: an event recorded behind the upload of ``points`` / ``offsets`` on the stream that made it; the side
        stream waits for it alone.  None: the inputs are taken to be made on the current stream, and the side stream waits
        for everything queued there so far."""
        n, C = offsets.numel() - 1, self.max_clusters
        main = ops.current_stream()
        if ready is None:
            ready = torch.cuda.Event()
            ready.record(main)
        self.side.wait_event(ready)
        with ops.on_stream(self.side):
            _, ncl, count, cen, grouped, seg = ops.scene_cluster(points, offsets, self.eps2, self.wz2, self.wv2,
                                                                 self.min_points, C, self.err, zero_fill=False)
            packed = torch.cat([ncl, count.reshape(-1), cen.view(torch.int32).reshape(-1), seg.reshape(-1)])
            host = torch.empty(packed.numel(), dtype=torch.int32, pin_memory=True)
            host.copy_(packed, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.side)
        for t in (points, offsets):
            t.record_stream(self.side)
        grouped.record_stream(main)
        done.synchronize()                          # THE host wait of the front end
        main.wait_event(done)
        h = host.numpy()
        a = np.cumsum([0, n, n * C, n * C * 4, n * (C + 1)])
        return (grouped, h[a[0]:a[1]], h[a[1]:a[2]].reshape(n, C), h[a[2]:a[3]].view(np.float32).reshape(n, C, 4),
                h[a[3]:a[4]].reshape(n, C + 1))

    def split(self, points, offsets, ready=None, accept=None):
        """steps 1 - 6 -> ``(plan, track ids, frames per track, points', offsets' (device), offsets' (host), noise)``: the
        detections of the tick's emitted segments, track by track in track-id order, in the layout ``push_raw`` takes.
        ``accept(state', plan)``: called before the new state is kept; it may ``refuse`` tracks, and if it raises the front
        end is as it was before the call"""
        P, n = points.shape[0], offsets.numel() - 1
        if n == 0:
            plan = associate(self.state, np.zeros((0, self.max_clusters), np.int32), np.zeros((0, self.max_clusters, 4)),
                             self.params)[1]
            return plan, [], [], points[:0], offsets[:1], np.zeros(1, np.int64), 0
        grouped, _, count, centroid, seg_off = self.cluster(points, offsets, ready)
        state, plan = associate(self.state, count, centroid, self.params)
        if accept is not None:
            accept(state, plan)
        self.state = state
        tids = [t for t, segs in plan.segments.items() if segs]
        per_track = [len(plan.segments[t]) for t in tids]
        fc = np.array([s for t in tids for s in plan.segments[t]], dtype=np.int64).reshape(-1, 2)
        start = seg_off[fc[:, 0], fc[:, 1]].astype(np.int64)
        length = seg_off[fc[:, 0], fc[:, 1] + 1].astype(np.int64) - start
        M, rows = start.size, int(length.sum())
        if M == 0:
            return plan, [], [], points[:0], offsets[:1], np.zeros(1, np.int64), P
        table = torch.empty(2 * M + 1, dtype=torch.int32, pin_memory=True)
        t = table.numpy()
        t[:M], t[M] = start, 0
        np.cumsum(length, out=t[M + 1:])
        dev = table.to(self.device, non_blocking=True)
        out = ops.gather_segments(grouped, dev[:M], dev[M:], rows, err_flag=self.gather_err, zero_fill=False)
        return plan, tids, per_track, out, dev[M:], t[M:].astype(np.int64), P - rows


class SceneTick:
    """The result of one ``SceneSplitter.push``.  ``tick``: the scorer's ``Tick``; ``tids`` / ``sids`` / ``counts``: the
    tracks that were fed, their streams and their frames, in track-id order; ``track_of_stream`` / ``stream_of_track``:
    the confirmed tracks alive after the tick; ``opened`` / ``closed``: ``[(track id, stream id)]`` of this tick (a track
    that still received frames in the tick it died in was closed after they were scored, the others before the new
    streams were opened); ``refused``: track ids that were confirmed in this tick while every stream was in use -- they
    were taken out again (``refuse``), and a person still in view is born anew in the next tick; ``positions``:
    ``{track id: (x, y)}`` of every live track, tentative ones included; ``noise``: detections of the tick that went to
    no stream."""
    __slots__ = ("tick", "tids", "sids", "counts", "track_of_stream", "stream_of_track", "opened", "closed", "refused",
                 "positions", "noise")


class SceneSplitter:
    """Scene frames in, a ``MultiStreamScorer``'s ticks out.  ``push(points, offsets, ready=None)`` takes the next n scene
    frames (``datasets.pack_raw_frames`` layout, on the device; n <= the scorer's ``max_push``) and does, in order:

    1. ``ops.scene_cluster`` and the copy of its cluster tables (a few KB) to pinned memory, both on the splitter's own
       side stream.  That stream waits for ``ready`` alone: an event the caller recorded behind the upload of the frames
       on the stream that made it (an upload stream of the caller's own) -- then the clustering and the host's wait do
       NOT stand behind the previous tick's scoring, which is still running on the current stream.  Without ``ready`` the
       frames are taken to be made on the current stream; streams run in order, so the side stream then waits for all
       that is queued there and the host's wait covers what is left of the previous tick;
    2. ONE host wait, on that copy's event: the documented wait of the front end (a birth changes which streams exist,
       and the tick's plan is made on the host; the scorers themselves stay free of waits);
    3. ``associate``; tracks confirmed beyond the scorer's free slots are refused before the state is kept;
    4. ``ms.close`` for the tracks that died, ``ms.open`` for the tracks confirmed in this tick (track-id order);
    5. one pinned upload of the segment table;
    6. ``ops.gather_segments`` on the current stream;
    7. ``ms.push_raw(sids, counts, points', offsets')``.

    The metric is ``dx^2 + dy^2 + z_weight dz^2 + doppler_weight dv^2 <= eps^2`` (metres; ``metric``).  The defaults are
    choices from the scale of a person in the tracks, not measurements.  ``err`` is a device flag beside
    ``ms.raw_err``: bit 0 a scene frame that could not be clustered, bit 1 a frame with more than ``max_clusters``
    clusters."""

    def __init__(self, ms, eps=0.5, min_points=3, z_weight=0.1, doppler_weight=0.0, max_clusters=16, gate=0.6, confirm=3,
                 max_missed=5, birth_points=5, alpha=0.5, beta=0.2):
        self.ms = ms
        params = AssocParams(float(gate), int(confirm), int(max_missed), int(birth_points), float(alpha), float(beta))
        self.front = SceneFront(ms.ring.device, eps, min_points, z_weight, doppler_weight, max_clusters, params)
        self.stream_of_track = {}

    @property
    def err(self):
        return self.front.err

    def _accept(self, state, plan):
        """the slots the tick needs against the slots the scorer has, BEFORE anything is kept: the streams free now, plus
        those of the tracks that died without frames in this tick (closed before the opens), are handed out in the
        order of confirmation; the rest is refused.  (A track that dies in a tick it was still fed in frees its slot
        only after the tick: a birth that would need it waits for the next tick.)"""
        free = int(self.ms.max_streams - np.count_nonzero(self.ms._open))
        free += sum(1 for t, _ in plan.deaths if t in self.stream_of_track and not plan.segments.get(t))
        late = [t for t, _ in plan.confirmed][free:]
        if late:
            refuse(state, plan, late)

    @torch.no_grad()
    def push(self, points, offsets, ready=None) -> SceneTick:
        from . import frame_table
        ms = self.ms
        n = frame_table.check_raw(points, offsets, None, ms._N, "SceneSplitter.push")
        if n > ms.max_push:
            raise ValueError(f"SceneSplitter.push: {n} scene frames exceed the scorer's max_push = {ms.max_push}")
        plan, tids, per_track, pts, offs, _, noise = self.front.split(points, offsets, ready, self._accept)
        born = {t for t, _ in plan.confirmed}
        dead = [t for t, _ in plan.deaths if t in self.stream_of_track or t in born]
        fed = set(tids)
        out = SceneTick()
        out.opened, out.closed, out.refused = [], [], list(plan.refused)
        for t in dead:
            if t not in fed:
                sid = self.stream_of_track.pop(t)
                ms.close(sid)
                out.closed.append((t, sid))
        for t, _ in plan.confirmed:
            self.stream_of_track[t] = ms.open()             # (its confirming hit is a segment of this tick; _accept counted the slot)
            out.opened.append((t, self.stream_of_track[t]))
        out.tids = list(tids)
        out.sids = [self.stream_of_track[t] for t in tids]
        out.counts = list(per_track)
        out.tick = ms.push_raw(np.array(out.sids, np.int64), np.array(out.counts, np.int64), pts, offs)
        for t in dead:
            if t in fed:
                sid = self.stream_of_track.pop(t)
                ms.close(sid)
                out.closed.append((t, sid))
        out.stream_of_track = dict(self.stream_of_track)
        out.track_of_stream = {s: t for t, s in self.stream_of_track.items()}
        out.positions, out.noise = plan.positions, noise
        return out


@torch.no_grad()
def split_recording(points, offsets, eps=0.5, min_points=3, z_weight=0.1, doppler_weight=0.0, max_clusters=16, gate=0.6,
                    confirm=3, max_missed=5, birth_points=5, alpha=0.5, beta=0.2, chunk=64):
    """A stored scene recording -> ``{track id: (points, offsets, first_frame)}`` on the device: every confirmed track's
    own frames in the layout ``OpenSetScorer.embed_raw_track`` takes, ``first_frame`` the scene frame of its first one.
    ``points`` [P, 5] fp32 / fp64 and ``offsets`` int32 [F + 1] on the device; the recording goes through
    ``SceneSplitter``'s front end (same kernels, same association, one host wait per chunk) ``chunk`` frames at a time."""
    from . import frame_table
    F = frame_table.check_raw(points, offsets, None, 1, "split_recording")
    params = AssocParams(float(gate), int(confirm), int(max_missed), int(birth_points), float(alpha), float(beta))
    front = SceneFront(points.device, eps, min_points, z_weight, doppler_weight, max_clusters, params)
    host_off = offsets.cpu().numpy().astype(np.int64)
    parts, cards, first = {}, {}, {}
    for a in range(0, F, int(chunk)):
        b = min(a + int(chunk), F)
        lo, hi = int(host_off[a]), int(host_off[b])
        lo, hi = min(max(lo, 0), points.shape[0]), min(max(hi, 0), points.shape[0])
        sub = (offsets[a:b + 1] - lo).contiguous()
        plan, tids, per_track, pts, _, oh, _ = front.split(points[lo:max(hi, lo)], sub)
        if not tids:
            continue
        at = 0
        for t, k in zip(tids, per_track):
            parts.setdefault(t, []).append(pts[oh[at]:oh[at + k]])
            cards.setdefault(t, []).append(np.diff(oh[at:at + k + 1]))
            first.setdefault(t, a + plan.segments[t][0][0])
            at += k
    out = {}
    for t in sorted(parts):
        off = np.concatenate([[0], np.cumsum(np.concatenate(cards[t]))]).astype(np.int32)
        out[t] = (torch.cat(parts[t]).contiguous(), torch.from_numpy(off).to(points.device), first[t])
    return out
