"""fp64 restatements, gates and planted defects of the backward through the track routes: ``ops.segment_weighted_mean_bwd``
(csrc/segment_pool.hip) and ``ops.gather_sum_rows`` (csrc/track_infer.hip), and the generators and oracle pieces the
module tests share.  Used by tests/test_track_bwd_branches.py (the kernels and modules, on the GPU) and
tests/test_track_bwd_gates_cpu.py (the gates' power and the identity, on the CPU).  Built from tests/eval_bwd_ref.py /
tests/elementwise_ref.py (every gate and the "same stored values on both sides" rule are theirs) and
tests/raw_unique_ref.py (the frames).  numpy / torch on the host only.

The segment backward
--------------------
For row r of a valid segment f (``u_off[f] <= r < u_off[f + 1]``, inside ``[0, M]``, not running backwards):

    g = dpool[f] * weight[r] / N;   dz = g ELU'(y[r] scale + shift);   dy[r] = scale dz
    stats = {sum_r dz, sum_r dz (y - mean) rstd}       (mean, rstd: the RUNNING moments of the bias-free y)

and dy = 0 on every row no valid segment owns.  The reference forms the per-row g in fp64 from the stored fp32 dpool and
weight and hands it to ``eval_bwd_ref.bn_eval_act_bwd_ref`` as a dense ``da`` -- the same arithmetic from there on.

* dy: ``eval_bwd_ref``'s dy gate in its ``da`` form, |dy| (rel_e + 2u) + 8u |dy|, whose 2u stand for the products g*e and
  pool_scale*dpool.  Here g has one rounding more: weight / N is rounded (u), its product with dpool is rounded (u), g*e
  is rounded (u) -- 3u.  So the gate is that gate plus u |dy|; 2^-8 |dy| more for a bf16 dy.  A row that no valid segment
  owns has gate 0: it must be exactly zero.
* both statistics: the kernel sums a row lane's rows of at most 128 consecutive rows OF A SEGMENT in fp32 (four row lanes,
  row r of the chunk on lane r % 4) and adds the lanes' partials in fp64.  The gate is ``elementwise_ref.sum_gate`` (lanes
  = 4) summed over the 128-row chunks of every valid segment: the 128-row-partial gate of ``bn_act_bwd_dz``, with the
  partials cut at the segments' ends.  (The gate allows the four lane sums to meet in fp32; the kernel meets them in
  fp64, which is covered.)  The summands' own roundings are sum_gate's SUM_PAD, as there.

The overlap-add
---------------
``dst[u] = sum_{k in [csr_off[u], csr_off[u + 1])} src[csr_idx[k]]`` starting from +0, ascending k, fp32, plain adds.  The
reference is that loop in numpy float32: no gate, the comparison is bit for bit.  ``csr_ref`` restates the plan's
transpose from the windows' start rows by the rule of ``ops.WindowRows.row_index`` (a window wraps inside the ring it
starts in) with Python loops.

Planted defects
---------------
``SEGMENT_DEFECTS``: "no_weight" (g = dpool / N), "no_inv_n" (g = dpool weight), "next_segment_grad" (segment f takes
dpool[f + 1]), "tail_unwritten" (the rows behind u_off[n] keep what the buffer held: NaN), "batch_stats" (xhat from the
batch's own moments of y).  ``OVERLAP_DEFECTS``: "drop_last" (a row's last contributor left out), "next_row" (row u gets
the contributors of row u + 1).
"""
import numpy as np
import torch

import elementwise_ref as E
import eval_bwd_ref as EB
import raw_unique_ref as RU
from opensetgaitrecognition_pcaa_amd import datasets, synthetic as syn
from oracle import pcaa_oracle as O

U = E.U
STAT_ROWS = 128          # consecutive rows of a segment whose statistics the kernel sums in fp32
LANES = 4                # its row lanes
SEGMENT_DEFECTS = ("no_weight", "no_inv_n", "next_segment_grad", "tail_unwritten", "batch_stats")
OVERLAP_DEFECTS = ("drop_last", "next_row")

# one launch with every segment length the kernel treats differently: empty, one row (three lanes idle), 3 / 4 / 5 (around
# the four row lanes), 129 (a second statistics chunk of one row), 1024 (eight chunks)
SEGMENTS = (0, 1, 3, 4, 5, 129, 1024)
TAIL = 37                # rows behind u_off[n] that no segment owns
CHANNELS = (8, 16, 520, 1024)
N_POINTS = 32


def valid_segments(u_off, M):
    u = np.asarray(u_off, dtype=np.int64)
    return [(f, int(u[f]), int(u[f + 1])) for f in range(u.size - 1) if 0 <= u[f] <= u[f + 1] <= M]


def segment_case(ch, dtype, seed=0, device="cpu"):
    """-> dict of the inputs of one launch over SEGMENTS (+ TAIL unowned rows): the same stored values for the kernel and
    the reference.  Some rows inside the segments have weight 0."""
    u_off = np.concatenate([[0], np.cumsum(SEGMENTS)]).astype(np.int32)
    n, M = len(SEGMENTS), int(u_off[-1]) + TAIL
    s = E.seed_of(ch, 7 + seed)
    y = E.activations(M, ch, dtype, s, device)
    scale, shift, mean, rstd = E.bn_vectors(ch, s, device)
    dpool = E.uniform(n * ch, s + 11, device, -1.0, 1.0).view(n, ch).float()
    weight = torch.floor(E.uniform(M, s + 12, device, 0.0, 6.0)).float()          # integer multiplicities 0 .. 5
    weight[int(u_off[6])] = 32.0
    weight[M - TAIL:] = 0.0
    return dict(y=y, scale=scale, shift=shift, mean=mean, rstd=rstd, dpool=dpool, weight=weight,
                u_off=torch.from_numpy(u_off).to(device), N=N_POINTS, M=M, n=n, ch=ch)


def row_gradient(dpool, weight, u_off, N, M, defect=None):
    """fp64 [M, ch]: g of every row (zero where no valid segment owns it)"""
    dp, w = dpool.double(), weight.double()
    n = dp.shape[0]
    g = torch.zeros((M, dp.shape[1]), dtype=torch.float64, device=dp.device)
    for f, u0, u1 in valid_segments(u_off.cpu().numpy(), M):
        src = dp[min(f + 1, n - 1)] if defect == "next_segment_grad" else dp[f]
        wr = torch.ones(u1 - u0, 1, dtype=torch.float64, device=dp.device) if defect == "no_weight" else w[u0:u1, None]
        g[u0:u1] = src[None, :] * wr * (1.0 if defect == "no_inv_n" else 1.0 / N)
    return g


def segment_bwd_ref(y, scale, shift, mean, rstd, dpool, weight, u_off, N, defect=None, **_):
    """-> dict(dy [M, ch] fp64, dy_gate (for y's dtype), stats [2, ch], stats_gate [2, ch])"""
    M, ch = y.shape
    g = row_gradient(dpool, weight, u_off, N, M, defect)
    ref = EB.bn_eval_act_bwd_ref(y, scale, shift, mean, rstd, da=g, defect="batch_stats" if defect == "batch_stats" else None)
    dy = ref["dy"]
    gate = E.out_gate(ref["dy_gate"] + U * dy.abs(), dy, y.dtype)
    yd, z, T, neg = E._z(y, scale.double(), shift.double())
    dz = g * E.elu_grad(z)
    t2 = dz * ((yd - mean.double()) * rstd.double())
    m1, m2 = dz.abs(), dz.abs() * (yd.abs() + mean.double().abs()) * rstd.double()
    sg = torch.zeros((2, ch), dtype=torch.float64, device=y.device)
    for _, u0, u1 in valid_segments(u_off.cpu().numpy(), M):
        if u1 > u0:
            sg[0] += E.block_sum_gate(dz[u0:u1], m1[u0:u1], STAT_ROWS, LANES)
            sg[1] += E.block_sum_gate(t2[u0:u1], m2[u0:u1], STAT_ROWS, LANES)
    if defect == "tail_unwritten":
        dy = dy.clone()
        dy[int(u_off[-1]):] = float("nan")
    return {"dy": dy, "dy_gate": gate, "stats": ref["stats"], "stats_gate": sg}


def segment_bwd_fp32(y, scale, shift, mean, rstd, dpool, weight, u_off, N, **_):
    """The kernel's arithmetic in plain fp32 torch, statistics chunk by chunk as the kernel adds them -> (dy in y's dtype,
    stats fp64 [2, ch]): what the CPU file holds against the gates."""
    M, ch = y.shape
    yf = y.float()
    dy = torch.zeros((M, ch), dtype=torch.float32)
    stats = torch.zeros((2, ch), dtype=torch.float64)
    for f, u0, u1 in valid_segments(u_off.numpy(), M):
        if u1 == u0:
            continue
        wn = weight[u0:u1] / torch.tensor(float(N), dtype=torch.float32)
        z = yf[u0:u1] * scale + shift
        dz = (dpool[f][None, :] * wn[:, None]) * torch.where(z > 0, torch.ones_like(z), torch.exp(z))
        dy[u0:u1] = scale * dz
        t2 = dz * ((yf[u0:u1] - mean) * rstd)
        for a in range(0, u1 - u0, STAT_ROWS):
            for lane in range(LANES):
                p1 = torch.zeros(ch, dtype=torch.float32)
                p2 = torch.zeros(ch, dtype=torch.float32)
                for r in range(a + lane, min(a + STAT_ROWS, u1 - u0), LANES):
                    p1 = p1 + dz[r]
                    p2 = p2 + t2[r]
                stats[0] += p1.double()
                stats[1] += p2.double()
    return dy.to(y.dtype), stats


def ratio(got, want, gate):
    """largest |got - want| / gate; inf where ``got`` is not finite or an element with a zero gate is not exact"""
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    gate = torch.as_tensor(gate).double().cpu()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - want).abs()
    if bool(((gate == 0) & (err != 0)).any()):
        return float("inf")
    return float((err / torch.where(gate > 0, gate, torch.ones_like(gate))).max()) if err.numel() else 0.0


# ------------------------------------------------------------------------------------------------ the overlap-add
def row_index_ref(starts, T, table_rows, ring_rows=0, segments=0):
    """the table row of every (window, step), by the rule of ops.WindowRows.row_index, in Python integers"""
    ring = ring_rows or table_rows or 1
    out = []
    for s in (int(v) for v in starts):
        base, off = s - s % ring, s % ring
        out += [base + (off + t) % ring for t in range(T)]
    return np.asarray(out, dtype=np.int64)


def csr_of(idx, n_dst):
    """the transpose of a gather index -> (csr_off int32 [n_dst + 1], csr_idx int32 [len(idx)]), contributors ascending"""
    rows = [[] for _ in range(n_dst)]
    for k, u in enumerate(int(v) for v in idx):
        rows[u].append(k)
    off = np.zeros(n_dst + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(r) for r in rows])
    return off, np.asarray([k for r in rows for k in r], dtype=np.int32)


def gather_sum_rows_ref(src, csr_off, csr_idx, defect=None):
    """numpy float32, ascending k from +0 -> [n_dst, words]; an index outside the source is skipped"""
    src = np.ascontiguousarray(src, dtype=np.float32).reshape(src.shape[0], -1)
    off, idx = np.asarray(csr_off, dtype=np.int64), np.asarray(csr_idx, dtype=np.int64)
    n_dst = off.size - 1
    out = np.zeros((n_dst, src.shape[1]), dtype=np.float32)
    for u in range(n_dst):
        v = min(u + 1, n_dst - 1) if defect == "next_row" else u
        k0, k1 = int(off[v]), int(off[v + 1])
        if defect == "drop_last" and k1 > k0:
            k1 -= 1
        for k in range(k0, k1):
            if 0 <= idx[k] < src.shape[0]:
                out[u] = out[u] + src[idx[k]]
    return out


# ------------------------------------------------------------------------------------------------ tracks and the oracle
def make_track(n_frames, N, C, seed, cards=(1, 2, 31, 32)):
    """A processed track [n_frames, N, C] fp32 (numpy) whose frames are repeat-padded from ``cards`` detections, then a
    synthetic raw track's (some with more than N detections: subsampled) -> (raw frames, host picks, the track)"""
    rng = np.random.default_rng(seed)
    lead = [RU.make_frame(rng, c) for c in cards]
    raw = lead + syn.synthetic_raw_track(seed + 70, n_frames - len(lead), max_points=2 * N - 4)
    np.random.seed(seed + 21)
    picks = datasets.draw_picks(RU.cards_of(raw), N)
    return raw, picks, RU.padded_frames64(raw, picks, C).astype(np.float32)


def crops_of(track, T, hop, W):
    """the W materialised windows of a track [F, N, C] -> point-major crops [W, T, N, C]"""
    return np.stack([track[j * hop:j * hop + T] for j in range(W)])


def compact_of(track):
    """the compact table of padded frames [F, N, C] on the host: rows equal iff their bits are, order of first occurrence
    -> (rows [M, C], weight [M], u_off [F + 1], inverse [F * N]: the compact row of every padded row)"""
    rows, weight, u_off, inverse = [], [], [0], []
    for fr in np.asarray(track):
        keys = [r.tobytes() for r in fr]
        first = {}
        for i, k in enumerate(keys):
            first.setdefault(k, len(first))
        cnt = np.zeros(len(first))
        for k in keys:
            cnt[first[k]] += 1
        order = sorted(first, key=first.get)
        rows += [fr[keys.index(k)] for k in order]
        weight += list(cnt)
        inverse += [u_off[-1] + first[k] for k in keys]
        u_off.append(u_off[-1] + len(first))
    return np.asarray(rows), np.asarray(weight), np.asarray(u_off, dtype=np.int64), np.asarray(inverse, dtype=np.int64)


def oracle_point_net(sd, pts):
    """the oracle's eval PointNet block on point rows [R, C] (fp64 tensor, differentiable) -> [R, 1024]"""
    return O.pointnet_block(pts.t()[None, :, None, :], sd, "pc_block.", False)[0, :, 0, :].t()


def oracle_windows(sd, windows, head):
    """the oracle's eval temporal block, mean over T and heads on windows [W, T, 1024] -> (logits, sup_fv)"""
    x4 = O.temporal_block(windows.permute(0, 2, 1), sd, "tc_block.", False).mean(dim=2)
    fv = O.elu(O.linear(x4, sd["MLP_sup1.0.weight"], sd["MLP_sup1.0.bias"]))
    h = O.elu(O.linear(fv, sd["MLP_head.0.weight"], sd["MLP_head.0.bias"])) if head else fv
    return O.elu(O.linear(h, sd["MLP_sup2.0.weight"], sd["MLP_sup2.0.bias"])), fv
