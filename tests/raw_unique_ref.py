"""fp64 references, gates and case lists of the padding-free raw path: ``ops.frames_from_raw_unique`` (csrc/raw_frames.hip),
``ops.segment_weighted_mean`` (csrc/segment_pool.hip), ``functional.encoder_frame_features_ragged`` and the scorers'
``dedup_points``.  Used by tests/test_raw_unique_branches.py (the kernels, on the GPU) and tests/test_raw_unique_gates_cpu.py
(the identity and the gates' power, on the CPU).  numpy / torch on the host only.

The identity
------------
In eval mode BatchNorm is a fixed per-channel affine map, so the per-point network f is a pure function of the point.  A
padded frame repeats detections (``process_track``: ``concat(arr, arr[choice(card, N - card)])``), hence

    mean over the N padded rows of f(row)  =  (1 / N) sum_i m_i f(p_i)

over the DISTINCT picked detections p_i with multiplicities m_i.  The centring mean (and std) are statistics of the padded
frame; every copy of a point is centred identically, so the compact rows are rows of the padded frame.

The compact table (``compact_plan``)
------------------------------------
Frame f owns ``u_cnt[f] = min(card_f, N)`` rows from ``u_off[f]`` on; a frame whose offsets are bad (card < 1 or > 1024,
offsets outside [0, P]) owns one.  Its rows are its distinct picks in order of first occurrence in the pick row
(``np.unique(return_index, return_counts)`` re-ordered by the index), weight = the count; rows of the allotment the picks
leave unused and the rows from ``u_off[n]`` on are zero with weight 0.  A bad frame (a supplied pick outside [0, card)
included) is ONE zero row of weight N: pooled, f(0), what the padded path's all-zero frame gives.

The pool gate (``pool_gate``), u = 2^-24
---------------------------------------
The kernel adds a segment's R rows in fp32 in a fixed order (four row lanes, each ascending with one fused multiply-add per
row, the lanes added in order, one division by N).  Any fixed-order fp32 sum of R terms with at most R - 1 additions on a
path, each product rounded (m_r a_r: m_r an integer, one rounding, or none inside an fma) errs by at most
(R - 1 + 1) u sum|m_r a_r| to first order; the issue's form leaves two more roundings of slack and adds the final division:

    |err| <= (R + 2) u (1 / N) sum_r |m_r a_r|  +  u |result|

bf16 input adds nothing: the reference takes the bf16 values as given.  With (scale, shift) the kernel evaluates
v = ELU(fma(y, scale, shift)) in fp32 before it sums, and the reference does so in fp64 from the same y, scale, shift:
z_hat = fma(...) is z (1 + d), |d| <= u (one rounding); ELU is 1-Lipschitz, so that moves v by at most u |z|; expm1f is
documented to 1 ulp by the device library and 2 u |v| is allowed for it (ELU_ULPS).  Each row's |m_r| (u |z_r| + 2 u |v_r|)
/ N is added to the gate; the sum term then uses the fp64 |v_r|.

The scorer gates
----------------
``sup_fv``: the mode's parity gate (fp32 1e-4, bf16 5e-2: DESIGN.md section 2, tests/test_round2_parity.py) times the
other side's largest |sup_fv|.  ``lik`` = (1/K) sum_k exp(-0.5 (D log 2 pi + |x - mu_k|^2)): moving every component of x
by at most g changes |x - mu_k|^2 by at most 2 g |x - mu_k|_1 + D g^2, so every term, and the sum, changes by a factor
inside exp(+-E), E = max_k (g |x - mu_k|_1 + D g^2 / 2): |lik' - lik| <= (exp(E) - 1) lik (``lik_rel_bound``), plus
1e-12 lik for the fp64 evaluation.  ``preds`` / ``votes``: equal wherever the fp64 oracle's top-2 logit margin exceeds twice
the logit gate (gate x the oracle's largest |logit|); at most 10 % of the windows may fall under that rule.

Planted defects: ``DEFECTS``; ``defect=`` of ``compact_plan`` / ``weighted_pool`` returns what a subtly wrong kernel gives.
"""
import numpy as np
import torch

from opensetgaitrecognition_pcaa_amd import datasets
from oracle import pcaa_oracle as O

U = 2.0 ** -24
ELU_ULPS = 2.0
RAW_MAX_CARD = 1024
MODE_GATE = {"fp32": 1e-4, "bf16": 5e-2}
MAX_EXCLUDED = 0.10
DEFECTS = ("mult_off_by_one", "raw_order", "no_inv_n", "bad_frame_zero")

# cardinalities that hit every branch at N = 32: repeat-pad from one and two points, one short of N, exactly N (a
# permutation: every weight 1), subsampling from N + 1, 60 and the cap
CARDS_N32 = (1, 2, 31, 32, 33, 60, 1024)


def make_frame(rng, n):
    """one raw frame of n detections, the layout of synthetic.synthetic_raw_track"""
    return {"cardinality": np.array([n]), "elements": rng.standard_normal((n, 2)) * 0.4 + rng.standard_normal(2),
            "z_coord": rng.standard_normal(n) * 0.5 + 1.0, "dopplers": rng.standard_normal(n) * 0.8,
            "powers": np.exp(rng.standard_normal(n) * 1.5)}


def cards_of(raw):
    return np.array([len(fr["z_coord"]) for fr in raw])


def unique_first(pick_row):
    """-> (positions of the first occurrences, ascending; the multiplicity of the detection at each)"""
    _, index, counts = np.unique(np.asarray(pick_row), return_index=True, return_counts=True)
    order = np.argsort(index)
    return index[order], counts[order]


def offsets_bad(off0, off1, P):
    card = off1 - off0
    return off0 < 0 or off1 > P or card < 1 or card > RAW_MAX_CARD


def compact_plan(offsets, P, picks, N, M, defect=None):
    """Host restatement of the compact table's layout -> ``(u_off int32 [n + 1], weight fp32 [M], src int64 [M])``:
    row r of the table is row ``src[r]`` of the padded frames viewed as [n N, C] (``src[r] = -1``: a zero row)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    n = offsets.size - 1
    u_off = np.zeros(n + 1, dtype=np.int64)
    weight = np.zeros(M, dtype=np.float32)
    src = np.full(M, -1, dtype=np.int64)
    for f in range(n):
        off0, off1 = int(offsets[f]), int(offsets[f + 1])
        bad = offsets_bad(off0, off1, P)
        card = 1 if bad else off1 - off0
        u_off[f + 1] = u_off[f] + min(card, N)
        row = None if picks is None else np.asarray(picks[f])
        bad = bad or (row is not None and ((row < 0) | (row >= card)).any())
        if bad:
            weight[u_off[f]] = N
            continue
        first, mult = unique_first(row)
        if defect == "raw_order" and card >= N:
            order = np.argsort(row[first], kind="stable")
            first, mult = first[order], mult[order]
        if defect == "mult_off_by_one":
            mult = mult.copy()
            mult[-1] += 1
        weight[u_off[f]:u_off[f] + first.size] = mult
        src[u_off[f]:u_off[f] + first.size] = f * N + first
    assert u_off[n] <= M, (u_off[n], M)
    return u_off.astype(np.int32), weight, src


def gather_rows(padded, src):
    """rows ``src`` of the padded frames [n, N, C] (any float dtype), zero rows where ``src < 0``"""
    flat = np.asarray(padded).reshape(-1, padded.shape[-1])
    out = np.zeros((src.size, flat.shape[1]), dtype=flat.dtype)
    out[src >= 0] = flat[src[src >= 0]]
    return out


def padded_frames64(raw, picks, C, div=False):
    """``datasets.frames_from_picks``: the fp64 row values"""
    return datasets.frames_from_picks(raw, picks, C, div)


def elu64(z):
    return np.where(z > 0, z, np.expm1(np.minimum(z, 0.0)))


def weighted_pool(a, weight, u_off, N, scale=None, shift=None, defect=None):
    """fp64: out[f] = (1 / N) sum_{r in [u_off[f], u_off[f + 1])} weight[r] v(a[r]) -> (out [n, ch], the gate [n, ch]);
    a segment outside [0, M] (or running backwards) is zero with a zero gate."""
    a = np.asarray(a, dtype=np.float64)
    w = np.asarray(weight, dtype=np.float64)
    u_off = np.asarray(u_off, dtype=np.int64)
    M, ch = a.shape
    n = u_off.size - 1
    if scale is not None:
        z = a * np.asarray(scale, dtype=np.float64) + np.asarray(shift, dtype=np.float64)
        v = elu64(z)
        own = U * np.abs(z) + ELU_ULPS * U * np.abs(v)
    else:
        v, own = a, np.zeros_like(a)
    out, gate = np.zeros((n, ch)), np.zeros((n, ch))
    inv = 1.0 if defect == "no_inv_n" else 1.0 / N
    for f in range(n):
        u0, u1 = int(u_off[f]), int(u_off[f + 1])
        if u0 < 0 or u1 < u0 or u1 > M:
            continue
        R = u1 - u0
        wr = w[u0:u1, None]
        out[f] = (wr * v[u0:u1]).sum(axis=0) * inv
        gate[f] = ((R + 2) * U * (np.abs(wr * v[u0:u1])).sum(axis=0) + (np.abs(wr) * own[u0:u1]).sum(axis=0)) / N \
            + U * np.abs(out[f])
    return out, gate


def ratio(got, want, gate):
    """largest |got - want| / gate; an element with a zero gate must be exact"""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    if ((gate == 0) & (err != 0)).any():
        return np.inf
    return float((err / np.where(gate > 0, gate, 1.0)).max()) if err.size else 0.0


# ---------------------------------------------------------------------------------------------------- the fp64 oracle
def sd64(enc):
    return {k: v.detach().cpu().double() for k, v in enc.state_dict().items()}


def oracle_point_features(sd, pts):
    """f(point) for every row of ``pts`` [R, C]: the oracle's eval PointNet block in fp64 -> [R, 1024]"""
    x = torch.as_tensor(np.asarray(pts), dtype=torch.float64).t()[None, :, None, :]        # [1, C, 1, R]
    with torch.no_grad():
        return O.pointnet_block(x, sd, "pc_block.", False)[0, :, 0, :].t().numpy()


def oracle_frame_features(sd, padded):
    """the oracle's pooled PointNet output of padded frames [n, N, C]: its x2 -> [n, 1024]"""
    padded = np.asarray(padded, dtype=np.float64)
    n, N, C = padded.shape
    return oracle_point_features(sd, padded.reshape(n * N, C)).reshape(n, N, -1).mean(axis=1)


def oracle_ragged_features(sd, rows, weight, u_off, N, bad_as_zero=False):
    """the weighted pool of the oracle's per-point activations on the compact rows -> [n, 1024]"""
    weight = np.asarray(weight, dtype=np.float64)
    if bad_as_zero:                                   # the planted defect: a bad frame (one zero row of weight N) pooled as 0
        rows = np.asarray(rows)
        weight = np.where((weight == N) & ~np.asarray(rows).any(axis=1), 0.0, weight)
    return weighted_pool(oracle_point_features(sd, rows), weight, u_off, N)[0]


def oracle_window_logits(sd, frame_feats, T, hop, head):
    """frame features [F, 1024] of one track -> the oracle's logits of its eager windows [W, K] (W = (F - T) // hop + 1)"""
    F = frame_feats.shape[0]
    if F < T:
        return np.zeros((0, sd["MLP_sup2.0.weight"].shape[0]))
    W = (F - T) // hop + 1
    x2 = torch.stack([torch.as_tensor(frame_feats[j * hop:j * hop + T]) for j in range(W)]).permute(0, 2, 1)   # [W, 1024, T]
    with torch.no_grad():
        x4 = O.temporal_block(x2, sd, "tc_block.", False).mean(dim=2)
        h = O.elu(O.linear(x4, sd["MLP_sup1.0.weight"], sd["MLP_sup1.0.bias"]))
        if head:
            h = O.elu(O.linear(h, sd["MLP_head.0.weight"], sd["MLP_head.0.bias"]))
        return O.elu(O.linear(h, sd["MLP_sup2.0.weight"], sd["MLP_sup2.0.bias"])).numpy()


def safe_windows(logits64, mode):
    """windows whose fp64 top-2 logit margin exceeds twice the logit gate -> bool [W]"""
    if logits64.shape[0] == 0:
        return np.zeros(0, bool)
    top = np.sort(logits64, axis=1)
    return (top[:, -1] - top[:, -2]) > 2 * MODE_GATE[mode] * np.abs(logits64).max()


def lik_rel_bound(sup_fv, means, g):
    """(exp(E) - 1) + 1e-12 per window, E = max_k (g |x - mu_k|_1 + D g^2 / 2): see the module docstring"""
    x = np.asarray(sup_fv, dtype=np.float64)
    mu = np.asarray(means, dtype=np.float64)
    l1 = np.abs(x[:, None, :] - mu[None]).sum(axis=2).max(axis=1)
    with np.errstate(over="ignore"):
        return np.expm1(g * l1 + 0.5 * x.shape[1] * g * g) + 1e-12
