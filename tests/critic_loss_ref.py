"""fp64 restatements of the operations of csrc/losses.hip, csrc/disc.hip, csrc/scoring.hip and csrc/orced.hip, the gate of
every output, the input conditions the gates need, and planted defects.

Used by tests/test_critic_loss_branches.py (the kernels, on the GPU) and tests/test_critic_loss_gates_cpu.py (the gates
themselves, on the CPU).  Plain torch and numpy, device-agnostic: a reference runs where its inputs live, in float64.
Inputs come from ``elementwise_ref.uniform``: the same bits on the CPU and on the device.  Kernel and reference get the
SAME stored fp32 values, so only the kernel's arithmetic separates them.  u = 2^-24 throughout.

Chamfer (``chamfer_ref``)
-------------------------
Reference: the direct form D(i, j) = sum_c (g_ic - p_jc)^2 in fp64; nearest neighbours with the lowest index on exact
ties (torch.min's documented rule, and the kernel's strict ``<``).

* distance gate.  The kernel evaluates |g|^2 + |p|^2 - 2 g.p over 8 padded channels.  Each of the three dot products is
  a chain of 8 fmas: <= 8 roundings, each relative to a partial sum bounded by the sum of the magnitudes, so 8u |g|^2,
  8u |p|^2 and 8u sum|g_c p_c|.  rg + rp rounds once (u (|g|^2 + |p|^2)), 2 dot is exact, the subtraction rounds once
  (u |P| <= u M) with M = |g|^2 + |p|^2 + 2 sum_c |g_c p_c| = sum_c (|g_c| + |p_c|)^2.  Together
  (8 + 1 + 1) u (|g|^2 + |p|^2) + (8 + 1) u 2 sum|g_c p_c| <= CH_C u M, CH_C = 10.
* loss gate.  min is 1-Lipschitz: |min_o P~_o - min_o P_o| <= the distance gate at the reference's choice (from above)
  or at the kernel's choice (from below); the kernel's choice is the reference's or a near tie, so an item's gate is the
  larger of the gates of its two closest candidates.  The frame's gate is the sum of its 2N items' gates plus the fp32
  summation in the kernel's order: a lane adds ceil(2N / 256) non-negative minima, wave_sum adds 6 levels, thread 0
  adds 4 waves: every addition rounds by at most u (the running sum) <= u loss, so (ceil(2N / 256) + 10) u loss.
* gradient gate.  dpred_j = sum over the m_j + 1 chosen partners of 2w (p_j - g): w = grad_scale * grad_per_b[b] rounds
  once, the difference once, the product once (2w is exact): 3u |term|; the m_j additions round by at most u sum|terms|
  each: (4 + m_j) u sum |2w (p_j - g)| is the worst case, which one evaluation can realise to 3/4 where m_j = 0.  The
  gate is twice that, CH_G (4 + m_j) with CH_G = 2, so that an evaluation which realises the count sits at half: with
  CH_G = 1 the fp32 torch evaluation of the CPU file reached 0.555 at (B, T, N, C) = (3, 2, 128, 4).
* unsettled prediction points.  The gradient jumps where an argmin changes.  An item (a prediction scanning ground
  truth, or a ground-truth point scanning predictions) is undecided when its closest candidate at DIFFERENT coordinates
  lies within the sum of the two distance gates of its nearest neighbour.  Prediction j is unsettled when item j is
  undecided, or when an undecided ground-truth point has j among its candidates (anything no further than its
  runner-up).  Unsettled points leave the gradient comparison only; the loss is compared in full.  CH_UNSETTLED_CAP =
  2 % is a condition on the inputs, asserted on the reference by the CPU file for every case.  Candidates at EQUAL
  coordinates (duplicates) do not unsettle anything: duplicated ground truth gives the same gradient whichever is
  chosen, duplicated predictions are compared summed over each duplicate set plus the lowest-index rule.

Cross-entropy (``ce_ref``)
--------------------------
fp64 logsumexp - x[t], softmax - onehot, argmax of the logits with the first index on ties.  Logits lie on the grid
2^-6, so the top-two gap of a row is 0 or >= 2^-6 > 1e-3 (``gap``; asserted) and ``preds`` must be equal.
s_k = x_k - max (one rounding: the exponential's argument moves by u |s_k|), expf good to 2 ulp = 4u, K additions:
rel(se) = u (K + 4 + A), A = sum_k softmax_k |s_k|.  Row loss = logf(se) + max - x_t: rel(se) + 4u |log se| (logf 2 ulp)
+ u |log se + max| + u |row loss|.  The rows meet in fp64; the mean is cast once: mean(row gates) + u |loss|.
Gradient gs (e_k inv - onehot) / B: e_k to u (|s_k| + 4), inv = 1 / se to rel(se) + u, the product u, the difference
u |p_k - onehot|, times gs, over B: four roundings of |p_k - onehot|.  As for the chamfer gradient, an evaluation can
realise such a short count almost in full, so both parts are doubled to put one that does at half (with the single count
the fp32 torch evaluation of the CPU file reached 0.54 at (B, K) = (600, 2)):
|gs| / B [2 p_k u (|s_k| + K + A + 10) + 8u |p_k - onehot|] + |gs| / B 2^-126 (a softmax value below the normal range
may be flushed to 0).

Critic and OR-CED: running error analysis (``EN``)
--------------------------------------------------
The reference is fp64 torch autograd (``disc_*_ref``, ``orced_*_ref``).  The issue's gate c u F_abs is evaluated by carrying,
beside every node's fp64 value v, a bound f on the fp32 evaluation's error in units of u through the kernel's own
expression tree (the closed forms of the kernels, written out below and checked against autograd by the CPU file):
    x * y     f = f_x |y| + |x| f_y + |xy|             x + y   f = f_x + f_y + |x + y|
    a . W (a chain of n fmas from a bias)            f = f_a |W| + |a| f_W + n (|a| |W| + |bias|)
    exp       f = e f_a + 4 e (expf: 2 ulp = 4u)       sqrt    f = f_a / (2 v) + v
    ELU(a)    f = ELU'(a) f_a + 4 (|h| + [a <= 0])     ELU'    f = ELU''(a) f_a + 4 ELU'     ELU'' likewise
    a column summed over rows in fp64 and cast once  f = sum f + |v|
That IS the expression tree with every weight, input and upstream gradient replaced by its magnitude and ELU', ELU''
kept at their values -- F_abs -- with c applied node by node instead of once: c is each node's own rounding count (n for
a chain of n fmas, at most 64 for W2's rows and W1's columns, 65 for W1's rows at K = 32; 1 for a product or a sum; 4
for expf / expm1f).  One more term than the issue lists: ELU' and ELU'' are functions of the pre-activation and inherit
its error (ELU'' f_a above), without which a pre-activation with |a| |W| >> 1 would be held to a bound its derivative
cannot meet.  u f is the worst case, first order in u: every rounding at its bound and all of them aligned.  Through
three layers and up to ten chained dot products that is 10^3 .. 10^5 u, where an fp32 evaluation realises ~10 u, and
a gate that wide lets planted defects through (the (1 - alpha) missing from dz moved 1.6 % of dz by ten gates, the missing
penalty outer products 33 % of dW1).  So every node also carries q, the SUM OF THE SQUARES of the
same terms (x * y: q = q_x y^2 + x^2 q_y + (xy)^2; a chain of n fmas: q = q_a W^2 + a^2 q_W + n (|a| |W| + |bias|)^2;
and so on, rule by rule).  A rounding error is at most u |x| and, taken as uniform, has standard deviation u |x| / sqrt 3;
an output's error is the sum of many of them, so under independence (the model of Higham and Mary, "A new approach to
probabilistic rounding error analysis", 2019) its standard deviation is at most u sqrt(q / 3).  The gate is
    u min(2 f, LAMBDA sqrt q),   LAMBDA = 8:
13.8 standard deviations under independence, still 8 where a node that is used three times over correlates its terms
fully (sqrt 3), and never wider than twice the worst case.  Twice, because a short count (an output that is two or
three roundings away from its inputs) is realised almost in full by one evaluation, which then has to sit at half:
with 1 f the fp32 torch evaluation of the CPU file reached 0.73 (d_mu of orced_kl: three roundings) and 0.61 (dWc of
the OR-CED heads at B = 3).  Neither figure comes from a kernel's output.
ELU'' jumps at 0: every critic case satisfies min |pre-activation| >= DISC_MIN_PRE = 1e-3 over all units, rows and passes
with both signs present in both layers (``disc_case`` draws candidate rows and keeps the first B that satisfy it; the
condition is asserted on the reference).  No element is excluded.  db3 of the WGAN-GP step is exactly 0.
OR-CED's backward receives logvar and sup_fv as stored fp32: the reference differentiates the whole expression in fp64
and the kernel gets the reference's values rounded once, which the gate carries as f = |v| on those inputs.

Scoring
-------
``joint_likelihood_ref``: np.longdouble where it is wider than double, else math.fsum over exact products.  The kernel's
argument a_k = -0.5 (D log 2pi + |x - mu_k|^2): the differences of fp32 values are exact in fp64, D squares and D
additions, the constant (rounded to double) times D, one sum: |da_k| <= (D + 4) 2^-53 |a_k| (all terms share a sign).
exp turns that into a relative error and adds its own (<= 2 ulp = 4 2^-53), the K positive terms add (K 2^-53), the
division by K rounds: gate = sum_k t_k ((D + 4) |a_k| + 4) 2^-53 / K + (K + 1) 2^-53 lik + (K + 2) 2^-1074 (each
denormal term is on a grid of 2^-1074, and so is the result).
``kvote_ref``: oracle.k_vote.  ``stream_ref``: per stream, its windows over all ticks concatenated, then the fp64 argmax,
``joint_likelihood_ref`` and oracle.k_vote -- no sibling kernel.

Planted defects
---------------
``defect=`` returns what a subtly wrong kernel would have produced (names: the ``*_DEFECTS`` tuples).  The CPU file
shows each moves >= 80 % of the elements it touches by more than 10 x the gate; for the integer outputs of the vote a
touched element is a moved one.
"""
import math

import numpy as np
import torch

from elementwise_ref import U, f32, moved, ratio, seed_of, uniform  # noqa: F401  (re-exported for the two test files)

CH_C = 10
CH_G = 2
CH_UNSETTLED_CAP = 0.02
DISC_MIN_PRE = 1e-3
CE_GRID = 2.0 ** -6
U64 = 2.0 ** -53

CHAMFER_DEFECTS = ("drop_dir2_grad", "skip_last_gt", "pad_nonzero", "swap_bt", "next_b_grad")
CE_DEFECTS = ("drop_rows_ge_256", "mean_over_256", "max_skip_last")
DISC_DEFECTS = ("elu_pp_wrong_side", "label_shift", "w1_pitch_odd", "dz_no_1_minus_alpha", "gp_outer_missing", "alpha_next_row")
SCORING_DEFECTS = ("fp32_maha", "d_fixed_32", "no_1_over_k", "ge_threshold", "lt_half", "highest_on_ties")
ORCED_DEFECTS = ("std_half_dropped", "dmu_reads_dlv_row", "bias_last_row_missing")


# ====================================================================================================== chamfer
def chamfer_inputs(B, T, N, C, device="cpu", dup=None):
    """fp32 (preds, gts) [B, C, T, N] in [-1, 1).  dup="gt": every third ground-truth point repeats its predecessor;
    dup="pred": every fourth prediction repeats the one two before it"""
    seed = seed_of(N, 1000 * C + 10 * B + T)
    n = B * C * T * N
    preds = uniform(n, seed, device, -1.0, 1.0).view(B, C, T, N).float()
    gts = uniform(n, seed + 1, device, -1.0, 1.0).view(B, C, T, N).float()
    if dup == "gt" and N >= 3:
        gts[..., 2::3] = gts[..., 1:N - 1:3][..., : gts[..., 2::3].shape[-1]]
    if dup == "pred" and N >= 4:
        preds[..., 3::4] = preds[..., 1:N - 2:4][..., : preds[..., 3::4].shape[-1]]
    return preds.contiguous(), gts.contiguous()


def chamfer_grad_per_b(B, device="cpu"):
    return uniform(B, 77, device, 0.5, 1.5).float()


def _take(M, idx, dim):
    """M [B,T,N,N]: the entries at ``idx`` [B,T,N] along ``dim`` (2: out[j] = M[idx[j], j]; 3: out[i] = M[i, idx[i]])"""
    return M.gather(dim, idx.unsqueeze(dim)).squeeze(dim)


def chamfer_ref(preds, gts, grad_scale=1.0, grad_per_b=None, defect=None):
    """preds, gts: logical [B, C, T, N] fp32 (any strides) -> dict:
    loss, loss_gate [B, T];  nn_pred [B, T, N] (ground-truth index chosen by prediction j), nn_gt (prediction chosen by
    ground-truth point i);  grad, grad_gate [B, C, T, N];  margin_pred, margin_gt (distance to the closest candidate at
    other coordinates minus the nearest distance);  unsettled [B, T, N] bool (prediction points)"""
    p = preds.double().permute(0, 2, 3, 1).contiguous()            # [B, T, N, C]
    g = gts.double().permute(0, 2, 3, 1).contiguous()
    B, T, N, C = p.shape
    pd, gd = p, g
    if defect == "pad_nonzero" and C < 8:                          # channel C of the ground truth holds a neighbour's channel 0
        gd = torch.cat([g, g[..., :1].roll(1, dims=2)], -1)
        pd = torch.cat([p, torch.zeros_like(p[..., :1])], -1)
    D = ((gd.unsqueeze(3) - pd.unsqueeze(2)) ** 2).sum(-1)         # [B, T, i (gt), j (pred)]
    G = CH_C * U * ((g.abs().unsqueeze(3) + p.abs().unsqueeze(2)) ** 2).sum(-1)
    D1 = D
    if defect == "skip_last_gt" and N >= 2:
        D1 = D.clone()
        D1[:, :, N - 1, :] = float("inf")
    inf = float("inf")
    d_pred, nn_pred = D1.min(dim=2)                                 # per prediction j
    d_gt, nn_gt = D.min(dim=3)                                      # per ground-truth point i
    same_g = (g.unsqueeze(3) == g.unsqueeze(2)).all(-1)            # [B, T, i, i']
    same_p = (p.unsqueeze(3) == p.unsqueeze(2)).all(-1)
    # the closest candidate at other coordinates than the chosen one
    eq1 = same_g.gather(3, nn_pred.unsqueeze(2).expand(B, T, N, N))          # [i, j] = same_g[i, nn_pred[j]]
    r_pred_d, r_pred = D.masked_fill(eq1, inf).min(dim=2)
    eq2 = same_p.gather(2, nn_gt.unsqueeze(3).expand(B, T, N, N))            # [i, j] = same_p[nn_gt[i], j]
    r_gt_d, r_gt = D.masked_fill(eq2, inf).min(dim=3)
    g_pred, g_pred_r = _take(G, nn_pred, 2), _take(G, r_pred, 2)
    g_gt, g_gt_r = _take(G, nn_gt, 3), _take(G, r_gt, 3)
    und_pred = (r_pred_d - d_pred) <= g_pred + g_pred_r
    und_gt = (r_gt_d - d_gt) <= g_gt + g_gt_r
    unsettled = und_pred | (und_gt.unsqueeze(3) & (D <= r_gt_d.unsqueeze(3))).any(2)
    ig_pred = torch.maximum(g_pred, torch.where(r_pred_d < inf, g_pred_r, g_pred))
    ig_gt = torch.maximum(g_gt, torch.where(r_gt_d < inf, g_gt_r, g_gt))
    item_gates = ig_pred.sum(-1) + ig_gt.sum(-1)
    loss = d_pred.sum(-1) + d_gt.sum(-1)
    loss_gate = item_gates + (-(-2 * N // 256) + 10) * U * loss
    if defect == "swap_bt":                                         # frame f reads (b, t) = (f % B, f / B)
        f = torch.arange(B * T, device=loss.device)
        loss = loss[f % B, f // B].view(B, T)
    # gradient
    w = torch.full((B,), f32(grad_scale), dtype=torch.float64, device=p.device)
    if grad_per_b is not None:
        gpb = grad_per_b.double()
        w = w * (gpb.roll(-1) if defect == "next_b_grad" else gpb)
    w = w.view(B, 1, 1, 1)
    ix = lambda idx: idx.unsqueeze(-1).expand(B, T, N, C)
    t1 = p - g.gather(2, ix(nn_pred))
    t2 = p.gather(2, ix(nn_gt)) - g                                 # [B, T, i, C]: the term ground-truth point i sends to nn_gt[i]
    s2 = torch.zeros_like(p).scatter_add_(2, ix(nn_gt), t2)
    m2 = torch.zeros_like(p).scatter_add_(2, ix(nn_gt), t2.abs())
    cnt = torch.zeros_like(p).scatter_add_(2, ix(nn_gt), torch.ones_like(p))
    if defect == "drop_dir2_grad":
        s2 = torch.zeros_like(s2)
    grad = 2 * w * (t1 + s2)
    grad_gate = CH_G * U * (4 + cnt) * 2 * w.abs() * (t1.abs() + m2)
    back = lambda x: x.permute(0, 3, 1, 2).contiguous()
    return {"loss": loss, "loss_gate": loss_gate, "nn_pred": nn_pred, "nn_gt": nn_gt, "grad": back(grad),
            "grad_gate": back(grad_gate), "margin_pred": r_pred_d - d_pred, "margin_gt": r_gt_d - d_gt,
            "unsettled": unsettled, "d_pred": d_pred, "d_gt": d_gt, "item_gate_pred": ig_pred, "item_gate_gt": ig_gt,
            "same_pred": same_p}


def settled_mask(ref):
    """bool [B, C, T, N]: the gradient elements that are compared"""
    C = ref["grad"].shape[1]
    return (~ref["unsettled"]).unsqueeze(1).expand(-1, C, -1, -1)


def duplicate_set_sums(grad, same_pred):
    """grad [B, C, T, N] summed over each set of predictions at equal coordinates (every member carries its set's sum)"""
    return torch.einsum("btjk,bctk->bctj", same_pred.double(), grad.double())


# ====================================================================================================== cross-entropy
def ce_inputs(B, K, mag=4.0, device="cpu"):
    """fp32 logits [B, K] on the grid 2^-6 in [-mag, mag], int64 targets.  Rows r % 5 == 2 are all equal, rows r % 5 == 4
    carry two equal maxima (classes 0 and K - 1: the first must win)"""
    seed = seed_of(B, K + 131 * int(mag))
    x = torch.round(uniform(B * K, seed, device, -mag, mag).view(B, K) / CE_GRID) * CE_GRID
    r = torch.arange(B, device=device)
    x[r % 5 == 2] = x[r % 5 == 2][:, :1]
    top = x.max(1).values + 0.5
    two = r % 5 == 4
    x[two, 0] = top[two]
    x[two, K - 1] = top[two]
    return x.float().contiguous(), ((r * 7 + 3) % K).long()


def ce_ref(logits, target=None, grad_scale=1.0, defect=None):
    """-> dict(loss, loss_gate (0-d); grad, grad_gate [B, K]; preds [B]; gap [B]: top-two gap of every row)"""
    x = logits.double()
    B, K = x.shape
    gs = f32(grad_scale)
    mx = x.max(1, keepdim=True).values
    if defect == "max_skip_last" and K >= 2:
        # the shift no longer bounds the exponent: fp32 expf overflows where the last class leads by more than 88.7
        mx = x[:, : K - 1].max(1, keepdim=True).values
    s = x - mx
    e = torch.exp(s.float()).double() if defect == "max_skip_last" else torch.exp(s)
    se = e.sum(1, keepdim=True)
    p = torch.nan_to_num(e / se, nan=float("inf"))
    srt = x.sort(1, descending=True).values
    ismax = x == x.max(1, keepdim=True).values
    # (torch.argmax does not promise the first index on ties: the lowest index among the maxima)
    out = {"preds": torch.where(ismax, torch.arange(K, device=x.device).expand(B, K), K).min(1).values,
           "gap": (srt[:, 0] - srt[:, 1]) if K > 1 else torch.full((B,), float("inf"), dtype=torch.float64, device=x.device)}
    if target is None:
        return out
    oh = torch.nn.functional.one_hot(target, K).double()
    A = (p * s.abs()).sum(1, keepdim=True)
    rel_se = U * (K + 4 + A)
    lse = torch.log(se)
    row = (lse + mx - (x * oh).sum(1, keepdim=True)).squeeze(1)
    row_gate = (rel_se + U * (4 * lse.abs() + (lse + mx).abs())).squeeze(1) + U * row.abs()
    denom = B
    keep = torch.ones(B, dtype=torch.float64, device=x.device)
    if defect == "drop_rows_ge_256":
        keep[256:] = 0.0
    if defect == "mean_over_256":
        denom = 256
    out["loss"] = (row * keep).sum() / denom
    out["loss_gate"] = row_gate.mean() + U * out["loss"].abs()
    out["grad"] = gs * (p - oh) / denom
    out["grad_gate"] = abs(gs) / B * (U * (2 * p * (s.abs() + K + A + 10) + 8 * (p - oh).abs()) + 2.0 ** -126)
    return out


# ====================================================================================================== running error
LAMBDA = 8.0


class EN:
    """a node: value ``v``; ``f``, the worst-case bound on the fp32 evaluation's error in units of u; ``q``, the sum of the
    squares of the same error terms in units of u^2 (module docstring)"""
    __slots__ = ("v", "f", "q")

    def __init__(self, v, f=None, q=None):
        self.v = v
        self.f = torch.zeros_like(v) if f is None else f
        self.q = torch.zeros_like(v) if q is None else q

    @property
    def T(self):
        return EN(self.v.t(), self.f.t(), self.q.t())

    def __getitem__(self, k):
        return EN(self.v[k], self.f[k], self.q[k])

    def view(self, *shape):
        return EN(self.v.reshape(*shape), self.f.reshape(*shape), self.q.reshape(*shape))


def en_rounded(v):
    """an input that was rounded to fp32 once on its way to the kernel"""
    return EN(v, v.abs(), v * v)


def en_cat(a, b):
    return EN(torch.cat([a.v, b.v], 1), torch.cat([a.f, b.f], 1), torch.cat([a.q, b.q], 1))


def mul(a, b):
    v = a.v * b.v
    return EN(v, a.f * b.v.abs() + a.v.abs() * b.f + v.abs(), a.q * b.v ** 2 + a.v ** 2 * b.q + v ** 2)


def div(a, b):
    v = a.v / b.v
    return EN(v, a.f / b.v.abs() + v.abs() * b.f / b.v.abs() + v.abs(), a.q / b.v ** 2 + v ** 2 * b.q / b.v ** 2 + v ** 2)


def add(a, b, sign=1.0):
    v = a.v + sign * b.v
    return EN(v, a.f + b.f + v.abs(), a.q + b.q + v ** 2)


def sub(a, b):
    return add(a, b, -1.0)


def scale(a, k):
    """times a power of two (or a sign): exact"""
    return EN(a.v * k, a.f * abs(k), a.q * k * k)


def const(x, like):
    return EN(torch.as_tensor(float(x), dtype=like.v.dtype, device=like.v.device))


def mm(a, w, n=None, bias=None):
    """a [B, n] . w [n, m] as a chain of ``n`` fmas (starting from ``bias``): every one of the n roundings is relative to
    a partial sum no larger than the sum of the magnitudes"""
    n = a.v.shape[-1] if n is None else n
    v = a.v @ w.v
    mag = a.v.abs() @ w.v.abs()
    f = a.f @ w.v.abs() + a.v.abs() @ w.f
    q = a.q @ w.v ** 2 + a.v ** 2 @ w.q
    if bias is not None:
        v, mag, f, q = v + bias.v, mag + bias.v.abs(), f + bias.f, q + bias.q
    return EN(v, f + n * mag, q + n * mag ** 2)


def _sum64(x, *dims):
    """a sum the kernels accumulate in fp64 and cast once"""
    return x.double().sum(*dims).to(x.dtype)


def tmm(a, b, n=0):
    """a^T . b over the rows.  n = 0: products and sums in fp64, one cast; else a chain of n fp32 fmas"""
    v = (a.v.double().t() @ b.v.double()).to(a.v.dtype) if n == 0 else a.v.t() @ b.v
    f = a.f.t() @ b.v.abs() + a.v.abs().t() @ b.f
    q = a.q.t() @ b.v ** 2 + (a.v ** 2).t() @ b.q
    mag = a.v.abs().t() @ b.v.abs()
    return EN(v, f + (v.abs() if n == 0 else n * mag), q + (v ** 2 if n == 0 else n * mag ** 2))


def colsum(a, n=0):
    v = _sum64(a.v, 0) if n == 0 else a.v.sum(0)
    mag = a.v.abs().sum(0)
    return EN(v, a.f.sum(0) + (v.abs() if n == 0 else n * mag), a.q.sum(0) + (v ** 2 if n == 0 else n * mag ** 2))


def rowsum(a, n):
    """sum over the last dimension with ``n`` fp32 additions on the longest path"""
    mag = a.v.abs().sum(-1, keepdim=True)
    return EN(a.v.sum(-1, keepdim=True), a.f.sum(-1, keepdim=True) + n * mag, a.q.sum(-1, keepdim=True) + n * mag ** 2)


def plus(a, b):
    """two fp64 partial sums of one accumulator: no rounding of its own"""
    return EN(a.v + b.v, a.f + b.f, a.q + b.q)


def en_exp(a):
    v = torch.exp(a.v)
    return EN(v, v * a.f + 4 * v, v ** 2 * a.q + 16 * v ** 2)


def en_sqrt(a):
    v = torch.sqrt(a.v)
    return EN(v, a.f / (2 * v) + v, a.q / (4 * v ** 2) + v ** 2)


def en_elu(a, wrong_side=False):
    """-> (ELU, ELU', ELU'') of the pre-activation ``a``"""
    pos = a.v > 0
    ex = torch.exp(a.v)
    one, zero = torch.ones_like(ex), torch.zeros_like(ex)
    e = torch.where(pos, one, ex)
    epp = torch.where(pos, zero, ex)
    h = torch.where(pos, a.v, torch.expm1(a.v))
    own = h.abs() + (~pos).to(ex.dtype)
    f, q = epp * a.f + 4 * epp, epp ** 2 * a.q + 16 * epp ** 2        # of ELU' and of ELU'' alike (both are e^a for a <= 0)
    return (EN(h, e * a.f + 4 * own, e ** 2 * a.q + 16 * own ** 2), EN(e, f, q),
            EN(torch.where(pos, e, zero) if wrong_side else epp, f.clone(), q.clone()))


def gate_of(node, floor=0.0):
    """min(twice the worst case, LAMBDA x the root of the sum of squares) x u"""
    return U * torch.minimum(2 * node.f.double(), LAMBDA * node.q.double().clamp_min(0).sqrt()) + floor


# ====================================================================================================== critic
XD, H1, H2 = 32, 64, 32


def disc_params(K, device="cpu"):
    """fp32 [W1 [64, 32 + K], b1, W2 [32, 64], b2, W3 [1, 32], b3 [1]]"""
    IN, seed = XD + K, 500 + K
    r = lambda n, s, a: uniform(n, seed + s, device, -a, a).float()
    return [r(H1 * IN, 0, 1.5 / IN ** 0.5).view(H1, IN), r(H1, 1, 0.5), r(H2 * H1, 2, 1.5 / 8).view(H2, H1), r(H2, 3, 0.5),
            r(H2, 4, 0.6).view(1, H2), r(1, 5, 0.5)]


def _pre(u, P):
    a1 = u @ P[0].t() + P[1]
    h1 = torch.where(a1 > 0, a1, torch.expm1(a1))
    a2 = h1 @ P[2].t() + P[3]
    return a1, a2


def disc_case(B, K, dense=False, device="cpu"):
    """dict(params, x = z, fv, label, alphas, gout, gbar, min_pre, signs): rows drawn from 4B + 16 candidates, the first B
    whose pre-activations (at z, at fv and at the interpolate) all keep DISC_MIN_PRE from 0"""
    P = disc_params(K, device)
    P64 = [p.double() for p in P]
    M = 4 * B + 16
    seed = seed_of(B, K + (50 if dense else 0))
    z = uniform(M * XD, seed, device, -1.5, 1.5).view(M, XD).float()
    fv = uniform(M * XD, seed + 1, device, -1.5, 1.5).view(M, XD).float()
    al = uniform(M, seed + 2, device, 0.0, 1.0).float()
    if K == 0:
        lab = torch.zeros((M, 0), dtype=torch.float32, device=device)
    elif dense:
        lab = uniform(M * K, seed + 3, device, 0.0, 1.0).view(M, K).float()
    else:
        lab = torch.nn.functional.one_hot((torch.arange(M, device=device) * 5 + 1) % K, K).float()
    interp = z.double() + al.double().view(M, 1) * (fv.double() - z.double())
    pres = [torch.cat(_pre(torch.cat([v.double(), lab.double()], 1), P64), 1) for v in (z, fv, interp.float())] + \
        [torch.cat(_pre(torch.cat([interp, lab.double()], 1), P64), 1)]
    allpre = torch.stack(pres)                                              # [4, M, 96]
    ok = (allpre.abs().amin((0, 2)) >= DISC_MIN_PRE).nonzero().flatten()[:B]
    assert ok.numel() == B, "disc_case: not enough candidate rows keep their pre-activations from 0"
    sel = allpre[:, ok]
    signs = all(bool((sel[..., a:b] > 0).any()) and bool((sel[..., a:b] < 0).any()) for a, b in ((0, H1), (H1, H1 + H2)))
    return {"params": P, "x": z[ok].contiguous(), "fv": fv[ok].contiguous(), "label": lab[ok].contiguous(),
            "alphas": al[ok].contiguous(), "gout": uniform(B, seed + 4, device, -1.0, 1.0).float(),
            "gbar": uniform(B * XD, seed + 5, device, -1.0, 1.0).view(B, XD).float(),
            "min_pre": float(sel.abs().min()), "signs": signs, "B": B, "K": K}


def _leaves(ts):
    return [t.detach().double().clone().requires_grad_(True) for t in ts]


def disc_D(x, label, P):
    u = torch.cat([x, label], 1)
    elu = lambda a: torch.where(a > 0, a, torch.expm1(a))
    return elu(elu(u @ P[0].t() + P[1]) @ P[2].t() + P[3]) @ P[4].t() + P[5]


def disc_forward_ref(x, label, P):
    return disc_D(x.double(), label.double(), [p.double() for p in P])


def disc_backward_ref(x, label, P, gout):
    """-> (dx, dlabel, [6 parameter gradients]) of sum_b gout_b D_b, fp64 autograd"""
    lv = _leaves([x, label] + list(P))
    tot = (disc_D(lv[0], lv[1], lv[2:]).view(-1) * gout.double().view(-1)).sum()
    g = torch.autograd.grad(tot, lv, allow_unused=True)
    g = [torch.zeros_like(l) if v is None else v for v, l in zip(g, lv)]
    return g[0], g[1], g[2:]


def disc_backward_backward_ref(x, label, P, gout, gbar):
    """-> (dx2, dlabel2, dgout, [6]) of <gbar, d(sum gout D)/dx>, fp64 autograd with create_graph"""
    lv = _leaves([x, label, gout.view(-1)] + list(P))
    tot = (disc_D(lv[0], lv[1], lv[3:]).view(-1) * lv[2]).sum()
    dx = torch.autograd.grad(tot, lv[0], create_graph=True)[0]
    g = torch.autograd.grad((dx * gbar.double()).sum(), lv, allow_unused=True)
    g = [torch.zeros_like(l) if v is None else v for v, l in zip(g, lv)]
    return g[0], g[1], g[2], g[3:]


def disc_wgan_gp_ref(z, fv, label, alphas, P, gp_weight):
    """-> (losses [2] = (d_loss, gp), [6 parameter gradients], dz): oracle.wgan_gp_d_loss under fp64 autograd"""
    from oracle import pcaa_oracle as O
    lv = _leaves([z] + list(P))
    sd = dict(zip(("model.0.weight", "model.0.bias", "model.2.weight", "model.2.bias", "model.4.weight", "model.4.bias"), lv[1:]))
    d_loss, gp = O.wgan_gp_d_loss(sd, fv.double(), label.double(), lv[0], alphas.double().view(-1, 1), float(f32(gp_weight)))
    g = torch.autograd.grad(d_loss, lv)
    return torch.stack([d_loss.detach(), gp.detach()]), list(g[1:]), g[0]


def _bad_w1(W1):
    """W1 [64, IN] stored at pitch IN, rows read at pitch IN + 1 (what is read past the end: 0)"""
    IN = W1.shape[1]
    flat = torch.cat([W1.reshape(-1), torch.zeros(H1 + IN, dtype=W1.dtype, device=W1.device)])
    idx = torch.arange(H1, device=W1.device).view(H1, 1) * (IN + 1) + torch.arange(IN, device=W1.device).view(1, IN)
    return flat[idx]


def _disc_fwd(u, P, defect=None):
    W1, b1, W2, b2, w3, b3 = P
    a1 = mm(u, W1.T, bias=b1)
    h1, e1, e1pp = en_elu(a1, defect == "elu_pp_wrong_side")
    a2 = mm(h1, W2.T, bias=b2)
    h2, e2, e2pp = en_elu(a2, defect == "elu_pp_wrong_side")
    D = add(rowsum(mul(h2, w3), 6), b3)
    return dict(u=u, h1=h1, e1=e1, e1pp=e1pp, h2=h2, e2=e2, e2pp=e2pp, D=D)


def _disc_first(fw, c, P):
    """first-order backward of sum_b c_b D_b: the record of disc.hip::first_order"""
    W1, b1, W2, b2, w3, b3 = P
    d2 = mul(mul(c, w3), fw["e2"])
    r1 = mm(d2, W2, n=H2)
    d1 = mul(fw["e1"], r1)
    du = mm(d1, W1, n=H1)
    return dict(d2=d2, r1=r1, d1=d1, du=du, h2c=mul(c, fw["h2"]), c=c)


def _first_params(fw, fo):
    return [tmm(fo["d1"], fw["u"]), colsum(fo["d1"]), tmm(fo["d2"], fw["h1"]), colsum(fo["d2"]),
            colsum(fo["h2c"]).view(1, H2), colsum(fo["c"]).view(1)]


def _disc_second(fw, fo, gbar, P, defect=None):
    """backward of <gbar, du[:, :32]> (disc.hip MODE 3 / the penalty of MODE 2) -> (du2, dc, [6 parameter gradients])"""
    W1, b1, W2, b2, w3, b3 = P
    B, IN = fw["u"].v.shape
    G = en_cat(gbar, EN(torch.zeros((B, IN - XD), dtype=gbar.v.dtype, device=gbar.v.device)))
    c = fo["c"]
    sb1 = mm(G, W1.T, n=XD)
    rb1 = mul(fw["e1"], sb1)
    ab1d = mul(mul(fw["e1pp"], fo["r1"]), sb1)
    sb2 = mm(rb1, W2.T, n=H1)
    ab2 = mul(mul(mul(fw["e2pp"], c), w3), sb2)
    h2c = mul(mul(c, fw["e2"]), sb2)
    dc = rowsum(mul(mul(fw["e2"], w3), sb2), 6)
    hb1 = mm(ab2, W2, n=H2)
    ab1 = add(mul(fw["e1"], hb1), ab1d)
    du2 = mm(ab1, W1, n=H1)
    dW1, dW2 = tmm(ab1, fw["u"]), tmm(ab2, fw["h1"])
    if defect != "gp_outer_missing":
        dW1, dW2 = plus(dW1, tmm(fo["d1"], G)), plus(dW2, tmm(fo["d2"], rb1))
    zero = torch.zeros(1, dtype=gbar.v.dtype, device=gbar.v.device)
    return du2, dc, [dW1, colsum(ab1), dW2, colsum(ab2), colsum(h2c).view(1, H2), EN(zero)]


def _en_inputs(x, label, P, dtype, defect=None):
    lab = label.to(dtype)
    if defect == "label_shift" and lab.shape[1] >= 2:
        lab = lab.roll(1, dims=1)
    Pv = [p.to(dtype) for p in P]
    if defect == "w1_pitch_odd" and Pv[0].shape[1] % 2 == 1:
        Pv[0] = _bad_w1(Pv[0])
    Pe = [EN(Pv[0]), EN(Pv[1].view(1, -1)), EN(Pv[2]), EN(Pv[3].view(1, -1)), EN(Pv[4].view(1, -1)), EN(Pv[5].view(1, 1))]
    return EN(torch.cat([x.to(dtype), lab], 1)), Pe


def _split(du):
    return du[:, :XD], du[:, XD:]


def disc_forward_en(x, label, P, dtype=torch.float64, defect=None):
    u, Pe = _en_inputs(x, label, P, dtype, defect)
    return _disc_fwd(u, Pe, defect)["D"]


def disc_backward_en(x, label, P, gout, dtype=torch.float64, defect=None):
    """the kernel's formulation of disc_backward -> (dx, dlabel, [6]) as EN nodes (dtype float32: an fp32 evaluation)"""
    u, Pe = _en_inputs(x, label, P, dtype, defect)
    fw = _disc_fwd(u, Pe, defect)
    fo = _disc_first(fw, EN(gout.to(dtype).view(-1, 1)), Pe)
    dx, dl = _split(fo["du"])
    return dx, dl, _first_params(fw, fo)


def disc_backward_backward_en(x, label, P, gout, gbar, dtype=torch.float64, defect=None):
    """-> (dx2, dlabel2, dgout [B, 1], [6])"""
    u, Pe = _en_inputs(x, label, P, dtype, defect)
    fw = _disc_fwd(u, Pe, defect)
    fo = _disc_first(fw, EN(gout.to(dtype).view(-1, 1)), Pe)
    du2, dc, grads = _disc_second(fw, fo, EN(gbar.to(dtype)), Pe, defect)
    dx, dl = _split(du2)
    return dx, dl, dc, grads


def disc_wgan_gp_en(z, fv, label, alphas, P, gp_weight, dtype=torch.float64, defect=None):
    """-> (losses [2], [6], dz) as EN nodes: the three passes of disc.hip MODE 2"""
    B = z.shape[0]
    al = alphas.to(dtype).view(-1, 1)
    if defect == "alpha_next_row":
        al = al.roll(-1, dims=0)
    uz, Pe = _en_inputs(z, label, P, dtype, defect)
    uf, _ = _en_inputs(fv, label, P, dtype, defect)
    one = torch.ones((B, 1), dtype=dtype, device=z.device)
    invB = en_rounded(one / B)
    fr = _disc_fwd(uz, Pe, defect)
    fo_r = _disc_first(fr, scale(invB, -1.0), Pe)
    ff = _disc_fwd(uf, Pe, defect)
    fo_f = _disc_first(ff, invB, Pe)
    K = label.shape[1]
    zx, fx, lab = EN(uz.v[:, :XD]), EN(uf.v[:, :XD]), uz.v[:, XD:]
    it = add(zx, mul(EN(al), sub(fx, zx)))
    ui = en_cat(it, EN(lab))
    fi = _disc_fwd(ui, Pe, defect)
    fo_i = _disc_first(fi, EN(one), Pe)
    g = fo_i["du"][:, :XD]
    nrm = en_sqrt(add(rowsum(mul(g, g), 6), const(1e-12, g)))
    nm1 = sub(nrm, const(1.0, g))
    gprow = mul(nm1, nm1)
    gpw = const(f32(gp_weight), g)
    gbar = mul(div(mul(mul(scale(gpw, 2.0), invB), nm1), nrm), g)
    du2, _, g2 = _disc_second(fi, fo_i, gbar, Pe, defect)
    grads = [plus(plus(a, b), c) for a, b, c in zip(_first_params(fr, fo_r), _first_params(ff, fo_f), g2)]
    grads[5] = EN(torch.zeros(1, dtype=dtype, device=z.device))               # sum(-1/B) + sum(+1/B): exactly 0
    k = 1.0 if defect == "dz_no_1_minus_alpha" else None
    fac = const(1.0, g) if k else sub(const(1.0, g), EN(al))
    dz = add(mul(fac, du2[:, :XD]), fo_r["du"][:, :XD])
    mean = lambda a: EN(_sum64(a.v) / B, a.f.sum() / B, a.q.sum() / B ** 2)                # fp64 sums of the rows' fp32 values
    real, fake, gp = mean(fr["D"]), mean(ff["D"]), mean(gprow)
    dl = EN(fake.v - real.v + gpw.v * gp.v, fake.f + real.f + gpw.v.abs() * gp.f, fake.q + real.q + gpw.v ** 2 * gp.q)
    cast = lambda a: EN(a.v, a.f + a.v.abs(), a.q + a.v ** 2)
    dl, gp = cast(dl), cast(gp)
    return EN(torch.stack([dl.v, gp.v]), torch.stack([dl.f, gp.f]), torch.stack([dl.q, gp.q])), grads, dz


# ====================================================================================================== OR-CED
def orced_inputs(B, K, d_in, L, device="cpu"):
    seed = seed_of(B * 7 + K, d_in * 3 + L)
    r = lambda s, a, *shape: uniform(int(np.prod(shape)), seed + s, device, -a, a).view(*shape).float()
    w = 1.0 / d_in ** 0.5
    return {"x4": r(0, 1.7, B, d_in), "Wmu": r(1, 1.5 * w, L, d_in), "bmu": r(2, 0.3, L), "Wlv": r(3, 0.8 * w, L, d_in),
            "blv": r(4, 0.3, L), "eps": r(5, 1.7, B, L), "Wc": r(6, 1.5 / L ** 0.5, K, L), "bc": r(7, 0.3, K),
            "d_logits": r(8, 1.0, B, K), "d_sup": r(9, 1.0, B, L), "d_mu": r(10, 1.0, B, L), "d_logvar": r(11, 1.0, B, L)}


_ORCED_LEAVES = ("x4", "Wmu", "bmu", "Wlv", "blv", "Wc", "bc")


def orced_fwd_ref(c):
    """fp64 (logits, sup_fv, mu, logvar) with the leaves they were computed from"""
    lv = dict(zip(_ORCED_LEAVES, _leaves([c[k] for k in _ORCED_LEAVES])))
    mu = lv["x4"] @ lv["Wmu"].t() + lv["bmu"]
    lg = lv["x4"] @ lv["Wlv"].t() + lv["blv"]
    sup = mu + c["eps"].double() * torch.exp(0.5 * lg)
    logits = sup @ lv["Wc"].t() + lv["bc"]
    return (logits, sup, mu, lg), lv


def orced_bwd_ref(c, use):
    """``use``: which of d_logits, d_sup, d_mu, d_logvar are present -> dict of fp64 gradients (dx4, dWmu, ...)"""
    (logits, sup, mu, lg), lv = orced_fwd_ref(c)
    tot = 0.0
    for name, out in (("d_logits", logits), ("d_sup", sup), ("d_mu", mu), ("d_logvar", lg)):
        if name in use:
            tot = tot + (out * c[name].double()).sum()
    g = torch.autograd.grad(tot, [lv[k] for k in _ORCED_LEAVES], allow_unused=True)
    return {"d" + k: (torch.zeros_like(lv[k]) if v is None else v) for k, v in zip(_ORCED_LEAVES, g)}


def orced_fwd_en(c, dtype=torch.float64):
    e = {k: EN(v.to(dtype)) for k, v in c.items()}
    d_in = c["x4"].shape[1]
    L = c["Wmu"].shape[0]
    n_in = -(-d_in // 64) + 7                      # a lane's fmas, the 6 levels of wave_sum, the bias
    row = lambda b: EN(b.v.view(1, -1))
    mu = mm(e["x4"], e["Wmu"].T, n=n_in, bias=row(e["bmu"]))
    lg = mm(e["x4"], e["Wlv"].T, n=n_in, bias=row(e["blv"]))
    sup = add(mu, mul(e["eps"], en_exp(scale(lg, 0.5))))
    logits = mm(sup, e["Wc"].T, n=L, bias=row(e["bc"]))
    return logits, sup, mu, lg


def orced_bwd_en(c, use, logvar, sup, dtype=torch.float64, defect=None):
    """the kernels' formulation of pcaa_orced_heads_bwd.  ``logvar`` / ``sup``: the stored inputs of the kernel as EN nodes
    (``en_rounded`` of the reference's values) -> dict of EN nodes"""
    e = {k: EN(v.to(dtype)) for k, v in c.items()}
    B, d_in = c["x4"].shape
    L, K = c["Wmu"].shape[0], c["Wc"].shape[0]
    zero = EN(torch.zeros((B, L), dtype=dtype, device=c["x4"].device))
    ds = e["d_sup"] if "d_sup" in use else zero
    if "d_logits" in use:
        ds = mm(e["d_logits"], e["Wc"], n=K, bias=ds)
    gm = add(e["d_mu"] if "d_mu" in use else zero, ds)
    std = mul(mul(ds, e["eps"]), en_exp(scale(logvar, 0.5)))
    gl = add(e["d_logvar"] if "d_logvar" in use else zero, std if defect == "std_half_dropped" else scale(std, 0.5))
    dx = plus(mm(gm, e["Wmu"], n=2 * L), mm(gl, e["Wlv"], n=2 * L))
    gmu = gl if defect == "dmu_reads_dlv_row" else gm
    out = {"dx4": dx, "dWmu": tmm(gmu, e["x4"], n=B), "dWlv": tmm(gl, e["x4"], n=B),
           "dbmu": colsum(gmu[: B - 1] if defect == "bias_last_row_missing" else gmu, n=B), "dblv": colsum(gl, n=B)}
    if "d_logits" in use:
        out["dWc"], out["dbc"] = tmm(e["d_logits"], sup, n=B), colsum(e["d_logits"], n=B)
    else:
        zk = torch.zeros((K, L), dtype=dtype, device=c["x4"].device)
        out["dWc"], out["dbc"] = EN(zk), EN(zk[:, 0].clone())
    return out


def kl_inputs(B, L, device="cpu"):
    seed = seed_of(B, L + 900)
    r = lambda s, a: uniform(B * L, seed + s, device, -a, a).view(B, L).float()
    return r(0, 1.5), r(1, 1.2), r(2, 1.5)


def kl_ref(mu, logvar, mu_k, gscale):
    """-> (loss, d_mu, d_logvar, d_muk) fp64 autograd of CG_kl_divergence times gscale"""
    lv = _leaves([mu, logvar, mu_k])
    loss = torch.mean(-0.5 * torch.sum(1 + lv[1] - (lv[0] - lv[2]) ** 2 - torch.exp(lv[1]), dim=1))
    g = torch.autograd.grad(loss * float(f32(gscale)), lv)
    return loss.detach(), g[0], g[1], g[2]


def kl_en(mu, logvar, mu_k, gscale, dtype=torch.float64):
    m, lg, mk = EN(mu.to(dtype)), EN(logvar.to(dtype)), EN(mu_k.to(dtype))
    B = mu.shape[0]
    d = sub(m, mk)
    e = en_exp(lg)
    t = sub(sub(add(const(1.0, m), lg), mul(d, d)), e)
    loss = EN(-0.5 * _sum64(t.v) / B, 0.5 * t.f.sum() / B, 0.25 * t.q.sum() / B ** 2)
    loss.f, loss.q = loss.f + loss.v.abs(), loss.q + loss.v ** 2
    gs = div(const(f32(gscale), m), const(float(B), m))
    return loss, mul(gs, d), mul(scale(gs, -0.5), sub(const(1.0, m), e)), scale(mul(gs, d), -1.0)


# ====================================================================================================== scoring
WIDE = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
LOG2PI = 1.8378770664093453                       # the double the kernel holds


def likelihood_inputs(B, K, D, device="cpu"):
    """fp32 (x [B, D], means [K, D]): row b sits at distance^2 of about 0 (exactly on its centroid), 50, the value that
    makes the result denormal (1460 - D log 2pi: 1400 at D = 32), and 1600 (the result is exactly 0) from centroid b % K,
    in turn"""
    seed = seed_of(B, 10 * K + D)
    means = uniform(K * D, seed, device, -2.0, 2.0).view(K, D).float()
    b = torch.arange(B, device=device)
    d2 = torch.tensor([0.0, 50.0, 1460.0 - D * LOG2PI, 1600.0], dtype=torch.float64, device=device)[b % 4]
    sign = torch.where(uniform(B * D, seed + 1, device).view(B, D) < 0.5, -1.0, 1.0)
    x = means.double()[b % K] + sign * torch.sqrt(d2 / D).view(B, 1)
    return x.float().contiguous(), means.contiguous()


def joint_likelihood_ref(x, means, defect=None, wide=None):
    """x [B, D], means [K, D] fp32 -> (lik, gate) float64 numpy [B].  ``wide``: np.longdouble arithmetic (default: where
    it is wider than double); otherwise every |x - mu|^2 is math.fsum over exact products (a difference of fp32 values
    is exact in double, its square splits exactly into two doubles), so only log, exp and the K-term sum round"""
    x = x.detach().cpu().numpy()
    mu = means.detach().cpu().numpy()
    B, D = x.shape
    K = mu.shape[0]
    Dc = 32 if defect == "d_fixed_32" else D
    wide = WIDE if wide is None else wide
    ld = np.longdouble if wide else np.float64
    d64 = x.astype(np.float64)[:, None, :] - mu.astype(np.float64)[None]          # exact
    if defect == "fp32_maha":
        d32 = d64.astype(np.float32)
        maha = np.cumsum(d32 * d32, axis=-1, dtype=np.float32)[..., -1].astype(ld)
    elif wide:
        maha = (d64.astype(ld) ** 2).sum(-1)
    else:
        hi = np.float64(134217729.0) * d64                                       # Veltkamp split: d = a + b, 26 bits each
        a = hi - (hi - d64)
        b_ = d64 - a
        maha = np.array([[math.fsum(np.concatenate([a[i, k] * a[i, k], 2 * a[i, k] * b_[i, k], b_[i, k] * b_[i, k]]))
                          for k in range(K)] for i in range(B)])
    arg = ld(-0.5) * (ld(Dc) * np.log(ld(2) * ld(np.pi)) + maha)
    terms = np.exp(arg)
    lik = terms.sum(1) if defect == "no_1_over_k" else terms.sum(1) / K
    a = np.abs(arg).astype(np.float64)
    t = terms.astype(np.float64)
    lik64 = lik.astype(np.float64)
    gate = (t * ((D + 4) * a + 4)).sum(1) * U64 / K + (K + 1) * U64 * lik64 + (K + 2) * 2.0 ** -1074
    return lik64, gate


def kvote_ref(lik, preds, thr, k, n_labels, defect=None):
    """numpy in, numpy out: oracle.k_vote, or a defective vote"""
    from oracle import pcaa_oracle as O
    lik, preds = np.asarray(lik, dtype=np.float64), np.asarray(preds, dtype=np.int64)
    if defect is None:
        return O.k_vote(lik, preds, thr, k, n_labels)
    nwin = len(preds) // k
    out = np.empty(nwin, dtype=np.int64)
    for w in range(nwin):
        lk, pr = lik[w * k:(w + 1) * k], preds[w * k:(w + 1) * k]
        above = int(np.sum(lk >= thr if defect == "ge_threshold" else lk > thr))
        known = 2 * above >= k if defect == "lt_half" else 2 * above > k
        cnt = np.bincount(pr)
        best = len(cnt) - 1 - int(np.argmax(cnt[::-1])) if defect == "highest_on_ties" else int(np.argmax(cnt))
        out[w] = best if known else n_labels
    return out


def kvote_exhaustive(n_classes=3, ks=(1, 2, 3, 4), thr=0.5):
    """every (prediction, above / not above) pattern: for each k in ``ks`` all n_classes^k prediction tuples x all 2^k
    tuples of above / not above -> {k: (lik float64 [n * k], preds int64 [n * k])}.  'Above' is 2 thr; 'not above'
    alternates between thr itself (equal is not above) and thr / 2"""
    import itertools
    out = {}
    for k in ks:
        lik, preds = [], []
        for pr in itertools.product(range(n_classes), repeat=k):
            for ab in itertools.product((0, 1), repeat=k):
                preds.extend(pr)
                lik.extend([2 * thr if a else (thr if (i + sum(pr)) % 2 else thr / 2) for i, a in enumerate(ab)])
        out[k] = (np.array(lik, dtype=np.float64), np.array(preds, dtype=np.int64))
    return out


def stream_ref(logits, sup_fv, means, thr, k, n_labels):
    """one stream's windows over all ticks, concatenated: fp32 logits [n, K], sup_fv [n, D] ->
    (preds int64 [n], lik [n], lik_gate [n], votes [n // k]) numpy"""
    from oracle import pcaa_oracle as O
    preds = ce_ref(logits)["preds"].cpu().numpy()
    lik, gate = joint_likelihood_ref(sup_fv, means)
    n = len(preds) // k * k
    return preds, lik, gate, O.k_vote(lik[:n], preds[:n], thr, k, n_labels)


# ====================================================================================================== the cases of both files
CHAMFER_SHAPES = [(2, 3, 1, 1), (2, 3, 2, 3), (3, 2, 64, 1), (3, 2, 128, 4), (2, 2, 129, 5), (1, 2, 256, 8), (1, 2, 257, 8),
                  (1, 2, 300, 4), (1, 1, 819, 8), (1, 2, 820, 3), (1, 1, 1920, 2)]          # (B, T, N, C)
CHAMFER_SMALL = CHAMFER_SHAPES[:5]
CE_CASES = [(1, 1, 4), (1, 6, 4), (37, 6, 4), (37, 2, 80), (256, 64, 4), (257, 1, 4), (257, 6, 80), (600, 2, 4),
            (600, 64, 80)]                                                                 # (B, K, magnitude)
DISC_CASES = [(0, 6, False), (1, 1, False), (4, 257, False), (7, 6, True), (8, 1, True), (31, 257, True), (32, 6, False),
              (32, 257, True)]                                                             # (K, B, dense labels)
LIK_CASES = [(1, 4, 32), (127, 1, 1), (128, 8, 33), (129, 4, 32), (300, 8, 33), (300, 1, 1)]   # (B, K, D)
ORCED_SHAPES = [(1, 1, 1, 1), (5, 7, 1000, 33), (3, 64, 1024, 128), (70, 3, 257, 5)]       # (B, K, d_in, L)
ORCED_USES = [("d_logits",), ("d_sup",), ("d_mu",), ("d_logvar",), ("d_logits", "d_sup", "d_mu", "d_logvar")]
KL_SHAPES = [(1, 1), (5, 51), (8, 32), (257, 1), (50, 100)]                                # B L = 1, 255, 256, 257, 5000
GP_WEIGHT = 10.0
