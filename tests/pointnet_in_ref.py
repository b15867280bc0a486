"""fp64 restatements of the operations of csrc/pointnet_in.hip (the first PointNet layer), the gate of each output, the
cases, and planted defects.

Used by tests/test_pointnet_in_branches.py (the kernels, on the GPU) and tests/test_pointnet_in_gates_cpu.py (the gates
themselves, on the CPU).  Plain torch, device-agnostic: a reference runs where its inputs live, in float64.  The
generator, the BatchNorm vectors, the gradient, ``ratio`` / ``moved`` and the sum gates are those of
tests/elementwise_ref.py; nothing of it is restated here.

Same stored values on both sides
--------------------------------
The points ``x`` and the weight ``W`` are fp32 tensors on both sides; a bf16 ``da`` / ``dy`` is rounded first and that
tensor is widened; ``scale``, ``shift``, ``mean``, ``rstd``, ``coef`` and the fp64 moments ``mom`` (hence the pivot,
fp32(mom_sum * (1/P)), formed by the same two operations) are the same tensors on both sides.  What is left is the
kernels' own fp32 arithmetic.

The gates, with u = 2^-24
-------------------------
ymag = |x| . |W|^T (the magnitudes the C fused multiply-adds of y = x . W^T add up); yg = 2 C u ymag is the gate of y:
C fmas, each rounding at most u of a partial sum that ymag bounds, doubled as elementwise_ref doubles its counts.
z = y scale + shift; T = |y scale| + |shift|; neg = [z <= 0].

* ``pointnet_in_fwd``  y + bias:  yg + u (|y| + |bias|) (the one addition);  bf16: + 2^-8 |want|.
  Statistics (of the bias-free product): summand y has error yg, summand y^2 has 2 ymag yg + u ymag^2 (two factors, one
  product).  A workgroup adds its 128 rows in fp32, row r in lane r % rl (rl = 1024 / cout): ``sum_gate`` with
  lanes = rl, over the rows the workgroup really has, plus the sum of its summands' errors (the summands' errors are
  counted, not left to SUM_PAD: C fmas per summand is more than SUM_PAD stands for).  Lanes and workgroups meet in fp64:
  the statistic's gate is the sum of the workgroups' gates.
* ``pointnet_in_apply``  ELU(z):  elementwise_ref.bn_act_fwd_ref's gate (4u (T + neg) + neg u |z|, the same for expm1f
  and for the 2-byte types' exp2(z log2e) - 1) + yg |scale| (y's error through z; ELU has slope <= 1).  bf16: + 2^-8
  |want|; e4m3: the interval check of fp8_ref.in_interval; split image: the assertion of test_split_image_producers.
* dz = da ELU'(z) (all backward modes):  |da| e (rel_e + neg yg |scale| + 2u), rel_e = elementwise_ref's
  u (4T + neg (|z| + 3)) (it already holds the two extra roundings of the bf16 one-pass path, which folds log2e into
  scale and shift; the 2-byte MODE 0-2 paths call __expf = exp2(z log2e)), e' = e gives the relative error of e from
  the error of z.
* MODE 0 / MODE 3 statistics  sum dz, sum dz yhat, yhat = (y - mean) rstd:  summand errors dz_gate and
  dz_gate (ymag + |mean|) rstd + |dz| (yg + 3u (ymag + |mean|)) rstd (difference, product, product; the packed path's
  two fmas round less); 256-row workgroups, lanes = rl, workgroups in fp64: as for the forward.
* MODE 1 / MODE 2  dW = sum_p dy x, dy = k0 d + k1 y + k2 (d = dz, or the incoming tensor under dz_is_pre):
  dy has |k0| d_gate + |k1| yg + 8u (|k0 d| + |k1| ymag + |k2|) (elementwise_ref's dy count), the summand dy x that
  times |x| (the fma rounds once, inside the sum gate).  Per workgroup: sum_gate(256 rows, lanes = rl) + the summand
  errors.  The workgroups meet in fp32 atomics in no fixed order: the order-free bound of recursive summation,
  (number of workgroups) u sum_b |partial_b|, on top of the workgroups' gates.
* MODE 3  G_b = sum_{p in workgroup b} dz (x - pivot):  the centred point is one fp32 subtraction, u |x - pivot|; the
  summand dz xc has dz_gate |xc| + u |dz xc|; per workgroup as above.  Rows form: G_b is stored.  Replica form: the
  workgroups b = r mod nrep meet in fp32 atomics: + (their number) u sum |G_b|.
* ``pointnet_in_bwd_combine``  dW = c0 G' + c1 W.(XtX - pivot (x) sum x) + c2 (sum x - P pivot): an fp64 combination
  rounded once to fp32: 2^-23 |want| + |c0| (gate of G' = the sum of the gates of G's rows; 0 when the reference is
  handed the kernel's own G) + 2^-50 (|c0 G'| + |c1| |W|.(|XtX| + |pivot| |sum x|) + |c2| (|sum x| + P |pivot|)).
  THE COMBINE DROPS pivot (x) sum_p dy ON PURPOSE: BatchNorm's backward makes sum_p dy = 0.  With a pivot ``combine_ref``
  therefore equals dy^T x only when coef is bn_bwd_finalize's of the same statistics; the tests compare with the
  formula as pointnet_in.hip states it (coef from the launch's own finalize), and use arbitrary coef vectors only with
  pivot_mom = NULL, where nothing is dropped.
* ``points_moments``: products of fp32 values are exact in fp64; P fp64 additions in some order (lane, wave, workgroup,
  atomics), and as many in the reference: P 2^-52 sum |x_k x_c| (resp. sum |x_c|).  Exactly 0 outside C.
* ``pointnet_in_moment_coeffs``: sum y = W . sum x and sum y^2 = w^T XtX w in fp64 from the same moments, then
  elementwise_ref.bn_finalize_ref.  The two contractions cancel where the points are off-centre: (C + 2) 2^-52 of the
  magnitudes they add, carried through 1 / (2 (var + eps)) like bn_finalize_ref's own ``amp``.
* ``pointnet_in_wgrad``  dW = dy^T x: every summand is one fma (no error of its own): per 256-row workgroup
  sum_gate(lanes = rl), then the atomics' order-free bound.
* ``cast_bf16``: bitwise torch's round-to-nearest-even cast.

No constant above was moved after the first count; the CPU file's fp32 evaluations (its docstring has the ratios) stay
within every gate.

Planted defects
---------------
``defect=``: "drop_tail_rows" (a lane's rows after its last full trip left out), "count_clamped_row" (the clamped last
row of a workgroup added once more for every skipped slot of a trip: a missing ``break``), "swap_quads" (adjacent
channel quads exchange W / bias / scale / shift / mean / rstd / coef), "stride_cp" (points read with row stride CP =
4 or 8 instead of C), "bias_in_stats", "elu_twice" (MODE 2 applies ELU' to the incoming dz), "uncentred_combine" (G
centred, the combine with pivot 0), "lower_triangle_missing" (moments only at k <= c), "replica_overwrite" (a replica
of G holds its LAST workgroup instead of the sum), "swap_coef" (coef1 and coef2 exchanged).
"""
import torch

import elementwise_ref as E
from elementwise_ref import U, sum_gate

F32, BF16 = torch.float32, torch.bfloat16
MAXC, NREP, FWD_ROWS, BWD_ROWS = 8, 16, 128, 256
MOM_SIZE = MAXC * MAXC + MAXC
R32, C64 = 2.0 ** -23, 2.0 ** -50
OFFS = (40.0, -25.0, 3.0, 0.5, 900.0)            # mean / deviation up to 3 000 (test_first_layer_with_offcentre_features)
DEVS = (0.3, 0.2, 0.5, 1.0, 0.3)

# ------------------------------------------------------------------------------------------------ the cases
# widths: every cout at C = 4 and 5 (CP = 4 and 8), every C at cout = 64 and 512 -- not the full cross product: the
# channel-quad / row-lane layout depends on cout alone and the feature loops on C alone
WIDTHS = [(cout, C) for cout in (4, 64, 512, 1024) for C in (4, 5)] + [(cout, C) for cout in (64, 512) for C in (1, 3, 8)]
FWD_WRAP, BWD_WRAP = FWD_ROWS * 17 + 5, BWD_ROWS * 17 + 5


def rl_of(cout):
    return 1024 // cout


def row_counts(cout, C, wrap):
    """P of a width: the full list at C = 4 / 5, three of them at the other C"""
    if C not in (4, 5):
        return [1, 129, 300]
    rl = rl_of(cout)
    ps = {1, 127, 128, 129, 255, 256, 257, 300, wrap} | {p for p in (rl - 1, rl + 1) if p >= 1}
    return sorted(ps)


def seed(cout, C, P):
    return E.seed_of(cout * 16 + C, P)


def points(P, C, sd, device="cpu", offcentre=False):
    """fp32 [P, C], unit variance; offcentre: scaled to DEVS and moved to OFFS (C <= 5)"""
    x = E.uniform(P * C, sd + 11, device, -3.0 ** 0.5, 3.0 ** 0.5).view(P, C)
    if offcentre:
        x = x * torch.tensor(DEVS[:C], dtype=torch.float64, device=device) + torch.tensor(OFFS[:C], dtype=torch.float64, device=device)
    return x.float()


def weights(cout, C, sd, device="cpu"):
    return E.uniform(cout * C, sd + 12, device, -0.5, 0.5).view(cout, C).float()


def lin_bias(cout, sd, device="cpu"):
    return E.uniform(cout, sd + 13, device, -0.3, 0.3).float()


def gamma_of(cout, sd, device="cpu"):
    return E.uniform(cout, sd + 14, device, 0.7, 1.3).float()


def batch_vectors(x, W, sd):
    """fp32 (scale, shift, mean, rstd) of train-mode BatchNorm over THESE points (fp64 statistics, eps 1e-5, gamma =
    gamma_of, beta +- 0.5): what the off-centre input needs -- arbitrary vectors would put every z on one ELU branch"""
    cout = W.shape[0]
    y = x.double() @ W.double().t()
    mean, var = y.mean(0), y.var(0, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    g = gamma_of(cout, sd, x.device).double()
    beta = E.uniform(cout, sd + 15, x.device, -0.5, 0.5)
    return (g * rstd).float(), (beta - mean * g * rstd).float(), mean.float(), rstd.float()


def case(cout, C, P, dtype, device="cpu", offcentre=False):
    """the inputs of one case: dict(x, W, bias, da, scale, shift, mean, rstd, coef, gamma)"""
    sd = seed(cout, C, P)
    x, W = points(P, C, sd, device, offcentre), weights(cout, C, sd, device)
    sc, sh, mu, rs = batch_vectors(x, W, sd) if offcentre else E.bn_vectors(cout, sd, device)
    return {"x": x, "W": W, "bias": lin_bias(cout, sd, device), "da": E.gradient(P, cout, dtype, sd, device),
            "scale": sc, "shift": sh, "mean": mu, "rstd": rs, "coef": E.coef_vectors(cout, sd, device, 1.0 / P),
            "gamma": gamma_of(cout, sd, device)}


# ------------------------------------------------------------------------------------------------ shared pieces
def _prep(x, W, defect, *vecs):
    C = x.shape[1]
    x, W = x.double(), W.double()
    if defect == "stride_cp":
        CP = 4 if C <= 4 else 8
        flat = x.reshape(-1)
        idx = torch.arange(x.shape[0], device=x.device).view(-1, 1) * CP + torch.arange(C, device=x.device)
        x = flat[idx.clamp_max(flat.numel() - 1)] * (idx < flat.numel())
    vs = [v.double() for v in vecs]
    if defect == "swap_quads":
        W = E.swap_quads(W.t()).t()
        vs = [E.swap_quads(v) for v in vs]
    return x, W, vs


def _y(x, W):
    """-> y, ymag, yg"""
    ymag = x.abs() @ W.abs().t()
    return x @ W.t(), ymag, 2 * x.shape[1] * U * ymag


def row_weights(P, block, trip, rl, defect=None, device="cpu"):
    """[P, 1] float64: how often each row enters a workgroup's sums.  The kernels give row r of a workgroup to lane
    r % rl; a lane walks its rows ``trip`` at a time."""
    w = torch.ones(P, dtype=torch.float64, device=device)
    if defect not in ("drop_tail_rows", "count_clamped_row"):
        return w.view(P, 1)
    for n, starts in ((block, range(0, P - block + 1, block)), (P % block, [P // block * block])):
        if n == 0:
            continue
        r = torch.arange(n, device=device)
        lane, j = r % rl, r // rl
        k = (n - lane + rl - 1) // rl                          # rows of this row's lane
        if defect == "drop_tail_rows":
            pat = (j < k // trip * trip).double()
        else:
            kl = (n - torch.arange(min(rl, n), device=device) + rl - 1) // rl
            pat = torch.ones(n, dtype=torch.float64, device=device)
            pat[n - 1] += float(((kl + trip - 1) // trip * trip - kl).sum())
        for b0 in starts:
            w[b0:b0 + n] = pat
    return w.view(P, 1)


def has_tail(P, block, trip, rl):
    """whether "drop_tail_rows" leaves out any row at this P"""
    return bool((row_weights(P, block, trip, rl, "drop_tail_rows") == 0).any())


def block_sums(t, block):
    """[P, ch] -> [nb, ch]: the sum of each workgroup's rows"""
    P, ch = t.shape
    nb = -(-P // block)
    p = torch.zeros((nb * block, ch), dtype=t.dtype, device=t.device)
    p[:P] = t
    return p.view(nb, block, ch).sum(1)


def block_gates(t, mag, err, block, lanes):
    """[nb, ch]: the gate of each workgroup's fp32 sum of the summands t (magnitudes mag, own errors err), over the
    rows the workgroup really has"""
    P, ch = t.shape
    nf, out = P // block, []
    if nf:
        v = lambda a: a[:nf * block].view(nf, block, ch)
        out.append(sum_gate(v(t), v(mag), lanes) + v(err).sum(1))
    if P % block:
        v = lambda a: a[nf * block:].unsqueeze(0)
        out.append(sum_gate(v(t), v(mag), lanes) + v(err).sum(1))
    return torch.cat(out)


def replicas(per_block, nrep=NREP, defect=None):
    """[nb, ...] -> [nrep, ...]: workgroup b adds into replica b % nrep"""
    nb = per_block.shape[0]
    out = torch.zeros((nrep,) + tuple(per_block.shape[1:]), dtype=per_block.dtype, device=per_block.device)
    if defect == "replica_overwrite":
        for b in range(nb):
            out[b % nrep] = per_block[b]
        return out
    return out.index_add_(0, torch.arange(nb, device=per_block.device) % nrep, per_block)


def atomic_gate(per_block, nrep=1):
    """the order-free bound of fp32 atomics: (workgroups that meet in one word) u sum |partial|, per replica"""
    nb = per_block.shape[0]
    return -(-nb // nrep) * U * replicas(per_block.abs(), nrep)


# ------------------------------------------------------------------------------------------------ forward, apply
def fwd_ref(x, W, bias, defect=None):
    """-> dict(y, y_gate [P, cout]; block_stats, block_stats_gate [nb, 2, cout]; stats, stats_gate [2, cout])"""
    cout = W.shape[0]
    b0 = bias if bias is not None else torch.zeros(cout, device=x.device)
    x, W, (b,) = _prep(x, W, defect, b0)
    y0, ymag, yg = _y(x, W)
    s = y0 + b if defect == "bias_in_stats" else y0
    bs = torch.stack([block_sums(s, FWD_ROWS), block_sums(s * s, FWD_ROWS)], 1)
    bg = torch.stack([block_gates(y0, ymag, yg, FWD_ROWS, rl_of(cout)),
                      block_gates(y0 * y0, ymag * ymag, 2 * ymag * yg + U * ymag * ymag, FWD_ROWS, rl_of(cout))], 1)
    return {"y": y0 + b, "y_gate": yg + U * (y0.abs() + b.abs()), "block_stats": bs, "block_stats_gate": bg,
            "stats": bs.sum(0), "stats_gate": bg.sum(0)}


def apply_ref(x, W, scale, shift, defect=None):
    """-> (a, gate32)"""
    x, W, (sc, sh) = _prep(x, W, defect, scale, shift)
    y, ymag, yg = _y(x, W)
    a, gate = E.bn_act_fwd_ref(y, sc, sh)
    return a, gate + yg * sc.abs()


# ------------------------------------------------------------------------------------------------ backward
def _dz(da, y, yg, sc, sh):
    _, z, T, neg = E._z(y, sc, sh)
    e = E.elu_grad(z)
    g = da.double()
    return g * e, g.abs() * e * (E._rel_e(z, T, neg) + neg * yg * sc.abs() + 2 * U)


def _trip(dtype, onepass):
    return 8 if (onepass and dtype == BF16) else 4


def bwd_stats_ref(da, x, W, scale, shift, mean, rstd, defect=None, onepass=False):
    """MODE 0 (and the statistics of MODE 3: onepass=True only changes the trip length of the row defects)
    -> dict(block_stats, block_stats_gate [nb, 2, cout]; stats, stats_gate [2, cout])"""
    P, cout = da.shape
    rl = rl_of(cout)
    x, W, (sc, sh, mu, rs) = _prep(x, W, defect, scale, shift, mean, rstd)
    y, ymag, yg = _y(x, W)
    dz, dzg = _dz(da, y, yg, sc, sh)
    ymm = (ymag + mu.abs()) * rs
    t2, m2 = dz * ((y - mu) * rs), dz.abs() * ymm
    e2 = dzg * ymm + dz.abs() * (yg + 3 * U * (ymag + mu.abs())) * rs
    w = row_weights(P, BWD_ROWS, _trip(da.dtype, onepass), rl, defect, da.device)
    bs = torch.stack([block_sums(dz * w, BWD_ROWS), block_sums(t2 * w, BWD_ROWS)], 1)
    bg = torch.stack([block_gates(dz, dz.abs(), dzg, BWD_ROWS, rl), block_gates(t2, m2, e2, BWD_ROWS, rl)], 1)
    return {"block_stats": bs, "block_stats_gate": bg, "stats": bs.sum(0), "stats_gate": bg.sum(0)}


def _contract(d, dg, xs, w, cout, rl):
    """per-workgroup sums of d[p, o] xs[p, c] -> (sums, gates) [nb, cout, C]; dg: the error of d"""
    S, Gt = [], []
    for c in range(xs.shape[1]):
        xc = xs[:, c:c + 1]
        t = d * xc
        S.append(block_sums(t * w, BWD_ROWS))
        Gt.append(block_gates(t, t.abs(), dg * xc.abs(), BWD_ROWS, rl))
    return torch.stack(S, 2), torch.stack(Gt, 2)


def bwd_wgrad_ref(d_in, x, W, scale, shift, coef, dz_is_pre=False, defect=None):
    """MODE 1 (d_in = da) / MODE 2 (d_in = dz) -> (dW [cout, C], gate)"""
    P, cout = d_in.shape
    rl = rl_of(cout)
    x, W, (sc, sh, cf) = _prep(x, W, defect, scale, shift, coef)
    k0, k1, k2 = (cf[0], cf[2], cf[1]) if defect == "swap_coef" else cf.unbind(0)
    y, ymag, yg = _y(x, W)
    if dz_is_pre and defect != "elu_twice":
        d, dg = d_in.double(), torch.zeros_like(y)
    else:
        d, dg = _dz(d_in, y, yg, sc, sh)
    dy = k0 * d + k1 * y + k2
    dyg = k0.abs() * dg + k1.abs() * yg + 8 * U * ((k0 * d).abs() + k1.abs() * ymag + k2.abs())
    w = row_weights(P, BWD_ROWS, 4, rl, defect, d_in.device)
    S, Gt = _contract(dy, dyg, x, w, cout, rl)
    return S.sum(0), Gt.sum(0) + atomic_gate(S)[0]


def pivot_of(mom, P, C):
    """the fp32 pivot, formed as the kernels form it: fp32(mom_sum * (1 / P)); None -> zeros"""
    if mom is None:
        return None
    return (mom[MAXC * MAXC:MAXC * MAXC + C].double() * (1.0 / P)).float()


def onepass_G_ref(da, x, W, scale, shift, pivot, defect=None):
    """MODE 3 -> dict(G, G_gate [g_rows, cout, C] per 256-row workgroup; sum, sum_gate [cout, C]; rep, rep_gate
    [NREP, cout, C]: the replica form).  pivot: fp32 [C] or None."""
    P, cout = da.shape
    rl = rl_of(cout)
    x, W, (sc, sh) = _prep(x, W, defect, scale, shift)
    y, ymag, yg = _y(x, W)
    dz, dzg = _dz(da, y, yg, sc, sh)
    xc = x - pivot.double() if pivot is not None else x
    w = row_weights(P, BWD_ROWS, _trip(da.dtype, True), rl, defect, da.device)
    # the centring subtraction rounds xc by u |xc|: an error u |dz xc| of the summand, beside the fma's own
    S, Gt = _contract(dz, dzg + (U * dz.abs() if pivot is not None else 0.0), xc, w, cout, rl)
    return {"G": S, "G_gate": Gt, "sum": S.sum(0), "sum_gate": Gt.sum(0),
            "rep": replicas(S, NREP, defect), "rep_gate": replicas(Gt) + atomic_gate(S, NREP)}


def combine_ref(G, W, mom, coef, P, pivot, G_gate=None, defect=None):
    """dW as pointnet_in_bwd_combine_kernel states it -> (dW [cout, C], gate).  G: [rows, cout, C] (any row count);
    G_gate: the gate of G's row sum, None when G is the kernel's own"""
    cout, C = W.shape
    W, cf, mom = W.double(), coef.double(), mom.double()
    k0, k1, k2 = (cf[0], cf[2], cf[1]) if defect == "swap_coef" else cf.unbind(0)
    g = G.double().sum(0)
    XtX, sx = mom[:MAXC * MAXC].view(MAXC, MAXC)[:C, :C], mom[MAXC * MAXC:MAXC * MAXC + C]
    piv = torch.zeros(C, dtype=torch.float64, device=W.device) if (pivot is None or defect == "uncentred_combine") else pivot.double()
    yx = W @ (XtX - sx.view(C, 1) * piv.view(1, C))
    sxc = sx - P * piv
    want = k0.view(-1, 1) * g + k1.view(-1, 1) * yx + k2.view(-1, 1) * sxc
    mags = ((k0.view(-1, 1) * g).abs() + k1.abs().view(-1, 1) * (W.abs() @ (XtX.abs() + sx.abs().view(C, 1) * piv.abs().view(1, C)))
            + k2.abs().view(-1, 1) * (sx.abs() + P * piv.abs()))
    gate = R32 * want.abs() + C64 * mags + (k0.abs().view(-1, 1) * G_gate if G_gate is not None else 0.0)
    return want, gate + 1e-300


# ------------------------------------------------------------------------------------------------ moments
def moments_ref(x, defect=None):
    """-> (mom [72], gate [72]): x^T x at [k * 8 + c], the sums at [64 + c], zeros elsewhere"""
    P, C = x.shape
    xd = x.double()
    mom, gate = (torch.zeros(MOM_SIZE, dtype=torch.float64, device=x.device) for _ in range(2))
    M = xd.t() @ xd
    if defect == "lower_triangle_missing":
        M = torch.triu(M)
    mom[:MAXC * MAXC].view(MAXC, MAXC)[:C, :C] = M
    mom[MAXC * MAXC:MAXC * MAXC + C] = xd.sum(0)
    gate[:MAXC * MAXC].view(MAXC, MAXC)[:C, :C] = xd.abs().t() @ xd.abs()
    gate[MAXC * MAXC:MAXC * MAXC + C] = xd.abs().sum(0)
    return mom, gate * (P * 2.0 ** -52)


def moment_stats_ref(mom, W, P, lin_bias, gamma, beta, running_mean, running_var, momentum, eps):
    """-> dict of (want, gate): scale, shift, mean, rstd (+ running_mean, running_var), from the moments"""
    cout, C = W.shape
    W, mom = W.double(), mom.double()
    XtX, sx = mom[:MAXC * MAXC].view(MAXC, MAXC)[:C, :C], mom[MAXC * MAXC:MAXC * MAXC + C]
    s1, s2 = W @ sx, ((W @ XtX) * W).sum(1)
    out = E.bn_finalize_ref(torch.stack([s1, s2]).unsqueeze(0), P, lin_bias, gamma, beta, running_mean, running_var, momentum, eps)
    # the fp64 contractions cancel where the points are off-centre
    k = (C + 2) * 2.0 ** -52
    d1, d2 = k * (W.abs() @ sx.abs()) / P, k * ((W.abs() @ XtX.abs()) * W.abs()).sum(1) / P
    m0 = s1 / P
    var = (s2 / P - m0 * m0).clamp_min(0.0)
    amp2 = (d2 + 2 * m0.abs() * d1) / (2 * (var + eps))
    g, b = gamma.double(), beta.double()
    rstd = 1.0 / torch.sqrt(var + eps)
    extra = {"mean": d1, "rstd": amp2 * rstd, "scale": amp2 * (g * rstd).abs(),
             "shift": amp2 * (m0 * g * rstd).abs() + d1 * (g * rstd).abs(),
             "running_mean": d1, "running_var": 2 * (d2 + 2 * m0.abs() * d1)}
    return {k_: (v[0], v[1] + extra[k_]) for k_, v in out.items()}


# ------------------------------------------------------------------------------------------------ plain wgrad, cast
def wgrad_ref(dy, x, defect=None):
    """-> (dW [cout, C], gate)"""
    P, cout = dy.shape
    rl = rl_of(cout)
    xd, _, _ = _prep(x, x.new_zeros((cout, x.shape[1])), defect)
    d = dy.double()
    if defect == "swap_quads":
        d = E.swap_quads(d)
    w = row_weights(P, BWD_ROWS, 4, rl, defect, dy.device)
    S, Gt = _contract(d, torch.zeros_like(d), xd, w, cout, rl)
    return S.sum(0), Gt.sum(0) + atomic_gate(S)[0]


def cast_bf16_ref(src):
    """-> (plain [R, C], transposed [C, R]) bf16"""
    w = src.to(BF16)
    return w, w.t().contiguous()


def cast_values(R, C, sd, device="cpu"):
    """fp32 [R, C] of order 1 whose first elements are the cast's edge cases: +-0, ties, values that round up across a
    binade (1.9990234 -> 2, the largest fp32 below 1 -> 1), the smallest normal, a subnormal, a value next to bf16's
    largest"""
    v = E.uniform(R * C, sd, device, -2.0, 2.0).float()
    edge = torch.tensor([0.0, -0.0, 1.99902344, -3.9990234, 0.99999994, 1.00390625, 1.01171875, -1.00390625,
                         1.17549435e-38, 1e-40, 3.3895314e38, 255.5], dtype=F32, device=device)[:R * C]
    v[:edge.numel()] = edge
    return v.view(R, C)
