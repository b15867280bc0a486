"""fp64 restatements of the operations of csrc/elementwise.hip, the gate of each output, and planted defects.

Used by tests/test_elementwise_branches.py (the kernels, on the GPU) and tests/test_elementwise_gates_cpu.py (the gates
themselves, on the CPU).  Plain torch, device-agnostic: a reference runs where its inputs live, in float64.

Same stored values on both sides
--------------------------------
Every comparison hands the kernel and the reference the SAME stored numbers: a bf16 ``y`` is generated, rounded to
bf16, and that tensor is what the reference widens to float64; ``scale``, ``shift``, ``mean``, ``rstd``, ``coef`` are
fp32 tensors on both sides.  What is left between the two is the kernel's own fp32 arithmetic, so the gates below are
rounding-level.  Inputs come from a counter-based integer hash (``uniform``): the same bits on the CPU and on the device,
and a tensor with fewer groups is a prefix of the one with more -- the CPU file checks the gates at the values the GPU
file uses.

The gates, with u = 2^-24 (half an fp32 ulp, relative)
------------------------------------------------------
z = y*scale + shift;  T = |y*scale| + |shift| (the magnitudes summed to form z);  [z<=0] is 1 on the exponential branch.

* ELU(z), fp32 out (``bn_act_fwd``):  4u (T + [z<=0]) + [z<=0] u |z|.
  Roundings: the product and the sum (or one fma) give z to 2uT, which ELU passes on with slope <= 1.  On the
  exponential branch the fp32 kernels call expm1f (2 ulp = 4u of |a| <= 1); the bf16-storage kernels form
  exp2(z log2e) - 1: the argument product moves the result by u|z| e^z (the argument-rounding term), the hardware
  exp2 is good to 1 ulp (2u of e^z <= 1), the subtraction rounds once more (u|a|).  Both paths: <= 4 roundings of
  magnitudes bounded by T + 1, plus u|z|.  c = 4.
* ELU'(z) = e: relative error  rel_e = u (4T + [z<=0](|z| + 3)).
  2uT from z; the bf16 fused kernel folds log2e into scale and shift first (two more roundings of the same magnitudes,
  hence 4T); argument rounding |z|; exp 2u; for z > 0 the value 1 is exact, the 4uT only matters within rounding of 0.
* dz = g e (``bn_act_bwd_dz``; g = da, or dpool[group]*pool_scale):  |g| e (rel_e + 2u): pool_scale product, g*e product.
* dy = k0 dz + k1 y + k2 (``bn_bwd_dy``):  8u (|k0 dz| + |k1 y| + |k2|).  Two products and two sums: the worst case is
  3u (|k0 dz| + |k1 y|) + u |k2|, and c = 8 = twice the four roundings puts an evaluation that realises it at half
  the gate (with c = 4 the fp32 torch evaluation of the CPU file reached 0.60).
* dy = k0 (g e) + k1 y + k2 (``bn_bwd_dy_fused``):  |k0 g e| (rel_e + 2u) + 8u (|k0 g e| + |k1 y| + |k2|).
* any bf16 output: the above plus one bf16 rounding, 2^-8 |want|.  (The issue writes 2^-9; bf16 keeps 8 significant
  bits, so round-to-nearest moves a value by up to 2^-8 of itself: torch's own fp32 -> bf16 cast reached 1.99 x the
  2^-9 term.)  The rounding reaches the whole of its term by itself, so the CPU file holds the value before the
  rounding to half the fp32 part and the rounded value to the whole gate.
* a sum over R rows accumulated in fp32, s = the largest summand magnitude of that (group, channel):
    - the pooled mean, as the issue states it:  (R + SUM_PAD) u s on the mean itself, s = max_r |a| + 1 (the streaming
      kernel sums max(z,0) + e^min(z,0) and subtracts R at the end).  The sum reaches R s, every one of its R additions
      rounds by u of that, and the division by R brings the total back to R u s.
    - the sums that are not divided (e1 = sum_r e; e2 = sum_r e yhat and the second backward statistic with
      s = max_r |g| e (|y| + |mean|) rstd, yhat = y rstd - mean rstd cancelling; the first statistic sum_r dz):
      u (max(R s, sum of |every partial sum|) + SUM_PAD s), see ``sum_gate``.  The issue's (R + 16) u s assumes partial
      sums that stay near s; e1 adds R positive numbers, a pooled gradient gives dz one sign over a whole group, and
      e yhat has a positive mean (e is 1 where y is large): the partial sums reach R s / 2 and the fp32 evaluation of the
      CPU file exceeded (R + 16) u s by 8.3 x (e1), 3.9 x (e2) and 8.5 x (the pooled statistic) at R = 150 .. 255.  Each
      addition rounds by at most u |its result|, which is what the gate now adds up, in the kernels' order (row lanes).
    - SUM_PAD = 24 stands for the summands' own roundings (rel_e reaches 10 u at T = 2.7); with the issue's 16 the
      evaluation sat at 0.53 of the gate at R = 1 and R = 3.
    - the per-workgroup fp32 partials of the statistics kernels (``bn_act_bwd_dz``: 128 rows per workgroup;
      ``splitk_reduce_stats``: 32) then meet in fp64: the statistic's gate is the sum of its partials' gates, the fp64
      part is negligible.
* ``bn_pool_bwd_stats``: every summand (dpool*pool_scale)*e is two fp32 roundings and is added in fp64:
  2u sum_g |dpool pool_scale e|.
* ``splitk_reduce``: n fp32 terms (the slabs, and the previous contents under accumulate) added in order:
  n u sum |term| (recursive summation is bounded by (n - 1) u sum |term|; n keeps the two-term case at half).
* ``bn_finalize`` / ``bn_bwd_finalize``: fp64 arithmetic on fp64 statistics, one rounding to fp32 at the end.  A
  differently rounded last fp64 bit can move the result to the neighbouring fp32 value: 2^-23 |want|, plus the fp64
  cancellation of the expression, 2^-50 times the magnitudes it subtracts (amplified through 1/sqrt(var + eps) where the
  variance cancels: a constant column).  Running statistics: three fp32 roundings, 4u (|(1-mom) old| + |mom new|).
* ``bn_eval_coeffs`` (fp32): scale = gamma / sqrt(var + eps): sum, root, quotient, product: 8u |scale| (twice the four
  roundings, as for dy: 4u left the fp32 evaluation at 0.56);  shift = beta + (bias - mean) scale: those four, the
  difference, the product, the sum: 14u (|beta| + |(bias-mean) scale|).
* Adam, one step from the same fp32 state:  p: 2 ulp(p) + c_upd u step_size |m/denom| with 2 ulp(p) = 2^-22 |p|;
  m: 6u (|b1 m| + |(1-b1) g|) (grad_scale*g, (1-b1)*g, the fma: three roundings, doubled);  v: 4u v'.  The five rounding
  points of common.h::adam_update are m (fma), v (fma), denom (fma), the quotient, p (fma); around them sit
  grad_scale*g, the two products inside v, the root, and the fp32 roundings of step_size and 1/sqrt(1-b2^t).  The p
  fma's own rounding is the ulp(p) part.  The issue states c_upd = 4; every relative error of the update term counted
  once (m: 3, v through the root: 2, root, denom, 1/sqrt(bc2), quotient, step_size) gives 10, and with 4 the fp32
  evaluation reached 0.53 of the gate where |p| is small: ADAM_C_UPD = 10.  And |m/denom| is taken with the uncancelled
  magnitude of the new m, (|b1 m| + |(1-b1) g|) / denom: the roundings of m' are relative to its two terms, not to
  their sum (element 1 359 140 of the 3 000 001-element case: p = 9.3e-6, b1 m = 8.98e-3, (1-b1) g = -8.89e-3; the fp32
  evaluation sat at 1.16 of the gate relative to |m'/denom|).

Planted defects
---------------
``defect=`` of a reference returns what a subtly wrong kernel would have produced: "drop_last_row" (a group's last row
left out of its sums), "shift_rows" (every group reads rows one further on: the last row comes from the next group),
"swap_quads" (two adjacent channel quads exchange their coefficients), "next_group_grad" (the last row of group g takes
the pooled gradient of group g + 1), "swap_coef" (coef1 and coef2 exchanged).  ``moved`` counts, among the output
elements a defect touches at all, those it moves by more than 10 x the gate.
"""
import torch

U = 2.0 ** -24
BF16_ROUND = 2.0 ** -8      # bf16 keeps 8 significant bits: round-to-nearest moves a value by up to 2^-8 of itself
SUM_PAD = 24                   # the "+ 16" of the issue's sum gate, widened: see the module docstring
ADAM_C_UPD = 10                # the issue's 4, widened to the count of the module docstring

_M64 = (1 << 64)


def _s64(c):
    c %= _M64
    return c - _M64 if c >= (1 << 63) else c


_C0, _C1, _C2 = _s64(0x9E3779B97F4A7C15), _s64(0xBF58476D1CE4E5B9), _s64(0x94D049BB133111EB)


def uniform(n, seed, device="cpu", lo=0.0, hi=1.0):
    """n float64 values in [lo, hi): splitmix64 of (seed, index) in wrapping int64 arithmetic -- bit-identical on every
    device, and uniform(n1, seed) is a prefix of uniform(n2, seed)."""
    i = torch.arange(n, dtype=torch.int64, device=device)
    x = (i + 1) * _C0 + _s64(int(seed) * 0xD1B54A32D192ED03)
    x = (x ^ ((x >> 30) & ((1 << 34) - 1))) * _C1
    x = (x ^ ((x >> 27) & ((1 << 37) - 1))) * _C2
    x = x ^ ((x >> 31) & ((1 << 33) - 1))
    r = ((x >> 11) & ((1 << 53) - 1)).double() * 2.0 ** -53
    return r * (hi - lo) + lo


def activations(rows, ch, dtype, seed, device="cpu"):
    """[rows, ch] of order 1 (uniform, unit variance), rounded to the storage dtype"""
    return uniform(rows * ch, seed, device, -3.0 ** 0.5, 3.0 ** 0.5).view(rows, ch).to(dtype)


def bn_vectors(ch, seed, device="cpu"):
    """fp32 (scale, shift, mean, rstd): scale 1 +- 0.3 of either sign of shift +- 0.5"""
    scale = uniform(ch, seed + 1, device, 0.7, 1.3).float()
    shift = uniform(ch, seed + 2, device, -0.5, 0.5).float()
    mean = uniform(ch, seed + 3, device, -0.3, 0.3).float()
    rstd = uniform(ch, seed + 4, device, 0.8, 1.25).float()
    return scale, shift, mean, rstd


def coef_vectors(ch, seed, device="cpu", grad_scale=1.0):
    """fp32 [3, ch]: k0 1 +- 0.3, k1 and k2 +- 0.4 grad_scale.  k1 and k2 are means of the incoming gradient (times O(1)
    factors), so a pooled case, whose gradient per row is dpool / group_rows, passes grad_scale = 1 / group_rows: the
    three terms of dy then stay comparable, as they are in a training step"""
    k0 = uniform(ch, seed + 5, device, 0.7, 1.3)
    k12 = uniform(2 * ch, seed + 6, device, -0.4, 0.4).view(2, ch) * grad_scale
    return torch.cat([k0.view(1, ch), k12]).float().contiguous()


def gradient(rows, ch, dtype, seed, device="cpu"):
    return uniform(rows * ch, seed + 7, device, -1.0, 1.0).view(rows, ch).to(dtype)


def seed_of(a, b):
    """the seed of the case with these two defining sizes (channels and rows per group, say): both test files derive it here"""
    return 1 + (int(a) * 4099 + int(b) * 31) % 1000003


def finalize_case(ch, lin_bias, device="cpu", count=160, nrep=16):
    """BatchNorm statistics [nrep, 2, ch] (fp64) of ``count`` rows whose column 0 is constant, with the layer's vectors"""
    seed = seed_of(ch, count)
    y = uniform(count * ch, seed, device, -2.0, 2.0).view(count, ch)
    y[:, 0] = 3.0
    yr = y.view(nrep, count // nrep, ch)
    return {"stats": torch.stack([yr.sum(1), (yr * yr).sum(1)], 1).contiguous(), "count": count,
            "gamma": uniform(ch, seed + 1, device, 0.7, 1.3).float(), "beta": uniform(ch, seed + 2, device, -0.5, 0.5).float(),
            "rm": uniform(ch, seed + 3, device, -0.3, 0.3).float(), "rv": uniform(ch, seed + 4, device, 0.5, 1.5).float(),
            "lin_bias": uniform(ch, seed + 5, device, -0.3, 0.3).float() if lin_bias else None}


def adam_state(n, seed, device="cpu"):
    """fp32 (p, g, m, v) with non-zero moments"""
    return (uniform(n, seed + 20, device, -1.0, 1.0).float(), adam_gradient(n, seed, device),
            uniform(n, seed + 22, device, -0.05, 0.05).float(), uniform(n, seed + 23, device, 1e-4, 1e-2).float())


def adam_gradient(n, step, device="cpu"):
    return uniform(n, 1000 + step, device, -0.1, 0.1).float()


# ------------------------------------------------------------------------------------------------ defect helpers
def swap_quads(v):
    """the last dimension's adjacent channel quads exchanged (0<->1, 2<->3, ...; an odd last quad stays)"""
    ch = v.shape[-1]
    nq = ch // 4
    idx = torch.arange(ch, device=v.device).view(nq, 4)
    pairs = nq // 2 * 2
    perm = idx.clone()
    perm[0:pairs:2], perm[1:pairs:2] = idx[1:pairs:2], idx[0:pairs:2]
    return v[..., perm.reshape(-1)]


def swapped_channels(ch, device="cpu"):
    """bool [ch]: channels whose quad swap_quads moves"""
    m = torch.zeros(ch, dtype=torch.bool, device=device)
    m[: ch // 4 // 2 * 2 * 4] = True
    return m


def _vec(defect, *vs):
    vs = [v.double() for v in vs]
    return [swap_quads(v) for v in vs] if defect == "swap_quads" else vs


def elu(z):
    return torch.where(z > 0, z, torch.expm1(z))


def elu_grad(z):
    return torch.where(z > 0, torch.ones_like(z), torch.exp(z))


def _z(y, scale, shift):
    y = y.double()
    z = y * scale + shift
    return y, z, (y * scale).abs() + shift.abs(), (z <= 0).double()


def _rel_e(z, T, neg):
    return U * (4 * T + neg * (z.abs() + 3))


def out_gate(gate32, want, dtype):
    """the gate of a stored output: the fp32 gate, plus one bf16 rounding for bf16 storage"""
    return gate32 + (BF16_ROUND * want.abs() if dtype == torch.bfloat16 else 0.0)


def ratio(got, want, gate):
    """worst |err| / gate"""
    return float(((got.double() - want).abs() / gate.clamp_min(1e-300)).max())


def moved(want, bad, gate, mask=None, factor=10.0):
    """fraction of the (masked) elements a defect moves by more than factor x gate"""
    hit = (bad - want).abs() > factor * gate
    touched = bad != want               # e.g. ELU' is 1 on both sides of a coefficient swap where both z are positive
    if mask is not None:
        touched = touched & mask.expand_as(hit)
    return float(hit[touched].double().mean())


# ------------------------------------------------------------------------------------------------ element-wise family
def bn_act_fwd_ref(y, scale, shift, defect=None):
    """-> (a, gate32)"""
    scale, shift = _vec(defect, scale, shift)
    y, z, T, neg = _z(y, scale, shift)
    return elu(z), 4 * U * (T + neg) + neg * U * z.abs()


def _grad_rows(da, dpool, group_rows, pool_scale, rows, defect=None):
    if da is not None:
        return da.double()
    grp = torch.arange(rows, device=dpool.device) // group_rows
    if defect == "next_group_grad":
        last = (torch.arange(rows, device=dpool.device) % group_rows) == group_rows - 1
        grp = torch.where(last, (grp + 1).clamp_max(dpool.shape[0] - 1), grp)
    return (dpool.double() * float(torch.tensor(pool_scale, dtype=torch.float32)))[grp]


def last_rows_with_next(rows, group_rows, device="cpu"):
    """bool [rows, 1]: rows "next_group_grad" changes (the last row of every group but the last)"""
    r = torch.arange(rows, device=device)
    return ((r % group_rows == group_rows - 1) & (r < rows - group_rows)).view(rows, 1)


def bn_act_bwd_dz_ref(y, scale, shift, mean, rstd, *, da=None, dpool=None, group_rows=0, pool_scale=1.0, defect=None,
                      block_rows=128):
    """-> dict(dz, dz_gate32, stats [2, ch], stats_gate [2, ch]); "drop_last_row" leaves the last row of every group
    (dense: of every workgroup's block of rows) out of the statistics"""
    scale, shift, mean, rstd = _vec(defect, scale, shift, mean, rstd)
    y, z, T, neg = _z(y, scale, shift)
    rows, ch = y.shape
    g = _grad_rows(da, dpool, group_rows, pool_scale, rows, defect)
    e = elu_grad(z)
    dz = g * e
    dz_gate = g.abs() * e * (_rel_e(z, T, neg) + 2 * U)
    t1, t2 = dz, dz * ((y - mean) * rstd)
    m1, m2 = dz.abs(), dz.abs() * (y.abs() + mean.abs()) * rstd
    keep = torch.ones(rows, 1, dtype=torch.float64, device=y.device)
    if defect == "drop_last_row":
        per = group_rows if dpool is not None else block_rows
        keep[per - 1::per] = 0.0
        keep[rows - 1] = 0.0
    stats = torch.stack([(t1 * keep).sum(0), (t2 * keep).sum(0)])
    return {"dz": dz, "dz_gate": dz_gate, "stats": stats,
            "stats_gate": torch.stack([block_sum_gate(t1, m1, block_rows, row_lanes(ch)),
                                       block_sum_gate(t2, m2, block_rows, row_lanes(ch))])}


def sum_gate(x, mag, lanes=1):
    """the gate of an fp32 sum over dim 1 of the signed summands ``x`` [G, R, ch] (magnitude bounds ``mag``), added the
    way the kernels add: row r goes to lane r % lanes, a lane adds its rows in order, the lane sums are added in order.
    Every addition rounds by at most u |its result|:  u (max(R s, sum of |every partial sum|) + SUM_PAD s)."""
    G, R, ch = x.shape
    s = mag.amax(1)
    per = -(-R // lanes)
    px = torch.zeros((G, per * lanes, ch), dtype=x.dtype, device=x.device)
    px[:, :R] = x
    in_lane = px.view(G, per, lanes, ch).cumsum(1)
    partials = in_lane.abs().sum((1, 2)) + in_lane[:, -1].cumsum(1).abs().sum(1)
    return U * (torch.maximum(R * s, partials) + SUM_PAD * s)


def block_sum_gate(x, mag, block_rows, lanes=1):
    """sum of sum_gate over the blocks of rows: [rows, ch] -> [ch]"""
    rows, ch = mag.shape
    nb = -(-rows // block_rows)
    px, pm = (torch.zeros((nb * block_rows, ch), dtype=mag.dtype, device=mag.device) for _ in range(2))
    px[:rows], pm[:rows] = x, mag
    return sum_gate(px.view(nb, block_rows, ch), pm.view(nb, block_rows, ch), lanes).sum(0)


def bn_bwd_dy_ref(dz, y, coef, defect=None):
    """-> (dy, gate32)"""
    k0, k1, k2 = _coef(coef, defect)
    dz, y = dz.double(), y.double()
    return k0 * dz + k1 * y + k2, 8 * U * ((k0 * dz).abs() + (k1 * y).abs() + k2.abs())


def _coef(coef, defect):
    k0, k1, k2 = _vec(defect, *coef.double().unbind(0))
    return (k0, k2, k1) if defect == "swap_coef" else (k0, k1, k2)


def bn_bwd_dy_fused_ref(y, scale, shift, coef, *, da=None, dpool=None, group_rows=0, pool_scale=1.0, defect=None):
    """-> (dy, gate32)"""
    scale, shift = _vec(defect, scale, shift)
    k0, k1, k2 = _coef(coef, defect)
    y, z, T, neg = _z(y, scale, shift)
    g = _grad_rows(da, dpool, group_rows, pool_scale, y.shape[0], defect)
    t0 = k0 * g * elu_grad(z)
    mags = t0.abs() + (k1 * y).abs() + k2.abs()
    return t0 + k1 * y + k2, t0.abs() * (_rel_e(z, T, neg) + 2 * U) + 8 * U * mags


# ------------------------------------------------------------------------------------------------ mean-pool
def row_lanes(ch):
    """row lanes of the kernels whose 256 threads are (channel quad) x (row lane)"""
    return max(1, 256 // (ch // 4))


def meanpool_ref(y, scale, shift, mean, rstd, groups, group_rows, defect=None, lanes=1):
    """-> dict(pooled, e1, e2 [groups, ch] and their gates); lanes: 1 for the streaming kernel, row_lanes(ch) otherwise"""
    scale, shift, mean, rstd = _vec(defect, scale, shift, mean, rstd)
    R = group_rows
    y, z, T, neg = _z(y, scale, shift)
    ch = y.shape[1]
    if defect == "shift_rows":          # every group reads one row further on (the very last row: itself)
        idx = (torch.arange(y.shape[0], device=y.device) + 1).clamp_max(y.shape[0] - 1)
        y, z = y[idx], z[idx]
    a, e = elu(z), elu_grad(z)
    t2 = e * ((y - mean) * rstd)
    m2 = e * (y.abs() + mean.abs()) * rstd
    v = lambda t: t.view(groups, R, ch)
    keep = R - 1 if defect == "drop_last_row" else R
    out = {"pooled": v(a)[:, :keep].sum(1) / R, "e1": v(e)[:, :keep].sum(1), "e2": v(t2)[:, :keep].sum(1)}
    k = (R + SUM_PAD) * U
    out["pooled_gate"] = k * (v(a.abs()).amax(1) + 1)
    out["e1_gate"] = sum_gate(v(e), v(e), lanes)
    out["e2_gate"] = sum_gate(v(t2), v(m2), lanes)
    return out


def bn_pool_bwd_stats_ref(dpool, e, pool_scale, defect=None):
    """-> (stats [2, ch], gate [2, ch]); "drop_last_row": the last group left out"""
    ps = float(torch.tensor(pool_scale, dtype=torch.float32))
    t = (dpool.double() * ps).unsqueeze(0) * e.double()          # [2, groups, ch]
    keep = t.shape[1] - 1 if defect == "drop_last_row" else t.shape[1]
    return t[:, :keep].sum(1), 2 * U * t.abs().sum(1)


# ------------------------------------------------------------------------------------------------ finalize kernels
def bn_finalize_ref(stats, count, lin_bias, gamma, beta, running_mean, running_var, momentum, eps):
    """stats fp64 [nrep, 2, ch] -> dict of (want, gate) pairs; running_* may be None"""
    s = stats.double().sum(0)
    g, b = gamma.double(), beta.double()
    m0, ex2 = s[0] / count, s[1] / count
    var = (ex2 - m0 * m0).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    r32, c64 = 2.0 ** -23, 2.0 ** -50
    amp = c64 * (ex2.abs() + m0 * m0) / (2 * (var + eps))         # relative fp64 error of rstd where the variance cancels
    out = {"mean": (m0, r32 * m0.abs() + 1e-300), "rstd": (rstd, (r32 + amp) * rstd),
           "scale": (g * rstd, (r32 + amp) * (g * rstd).abs())}
    t = m0 * g * rstd
    out["shift"] = (b - t, r32 * (b - t).abs() + (c64 + amp) * (b.abs() + t.abs()))
    if running_mean is not None:
        mean = m0 + (lin_bias.double() if lin_bias is not None else 0.0)
        unbias = count / (count - 1) if count > 1 else 1.0
        mom1 = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(momentum, dtype=torch.float32))
        mom = float(torch.tensor(momentum, dtype=torch.float32))
        for name, old, new in (("running_mean", running_mean.double(), mean), ("running_var", running_var.double(), var * unbias)):
            mags = (mom1 * old).abs() + (mom * new).abs()
            out[name] = (mom1 * old + mom * new, 4 * U * mags + mom * (new.abs() * amp * 2 + c64 * (ex2.abs() + m0 * m0)))
    return out


def bn_bwd_finalize_ref(stats, count, gamma, mean, rstd):
    s = stats.double().sum(0)
    c1, c2 = s[0] / count, s[1] / count
    rs, mu = rstd.double(), mean.double()
    g = gamma.double() * rs
    r32, c64 = 2.0 ** -23, 2.0 ** -50
    k2a, k2b = -g * c1, g * c2 * rs * mu
    return {"dbeta": (s[0], r32 * s[0].abs() + 1e-300), "dgamma": (s[1], r32 * s[1].abs() + 1e-300),
            "coef0": (g, r32 * g.abs()), "coef1": (-g * c2 * rs, r32 * (g * c2 * rs).abs() + 1e-300),
            "coef2": (k2a + k2b, r32 * (k2a + k2b).abs() + c64 * (k2a.abs() + k2b.abs()) + 1e-300)}


def bn_eval_coeffs_ref(gamma, beta, running_mean, running_var, lin_bias, eps):
    """-> (scale, scale_gate, shift, shift_gate); eps as the fp32 value the kernel receives"""
    eps = float(torch.tensor(eps, dtype=torch.float32))
    sc = gamma.double() / torch.sqrt(running_var.double() + eps)
    d = (lin_bias.double() if lin_bias is not None else 0.0) - running_mean.double()
    return sc, 8 * U * sc.abs(), beta.double() + d * sc, 14 * U * (beta.double().abs() + (d * sc).abs())


# ------------------------------------------------------------------------------------------------ split-K reduction
def splitk_reduce_ref(slabs, nsplit, n, out0=None):
    """slabs fp32 [nsplit * n] -> (sum [n], gate [n]); out0: the previous contents under accumulate"""
    t = slabs.double()[: nsplit * n].view(nsplit, n)
    if out0 is not None:
        t = torch.cat([out0.double().view(1, n), t])
    return t.sum(0), t.shape[0] * U * t.abs().sum(0)


def colstats_of_ref(out, block_rows=32):
    ch = out.shape[1]
    """column statistics (sum, sum of squares) of the kernel's own fp32 result ``out`` [rows, ch] -> (stats, gate) [2, ch]"""
    o = out.double()
    return (torch.stack([o.sum(0), (o * o).sum(0)]),
            torch.stack([block_sum_gate(o, o.abs(), block_rows, row_lanes(ch)),
                         block_sum_gate(o * o, o * o, block_rows, row_lanes(ch))]))


# ------------------------------------------------------------------------------------------------ Adam
def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def adam_ref(p, g, m, v, lr, b1, b2, eps, step, grad_scale=1.0):
    """One torch.optim.Adam step (no amsgrad, no weight decay) in fp64 from the fp32 state (p, m, v) and gradient g.
    lr, betas, eps, grad_scale enter as the fp32 values the kernel receives.  -> dict of (want, gate)"""
    lr, b1, b2, eps, gs = f32(lr), f32(b1), f32(b2), f32(eps), f32(grad_scale)
    p, g, m, v = p.double(), g.double() * gs, m.double(), v.double()
    m1 = b1 * m + (1 - b1) * g
    v1 = b2 * v + (1 - b2) * g * g
    step_size = lr / (1 - b1 ** step)
    denom = torch.sqrt(v1) / (1 - b2 ** step) ** 0.5 + eps
    upd = step_size * m1 / denom
    mags = ((b1 * m).abs() + ((1 - b1) * g).abs()) / denom      # m' = b1 m + (1 - b1) g can cancel: its error does not
    return {"p": (p - upd, 2.0 ** -22 * p.abs() + ADAM_C_UPD * U * step_size * mags),
            "m": (m1, 6 * U * ((b1 * m).abs() + ((1 - b1) * g).abs()) + 1e-300),
            "v": (v1, 4 * U * v1 + 1e-300)}
