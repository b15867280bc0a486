"""fp64 restatements of the matrix products of csrc/gemm.hip, csrc/gemm_bf16.hip and csrc/gemm_v2.h, the gate of each
output, the launchers' dispatch as a plain-Python route table, the list of GPU cases, and planted defects.

Used by tests/test_gemm_branches.py (the kernels, on the GPU) and tests/test_gemm_gates_cpu.py (the gates, the route
table's coverage and the input conditions, on the CPU).  Plain torch, device-agnostic; ``uniform``, ``sum_gate``,
``BF16_ROUND``, ``U`` and the ELU / ELU' gates come from tests/elementwise_ref.py.

Same stored values on both sides
--------------------------------
An operand is generated as a LOGICAL [rows, K] float64 matrix (``logical``; ``uniform`` of a seed: the same bits on
every device, and fewer rows are a prefix of more), rounded to its storage dtype and laid out as the layout asks
(KC: [rows, K]; RC: [K, rows]) inside a larger NaN-filled allocation (``operand``: leading dimension, one-element base
offset).  The reference widens that stored window to float64 (``widen``); an fp32 operand under ``math=PCAA_BF16`` is
first rounded with torch's round-to-nearest-even cast, as the kernels' staging does.  Split operands are [hi | lo]
fp16 images (``split_image``, the restatement of pcaa_split_f16): the reference reads (hi + lo) / scale, exact in fp64,
subnormal lo halves included.  Operands are zero-mean (symmetric ranges): a stated condition of the statistical term.

Gates, with u = 2^-24; per output element S = sum_k |a_k b_k|, Q = sum_k (a_k b_k)^2, n = the terms one accumulator adds
-----------------------------------------------------------------------------------------------------------------
* fp32 accumulator:  u min(c_n S, C_STAT sqrt(n P2)),  P2 = Q / 6 + acc^2 / 3.  First term: recursive summation in ANY order is within
  (n - 1) u S; bf16 x bf16 and fp16 x fp16 products are exact in fp32 (c_n = n - 1), an fp32 operand makes every product
  round too: n more roundings of u |a_k b_k|, c_n = 2 n (CHANGED from the issue's c_n = n, which is the count of an fma
  chain: at K = 1 the one rounding of the one product reaches the whole of u |a b| by itself, and the fp32 evaluation of
  the 127 x 129 x 1 case sat at 0.99 of that gate).  Second term: every addition rounds by at most u |partial sum| (rms 0.42 u |partial sum| for
  a mantissa spread over a binade), independently, so the error's standard deviation is 0.42 u sqrt(sum_k partial_k^2).
  The partial sums of a zero-mean sum that ends at acc are a random bridge: E partial_k^2 = (k/n)^2 acc^2 + Q k (n - k) / n^2,
  on average over k  P2 = acc^2 / 3 + Q / 6.  C_STAT = 5 would put HALF the gate at 6 standard deviations of that model; an
  element's own partial sums scatter about P2 (more so over few terms), and the CPU file's half rule needs C_STAT = 8.5:
  with 5 the k-sequential evaluation of the 128 x 128 x 31 fp32 case sat at 0.808 of the gate, with 8.5 at 0.476.  CHANGED from
  the issue's 8 sqrt(n Q): that form ignores where the sum ends, and the error follows the partial sums -- slab 5 of the
  split3-slabs-8 case (192 lo.hi / hi.lo terms) has an element with acc = 2.7 sqrt(Q) whose k-sequential fp32 evaluation
  sat at 4.11 u sqrt(n Q), 0.514 of the gate, while the mean over the slab was 0.19 u sqrt(n Q): a constant large enough
  for such elements (10) is wide for every typical one.  With P2 and 8.5 the same evaluation is at the figure the CPU
  file prints, and the typical gate (acc^2 = Q) is 6 u sqrt(n Q).
* bias:  + u (|acc| + |bias|).      * bf16 output:  + BF16_ROUND |want|.
* slab split-K: each slab is a product over its own K range; the reduction adds n_s fp32 terms in order:
  n_s u sum |term| (the ``splitk_reduce`` gate of elementwise_ref.py) plus the slabs' own gates.
* atomic split-K / accumulate: the same magnitudes; (n - 1) u sum |term| holds for every order, n u sum |term| is used.
* split-fp16:  hi.hi + lo.hi + hi.lo with the lo.lo term dropped (|lo| <= 2^-11 |v| on both sides: 2^-22 S) and 3 K exact
  products accumulated: 2^-22 S + u min((3K - 1) S', C_STAT sqrt(K P2 + 2 K acc^2)) (hi.hi is walked first, the 2 K small
  terms are then added to the finished sum: their partial sums stay at acc), S' = S (1 + 2^-10); everything
  in the units of the fp32 tensors the images stand for (the kernel's out_scale = 1 / (s_A s_B) is a power of two).
* column statistics (sum v, sum v^2 of the bias-free accumulators): fp32 inside a slice of rows, the slices meet in
  fp64 atomics in replica (row tile % nrep).  Slice heights and row lanes, read from the kernels: 128-tile epilogue
  (fp32 kernel, small bf16 kernel) 64 rows, 2 lanes; register-staged 256-tile kernel 128 rows, 2 lanes; 4-wave loops
  128 rows, 8 lanes (4 lanes x the two halves of the packed accumulator pair).  Gate = ``sum_gate`` per slice, summed
  over the slices of a replica, plus the summands' own errors carried in.  CHANGED from the issue's starting form
  ("plus each summand's own product gate", i.e. the product gates added up): the sum of R accumulators is itself a
  zero-mean sum of R n products, so the carried part is again  u min(sum_i c_n S_i, C_STAT sqrt(sum_i n P2_i))  (and
  2 |v_i| times these for the squares, plus u v_i^2 for the square's own rounding).  Added up linearly the carried part
  grows with R while the defect "statistics from the bf16-rounded output" grows with sqrt(R): at the smallest shape of
  the fused path (256 rows, K = 320) that defect moved 13 % of the columns by 10 gates, against the 80 % the CPU
  file asks; with the statistical form it moves over 80 % (test_gemm_gates_cpu.py prints the figure).
* fused dgrad:  dz = da ELU'(z), z = y scale + shift:  (gate(da) + |da| (rel_e + 2u)) e, + the bf16 term for bf16 dz.
  Statistics {sum dz, sum dz yhat}, yhat = y rstd - mean rstd: as the column statistics, with m = |dz| (|y| + |mean|) rstd
  the magnitude bound of the second summand and its own roundings 4 u m added.
* affine + ELU epilogue:  a = ELU(scale acc + shift): the ELU gate of ``bn_act_fwd``, ELU_C u (T + [z<=0]) + [z<=0] u |z|,
  T = |scale acc| + |shift|, plus |scale| gate(acc) (ELU has slope <= 1).  The epilogue folds log2(e) into scale and
  shift and multiplies the linear branch back by ln 2 -- more roundings than ``bn_act_fwd`` -- but the accumulator's
  gate dominates: with the issue's ELU_C = 4 the fp32 evaluation of that formulation stays at 0.15, so 4 it is.
* pooled mean over R = pool_rows rows: (R + SUM_PAD) u (max |a| + 1) + the mean of the epilogue's own gates + the
  accumulators' errors carried as for the column statistics, |scale| min(sum_i c_n S_i, C_STAT sqrt(sum_i n P2_i)) / R
  (the mean of the elements' whole gates left the fp32 evaluation at 0.01 of the gate: 40 x wider than the rest).
No output element is left out of a comparison.

Planted defects (``defect=``): see ``DEFECTS``; each returns what a subtly wrong kernel would have produced.
"""
import torch

import elementwise_ref as E
from elementwise_ref import BF16_ROUND, SUM_PAD, U, sum_gate, uniform  # noqa: F401  (re-exported)

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
KC, RC = 0, 1
M_F32, M_BF16 = 0, 1                # PCAA_F32 / PCAA_BF16 of include/pcaa_hip.h
C_STAT = 8.5
ELU_C = 4.0
LOG2E = 1.4426950408889634

DEFECTS = ("drop_last_kstep", "drop_k_tail", "split_overlap", "split_gap", "stale_acc", "tile_twice", "tile_skipped",
           "ragged_row_wrap", "ragged_rows_in_stats", "ld_as_width", "bias_every_split", "bias_shift_col", "coef_shift_col",
           "stats_wrong_replica_lost", "stats_from_rounded", "pool_group_shift", "split_lo_swapped", "out_scale_once",
           "swap_layout_block")


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ inputs
def seed_of(M, N, K, which):
    return 1 + (M * 7919 + N * 4099 + K * 31 + which * 1009) % 1000003


def logical(rows, K, seed, device="cpu", amp=3.0 ** 0.5):
    """[rows, K] float64, uniform in [-amp, amp): unit variance at the default"""
    return uniform(rows * K, seed, device, -amp, amp).view(rows, K)


def logical_split(rows, K, seed, device="cpu", scale=1.0):
    """[rows, K] float64 with |scale v| in [16, 2048), either sign (the issue's range for the split-fp16 operands)"""
    r = uniform(rows * K, seed, device, -1.0, 1.0).view(rows, K)
    return torch.where(r < 0, -1.0, 1.0) * (16.0 + r.abs() * 2032.0) / scale


def operand(x64, dtype, layout, ld=None, off=0):
    """logical [rows, K] -> (buf, win): ``win`` is the stored window ([rows, K] for KC, [K, rows] for RC, row stride ld)
    inside the NaN-filled 1-D allocation ``buf``, starting ``off`` elements behind its (256-B aligned) base"""
    t = x64.to(dtype)
    return place(t.t() if layout == RC else t, ld, off)


def widen(win, layout, math):
    """the stored window as the kernel reads it -> logical [rows, K] float64"""
    t = win.to(BF16) if (math == M_BF16 and win.dtype == F32) else win
    t = t.double()
    return t.t() if layout == RC else t


def split_image(x64, scale):
    """restatement of pcaa_split_f16: fp32 [rows, ch] -> fp16 [rows, 2 ch] = [hi | lo], hi = fp16(s v), lo = fp16(s v - hi)"""
    v = x64.float() * float(scale)
    hi = v.to(F16)
    lo = (v - hi.float()).to(F16)
    return torch.cat([hi, lo], 1).contiguous()


def split_halves(img, scale, layout=KC):
    """-> (hi, lo) float64 as logical [rows, K], in the units of the fp32 tensor (RC: the image is that of the transpose)"""
    ch = img.shape[1] // 2
    hi, lo = img[:, :ch].double() / scale, img[:, ch:].double() / scale
    return (hi.t(), lo.t()) if layout == RC else (hi, lo)


def subnormal_lo_share(img):
    """share of the lo halves that are non-zero fp16 subnormals (|lo| < 2^-14)"""
    lo = img[:, img.shape[1] // 2:].double().abs()
    return float(((lo > 0) & (lo < 2.0 ** -14)).double().mean())


def vec4(n, seed, device="cpu", lo=-1.0, hi=1.0):
    return uniform(n, seed, device, lo, hi).float()


def out_gate(gate32, want, dtype):
    return gate32 + (BF16_ROUND * want.abs() if dtype == BF16 else 0.0)


ratio = E.ratio
moved = E.moved


# ------------------------------------------------------------------------------------------------ K ranges
def num_splits(math, K, split_k):
    """(nsplit, k_per_split) of gemm_num_splits (csrc/gemm.hip)"""
    bk = 64 if math == M_BF16 else 32
    kps = max(bk, cdiv(cdiv(K, split_k), bk) * bk)
    return cdiv(K, kps), kps


def k_ranges(math, K, split_k, defect=None):
    ns, kps = num_splits(math, K, split_k)
    rg = [(s * kps, min(K, (s + 1) * kps)) for s in range(ns)]
    step = 64 if math == M_BF16 else 32
    if defect == "split_overlap" and ns > 1:        # the first step of range 1 also counted by range 0
        rg[0] = (0, min(K, kps + step))
    if defect == "split_gap" and ns > 1:            # ... by neither
        rg[1] = (min(K, kps + step), rg[1][1])
    return rg


# ------------------------------------------------------------------------------------------------ the product
def acc_ref(a, b, exact, n=None, split_extra=False):
    """a [M, K], b [N, K] float64 -> dict(acc, worst, nq): the accumulator, u c_n S and n P2 (the sum of the squared
    partial sums, see the module docstring) per output element; gate = min(worst, C_STAT u sqrt(nq)).  ``n``: terms per
    accumulator if not K."""
    K = a.shape[1]
    n = K if n is None else n
    S = a.abs() @ b.abs().t()
    Q = (a * a) @ (b * b).t()
    acc = a @ b.t()
    nq = n * (Q / 6 + acc * acc / 3)
    if split_extra:                 # hi.hi is walked first: the K-long walk, then 2 K tiny terms added to the finished sum
        S = S * (1 + 2.0 ** -10)
        nq = (K * (Q / 6 + acc * acc / 3) + 2 * K * acc * acc) * (1 + 2.0 ** -10)
    return {"acc": acc, "worst": U * (n - 1 if exact else 2 * n) * S, "nq": nq, "S": S}


def acc_gate(r):
    return torch.minimum(r["worst"], C_STAT * U * torch.sqrt(r["nq"]))


def _zero_k(x, k0, k1=None):
    x = x.clone()
    x[:, k0:k1] = 0.0
    return x


def product_ref(a, b, *, exact, math=M_BF16, bias=None, split_k=1, out0=None, slabs=False, defect=None, tile=256, pre=None):
    """C = A . B^T (+ bias) over the K ranges of ``split_k`` (atomic unless ``slabs``), ``out0`` the previous contents under
    accumulate.  -> dict(want, gate [fp32 part], acc, r [acc_ref of the whole K], slabs [(want, gate) per range])"""
    M, K = a.shape
    N = b.shape[0]
    step = 64 if math == M_BF16 else 32
    if defect == "drop_last_kstep":
        a = _zero_k(a, (K - 1) // step * step)
    if defect == "drop_k_tail":
        chunk = 8 if math == M_BF16 else 4
        a = _zero_k(a, K // chunk * chunk)
    ranges = k_ranges(math, K, split_k, defect)
    parts = [pre] if (pre is not None and len(ranges) == 1 and defect is None) else \
        [acc_ref(a[:, k0:k1], b[:, k0:k1], exact) for k0, k1 in ranges]
    ns = len(parts)
    if ns == 1:
        r = parts[0]
        acc, gate = r["acc"], acc_gate(r)
    else:
        r = {"acc": sum(p["acc"] for p in parts), "worst": sum(p["worst"] for p in parts), "nq": sum(p["nq"] for p in parts)}
        terms = sum(p["acc"].abs() for p in parts) + (out0.double().abs() if out0 is not None else 0.0)
        acc = r["acc"]
        gate = sum(acc_gate(p) for p in parts) + (ns + (out0 is not None)) * U * terms
    if ns == 1 and out0 is not None:
        gate = gate + 2 * U * (acc.abs() + out0.double().abs())
    acc = _tile_defects(acc, defect, tile)
    want = acc + (out0.double() if out0 is not None and not slabs else 0.0)
    if defect == "tile_skipped":
        want[:min(tile, M), :min(tile, N)] = out0.double()[:min(tile, M), :min(tile, N)] if out0 is not None else 0.0
    if bias is not None:
        bv = bias.double()
        if defect == "bias_shift_col":
            bv = torch.roll(bv, -4)
        want = want + bv * (ns if defect == "bias_every_split" else 1)
        gate = gate + U * (acc.abs() + bv.abs())
    if defect == "ragged_row_wrap" and M % tile:
        pad = min(tile - M % tile, M)               # the rows past M are zeros (+ bias) and land on rows 0 ..
        want[:pad] = bias.double() if bias is not None else 0.0
    return {"want": want, "gate": gate, "acc": acc, "r": r, "dropped": 0.0,
            "slabs": [(p["acc"], acc_gate(p)) for p in parts]}


def _tile_defects(acc, defect, tile):
    M, N = acc.shape
    if defect == "stale_acc" and M > tile:          # every row tile but the first starts from the one before it
        acc = acc.clone()
        for t0 in range(tile, M, tile):
            h = min(tile, M - t0)
            acc[t0:t0 + h] += acc[t0 - tile:t0 - tile + h]
    if defect == "tile_twice":
        acc = acc.clone()
        acc[:min(tile, M), :min(tile, N)] *= 2
    if defect == "swap_layout_block":               # the first 8 x 8 block of every 32 x 32 fragment transposed
        acc = acc.clone()
        for r0 in range(0, M - 7, 32):
            for c0 in range(0, N - 7, 32):
                acc[r0:r0 + 8, c0:c0 + 8] = acc[r0:r0 + 8, c0:c0 + 8].t().clone()
    return acc


def ld_as_width(win):
    """the operand a kernel that addressed rows by the logical width would read: [r, w] taken densely from the window's
    first element on (the NaN padding it meets read as 0)"""
    r, w = win.shape
    ld = win.stride(0)
    flat = win.as_strided((r * ld,), (1,))[:r * w].clone()
    return torch.nan_to_num(flat.float(), nan=0.0).to(win.dtype).view(r, w)


def split_product_ref(ha, la, hb, lb, sb=1.0, *, split_k=1, defect=None, pre=None):
    """hi / lo halves (float64, logical [M, K] and [N, K], in the fp32 tensors' units) -> as product_ref (slab ranges over the
    3 K long walk hi.hi | lo.hi | hi.lo); sb: the B image's scale (for "out_scale_once"); pre: acc_ref of the same operands"""
    a, b = ha + la, hb + lb
    K = a.shape[1]
    r = pre if pre is not None else acc_ref(a, b, True, n=3 * K, split_extra=True)
    walked = ha @ hb.t() + la @ hb.t() + (la @ hb.t() if defect == "split_lo_swapped" else ha @ lb.t())
    want = r["acc"] if defect is None else walked
    if defect == "out_scale_once":
        want = want * sb
    dropped = r["lolo"] if "lolo" in r else (la @ lb.t()).abs()
    gate = dropped + acc_gate(r)
    out = {"want": want, "gate": gate, "acc": want, "r": r, "slabs": [], "dropped": dropped}
    if split_k > 1:
        # ranges of the concatenated contraction [hi_a | lo_a | hi_a] . [hi_b | hi_b | lo_b]
        ca, cb = torch.cat([ha, la, ha], 1), torch.cat([hb, hb, lb], 1)
        if defect == "split_lo_swapped":
            ca, cb = torch.cat([ha, la, la], 1), torch.cat([hb, hb, hb], 1)
        for k0, k1 in k_ranges(M_BF16, 3 * K, split_k, defect):
            p = acc_ref(ca[:, k0:k1], cb[:, k0:k1], True)
            out["slabs"].append((p["acc"], acc_gate(p)))
        terms = sum(s[0].abs() for s in out["slabs"])
        out["gate"] = dropped + sum(s[1] for s in out["slabs"]) + len(out["slabs"]) * U * terms
        if defect in ("split_overlap", "split_gap", "split_lo_swapped"):
            out["want"] = sum(s[0] for s in out["slabs"])
    return out


# ------------------------------------------------------------------------------------------------ column statistics
SLICES = {"tile128": (128, 64, 2), "staged256": (256, 128, 2), "v2": (256, 128, 8)}      # tile rows, slice rows, row lanes


def _slices(x, h):
    rows, ch = x.shape
    nb = cdiv(rows, h)
    px = torch.zeros((nb * h, ch), dtype=x.dtype, device=x.device)
    px[:rows] = x
    return px.view(nb, h, ch)


def replica_sums(x, mag, carried_worst, carried_nq, kernel, nrep, extra=None):
    """column sums of the summands ``x`` [rows, ch] per replica -> (want [nrep, ch], gate [nrep, ch]); ``mag`` bounds |x|,
    carried_worst / carried_nq: the summands' own worst-case error and n Q (see the module docstring), extra: further
    per-summand rounding"""
    tile, h, lanes = SLICES[kernel]
    xs, ms = _slices(x, h), _slices(mag, h)
    nb, ch = xs.shape[0], xs.shape[2]
    rep = (torch.arange(nb, device=x.device) // (tile // h)) % nrep
    carried = torch.stack([_slices(carried_worst, h).sum(1), _slices(carried_nq, h).sum(1)])
    ex = _slices(extra, h).sum(1) if extra is not None else 0.0
    want = torch.zeros((nrep, ch), dtype=torch.float64, device=x.device).index_add_(0, rep, xs.sum(1))
    g_sum = torch.zeros_like(want).index_add_(0, rep, sum_gate(xs, ms, lanes) + ex)
    cw = torch.zeros_like(want).index_add_(0, rep, carried[0])
    cq = torch.zeros_like(want).index_add_(0, rep, carried[1])
    return want, g_sum + torch.minimum(cw, C_STAT * U * torch.sqrt(cq)) + 1e-300


def colstats_ref(p, kernel, nrep, M=None, defect=None, cdt=F32):
    """statistics of the bias-free accumulators of product_ref's ``p`` -> (want [nrep, 2, ch], gate [nrep, 2, ch])"""
    v, r = p["acc"], p["r"]
    if defect == "stats_from_rounded":
        v = v.to(BF16).double()
    if defect == "ragged_rows_in_stats":
        tile = SLICES[kernel][0]
        pad = min((tile - v.shape[0] % tile) % tile, v.shape[0])        # the rows past M: taken as copies of rows 0 ..
        v = torch.cat([v, v[:pad]])
        r = {k: torch.cat([r[k], r[k][:pad]]) for k in ("worst", "nq")}
        p = dict(p, dropped=0.0)
    dr = p["dropped"] + torch.zeros_like(v)                    # split operands: the lo.lo term, a bias: added up
    w1, g1 = replica_sums(v, v.abs(), r["worst"], r["nq"], kernel, nrep, extra=dr)
    w2, g2 = replica_sums(v * v, v * v, 2 * v.abs() * r["worst"], 4 * v * v * r["nq"], kernel, nrep,
                          extra=U * v * v + 2 * v.abs() * dr)
    want, gate = torch.stack([w1, w2], 1), torch.stack([g1, g2], 1)
    if defect == "stats_wrong_replica_lost":
        want = want.clone()
        want[0] = 0.0
    return want, gate


# ------------------------------------------------------------------------------------------------ fused epilogues
def _shift_cols(v, defect):
    return torch.roll(v.double(), -4) if defect == "coef_shift_col" else v.double()


def dgrad_bn_ref(p, y, scale, shift, mean, rstd, nrep, dtype, defect=None):
    """p: product_ref / split_product_ref of da.  -> dict(dz, dz_gate [incl. bf16 term], stats [nrep, 2, ch], stats_gate)"""
    scale, shift, mean, rstd = (_shift_cols(t, defect) for t in (scale, shift, mean, rstd))
    da, r = p["want"], p["r"]
    yd = y.double()
    z = yd * scale + shift
    T, neg = (yd * scale).abs() + shift.abs(), (z <= 0).double()
    e = E.elu_grad(z)
    rel = E._rel_e(z, T, neg) + 2 * U
    dz = da * e
    dz_gate = (p["gate"] + da.abs() * rel) * e
    yh_mag = (yd.abs() + mean.abs()) * rstd
    yhat = (yd - mean) * rstd
    own = da.abs() * rel * e                                   # the epilogue's part of a summand's error: worst case, added
    cw, cq = r["worst"] * e + own, r["nq"] * e * e
    cw = cw + p["dropped"] * e                                 # split operands: the lo.lo term (a bias, not a rounding: added)
    v = dz
    if defect == "stats_from_rounded":
        v = dz.to(BF16).double()
    if defect == "ragged_rows_in_stats":
        pad = min((256 - v.shape[0] % 256) % 256, v.shape[0])
        cat = lambda t: torch.cat([t, t[:pad]])
        v, yhat, yh_mag, cw, cq = cat(v), cat(yhat), cat(yh_mag), cat(cw), cat(cq)
    w1, g1 = replica_sums(v, v.abs(), cw, cq, "v2", nrep)
    m2 = v.abs() * yh_mag
    w2, g2 = replica_sums(v * yhat, m2, cw * yh_mag, cq * yh_mag * yh_mag, "v2", nrep, extra=4 * U * m2)
    stats = torch.stack([w1, w2], 1)
    if defect == "stats_wrong_replica_lost":
        stats = stats.clone()
        stats[0] = 0.0
    return {"dz": dz, "dz_gate32": dz_gate, "dz_gate": out_gate(dz_gate, dz, dtype), "stats": stats, "stats_gate": torch.stack([g1, g2], 1)}


def affine_elu_ref(p, scale, shift, pool_rows=0, defect=None):
    """-> (want, gate, gate32): bf16 [M, N] (gate with the bf16 term, gate32 without) or the fp32 mean over groups of pool_rows rows"""
    scale, shift = _shift_cols(scale, defect), _shift_cols(shift, defect)
    acc = p["want"]
    z = acc * scale + shift
    T, neg = (acc * scale).abs() + shift.abs(), (z <= 0).double()
    a = E.elu(z)
    g = ELU_C * U * (T + neg) + neg * U * z.abs() + scale.abs() * p["gate"]
    if not pool_rows:
        return a, out_gate(g, a, BF16), g
    M, N = a.shape
    R = pool_rows
    grp = torch.arange(M, device=a.device) // R
    if defect == "pool_group_shift":
        last = torch.arange(M, device=a.device) % R == R - 1
        grp = torch.where(last, (grp + 1).clamp_max(M // R - 1), grp)
    want = torch.zeros((M // R, N), dtype=torch.float64, device=a.device).index_add_(0, grp, a) / R
    av, gv = a.view(M // R, R, N), g.view(M // R, R, N)
    # the elements' own errors: the epilogue's part added up, the accumulators' carried as for the column statistics (the
    # mean of R accumulators times scale is again a zero-mean sum of R n products)
    own = (g - scale.abs() * p["gate"]).view(M // R, R, N).mean(1)
    r = p["r"]
    cw = (scale.abs() * (r["worst"] + p["dropped"])).view(M // R, R, N).sum(1)
    cq = (scale * scale * r["nq"]).view(M // R, R, N).sum(1)
    gate = (R + SUM_PAD) * U * (av.abs().amax(1) + 1) + own + torch.minimum(cw, C_STAT * U * torch.sqrt(cq)) / R
    return want, gate, gate


# ------------------------------------------------------------------------------------------------ the route table
_DT = {F32: "f32", BF16: "bf16"}
_LAY = {KC: "KC", RC: "RC"}


def route(math, a_dtype, a_layout, b_dtype, b_layout, c_dtype, M, N, K, lda, ldb, ldc, split_k, accumulate, slabs, bias,
          colstats, v2_on, n_cu, aligned, *, split3=False, tail=False, tickets=True, rc_on=True):
    """The launchers' decisions (gemm_impl / gemm_split3_impl of csrc/gemm.hip, pcaa_launch_gemm_bf16_big / launch_dma of
    csrc/gemm_bf16.hip) restated: one name per distinct code path, ``refused/<reason>`` for an argument error.
    ``aligned``: True, or the set of operands ("A", "B", "C") whose base is 16-B aligned (a misaligned one sits one
    element off); ``slabs``: the slab entry points (c_split_stride != 0).  ``split3``: the [hi | lo] fp16 entry points
    (K is the logical contraction, lda / ldb cover the images).  A restatement on purpose, and now an observed one: the
    kernel a name implies (``kernel_id``) is what pcaa_gemm_route / pcaa_gemm_split3_route answer for every case, refusal
    and grid point (tests/test_gemm_route_cpu.py, no GPU needed) and what pcaa_gemm_last_kernel reports after every launch
    of tests/test_gemm_branches.py."""
    al = (lambda x: True) if aligned is True else (lambda x: x in aligned)
    if M <= 0 or N <= 0 or K <= 0:
        return "refused/bad_shape"
    if math not in (M_F32, M_BF16):
        return "refused/bad_math"
    if split_k < 1:
        return "refused/split_k"
    if split3:
        return _route_split3(a_layout, M, N, K, lda, ldb, ldc, split_k, slabs, colstats, v2_on, n_cu, al, tail, tickets, rc_on)
    need_a, need_b = (K if a_layout == KC else M), (K if b_layout == KC else N)
    if lda < need_a or ldb < need_b or ldc < N:
        return "refused/ld_too_small"
    atomic = (not slabs) and (split_k > 1 or accumulate)
    if atomic and c_dtype != F32:
        return "refused/atomic_needs_f32_c"
    if atomic and colstats:
        return "refused/colstats_need_one_pass"
    ns, kps = num_splits(math, K, split_k)
    if math == M_BF16:
        big = _route_big(a_dtype, a_layout, b_dtype, b_layout, c_dtype, M, N, K, lda, ldb, ldc, ns, kps, atomic, slabs, bias,
                         colstats, v2_on, n_cu, al, False, tail, tickets, rc_on)
        if big is not None:
            return big
        if a_dtype != BF16:
            return "refused/bf16_small_needs_bf16_a"
        if a_layout != KC or b_layout != KC:
            return "refused/bf16_small_needs_kc"
        if K % 8 or lda % 8 or ldb % 8:
            return "refused/bf16_small_needs_mult8"
        if not (al("A") and al("B")):
            return "refused/bf16_small_needs_alignment"
        return f"bf16_small/{_DT[b_dtype]},{_DT[c_dtype]}"
    if (a_dtype, b_dtype, c_dtype) not in ((F32, F32, F32), (BF16, BF16, F32), (BF16, F32, F32), (F32, F32, BF16)):
        return "refused/f32_dtype_combination"

    def vec_ok(name, lay, ld, rows):
        if not al(name) or ld % 4:
            return False
        return K % 4 == 0 if lay == KC else rows % 4 == 0
    vec = vec_ok("A", a_layout, lda, M) and vec_ok("B", b_layout, ldb, N)
    return f"f32/{_DT[a_dtype]},{_DT[b_dtype]},{_DT[c_dtype]}/{_LAY[a_layout]},{_LAY[b_layout]}/{'vec' if vec else 'scalar'}"


def persistent_grid(ntiles, n_cu):
    return min(ntiles, n_cu // 8 * 8 if n_cu >= 8 else 8)


def _v2_name(kind, M, ntiles, n_cu, bias, colstats, c_dtype, tail, tickets):
    rag = M % 256 != 0
    draw = tickets and ntiles > persistent_grid(ntiles, n_cu)
    if not colstats:
        st = "nostats"
    elif kind == "plain" and not rag and c_dtype == BF16 and not bias:
        st = "fused_stats"
    else:
        st = "sep_stats"
    return (f"v2/{kind}/{'ragged' if rag else 'whole'}/{'tickets' if draw else 'one_tile_each'}/{'bias' if bias else 'nobias'}/"
            f"{st}/{'tail' if (tail and colstats) else 'notail'}")


def _route_big(a_dtype, a_layout, b_dtype, b_layout, c_dtype, M, N, K, lda, ldb, ldc, ns, kps, atomic, slabs, bias, colstats,
               v2_on, n_cu, al, split3, tail, tickets, rc_on):
    """pcaa_launch_gemm_bf16_big: a route name, or None where it declines (split3: K is the walked contraction, 3 K)"""
    if N < 128 or lda % 8 or ldb % 8 or not (al("A") and al("B")):
        return None
    if (a_layout == KC or b_layout == KC) and K % 8:
        return None
    if (a_layout == RC and M % 8) or (b_layout == RC and N % 8):
        return None
    ntiles = cdiv(M, 256) * cdiv(N, 256)
    split_fast = bool(slabs) and ns >= 8 and ns % 8 == 0 and ntiles * ns >= 256
    m_ok = M % 256 == 0 or (a_layout == KC and ns == 1 and v2_on and K // 64 >= 5 and not atomic and not slabs)
    if (a_dtype == BF16 and b_dtype == BF16 and m_ok and N % 256 == 0 and K % 64 == 0 and kps % 64 == 0 and a_layout == b_layout):
        if a_layout == KC:
            if (v2_on and ns == 1 and not split_fast and not atomic and not slabs and K // 64 >= 5 and kps >= K
                    and ldc % 8 == 0 and al("C")):
                return _v2_name("split" if split3 else "plain", M, ntiles, n_cu, bias, colstats, c_dtype, tail, tickets)
        elif c_dtype == F32:
            if v2_on and rc_on and not atomic and M % 256 == 0 and not colstats and not bias:
                kind = "split" if split3 else "plain"
                return f"v2rc/{kind}/{'split_fast' if split_fast else ('slabs' if slabs else 'one_pass')}"
    if split3:
        return None
    inst = (_DT[a_dtype], _DT[b_dtype], _DT[c_dtype], _LAY[a_layout], _LAY[b_layout])
    served = {("bf16", "f32", "bf16", "KC", "KC"), ("bf16", "f32", "f32", "KC", "KC"), ("bf16", "bf16", "bf16", "KC", "KC"),
              ("bf16", "bf16", "f32", "KC", "KC"), ("f32", "f32", "f32", "KC", "KC"), ("bf16", "bf16", "f32", "RC", "RC"),
              ("f32", "f32", "f32", "RC", "RC"), ("f32", "f32", "f32", "KC", "RC")}
    if inst not in served:
        return None
    return "bf16_staged/%s,%s,%s,%s,%s" % inst


# PCAA_GEMM_KERNEL_* of include/pcaa_hip.h by the first component of a route name
KERNEL_IDS = {"f32": 0, "bf16_small": 1, "bf16_staged": 2, "v2": 3, "v2rc": 4, "v2_dgrad": 3, "v2_affine": 3, "refused": -1}


def kernel_id(route_name):
    return KERNEL_IDS[route_name.split("/")[0]]


def split3_supported(M, N, K, v2_on):
    """pcaa_gemm_split3_supported (the 4 GiB bound on the padded rows is out of reach at test size)"""
    return M > 0 and N > 0 and K > 0 and v2_on and 3 * K >= 320 and (M % 256 == 0 or K >= 320) and N % 256 == 0 and K % 64 == 0


def dgrad_bn_supported(M, N, K, v2_on):
    return M > 0 and N > 0 and K >= 320 and v2_on and N % 256 == 0 and K % 64 == 0


def _route_split3(layout, M, N, K, lda, ldb, ldc, split_k, slabs, colstats, v2_on, n_cu, al, tail, tickets, rc_on):
    if not split3_supported(M, N, K, v2_on) or (layout == RC and M % 256):
        return "refused/split3_shape"
    if M % 256 and (split_k > 1 or slabs):
        return "refused/split3_ragged_needs_one_pass"
    if M % 256 and (ldc % 8 or not al("C")):
        return "refused/ragged_out"
    cols_a, cols_b = (2 * K, 2 * K) if layout == KC else (2 * M, 2 * N)
    if lda < cols_a or ldb < cols_b or ldc < N or lda % 8 or ldb % 8:
        return "refused/split3_ld"
    if not (al("A") and al("B")):
        return "refused/split3_alignment"
    if colstats and (split_k > 1 or slabs):
        return "refused/colstats_need_one_pass"
    ns, kps = num_splits(M_BF16, 3 * K, split_k)
    big = _route_big(BF16, layout, BF16, layout, F32, M, N, 3 * K, 8, 8, ldc, ns, kps, False, slabs, False, colstats, v2_on, n_cu,
                     al, True, tail, tickets, rc_on)
    return big if big is not None else "refused/split3_not_served"


def route_fused(epi, M, N, K, ld_a, ld_b, ld_out, v2_on, n_cu, aligned=True, *, split3=False, pool_rows=0, tail=False, tickets=True):
    """pcaa_gemm_dgrad_bn[_split3] (epi "dgrad") and pcaa_gemm_affine_elu (epi "affine"): their own instantiations of
    the KC x KC loop.  ld_out: the leading dimension of y / dz, or of the (pooled) output."""
    al = (lambda x: True) if aligned is True else (lambda x: x in aligned)
    if epi == "affine" and pool_rows not in (0, 32, 64, 128):
        return "refused/pool_rows"
    ok = split3_supported(M, N, K, v2_on) if split3 else dgrad_bn_supported(M, N, K, v2_on)
    if not ok:
        return "refused/fused_shape"
    need = 2 * K if split3 else K
    ld_mult = 4 if (split3 and epi == "dgrad") else (8 if not (epi == "affine" and pool_rows) else 1)
    if ld_a < need or ld_b < need or ld_out < N or ld_a % 8 or ld_b % 8 or ld_out % ld_mult:
        return "refused/fused_ld"
    if epi == "dgrad" and M % 256 and (ld_out % 8 or not al("C")):
        return "refused/ragged_out"
    if not (al("A") and al("B") and al("C")):
        return "refused/fused_alignment"
    if epi == "affine" and M % 256 and (ld_out % 8 or not al("C")):
        return "refused/ragged_out"
    ntiles = cdiv(M, 256) * (N // 256)
    draw = tickets and ntiles > persistent_grid(ntiles, n_cu)
    shape = f"{'ragged' if M % 256 else 'whole'}/{'tickets' if draw else 'one_tile_each'}"
    if epi == "dgrad":
        return f"v2_dgrad/{'split' if split3 else 'plain'}/{shape}/{'tail' if tail else 'notail'}"
    return f"v2_affine/pool{pool_rows}/{shape}"


# ------------------------------------------------------------------------------------------------ the GPU cases
def _c(id, route, M, N, K, **kw):
    d = dict(id=id, route=route, M=M, N=N, K=K, math=M_BF16, adt=BF16, alay=KC, bdt=BF16, blay=KC, cdt=F32, lda=None, ldb=None,
             ldc=None, split_k=1, accumulate=False, slabs=False, bias=False, colstats=False, tail=False, v2_on=True,
             misaligned=(), nrep=16, split3=False, defects=())
    d.update(kw)
    return d


def case_lds(c):
    """(lda, ldb, ldc) of a case: the logical widths unless it pads them"""
    wa = c["K"] if c["alay"] == KC else c["M"]
    wb = c["K"] if c["blay"] == KC else c["N"]
    if c["split3"]:
        wa, wb = 2 * wa, 2 * wb
    return c["lda"] or wa, c["ldb"] or wb, c["ldc"] or c["N"]


def case_route(c, n_cu, tickets=True, rc_on=True):
    lda, ldb, ldc = case_lds(c)
    aligned = True if not c["misaligned"] else {"A", "B", "C"} - set(c["misaligned"])
    return route(c["math"], c["adt"], c["alay"], c["bdt"], c["blay"], c["cdt"], c["M"], c["N"], c["K"], lda, ldb, ldc,
                 c["split_k"], c["accumulate"], c["slabs"], c["bias"], c["colstats"], c["v2_on"], n_cu, aligned,
                 split3=c["split3"], tail=c["tail"], tickets=tickets, rc_on=rc_on)


F32_TRIPLES = [(F32, F32, F32), (BF16, BF16, F32), (BF16, F32, F32), (F32, F32, BF16)]
LAYOUTS = [(KC, KC), (KC, RC), (RC, KC), (RC, RC)]


def gemm_cases(n_cu):
    """the cases of ``pcaa_gemm`` / ``pcaa_gemm_slabs`` / the split3 products: each names the route it means to reach"""
    cs = []
    f = lambda a, b, c, al, bl, v: f"f32/{_DT[a]},{_DT[b]},{_DT[c]}/{_LAY[al]},{_LAY[bl]}/{v}"
    # ---- fp32 math: every dtype triple x layout pair, vec and scalar by shape (K % 4 for KC, rows % 4 for RC)
    for a, b, c in F32_TRIPLES:
        for al, bl in LAYOUTS:
            t = f"{_DT[a]}{_DT[b]}{_DT[c]}-{_LAY[al]}{_LAY[bl]}"
            cs.append(_c(f"f32-vec-{t}", f(a, b, c, al, bl, "vec"), 132, 136, 36, math=M_F32, adt=a, bdt=b, cdt=c, alay=al, blay=bl,
                         bias=True, defects=("bias_shift_col",) if (al, bl) == (KC, KC) else ()))
            cs.append(_c(f"f32-scalar-{t}", f(a, b, c, al, bl, "scalar"), 129, 127, 33, math=M_F32, adt=a, bdt=b, cdt=c, alay=al,
                         blay=bl, defects=("drop_k_tail",) if (a, c, al, bl) == (F32, F32, KC, KC) else ()))
    v = f(F32, F32, F32, KC, KC, "vec")
    s = f(F32, F32, F32, KC, KC, "scalar")
    # ---- vec / scalar by the leading dimension and by the base pointer
    cs.append(_c("f32-vec-ld-padded", v, 128, 128, 32, math=M_F32, adt=F32, bdt=F32, lda=40, ldb=36, ldc=140, defects=("ld_as_width",)))
    cs.append(_c("f32-scalar-by-ld", s, 128, 128, 32, math=M_F32, adt=F32, bdt=F32, lda=33, ldb=35))
    cs.append(_c("f32-scalar-by-pointer-A", s, 128, 128, 32, math=M_F32, adt=F32, bdt=F32, misaligned=("A",)))
    cs.append(_c("f32-scalar-by-pointer-B", f(F32, F32, F32, RC, RC, "scalar"), 128, 128, 32, math=M_F32, adt=F32, bdt=F32, alay=RC,
                 blay=RC, misaligned=("B",)))
    cs.append(_c("f32-scalar-by-pointer-bf16", f(BF16, BF16, F32, KC, KC, "scalar"), 128, 128, 32, math=M_F32, misaligned=("A",)))
    # ---- tile edges and K = 1, 31, 32, 33
    for m, n, k in [(127, 129, 1), (128, 128, 31), (129, 127, 32), (257, 130, 33)]:
        cs.append(_c(f"f32-edge-{m}x{n}x{k}", v if k % 4 == 0 else s, m, n, k, math=M_F32, adt=F32, bdt=F32,
                     defects=("drop_last_kstep",) if k == 33 else ()))
    # ---- K ranges: a partial last range; fewer ranges than asked; atomics with bias and accumulate; slabs; statistics
    cs.append(_c("f32-atomic-partial-last-range", v, 130, 132, 100, math=M_F32, adt=F32, bdt=F32, split_k=3, bias=True,
                 defects=("bias_every_split", "split_overlap", "split_gap", "tile_twice", "tile_skipped")))
    cs.append(_c("f32-atomic-fewer-ranges", v, 64, 132, 40, math=M_F32, adt=F32, bdt=F32, split_k=5, accumulate=True))
    cs.append(_c("f32-accumulate-one-range", v, 64, 132, 40, math=M_F32, adt=F32, bdt=F32, accumulate=True))
    cs.append(_c("f32-slabs", f(F32, F32, F32, RC, RC, "vec"), 132, 136, 200, math=M_F32, adt=F32, bdt=F32, alay=RC, blay=RC,
                 slabs=True, split_k=4))
    cs.append(_c("f32-colstats-three-row-tiles", v, 300, 132, 64, math=M_F32, adt=F32, bdt=F32, colstats=True, bias=True, nrep=2,
                 defects=("stats_wrong_replica_lost",)))
    # ---- bf16 math, small kernel (N < 128, or declined by the big launcher)
    sm = lambda b, c: f"bf16_small/{_DT[b]},{_DT[c]}"
    for b, c in [(BF16, BF16), (BF16, F32), (F32, BF16), (F32, F32)]:
        cs.append(_c(f"small-{_DT[b]}-{_DT[c]}", sm(b, c), 130, 120, 72, bdt=b, cdt=c, bias=True, colstats=True,
                     defects=("drop_last_kstep",) if c == F32 else ()))
    cs.append(_c("small-atomic", sm(BF16, F32), 130, 100, 200, split_k=2, bias=True))
    # ---- bf16 math, register-staged 256-tile kernel: every instantiation, by the cheapest declining condition
    st = lambda a, b, c, al, bl: "bf16_staged/%s,%s,%s,%s,%s" % (_DT[a], _DT[b], _DT[c], _LAY[al], _LAY[bl])
    cs.append(_c("staged-bf16f32-bf16-by-fp32-B", st(BF16, F32, BF16, KC, KC), 300, 260, 72, bdt=F32, cdt=BF16, bias=True,
                 colstats=True, defects=("bias_shift_col",)))
    cs.append(_c("staged-bf16f32-f32-by-fp32-B", st(BF16, F32, F32, KC, KC), 256, 256, 320, bdt=F32))
    cs.append(_c("staged-bf16bf16-bf16-by-short-K", st(BF16, BF16, BF16, KC, KC), 256, 256, 256, cdt=BF16, colstats=True))
    cs.append(_c("staged-bf16bf16-f32-by-N", st(BF16, BF16, F32, KC, KC), 257, 136, 328, bias=True, defects=("ragged_row_wrap",)))
    cs.append(_c("staged-bf16bf16-bf16-by-v2-off", st(BF16, BF16, BF16, KC, KC), 256, 256, 320, cdt=BF16, v2_on=False))
    cs.append(_c("staged-bf16bf16-f32-by-atomics", st(BF16, BF16, F32, KC, KC), 256, 256, 640, split_k=2, bias=True))
    cs.append(_c("staged-f32f32-f32-KCKC", st(F32, F32, F32, KC, KC), 130, 256, 72, adt=F32, bdt=F32))
    cs.append(_c("staged-f32f32-f32-KCRC", st(F32, F32, F32, KC, RC), 130, 264, 72, adt=F32, bdt=F32, blay=RC))
    cs.append(_c("staged-f32f32-f32-RCRC", st(F32, F32, F32, RC, RC), 264, 136, 100, adt=F32, bdt=F32, alay=RC, blay=RC,
                 defects=("swap_layout_block",)))
    cs.append(_c("staged-bf16bf16-f32-RCRC-by-M", st(BF16, BF16, F32, RC, RC), 264, 256, 128, alay=RC, blay=RC))
    cs.append(_c("staged-RCRC-atomics", st(BF16, BF16, F32, RC, RC), 256, 256, 256, alay=RC, blay=RC, split_k=3))
    cs.append(_c("staged-RCRC-slabs-7-ragged", st(BF16, BF16, F32, RC, RC), 264, 256, 448, alay=RC, blay=RC, slabs=True, split_k=7))
    # (the register-staged kernel's own split_fast grid remap -- block_coords, shared by all its instantiations; the route
    # name does not mark it: 8 ranges x 2 x 16 tiles = 256 workgroups, a partial last row tile keeps the 4-wave loop away)
    cs.append(_c("staged-RCRC-slabs-8-ragged-split-fast", st(BF16, BF16, F32, RC, RC), 264, 4096, 512, alay=RC, blay=RC, slabs=True,
                 split_k=8))
    cs.append(_c("staged-KCKC-ld-padded", st(BF16, BF16, F32, KC, KC), 256, 256, 128, lda=136, ldb=144, ldc=260,
                 defects=("ld_as_width",)))
    # ---- 4-wave loop, RC x RC
    cs.append(_c("v2rc-one-pass", "v2rc/plain/one_pass", 256, 256, 128, alay=RC, blay=RC))
    cs.append(_c("v2rc-slabs-one-step-each", "v2rc/plain/slabs", 256, 256, 448, alay=RC, blay=RC, slabs=True, split_k=7,
                 defects=("split_overlap", "split_gap")))
    cs.append(_c("v2rc-slabs-several-steps", "v2rc/plain/slabs", 256, 512, 384, alay=RC, blay=RC, slabs=True, split_k=3,
                 defects=("drop_last_kstep",)))
    # (split_fast: 8 ranges x 32 tiles = 256 workgroups, the smallest that reaches it; the same product asked for 7 ranges)
    cs.append(_c("v2rc-split-fast-8", "v2rc/plain/split_fast", 2048, 1024, 512, alay=RC, blay=RC, slabs=True, split_k=8))
    cs.append(_c("v2rc-not-split-fast-7", "v2rc/plain/slabs", 2048, 1024, 512, alay=RC, blay=RC, slabs=True, split_k=7))
    cs.append(_c("v2rc-declined-by-colstats", st(BF16, BF16, F32, RC, RC), 256, 256, 128, alay=RC, blay=RC, colstats=True))
    cs.append(_c("v2rc-declined-by-bias", st(BF16, BF16, F32, RC, RC), 256, 256, 128, alay=RC, blay=RC, bias=True))
    # ---- 4-wave loop, KC x KC: K = 320; every combination of the epilogue's branches at one tile each ...
    for r in (0, 1, 127, 128, 129, 255):
        M = 256 + r if r else 512
        for cdt in (BF16, F32):
            for bias in (False, True):
                for stats, tail in ((False, False), (True, False), (True, True)):
                    c = _c(f"v2-r{r}-{_DT[cdt]}-{'bias' if bias else 'nobias'}-{'stats' if stats else 'nostats'}{'-tail' if tail else ''}",
                           None, M, 256, 320, cdt=cdt, bias=bias, colstats=stats, tail=tail)
                    if r not in (0, 129) and (bias or tail or not stats) and cdt == F32:
                        continue                    # the remaining ragged heights: the statistics' row select, and bf16 C
                    c["route"] = _v2_name("plain", M, cdiv(M, 256), n_cu, bias, stats, cdt, tail, True)
                    cs.append(c)
    for c in cs:
        if c["id"] == "v2-r0-bf16-nobias-stats":
            c["defects"] = ("stats_from_rounded", "stale_acc", "drop_last_kstep")
        if c["id"] == "v2-r129-f32-nobias-stats":
            c["defects"] = ("ragged_rows_in_stats", "ragged_row_wrap")
        if c["id"] == "v2-r0-bf16-bias-nostats":
            c["defects"] = ("bias_shift_col",)
    # ... tile counts 1, 7, 8, 9 (N = 256) and three column tiles, ldc > N
    for t in (1, 7, 9):
        cs.append(_c(f"v2-{t}-tiles", _v2_name("plain", 256 * t, t, n_cu, False, True, BF16, False, True), 256 * t, 256, 320, cdt=BF16,
                     colstats=True, nrep=4, defects=("stats_wrong_replica_lost",) if t == 7 else ()))
    cs.append(_c("v2-8-tiles-ldc-padded", _v2_name("plain", 1024, 8, n_cu, True, False, F32, False, True), 1024, 512, 320, ldc=520,
                 lda=328, ldb=336, bias=True, defects=("ld_as_width",)))
    cs.append(_c("v2-declined-by-ldc", st(BF16, BF16, F32, KC, KC), 256, 256, 320, ldc=260))
    cs.append(_c("v2-declined-by-misaligned-C", st(BF16, BF16, BF16, KC, KC), 256, 256, 320, cdt=BF16, misaligned=("C",)))
    # ... and around the CU count: the last engages the ticket draw with a tile count that is no multiple of 8
    g = persistent_grid(1 << 30, n_cu)
    for t in (g - 1, g):
        cs.append(_c(f"v2-cus{t - g:+d}-tiles", _v2_name("plain", 256 * t, t, n_cu, False, False, BF16, False, True), 256 * t, 256, 320,
                     cdt=BF16))
    for cdt in (BF16, F32):
        for bias in (False, True):
            for stats, tail in ((False, False), (True, False), (True, True)):
                for r in (0, 77):
                    M = 256 * (g + 11) - (256 - r if r else 0)
                    cs.append(_c(f"v2-tickets-r{r}-{_DT[cdt]}-{'bias' if bias else 'nobias'}-{'stats' if stats else 'nostats'}"
                                 f"{'-tail' if tail else ''}", _v2_name("plain", M, g + 11, n_cu, bias, stats, cdt, tail, True),
                                 M, 256, 320, cdt=cdt, bias=bias, colstats=stats, tail=tail, big=True))
    # ---- split-fp16 products
    for lay, M in ((KC, 512), (KC, 300), (RC, 256)):
        for stats, tail in ((False, False), (True, False), (True, True)):
            if lay == RC and stats:
                continue
            cs.append(_c(f"split3-{_LAY[lay]}-{M}-{'stats' if stats else 'nostats'}{'-tail' if tail else ''}",
                         (_v2_name("split", M, cdiv(M, 256), n_cu, False, stats, F32, tail, True) if lay == KC else "v2rc/split/one_pass"),
                         M, 256, 128 if M != 300 else 320, alay=lay, blay=lay, split3=True, colstats=stats, tail=tail,
                         defects=("out_scale_once",) if (lay == KC and M == 512 and not stats) else ()))
    for r in (0, 77):
        for stats, tail in ((False, False), (True, False), (True, True)):
            M = 256 * (g + 11) - (256 - r if r else 0)
            cs.append(_c(f"split3-tickets-r{r}-{'stats' if stats else 'nostats'}{'-tail' if tail else ''}",
                         _v2_name("split", M, g + 11, n_cu, False, stats, F32, tail, True), M, 256, 320 if r else 128, split3=True,
                         colstats=stats, tail=tail, big=True))
    for sk in (2, 6, 8):        # (8: K = 512, ranges of 192 that straddle the hi.hi | lo.hi | hi.lo segments, 8 x 32 workgroups)
        cs.append(_c(f"split3-slabs-{sk}", "v2rc/split/split_fast" if sk == 8 else "v2rc/split/slabs", 256 if sk != 8 else 2048,
                     256 if sk != 8 else 1024, 128 if sk != 8 else 512, alay=RC, blay=RC, split3=True, slabs=True, split_k=sk,
                     defects=("split_lo_swapped",) if sk == 6 else ()))
    return cs


def route_grid(n_cu=256):
    """the grid of ``route``'s arguments that ``all_routes`` walks (the conditions of the launchers taken both ways), as
    case dicts.  The slab entry points have an fp32 result without bias or statistics: no other slab call exists."""
    g = persistent_grid(1 << 30, n_cu)
    for math in (M_F32, M_BF16):
        for a, b, c in [(x, y, z) for x in (F32, BF16) for y in (F32, BF16) for z in (F32, BF16)]:
            for al, bl in LAYOUTS:
                for M, N, K in [(129, 127, 33), (132, 136, 36), (130, 120, 72), (256, 256, 320), (300, 256, 320), (264, 256, 128),
                                (256, 256, 128), (256 * (g + 11), 256, 320), (256 * (g + 11) - 100, 256, 320), (2048, 1024, 512)]:
                    for sk, acc, slabs in [(1, False, False), (2, False, False), (1, True, False), (2, False, True), (8, False, True)]:
                        for bias in (False, True):
                            for stats, tail in ((False, False), (True, False), (True, True)):
                                if slabs and (c != F32 or bias or stats):
                                    continue
                                for v2 in (True, False):
                                    yield _c("grid", None, M, N, K, math=math, adt=a, bdt=b, cdt=c, alay=al, blay=bl, split_k=sk,
                                             accumulate=acc, slabs=slabs, bias=bias, colstats=stats, tail=tail, v2_on=v2)
    for lay in (KC, RC):
        for M, N, K in [(256, 256, 128), (300, 256, 320), (256 * (g + 11), 256, 128), (256 * (g + 11) - 100, 256, 320), (2048, 1024, 512)]:
            for sk, slabs in [(1, False), (2, True), (8, True)]:
                for stats, tail in ((False, False), (True, False), (True, True)):
                    yield _c("grid", None, M, N, K, alay=lay, blay=lay, split3=True, split_k=sk, slabs=slabs, colstats=stats, tail=tail)


def all_routes(n_cu=256):
    """every name ``route`` returns over the supported domain, enumerated from the function itself on ``route_grid``,
    refusals left out"""
    names = {case_route(c, n_cu) for c in route_grid(n_cu)}
    return {n for n in names if not n.startswith("refused/")}


def fused_cases(n_cu):
    """pcaa_gemm_dgrad_bn[_split3] and pcaa_gemm_affine_elu"""
    cs = []
    g = persistent_grid(1 << 30, n_cu)
    for split3 in (False, True):
        for M, ld, tail in [(512, None, False), (512, 264, True), (300, None, True), (256 + 129, 272, False)]:
            K = 128 if (split3 and M % 256 == 0) else 320
            cs.append(dict(id=f"dgrad{'-split3' if split3 else ''}-{M}{'-ld%d' % ld if ld else ''}{'-tail' if tail else ''}", epi="dgrad",
                           M=M, N=256, K=K, ld=ld, tail=tail, split3=split3, pool_rows=0,
                           defects=("coef_shift_col", "stats_from_rounded") if (M == 512 and ld is None and not split3) else
                           (("ragged_rows_in_stats",) if (M == 300 and not split3) else ())))
    big = 256 * (g + 11) - 128            # ragged, and whole mean-pool groups
    for split3 in (False, True):
        for tail in (False, True):
            cs.append(dict(id=f"dgrad{'-split3' if split3 else ''}-tickets{'-tail' if tail else ''}", epi="dgrad", M=big, N=256, K=320,
                           ld=None, tail=tail, split3=split3, pool_rows=0, defects=(), big=True))
    for pool in (0, 32, 64, 128):
        cs.append(dict(id=f"affine-pool{pool}-tickets", epi="affine", M=big, N=256, K=320, ld=None, tail=False, split3=False,
                       pool_rows=pool, defects=(), big=True))
    for pool in (0, 32, 64, 128):
        for M in (512, 256 + (pool or 33)):
            cs.append(dict(id=f"affine-pool{pool}-{M}", epi="affine", M=M, N=256, K=320, ld=None, tail=False, split3=False,
                           pool_rows=pool, defects=(("pool_group_shift", "coef_shift_col", "drop_last_kstep") if pool == 32 and M == 512 else
                                                    (("coef_shift_col",) if pool == 0 and M == 512 else ()))))
    for c in cs:
        ld_out = c["ld"] or c["N"]
        need = 2 * c["K"] if c["split3"] else c["K"]
        c["route"] = route_fused(c["epi"], c["M"], c["N"], c["K"], need, need, ld_out, True, n_cu, split3=c["split3"],
                                 pool_rows=c["pool_rows"], tail=c["tail"])
    return cs


def all_fused_routes(n_cu=256):
    names = set()
    g = persistent_grid(1 << 30, n_cu)
    for M in (512, 384, 256 * (g + 11) - 128):      # (whole tiles under the ticket draw: covered for the plain epilogues only)
        for split3 in (False, True):
            for tail in (False, True):
                names.add(route_fused("dgrad", M, 256, 320, 640, 640, 256, True, n_cu, split3=split3, tail=tail))
        for pool in (0, 32, 64, 128):
            names.add(route_fused("affine", M, 256, 320, 320, 320, 256, True, n_cu, pool_rows=pool))
    return names


# refusal reason -> a call that must be refused (built by the GPU file from these keywords; the CPU file checks that every
# reason ``route`` / ``route_fused`` can return is listed)
REFUSALS = {
    "bad_shape": dict(K=0),
    "bad_math": dict(math=7),
    "split_k": dict(split_k=0),
    "ld_too_small": dict(lda=63),
    "atomic_needs_f32_c": dict(split_k=2, cdt=BF16),
    "colstats_need_one_pass": dict(split_k=2, colstats=True),
    "bf16_small_needs_bf16_a": dict(adt=F32, bdt=F32, N=64),
    "bf16_small_needs_kc": dict(alay=RC, blay=RC, N=64, M=64),
    "bf16_small_needs_mult8": dict(K=60, N=64),
    "bf16_small_needs_alignment": dict(misaligned=("A",)),
    "f32_dtype_combination": dict(math=M_F32, adt=F32, bdt=BF16),
    "split3_shape": dict(split3=True, K=64),
    "split3_ragged_needs_one_pass": dict(split3=True, M=300, K=320, slabs=True, split_k=2),
    "ragged_out": dict(split3=True, M=300, K=320, ldc=260),
    "split3_ld": dict(split3=True, K=128, lda=248),
    "split3_alignment": dict(split3=True, K=128, misaligned=("B",)),
    "split3_not_served": None,        # every shape the checks admit is served at test size: stated as not reachable
    "pool_rows": dict(fused="affine", pool_rows=16),
    "fused_shape": dict(fused="dgrad", K=256),
    "fused_ld": dict(fused="dgrad", ld=260),
    "fused_alignment": dict(fused="affine", misaligned=("A",)),
}


# ------------------------------------------------------------------------------------------------ a case's inputs and reference
SPLIT_SCALES = (1.0, 256.0)           # ops.SPLIT_SCALE_ACT, ops.SPLIT_SCALE_WEIGHT
_BIG = {}                             # the operands and accumulators of the over-CU-count cases, computed once


def place(t, ld=None, off=0):
    """a 2-D tensor inside a NaN-filled allocation -> (buf, win)"""
    r, w = t.shape
    ld = w if ld is None else ld
    buf = torch.full((off + r * ld + 64,), float("nan"), dtype=t.dtype, device=t.device)
    win = buf[off:off + r * ld].view(r, ld)[:, :w]
    win.copy_(t)
    return buf, win


def kernel_of(route_name):
    return "tile128" if route_name.startswith(("f32/", "bf16_small")) else ("staged256" if route_name.startswith("bf16_staged") else "v2")


def _logical_pair(c, device, M, N):
    K = c["K"]
    sm = 0 if c.get("big") else c["M"]
    if c["split3"]:
        return (logical_split(M, K, seed_of(sm, c["N"], K, 0), device, SPLIT_SCALES[0]),
                logical_split(N, K, seed_of(sm, c["N"], K, 1), device, SPLIT_SCALES[1]))
    return (logical(M, K, seed_of(sm, c["N"], K, 0), device), logical(N, K, seed_of(sm, c["N"], K, 1), device, (3.0 / K) ** 0.5))


def build(c, device="cpu", max_rows=None, max_cols=None):
    """the stored inputs of a product case (reduced to the first max_rows x max_cols of the result on request: the
    generator makes them a prefix) -> dict(M, N, A, B [stored windows], bufs, bias, out0)"""
    M = min(c["M"], max_rows) if max_rows else c["M"]
    N = min(c["N"], max_cols) if max_cols else c["N"]
    off = lambda n: 1 if n in c["misaligned"] else 0
    key = (c["N"], c["K"], c["split3"], c["adt"], c["bdt"], str(device))
    if c.get("big") and key in _BIG and _BIG[key]["xa"].shape[0] >= M:
        xa, xb = _BIG[key]["xa"][:M], _BIG[key]["xb"]
    else:
        xa, xb = _logical_pair(c, device, M, N)
        if c.get("big") and not max_rows:
            _BIG.clear()
            _BIG[key] = {"xa": xa, "xb": xb}
    lda, ldb, _ = case_lds(c)
    if max_rows or max_cols:
        lda = lda if c["alay"] == KC else None
        ldb = ldb if c["blay"] == KC else None
    if c["split3"]:
        ia = split_image(xa.t() if c["alay"] == RC else xa, SPLIT_SCALES[0])
        ib = split_image(xb.t() if c["blay"] == RC else xb, SPLIT_SCALES[1])
        bufa, A = place(ia, c["lda"], off("A"))
        bufb, B = place(ib, c["ldb"], off("B"))
    else:
        bufa, A = operand(xa, c["adt"], c["alay"], lda if c["lda"] else None, off("A"))
        bufb, B = operand(xb, c["bdt"], c["blay"], ldb if c["ldb"] else None, off("B"))
    sm = 0 if c.get("big") else c["M"]
    bias = vec4(N, seed_of(sm, c["N"], c["K"], 2), device) if c["bias"] else None
    out0 = uniform(M * N, seed_of(sm, c["N"], c["K"], 3), device, -1.0, 1.0).float().view(M, N) if c["accumulate"] else None
    return {"M": M, "N": N, "A": A, "B": B, "bufs": (bufa, bufb), "bias": bias, "out0": out0, "key": key}


def reference(c, bt, defect=None):
    """product_ref / split_product_ref of a built case, with its statistics: dict(want, gate [of the stored output], acc,
    slabs, stats, stats_gate, ...)"""
    kern = kernel_of(c["route"])
    big = _BIG.get(bt["key"]) if (c.get("big") and defect is None) else None
    if c["split3"]:
        ha, la = split_halves(bt["A"], SPLIT_SCALES[0], c["alay"])
        hb, lb = split_halves(bt["B"], SPLIT_SCALES[1], c["blay"])
        pre = None
        if big is not None:
            if "r" not in big:
                big["r"] = acc_ref(ha + la, hb + lb, True, n=3 * c["K"], split_extra=True)
                big["r"]["lolo"] = (la @ lb.t()).abs()
            pre = {k: v[:bt["M"]] for k, v in big["r"].items()}
        p = split_product_ref(ha, la, hb, lb, SPLIT_SCALES[1], split_k=c["split_k"] if c["slabs"] else 1, defect=defect, pre=pre)
    else:
        A = ld_as_width(bt["A"]) if defect == "ld_as_width" else bt["A"]
        a, b = widen(A, c["alay"], c["math"]), widen(bt["B"], c["blay"], c["math"])
        exact = c["math"] == M_BF16 or (c["adt"] == BF16 and c["bdt"] == BF16)
        pre = None
        if big is not None:
            if "r" not in big:
                big["r"] = acc_ref(a, b, exact)
            pre = {k: v[:bt["M"]] for k, v in big["r"].items()}
        p = product_ref(a, b, exact=exact, math=c["math"], bias=bt["bias"], split_k=c["split_k"], out0=bt["out0"], slabs=c["slabs"],
                        defect=defect, tile=SLICES[kern][0], pre=pre)
    if c["colstats"]:
        p["stats"], p["stats_gate"] = colstats_ref(p, kern, c["nrep"], defect=defect)
    p["gate32"] = p["gate"]
    p["gate"] = out_gate(p["gate"], p["want"], c["cdt"])
    return p


def fused_inputs(c, device="cpu", max_rows=None):
    """the stored inputs of a fused-epilogue case -> dict; y has both signs of z in every column"""
    M = min(c["M"], max_rows) if max_rows else c["M"]
    N, K = c["N"], c["K"]
    cc = _c(c["id"], c["route"], c["M"], N, K, split3=c["split3"], big=c.get("big", False))
    bt = build(cc, device, max_rows=max_rows)
    ydt = F32 if c["split3"] else BF16
    sm = 0 if c.get("big") else c["M"]
    ld = c["ld"] or N
    bt["ybuf"], bt["y"] = place(logical(M, N, seed_of(sm, N, K, 4), device).to(ydt), ld)
    bt["scale"] = uniform(N, seed_of(sm, N, K, 5), device, 0.7, 1.3).float()
    bt["shift"] = uniform(N, seed_of(sm, N, K, 6), device, -0.5, 0.5).float()
    bt["mean"] = uniform(N, seed_of(sm, N, K, 7), device, -0.3, 0.3).float()
    bt["rstd"] = uniform(N, seed_of(sm, N, K, 8), device, 0.8, 1.25).float()
    bt["case"] = cc
    return bt


def fused_reference(c, bt, defect=None):
    cc = dict(bt["case"], route="v2/x")
    p = reference(cc, bt, defect=defect if defect in ("drop_last_kstep",) else None)
    p["gate"] = p["gate32"]
    if c["epi"] == "dgrad":
        return dgrad_bn_ref(p, bt["y"], bt["scale"], bt["shift"], bt["mean"], bt["rstd"], 16, F32 if c["split3"] else BF16, defect)
    want, gate, gate32 = affine_elu_ref(p, bt["scale"], bt["shift"], c["pool_rows"], defect)
    return {"want": want, "gate": gate, "gate32": gate32}


def refusal_case(reason):
    """the case (product: a ``_c`` dict; fused: a fused-case dict with key "epi") of one refusal reason"""
    kw = dict(REFUSALS[reason])
    fused = kw.pop("fused", None)
    if fused:
        c = dict(id=reason, epi=fused, M=256, N=256, K=320, ld=None, tail=False, split3=False, pool_rows=0, misaligned=(), route=None)
        c.update(kw)
        return c
    c = _c(reason, None, 256, 256, 128 if kw.get("split3") else 320)
    c.update(kw)
    return c


def refusal_route(c, n_cu=256):
    if "epi" in c:
        aligned = {"A", "B", "C"} - set(c["misaligned"])
        return route_fused(c["epi"], c["M"], c["N"], c["K"], c["K"], c["K"], c["ld"] or c["N"], True, n_cu, aligned,
                           pool_rows=c["pool_rows"])
    return case_route(c, n_cu)


# (message prefix, fragment of pcaa_last_error()) of the refusal each REFUSALS case must end in
REFUSAL_MESSAGES = {
    "bad_shape": ("pcaa_gemm:", "bad shape"), "bad_math": ("pcaa_gemm:", "bad math"), "split_k": ("pcaa_gemm:", "split_k must be"),
    "ld_too_small": ("pcaa_gemm:", "leading dimension too small"),
    "atomic_needs_f32_c": ("pcaa_gemm:", "atomic accumulation needs fp32 C"),
    "colstats_need_one_pass": ("pcaa_gemm:", "column statistics need a single K pass"),
    "bf16_small_needs_bf16_a": ("pcaa_gemm:", "needs a bf16 A operand"), "bf16_small_needs_kc": ("pcaa_gemm:", "needs KC operands"),
    "bf16_small_needs_mult8": ("pcaa_gemm:", "bf16 math needs K, lda, ldb"),
    "bf16_small_needs_alignment": ("pcaa_gemm:", "needs 16-B aligned operands"),
    "f32_dtype_combination": ("pcaa_gemm:", "unsupported dtype combination"),
    "split3_shape": ("pcaa_gemm_split3:", "N must be a multiple of 256"),
    "split3_ragged_needs_one_pass": ("pcaa_gemm_split3:", "needs a single K pass"),
    "ragged_out": ("pcaa_gemm_split3:", "partial last row tile needs ldc"),
    "split3_ld": ("pcaa_gemm_split3:", "leading dimensions must cover"), "split3_alignment": ("pcaa_gemm_split3:", "16-B aligned operands"),
    "pool_rows": ("pcaa_gemm_affine_elu:", "pool_rows must be"), "fused_shape": ("pcaa_gemm_dgrad_bn:", "N must be a multiple of 256"),
    "fused_ld": ("pcaa_gemm_dgrad_bn:", "bad leading dimension"), "fused_alignment": ("pcaa_gemm_affine_elu:", "16-B alignment"),
}

# Further refusals, one per PCAA_CHECK_ARG of the entry points that the route table does not name (it restates shapes,
# not null pointers or one entry point's copy of another's check): (entry point, message prefix, fragment, overrides of a
# valid call at M = N = 256, K = 320).  Pointer overrides: "NULL", "+4" (the pointer 4 bytes on: not 16-B aligned).
ABI_REFUSALS = [
    ("gemm", "pcaa_gemm:", "null operand", dict(A="NULL")),
    ("gemm", "pcaa_gemm:", "null operand", dict(C="NULL")),
    ("gemm", "pcaa_gemm:", "bad dtype", dict(a_dtype=2)),
    ("gemm", "pcaa_gemm:", "bad dtype", dict(c_dtype=3)),
    ("gemm", "pcaa_gemm:", "bad layout", dict(b_layout=2)),
    ("gemm", "pcaa_gemm:", "nrep must be", dict(colstats="stats", nrep=0)),
    ("slabs", "pcaa_gemm_slabs:", "slab stride must cover", dict(slab_stride=256 * 256 - 1)),
    ("slabs", "pcaa_gemm_slabs:", "slab stride must cover", dict(slabs="NULL")),
    ("slabs_split3", "pcaa_gemm_slabs_split3:", "slab stride must cover", dict(slab_stride=256 * 256 - 1)),
    ("group", "pcaa_gemm_group_rc_f32:", "bad args", dict(n=0)),
    ("group", "pcaa_gemm_group_rc_f32:", "bad args", dict(n=9)),
    ("group", "pcaa_gemm_group_rc_f32:", "bad shape", dict(K0=0)),
    ("group", "pcaa_gemm_group_rc_f32:", "multiples of 4", dict(M0=130)),
    ("group", "pcaa_gemm_group_rc_f32:", "multiples of 4", dict(A0="+4")),
    ("split3", "pcaa_gemm_split3:", "null operand", dict(B="NULL")),
    ("split3", "pcaa_gemm_split3:", "bad layout", dict(layout=2)),
    ("split3", "pcaa_gemm_split3:", "N must be a multiple of 256", dict(layout=RC, M=300, lda=600, ldb=512)),
    ("split3", "pcaa_gemm_split3:", "N must be a multiple of 256", dict(N=260)),
    ("split3", "pcaa_gemm_split3:", "partial last row tile needs ldc", dict(M=300, C="+4")),
    ("dgrad", "pcaa_gemm_dgrad_bn:", "null pointer", dict(dy="NULL")),
    ("dgrad", "pcaa_gemm_dgrad_bn:", "null pointer", dict(stats="NULL")),
    ("dgrad", "pcaa_gemm_dgrad_bn:", "y is required", dict(y="NULL")),
    ("dgrad", "pcaa_gemm_dgrad_bn:", "y is required", dict(x="vec")),
    ("dgrad", "pcaa_gemm_dgrad_bn:", "bad leading dimension", dict(nrep=0)),
    ("dgrad", "pcaa_gemm_dgrad_bn:", "partial last row tile needs ld", dict(M=300, dz="+4")),
    ("dgrad", "pcaa_gemm_dgrad_bn:", "16-B alignment", dict(dy="+4")),
    ("dgrad", "pcaa_gemm_dgrad_bn:", "16-B alignment", dict(scale="+4")),
    ("dgrad_split3", "pcaa_gemm_dgrad_bn_split3:", "null pointer", dict(y="NULL")),
    ("dgrad_split3", "pcaa_gemm_dgrad_bn_split3:", "N must be a multiple of 256", dict(K=64, lddy=128, ldw=128)),
    ("dgrad_split3", "pcaa_gemm_dgrad_bn_split3:", "N must be a multiple of 256", dict(M=300, K=128, lddy=256, ldw=256)),
    ("dgrad_split3", "pcaa_gemm_dgrad_bn_split3:", "bad leading dimension", dict(lddy=632)),
    ("dgrad_split3", "pcaa_gemm_dgrad_bn_split3:", "bad leading dimension", dict(ld=258)),
    ("dgrad_split3", "pcaa_gemm_dgrad_bn_split3:", "partial last row tile needs ld", dict(M=300, ld=260)),
    ("dgrad_split3", "pcaa_gemm_dgrad_bn_split3:", "partial last row tile needs ld", dict(M=300, dz="+4")),
    ("dgrad_split3", "pcaa_gemm_dgrad_bn_split3:", "16-B alignment", dict(Wt="+4")),
    ("affine", "pcaa_gemm_affine_elu:", "null pointer", dict(shift="NULL")),
    ("affine", "pcaa_gemm_affine_elu:", "N must be a multiple of 256", dict(K=256)),
    ("affine", "pcaa_gemm_affine_elu:", "N must be a multiple of 256", dict(N=260)),
    ("affine", "pcaa_gemm_affine_elu:", "bad leading dimension", dict(lda=312)),
    ("affine", "pcaa_gemm_affine_elu:", "bad leading dimension", dict(ldo=260)),
    ("affine", "pcaa_gemm_affine_elu:", "partial last row tile needs ldo", dict(M=288, pool_rows=32, ldo=260)),
    ("affine", "pcaa_gemm_affine_elu:", "16-B alignment", dict(out="+4")),
]

# exits that no call of test size reaches (the message fragments of csrc/gemm.hip): the 4 GiB bounds live inside
# pcaa_gemm_4wave_kernel (asked through ragged_out_ok and the predicates) and have no message of their own
OUT_OF_REACH = [("pcaa_gemm:", "too many tiles"), ("pcaa_gemm_group_rc_f32:", "too many blocks"), ("pcaa_gemm_split3:", "K too large"),
                # pcaa_gemm_split3 takes no split count and pcaa_gemm_slabs_split3 no statistics: the impl's check is unreachable
                ("pcaa_gemm_split3:", "column statistics need a single K pass")]
