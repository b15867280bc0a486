"""fp64 restatements of the batch-skinny decoder kernels of csrc/gemm_skinny.hip, the gate of each output, the
launchers' decisions as a plain-Python route table, the shared case lists, and planted defects.

Used by tests/test_skinny_branches.py (the kernels, on the GPU, through the C ABI) and tests/test_skinny_gates_cpu.py
(the gates, the coverage of routes / defects / argument checks and the input conditions, on the CPU).  Plain torch,
device-agnostic.  ``U``, ``BF16_ROUND``, ``uniform``, ``adam_ref``, ``ADAM_C_UPD``, ``moved``, ``ratio`` come from
tests/elementwise_ref.py; ``acc_ref``, ``acc_gate``, ``C_STAT``, ``ELU_C``, ``place`` from tests/gemm_ref.py.

Same stored values on both sides
--------------------------------
Operands are ``uniform`` draws over symmetric ranges (zero mean: the condition of ``acc_gate``'s statistical term; the
CPU file checks |mean| / rms <= 0.05), stored as fp32 inside larger allocations (``Framed``: a leading dimension above
the width, eight elements in front of the base, rows behind the last).  Inputs are framed in NaN wherever the kernel's
contract allows, outputs and the Adam state in a finite sentinel that is distinct per array and must come back
bit-identical (``Framed.intact``).  The reference widens the stored window: the bf16 routes round it first with
torch's round-to-nearest-even cast (the kernels' ``pk2``), the bf16-image routes read the stored image, the ``exact``
routes widen unrounded.  A fused update's second step starts from the fp32 state the kernel itself left.  (``Framed`` is
``gemm_ref.place`` with what this file's memory checks need on top: a fill of the caller's choice, the element in front
of the base, whole rows behind the last, and the comparison of everything outside the window.)

Gates, u = 2^-24, element-wise, no output element left out
----------------------------------------------------------
* the contraction: ``gemm_ref.acc_gate`` with n = the terms one accumulator adds (a split's chunks x 64; the weight
  gradient: 64 per chunk of rows, zeros behind M included).  bf16 x bf16 products are exact in fp32 (c_n = n - 1);
  the exact routes round every product (c_n = 2 n).
* slab sums (forward with nsplit > 1; every dgrad): n_s u sum |slab| + the slabs' own gates.  The dgrad with one slab
  adds nothing to it (n_s = 1: the reduction's sum is the slab itself).
* bias:  u (|acc| + |bias|).  ELU: ELU_C u (T + [z<=0]) + [z<=0] u |z| with T = |acc| + |bias| (``bn_act_fwd``'s form;
  ELU has slope <= 1, so the gate before it passes through).
* ELU'(a) = a > 0 ? 1 : a + 1 from the ELU OUTPUT: gate |f| + 2 u |v f| (the rounding of a + 1, the product).
* accumulate:  u (|v| + |out0|).      * bf16 output:  + BF16_ROUND |want|.
* Adam from a gradient g = s acc (s = grad_scale as fp32) that carries dg = s gate(acc) + u |s acc|: the three gates of
  ``elementwise_ref.adam_ref`` (which already count the rounding of s g) plus, to first order in dg,
    m' = b1 m + (1 - b1) g                      ->  (1 - b1) dg
    v' = b2 v + (1 - b2) g^2                    ->  2 (1 - b2) |g| dg     (+ (1 - b2) dg^2, the exact remainder)
    p' = p - ss m' / denom, denom = sqrt(v') ibc + eps, ibc = 1 / sqrt(bc2):
         d(m'/denom) = dm'/denom + |m'| d(denom)/denom^2,  d(denom) = ibc dv' / (2 sqrt v') = ibc (1 - b2) |g| dg / sqrt v'
                                                ->  ss ((1 - b1) / denom + |m'| (1 - b2) |g| ibc / (sqrt(v') denom^2)) dg
  ss and ibc are the fp32 values of StepCount.coef_dev (the kernels receive those); ``adam_ref`` recomputes them in fp64
  from lr, b1, b2 and the step, one fp32 rounding away, which ADAM_C_UPD counts.  The wanted values are formed with the
  stored coefficients; the gates come from ``adam_ref``.

Nothing above was widened from the issue's starting forms: the CPU file's half rule holds for all of them (it prints
the figure per route).

Planted defects: ``DEFECTS``; ``defect=`` of a reference returns what that subtly wrong kernel would have produced,
``DEFECT_CASE`` names the case each is looked for at, ``touched`` the elements it can move.

A shape the issue states that does not exist: the reduction's second grid-stride trip "at K = 64" -- one chunk admits
one split only, and one split has no reduction launch.  ``BIG_REDUCE`` is 64 x 65 600 x 128 with nsplit = 2: the
smallest forward whose reduction walks M N / 4 > 4096 x 256 quads.
"""
import torch

import elementwise_ref as E
from elementwise_ref import ADAM_C_UPD, BF16_ROUND, U, adam_ref, moved, ratio, uniform  # noqa: F401  (re-exported)
from gemm_ref import C_STAT, ELU_C, acc_gate, acc_ref, place  # noqa: F401  (re-exported)

F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")
SENTINEL = {"W": 3.0e12, "m": -5.0e13, "v": 7.0e14, "dW": -1.1e15, "y": 1.3e16, "dx": -1.7e17, "P": 1.9e18}
HP = dict(lr=1e-3, b1=0.9, b2=0.99, eps=1e-8, gs=0.5)
REDUCE_QUADS = 4096 * 256            # quads one trip of skinny_reduce_kernel's capped grid covers

DEFECTS = ("drop_last_chunk", "split_overlap", "split_gap", "row_past_M_read", "col_clamp_dup", "pair_swapped",
           "w16_halves_swapped", "bias_shift_col", "bias_after_elu", "elu_grad_from_pre", "accumulate_dropped",
           "reduce_second_trip_skipped", "jn_tail_dropped", "ring_stale", "state_ld_is_K", "row_live_off_by_one",
           "bf16_rows_swapped", "chunk_dropped", "dz_rows_unmasked", "kslot_mismatch", "grad_scale_twice",
           "grad_scale_missing", "moments_swapped", "truncating_bf16")


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the launchers, restated
def resident_blocks(kind):
    return {0: 768, 1: 512, 2: 512, 3: 768}.get(kind, 512)


def splits(kind, N, K):
    """pcaa_skinny_splits restated (kind 0 / 2: forward, 1 / 3: dgrad; 2 / 3 the exact forms)"""
    fwd = kind % 2 == 0
    groups = cdiv(N if fwd else K, 128 if fwd else 256)
    chunks = (K if fwd else N) // 64
    if chunks < 1:
        return 1
    ns = max(1, min(max(1, chunks // 2), resident_blocks(kind) // groups))
    return cdiv(chunks, cdiv(chunks, ns))


def split_ranges(chunks, nsplit, defect=None):
    """the element ranges of the contraction each split owns: cps = cdiv(chunks, nsplit) chunks of 64"""
    cps = cdiv(chunks, nsplit)
    rg = [(s * cps * 64, min(chunks, (s + 1) * cps) * 64) for s in range(nsplit)]
    if defect == "drop_last_chunk":
        rg[-1] = (rg[-1][0], rg[-1][1] - 64)
    if defect == "split_overlap":
        rg[0] = (0, rg[0][1] + 64)
    if defect == "split_gap":
        rg[1] = (rg[1][0] + 64, rg[1][1])
    return [r for r in rg if r[1] > r[0]]


def cols_per_wave(N, K, want=1024):
    """wgrad_cols_per_wave restated: JL, the widest 32 JL columns per wave that still leave ``want`` workgroups"""
    ntile = lambda jl: cdiv(K, 128 * jl) * cdiv(N, 128)
    return 4 if ntile(4) >= want else 2 if ntile(2) >= want else 1


def mc_of(M):
    return 1 if M <= 64 else 2 if M <= 128 else 4 if M <= 256 else 8


def wave_steps(K, JL):
    """[(kb, jn)] of every wave of a row panel that has column steps: jn = min(JL, (K - kb) / 32)"""
    return [(kb, min(JL, (K - kb) // 32)) for kb in range(0, K, 32 * JL)]


def route(entry, variant="bf16", N=128, K=64, *, nsplit=None, ldw=None, w_off=0, M=1, chunks=1):
    """the kernel an entry point launches, by the launcher's own conditions.  variant: bf16 / exact / w16 (forward,
    dgrad), f32 / exact / bf16 (plain weight gradient), bf16 / exact (fused update).  w_off: W's base offset in
    elements from a 16-B aligned address."""
    full = "full" if N % 128 == 0 else "ragged"
    if entry == "fwd":
        ns = splits(2 if variant == "exact" else 0, N, K) if nsplit is None else nsplit
        return f"fwd/{variant}/{'epilogue' if ns == 1 else 'slabs'}"
    if entry == "dgrad":
        ldw = K if ldw is None else ldw
        if variant == "w16":
            return "dgrad2_w16" if ldw % 2 == 0 and w_off % 2 == 0 else "refused"
        pairs = ldw % 2 == 0 and (4 * w_off) % 8 == 0
        if variant == "exact":
            return "dgrad2_exact" if pairs else "refused"
        return "dgrad2" if pairs else "dgrad1"
    if entry == "wgrad":
        return f"wgrad/{variant}/{full}"
    if entry == "adam":
        return f"adam/{variant}/JL{cols_per_wave(N, K)}/{full}"
    if entry == "rows":
        return f"rows/MC{mc_of(M)}/JL{cols_per_wave(N, K)}/{full}"
    if entry == "t16":
        deep = chunks >= 4
        return f"t16/NB{4 if deep else 2}/JL{cols_per_wave(N, K, 384 if deep else 1024)}/{full}"
    raise ValueError(entry)


def all_routes():
    r = ["dgrad1", "dgrad2", "dgrad2_exact", "dgrad2_w16"]
    r += [f"fwd/{v}/{e}" for v in ("bf16", "exact", "w16") for e in ("epilogue", "slabs")]
    r += [f"wgrad/{v}/{f}" for v in ("f32", "bf16", "exact") for f in ("full", "ragged")]
    tail = [f"JL{j}/{f}" for j in (1, 2, 4) for f in ("full", "ragged")]
    r += [f"adam/{v}/{t}" for v in ("bf16", "exact") for t in tail]
    r += [f"rows/MC{mc}/{t}" for mc in (1, 2, 4, 8) for t in tail]
    r += [f"t16/NB{nb}/{t}" for nb in (2, 4) for t in tail]
    return r


# ------------------------------------------------------------------------------------------------ stored operands
class Framed:
    """a 2-D tensor inside a filled 1-D allocation: ``front`` elements before the base (8: the base stays 16-B aligned
    for fp32, 9: 4 bytes off an 8-B boundary), leading dimension ld >= width, ``behind`` whole rows after the last"""

    def __init__(self, t, ld=None, fill=NAN, front=8, behind=1):
        r, w = t.shape
        self.r, self.w, self.ld, self.front = r, w, (w if ld is None else ld), front
        self.buf = torch.full((front + (r + behind) * self.ld + 8,), fill, dtype=t.dtype, device=t.device)
        self.win = self.buf[front:front + r * self.ld].view(r, self.ld)[:, :w]
        self.win.copy_(t)

    def rows(self, n):
        """the window over the first n rows of the allocation (n may exceed the logical rows: the rows behind)"""
        return self.buf[self.front:self.front + n * self.ld].view(n, self.ld)[:, :self.w]

    def ptr(self):
        return self.buf.data_ptr() + self.front * self.buf.element_size()

    def snapshot(self):
        return self.buf.clone()

    def intact(self, before, rows=None):
        """every element outside the logical window (rows: fewer than all) has its bits of ``before``"""
        keep = torch.ones(self.buf.shape, dtype=torch.bool, device=self.buf.device)
        r = self.r if rows is None else rows
        keep[self.front:self.front + r * self.ld].view(r, self.ld)[:, :self.w] = False
        it = torch.int32 if self.buf.element_size() == 4 else torch.int16
        return bool(torch.equal(self.buf.view(it)[keep], before.view(it)[keep]))


def seed_of(*a):
    s = 17
    for v in a:
        s = (s * 7919 + int(v) * 4099 + 31) % 1000003
    return 1 + s


def mat(rows, cols, seed, device="cpu", amp=3.0 ** 0.5):
    """[rows, cols] fp32, uniform in [-amp, amp): zero mean, unit variance at the default"""
    return uniform(rows * cols, seed, device, -amp, amp).view(rows, cols).float()


def rows_of(n_cols, rows, seed, device="cpu", amp=3.0 ** 0.5):
    """[rows, n_cols] fp32 generated column-major: fewer columns are a prefix (the CPU file evaluates a long N at its
    first columns)"""
    return mat(n_cols, rows, seed, device, amp).t()


def mean_over_rms(t):
    """|mean| / rms of an operand, or None below 4096 values: as in test_gemm_gates_cpu.py, so small an operand has no
    mean to speak of (sampling noise alone is 1 / sqrt(n)) and its gate is the worst-case term"""
    t = t.double().reshape(-1)
    return float(t.mean().abs() / t.pow(2).mean().sqrt()) if t.numel() >= 4096 else None


def widen(t, variant, defect=None):
    """the stored window as the kernel's MFMA sees it, float64"""
    if t.dtype == BF16 or variant == "exact":
        return t.double()
    if defect == "truncating_bf16":
        return (t.contiguous().view(torch.int32) & -65536).view(F32).double()
    return t.to(BF16).double()


def coef_ref(step, lr=HP["lr"], b1=HP["b1"], b2=HP["b2"]):
    """(step_size, 1 / sqrt(bc2)) as pcaa_adam_advance stores them: fp64 from the fp32 arguments, rounded to fp32"""
    lr, b1, b2 = E.f32(lr), E.f32(b1), E.f32(b2)
    return E.f32(lr / (1.0 - b1 ** step)), E.f32(1.0 / (1.0 - b2 ** step) ** 0.5)


# ------------------------------------------------------------------------------------------------ forward, dgrad
def _slab_sum(parts):
    v = sum(p["acc"] for p in parts)
    gate = sum(acc_gate(p) for p in parts)
    if len(parts) > 1:
        gate = gate + len(parts) * U * sum(p["acc"].abs() for p in parts)
    return v, gate


def fwd_ref(x, W, bias, act, nsplit, variant="bf16", defect=None, before=None):
    """x [M, K], W [N, K] stored windows -> dict(want, gate [M, N], slabs)"""
    a, b = widen(x, variant, defect), widen(W, variant, defect)
    pe = variant != "exact"                                   # products exact in fp32
    parts = [acc_ref(a[:, k0:k1], b[:, k0:k1], pe) for k0, k1 in split_ranges(a.shape[1] // 64, nsplit, defect)]
    v, gate = _slab_sum(parts)
    bb = torch.zeros(v.shape[1], dtype=torch.float64, device=v.device) if bias is None else bias.double()
    if defect == "bias_shift_col":
        bb = bb.roll(1)
    if defect == "bias_after_elu":
        z = v
    else:
        z = v + bb
        if bias is not None:
            gate = gate + U * (v.abs() + bb.abs())
    want = z
    if act:
        neg = (z <= 0).double()
        want = E.elu(z)
        gate = gate + ELU_C * U * (v.abs() + bb.abs() + neg) + neg * U * z.abs()
    if defect == "bias_after_elu":
        want = want + bb
    if defect == "reduce_second_trip_skipped":
        want = want.clone()
        want.view(-1)[4 * REDUCE_QUADS:] = before.double().reshape(-1)[4 * REDUCE_QUADS:]
    return {"want": want, "gate": gate + 1e-300, "slabs": [p["acc"] for p in parts]}


def elu_out(n_rows, n_cols, seed, device="cpu"):
    """an ELU output [rows, cols] fp32 with both branches in every column: a = ELU(z), z uniform in [-2, 2)"""
    return E.elu(uniform(n_rows * n_cols, seed, device, -2.0, 2.0)).view(n_rows, n_cols).float()


def dgrad_ref(dz, W, a_prev, out0, accumulate, nsplit, variant="bf16", defect=None):
    """dz [M, N], W [N, K] stored windows -> dict(want, gate [M, K], slabs)"""
    a, b = widen(dz, variant, defect), widen(W, variant, defect)
    if defect == "w16_halves_swapped":                        # the low halves feed the odd columns' fragment
        b = b.view(b.shape[0], -1, 2).flip(2).reshape(b.shape)
    pe = variant != "exact"
    bt = b.t().contiguous()                                   # [K, N]: acc_ref contracts the second index of both
    parts = [acc_ref(a[:, n0:n1], bt[:, n0:n1], pe) for n0, n1 in split_ranges(a.shape[1] // 64, nsplit, defect)]
    v, gate = _slab_sum(parts)
    if defect == "pair_swapped":
        v = v.view(v.shape[0], -1, 2).flip(2).reshape(v.shape)
    if defect == "col_clamp_dup":
        v = v.clone()
        v[:, -1] = v[:, -2]
    if a_prev is not None:
        ap = a_prev.double()
        f = torch.where(ap > 0, torch.ones_like(ap), torch.exp(ap) if defect == "elu_grad_from_pre" else ap + 1)
        v = v * f
        gate = gate * f.abs() + 2 * U * v.abs()
    if accumulate and defect != "accumulate_dropped":
        o = out0.double()
        gate = gate + U * (v.abs() + o.abs())
        v = v + o
    return {"want": v, "gate": gate + 1e-300, "slabs": [p["acc"] for p in parts]}


# ------------------------------------------------------------------------------------------------ weight gradient
def kslot_perm(device="cpu"):
    """batch row of k-slot (s, h, e) of the row-major kernels (16 s + 8 h + e) -> of the packed ones (32 h + 8 s + e)"""
    m = torch.arange(64, device=device)
    s, h, e = m // 16, (m // 8) % 2, m % 8
    return 32 * h + 8 * s + e


def wgrad_acc(dz, x, M, variant="bf16", defect=None):
    """dz [R, N], x [R, K] stored windows over all allocated rows (R >= M; the rows behind M enter only through a
    defect) -> acc_ref dict of dW [N, K] with n = 64 x chunks terms"""
    R = dz.shape[0]
    chunks = mc_of(M) if M > 64 else 1
    rows = M
    if defect == "row_past_M_read":
        rows = min(M + 1, R)
    if defect == "dz_rows_unmasked":
        rows = min(64 * chunks, R)
    if defect == "chunk_dropped":
        rows = min(M, 64 * (chunks - 1))
    a, b = widen(dz[:rows], variant, defect).t().contiguous(), widen(x[:rows], variant, defect).t().contiguous()
    if defect == "kslot_mismatch":
        pa = torch.zeros((a.shape[0], 64 * chunks), dtype=a.dtype, device=a.device)
        pa[:, :rows] = a
        pb = torch.zeros((b.shape[0], 64 * chunks), dtype=a.dtype, device=a.device)
        pb[:, :rows] = b
        idx = torch.cat([kslot_perm(a.device) + 64 * c for c in range(chunks)])
        a, b = pa, pb[:, idx]
    return acc_ref(a, b, variant != "exact", n=64 * chunks)


def packed_acc(P, chunk_stride, chunks, N, K, defect=None):
    """the packed buffer (bf16, 1-D) -> acc_ref dict of dW [N, K], n = 64 x chunks"""
    a, b = [], []
    for c in range(chunks - 1 if defect == "chunk_dropped" else chunks):
        img = P[c * chunk_stride:c * chunk_stride + (N + K) * 64].view(N + K, 64).double()
        a.append(img[:N])
        b.append(img[N:][:, kslot_perm(P.device)] if defect == "kslot_mismatch" else img[N:])
    return acc_ref(torch.cat(a, 1), torch.cat(b, 1), True, n=64 * chunks)


def pack_ref(dz, x, rows):
    """the packed chunk of pcaa_pack_rows_t16: [(N + K), 64] bf16, transposed, rounded to nearest even, zero behind rows"""
    N, K = dz.shape[1], x.shape[1]
    out = torch.zeros((N + K, 64), dtype=BF16, device=dz.device)
    out[:N, :rows] = dz[:rows].t().to(BF16)
    out[N:, :rows] = x[:rows].t().to(BF16)
    return out


def _keep_mask(N, K, JL, defect, device):
    """bool [N, K]: elements a store defect leaves at their previous contents"""
    keep = torch.zeros((N, K), dtype=torch.bool, device=device)
    if defect == "jn_tail_dropped":
        for kb, jn in wave_steps(K, JL):
            keep[:, kb + 32 * (jn - 1):kb + 32 * jn] = True
    if defect == "row_live_off_by_one":
        keep[N - 1] = True
    return keep


def wgrad_ref(dz, x, M, out_dtype=F32, variant="bf16", defect=None, before=None):
    """the plain weight gradient (always 4 column steps per wave) -> dict(want, gate [N, K], touched)"""
    r = wgrad_acc(dz, x, M, variant, defect)
    want, gate = r["acc"], acc_gate(r)
    N, K = want.shape
    touched = None
    if defect == "bf16_rows_swapped":
        n2 = N // 2 * 2
        want = torch.cat([want[:n2].view(n2 // 2, 2, K).flip(1).reshape(n2, K), want[n2:]])
    if defect in ("jn_tail_dropped", "row_live_off_by_one"):
        touched = _keep_mask(N, K, 4, defect, want.device)
        want = torch.where(touched, before.double(), want)
    if out_dtype == BF16:
        gate = gate + BF16_ROUND * want.abs()
    return {"want": want, "gate": gate + 1e-300, "touched": touched}


def _stale(t, N, NB):
    """every element's value of the fragment NB - 1 further on in its wave's ring: fragment f = 4 j + i is rows [32 i, +32)
    of a 128-row panel at column step j; past the panel's live rows or the matrix's columns: its own"""
    n = torch.arange(t.shape[0], device=t.device).view(-1, 1)
    k = torch.arange(t.shape[1], device=t.device).view(1, -1)
    f = (n % 128) // 32 + NB - 1
    n2 = n - (n % 128) // 32 * 32 + (f % 4) * 32
    k2 = k + 32 * (f // 4)
    ok = (n2 < N) & (k2 < t.shape[1])
    return torch.where(ok, t[n2.clamp_max(t.shape[0] - 1).expand_as(ok), k2.clamp_max(t.shape[1] - 1).expand_as(ok)], t)


def wgrad_adam_ref(r, p, m, v, step, coef, JL=1, NB=2, hp=HP, defect=None, frames=None):
    """One fused update.  r: the gradient's acc_ref dict; p, m, v: the stored fp32 state [N, K] before the step; coef:
    (step_size, 1 / sqrt(bc2)) as stored in StepCount.coef_dev; frames: the state's (W, m, v) ``Framed`` (state_ld_is_K
    reads exp_avg through them).  -> dict p / m / v -> (want, gate), touched"""
    acc, gacc = r["acc"], acc_gate(r)
    N, K = acc.shape
    gs, b1, b2, eps = E.f32(hp["gs"]), E.f32(hp["b1"]), E.f32(hp["b2"]), E.f32(hp["eps"])
    ss, ibc = float(coef[0]), float(coef[1])
    p0, m0, v0 = p.double(), m.double(), v.double()
    gscale = gs * gs if defect == "grad_scale_twice" else 1.0 if defect == "grad_scale_missing" else gs
    if defect == "moments_swapped":                           # (|exp_avg| in exp_avg_sq's place: the square root stays real)
        m0, v0 = v.double(), m.double().abs()
    if defect == "ring_stale":
        m0, v0 = _stale(m0, N, NB), _stale(v0, N, NB)
    if defect == "state_ld_is_K":                             # exp_avg fetched at n K + k of its allocation
        fm = frames[1]
        m0 = fm.buf[fm.front:fm.front + N * K].view(N, K).double()
    g = acc * gscale
    dg = gs * gacc + U * g.abs()
    e = adam_ref(p0.float(), acc.float(), m0.float(), v0.float(), hp["lr"], b1, b2, eps, step, gs)   # the gates
    m1 = b1 * m0 + (1 - b1) * g
    v1 = b2 * v0 + (1 - b2) * g * g
    rt = torch.sqrt(v1)
    denom = rt * ibc + eps
    p1 = p0 - ss * m1 / denom
    carry_p = ss * ((1 - b1) / denom + m1.abs() * (1 - b2) * g.abs() * ibc / (rt.clamp_min(1e-300) * denom * denom)) * dg
    out = {"p": (p1, e["p"][1] + carry_p), "m": (m1, e["m"][1] + (1 - b1) * dg),
           "v": (v1, e["v"][1] + 2 * (1 - b2) * g.abs() * dg + (1 - b2) * dg * dg)}
    touched = None
    if defect in ("jn_tail_dropped", "row_live_off_by_one"):
        touched = _keep_mask(N, K, JL, defect, acc.device)
        out = {k: (torch.where(touched, old.double(), w), gt) for (k, (w, gt)), old in zip(out.items(), (p, m, v))}
    out["touched"] = touched
    return out


# ------------------------------------------------------------------------------------------------ the shared case lists
MS = (1, 7, 8, 9, 31, 32, 33, 63, 64)
FWD_NK = ((128, 64), (192, 128), (128, 192), (192, 256), (320, 448))
FWD_VARIANTS = ("bf16", "exact", "w16")
BIG_REDUCE = (64, 65600, 128, 2)                              # M, N, K, nsplit: see the module docstring
FWD_CALLER_SPLITS = (2, 4, 7)                                 # of 7 chunks: 4 + 3, 2 + 2 + 2 + 1, one chunk each
DGRAD_N, DGRAD_K = (128, 192, 448), (64, 128, 192, 320)
DGRAD_FORMS = ("dgrad2", "dgrad1_ld", "dgrad1_off", "dgrad2_exact", "dgrad2_w16")
WG_M, WG_N, WG_K = (1, 9, 33, 64), (1, 2, 127, 128, 129, 130, 131, 257), (32, 96, 128, 160)
WG_VARIANTS = ("f32", "exact", "bf16")
ADAM_VARIANTS = ("bf16", "exact")
WIDE_JL = {(131072, 160): 4, (130950, 160): 4, (65536, 288): 2, (65412, 288): 2}      # want = 1024 tiles
ROWS_M = (1, 64, 65, 127, 128, 129, 256, 257, 511, 512)
ROWS_NK = ((130, 96), (256, 160))
ROWS_WIDE_M = (40, 100, 200, 300)                             # MC = 1, 2, 4, 8 at the JL > 1 shapes (the issue asks for MC = 2)
T16_CHUNKS = (1, 2, 3, 4, 5, 8)
T16_DEEP_JL = {(49030, 160): 4, (49152, 160): 4, (24580, 288): 2, (24576, 288): 2}     # chunks >= 4: want = 384 tiles
PACK_ROWS = (1, 8, 9, 63, 64)


def dgrad_form(form, K):
    """-> (variant, ldw, front) of a dgrad form: the leading dimension and base offset that select its kernel"""
    return {"dgrad2": ("bf16", K + 8, 8), "dgrad1_ld": ("bf16", K + 7, 8), "dgrad1_off": ("bf16", K + 8, 9),
            "dgrad2_exact": ("exact", K + 8, 8), "dgrad2_w16": ("w16", K + 8, 8)}[form]


def cases():
    """every case of the two files as a dict: entry, variant, M, N, K and what selects the route"""
    out = []
    for v in FWD_VARIANTS:
        for N, K in FWD_NK:
            for M in MS:
                for bias in (True, False):
                    for act in (1, 0):
                        out.append(dict(entry="fwd", variant=v, M=M, N=N, K=K, bias=bias, act=act, nsplit=None))
    M, N, K, ns = BIG_REDUCE
    out.append(dict(entry="fwd", variant="bf16", M=M, N=N, K=K, bias=True, act=1, nsplit=ns))
    for ns in FWD_CALLER_SPLITS:                                # the C ABI takes nsplit from the caller
        out.append(dict(entry="fwd", variant="bf16", M=33, N=320, K=448, bias=True, act=1, nsplit=ns))
    for form in DGRAD_FORMS:
        for K in DGRAD_K:
            for N in DGRAD_N:
                for M in MS:
                    for ap in (True, False):
                        for accu in (True, False):
                            out.append(dict(entry="dgrad", form=form, variant=dgrad_form(form, K)[0], M=M, N=N, K=K,
                                            a_prev=ap, accumulate=accu))
    for v in WG_VARIANTS:
        for K in WG_K:
            for N in WG_N:
                for M in WG_M:
                    out.append(dict(entry="wgrad", variant=v, M=M, N=N, K=K))
    for v in ADAM_VARIANTS:
        for K in WG_K:
            for N in WG_N:
                for M in WG_M:
                    out.append(dict(entry="adam", variant=v, M=M, N=N, K=K, zero=False))
        out.append(dict(entry="adam", variant=v, M=33, N=130, K=96, zero=True))
        for (N, K) in WIDE_JL:
            out.append(dict(entry="adam", variant=v, M=33, N=N, K=K, zero=False))
    for N, K in ROWS_NK:
        for M in ROWS_M:
            out.append(dict(entry="rows", variant="bf16", M=M, N=N, K=K, zero=False))
    out.append(dict(entry="rows", variant="bf16", M=100, N=130, K=96, zero=True))
    for (N, K) in WIDE_JL:
        for M in ROWS_WIDE_M:
            out.append(dict(entry="rows", variant="bf16", M=M, N=N, K=K, zero=False))
    for N, K in ROWS_NK:
        for c in T16_CHUNKS:
            out.append(dict(entry="t16", variant="bf16", chunks=c, M=37, N=N, K=K, zero=False))
    out.append(dict(entry="t16", variant="bf16", chunks=3, M=37, N=130, K=96, zero=True))
    for (N, K) in T16_DEEP_JL:
        out.append(dict(entry="t16", variant="bf16", chunks=4, M=64, N=N, K=K, zero=False))
    for (N, K) in WIDE_JL:
        out.append(dict(entry="t16", variant="bf16", chunks=2, M=64, N=N, K=K, zero=False))
    return out


def case_route(c):
    if c["entry"] == "dgrad":
        _, ldw, front = dgrad_form(c["form"], c["K"])
        return route("dgrad", c["variant"], c["N"], c["K"], ldw=ldw, w_off=front - 8)
    return route(c["entry"], c["variant"], c["N"], c["K"], nsplit=c.get("nsplit"), M=c["M"], chunks=c.get("chunks", 1))


def case_id(c):
    extra = "".join(f"-{k}{int(c[k])}" for k in ("bias", "act", "nsplit", "a_prev", "accumulate", "chunks", "zero")
                    if c.get(k) is not None)
    return f"{c['entry']}-{c.get('form', c['variant'])}-{c['M']}x{c['N']}x{c['K']}{extra}"


# the case each planted defect is looked for at (a key of case_id); a defect that keeps previous contents is looked for at
# the elements it keeps (``touched``)
DEFECT_CASE = {
    "drop_last_chunk": "fwd-bf16-33x320x448-bias1-act0", "split_overlap": "fwd-bf16-33x320x448-bias1-act0",
    "split_gap": "fwd-exact-33x320x448-bias1-act0", "bias_shift_col": "fwd-bf16-9x192x128-bias1-act1",
    "bias_after_elu": "fwd-bf16-9x192x128-bias1-act1", "reduce_second_trip_skipped": "fwd-bf16-64x65600x128-bias1-act1-nsplit2",
    "truncating_bf16": "fwd-bf16-64x128x192-bias0-act0",
    "col_clamp_dup": "dgrad-dgrad2-33x192x320-a_prev0-accumulate0", "pair_swapped": "dgrad-dgrad2-33x192x320-a_prev0-accumulate0",
    "w16_halves_swapped": "dgrad-dgrad2_w16-33x192x320-a_prev0-accumulate0",
    "elu_grad_from_pre": "dgrad-dgrad2-31x192x320-a_prev1-accumulate0",
    "accumulate_dropped": "dgrad-dgrad1_ld-63x192x320-a_prev0-accumulate1",
    "row_past_M_read": "wgrad-f32-33x129x160", "bf16_rows_swapped": "wgrad-bf16-33x129x160",
    "row_live_off_by_one": "wgrad-f32-33x129x160", "jn_tail_dropped": "adam-bf16-33x130x96-zero0",
    "ring_stale": "adam-bf16-33x257x160-zero0", "state_ld_is_K": "adam-bf16-33x257x160-zero0",
    "grad_scale_twice": "adam-exact-33x130x96-zero0", "grad_scale_missing": "adam-bf16-33x130x96-zero0",
    "moments_swapped": "adam-bf16-33x130x96-zero0", "chunk_dropped": "rows-bf16-127x130x96-zero0",
    "dz_rows_unmasked": "rows-bf16-65x130x96-zero0", "kslot_mismatch": "t16-bf16-37x130x96-chunks3-zero0",
}


# ------------------------------------------------------------------------------------------------ a case's stored inputs
def build(c, device="cpu", n_max=None, tail="contract", step=1):
    """the stored inputs of a case -> dict of ``Framed`` (and the plain values).  n_max: the first n_max of N only (the
    CPU file; the generators make them a prefix).  tail = "finite": the rows behind M hold ordinary data instead of
    NaN / 1e30 (what a defect that reads them would have met)."""
    e, M, K = c["entry"], c["M"], c["K"]
    N = min(c["N"], n_max) if n_max else c["N"]
    sd = lambda w: seed_of(c["N"], K, M, w, step)
    d = {"N": N}
    if e == "fwd":
        d["x"] = Framed(mat(M, K, sd(0), device), K + 4)
        W = mat(N, K, sd(1), device, (3.0 / K) ** 0.5)
        d["W"] = Framed(W.to(BF16) if c["variant"] == "w16" else W, K + 8, behind=2)
        d["bias"] = uniform(N, sd(2), device, -1.0, 1.0).float() if c["bias"] else None
        d["y"] = Framed(torch.full((M, N), SENTINEL["y"], dtype=F32, device=device), fill=SENTINEL["y"])
    elif e == "dgrad":
        variant, ldw, front = dgrad_form(c["form"], K)
        d["dz"] = Framed(mat(M, N, sd(0), device), N + 4)
        W = mat(N, K, sd(1), device, (3.0 / N) ** 0.5)
        d["W"] = Framed(W.to(BF16) if variant == "w16" else W, ldw, front=front, behind=2)
        d["a_prev"] = elu_out(M, K, sd(2), device) if c["a_prev"] else None
        d["out0"] = mat(M, K, sd(3), device, 1.0)
        d["dx"] = Framed(d["out0"] if c["accumulate"] else torch.full((M, K), SENTINEL["dx"], dtype=F32, device=device),
                         fill=SENTINEL["dx"])
    elif e == "pack":
        d["dz"] = Framed(mat(M, N, sd(0), device, 0.5), N + 3)
        d["x"] = Framed(mat(M, K, sd(1), device), K + 5)
    else:
        chunks = c.get("chunks", 1) if e == "t16" else (mc_of(M) if e == "rows" else 1)
        R = 64 * chunks if e in ("rows", "t16") else M
        R = R + c.get("rows_extra", 0)
        dz_all = rows_of(N, R, sd(0), device, 0.5)            # [R, N], a prefix in N
        x_all = mat(R, K, sd(1), device)
        if e == "t16":                                        # chunk ch holds rows [64 ch, 64 ch + M)
            d["chunks"] = [(dz_all[64 * ch:64 * ch + M].contiguous(), x_all[64 * ch:64 * ch + M].contiguous()) for ch in range(chunks)]
        else:
            fz, fx = dz_all.clone(), x_all.clone()
            if tail != "finite" and R > M:
                fz[M:] = NAN
                fx[M:] = 1e30 if e == "rows" else NAN
                if e == "rows":
                    fx[64 * chunks:] = NAN
            d["dz"] = Framed(fz, N + 3)
            d["x"] = Framed(fx, K + 5)
    return d


def state(c, device="cpu", n_max=None, ldw=None):
    """the fused update's (W, exp_avg, exp_avg_sq) as sentinel-framed fp32 [N, K]: nonzero moments with exp_avg_sq >= 1e-4
    (``elementwise_ref.adam_state``), or zero moments for the first-step cases"""
    N, K = (min(c["N"], n_max) if n_max else c["N"]), c["K"]
    p, _, m, v = E.adam_state(N * K, seed_of(c["N"], K, 5), device)
    if c.get("zero"):
        m, v = torch.zeros_like(m), torch.zeros_like(v)
    return tuple(Framed(t.view(N, K), ldw, fill=SENTINEL[k]) for t, k in ((p, "W"), (m, "m"), (v, "v")))


# ------------------------------------------------------------------------------------------------ refusals (C ABI)
# (entry point key, fragment of pcaa_last_error(), overrides of a valid call).  Pointer overrides: "NULL", "+4" (4 bytes
# on).  The entry point keys and their valid calls: tests/test_skinny_branches.py::VALID.  The format strings of the
# weight-gradient family start with "%s:"; their prefix is matched as such.
BIG = 1 << 30
REFUSALS = [
    ("fwd", "pcaa_skinny_linear_fwd:", "null pointer", dict(ws="NULL")),
    ("fwd", "pcaa_skinny_linear_fwd:", "unsupported shape", dict(M=65)),
    ("fwd", "pcaa_skinny_linear_fwd:", "unsupported shape", dict(N=96)),
    ("fwd_exact", "pcaa_skinny_linear_fwd:", "unsupported shape", dict(K=96)),
    ("fwd", "pcaa_skinny_linear_fwd:", "bad leading dimensions", dict(ldx=126)),
    ("fwd", "pcaa_skinny_linear_fwd:", "bad leading dimensions", dict(ldw=130)),
    ("fwd_w16", "pcaa_skinny_linear_fwd:", "bad leading dimensions", dict(ldw=1 << 24)),      # ldw N = 2^31
    ("fwd", "pcaa_skinny_linear_fwd:", "buffers must be 16-B aligned", dict(y="+4")),
    ("fwd", "pcaa_skinny_linear_fwd:", "buffers must be 16-B aligned", dict(bias="+4")),
    ("fwd", "pcaa_skinny_linear_fwd:", "bad act", dict(act=2)),
    ("fwd", "pcaa_skinny_linear_fwd:", "bad nsplit", dict(nsplit=0)),
    ("fwd", "pcaa_skinny_linear_fwd:", "bad nsplit", dict(nsplit=5)),
    ("fwd", "pcaa_skinny_linear_fwd:", "nsplit leaves empty splits", dict(nsplit=3)),          # 4 chunks: cps = 2, 2 splits
    ("fwd", "pcaa_skinny_linear_fwd:", "workspace too small", dict(nsplit=2, ws_floats=2 * 8 * 128 - 1)),
    ("dgrad", "pcaa_skinny_linear_dgrad:", "null pointer", dict(dx="NULL")),
    ("dgrad", "pcaa_skinny_linear_dgrad:", "unsupported shape", dict(M=0)),
    ("dgrad", "pcaa_skinny_linear_dgrad:", "bad leading dimensions", dict(lddz=254)),
    ("dgrad", "pcaa_skinny_linear_dgrad:", "bad leading dimensions", dict(ldw=127)),
    ("dgrad", "pcaa_skinny_linear_dgrad:", "bad leading dimensions", dict(ldw=1 << 23)),       # ldw N = 2^31
    ("dgrad", "pcaa_skinny_linear_dgrad:", "buffers must be 16-B aligned", dict(dz="+4")),
    ("dgrad", "pcaa_skinny_linear_dgrad:", "buffers must be 16-B aligned", dict(a_prev="+4")),
    ("dgrad", "pcaa_skinny_linear_dgrad:", "bad nsplit", dict(nsplit=5)),
    ("dgrad", "pcaa_skinny_linear_dgrad:", "nsplit leaves empty splits", dict(nsplit=3)),
    ("dgrad", "pcaa_skinny_linear_dgrad:", "workspace too small", dict(ws_floats=8 * 128 - 1)),
    ("dgrad_exact", "pcaa_skinny_linear_dgrad_exact:", "8-B aligned with an even leading dimension", dict(ldw=129)),
    ("dgrad_exact", "pcaa_skinny_linear_dgrad_exact:", "8-B aligned with an even leading dimension", dict(W="+4")),
    ("dgrad_w16", "pcaa_skinny_linear_dgrad_w16:", "4-B aligned with an even leading dimension", dict(ldw=129)),
    ("dgrad_w16", "pcaa_skinny_linear_dgrad_w16:", "4-B aligned with an even leading dimension", dict(W="+2")),
    ("wgrad", "%s:", "null pointer", dict(dW="NULL")),
    ("adam", "%s:", "null pointer", dict(coef="NULL")),
    ("rows", "%s:", "null pointer", dict(v="NULL")),
    ("wgrad", "%s:", "unsupported shape", dict(M=65)),
    ("wgrad_exact", "%s:", "unsupported shape", dict(K=48)),
    ("wgrad_bf16", "%s:", "unsupported shape", dict(N=0)),
    ("adam_exact", "%s:", "unsupported shape", dict(K=16)),
    ("rows", "%s:", "unsupported shape", dict(M=513)),
    ("rows", "%s:", "x must be allocated (and finite) for", dict(M=65, rows_alloc=127)),
    ("wgrad_bf16", "%s:", "bad leading dimensions / alignment", dict(lddw=129)),
    ("wgrad_bf16", "%s:", "bad leading dimensions / alignment", dict(dW="+2")),
    ("wgrad", "%s:", "bad leading dimensions", dict(lddz=255)),
    ("wgrad", "%s:", "bad leading dimensions", dict(lddw=127)),
    ("adam", "%s:", "bad leading dimensions", dict(ldx=127)),
    ("wgrad", "%s:", "operands beyond 32-bit", dict(lddw=1 << 23)),                            # N lddw = 2^31
    ("wgrad", "%s:", "operands beyond 32-bit", dict(lddz=1 << 28)),                            # M lddz = 2^31
    ("wgrad_bf16", "%s:", "operands beyond 32-bit", dict(ldx=1 << 28)),
    ("adam", "%s:", "operands beyond 32-bit", dict(ldw=1 << 22)),                              # fused: N ldw = 2^30
    ("rows", "%s:", "operands beyond 32-bit", dict(ldx=1 << 21)),                              # 512 ldx = 2^30
    ("rows", "%s:", "operands beyond 32-bit", dict(x="+2")),
    ("pack", "pcaa_pack_rows_t16:", "null pointer", dict(chunk="NULL")),
    ("pack", "pcaa_pack_rows_t16:", "unsupported shape", dict(rows=65)),
    ("pack", "pcaa_pack_rows_t16:", "unsupported shape", dict(rows=0)),
    ("pack", "pcaa_pack_rows_t16:", "bad leading dimensions / alignment", dict(ldx=127)),
    ("pack", "pcaa_pack_rows_t16:", "bad leading dimensions / alignment", dict(chunk="+8")),
    ("t16", "pcaa_skinny_linear_wgrad_adam_t16:", "null pointer", dict(P="NULL")),
    ("t16", "pcaa_skinny_linear_wgrad_adam_t16:", "unsupported shape", dict(chunks=9)),
    ("t16", "pcaa_skinny_linear_wgrad_adam_t16:", "unsupported shape", dict(K=48)),
    ("t16", "pcaa_skinny_linear_wgrad_adam_t16:", "below (N + K) * 64 or misaligned", dict(cs=(256 + 128) * 64 - 8)),
    ("t16", "pcaa_skinny_linear_wgrad_adam_t16:", "below (N + K) * 64 or misaligned", dict(cs=(256 + 128) * 64 + 4)),
    ("t16", "pcaa_skinny_linear_wgrad_adam_t16:", "below (N + K) * 64 or misaligned", dict(P="+8")),
    ("t16", "pcaa_skinny_linear_wgrad_adam_t16:", "operands beyond 32-bit offsets", dict(ldw=1 << 22)),
    ("t16", "pcaa_skinny_linear_wgrad_adam_t16:", "operands beyond 32-bit offsets", dict(cs=BIG)),   # 1 chunk x 2^30 x 2 B
]
OUT_OF_REACH = []                  # every PCAA_CHECK_ARG of csrc/gemm_skinny.hip ends a case above


# ------------------------------------------------------------------------------------------------ a case's reference
def case_nsplit(c):
    if c["entry"] == "fwd":
        return c["nsplit"] or splits(2 if c["variant"] == "exact" else 0, c["N"], c["K"])
    return splits(3 if c["variant"] == "exact" else 1, c["N"], c["K"])


def reference(c, bt, defect=None, before=None):
    """fwd / dgrad / wgrad of a built case -> dict(want, gate, ...)"""
    if c["entry"] == "fwd":
        return fwd_ref(bt["x"].win, bt["W"].win, bt["bias"], c["act"], case_nsplit(c), c["variant"], defect, before)
    if c["entry"] == "dgrad":
        return dgrad_ref(bt["dz"].win, bt["W"].win, bt["a_prev"], bt["out0"], c["accumulate"], case_nsplit(c), c["variant"], defect)
    v = c["variant"]
    return wgrad_ref(bt["dz"].rows(bt["dz"].r), bt["x"].rows(bt["x"].r), c["M"], BF16 if v == "bf16" else F32,
                     "exact" if v == "exact" else "bf16", defect, before)


def packed(c, bt, N, chunk_stride, device="cpu"):
    """the packed buffer of a t16 case: chunk ch at ch * chunk_stride, NaN in the gaps and in one chunk behind the last"""
    P = torch.full(((c["chunks"] + 1) * chunk_stride,), NAN, dtype=BF16, device=device)
    for ch, (dz, x) in enumerate(bt["chunks"]):
        P[ch * chunk_stride:ch * chunk_stride + (N + c["K"]) * 64] = pack_ref(dz, x, c["M"]).view(-1)
    return P


def gradient(c, bt, defect=None, P=None, chunk_stride=None):
    """the acc_ref dict of a fused-update case's gradient"""
    if c["entry"] == "t16":
        return packed_acc(P, chunk_stride, c["chunks"], bt["N"], c["K"], defect)
    return wgrad_acc(bt["dz"].rows(bt["dz"].r), bt["x"].rows(bt["x"].r), c["M"], c["variant"], defect)


def ring_of(c):
    """(JL, NB) of a fused-update case"""
    deep = c["entry"] == "t16" and c["chunks"] >= 4
    return cols_per_wave(c["N"], c["K"], 384 if deep else 1024), 4 if deep else 2
