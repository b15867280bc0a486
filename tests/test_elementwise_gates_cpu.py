"""The gates of tests/elementwise_ref.py, checked on the CPU at the inputs the GPU tests use (same seeds; the hash
generator makes a tensor with fewer groups a prefix of the full one).  Two conditions per gated quantity:

* NOT TOO TIGHT: a float32 torch evaluation of the same formula -- not the kernel; where the kernel's formulation
  differs from the textbook one (exp2 with log2e folded in, the streaming sum of max(z,0) + e^min(z,0), row lanes,
  fused multiply-adds emulated by rounding the exact fp64 result once) the evaluation follows it -- stays within HALF
  the gate.
* NOT VACUOUS: every planted defect, applied to the fp64 reference, moves at least 80 % of the output elements it
  touches by more than 10 x the gate.
"""
import pytest
import torch

import elementwise_ref as R

F32, BF16 = torch.float32, torch.bfloat16
LOG2E = 1.4426950408889634


def groups_for(ch):
    """reduced; the values are those of the GPU cases' first groups (more of them where a group has few channels, so
    that a defect's fraction is taken over a few thousand elements)"""
    return max(6, 4096 // ch)


STREAM = [4, 12, 32, 8, 128, 36]
GENERIC = [(ch, r) for ch in (4, 16, 64, 512, 1024) for r in (1, 3, 30, 150, 255)] + [(1024, 128), (1024, 150), (512, 128)]


def fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def f32c(x):
    return torch.tensor(x, dtype=F32)


def e_of(z, fast):
    """ELU'(z) in fp32: expf, or the bf16-storage kernels' exp2(z log2e)"""
    ex = torch.exp2(torch.minimum(z, f32c(0.0)) * f32c(LOG2E)) if fast else torch.exp(torch.minimum(z, f32c(0.0)))
    return torch.where(z > 0, torch.ones_like(z), ex)


def elu32(z, fast):
    return torch.where(z > 0, z, torch.exp2(z * f32c(LOG2E)) - 1 if fast else torch.expm1(z))


def inputs(rows, ch, dtype, seed):
    y = R.activations(rows, ch, dtype, seed)
    return (y,) + R.bn_vectors(ch, seed)


def half_gate(name, got, want, gate):
    r = R.ratio(got, want, gate)
    print(f"[gate cpu] {name}: fp32 evaluation worst |err| / gate = {r:.3f}")
    assert r <= 0.5, (name, r)


def stored_half_gate(name, got32, want, gate32, dtype):
    """a stored output: the fp32 value within half the fp32 gate; after the bf16 rounding, which reaches the whole of
    its 2^-8 |want| by itself, within the whole gate"""
    half_gate(name, got32, want, gate32)
    if dtype == BF16:
        r = R.ratio(got32.to(BF16), want, R.out_gate(gate32, want, BF16))
        print(f"[gate cpu] {name}: rounded to bf16, worst |err| / gate = {r:.3f}")
        assert r <= 1.0, (name, r)


def defect_moves(name, want, bad, gate, mask=None):
    f = R.moved(want, bad, gate, mask)
    print(f"[gate cpu] {name}: moved {f:.1%}")
    assert f >= 0.8, (name, f)


# ------------------------------------------------------------------------------------------------ mean-pool
def stream_eval(y, sc, sh, mu, rs, G, Rr):
    """the streaming kernel's formulation, rows added in order"""
    ch = y.shape[1]
    v = y.float().view(G, Rr, ch)
    l2 = f32c(LOG2E)
    sl2, tl2, nm = sc * l2, sh * l2, -mu * rs
    p = torch.zeros(G, ch)
    e1, e2 = p.clone(), p.clone()
    zero = f32c(0.0)
    for r in range(Rr):
        x = torch.exp2(torch.minimum(fma(v[:, r], sl2, tl2), zero))
        p = p + (torch.maximum(fma(v[:, r], sc, sh), zero) + x)
        e1 = e1 + x
        e2 = fma(x, fma(v[:, r], rs, nm), e2)
    n = f32c(float(Rr))
    return (p - n) * (f32c(1.0) / n), e1, e2


def generic_eval(y, sc, sh, mu, rs, G, Rr, fast):
    """the generic kernel: 256 / (ch / 4) row lanes, each adding its rows in order, the lanes then added in order"""
    ch = y.shape[1]
    rl = 256 // (ch // 4)
    v = y.float().view(G, Rr, ch)
    lanes = [[torch.zeros(G, ch) for _ in range(3)] for _ in range(rl)]
    for r in range(Rr):
        z = v[:, r] * sc + sh
        a = elu32(z, fast)
        d = torch.where(z > 0, torch.ones_like(z), a + 1)
        acc = lanes[r % rl]
        acc[0] = acc[0] + a
        acc[1] = acc[1] + d
        acc[2] = acc[2] + d * ((v[:, r] - mu) * rs)
    tot = lanes[0]
    for l in range(1, min(rl, Rr)):
        tot = [t + x for t, x in zip(tot, lanes[l])]
    return tot[0] * (f32c(1.0) / f32c(float(Rr))), tot[1], tot[2]


def _meanpool_case(ch, Rr, dtype, stream):
    seed = R.seed_of(ch, Rr)
    GROUPS = groups_for(ch)
    y, sc, sh, mu, rs = inputs(GROUPS * Rr, ch, dtype, seed)
    lanes = 1 if stream else R.row_lanes(ch)
    ref = R.meanpool_ref(y, sc, sh, mu, rs, GROUPS, Rr, lanes=lanes)
    got = stream_eval(y, sc, sh, mu, rs, GROUPS, Rr) if stream else generic_eval(y, sc, sh, mu, rs, GROUPS, Rr, dtype == BF16)
    tag = f"meanpool {'stream' if stream else 'generic'} ch={ch} R={Rr} {dtype}"
    for k, g in zip(("pooled", "e1", "e2"), got):
        half_gate(f"{tag} {k}", g, ref[k], ref[k + "_gate"])
    defects = ["drop_last_row", "shift_rows"] + (["swap_quads"] if ch >= 8 else [])
    for d in defects:
        bad = R.meanpool_ref(y, sc, sh, mu, rs, GROUPS, Rr, defect=d, lanes=lanes)
        mask = R.swapped_channels(ch) if d == "swap_quads" else None
        if d == "shift_rows":       # the last group has no next group to read from
            mask = (torch.arange(GROUPS) < GROUPS - 1).view(GROUPS, 1)
        for k in ("pooled", "e1", "e2"):
            defect_moves(f"{tag} {k} {d}", ref[k], bad[k], ref[k + "_gate"], mask)


@pytest.mark.parametrize("Rr", STREAM)
def test_meanpool_stream_gates(Rr):
    _meanpool_case(1024, Rr, BF16, True)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("ch,Rr", GENERIC)
def test_meanpool_generic_gates(ch, Rr, dtype):
    _meanpool_case(ch, Rr, dtype, False)


# ------------------------------------------------------------------------------------------------ element-wise family
ELEM = [(4, 390), (20, 300), (96, 150), (512, 129), (1020, 33), (1024, 150), (16, 127)]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("ch,rows", ELEM)
def test_bn_act_fwd_and_bwd_dy_gates(ch, rows, dtype):
    seed = R.seed_of(ch, rows)
    y, sc, sh, mu, rs = inputs(rows, ch, dtype, seed)
    want, gate = R.bn_act_fwd_ref(y, sc, sh)
    stored_half_gate(f"bn_act_fwd ch={ch} {dtype}", elu32(y.float() * sc + sh, dtype == BF16), want, gate, dtype)
    if ch >= 8:
        bad, _ = R.bn_act_fwd_ref(y, sc, sh, defect="swap_quads")
        defect_moves(f"bn_act_fwd ch={ch} {dtype} swap_quads", want, bad, R.out_gate(gate, want, dtype), R.swapped_channels(ch))
    coef = R.coef_vectors(ch, seed)
    dz = R.gradient(rows, ch, dtype, seed)
    want, gate = R.bn_bwd_dy_ref(dz, y, coef)
    stored_half_gate(f"bn_bwd_dy ch={ch} {dtype}", coef[0] * dz.float() + coef[1] * y.float() + coef[2], want, gate, dtype)
    for d in ["swap_coef"] + (["swap_quads"] if ch >= 8 else []):
        bad, _ = R.bn_bwd_dy_ref(dz, y, coef, defect=d)
        defect_moves(f"bn_bwd_dy ch={ch} {dtype} {d}", want, bad, R.out_gate(gate, want, dtype),
                     R.swapped_channels(ch) if d == "swap_quads" else None)


@pytest.mark.parametrize("pooled", [False, True])
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("ch,rows,gr", [(4, 390, 30), (20, 300, 150), (96, 150, 1), (512, 258, 129), (1020, 35, 7), (1024, 300, 150),
                                        (1024, 256, 128)])
def test_bn_bwd_dy_fused_gates(ch, rows, gr, dtype, pooled):
    seed = R.seed_of(ch, gr)
    y, sc, sh, mu, rs = inputs(rows, ch, dtype, seed)
    coef = R.coef_vectors(ch, seed, grad_scale=1.0 / gr if pooled else 1.0)
    kw = ({"dpool": R.gradient(rows // gr, ch, F32, seed), "group_rows": gr, "pool_scale": 1.0 / gr} if pooled
          else {"da": R.gradient(rows, ch, dtype, seed)})
    want, gate32 = R.bn_bwd_dy_fused_ref(y, sc, sh, coef, **kw)
    gate = R.out_gate(gate32, want, dtype)
    fast = dtype == BF16
    if fast:        # log2e folded into the affine pair
        e = torch.exp2(torch.minimum(y.float() * (sc * f32c(LOG2E)) + sh * f32c(LOG2E), f32c(0.0)))
    else:
        e = e_of(y.float() * sc + sh, False)
    g = (kw["dpool"] * f32c(1.0 / gr)).repeat_interleave(gr, 0) if pooled else kw["da"].float()
    tag = f"bn_bwd_dy_fused ch={ch} gr={gr} {dtype} {'pooled' if pooled else 'dense'}"
    stored_half_gate(tag, coef[0] * (g * e) + coef[1] * y.float() + coef[2], want, gate32, dtype)
    defects = ["swap_coef"] + (["swap_quads"] if ch >= 8 else []) + (["next_group_grad"] if pooled and rows > gr else [])
    for d in defects:
        bad, _ = R.bn_bwd_dy_fused_ref(y, sc, sh, coef, defect=d, **kw)
        mask = {"swap_quads": R.swapped_channels(ch), "next_group_grad": R.last_rows_with_next(rows, gr)}.get(d)
        defect_moves(f"{tag} {d}", want, bad, gate, mask)


@pytest.mark.parametrize("pooled", [False, True])
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("ch,rows,gr", [(4, 3870, 30), (16, 129, 1), (512, 127, 1), (1024, 300, 150), (512, 128, 1), (16, 1, 1),
                                        (1024, 133, 7)])
def test_bn_act_bwd_dz_gates(ch, rows, gr, dtype, pooled):
    seed = R.seed_of(ch, rows)
    y, sc, sh, mu, rs = inputs(rows, ch, dtype, seed)
    kw = ({"dpool": R.gradient(rows // gr, ch, F32, seed), "group_rows": gr, "pool_scale": 1.0 / gr} if pooled
          else {"da": R.gradient(rows, ch, dtype, seed)})
    ref = R.bn_act_bwd_dz_ref(y, sc, sh, mu, rs, **kw)
    fast = dtype == BF16
    g = (kw["dpool"] * f32c(1.0 / gr)).repeat_interleave(gr, 0) if pooled else kw["da"].float()
    d = g * e_of(y.float() * sc + sh, fast)
    tag = f"bn_act_bwd_dz ch={ch} rows={rows} gr={gr} {dtype} {'pooled' if pooled else 'dense'}"
    stored_half_gate(tag + " dz", d, ref["dz"], ref["dz_gate"], dtype)
    # the statistics: per 128-row workgroup the row lanes add in fp32, the rest in fp64
    rl = 256 // (ch // 4)
    t = torch.stack([d, d * ((y.float() - mu) * rs)])            # [2, rows, ch]
    stats = torch.zeros(2, ch, dtype=torch.float64)
    for r0 in range(0, rows, 128):
        blk = t[:, r0:r0 + 128]
        for lane in range(rl):
            acc = torch.zeros(2, ch)
            for r in range(lane, blk.shape[1], rl):
                acc = acc + blk[:, r]
            stats += acc.double()
    half_gate(tag + " stats", stats, ref["stats"], ref["stats_gate"])
    defects = ["drop_last_row"] + (["swap_quads"] if ch >= 8 else []) + (["next_group_grad"] if pooled and rows > gr else [])
    for df in defects:
        bad = R.bn_act_bwd_dz_ref(y, sc, sh, mu, rs, defect=df, **kw)
        if df != "drop_last_row":
            mask = {"swap_quads": R.swapped_channels(ch), "next_group_grad": R.last_rows_with_next(rows, gr)}[df]
            defect_moves(f"{tag} dz {df}", ref["dz"], bad["dz"], R.out_gate(ref["dz_gate"], ref["dz"], dtype), mask)
        if df != "next_group_grad":
            defect_moves(f"{tag} stats {df}", ref["stats"], bad["stats"], ref["stats_gate"],
                         R.swapped_channels(ch) if df == "swap_quads" else None)


@pytest.mark.parametrize("groups,ch", [(1, 4), (7, 512), (255, 1028), (773, 1024)])
def test_bn_pool_bwd_stats_gate(groups, ch):
    seed = R.seed_of(ch, groups)
    dpool = R.gradient(groups, ch, F32, seed)
    e = torch.stack([R.uniform(groups * ch, seed + 8, lo=0.0, hi=128.0).view(groups, ch),
                     R.uniform(groups * ch, seed + 9, lo=-100.0, hi=100.0).view(groups, ch)]).float()
    want, gate = R.bn_pool_bwd_stats_ref(dpool, e, 1.0 / 128)
    got = ((dpool * f32c(1.0 / 128)).unsqueeze(0) * e).double().sum(1)
    half_gate(f"bn_pool_bwd_stats groups={groups} ch={ch}", got, want, gate)
    bad, _ = R.bn_pool_bwd_stats_ref(dpool, e, 1.0 / 128, defect="drop_last_row")
    defect_moves(f"bn_pool_bwd_stats groups={groups} ch={ch} last group dropped", want, bad, gate)


# ------------------------------------------------------------------------------------------------ finalize, split-K
@pytest.mark.parametrize("ch", [4, 100, 1024])
@pytest.mark.parametrize("lin_bias", [False, True])
def test_finalize_gates(ch, lin_bias):
    case = R.finalize_case(ch, lin_bias)
    ref = R.bn_finalize_ref(case["stats"], case["count"], case["lin_bias"], case["gamma"], case["beta"], case["rm"], case["rv"],
                            0.1, R.f32(1e-5))
    # the kernel's order of operations, in fp64, rounded once
    s = case["stats"]
    s1, s2 = torch.zeros(ch, dtype=torch.float64), torch.zeros(ch, dtype=torch.float64)
    for r in range(s.shape[0]):
        s1, s2 = s1 + s[r, 0], s2 + s[r, 1]
    inv = 1.0 / case["count"]
    m0 = s1 * inv
    var = (s2 * inv - m0 * m0).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + R.f32(1e-5))
    g, b = case["gamma"].double(), case["beta"].double()
    got = {"mean": m0.float(), "rstd": rstd.float(), "scale": (g * rstd).float(), "shift": (b - m0 * g * rstd).float()}
    mean = (m0 + (case["lin_bias"].double() if lin_bias else 0.0)).float()
    unb = case["count"] / (case["count"] - 1)
    got["running_mean"] = (f32c(1.0) - f32c(0.1)) * case["rm"] + f32c(0.1) * mean
    got["running_var"] = (f32c(1.0) - f32c(0.1)) * case["rv"] + f32c(0.1) * (var * unb).float()
    for k, v in got.items():
        half_gate(f"bn_finalize ch={ch} {k}", v, *ref[k])
    # the constant column clamps at zero variance
    assert float(ref["rstd"][0][0]) == pytest.approx(1.0 / (R.f32(1e-5) ** 0.5), rel=1e-6)
    # eval coefficients in fp32
    sc, scg, sft, sftg = R.bn_eval_coeffs_ref(case["gamma"], case["beta"], case["rm"], case["rv"], case["lin_bias"], 1e-5)
    rstd32 = f32c(1.0) / torch.sqrt(case["rv"] + f32c(1e-5))
    sc32 = case["gamma"] * rstd32
    lb = case["lin_bias"] if lin_bias else torch.zeros(ch)
    half_gate(f"bn_eval_coeffs ch={ch} scale", sc32, sc, scg)
    half_gate(f"bn_eval_coeffs ch={ch} shift", case["beta"] + (lb - case["rm"]) * sc32, sft, sftg)


@pytest.mark.parametrize("nsplit", [1, 7, 8, 9, 64])
@pytest.mark.parametrize("accumulate", [False, True])
def test_splitk_reduce_gate(nsplit, accumulate):
    n = 900 * 4
    slabs = R.uniform(nsplit * n, R.seed_of(nsplit, n), lo=-1.0, hi=1.0).float()
    out0 = R.uniform(n, 5, lo=-1.0, hi=1.0).float() if accumulate else None
    want, gate = R.splitk_reduce_ref(slabs, nsplit, n, out0)
    acc = out0.clone() if accumulate else torch.zeros(n)
    for s in range(nsplit):
        acc = acc + slabs[s * n:(s + 1) * n]
    half_gate(f"splitk_reduce nsplit={nsplit} accumulate={accumulate}", acc, want, gate)
    if nsplit > 1:          # a reduction that loses its last slab
        bad, _ = R.splitk_reduce_ref(slabs, nsplit - 1, n, out0)
        defect_moves(f"splitk_reduce nsplit={nsplit} last slab dropped", want, bad, gate)
    o = acc.view(900, 4)
    sw, sg = R.colstats_of_ref(o)
    st = torch.zeros(2, 4, dtype=torch.float64)
    for r in range(900):          # ch = 4: 256 row lanes for a block's 32 rows, one row each; the lanes meet in fp64
        st += torch.stack([o[r], o[r] * o[r]]).double()
    half_gate(f"splitk_reduce_stats nsplit={nsplit}", st, sw, sg)


# ------------------------------------------------------------------------------------------------ Adam
@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
def test_adam_gate(grad_scale):
    n = 3000001
    p, g, m, v = R.adam_state(n, 0)
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    for step in range(1, 6):
        g = R.adam_gradient(n, step)
        ref = R.adam_ref(p, g, m, v, lr, b1, b2, eps, step, grad_scale)
        # common.h::adam_update with its rounding points
        fb1, fb2 = f32c(b1), f32c(b2)
        gg = g * f32c(grad_scale)
        m1 = fma(fb1, m, (f32c(1.0) - fb1) * gg)
        v1 = fma(fb2, v, ((f32c(1.0) - fb2) * gg) * gg)
        ss = f32c(R.f32(lr) / (1.0 - R.f32(b1) ** step))
        ib = f32c(1.0 / (1.0 - R.f32(b2) ** step) ** 0.5)
        denom = fma(torch.sqrt(v1), ib, f32c(eps))
        p1 = fma(-ss, m1 / denom, p)
        for k, t in (("p", p1), ("m", m1), ("v", v1)):
            half_gate(f"adam step {step} grad_scale={grad_scale} {k}", t, *ref[k])
        # a kernel that applies the update with the previous step's bias correction (the early steps: the correction
        # changes by a factor 1.9, 1.4, ... and soon by too little to count as a planted defect)
        if step in (2, 3):
            bad = R.adam_ref(p, g, m, v, lr, b1, b2, eps, step - 1, grad_scale)
            defect_moves(f"adam step {step}: bias correction of step {step - 1}", ref["p"][0], bad["p"][0], ref["p"][1])
        p, m, v = p1, m1, v1
