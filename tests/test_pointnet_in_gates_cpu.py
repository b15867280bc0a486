"""The gates of tests/pointnet_in_ref.py, checked on the CPU at the inputs the GPU tests use (same seeds and shapes:
pointnet_in_ref.case; the hash generator gives the same bits on every device).

* NOT TOO TIGHT: a float32 torch evaluation in the kernels' order -- y by C fused multiply-adds (the exact fp64 result
  rounded once), row r of a workgroup in lane r % rl, a lane adding its rows in order, the lanes then added in order
  (fp64 for the statistics, fp32 for G and dW), workgroups in fp64 for the statistics and in fp32 in two different
  orders for the atomic outputs; the bf16 one-pass path with exp2 of the pre-scaled z and its fused multiply-adds --
  stays within every gate (ratio <= 1.0).  The worst ratio per output is printed.
* NOT VACUOUS: every planted defect, applied to the fp64 restatement at a case where it can matter (checked here: a
  tail for the row defects, C < CP for "stride_cp", two workgroups in a replica for "replica_overwrite", the
  off-centre input for "uncentred_combine"), moves at least 80 % of the output elements it touches by more than 10 x
  the gate.
* EXPORTS: the built library exports what include/pcaa_hip.h declares for this file, and the two size functions answer
  as documented (no GPU call is made).
"""
import os

import pytest
import torch

import elementwise_ref as E
import pointnet_in_ref as R

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
LOG2E = 1.4426950408889634
WORST = {}


def f32c(v):
    return torch.tensor(v, dtype=F32)


def fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def e_of(z, fast):
    """ELU'(z) in fp32: expf, or the 2-byte kernels' exp2(z log2e)"""
    zn = torch.minimum(z, f32c(0.0))
    return torch.where(z > 0, torch.ones_like(z), torch.exp2(zn * f32c(LOG2E)) if fast else torch.exp(zn))


def elu32(z, fast):
    return torch.where(z > 0, z, torch.exp2(z * f32c(LOG2E)) - 1 if fast else torch.expm1(z))


def y32(x, W):
    acc = torch.zeros(x.shape[0], W.shape[0])
    for c in range(x.shape[1]):
        acc = fma(W[:, c].view(1, -1), x[:, c:c + 1], acc)
    return acc


def lanes32(a, b, block, rl):
    """per-lane fp32 sums of a [P, ch] (b None), or of the products a[p, o] b[p, c] by fused multiply-adds:
    -> [nb, lanes, ch] or [nb, lanes, ch, C]"""
    P, ch = a.shape
    rl = min(rl, block)
    nb = -(-P // block)

    def pad(t):
        p = torch.zeros((nb * block, t.shape[1]))
        p[:P] = t
        return p.view(nb, block // rl, rl, t.shape[1])
    a = pad(a)
    if b is None:
        acc = torch.zeros(nb, rl, ch)
        for j in range(block // rl):
            acc = acc + a[:, j]
        return acc
    b = pad(b)
    acc = torch.zeros(nb, rl, ch, b.shape[3])
    for j in range(block // rl):
        acc = fma(a[:, j].unsqueeze(3), b[:, j].unsqueeze(2), acc)
    return acc


def seq32(t, dim, reverse=False):
    """fp32 sum along dim, in order"""
    parts = t.unbind(dim)
    parts = parts[::-1] if reverse else parts
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    return acc


def within(name, got, want, gate):
    r = E.ratio(got, want, gate)
    WORST[name] = max(WORST.get(name, 0.0), r)
    assert r <= 1.0, (name, r)


def report(prefix):
    for k in sorted(WORST):
        if k.startswith(prefix):
            print(f"[pointnet-in gate cpu] {k}: fp32 evaluation worst |err| / gate = {WORST[k]:.3f}")


def defect_moves(name, want, bad, gate, mask=None):
    f = E.moved(want, bad, gate, mask)
    print(f"[pointnet-in gate cpu] {name}: moved {f:.1%}")
    assert f >= 0.8, (name, f)


WIDTH_IDS = [f"{cout}x{C}" for cout, C in R.WIDTHS]


# ------------------------------------------------------------------------------------------------ not too tight
@pytest.mark.parametrize("cout,C", R.WIDTHS, ids=WIDTH_IDS)
def test_forward_and_apply_gates_hold_for_an_fp32_evaluation(cout, C):
    rl = R.rl_of(cout)
    for P in R.row_counts(cout, C, R.FWD_WRAP):
        k = R.case(cout, C, P, F32)
        x, W, b, sc, sh = k["x"], k["W"], k["bias"], k["scale"], k["shift"]
        acc = y32(x, W)
        ref = R.fwd_ref(x, W, b)
        for dtype in DTYPES:
            within(f"fwd y {dtype}", (acc + b).to(dtype), ref["y"], E.out_gate(ref["y_gate"], ref["y"], dtype))
        st = torch.stack([lanes32(acc, None, R.FWD_ROWS, rl).double().sum(1), lanes32(acc * acc, None, R.FWD_ROWS, rl).double().sum(1)], 1)
        within("fwd stats per workgroup", st, ref["block_stats"], ref["block_stats_gate"])
        within("fwd stats", st.sum(0), ref["stats"], ref["stats_gate"])
        a, gate = R.apply_ref(x, W, sc, sh)
        for dtype in DTYPES:
            within(f"apply {dtype}", elu32(acc * sc + sh, dtype == BF16).to(dtype), a, E.out_gate(gate, a, dtype))
    report("fwd")
    report("apply")


def atomic32(name, per_wg, want, gate):
    """fp32 workgroup partials [nb, ...] met in two different orders"""
    for rev in (False, True):
        within(name, seq32(per_wg, 0, rev), want, gate)


def contract32(d, xs, rl):
    """[nb, cout, C]: per-workgroup fp32 sums of d x by fused multiply-adds, lanes added in order"""
    return seq32(lanes32(d, xs, R.BWD_ROWS, rl), 1)


@pytest.mark.parametrize("cout,C", R.WIDTHS, ids=WIDTH_IDS)
def test_backward_gates_hold_for_an_fp32_evaluation(cout, C):
    rl = R.rl_of(cout)
    for P in R.row_counts(cout, C, R.BWD_WRAP):
        for dtype in DTYPES:
            _backward_case(cout, C, P, dtype, rl, False)
    report("bwd")
    report("onepass")
    report("wgrad")


def _backward_case(cout, C, P, dtype, rl, offcentre):
    k = R.case(cout, C, P, dtype, offcentre=offcentre)
    x, W, da, sc, sh, mu, rs, cf = (k[n] for n in ("x", "W", "da", "scale", "shift", "mean", "rstd", "coef"))
    fast = dtype == BF16
    g = da.float()
    yv = y32(x, W)
    tag = f"{dtype}" + (" off-centre" if offcentre else "")
    # MODE 0
    d = g * e_of(yv * sc + sh, fast)
    st = torch.stack([lanes32(d, None, R.BWD_ROWS, rl).double().sum(1),
                      lanes32(d * ((yv - mu) * rs), None, R.BWD_ROWS, rl).double().sum(1)], 1)
    ref = R.bwd_stats_ref(da, x, W, sc, sh, mu, rs)
    within(f"bwd_stats {tag}", st.sum(0), ref["stats"], ref["stats_gate"])
    within(f"bwd_stats per workgroup {tag}", st, ref["block_stats"], ref["block_stats_gate"])
    # MODE 1 / MODE 2
    if not offcentre:
        for pre in (False, True):
            dd = g if pre else d
            dy = cf[0] * dd + cf[1] * yv + cf[2]
            want, gate = R.bwd_wgrad_ref(da, x, W, sc, sh, cf, dz_is_pre=pre)
            atomic32(f"bwd_wgrad MODE {2 if pre else 1} {tag}", contract32(dy, x, rl), want, gate)
        want, gate = R.wgrad_ref(da, x)
        atomic32(f"wgrad {tag}", contract32(g, x, rl), want, gate)
    # MODE 3, with and without a pivot
    mom, _ = R.moments_ref(x)
    for piv in (R.pivot_of(mom, P, C), None):
        xc = x - piv if piv is not None else x
        if fast:
            l2 = f32c(LOG2E)
            e = torch.exp2(torch.minimum(fma(yv, sc * l2, sh * l2), f32c(0.0)))
            d3 = g * e
            s2 = _fma_lanes(d3, fma(yv, rs, -mu * rs), rl)
        else:
            d3 = d
            s2 = lanes32(d3 * ((yv - mu) * rs), None, R.BWD_ROWS, rl)
        st3 = torch.stack([lanes32(d3, None, R.BWD_ROWS, rl).double().sum(1), s2.double().sum(1)], 1)
        ref3 = R.bwd_stats_ref(da, x, W, sc, sh, mu, rs, onepass=True)
        within(f"onepass stats {tag}", st3.sum(0), ref3["stats"], ref3["stats_gate"])
        G = contract32(d3, xc, rl)
        rg = R.onepass_G_ref(da, x, W, sc, sh, piv)
        ptag = "pivot" if piv is not None else "no pivot"
        within(f"onepass G rows {tag} {ptag}", G, rg["G"], rg["G_gate"])
        nb = G.shape[0]
        for rev in (False, True):
            order = list(range(nb))[::-1] if rev else list(range(nb))
            rep = torch.zeros(R.NREP, cout, C)
            for b in order:
                rep[b % R.NREP] = rep[b % R.NREP] + G[b]
            within(f"onepass G replicas {tag} {ptag}", rep, rg["rep"], rg["rep_gate"])
        # the combine on the fp32 G: the whole chain's dW against the reference's, with the gate of G' carried
        coef = cf if piv is None else _finalize_coef(st3, P, k["gamma"], mu, rs)
        want, gate = R.combine_ref(rg["G"], W, mom, coef, P, piv, G_gate=rg["sum_gate"])
        within(f"onepass dW {tag} {ptag}", _combine_other_order(G, W, mom, coef, P, piv), want, gate)
        # and the combine alone, handed the same G on both sides
        want, gate = R.combine_ref(G, W, mom, coef, P, piv)
        within(f"combine alone {tag} {ptag}", _combine_other_order(G, W, mom, coef, P, piv), want, gate)


def _fma_lanes(a, b, rl):
    """per-lane sums of the element-wise products a b, by fused multiply-adds"""
    P, ch = a.shape
    nb = -(-P // R.BWD_ROWS)
    pa, pb = torch.zeros(nb * R.BWD_ROWS, ch), torch.zeros(nb * R.BWD_ROWS, ch)
    pa[:P], pb[:P] = a, b
    pa, pb = (t.view(nb, R.BWD_ROWS // rl, rl, ch) for t in (pa, pb))
    acc = torch.zeros(nb, rl, ch)
    for j in range(R.BWD_ROWS // rl):
        acc = fma(pa[:, j], pb[:, j], acc)
    return acc


def _finalize_coef(stats_per_wg, P, gamma, mean, rstd):
    """fp32 coef [3, cout] of bn_bwd_finalize from these statistics (what the carried finalize hands the combine)"""
    out = E.bn_bwd_finalize_ref(stats_per_wg.double().sum(0).unsqueeze(0), P, gamma, mean, rstd)
    return torch.stack([out["coef0"][0], out["coef1"][0], out["coef2"][0]]).float()


def _combine_other_order(G, W, mom, coef, P, piv):
    """the combine in fp64 in the kernel's order of operations (G's rows strided over 256 lanes, the sum over k in
    order), rounded once to fp32"""
    cout, C = W.shape
    rows = G.shape[0]
    g = torch.zeros(256, cout, C, dtype=torch.float64)
    for r in range(rows):
        g[r % 256] += G[r].double()
    g = g.view(4, 64, cout, C).sum(1)
    g = (g[0] + g[1]) + (g[2] + g[3])
    M, sx = mom[:64].view(8, 8), mom[64:]
    p = piv.double() if piv is not None else torch.zeros(C, dtype=torch.float64)
    yx = torch.zeros(cout, C, dtype=torch.float64)
    for kk in range(C):
        yx += W[:, kk:kk + 1].double() * (M[kk, :C] - p * sx[kk]).view(1, C)
    cf = coef.double()
    return (cf[0].view(-1, 1) * g + cf[1].view(-1, 1) * yx + cf[2].view(-1, 1) * (sx[:C] - float(P) * p).view(1, C)).float()


@pytest.mark.parametrize("C", [4, 5])
@pytest.mark.parametrize("P", [300, R.BWD_WRAP])
def test_offcentre_gates_hold_for_an_fp32_evaluation(P, C):
    for dtype in DTYPES:
        _backward_case(512, C, P, dtype, 2, True)
    report("bwd")
    report("onepass")
    report("combine")


def test_long_G_combine_gate():
    """g_rows > 256: the combine's strided row loop (the GPU case's P, cout, C; G from the fp64 reference rounded to fp32)"""
    cout, C, P = 64, 4, 256 * 256 + 1
    k = R.case(cout, C, P, BF16)
    mom, _ = R.moments_ref(k["x"])
    piv = R.pivot_of(mom, P, C)
    rg = R.onepass_G_ref(k["da"], k["x"], k["W"], k["scale"], k["shift"], piv)
    G = rg["G"].float()
    assert G.shape[0] == 257
    want, gate = R.combine_ref(G, k["W"], mom, k["coef"], P, piv)
    within("combine g_rows 257", _combine_other_order(G, k["W"], mom, k["coef"], P, piv), want, gate)
    report("combine")


@pytest.mark.parametrize("C", [1, 3, 4, 5, 8])
def test_moment_gates(C):
    for P in (1, 255, 1025):
        x = R.points(P, C, R.seed(0, C, P))
        want, gate = R.moments_ref(x)
        xd = x.double()
        got = torch.zeros(R.MOM_SIZE, dtype=torch.float64)
        for r in range(P - 1, -1, -1):               # one point at a time, from the end
            got[:64].view(8, 8)[:C, :C] += xd[r].view(C, 1) * xd[r].view(1, C)
            got[64:64 + C] += xd[r]
        within("moments", got, want, gate)
        # the coefficients from them: the kernel's loops (k outer, c inner) against the reference's matrix products
        for cout in (4, 512):
            sd = R.seed(cout, C, P)
            W = R.weights(cout, C, sd)
            vec = dict(lin_bias=R.lin_bias(cout, sd), gamma=R.gamma_of(cout, sd), beta=E.uniform(cout, sd + 15, "cpu", -0.5, 0.5).float(),
                       running_mean=E.uniform(cout, sd + 16, "cpu", -0.3, 0.3).float(), running_var=E.uniform(cout, sd + 17, "cpu", 0.5, 1.5).float())
            ref = R.moment_stats_ref(want, W, P, momentum=0.1, eps=1e-5, **vec)
            Wd = W.double()
            s1, s2 = torch.zeros(cout, dtype=torch.float64), torch.zeros(cout, dtype=torch.float64)
            for kk in range(C):
                s1 += Wd[:, kk] * want[64 + kk]
                row = torch.zeros(cout, dtype=torch.float64)
                for c in range(C):
                    row += want[kk * 8 + c] * Wd[:, c]
                s2 += Wd[:, kk] * row
            got = E.bn_finalize_ref(torch.stack([s1, s2]).unsqueeze(0), P, vec["lin_bias"], vec["gamma"], vec["beta"],
                                    vec["running_mean"], vec["running_var"], 0.1, 1e-5)
            for name in ref:
                within(f"moment_coeffs {name}", got[name][0].float(), *ref[name])
    report("moment")


# ------------------------------------------------------------------------------------------------ not vacuous
ROW_DEFECT_CASES = [(512, 4, 300), (512, 5, 300), (64, 4, 300), (1024, 5, 257), (512, 4, R.BWD_WRAP)]


@pytest.mark.parametrize("defect", ["drop_tail_rows", "count_clamped_row"])
@pytest.mark.parametrize("cout,C,P", ROW_DEFECT_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_row_defects_fail_the_gates(dtype, cout, C, P, defect):
    rl = R.rl_of(cout)
    for trip in (4, 8):
        assert R.has_tail(P, R.BWD_ROWS, trip, rl), "the case has no tail: the defect could not matter"
    k = R.case(cout, C, P, dtype)
    x, W, da, sc, sh, mu, rs, cf = (k[n] for n in ("x", "W", "da", "scale", "shift", "mean", "rstd", "coef"))
    tag = f"{defect} {dtype} {cout}x{C} P={P}"
    for onepass in (False, True):
        good, bad = (R.bwd_stats_ref(da, x, W, sc, sh, mu, rs, defect=d, onepass=onepass) for d in (None, defect))
        defect_moves(tag + f" stats (MODE {3 if onepass else 0})", good["stats"], bad["stats"], good["stats_gate"])
    for pre in (False, True):
        (want, gate), (bad, _) = (R.bwd_wgrad_ref(da, x, W, sc, sh, cf, dz_is_pre=pre, defect=d) for d in (None, defect))
        defect_moves(tag + f" dW (MODE {2 if pre else 1})", want, bad, gate)
    mom, _ = R.moments_ref(x)
    piv = R.pivot_of(mom, P, C)
    good, bad = (R.onepass_G_ref(da, x, W, sc, sh, piv, defect=d) for d in (None, defect))
    last = torch.zeros(good["G"].shape[0], 1, 1, dtype=torch.bool)
    last[-1] = True                                      # the workgroup with the tail
    defect_moves(tag + " G rows", good["G"], bad["G"], good["G_gate"], last if defect == "drop_tail_rows" else None)
    (want, gate), (bad, _) = (R.wgrad_ref(da, x, defect=d) for d in (None, defect))
    defect_moves(tag + " wgrad", want, bad, gate)


@pytest.mark.parametrize("cout,C,P", [(64, 4, 129), (512, 5, 300), (1024, 4, 257), (64, 8, 300)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_swapped_quads_and_coefficients_fail_the_gates(dtype, cout, C, P):
    k = R.case(cout, C, P, dtype)
    x, W, b, da, sc, sh, mu, rs, cf = (k[n] for n in ("x", "W", "bias", "da", "scale", "shift", "mean", "rstd", "coef"))
    ch = E.swapped_channels(cout)
    tag = f"swap_quads {dtype} {cout}x{C} P={P}"
    good, bad = (R.fwd_ref(x, W, b, defect=d) for d in (None, "swap_quads"))
    defect_moves(tag + " fwd y", good["y"], bad["y"], E.out_gate(good["y_gate"], good["y"], dtype), ch)
    defect_moves(tag + " fwd stats", good["stats"], bad["stats"], good["stats_gate"], ch)
    (a, gate), (abad, _) = (R.apply_ref(x, W, sc, sh, defect=d) for d in (None, "swap_quads"))
    defect_moves(tag + " apply", a, abad, E.out_gate(gate, a, dtype), ch)
    good, bad = (R.bwd_stats_ref(da, x, W, sc, sh, mu, rs, defect=d) for d in (None, "swap_quads"))
    defect_moves(tag + " bwd_stats", good["stats"], bad["stats"], good["stats_gate"], ch)
    for d in ("swap_quads", "swap_coef"):
        for pre in (False, True):
            (want, gate), (wbad, _) = (R.bwd_wgrad_ref(da, x, W, sc, sh, cf, dz_is_pre=pre, defect=dd) for dd in (None, d))
            defect_moves(f"{d} {dtype} {cout}x{C} P={P} dW (MODE {2 if pre else 1})", want, wbad, gate, ch.view(-1, 1) if d == "swap_quads" else None)
    good, bad = (R.onepass_G_ref(da, x, W, sc, sh, None, defect=d) for d in (None, "swap_quads"))
    defect_moves(tag + " G", good["G"], bad["G"], good["G_gate"], ch.view(1, -1, 1))
    (want, gate), (wbad, _) = (R.wgrad_ref(da, x, defect=d) for d in (None, "swap_quads"))
    defect_moves(tag + " wgrad", want, wbad, gate, ch.view(-1, 1))
    mom, _ = R.moments_ref(x)
    G = good["G"].float()
    (want, gate), (wbad, _) = (R.combine_ref(G, W, mom, cf, P, None, defect=d) for d in (None, "swap_coef"))
    defect_moves(f"swap_coef {dtype} {cout}x{C} P={P} combine", want, wbad, gate)


@pytest.mark.parametrize("cout,C,P", [(64, 1, 129), (512, 3, 300), (64, 5, 257), (512, 5, R.BWD_WRAP)])
def test_stride_cp_fails_the_gates(cout, C, P):
    assert C < (4 if C <= 4 else 8), "C == CP: the stride is the right one"
    k = R.case(cout, C, P, BF16)
    x, W, b, da, sc, sh, mu, rs, cf = (k[n] for n in ("x", "W", "bias", "da", "scale", "shift", "mean", "rstd", "coef"))
    rows = torch.ones(P, 1, dtype=torch.bool)
    rows[0] = False                                       # row 0 is read at the right place
    tag = f"stride_cp {cout}x{C} P={P}"
    good, bad = (R.fwd_ref(x, W, b, defect=d) for d in (None, "stride_cp"))
    defect_moves(tag + " fwd y", good["y"], bad["y"], E.out_gate(good["y_gate"], good["y"], BF16), rows)
    defect_moves(tag + " fwd stats", good["stats"], bad["stats"], good["stats_gate"])
    (a, gate), (abad, _) = (R.apply_ref(x, W, sc, sh, defect=d) for d in (None, "stride_cp"))
    defect_moves(tag + " apply", a, abad, E.out_gate(gate, a, BF16), rows)
    good, bad = (R.bwd_stats_ref(da, x, W, sc, sh, mu, rs, defect=d) for d in (None, "stride_cp"))
    defect_moves(tag + " bwd_stats", good["stats"], bad["stats"], good["stats_gate"])
    (want, gate), (wbad, _) = (R.bwd_wgrad_ref(da, x, W, sc, sh, cf, defect=d) for d in (None, "stride_cp"))
    defect_moves(tag + " dW", want, wbad, gate)
    good, bad = (R.onepass_G_ref(da, x, W, sc, sh, None, defect=d) for d in (None, "stride_cp"))
    defect_moves(tag + " G", good["G"], bad["G"], good["G_gate"])
    (want, gate), (wbad, _) = (R.wgrad_ref(da, x, defect=d) for d in (None, "stride_cp"))
    defect_moves(tag + " wgrad", want, wbad, gate)


@pytest.mark.parametrize("cout,C,P", [(4, 4, 1), (512, 5, 300), (64, 3, 129)])
def test_bias_in_stats_fails_the_gate(cout, C, P):
    k = R.case(cout, C, P, F32)
    good, bad = (R.fwd_ref(k["x"], k["W"], k["bias"], defect=d) for d in (None, "bias_in_stats"))
    defect_moves(f"bias_in_stats {cout}x{C} P={P}", good["stats"], bad["stats"], good["stats_gate"])


@pytest.mark.parametrize("cout,C,P", [(4, 4, 255), (512, 5, 300), (1024, 4, 1)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_elu_twice_fails_the_gate(dtype, cout, C, P):
    k = R.case(cout, C, P, dtype)
    args = (k["da"], k["x"], k["W"], k["scale"], k["shift"], k["coef"])
    (want, gate), (bad, _) = (R.bwd_wgrad_ref(*args, dz_is_pre=True, defect=d) for d in (None, "elu_twice"))
    defect_moves(f"elu_twice {dtype} {cout}x{C} P={P}", want, bad, gate)


@pytest.mark.parametrize("C", [4, 5])
@pytest.mark.parametrize("P", [300, R.BWD_WRAP])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_uncentred_combine_fails_the_gate_on_the_offcentre_input(dtype, P, C):
    cout = 512
    k = R.case(cout, C, P, dtype, offcentre=True)
    x = k["x"].double()
    assert float((x.mean(0).abs() / x.std(0)).max()) > 50, "the input is not off-centre"
    mom, _ = R.moments_ref(k["x"])
    piv = R.pivot_of(mom, P, C)
    rg = R.onepass_G_ref(k["da"], k["x"], k["W"], k["scale"], k["shift"], piv)
    st = R.bwd_stats_ref(k["da"], k["x"], k["W"], k["scale"], k["shift"], k["mean"], k["rstd"], onepass=True)
    coef = _finalize_coef(st["block_stats"], P, k["gamma"], k["mean"], k["rstd"])
    (want, gate), (bad, _) = (R.combine_ref(rg["G"], k["W"], mom, coef, P, piv, G_gate=rg["sum_gate"], defect=d)
                              for d in (None, "uncentred_combine"))
    defect_moves(f"uncentred_combine {dtype} C={C} P={P}", want, bad, gate)
    # with coef from the finalize of the same statistics the dropped term is rounding noise: the formula IS dy^T x
    y = x @ k["W"].double().t()
    z = y * k["scale"].double() + k["shift"].double()
    dz = k["da"].double() * E.elu_grad(z)
    dy = coef[0].double() * dz + coef[1].double() * y + coef[2].double()
    full = dy.t() @ x
    dropped = dy.sum(0).abs().view(-1, 1) * piv.double().abs().view(1, -1)
    assert float(((want - full).abs() / (gate + dropped)).max()) <= 1.0


@pytest.mark.parametrize("C", [3, 4, 5, 8])
def test_lower_triangle_missing_fails_the_gate(C):
    for P in (1, 255, 1025):
        x = R.points(P, C, R.seed(0, C, P))
        (want, gate), (bad, _) = (R.moments_ref(x, defect=d) for d in (None, "lower_triangle_missing"))
        defect_moves(f"lower_triangle_missing C={C} P={P}", want, bad, gate + 1e-300)


@pytest.mark.parametrize("cout,C", [(64, 4), (512, 5)])
def test_replica_overwrite_fails_the_gate(cout, C):
    P = R.BWD_WRAP
    assert -(-P // R.BWD_ROWS) > R.NREP, "no replica receives two workgroups"
    k = R.case(cout, C, P, BF16)
    good, bad = (R.onepass_G_ref(k["da"], k["x"], k["W"], k["scale"], k["shift"], None, defect=d) for d in (None, "replica_overwrite"))
    defect_moves(f"replica_overwrite {cout}x{C}", good["rep"], bad["rep"], good["rep_gate"])
    assert bool((good["rep"][2:] == bad["rep"][2:]).all())


# ------------------------------------------------------------------------------------------------ the C ABI, no GPU needed
DECLARED = ("pcaa_pointnet_in_fwd", "pcaa_pointnet_in_wgrad", "pcaa_pointnet_in_apply", "pcaa_pointnet_in_bwd_stats",
            "pcaa_pointnet_in_bwd_onepass", "pcaa_pointnet_in_bwd_onepass_rows", "pcaa_pointnet_in_bwd_g_rows",
            "pcaa_pointnet_in_bwd_combine", "pcaa_pointnet_in_moment_stats", "pcaa_pointnet_in_bwd_wgrad",
            "pcaa_points_moments_size", "pcaa_points_moments", "pcaa_cast_bf16")


def test_library_exports_what_the_header_declares():
    from opensetgaitrecognition_pcaa_amd import _lib
    protos = _lib.parse_header()
    declared = sorted(n for n in protos if n.startswith(("pcaa_pointnet_in_", "pcaa_points_moments")) or n == "pcaa_cast_bf16")
    assert declared == sorted(DECLARED)
    assert os.path.exists(_lib.LIB_PATH), "libpcaa_hip.so has not been built (python -m opensetgaitrecognition_pcaa_amd.build)"
    lib = _lib.load()                         # dlopen and prototypes only: no HIP call is made
    for name in DECLARED:
        assert hasattr(lib, name), f"libpcaa_hip.so does not export {name}"
    assert lib.pcaa_points_moments_size() == R.MOM_SIZE == 72
    ps = {P for cout, C in R.WIDTHS for P in R.row_counts(cout, C, R.BWD_WRAP)} | {R.FWD_WRAP, 256 * 256 + 1, 512 * 1024 + 300}
    for P in sorted(ps):
        assert lib.pcaa_pointnet_in_bwd_g_rows(P) == -(-P // 256), P
