"""Every launcher branch of csrc/pointnet_in.hip against fp64 (references, gates, cases and inputs:
tests/pointnet_in_ref.py; the gates themselves are shown reference-safe and defect-sensitive by
tests/test_pointnet_in_gates_cpu.py).

Every comparison prints ``worst |err| / gate`` (pytest -rP); the numbers are reported, the assertion is ``<= 1``
element-wise.  Widths: every cout in {4, 64, 512, 1024} (rl = 256, 16, 2, 1) at C = 4 and 5, every C in {1, 3, 4, 5, 8}
at cout = 64 and 512 (pointnet_in_ref.WIDTHS: the channel layout depends on cout alone, the feature loops on C alone);
row counts: pointnet_in_ref.row_counts (1, rl -+ 1, 127 .. 129, 255 .. 257, 300, and 17 tiles + 5 for the replica wrap).

    branch of the launcher                                            test
    ----------------------------------------------------------------  ------------------------------------------------
    pointnet_in_fwd: fp32 / bf16 y, CP 4 / 8, bias / none,            test_forward
      stats / none, y == NULL (statistics only), blockIdx % nrep
    pointnet_in_apply: fp32 / bf16, CP 4 / 8                          test_apply
    pointnet_in_apply: e4m3, split image at P / cout edges            test_apply_e4m3_and_split_edges
    bwd MODE 0: fp32 / bf16 da, CP 4 / 8, replica wrap                test_bwd_stats
    bwd MODE 1 / MODE 2 (dz_is_pre): fp32 / bf16, CP 4 / 8,           test_bwd_wgrad
      out given (dirty, zeroed with out_is_zero) / not
    bwd MODE 3: bf16 packed / fp32 scalar path, CP 4 / 8,             test_onepass
      rows form / replica form of G, pivot / pivot_mom == NULL,
      carried finalize, combine with g_rows / nrep rows
    bwd MODE 3 + combine on off-centre points                         test_onepass_offcentre
    combine: g_rows > 256 (the strided row loop)                      test_combine_long_G
    points_moments: CP 4 vector load (C == 4) / scalar, CP 8,         test_points_moments
      grid cap 512 (grid-stride loop)
    pointnet_in_moment_stats: one block / several, bias / none,       test_moment_coeffs
      running statistics on / off
    pointnet_in_wgrad: fp32 / bf16 dy, main loop / remainder / both   test_wgrad
    cast_bf16: plain / transposed / both, grid cap 2048               test_cast_bf16
    shape_ok and the wrappers' shape checks                           test_refusals_of_unsupported_widths,
                                                                      test_refusals_of_mismatched_shapes
"""
import re

import pytest
import torch

import elementwise_ref as E
import fp8_ref
import pointnet_in_ref as R
from opensetgaitrecognition_pcaa_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
WIDTH_IDS = [f"{cout}x{C}" for cout, C in R.WIDTHS]
PCAA_F32, PCAA_BF16 = 0, 1


def check(name, got, want, gate, worst=None):
    err = (got.double() - want).abs() / gate.clamp_min(1e-300)
    r = float(err.max())
    if worst is None:
        print(f"[pointnet-in] {name}: worst |err| / gate = {r:.3f}")
    else:
        key = re.sub(r" P=\d+", "", name)
        worst[key] = max(worst.get(key, 0.0), r)
    if not r <= 1.0:
        at = [int(i) for i in torch.unravel_index(err.argmax(), err.shape)]
        over = (err > 1.0).nonzero()
        print(f"[pointnet-in] {name}: worst at {at}; {over.shape[0]} of {err.numel()} over the gate, first {over[:8].tolist()}")
    assert r <= 1.0, (name, r)
    return r


def report(worst):
    for k in sorted(worst):
        print(f"[pointnet-in] {k}: worst |err| / gate = {worst[k]:.3f}")


def bn_of(cout, k, sd=0):
    bn = torch.nn.BatchNorm1d(cout).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(k["gamma"])
        bn.bias.copy_(E.uniform(cout, sd + 15, DEV, -0.5, 0.5).float())
        bn.running_mean.copy_(E.uniform(cout, sd + 16, DEV, -0.3, 0.3).float())
        bn.running_var.copy_(E.uniform(cout, sd + 17, DEV, 0.5, 1.5).float())
    return bn


# ===================================================================================================== forward, apply
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("cout,C", R.WIDTHS, ids=WIDTH_IDS)
def test_forward(cout, C, dtype):
    worst = {}
    for P in R.row_counts(cout, C, R.FWD_WRAP):
        k = R.case(cout, C, P, dtype, DEV)
        x, W, b = k["x"], k["W"], k["bias"]
        ref = R.fwd_ref(x, W, b)
        tag = f"fwd {dtype} {cout}x{C} P={P}"
        stats = ops.new_stats(cout, DEV)
        y = ops.pointnet_in_fwd(x, W, b, dtype, stats)
        assert y.dtype == dtype
        check(tag + " y", y, ref["y"], E.out_gate(ref["y_gate"], ref["y"], dtype), worst)
        check(tag + " stats", stats.sum(0), ref["stats"], ref["stats_gate"], worst)      # of the bias-free product
        check(tag + " stats per replica", stats, R.replicas(ref["block_stats"]), R.replicas(ref["block_stats_gate"]), worst)
        if -(-P // R.FWD_ROWS) <= R.NREP:
            assert not bool(stats[-(-P // R.FWD_ROWS):].any()), "a replica no workgroup maps to was written"
        # no bias, no statistics
        ref0 = R.fwd_ref(x, W, None)
        y0 = ops.pointnet_in_fwd(x, W, None, dtype)
        check(tag + " y (no bias, no stats)", y0, ref0["y"], E.out_gate(ref0["y_gate"], ref0["y"], dtype), worst)
        # statistics only: the same sums, bitwise per workgroup order aside
        only = ops.new_stats(cout, DEV)
        assert ops.pointnet_in_fwd(x, W, None, None, only) is None
        check(tag + " stats (statistics only)", only, R.replicas(ref["block_stats"]), R.replicas(ref["block_stats_gate"]), worst)
    report(worst)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("cout,C", R.WIDTHS, ids=WIDTH_IDS)
def test_apply(cout, C, dtype):
    worst = {}
    for P in R.row_counts(cout, C, R.FWD_WRAP):
        k = R.case(cout, C, P, dtype, DEV)
        a, gate = R.apply_ref(k["x"], k["W"], k["scale"], k["shift"])
        got = ops.pointnet_in_apply(k["x"], k["W"], k["scale"], k["shift"], dtype)
        check(f"apply {dtype} {cout}x{C} P={P}", got, a, E.out_gate(gate, a, dtype), worst)
    report(worst)


@pytest.mark.parametrize("cout,C,P", [(4, 4, 1), (1024, 5, 129), (64, 3, R.FWD_WRAP), (1024, 4, 255)])
def test_apply_e4m3_and_split_edges(cout, C, P):
    """the P and cout edges test_pointnet_in_apply_e4m3 (512 channels, P 300 / 129) and test_split_image_producers
    (512 channels, P 3840) lack; their checks: the e4m3 interval of fp8_ref, the split image against the fp32 output"""
    k = R.case(cout, C, P, F32, DEV)
    x = k["x"].clone()
    x[P // 2, 0] = 3000.0                                 # a point far out: outputs beyond 448 before the clamp
    a, gate = R.apply_ref(x, k["W"], k["scale"], k["shift"])
    a32 = ops.pointnet_in_apply(x, k["W"], k["scale"], k["shift"], F32)
    check(f"apply f32 {cout}x{C} P={P} (far point)", a32, a, gate)
    a8 = ops.pointnet_in_apply(x, k["W"], k["scale"], k["shift"], fp8_ref.FP8)
    assert a8.dtype == fp8_ref.FP8 and tuple(a8.shape) == (P, cout)
    ok = fp8_ref.in_interval(a8, a, gate)
    print(f"[pointnet-in] apply e4m3 {cout}x{C} P={P}: {int((~ok).sum())} of {ok.numel()} outside the interval")
    assert bool(ok.all())
    ai = ops.pointnet_in_apply(k["x"], k["W"], k["scale"], k["shift"], ops.SplitImage.dtype)
    a1 = ops.pointnet_in_apply(k["x"], k["W"], k["scale"], k["shift"], F32)
    assert tuple(ai.img.shape) == (P, 2 * cout)
    assert (ai.float() - a1).abs().max().item() <= 1e-6 * a1.abs().max().item()


# ===================================================================================================== backward, two passes
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("cout,C", R.WIDTHS, ids=WIDTH_IDS)
def test_bwd_stats(cout, C, dtype):
    worst = {}
    for P in R.row_counts(cout, C, R.BWD_WRAP):
        k = R.case(cout, C, P, dtype, DEV)
        args = (k["da"], k["x"], k["W"], k["scale"], k["shift"], k["mean"], k["rstd"])
        ref = R.bwd_stats_ref(*args)
        stats = ops.pointnet_in_bwd_stats(*args)
        tag = f"bwd_stats {dtype} {cout}x{C} P={P}"
        check(tag, stats.sum(0), ref["stats"], ref["stats_gate"], worst)
        check(tag + " per replica", stats, R.replicas(ref["block_stats"]), R.replicas(ref["block_stats_gate"]), worst)
    report(worst)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("cout,C", R.WIDTHS, ids=WIDTH_IDS)
def test_bwd_wgrad(cout, C, dtype):
    worst = {}
    for P in R.row_counts(cout, C, R.BWD_WRAP):
        k = R.case(cout, C, P, dtype, DEV)
        args = (k["da"], k["x"], k["W"], k["scale"], k["shift"], k["coef"])
        for pre in (False, True):
            want, gate = R.bwd_wgrad_ref(*args, dz_is_pre=pre)
            tag = f"bwd_wgrad MODE {2 if pre else 1} {dtype} {cout}x{C} P={P}"
            check(tag, ops.pointnet_in_bwd_wgrad(*args, dz_is_pre=pre), want, gate, worst)
            dirty = torch.full((cout, C), 7.0, device=DEV)
            out = ops.pointnet_in_bwd_wgrad(*args, out=dirty, dz_is_pre=pre)          # a dirty out is cleared first
            assert out is dirty
            check(tag + " (dirty out)", out, want, gate, worst)
            zeroed = torch.zeros((cout, C), device=DEV)
            check(tag + " (out_is_zero)", ops.pointnet_in_bwd_wgrad(*args, out=zeroed, out_is_zero=True, dz_is_pre=pre), want, gate, worst)
    report(worst)


# ===================================================================================================== backward, one pass
def raw_onepass(k, rows_form, pivot_mom, P):
    """one launch of MODE 3 through the C ABI -> (G, stats).  Rows form: G [g_rows, cout, C], sentinel-filled (every row is
    stored); replica form: zeroed G [NREP, cout, C]."""
    lib = _lib.load()
    da, x, W = k["da"], k["x"], k["W"]
    cout, C = W.shape
    stats = ops.new_stats(cout, DEV)
    if rows_form:
        G = torch.full((lib.pcaa_pointnet_in_bwd_g_rows(P), cout, C), float("nan"), device=DEV)
        fn = lib.pcaa_pointnet_in_bwd_onepass_rows
    else:
        G = torch.zeros((R.NREP, cout, C), device=DEV)
        fn = lib.pcaa_pointnet_in_bwd_onepass
    _lib.check(fn(ops._p(da), PCAA_BF16 if da.dtype == BF16 else PCAA_F32, ops._p(x), C, ops._p(W), ops._p(k["scale"]),
                  ops._p(k["shift"]), ops._p(k["mean"]), ops._p(k["rstd"]), ops._p(stats), R.NREP, ops._p(G), P, cout,
                  ops._p(pivot_mom), 1.0 / P, ops._s()), "onepass")
    return G, stats


def raw_combine(G, W, mom, coef, P, pivot_mom):
    cout, C = W.shape
    out = torch.full((cout, C), float("nan"), device=DEV)
    _lib.check(_lib.load().pcaa_pointnet_in_bwd_combine(ops._p(G), G.shape[0], ops._p(W), ops._p(mom), ops._p(coef), ops._p(out),
                                                        cout, C, P, ops._p(pivot_mom), 1.0 / P, ops._s()), "combine")
    return out


class pooled_stats:
    """the statistics buffer ops.pointnet_in_bwd_onepass takes for itself, made readable: a stats pool of the test's own"""

    def __init__(self, cout):
        self.pool = ops.StatsPool(DEV, capacity_doubles=R.NREP * 2 * cout + 64)
        self.n, self.cout = R.NREP * 2 * cout, cout

    def __enter__(self):
        self.prev = ops.STATS_POOL
        ops.set_stats_pool(self.pool)
        return self

    def begin(self):
        self.pool.off = self.pool.buf.numel()              # clear everything handed out or not
        self.pool.begin()

    def stats(self):
        return self.pool.buf[:self.n].view(R.NREP, 2, self.cout).clone()

    def __exit__(self, *exc):
        ops.set_stats_pool(self.prev)
        return False


def _onepass_case(cout, C, P, dtype, worst, offcentre=False):
    k = R.case(cout, C, P, dtype, DEV, offcentre=offcentre)
    da, x, W, sc, sh, mu, rs = (k[n] for n in ("da", "x", "W", "scale", "shift", "mean", "rstd"))
    tag = f"onepass {dtype} {cout}x{C}" + (" off-centre" if offcentre else "")
    mom = ops.points_moments(x)
    want_mom, mom_gate = R.moments_ref(x)
    check(tag + f" moments P={P}", mom, want_mom, mom_gate + 1e-300, worst)
    piv = R.pivot_of(mom, P, C)
    sref = R.bwd_stats_ref(da, x, W, sc, sh, mu, rs, onepass=True)
    bn = bn_of(cout, k)
    out = {}
    with pooled_stats(cout) as ps:
        for pm, pv, ptag in ((mom, piv, "pivot"), (None, None, "no pivot")):
            rg = R.onepass_G_ref(da, x, W, sc, sh, pv)
            # rows form
            G, stats = raw_onepass(k, True, pm, P)
            check(f"{tag} G rows, {ptag} P={P}", G, rg["G"], rg["G_gate"], worst)
            check(f"{tag} stats P={P}", stats, R.replicas(sref["block_stats"]), R.replicas(sref["block_stats_gate"]), worst)
            G2, _ = raw_onepass(k, True, pm, P)
            assert torch.equal(G, G2), "the rows form must give the same bits every run"
            # replica form and the combine over nrep = NREP rows
            Gr, stats_r = raw_onepass(k, False, pm, P)
            check(f"{tag} G replicas, {ptag} P={P}", Gr, rg["rep"], rg["rep_gate"], worst)
            check(f"{tag} stats (replica form) P={P}", stats_r.sum(0), sref["stats"], sref["stats_gate"], worst)
            if pm is not None:
                # the wrapper: rows form, carried finalize, combine -- twice, the same bits
                ps.begin()
                tail = ops.BnTailBwd(P, bn, mu, rs, cout)
                dW = ops.pointnet_in_bwd_onepass(da, x, W, sc, sh, mu, rs, tail, mom=mom)
                st = ps.stats()
                coef, dgamma, dbeta = (t.clone() for t in tail.out)
                fin = E.bn_bwd_finalize_ref(st, P, k["gamma"], mu, rs)
                for name, got in (("dbeta", dbeta), ("dgamma", dgamma), ("coef0", coef[0]), ("coef1", coef[1]), ("coef2", coef[2])):
                    check(f"{tag} finalize {name} P={P}", got, *fin[name], worst)
                ps.begin()
                tail2 = ops.BnTailBwd(P, bn, mu, rs, cout)
                dW2 = ops.pointnet_in_bwd_onepass(da, x, W, sc, sh, mu, rs, tail2, mom=mom)
                assert torch.equal(dW, dW2) and torch.equal(tail2.out[0], coef), "the same bits every run"
                want, gate = R.combine_ref(G, W, mom, coef, P, pv)                       # the kernel's own G: the combine alone
                check(f"{tag} dW against its own G, {ptag} P={P}", dW, want, gate, worst)
                out["dW"], out["coef"] = dW, coef
            else:
                coef = k["coef"]                                                        # arbitrary: nothing is dropped without a pivot
                dW = raw_combine(G, W, mom, coef, P, None)
                want, gate = R.combine_ref(G, W, mom, coef, P, None)
                check(f"{tag} dW against its own G, {ptag} P={P}", dW, want, gate, worst)
            want, gate = R.combine_ref(rg["G"], W, mom, coef, P, pv, G_gate=rg["sum_gate"])
            check(f"{tag} dW, {ptag} P={P}", dW, want, gate, worst)
            check(f"{tag} dW from replicas, {ptag} P={P}", raw_combine(Gr, W, mom, coef, P, pm), want,
                  gate + coef[0].double().abs().view(-1, 1) * R.atomic_gate(rg["G"], R.NREP).sum(0), worst)
            if pm is not None:
                out.update(want=want, gate=gate, rg=rg, mom=mom, piv=pv, k=k)
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("cout,C", R.WIDTHS, ids=WIDTH_IDS)
def test_onepass(cout, C, dtype):
    worst = {}
    for P in R.row_counts(cout, C, R.BWD_WRAP):
        _onepass_case(cout, C, P, dtype, worst)
    report(worst)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [4, 5])
@pytest.mark.parametrize("P", [300, R.BWD_WRAP])
def test_onepass_offcentre(P, C, dtype):
    """feature means up to 3 000 deviations: dW with the pivot meets its gate; the same formula with the combine's pivot
    left at 0 does not, neither as a reference for the kernel nor against the right reference"""
    worst = {}
    o = _onepass_case(512, C, P, dtype, worst, offcentre=True)
    report(worst)
    k = o["k"]
    bad, _ = R.combine_ref(o["rg"]["G"], k["W"], o["mom"], o["coef"], P, o["piv"], G_gate=o["rg"]["sum_gate"], defect="uncentred_combine")
    assert E.ratio(bad, o["want"], o["gate"]) > 10.0
    assert E.ratio(o["dW"], bad, o["gate"]) > 10.0


def test_combine_long_G():
    """g_rows = 257 > 256: the combine's lanes take a second row"""
    cout, C, P = 64, 4, 256 * 256 + 1
    worst = {}
    _onepass_case(cout, C, P, BF16, worst)
    report(worst)


# ===================================================================================================== moments
# the grid-stride case (more than 512 workgroups' worth of points) at C = 4 (vector load) and C = 5 (CP = 8)
@pytest.mark.parametrize("P,C", [(P, C) for P in (1, 255, 1025) for C in (1, 3, 4, 5, 8)] + [(512 * 1024 + 300, 4), (512 * 1024 + 300, 5)])
def test_points_moments(P, C):
    x = R.points(P, C, R.seed(0, C, P), DEV)
    mom = ops.points_moments(x)
    want, gate = R.moments_ref(x)
    assert mom.numel() == R.MOM_SIZE
    check(f"points_moments C={C} P={P}", mom, want, gate + 1e-300)
    outside = want == 0
    outside[:64].view(8, 8)[:C, :C] = False
    outside[64:64 + C] = False
    assert not bool(mom[outside].any()), "something was written outside C"
    M = mom[:64].view(8, 8)
    check(f"points_moments C={C} P={P} symmetry", M, M.t().double(), 2 * gate[:64].view(8, 8) + 1e-300)
    if C > 1:
        bad, _ = R.moments_ref(x, defect="lower_triangle_missing")
        assert E.ratio(mom, bad, gate + 1e-300) > 10.0


@pytest.mark.parametrize("update_running", [True, False], ids=["running", "frozen"])
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("cout,C,P", [(4, 4, 129), (512, 5, 1025), (1024, 3, 300), (512, 4, 2)])
def test_moment_coeffs(cout, C, P, with_bias, update_running):
    sd = R.seed(cout, C, P)
    k = R.case(cout, C, P, F32, DEV)
    x, W = k["x"], k["W"]
    bias = k["bias"] if with_bias else None
    bn = bn_of(cout, k, sd)
    beta, rm0, rv0 = bn.bias.detach().clone(), bn.running_mean.clone(), bn.running_var.clone()
    mom = ops.points_moments(x)
    scale, shift, mean, rstd, mom_out = ops.pointnet_in_moment_coeffs(x, W, bias, bn, mom=mom, update_running=update_running)
    assert mom_out is mom
    ref = R.moment_stats_ref(mom, W, P, bias, k["gamma"], beta, rm0, rv0, 0.1, bn.eps)
    tag = f"moment_coeffs {cout}x{C} P={P}"
    for name, got in (("scale", scale), ("shift", shift), ("mean", mean), ("rstd", rstd)):
        check(f"{tag} {name}", got, *ref[name])
    if update_running:
        check(tag + " running_mean", bn.running_mean, *ref["running_mean"])
        check(tag + " running_var", bn.running_var, *ref["running_var"])
        assert int(bn.num_batches_tracked) == 1
    else:
        assert torch.equal(bn.running_mean, rm0) and torch.equal(bn.running_var, rv0) and int(bn.num_batches_tracked) == 0
    # and against the statistics of the product itself (the moments' own gate carried by the reference's)
    y = x.double() @ W.double().t()
    assert torch.allclose(mean.double(), y.mean(0), rtol=1e-6, atol=1e-7)


# ===================================================================================================== plain wgrad, cast
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("cout,C", R.WIDTHS, ids=WIDTH_IDS)
def test_wgrad(cout, C, dtype):
    """a lane has rows-in-tile / rl rows: P = 4 rl is the 4-row main loop alone, P <= 3 rl the remainder loop alone"""
    rl = R.rl_of(cout)
    worst = {}
    for P in sorted(set(R.row_counts(cout, C, R.BWD_WRAP)) | {p for p in (3 * rl, 4 * rl) if p <= 256}):
        k = R.case(cout, C, P, dtype, DEV)
        want, gate = R.wgrad_ref(k["da"], k["x"])
        tag = f"wgrad {dtype} {cout}x{C} P={P}"
        check(tag, ops.pointnet_in_wgrad(k["da"], k["x"]), want, gate, worst)
        dirty = torch.full((cout, C), -3.0, device=DEV)
        check(tag + " (dirty out)", ops.pointnet_in_wgrad(k["da"], k["x"], out=dirty), want, gate, worst)
    report(worst)


@pytest.mark.parametrize("Rr,Cc", [(1, 1), (7, 5), (512, 4), (1030, 512)])
def test_cast_bf16(Rr, Cc):
    src = R.cast_values(Rr, Cc, R.seed(Rr, Cc, 0), DEV)
    plain, transposed = R.cast_bf16_ref(src)
    bits = lambda t: t.view(torch.int16)
    w, wt = ops.cast_bf16(src)
    assert torch.equal(bits(w), bits(plain)) and torch.equal(bits(wt), bits(transposed))
    w, wt = ops.cast_bf16(src, want_transposed=False)
    assert wt is None and torch.equal(bits(w), bits(plain))
    w, wt = ops.cast_bf16(src, want_plain=False)
    assert w is None and torch.equal(bits(wt), bits(transposed))
    out = torch.empty((Rr, Cc), dtype=BF16, device=DEV)
    w, wt = ops.cast_bf16(src, want_transposed=False, out=out)
    assert w is out and torch.equal(bits(out), bits(plain))


# ===================================================================================================== refusals, no launch
BAD_WIDTHS = [(4, 0), (4, 9), (6, 4), (96, 4), (2048, 4)]


def _calls(x, W, da, vec, coef):
    cout = W.shape[0]
    bn = torch.nn.BatchNorm1d(max(cout, 1)).to(DEV)
    return {
        "fwd": lambda: ops.pointnet_in_fwd(x, W, None, F32),
        "apply": lambda: ops.pointnet_in_apply(x, W, vec, vec, F32),
        "bwd_stats": lambda: ops.pointnet_in_bwd_stats(da, x, W, vec, vec, vec, vec),
        "bwd_wgrad": lambda: ops.pointnet_in_bwd_wgrad(da, x, W, vec, vec, coef),
        "bwd_wgrad(dz_is_pre)": lambda: ops.pointnet_in_bwd_wgrad(da, x, W, vec, vec, coef, dz_is_pre=True),
        "onepass": lambda: ops.pointnet_in_bwd_onepass(da, x, W, vec, vec, vec, vec, ops.BnTailBwd(x.shape[0], bn, vec, vec, cout)),
        "wgrad": lambda: ops.pointnet_in_wgrad(da, x),
    }


@pytest.mark.parametrize("cout,C", BAD_WIDTHS, ids=[f"{a}x{b}" for a, b in BAD_WIDTHS])
def test_refusals_of_unsupported_widths(cout, C):
    P = 8
    x, W = torch.zeros((P, C), device=DEV), torch.zeros((cout, C), device=DEV)
    da, vec, coef = torch.zeros((P, cout), device=DEV), torch.zeros(cout, device=DEV), torch.zeros((3, cout), device=DEV)
    for name, call in _calls(x, W, da, vec, coef).items():
        with pytest.raises(ValueError):
            call()
    if not 1 <= C <= 8:
        with pytest.raises(ValueError):
            ops.points_moments(x)
        with pytest.raises(ValueError):
            ops.pointnet_in_moment_coeffs(x, W, None, torch.nn.BatchNorm1d(cout).to(DEV))
    # the C ABI: the invalid-argument status and a message, nothing launched (the buffers hold 8 x 2048 values)
    lib = _lib.load()
    big = torch.zeros(P * 2048 * 2, device=DEV)
    dW = torch.full((2048 * 9,), 5.0, device=DEV)
    st = torch.zeros(R.NREP * 2 * 2048 + 2, dtype=torch.float64, device=DEV)
    p, s = ops._p, ops._s()
    raw = [
        ("pcaa_pointnet_in_fwd", lambda: lib.pcaa_pointnet_in_fwd(p(big), C, p(big), None, p(big), 0, P, cout, None, 1, s)),
        ("pcaa_pointnet_in_apply", lambda: lib.pcaa_pointnet_in_apply(p(big), C, p(big), p(big), p(big), p(big), 0, P, cout, s)),
        ("pcaa_pointnet_in_bwd_stats", lambda: lib.pcaa_pointnet_in_bwd_stats(p(big), 0, p(big), C, p(big), p(big), p(big), p(big), p(big), p(st), R.NREP, P, cout, s)),
        ("pcaa_pointnet_in_bwd_wgrad", lambda: lib.pcaa_pointnet_in_bwd_wgrad(p(big), 0, p(big), C, p(big), p(big), p(big), p(big), p(dW), P, cout, 0, s)),
        ("pcaa_pointnet_in_bwd_onepass", lambda: lib.pcaa_pointnet_in_bwd_onepass(p(big), 0, p(big), C, p(big), p(big), p(big), p(big), p(big), p(st), R.NREP, p(dW), P, cout, None, 0.0, s)),
        ("pcaa_pointnet_in_bwd_onepass", lambda: lib.pcaa_pointnet_in_bwd_onepass_rows(p(big), 1, p(big), C, p(big), p(big), p(big), p(big), p(big), p(st), R.NREP, p(dW), P, cout, None, 0.0, s)),
        ("pcaa_pointnet_in_wgrad", lambda: lib.pcaa_pointnet_in_wgrad(p(big), 0, p(big), C, p(dW), P, cout, s)),
    ]
    for name, call in raw:
        rc = call()
        msg = (lib.pcaa_last_error() or b"").decode()
        assert rc == 1 and msg.startswith(name), (name, rc, msg)
    torch.cuda.synchronize()
    assert bool((dW == 5.0).all()) and not bool(st.any()) and not bool(big.any())


def test_refusals_of_mismatched_shapes():
    P, C, cout = 8, 4, 64
    x, W = torch.zeros((P, C), device=DEV), torch.zeros((cout, C), device=DEV)
    da, vec, coef = torch.zeros((P, cout), device=DEV), torch.zeros(cout, device=DEV), torch.zeros((3, cout), device=DEV)
    for W_bad in (torch.zeros((cout, C + 1), device=DEV), torch.zeros((cout // 2, C), device=DEV)):
        for name, call in _calls(x, W_bad, da, vec, coef).items():
            if name == "wgrad" or (W_bad.shape[1] == C and name in ("fwd", "apply")):
                continue                                  # no W; a narrower layer is a valid forward
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        ops.pointnet_in_moment_coeffs(x, torch.zeros((cout, C + 1), device=DEV), None, torch.nn.BatchNorm1d(cout).to(DEV))
    x_short = torch.zeros((P - 1, C), device=DEV)
    for name, call in _calls(x_short, W, da, vec, coef).items():
        if name in ("fwd", "apply"):
            continue                                      # no da
        with pytest.raises(ValueError):
            call()
