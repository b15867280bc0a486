"""The gates of tests/critic_loss_ref.py themselves, on the CPU, at the inputs tests/test_critic_loss_branches.py uses:

* an fp32 torch evaluation of each kernel's formulation (chamfer: the expanded form |g|^2 + |p|^2 - 2 g.p) stays within
  HALF the gate;
* every planted defect moves >= 80 % of the output elements it touches by more than 10 x the gate;
* every input condition holds on the fp64 reference: the chamfer cap of 2 % unsettled prediction points, the logit gap,
  min |pre-activation| of the critic with both ELU sides present;
* the closed forms the gates are propagated through (``*_en``) equal fp64 autograd.

Each check prints its figure (pytest -rP)."""
import numpy as np
import pytest
import torch

import critic_loss_ref as R

F32 = torch.float32


def half(name, got, want, gate, mask=None):
    err = (got.double() - want).abs() / gate.clamp_min(1e-300)
    if mask is not None:
        err = err[mask]
    r = float(err.max()) if err.numel() else 0.0
    print(f"[gates] {name}: fp32 evaluation, worst |err| / gate = {r:.4f}")
    assert r <= 0.5, (name, r)
    return r


def bites(name, want, bad, gate, mask=None):
    touched = int(((bad != want) if mask is None else ((bad != want) & mask)).sum())
    assert touched > 0, (name, "the defect touches nothing at this case")
    m = R.moved(want, bad, gate, mask)
    print(f"[gates] {name}: moves {100 * m:.1f} % of the {touched} elements it touches by > 10 x gate")
    assert m >= 0.8, (name, m)


# ====================================================================================================== chamfer
def chamfer_expanded_f32(preds, gts):
    """the kernel's formulation in fp32 torch -> (P [B, T, i, j], per-prediction minima, per-ground-truth minima)"""
    x, y = gts.permute(0, 2, 3, 1), preds.permute(0, 2, 3, 1)
    P = (x * x).sum(-1).unsqueeze(3) + (y * y).sum(-1).unsqueeze(2) - 2 * (x @ y.transpose(2, 3))
    return P, P.min(dim=2), P.min(dim=3)


def grad_from_nn(preds, gts, nn_pred, nn_gt, w):
    """fp32 gradient from given nearest neighbours (the kernel's gather)"""
    p, g = preds.permute(0, 2, 3, 1), gts.permute(0, 2, 3, 1)
    B, T, N, C = p.shape
    ix = lambda idx: idx.unsqueeze(-1).expand(B, T, N, C)
    out = 2 * w * (p - g.gather(2, ix(nn_pred)))
    out = out.scatter_add(2, ix(nn_gt), 2 * w * (p.gather(2, ix(nn_gt)) - g))
    return out.permute(0, 3, 1, 2)


CHAMFER_RUNS = [(s, None) for s in R.CHAMFER_SHAPES] + [(s, d) for s in R.CHAMFER_SMALL[2:] for d in ("gt", "pred")]


@pytest.mark.parametrize("shape,dup", CHAMFER_RUNS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_chamfer_gates(shape, dup):
    B, T, N, C = shape
    preds, gts = R.chamfer_inputs(B, T, N, C, dup=dup)
    gpb = R.chamfer_grad_per_b(B)
    ref = R.chamfer_ref(preds, gts, -0.37, gpb)
    share = float(ref["unsettled"].double().mean())
    print(f"[gates] chamfer {shape} dup={dup}: unsettled prediction points {100 * share:.3f} %")
    assert share <= R.CH_UNSETTLED_CAP
    tag = f"chamfer {shape} dup={dup}"
    P, (dp, np_), (dg, ng) = chamfer_expanded_f32(preds, gts)
    half(tag + " nearest distance (pred)", dp, ref["d_pred"], ref["item_gate_pred"])
    half(tag + " nearest distance (gt)", dg, ref["d_gt"], ref["item_gate_gt"])
    half(tag + " loss", dp.sum(-1) + dg.sum(-1), ref["loss"], ref["loss_gate"])
    w = (torch.tensor(-0.37, dtype=F32) * gpb).view(B, 1, 1, 1)
    if dup != "pred":
        half(tag + " grad", grad_from_nn(preds, gts, np_, ng, w), ref["grad"], ref["grad_gate"], R.settled_mask(ref))
    else:      # a duplicate set is compared by its sum (whichever member the ground truth chose), settled sets only
        same = ref["same_pred"]
        set_ok = ~(same & ref["unsettled"].unsqueeze(2)).any(3)
        got = R.duplicate_set_sums(grad_from_nn(preds, gts, np_, ng, w), same)
        half(tag + " grad summed over duplicate sets", got, R.duplicate_set_sums(ref["grad"], same),
             R.duplicate_set_sums(ref["grad_gate"], same), set_ok.unsqueeze(1).expand_as(got))
        first = torch.where(same, torch.arange(N).view(1, 1, 1, N), N).min(3).values      # lowest index of every set
        assert torch.equal(first.gather(2, ref["nn_gt"]), ref["nn_gt"]), "the reference chooses the lowest index of a duplicate set"


@pytest.mark.parametrize("defect", R.CHAMFER_DEFECTS)
def test_chamfer_defects(defect):
    for B, T, N, C in ((2, 3, 2, 3), (3, 2, 128, 4), (2, 2, 129, 5)):
        preds, gts = R.chamfer_inputs(B, T, N, C)
        gpb = R.chamfer_grad_per_b(B)
        ref = R.chamfer_ref(preds, gts, 1.0, gpb)
        bad = R.chamfer_ref(preds, gts, 1.0, gpb, defect=defect)
        tag = f"chamfer defect {defect} {(B, T, N, C)}"
        if defect in ("skip_last_gt", "pad_nonzero", "swap_bt"):
            bites(tag + " loss", ref["loss"], bad["loss"], ref["loss_gate"])
        if defect != "swap_bt":
            bites(tag + " grad", ref["grad"], bad["grad"], ref["grad_gate"], R.settled_mask(ref))


# ====================================================================================================== cross-entropy
def ce_f32(x, target, gs):
    B, K = x.shape
    mx = x.max(1, keepdim=True).values
    e = torch.exp(x - mx)
    se = e.sum(1, keepdim=True)
    oh = torch.nn.functional.one_hot(target, K).float()
    row = (torch.log(se) + mx).squeeze(1) - (x * oh).sum(1)
    return (row.double().sum() / B).float(), gs * (e * (1.0 / se) - oh) / B, (e / se).argmax(1)


@pytest.mark.parametrize("case", R.CE_CASES, ids=lambda s: "x".join(map(str, s)))
def test_cross_entropy_gates(case):
    B, K, mag = case
    x, t = R.ce_inputs(B, K, mag)
    ref = R.ce_ref(x, t, -2.5)
    assert bool(((ref["gap"] == 0) | (ref["gap"] >= 1e-3)).all()), "the top-two gap of a row is 0 or at least 1e-3"
    assert float(x.abs().max()) <= mag + 0.5
    loss, grad, _ = ce_f32(x, t, torch.tensor(-2.5, dtype=F32))
    tag = f"cross_entropy {case}"
    half(tag + " loss", loss, ref["loss"], ref["loss_gate"])
    half(tag + " grad", grad, ref["grad"], ref["grad_gate"])
    ties = x == x.max(1, keepdim=True).values
    assert torch.equal(ref["preds"], ties.float().argmax(1)) and bool((x.gather(1, ref["preds"].view(-1, 1)) == x.max(1, keepdim=True).values).all())
    if B >= 5 and K >= 2:
        assert int((ties.sum(1) == K).sum()) > 0 and int((ties.sum(1) == 2).sum()) > 0, "all-equal rows and two-maxima rows"


@pytest.mark.parametrize("defect", R.CE_DEFECTS)
def test_cross_entropy_defects(defect):
    # (the last class left out of the max shows where it leads by more than fp32 expf can hold: K = 2 at magnitude 80)
    for B, K, mag in ((37, 2, 80),) if defect == "max_skip_last" else ((257, 6, 80), (600, 64, 80)):
        x, t = R.ce_inputs(B, K, mag)
        ref, bad = R.ce_ref(x, t), R.ce_ref(x, t, defect=defect)
        tag = f"cross_entropy defect {defect} {(B, K, mag)}"
        bites(tag + " loss", ref["loss"].view(1), bad["loss"].view(1), ref["loss_gate"].view(1))
        if defect == "mean_over_256":
            bites(tag + " grad", ref["grad"], bad["grad"], ref["grad_gate"], ref["grad"].abs() > 1e-30)


# ====================================================================================================== critic
def _disc_ids(c):
    return f"K{c[0]}-B{c[1]}-{'dense' if c[2] else 'onehot'}"


def _same(name, en_v, auto):
    if auto.numel() == 0:
        return
    err = float((en_v.double().reshape(auto.shape) - auto).abs().max())
    assert err <= 1e-11 * (1 + float(auto.abs().max())), (name, err)


@pytest.mark.parametrize("case", R.DISC_CASES, ids=_disc_ids)
def test_critic_gates(case):
    K, B, dense = case
    c = R.disc_case(B, K, dense)
    print(f"[gates] critic {_disc_ids(case)}: min |pre-activation| = {c['min_pre']:.3e}")
    assert c["min_pre"] >= R.DISC_MIN_PRE and c["signs"]
    x, lab, P, gout, gbar = c["x"], c["label"], c["params"], c["gout"], c["gbar"]
    tag = "critic " + _disc_ids(case)
    # forward
    want, en, lo = R.disc_forward_ref(x, lab, P), R.disc_forward_en(x, lab, P), R.disc_forward_en(x, lab, P, F32)
    _same("D", en.v, want)
    half(tag + " forward", lo.v, want, R.gate_of(en))
    # first order
    want = R.disc_backward_ref(x, lab, P, gout)
    en, lo = R.disc_backward_en(x, lab, P, gout), R.disc_backward_en(x, lab, P, gout, F32)
    for nm, w, e, l in zip(("dx", "dlabel"), want[:2], en[:2], lo[:2]):
        _same(nm, e.v, w)
        if w.numel():
            half(f"{tag} backward {nm}", l.v, w, R.gate_of(e))
    for i, (w, e, l) in enumerate(zip(want[2], en[2], lo[2])):
        _same(f"g{i}", e.v, w)
        half(f"{tag} backward param {i}", l.v.reshape(w.shape), w, R.gate_of(e).reshape(w.shape))
    # second order
    want = R.disc_backward_backward_ref(x, lab, P, gout, gbar)
    en, lo = R.disc_backward_backward_en(x, lab, P, gout, gbar), R.disc_backward_backward_en(x, lab, P, gout, gbar, F32)
    for nm, w, e, l in zip(("dx2", "dlabel2", "dgout"), want[:3], en[:3], lo[:3]):
        _same(nm, e.v, w)
        if w.numel():
            half(f"{tag} double backward {nm}", l.v.reshape(w.shape), w, R.gate_of(e).reshape(w.shape))
    for i, (w, e, l) in enumerate(zip(want[3], en[3], lo[3])):
        _same(f"gg{i}", e.v, w)
        half(f"{tag} double backward param {i}", l.v.reshape(w.shape), w, R.gate_of(e).reshape(w.shape))
    assert float(want[3][5].abs().max()) == 0.0
    # WGAN-GP
    args = (x, c["fv"], lab, c["alphas"], P, R.GP_WEIGHT)
    want, en, lo = R.disc_wgan_gp_ref(*args), R.disc_wgan_gp_en(*args), R.disc_wgan_gp_en(*args, dtype=F32)
    _same("losses", en[0].v, want[0])
    _same("dz", en[2].v, want[2])
    half(tag + " wgan losses", lo[0].v, want[0], R.gate_of(en[0]))
    half(tag + " wgan dz", lo[2].v, want[2], R.gate_of(en[2]))
    for i, (w, e, l) in enumerate(zip(want[1], en[1], lo[1])):
        if i < 5:
            _same(f"wg{i}", e.v, w)
            half(f"{tag} wgan param {i}", l.v.reshape(w.shape), w, R.gate_of(e).reshape(w.shape))
    assert float(en[1][5].v.abs().max()) == 0.0 and float(want[1][5].abs().max()) <= 1e-15


@pytest.mark.parametrize("defect", R.DISC_DEFECTS)
def test_critic_defects(defect):
    for K, B, dense in ((7, 6, True), (31, 257, True)):
        c = R.disc_case(B, K, dense)
        x, lab, P, gout, gbar = c["x"], c["label"], c["params"], c["gout"], c["gbar"]
        tag = f"critic defect {defect} K={K} B={B}"
        wargs = (x, c["fv"], lab, c["alphas"], P, R.GP_WEIGHT)
        good_w, bad_w = R.disc_wgan_gp_en(*wargs), R.disc_wgan_gp_en(*wargs, defect=defect)
        if defect in ("label_shift", "w1_pitch_odd"):
            g, b = R.disc_forward_en(x, lab, P), R.disc_forward_en(x, lab, P, defect=defect)
            bites(tag + " forward", g.v, b.v, R.gate_of(g))
            g, b = R.disc_backward_en(x, lab, P, gout), R.disc_backward_en(x, lab, P, gout, defect=defect)
            bites(tag + " backward dx", g[0].v, b[0].v, R.gate_of(g[0]))
            bites(tag + " backward dW1", g[2][0].v, b[2][0].v, R.gate_of(g[2][0]))
        if defect in ("elu_pp_wrong_side", "label_shift", "w1_pitch_odd"):
            g = R.disc_backward_backward_en(x, lab, P, gout, gbar)
            b = R.disc_backward_backward_en(x, lab, P, gout, gbar, defect=defect)
            bites(tag + " double backward dx2", g[0].v, b[0].v, R.gate_of(g[0]))
            bites(tag + " double backward dW2", g[3][2].v, b[3][2].v, R.gate_of(g[3][2]))
        if defect in ("dz_no_1_minus_alpha", "alpha_next_row", "elu_pp_wrong_side"):
            bites(tag + " wgan dz", good_w[2].v, bad_w[2].v, R.gate_of(good_w[2]))
        if defect in ("gp_outer_missing", "alpha_next_row"):
            bites(tag + " wgan dW1", good_w[1][0].v[:, :32], bad_w[1][0].v[:, :32], R.gate_of(good_w[1][0])[:, :32])
            bites(tag + " wgan dW2", good_w[1][2].v, bad_w[1][2].v, R.gate_of(good_w[1][2]))


# ====================================================================================================== scoring
def likelihood_f64(x, means):
    """the kernel's formulation in numpy float64, summed in order"""
    x, mu = x.numpy().astype(np.float64), means.numpy().astype(np.float64)
    D = x.shape[1]
    acc = np.zeros(x.shape[0])
    for k in range(mu.shape[0]):
        maha = np.zeros(x.shape[0])
        for d in range(D):
            diff = x[:, d] - mu[k, d]
            maha = maha + diff * diff
        acc = acc + np.exp(-0.5 * (D * R.LOG2PI + maha))
    return acc / mu.shape[0]


@pytest.mark.parametrize("case", R.LIK_CASES, ids=lambda s: "x".join(map(str, s)))
def test_joint_likelihood_gate(case):
    B, K, D = case
    x, means = R.likelihood_inputs(B, K, D)
    want, gate = R.joint_likelihood_ref(x, means)
    got = likelihood_f64(x, means)
    r = float((np.abs(got - want) / gate).max())
    print(f"[gates] joint_likelihood {case}: fp64 evaluation, worst |err| / gate = {r:.4f} (longdouble reference: {R.WIDE})")
    assert r <= 0.5
    other, _ = R.joint_likelihood_ref(x, means, wide=not R.WIDE)        # the reference's two arithmetics agree
    assert (np.abs(other - want) <= gate).all()
    tiny = np.finfo(np.float64).tiny
    if B >= 4:      # every class of result occurs (with K > 1 another centroid may be the nearer one: by class, not by row)
        assert (want == 0).any() and ((want > 0) & (want < tiny)).any() and (want > 1e-30).any() and \
            ((want > tiny) & (want < 1e-6)).any()
    if B >= 4 and K == 1:
        assert (want[3::4] == 0).all() and ((want[2::4] > 0) & (want[2::4] < tiny)).all() and (want[0::4] > 0.01).all()
    for defect in ("fp32_maha", "d_fixed_32", "no_1_over_k"):
        if (defect == "d_fixed_32" and D == 32) or (defect == "no_1_over_k" and K == 1) or B < 4:
            continue
        bad, _ = R.joint_likelihood_ref(x, means, defect=defect)
        # (a row that sits on its centroid has |x - mu|^2 = 0 in either precision, and a denormal result is a few hundred
        # units of 2^-1074, too coarse to show a relative 1e-5: the downgrade is judged where the result is normal)
        mask = torch.from_numpy((np.arange(B) % 4 != 0) & (want > 1e-290)) if defect == "fp32_maha" else None
        bites(f"joint_likelihood defect {defect} {case}", torch.from_numpy(want), torch.from_numpy(bad), torch.from_numpy(gate), mask)


def test_kvote_defects():
    thr = 0.5
    for k, (lik, preds) in R.kvote_exhaustive().items():
        want = R.kvote_ref(lik, preds, thr, k, 3)
        assert len(want) == 3 ** k * 2 ** k
        for defect in ("ge_threshold", "lt_half", "highest_on_ties"):
            bad = R.kvote_ref(lik, preds, thr, k, 3, defect=defect)
            n = int((bad != want).sum())
            print(f"[gates] k_vote defect {defect} k={k}: {n} of {len(want)} windows change")
            if defect == "lt_half":
                assert (n > 0) == (k % 2 == 0)
            elif defect == "highest_on_ties":
                assert (n > 0) == (k >= 2)
            else:
                assert n > 0


# ====================================================================================================== OR-CED
def _orced_gate_c(shape):
    return "x".join(map(str, shape))


@pytest.mark.parametrize("shape", R.ORCED_SHAPES, ids=_orced_gate_c)
def test_orced_gates(shape):
    c = R.orced_inputs(*shape)
    tag = f"orced {shape}"
    (logits, sup, mu, lv), _ = R.orced_fwd_ref(c)
    en, lo = R.orced_fwd_en(c), R.orced_fwd_en(c, F32)
    for nm, w, e, l in zip(("logits", "sup_fv", "mu", "logvar"), (logits, sup, mu, lv), en, lo):
        _same(nm, e.v, w.detach())
        half(f"{tag} fwd {nm}", l.v, w.detach(), R.gate_of(e))
    lv_in, sup_in = R.en_rounded(lv.detach()), R.en_rounded(sup.detach())
    lo_in = (R.EN(lv.detach().float()), R.EN(sup.detach().float()))
    for use in R.ORCED_USES:
        want = R.orced_bwd_ref(c, use)
        en, lo = R.orced_bwd_en(c, use, lv_in, sup_in), R.orced_bwd_en(c, use, *lo_in, dtype=F32)
        for k in en:
            _same(k, en[k].v, want[k])
            half(f"{tag} bwd {'+'.join(use)} {k}", lo[k].v, want[k], R.gate_of(en[k]))
    if shape[0] >= 2:
        use = R.ORCED_USES[-1]
        good = R.orced_bwd_en(c, use, lv_in, sup_in)
        for defect, keys in (("std_half_dropped", ("dWlv", "dblv", "dx4")), ("dmu_reads_dlv_row", ("dWmu", "dbmu")),
                             ("bias_last_row_missing", ("dbmu",))):
            bad = R.orced_bwd_en(c, use, lv_in, sup_in, defect=defect)
            for k in keys:
                bites(f"{tag} defect {defect} {k}", good[k].v, bad[k].v, R.gate_of(good[k]))


@pytest.mark.parametrize("shape", R.KL_SHAPES, ids=_orced_gate_c)
def test_orced_kl_gates(shape):
    mu, lv, mk = R.kl_inputs(*shape)
    want = R.kl_ref(mu, lv, mk, 0.7)
    en, lo = R.kl_en(mu, lv, mk, 0.7), R.kl_en(mu, lv, mk, 0.7, F32)
    for nm, w, e, l in zip(("loss", "d_mu", "d_logvar", "d_muk"), want, en, lo):
        _same(nm, e.v, w)
        half(f"orced_kl {shape} {nm}", l.v, w, R.gate_of(e))
