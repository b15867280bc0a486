"""Every branch of csrc/losses.hip, csrc/disc.hip, csrc/scoring.hip and csrc/orced.hip against fp64 (references, gates,
input conditions and cases: tests/critic_loss_ref.py; the gates themselves are shown reference-safe and
defect-sensitive by tests/test_critic_loss_gates_cpu.py).

Every comparison prints ``worst |err| / gate`` of its case (pytest -rP); the assertion is ``err <= gate``, elementwise.

    gap (branch of a launcher, or an input nothing exercised)           test
    ------------------------------------------------------------------  --------------------------------------------------
    chamfer: N = 1, C = 1, C = 8 (padded channels), N > 256 (norm loop  test_chamfer_shapes (one case per shape of
      trips), LDS tile 65 520 B (no attribute call), 65 600 B             critic_loss_ref.CHAMFER_SHAPES, strided preds and
      (hipFuncSetAttribute), N = 1920 (the limit), B != T with            gts, grad_scale -0.37, grad_per_b)
      grad_per_b
    chamfer: grad_scale 1 / -0.37 x grad_per_b absent / present,        test_chamfer_scales_and_want_grad
      want_grad False
    chamfer: non-contiguous dpreds through the raw entry point          test_chamfer_strided_dpreds_leaves_the_gaps_alone
    chamfer: duplicated ground truth; duplicated predictions and the    test_chamfer_duplicate_ground_truth,
      strict-< first-index rule                                           test_chamfer_duplicate_predictions
    chamfer: C = 9, N = 1921, shape mismatch, CPU tensor                test_chamfer_refusals
    cross_entropy: B > 256 (the r += 256 loop), K = 1, grad_scale,      test_cross_entropy (CE_CASES: B 1 .. 600, K 1 .. 64,
      each output alone, target None with preds, logits up to 80,         magnitude 4 and 80)
      all-equal rows, two equal maxima
    critic: K = 0 (wrapper and ABI), odd IN, IN = 64, B > 256           test_critic_forward_and_backward,
      (disc_loss_kernel's loop, disc_param_grad_kernel's unroll           test_critic_double_backward, test_critic_wgan_gp
      remainders), dense labels with dlabel, every nullable output        (DISC_CASES: K 0 .. 32, B 1 / 6 / 257)
      off in turn, dx_out / grads_out / losses_out, double backward
      on its own, db3 == 0.0
    critic: K = 33, wrong gout length, workspace one float short        test_critic_refusals
    joint_likelihood: B across the 128-thread block, D != 32, K = 1,    test_joint_likelihood
      denormal and exactly-zero results
    k_vote: every pattern for k 1 .. 4 (1296 windows), lik == thr,      test_kvote_exhaustive, test_kvote_classes_and_tail
      even k with half above, count ties, n_classes > n_labels,
      trailing partial window
    stream_score against an independent restatement, 150 windows of     test_stream_score_restated
      one stream in one tick (the i += 64 loop), groups across ticks,
      an absent stream
    orced heads: the declared limits, each upstream gradient alone,     test_orced_heads
      need_dx False, B L across 256
    orced_kl: B L 1 .. 5000, want_loss False, gscale None               test_orced_kl
    orced: K = 65, d_in = 1025, L = 129                                 test_orced_refusals
"""
import numpy as np
import pytest
import torch

import critic_loss_ref as R
from opensetgaitrecognition_pcaa_amd import _lib, inference, ops
from opensetgaitrecognition_pcaa_amd._lib import PcaaError

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32


def check(name, got, want, gate, mask=None):
    got = got.double().reshape(want.shape)
    gate = torch.as_tensor(gate, dtype=torch.float64, device=want.device).expand_as(want)
    assert bool(torch.isfinite(got).all()), (name, "non-finite output")
    err = (got - want).abs() / gate.clamp_min(1e-300)
    if mask is not None:
        err = torch.where(mask, err, torch.zeros_like(err))
    r = float(err.max()) if err.numel() else 0.0
    print(f"[critic_loss] {name}: worst |err| / gate = {r:.3f}")
    if not r <= 1.0:
        at = [int(i) for i in torch.unravel_index(err.argmax(), err.shape)]
        print(f"[critic_loss] {name}: worst at {at}; {int((err > 1.0).sum())} of {err.numel()} over the gate")
    assert r <= 1.0, (name, r)
    return r


def ids(v):
    return "x".join(str(int(x)) if not isinstance(x, str) else x for x in v) if isinstance(v, tuple) else str(v)


# ====================================================================================================== chamfer
def strided(x, order):
    """the same logical [B, C, T, N] tensor stored with its dimensions in ``order``"""
    inv = [order.index(i) for i in range(4)]
    return x.permute(*order).contiguous().permute(*inv)


def _chamfer(shape, dup=None, grad_scale=-0.37, per_b=True, tag=""):
    B, T, N, C = shape
    preds, gts = R.chamfer_inputs(B, T, N, C, DEV, dup=dup)
    gpb = R.chamfer_grad_per_b(B, DEV) if per_b else None
    ref = R.chamfer_ref(preds, gts, grad_scale, gpb)
    share = float(ref["unsettled"].double().mean())
    assert share <= R.CH_UNSETTLED_CAP, share
    pv, gv = strided(preds, (0, 2, 3, 1)), strided(gts, (3, 0, 1, 2))          # two different layouts, neither contiguous
    fl, dp = ops.chamfer(pv, gv, True, grad_scale, gpb)
    name = f"chamfer {shape}{tag} gs={grad_scale} per_b={per_b}"
    print(f"[critic_loss] {name}: unsettled prediction points {100 * share:.3f} %")
    check(name + " loss", fl, ref["loss"], ref["loss_gate"])
    return preds, gts, gpb, ref, fl, dp, name


@pytest.mark.parametrize("shape", R.CHAMFER_SHAPES, ids=ids)
def test_chamfer_shapes(shape):
    B, T, N, C = shape
    lds = (2 * N * 8 + 4 * N) * 4
    assert {819: 65520, 820: 65600, 1920: 150 * 1024}.get(N, lds) == lds
    *_, ref, fl, dp, name = _chamfer(shape)
    assert dp.is_contiguous() and tuple(dp.shape) == (B, C, T, N)
    check(name + " grad", dp, ref["grad"], ref["grad_gate"], R.settled_mask(ref))


@pytest.mark.parametrize("per_b", [False, True])
@pytest.mark.parametrize("grad_scale", [1.0, -0.37])
@pytest.mark.parametrize("shape", R.CHAMFER_SMALL, ids=ids)
def test_chamfer_scales_and_want_grad(shape, grad_scale, per_b):
    preds, gts, gpb, ref, fl, dp, name = _chamfer(shape, grad_scale=grad_scale, per_b=per_b)
    check(name + " grad", dp, ref["grad"], ref["grad_gate"], R.settled_mask(ref))
    fl2, none = ops.chamfer(preds, gts, False, grad_scale, gpb)               # contiguous this time, and no gradient
    assert none is None and torch.equal(fl2, fl)


@pytest.mark.parametrize("shape", [(3, 2, 128, 4), (2, 2, 129, 5)], ids=ids)
def test_chamfer_strided_dpreds_leaves_the_gaps_alone(shape):
    B, T, N, C = shape
    preds, gts = R.chamfer_inputs(B, T, N, C, DEV)
    gpb = R.chamfer_grad_per_b(B, DEV)
    ref = R.chamfer_ref(preds, gts, -0.37, gpb)
    big = torch.full((B, T + 1, C, 2 * N + 3), 12345.0, dtype=F32, device=DEV)
    view = big[:, :T, :, 1:1 + 2 * N:2].permute(0, 2, 1, 3)                  # logical [B, C, T, N], every stride unusual
    assert tuple(view.shape) == (B, C, T, N) and not view.is_contiguous()
    fl = torch.empty((B, T), dtype=F32, device=DEV)
    ps, gs, ds = preds.stride(), gts.stride(), view.stride()
    _lib.check(_lib.load().pcaa_chamfer_fwd_bwd(
        preds.data_ptr(), ps[0], ps[1], ps[2], ps[3], gts.data_ptr(), gs[0], gs[1], gs[2], gs[3], B, T, N, C,
        fl.data_ptr(), view.data_ptr(), ds[0], ds[1], ds[2], ds[3], -0.37, gpb.data_ptr(), ops._s()), "pcaa_chamfer_fwd_bwd")
    name = f"chamfer {shape} strided dpreds"
    check(name + " loss", fl, ref["loss"], ref["loss_gate"])
    check(name + " grad", view, ref["grad"], ref["grad_gate"], R.settled_mask(ref))
    written = torch.zeros_like(big, dtype=torch.bool)
    written[:, :T, :, 1:1 + 2 * N:2] = True
    assert bool((big[~written] == 12345.0).all()), "bytes between the elements of dpreds were written"


@pytest.mark.parametrize("shape", R.CHAMFER_SMALL[2:], ids=ids)
def test_chamfer_duplicate_ground_truth(shape):
    """a third of the ground-truth points repeat another: whichever the scan keeps, the gradient is the same -- in full"""
    *_, ref, fl, dp, name = _chamfer(shape, dup="gt", tag=" dup=gt")
    assert int((ref["margin_pred"] < float("inf")).sum()) > 0
    check(name + " grad", dp, ref["grad"], ref["grad_gate"], R.settled_mask(ref))


@pytest.mark.parametrize("shape", R.CHAMFER_SMALL[2:], ids=ids)
def test_chamfer_duplicate_predictions(shape):
    """a quarter of the predictions repeat another.  The gradient summed over a duplicate set does not depend on which
    member a ground-truth point chose; the member itself is the lowest index (strict <), which the reference follows"""
    *_, ref, fl, dp, name = _chamfer(shape, dup="pred", tag=" dup=pred")
    same = ref["same_pred"]
    assert int(same.sum()) > same.shape[0] * same.shape[1] * same.shape[2]
    set_ok = ~(same & ref["unsettled"].unsqueeze(2)).any(3)
    check(name + " grad summed over duplicate sets", R.duplicate_set_sums(dp, same), R.duplicate_set_sums(ref["grad"], same),
          R.duplicate_set_sums(ref["grad_gate"], same), set_ok.unsqueeze(1).expand_as(dp))
    check(name + " grad (lowest index of a set takes the term)", dp, ref["grad"], ref["grad_gate"], R.settled_mask(ref))


def test_chamfer_refusals():
    mk = lambda *s: torch.zeros(s, dtype=F32, device=DEV)
    with pytest.raises(PcaaError):
        ops.chamfer(mk(1, 9, 1, 4), mk(1, 9, 1, 4), True)
    with pytest.raises(PcaaError):
        ops.chamfer(mk(1, 2, 1, 1921), mk(1, 2, 1, 1921), False)
    with pytest.raises(ValueError):
        ops.chamfer(mk(1, 2, 1, 4), mk(1, 2, 1, 5), True)
    with pytest.raises(RuntimeError):
        ops.chamfer(torch.zeros(1, 2, 1, 4), mk(1, 2, 1, 4), True)
    torch.cuda.synchronize()


# ====================================================================================================== cross-entropy
@pytest.mark.parametrize("case", R.CE_CASES, ids=ids)
def test_cross_entropy(case):
    B, K, mag = case
    x, t = R.ce_inputs(B, K, mag, DEV)
    ref = R.ce_ref(x, t, -2.5)
    assert bool(((ref["gap"] == 0) | (ref["gap"] >= 1e-3)).all())
    name = f"cross_entropy {case}"
    loss, dl, pr = ops.cross_entropy(x, t, want_loss=True, want_grad=True, grad_scale=-2.5, want_preds=True)
    check(name + " loss", loss, ref["loss"], ref["loss_gate"])
    check(name + " grad", dl, ref["grad"], ref["grad_gate"])
    assert torch.equal(pr, ref["preds"]), name
    # each output alone gives the same bits, and nothing else
    l1, d1, p1 = ops.cross_entropy(x, t, want_loss=True)
    assert d1 is None and p1 is None and torch.equal(l1, loss)
    l2, d2, p2 = ops.cross_entropy(x, t, want_loss=False, want_grad=True, grad_scale=-2.5)
    assert l2 is None and p2 is None and torch.equal(d2, dl)
    l3, d3, p3 = ops.cross_entropy(x, t, want_loss=False, want_preds=True)
    assert l3 is None and d3 is None and torch.equal(p3, pr)
    l4, d4, p4 = ops.cross_entropy(x, None, want_loss=True, want_preds=True)       # no target: predictions only
    assert l4 is None and d4 is None and torch.equal(p4, pr)
    ref1 = R.ce_ref(x, t, 1.0)
    check(name + " grad (grad_scale 1)", ops.cross_entropy(x, t, want_loss=False, want_grad=True)[1], ref1["grad"], ref1["grad_gate"])


# ====================================================================================================== critic
def _disc_id(c):
    return f"K{c[0]}-B{c[1]}-{'dense' if c[2] else 'onehot'}"


def _case(case):
    K, B, dense = case
    c = R.disc_case(B, K, dense, DEV)
    assert c["min_pre"] >= R.DISC_MIN_PRE and c["signs"], c["min_pre"]
    return c, "critic " + _disc_id(case)


def _check_params(name, got, want, en):
    for i, (g, w, e) in enumerate(zip(got, want, en)):
        check(f"{name} param {i}", g, w.reshape(g.shape), R.gate_of(e).reshape(g.shape))


@pytest.mark.parametrize("case", R.DISC_CASES, ids=_disc_id)
def test_critic_forward_and_backward(case):
    c, name = _case(case)
    x, lab, P, gout = c["x"], c["label"], c["params"], c["gout"]
    B, K = lab.shape
    check(name + " forward", ops.disc_forward(x, lab, P), R.disc_forward_ref(x, lab, P), R.gate_of(R.disc_forward_en(x, lab, P)))
    want = R.disc_backward_ref(x, lab, P, gout)
    en = R.disc_backward_en(x, lab, P, gout)
    dx, dl, grads = ops.disc_backward(x, lab, P, gout, want_dlabel=True)
    check(name + " backward dx", dx, want[0], R.gate_of(en[0]))
    if K:
        check(name + " backward dlabel", dl, want[1], R.gate_of(en[1]))
    _check_params(name + " backward", grads, want[2], en[2])
    # every nullable output off in turn: the others keep their bits
    a = ops.disc_backward(x, lab, P, gout, want_dx=False, want_dlabel=True)
    assert a[0] is None and torch.equal(a[1], dl) and all(torch.equal(g, h) for g, h in zip(a[2], grads))
    a = ops.disc_backward(x, lab, P, gout, want_dlabel=False)
    assert a[1] is None and torch.equal(a[0], dx) and all(torch.equal(g, h) for g, h in zip(a[2], grads))
    a = ops.disc_backward(x, lab, P, gout, want_dlabel=True, want_params=False)
    assert a[2] is None and torch.equal(a[0], dx) and torch.equal(a[1], dl)
    dx_out = torch.full_like(x, 7.0)
    g_out = [torch.full_like(p, 7.0) for p in P]
    a = ops.disc_backward(x, lab, P, gout, grads_out=g_out, dx_out=dx_out)
    assert a[0] is dx_out and a[2] is g_out and torch.equal(dx_out, dx) and all(torch.equal(g, h) for g, h in zip(g_out, grads))


@pytest.mark.parametrize("case", R.DISC_CASES, ids=_disc_id)
def test_critic_double_backward(case):
    c, name = _case(case)
    x, lab, P, gout, gbar = c["x"], c["label"], c["params"], c["gout"], c["gbar"]
    B, K = lab.shape
    want = R.disc_backward_backward_ref(x, lab, P, gout, gbar)
    en = R.disc_backward_backward_en(x, lab, P, gout, gbar)
    dx2, dl2, dgo, grads = ops.disc_backward_backward(x, lab, P, gout, gbar, want_dlabel=True)
    check(name + " double backward dx2", dx2, want[0], R.gate_of(en[0]))
    if K:
        check(name + " double backward dlabel2", dl2, want[1], R.gate_of(en[1]))
    check(name + " double backward dgout", dgo, want[2], R.gate_of(en[2]).view(-1))
    _check_params(name + " double backward", grads[:5], want[3][:5], en[3][:5])
    assert float(grads[5].abs().max()) == 0.0, "b3 is not reached by the input gradient"
    same = lambda a, b: all((u is None and v is None) or torch.equal(u, v) for u, v in zip(a, b))
    full = (dx2, dl2, dgo) + tuple(grads)
    for off in ("want_dx", "want_dlabel", "want_dgout", "want_params"):
        kw = {"want_dlabel": True, off: False}
        a = ops.disc_backward_backward(x, lab, P, gout, gbar, **kw)
        got = a[:3] + (tuple(a[3]) if a[3] is not None else (None,) * 6)
        expect = list(full)
        for i in {"want_dx": [0], "want_dlabel": [1], "want_dgout": [2], "want_params": range(3, 9)}[off]:
            assert got[i] is None, (off, i)
            expect[i] = None
        assert same(got, expect), off


@pytest.mark.parametrize("case", R.DISC_CASES, ids=_disc_id)
def test_critic_wgan_gp(case):
    c, name = _case(case)
    args = (c["x"], c["fv"], c["label"], c["alphas"], c["params"], R.GP_WEIGHT)
    want, en = R.disc_wgan_gp_ref(*args), R.disc_wgan_gp_en(*args)
    losses, grads, dz = ops.disc_wgan_gp(*args, want_dz=True)
    check(name + " wgan losses", losses, want[0], R.gate_of(en[0]))
    check(name + " wgan dz", dz, want[2], R.gate_of(en[2]))
    _check_params(name + " wgan", grads[:5], want[1][:5], en[1][:5])
    assert float(grads[5].item()) == 0.0, "db3 = sum(+1/B) + sum(-1/B) must be exactly 0"
    l_out = torch.full((2,), 7.0, dtype=F32, device=DEV)
    g_out = [torch.full_like(p, 7.0) for p in c["params"]]
    a = ops.disc_wgan_gp(*args, grads_out=g_out, losses_out=l_out)            # no dz: two values come back
    assert len(a) == 2 and a[0] is l_out and a[1] is g_out
    assert torch.equal(l_out, losses) and all(torch.equal(g, h) for g, h in zip(g_out, grads))


def test_critic_refusals():
    c = R.disc_case(6, 4, False, DEV)
    x, lab, P, gout = c["x"], c["label"], c["params"], c["gout"]
    P33 = R.disc_params(33, DEV)
    lab33 = torch.zeros((6, 33), dtype=F32, device=DEV)
    with pytest.raises(PcaaError):
        ops.disc_forward(x, lab33, P33)
    with pytest.raises(PcaaError):
        ops.disc_backward(x, lab33, P33, gout)
    with pytest.raises(ValueError):
        ops.disc_backward(x, lab, P, gout[:5].contiguous())
    lib = _lib.load()
    ws = ops.disc_workspace(6, 4, DEV)
    grads = [torch.empty_like(p) for p in P]
    losses = torch.empty(2, dtype=F32, device=DEV)
    call = lambda nbytes: lib.pcaa_disc_wgan_gp(
        x.data_ptr(), c["fv"].data_ptr(), lab.data_ptr(), c["alphas"].data_ptr(), 6, 4, *[p.data_ptr() for p in P],
        R.GP_WEIGHT, losses.data_ptr(), *[g.data_ptr() for g in grads], None, ws.data_ptr(), nbytes, ops._s())
    assert call(ws.numel() * 4 - 4) != 0, "a workspace one float short must be refused"
    assert call(ws.numel() * 4) == 0
    short = lib.pcaa_disc_backward(x.data_ptr(), lab.data_ptr(), 6, 4, *[p.data_ptr() for p in P], gout.data_ptr(), None, None,
                                   *[g.data_ptr() for g in grads], ws.data_ptr(), 6 * 272 * 4 - 4, ops._s())
    assert short != 0
    torch.cuda.synchronize()


# ====================================================================================================== scoring
@pytest.mark.parametrize("case", R.LIK_CASES, ids=ids)
def test_joint_likelihood(case):
    B, K, D = case
    x, means = R.likelihood_inputs(B, K, D, DEV)
    want, gate = R.joint_likelihood_ref(x, means)
    got = inference.joint_likelihood(x, means).cpu().numpy()
    r = float((np.abs(got - want) / gate).max())
    print(f"[critic_loss] joint_likelihood {case}: worst |err| / gate = {r:.3f}")
    assert r <= 1.0, r
    if B >= 4:
        tiny = np.finfo(np.float64).tiny
        assert (want == 0).any() and ((want > 0) & (want < tiny)).any() and (want > tiny).any()
        assert (got[want == 0] <= gate[want == 0]).all()


def test_kvote_exhaustive():
    thr = 0.5
    for k, (lik, preds) in R.kvote_exhaustive().items():
        want = R.kvote_ref(lik, preds, thr, k, 3)
        assert (lik == thr).any() and len(want) == 6 ** k
        got = inference.k_vote(torch.from_numpy(lik).to(DEV), torch.from_numpy(preds).to(DEV), thr, k, 3)
        bad = int((got.cpu().numpy() != want).sum())
        print(f"[critic_loss] k_vote k={k}: {len(want)} windows, {bad} differ")
        assert bad == 0


def test_kvote_classes_and_tail():
    lik, preds = R.kvote_exhaustive(ks=(3,))[3]
    lik, preds = np.concatenate([lik, [9.0, 9.0]]), np.concatenate([preds, [2, 2]])       # a trailing partial window
    want = R.kvote_ref(lik, preds, 0.5, 3, 2)                                              # 2 labels, 3 encoder classes
    got = inference.k_vote(torch.from_numpy(lik).to(DEV), torch.from_numpy(preds).to(DEV), 0.5, 3, 2, n_classes=3)
    assert got.shape[0] == 6 ** 3 and np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("k", [1, 3, 7])
def test_stream_score_restated(k):
    K, D, n_slots, ring = 4, 32, 4, 256
    per_tick = {0: [150, 0, 5, 2 * k + 1], 1: [2, k + 1, 3, k], 3: [0, 1, 64 + k, 1]}      # slot 2 never appears
    n_win = {s: sum(c) for s, c in per_tick.items()}
    means = R.uniform(K * D, 40, DEV, -2.0, 2.0).view(K, D).float()
    logits, fvs = {}, {}
    for s, n in n_win.items():
        logits[s] = R.ce_inputs(n, K, 4.0, DEV)[0]
        fvs[s] = (means[torch.arange(n, device=DEV) % K].double() +
                  R.uniform(n * D, 50 + s, DEV, -1.3, 1.3).view(n, D)).float().contiguous()
    all_lik = np.sort(np.concatenate([R.joint_likelihood_ref(fvs[s], means)[0] for s in n_win]))
    thr = float(0.5 * (all_lik[len(all_lik) // 2 - 1] + all_lik[len(all_lik) // 2]))
    ref = {s: R.stream_ref(logits[s], fvs[s], means, thr, k, K) for s in n_win}
    for s in n_win:      # the condition on the inputs: no likelihood within its gate of the threshold
        assert (np.abs(ref[s][1] - thr) > 2 * ref[s][2]).all()
    assert any((v[3] == K).any() for v in ref.values()) and any((v[3] != K).any() for v in ref.values())
    hist_lik = torch.full((n_slots, k), float("nan"), dtype=torch.float64, device=DEV)
    hist_pred = torch.full((n_slots, k), -7, dtype=torch.int64, device=DEV)
    nf, nw = np.zeros(n_slots, np.int64), np.zeros(n_slots, np.int64)
    got = {s: ([], [], {}) for s in n_win}
    for tick in range(4):
        order = [3, 0, 1] if tick % 2 else [1, 3, 0]
        counts = [per_tick[s][tick] for s in order]
        plan = inference.plan_tick(nf, nw, order, counts, 1, 1, k, ring, 1)      # T = hop = 1: one window per frame
        lg = torch.cat([logits[s][nw[s]:nw[s] + c] for s, c in zip(order, counts)]).contiguous()
        fv = torch.cat([fvs[s][nw[s]:nw[s] + c] for s, c in zip(order, counts)]).contiguous()
        nf[order], nw[order] = plan.n_frames, plan.n_windows
        preds, lik, votes = ops.stream_score(
            lg, fv, means, *(torch.from_numpy(a).to(DEV) for a in (plan.run_start, plan.win_stream, plan.win_j, plan.vote_pos)),
            plan.vote_group.size, thr, k, K, K, hist_lik, hist_pred)
        for s in n_win:
            m = torch.from_numpy(plan.win_stream == s).to(DEV)
            got[s][0].append(preds[m])
            got[s][1].append(lik[m])
        for v, s, g in zip(votes.tolist(), plan.vote_stream.tolist(), plan.vote_group.tolist()):
            assert g not in got[s][2]
            got[s][2][g] = v
    for s in n_win:
        rp, rl, rg, rv = ref[s]
        assert np.array_equal(torch.cat(got[s][0]).cpu().numpy(), rp), s
        r = float((np.abs(torch.cat(got[s][1]).cpu().numpy() - rl) / rg).max())
        print(f"[critic_loss] stream_score k={k} stream {s} ({n_win[s]} windows) lik: worst |err| / gate = {r:.3f}")
        assert r <= 1.0
        assert [got[s][2].get(g) for g in range(n_win[s] // k)] == rv.tolist(), s
    assert torch.isnan(hist_lik[2]).all() and bool((hist_pred[2] == -7).all()), "a stream that is in no tick keeps its history"


# ====================================================================================================== OR-CED
@pytest.mark.parametrize("shape", R.ORCED_SHAPES, ids=ids)
def test_orced_heads(shape):
    B, K, d_in, L = shape
    c = R.orced_inputs(B, K, d_in, L, DEV)
    name = f"orced {shape}"
    (logits, sup, mu, lv), _ = R.orced_fwd_ref(c)
    en = R.orced_fwd_en(c)
    got = ops.orced_heads_fwd(c["x4"], c["Wmu"], c["bmu"], c["Wlv"], c["blv"], c["eps"], c["Wc"], c["bc"])
    for nm, g, w, e in zip(("logits", "sup_fv", "mu", "logvar"), got, (logits, sup, mu, lv), en):
        check(f"{name} fwd {nm}", g, w.detach(), R.gate_of(e))
    lv32, sup32 = lv.detach().float().contiguous(), sup.detach().float().contiguous()
    lv_in, sup_in = R.en_rounded(lv.detach()), R.en_rounded(sup.detach())
    keys = ("dx4", "dWmu", "dbmu", "dWlv", "dblv", "dWc", "dbc")
    for use in R.ORCED_USES:
        want, en = R.orced_bwd_ref(c, use), R.orced_bwd_en(c, use, lv_in, sup_in)
        ups = [c[k] if k in use else None for k in ("d_logits", "d_sup", "d_mu", "d_logvar")]
        out = ops.orced_heads_bwd(c["x4"], c["eps"], lv32, sup32, c["Wmu"], c["Wlv"], c["Wc"], *ups)
        for k, g in zip(keys, out):
            check(f"{name} bwd {'+'.join(use)} {k}", g, want[k], R.gate_of(en[k]))
        nodx = ops.orced_heads_bwd(c["x4"], c["eps"], lv32, sup32, c["Wmu"], c["Wlv"], c["Wc"], *ups, need_dx=False)
        assert nodx[0] is None and all(torch.equal(a, b) for a, b in zip(nodx[1:], out[1:]))


@pytest.mark.parametrize("shape", R.KL_SHAPES, ids=ids)
def test_orced_kl(shape):
    mu, lv, mk = R.kl_inputs(*shape, DEV)
    want, en = R.kl_ref(mu, lv, mk, 0.7), R.kl_en(mu, lv, mk, 0.7)
    loss, grads = ops.orced_kl(mu, lv, mk, gscale=0.7)
    name = f"orced_kl {shape}"
    check(name + " loss", loss, want[0], R.gate_of(en[0]))
    for nm, g, w, e in zip(("d_mu", "d_logvar", "d_muk"), grads, want[1:], en[1:]):
        check(f"{name} {nm}", g, w, R.gate_of(e))
    l2, g2 = ops.orced_kl(mu, lv, mk, want_loss=False, gscale=0.7)
    assert l2 is None and all(torch.equal(a, b) for a, b in zip(g2, grads))
    l3, g3 = ops.orced_kl(mu, lv, mk)
    assert g3 == (None, None, None) and torch.equal(l3, loss)


@pytest.mark.parametrize("shape", [(2, 65, 8, 4), (2, 3, 1025, 4), (2, 3, 8, 129)], ids=ids)
def test_orced_refusals(shape):
    B, K, d_in, L = shape
    c = R.orced_inputs(B, K, d_in, L, DEV)
    assert _lib.load().pcaa_orced_heads_supported(B, K, d_in, L) == 0
    with pytest.raises(ValueError):
        ops.orced_heads_fwd(c["x4"], c["Wmu"], c["bmu"], c["Wlv"], c["blv"], c["eps"], c["Wc"], c["bc"])
    z = torch.zeros((B, L), dtype=F32, device=DEV)
    with pytest.raises(PcaaError):
        ops.orced_heads_bwd(c["x4"], c["eps"], z, z, c["Wmu"], c["Wlv"], c["Wc"], c["d_logits"], None, None, None)
    torch.cuda.synchronize()
