"""The drop-in modules in ``.eval()`` under autograd: BatchNorm is the fixed affine map of its running statistics, and
CGEncoder, ORCEDEncoder's trunk, PointNetBlock, TemporalConvolutionBlock / DilTempConv1d and GaussianMeanLearner are
differentiated as such on the HIP path (functional._bn_layer_backward's eval branch; csrc/elementwise.hip
pcaa_bn_eval_act_bwd).  Reference: the fp64 oracle's autograd (oracle/pcaa_oracle.py, ``training=False``) and, at two
shapes, the reference's own eval-mode gradients (tests/golden/eval_bwd_*.npz).

Gates (fp32 mode): outputs 1e-4 of scale; every parameter gradient 3e-4 of the tensor's scale -- the train-mode gate of
tests/test_hip_modules.py, here for EVERY parameter: the biases in front of the BatchNorms have real gradients in eval
mode and are compared like any other tensor; dx 2e-4 in relative l2.  No BatchNorm buffer may change by a bit.
"""
import numpy as np
import pytest
import torch

from helpers import T, check_against_record, load_golden, make_encoder
from opensetgaitrecognition_pcaa_amd import constants, functional as F_hip, models, synthetic as syn
from opensetgaitrecognition_pcaa_amd.adapt import finetune_frozen_bn
from oracle import pcaa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL, GTOL, DXTOL = 1e-4, 3e-4, 2e-4


def _close(a, ref, tol=TOL, floor=1e-6, what=""):
    a = a.detach().float().cpu().double()
    ref = torch.as_tensor(ref).detach().cpu().double()
    err = (a - ref).abs().max().item()
    den = max(ref.abs().max().item(), floor)
    assert err <= tol * den, f"{what}: abs err {err:.3e}, scale {den:.3e}, rel {err / den:.3e}"


def _rel_l2(a, ref):
    a, ref = a.detach().float().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    return float((a - ref).norm() / (ref.norm() + 1e-300))


def oracle_sd(module):
    """fp64 CPU copy of the state_dict for the oracle; its parameters require grad.  -> (sd, parameter names)"""
    sd = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()).clone()
          for k, v in module.state_dict().items()}
    names = [n for n, _ in module.named_parameters()]
    for n in names:
        sd[n].requires_grad_(True)
    return sd, names


def buffers_of(module):
    return {k: v.detach().clone() for k, v in module.named_buffers()}


def assert_buffers_unchanged(module, before):
    for k, v in module.named_buffers():
        assert torch.equal(v, before[k]), f"{k} changed in eval mode"


def check_grads(module, names, ref_grads, what):
    got = dict(module.named_parameters())
    for n, r in zip(names, ref_grads):
        assert got[n].grad is not None, f"{what}: {n} got no gradient"
        _close(got[n].grad, r, GTOL, what=f"{what}: d{n}")


def probe(B, K):
    """the probe loss of tests/golden/make_golden.py: (logits * r1).sum() + (sup_fv * r2).sum()"""
    rng = np.random.default_rng(77)
    return (torch.from_numpy(rng.standard_normal((B, K)).astype(np.float32)),
            torch.from_numpy(rng.standard_normal((B, 32)).astype(np.float32)))


def oracle_encoder_grads(sd, names, head, xpm, r1, r2, training=False):
    xr = xpm.permute(0, 3, 1, 2).double().requires_grad_(True)
    oc, fv = O.cg_encoder_forward(xr, sd, head, training=training, update_stats=False)
    loss = (oc * r1.double()).sum() + (fv * r2.double()).sum()
    grads = torch.autograd.grad(loss, [xr] + [sd[n] for n in names])
    return oc.detach(), fv.detach(), grads[0], dict(zip(names, grads[1:]))


# ------------------------------------------------------------------------------------------------ CGEncoder
@pytest.mark.parametrize("B,N,C,K,head,tag", [(2, 32, 4, 4, True, "eval_bwd_B2_N32_C4_K4"),
                                              (3, 150, 4, 6, False, "eval_bwd_B3_N150_C4_K6_nohead"),
                                              (2, 32, 5, 8, True, None)])
def test_cg_encoder_eval_backward(B, N, C, K, head, tag):
    F_hip.set_precision("fp32")
    enc = make_encoder(K, N, C, head, seed=0)
    sd, names = oracle_sd(enc)
    enc = enc.to(DEV).eval()
    before = buffers_of(enc)
    xpm = syn.synthetic_pcs(B, T, N, C, seed=1234)
    r1, r2 = probe(B, K)
    x = xpm.to(DEV).permute(0, 3, 1, 2)
    xg = x.detach().clone().requires_grad_(True)
    oc, fv = enc(xg)
    loss = (oc * r1.to(DEV)).sum() + (fv * r2.to(DEV)).sum()
    loss.backward()
    assert_buffers_unchanged(enc, before)
    assert not enc.training

    ref_oc, ref_fv, ref_dx, ref_g = oracle_encoder_grads(sd, names, head, xpm, r1, r2)
    _close(oc, ref_oc, what="out_classes")
    _close(fv, ref_fv, what="sup_fv")
    check_grads(enc, names, [ref_g[n] for n in names], "CGEncoder vs oracle")
    assert _rel_l2(xg.grad, ref_dx) <= DXTOL, f"dx rel-l2 {_rel_l2(xg.grad, ref_dx):.3e}"
    pre_bn = [n for n in names if n.endswith("module.0.bias") or n.endswith("conv1d.bias")]
    assert len(pre_bn) == 10
    wmax = max(float(ref_g[n].abs().max()) for n in names if ref_g[n].dim() > 1)
    assert all(float(dict(enc.named_parameters())[n].grad.abs().max()) > 1e-3 * wmax for n in pre_bn), \
        "the biases in front of the BatchNorms have real gradients in eval mode"

    # the with-grad forward (y and col stored) against the no-grad forward (today's route): two routes whose small
    # head GEMMs differ in their split-K atomics' order at most
    with torch.no_grad():
        oc0, fv0 = enc(x)
    _close(oc, oc0, 1e-5, what="with-grad vs no-grad out_classes")
    _close(fv, fv0, 1e-5, what="with-grad vs no-grad sup_fv")

    if tag is not None:          # the reference's own eval-mode gradients
        g, _ = load_golden(tag)
        _close(oc, g["out_classes"], what="golden out_classes")
        _close(fv, g["sup_fv"], what="golden sup_fv")
        assert abs(loss.item() - float(g["loss"])) <= TOL * abs(float(g["loss"])) + 1e-5
        for name, p in enc.named_parameters():
            check_against_record(g, "grad.", name, p.grad, GTOL)
        l2 = float(g["dx_l2"])
        assert abs(xg.grad.double().norm().item() - l2) <= DXTOL * l2
        smp = syn.checksum(xg.grad, 64)["samples"]
        assert np.abs(smp - g["dx_samples"]).max() <= DXTOL * max(np.abs(g["dx_samples"]).max(), l2 / np.sqrt(xg.grad.numel())) * 4


def test_encoder_backward_eval_writes_into_gout():
    """encoder_backward(..., gout=...) on an eval-mode state: the same values in pre-zeroed views, the ten pre-BN biases
    included, need_dx honoured; and a no-grad eval state is refused with a message instead of failing deep inside."""
    F_hip.set_precision("fp32")
    B, N, C, K = 2, 32, 4, 4
    enc = make_encoder(K, N, C, True, seed=0).to(DEV).eval()
    before = buffers_of(enc)
    x = syn.synthetic_pcs(B, T, N, C, seed=1234).to(DEV).permute(0, 3, 1, 2)
    r1, r2 = (t.to(DEV) for t in probe(B, K))
    with torch.no_grad():
        _, _, st = F_hip.encoder_forward(enc, x, False, want_bwd=True)
        g_ref, dx_ref = F_hip.encoder_backward(enc, st, r1.clone(), r2.clone(), need_dx=True)
        _, _, st = F_hip.encoder_forward(enc, x, False, want_bwd=True)
        params = dict(enc.named_parameters())
        flat = torch.zeros(sum(p.numel() for p in params.values()), device=DEV)
        gout, off = {}, 0
        for n, p in params.items():
            gout[n] = flat[off:off + p.numel()].view_as(p)
            off += p.numel()
        g, dx = F_hip.encoder_backward(enc, st, r1.clone(), r2.clone(), need_dx=False, gout=gout)
        assert dx is None and dx_ref is not None
        for n in params:
            assert g[n].data_ptr() == gout[n].data_ptr(), f"{n}: not written into gout"
            _close(gout[n], g_ref[n], 1e-5, what=f"gout {n}")
            assert float(gout[n].abs().max()) > 0.0, n
        _, _, st0 = F_hip.encoder_forward(enc, x, False)
        with pytest.raises(RuntimeError, match="want_bwd"):
            F_hip.encoder_backward(enc, st0, r1, r2)
    assert_buffers_unchanged(enc, before)


# ------------------------------------------------------------------------------------------------ the blocks
def _block_case(module, x_cpu, oracle_fn, what, r_seed=5):
    F_hip.set_precision("fp32")
    sd, names = oracle_sd(module)
    module = module.to(DEV).eval()
    before = buffers_of(module)
    xg = x_cpu.to(DEV).requires_grad_(True)
    out = module(xg)
    r = torch.randn(out.shape, generator=torch.Generator().manual_seed(r_seed))
    (out * r.to(DEV)).sum().backward()
    xr = x_cpu.double().requires_grad_(True)
    ref = oracle_fn(xr, sd)
    grads = torch.autograd.grad((ref * r.double()).sum(), [xr] + [sd[n] for n in names])
    _close(out, ref, what=f"{what}: forward")
    check_grads(module, names, grads[1:], what)
    assert _rel_l2(xg.grad, grads[0]) <= DXTOL, f"{what}: dx rel-l2 {_rel_l2(xg.grad, grads[0]):.3e}"
    assert_buffers_unchanged(module, before)


def test_pointnet_block_eval_backward():
    constants.NFEATURES = 4
    m = syn.deterministic_fill_(models.PointNetBlock().float(), 3)
    x = syn.synthetic_pcs(2, T, 32, 4, seed=8).permute(0, 3, 1, 2).contiguous()
    _block_case(m, x, lambda xr, sd: O.pointnet_block(xr, sd, "", False), "PointNetBlock")


def test_temporal_block_eval_backward():
    m = syn.deterministic_fill_(models.TemporalConvolutionBlock().float(), 4)
    x = torch.randn(2, constants.POINTNET_OUT_DIM, T, generator=torch.Generator().manual_seed(9)) * 0.5
    _block_case(m, x, lambda xr, sd: O.temporal_block(xr, sd, "", False), "TemporalConvolutionBlock")


def test_dil_temp_conv1d_eval_backward():
    m = syn.deterministic_fill_(models.DilTempConv1d(8, 16, 2).float(), 7)
    x = torch.randn(2, 8, T, generator=torch.Generator().manual_seed(10))
    _block_case(m, x, lambda xr, sd: O.dil_temp_conv1d(xr, sd, "", 2, training=False), "DilTempConv1d(8, 16, d=2)")


def test_gaussian_mean_learner_eval_backward():
    K = 4
    m = syn.deterministic_fill_(models.GaussianMeanLearner(K).float(), 3)
    _block_case(m, torch.eye(K), lambda xr, sd: O.gaussian_mean_learner_forward(xr, sd, training=False),
                "GaussianMeanLearner")


def test_orced_trunk_eval_backward():
    F_hip.set_precision("fp32")
    B, N, C, K = 2, 32, 4, 4
    constants.NFEATURES = C
    enc = syn.deterministic_fill_(models.ORCEDEncoder(K, nmax_points=N).float(), 2)
    sd, _ = oracle_sd(enc)
    names = [n for n in sd if (n.startswith("pc_block.") or n.startswith("tc_block.")) and sd[n].requires_grad]
    enc = enc.to(DEV).eval()
    before = buffers_of(enc)
    xpm = syn.synthetic_pcs(B, T, N, C, seed=12)
    x4 = F_hip.encoder_trunk(enc, xpm.to(DEV).permute(0, 3, 1, 2))
    r = torch.randn(x4.shape, generator=torch.Generator().manual_seed(6))
    (x4 * r.to(DEV)).sum().backward()
    xr = xpm.permute(0, 3, 1, 2).double()
    ref = O.temporal_block(O.pointnet_block(xr, sd, "pc_block.", False).mean(3), sd, "tc_block.", False).mean(2)
    grads = torch.autograd.grad((ref * r.double()).sum(), [sd[n] for n in names])
    _close(x4, ref, what="ORCEDEncoder trunk: forward")
    check_grads(enc, names, grads, "ORCEDEncoder trunk")
    assert_buffers_unchanged(enc, before)
    # and the whole module in eval mode under autograd (its heads follow the trunk): runs, every parameter gets a gradient
    enc.zero_grad()
    out = enc(xpm.to(DEV).permute(0, 3, 1, 2))
    (out[0].sum() + out[1].sum()).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in enc.parameters())
    assert_buffers_unchanged(enc, before)


# ------------------------------------------------------------------------------------------------ bf16 mode
def test_cg_encoder_eval_backward_bf16_mode():
    """bf16 mode: the with-grad eval forward takes the y-storing route (no fused-epilogue layers) and its embedding is
    within the project's 5e-2 of the oracle's scale (tests/test_round3_parity.py).  For the gradients no project number
    exists, so the yardstick is measured here: the TRAIN-mode bf16 backward of the same encoder and input against the
    fp64 oracle's train-mode autograd, relative l2 per weight tensor.  Every eval-mode gradient tensor must be within
    2 x the largest of those: eval mode does strictly less arithmetic on the same operands; the factor covers one route
    storing y where the other keeps it in an epilogue.  Both columns are printed (profiles/eval_backward.txt)."""
    B, N, C, K = 2, 128, 4, 8
    enc = make_encoder(K, N, C, True, seed=0)
    sd, names = oracle_sd(enc)
    enc = enc.to(DEV).eval()
    before = buffers_of(enc)
    xpm = syn.synthetic_pcs(B, T, N, C, seed=1234)
    r1, r2 = probe(B, K)
    x = xpm.to(DEV).permute(0, 3, 1, 2)
    with torch.no_grad():
        oc, fv, st = F_hip.encoder_forward(enc, x, False, "bf16", want_bwd=True)
        assert all(s.y is not None for s in st.pn[1:]) and all(s.col is not None for s in st.dtc), "the y-storing route"
        assert st.pn[1].y.dtype == torch.bfloat16
        g_eval, _ = F_hip.encoder_backward(enc, st, r1.to(DEV), r2.to(DEV))
    assert_buffers_unchanged(enc, before)
    ref_oc, ref_fv, _, ref_eval = oracle_encoder_grads(sd, names, True, xpm, r1, r2, training=False)
    scale = ref_fv.abs().max().item()
    emb = (fv.cpu().double() - ref_fv).abs().max().item() / scale
    print(f"[eval-bwd bf16] embedding err {emb:.2e} of scale")
    assert emb <= 5e-2

    enc.train()
    with torch.no_grad():
        _, _, st = F_hip.encoder_forward(enc, x, True, "bf16")
        g_train, _ = F_hip.encoder_backward(enc, st, r1.to(DEV), r2.to(DEV))
    _, _, _, ref_train = oracle_encoder_grads(sd, names, True, xpm, r1, r2, training=True)
    train_col = {n: _rel_l2(g_train[n], ref_train[n]) for n in names if n.endswith(".weight")}
    eval_col = {n: _rel_l2(g_eval[n], ref_eval[n]) for n in names}
    bound = 2.0 * max(train_col.values())
    print(f"[eval-bwd bf16] relative-l2 error of the gradients vs the fp64 oracle, B={B} N={N} C={C} K={K}")
    print(f"[eval-bwd bf16] {'tensor':44s} {'eval':>10s} {'train':>10s}")
    for n in names:
        tr = f"{train_col[n]:10.3e}" if n in train_col else f"{'-':>10s}"
        print(f"[eval-bwd bf16] {n:44s} {eval_col[n]:10.3e} {tr}")
    print(f"[eval-bwd bf16] largest train-mode error {max(train_col.values()):.3e} -> bound {bound:.3e}; "
          f"largest eval-mode error {max(eval_col.values()):.3e}")
    for n in names:
        assert eval_col[n] <= bound, f"{n}: eval-mode rel-l2 {eval_col[n]:.3e} above 2 x train-mode worst {bound:.3e}"


# ------------------------------------------------------------------------------------------------ the helper
@pytest.mark.parametrize("which", ["heads", "all"])
def test_finetune_frozen_bn_vs_oracle(which):
    F_hip.set_precision("fp32")
    B, N, C, K, steps, lr = 4, 32, 4, 4, 3, 1e-4          # (at 1e-3 the all-parameter loop overshoots at its third step)
    enc = make_encoder(K, N, C, True, seed=0)
    sd, names = oracle_sd(enc)
    enc = enc.to(DEV).train()
    before = buffers_of(enc)
    start = {n: p.detach().clone() for n, p in enc.named_parameters()}
    xpm = syn.synthetic_pcs(B, T, N, C, seed=31)
    labels = syn.synthetic_labels(B, K, seed=32)
    losses = finetune_frozen_bn(enc, xpm.to(DEV).permute(0, 3, 1, 2), labels.to(DEV), steps, lr, params=which)
    assert enc.training, "the mode it found is restored"
    assert all(p.requires_grad for p in enc.parameters())
    assert_buffers_unchanged(enc, before)
    assert len(losses) == steps and all(isinstance(l, float) for l in losses)

    # the same loop in the fp64 oracle: its cross_entropy and adam_step (torch.optim.Adam's defaults)
    chosen = [n for n in names if which == "all" or n.split(".")[0] in ("MLP_sup1", "MLP_head", "MLP_sup2")]
    xr = xpm.permute(0, 3, 1, 2).double()
    state, ref = {}, []
    for _ in range(steps):
        logits, _ = O.cg_encoder_forward(xr, sd, True, training=False)
        loss = O.cross_entropy(logits, labels)
        grads = torch.autograd.grad(loss, [sd[n] for n in chosen])
        with torch.no_grad():
            O.adam_step({n: sd[n] for n in chosen}, {n: g for n, g in zip(chosen, grads)}, state, lr, 0.9, 0.999)
        ref.append(float(loss.detach()))
    print(f"[finetune {which}] losses {losses} oracle {ref}")
    assert ref[-1] < ref[0], "the oracle's loop itself must descend"
    for s in range(steps):
        tol = TOL if s == 0 else 5e-4 * s          # the trajectory gate of test_v4_train_steps_vs_golden
        assert np.allclose(losses[s], ref[s], rtol=tol, atol=1e-5), (s, losses, ref)
    moved = 0
    for n, p in enc.named_parameters():
        if n in chosen:
            moved += int(not torch.equal(p, start[n]))
        else:
            assert torch.equal(p, start[n]), f"{n}: a trunk parameter changed under params='heads'"
    assert moved == len(chosen)
    with pytest.raises(ValueError):
        finetune_frozen_bn(enc, xpm.to(DEV).permute(0, 3, 1, 2), labels.to(DEV), 1, lr, params="trunk")
