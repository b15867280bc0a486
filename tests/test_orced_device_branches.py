"""pcaa_orced_triplet and pcaa_orced_ood (csrc/orced.hip) on the GPU against the fp64 references of
tests/orced_device_ref.py, inside its gates; the autograd route of ``orced_losses(triplet="hip")`` against
``triplet="aten"``; ``ORCEDScorer`` against the host rule.

    triplet: nothing to mine (one class; singletons only; far apart)      test_triplet_nothing_mined
    triplet: the shapes of the table (B across a wave and across 256
             threads, L at its bound, an anchor without a positive)         test_triplet_shapes
    triplet: a duplicated row (D == 0), gscale != 1, repeatability          test_triplet_duplicate_row, _gscale, _bit_identical
    triplet: B = 1025, L = 129 refused by the wrapper                       test_triplet_refusals
    autograd: orced_losses hip vs aten on the golden's step inputs          test_orced_losses_hip_vs_aten
    ood: (n, K, L) of the table, the golden block, each test alone          test_ood_shapes, test_ood_golden_block, test_ood_each_test_alone
    scorer: fit + score / decide vs ORCED_ensemble_ood_detection            test_scorer_golden_block, test_scorer_fit_and_score_vs_host_rule
"""
import numpy as np
import pytest
import torch

import orced_device_ref as R
from helpers import load_golden
from opensetgaitrecognition_pcaa_amd import constants, models, orced, synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
G, META = load_golden("orced")
ids = lambda s: "x".join(map(str, s))
_cache = {}


def _ops():
    from opensetgaitrecognition_pcaa_amd import ops
    return ops


def triplet_case(shape, kind="clustered"):
    """inputs and the fp64 reference of a case (on the CPU, once; shared and never modified)"""
    if (shape, kind) not in _cache:
        x, lab = R.triplet_inputs(*shape, kind=kind)
        d = R.triplet_dense(x, lab)
        _cache[(shape, kind)] = (x, lab, R.triplet_ref(x, lab), d, R.triplet_gates(d))
    return _cache[(shape, kind)]


def check_triplet(name, x, lab, want_loss, want_dx, gates, gscale=1.0):
    loss, dx = _ops().orced_triplet(x.to(DEV), lab.to(DEV), R.EPSILON, R.MARGIN, gscale=gscale)
    loss, dx = loss.cpu().double(), dx.cpu().double()
    rl = abs(float(loss - want_loss)) / max(float(gates["loss"]), 1e-300)
    rd = R.ratio(dx, want_dx, gates["dx"] * abs(R.f32(gscale)))
    print(f"{name}: loss {float(loss):.8g} (want {float(want_loss):.8g}) ratio {rl:.3f}; dx ratio {rd:.3f}")
    assert torch.isfinite(dx).all()
    assert rl <= 1.0 and rd <= 1.0, (name, rl, rd)
    return loss, dx


@pytest.mark.parametrize("shape", R.TRIPLET_EMPTY + ((4, 2, 2),), ids=ids)
def test_triplet_nothing_mined(shape):
    kind = "far" if shape == (4, 2, 2) else "clustered"
    x, lab, (want, want_dx, n_pos, n_neg), d, _ = triplet_case(shape, kind)
    assert d["count"] == 0 and float(want) == 0.0
    loss, dx = _ops().orced_triplet(x.to(DEV), lab.to(DEV), R.EPSILON, R.MARGIN, gscale=1.0)
    assert float(loss) == 0.0 and torch.equal(dx.cpu(), torch.zeros_like(x))
    loss_only, none = _ops().orced_triplet(x.to(DEV), lab.to(DEV), R.EPSILON, R.MARGIN)
    assert none is None and float(loss_only) == 0.0


@pytest.mark.parametrize("shape", R.TRIPLET_SHAPES, ids=ids)
def test_triplet_shapes(shape):
    x, lab, (want, want_dx, _, _), d, g = triplet_case(shape)
    assert d["count"] > 0 and g["mining"] > 1.0 and g["hinge"] > 1.0
    check_triplet(f"triplet {shape}", x, lab, want, want_dx, g)
    loss_only, none = _ops().orced_triplet(x.to(DEV), lab.to(DEV), R.EPSILON, R.MARGIN)          # dx = NULL: one-workgroup launch 3
    assert none is None and abs(float(loss_only.double().cpu() - want)) <= float(g["loss"])


def test_triplet_duplicate_row():
    x, lab, (want, want_dx, _, _), d, g = triplet_case((16, 32, 4), "dup")
    i, j = torch.nonzero(lab == lab[0]).flatten()[:2].tolist()
    assert float(d["D"][i, j]) == 0.0 and bool(d["P"][i, j])
    check_triplet("triplet dup", x, lab, want, want_dx, g)


def test_triplet_gscale():
    x, lab, (want, want_dx, _, _), d, g = triplet_case((64, 32, 6))
    for gs in (-2.5, 1.0 / 3.0):
        check_triplet(f"triplet gscale {gs:.3g}", x, lab, want, want_dx * R.f32(gs), g, gscale=gs)


def test_triplet_bit_identical():
    x, lab, _, _, _ = triplet_case((65, 33, 4))
    xd, ld = x.to(DEV), lab.to(DEV)
    a = _ops().orced_triplet(xd, ld, R.EPSILON, R.MARGIN, gscale=1.0)
    b = _ops().orced_triplet(xd, ld, R.EPSILON, R.MARGIN, gscale=1.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_triplet_refusals():
    from opensetgaitrecognition_pcaa_amd import _lib
    lib = _lib.load()
    assert lib.pcaa_orced_triplet_supported(1024, 128) == 1 and lib.pcaa_orced_triplet_supported(1, 1) == 1
    assert lib.pcaa_orced_triplet_supported(1025, 32) == 0 and lib.pcaa_orced_triplet_supported(64, 129) == 0
    lab = torch.zeros(1025, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        _ops().orced_triplet(torch.ones(1025, 4, device=DEV), lab, 0.1, 0.5, gscale=1.0)
    with pytest.raises(ValueError):
        _ops().orced_triplet(torch.ones(4, 129, device=DEV), lab[:4], 0.1, 0.5, gscale=1.0)
    with pytest.raises(ValueError):
        _ops().orced_triplet(torch.ones(4, 8, device=DEV), lab[:5], 0.1, 0.5, gscale=1.0)
    with pytest.raises(TypeError):
        _ops().orced_triplet(torch.ones(4, 8, device=DEV), lab[:4].int(), 0.1, 0.5, gscale=1.0)
    with pytest.raises(RuntimeError):
        _ops().orced_triplet(torch.ones(4, 8), lab[:4].cpu(), 0.1, 0.5, gscale=1.0)
    with pytest.raises(ValueError):
        orced.orced_losses(None, None, None, None, None, {}, 0.0, triplet="torch")


def test_triplet_autograd_function():
    """functional.orced_triplet_loss: the upstream gradient multiplies dx on the device"""
    from opensetgaitrecognition_pcaa_amd import functional as F_hip
    x, lab, (want, want_dx, _, _), d, g = triplet_case((8, 4, 2))
    xd = x.to(DEV).requires_grad_(True)
    loss = F_hip.orced_triplet_loss(xd, lab.to(DEV), R.EPSILON, R.MARGIN)
    (loss * 3.0).backward()
    assert abs(float(loss.detach().double().cpu() - want)) <= float(g["loss"])
    assert R.ratio(xd.grad.cpu(), 3.0 * want_dx, 3.0 * g["dx"] + 3.0 * R.U * want_dx.abs()) <= 1.0


def test_orced_losses_hip_vs_aten(monkeypatch):
    """the golden's step inputs with TRIPLET_W = 1: ``trip`` and every parameter gradient of triplet="hip" against
    triplet="aten", at the tolerances of test_orced.py::test_orced_train_step_vs_reference_golden (losses rtol 1e-4, atol
    1e-6; gradients 5e-4 of the tensor's largest entry, floor 1e-3)"""
    from opensetgaitrecognition_pcaa_amd.train import FlatBuffer
    m = META
    B, N, C, K = m["B"], m["N"], m["C"], m["K"]
    constants.NFEATURES = C
    enc = models.ORCEDEncoder(K, nmax_points=N).float()
    dec = models.ORCEDDecoder(nmax_points=N).float()
    gml = models.GaussianMeanLearner(K).float()
    for mod, seed in zip((enc, dec, gml), m["fill_seeds"]):
        syn.deterministic_fill_(mod, seed)
        mod.to(DEV).train()
    named = [("E." + n, p) for n, p in enc.named_parameters()]
    named += [("G." + n, p) for n, p in dec.named_parameters() if n.startswith("dense")]
    named += [("ML." + n, p) for n, p in gml.named_parameters()]
    flat = FlatBuffer(named, DEV)
    for name, p in named:
        p.grad = flat.grad_views[name]
    eps = torch.from_numpy(G["eps"]).to(DEV)
    monkeypatch.setattr(torch, "randn_like", lambda t, *a, **k: eps.clone())
    T = constants.NSTEPS
    pcs = syn.synthetic_pcs(B, T, N, C, seed=m["pcs_seed"]).to(DEV).permute(0, 3, 1, 2)
    gt = syn.synthetic_labels(B, K, seed=m["gt_seed"]).to(DEV)
    cfg = dict(TRAIN_CLASSES=list(range(K)), REC_W=m["REC_W"], CE_W=m["CE_W"], KL_W=m["KL_W"], TRIPLET_W=1.0,
               TRIPLET_MARGIN=0.5)
    state = [{k: v.clone() for k, v in mod.state_dict().items()} for mod in (enc, dec, gml)]      # (BN running statistics move)
    # the condition on the inputs, on the reference alone: no undecided mining decision or hinge among these embeddings
    with torch.no_grad():
        nfv = torch.nn.functional.normalize(enc(pcs)[1], p=2, dim=1).cpu()
    cond = R.triplet_gates(R.triplet_dense(nfv, gt.cpu()))
    print(f"mining margin {cond['mining']:.3g} gates, hinge margin {cond['hinge']:.3g} gates")
    assert cond["mining"] > 1.0 and cond["hinge"] > 1.0
    res = {}
    for route in ("aten", "hip"):
        for mod, sd in zip((enc, dec, gml), state):
            mod.load_state_dict(sd)
        flat.g.zero_()
        out = orced.orced_losses(enc, dec, gml, pcs, gt, cfg, m["kl_multiplier"], triplet=route)
        out["tot"].backward()
        torch.cuda.synchronize()
        res[route] = ({k: out[k].item() for k in ("rec", "sup", "trip", "kl", "tot")},
                      {name: p.grad.detach().clone() for name, p in named})
    monkeypatch.undo()
    la, lh = res["aten"][0], res["hip"][0]
    print("losses aten", la, "hip", lh)
    assert la["trip"] > 0.0
    for k in la:
        assert abs(lh[k] - la[k]) <= 1e-4 * abs(la[k]) + 1e-6, (k, lh[k], la[k])
    worst = 0.0
    for name, _ in named:
        a, h = res["aten"][1][name].double(), res["hip"][1][name].double()
        den = max(float(a.abs().max()), 1e-3)
        worst = max(worst, float((a - h).abs().max()) / den)
        assert float((a - h).abs().max()) <= 5e-4 * den + 1e-12, (name, float((a - h).abs().max()), den)
    print(f"worst gradient difference / scale {worst:.3g}")


# ------------------------------------------------------------------------------------------------ open-set rule
def check_ood(name, c):
    r = R.ood_ref(c)
    assert r["p_margin"] > 1.0 and r["re_margin"] > 0.0
    cd = {k: v.to(DEV) for k, v in c.items()}
    out, p = _ops().orced_ood(cd["z"], cd["re"], cd["pred"], cd["mean_z"], cd["sd_z"], cd["thr_re"], R.THRESHOLDS_G, want_p=True)
    worst = float(((p.cpu() - r["p"]).abs() / r["p_gate"]).max())
    print(f"{name}: p ratio {worst:.3f}")
    assert worst <= 1.0
    assert torch.equal(out.cpu(), r["out"])
    out2 = _ops().orced_ood(cd["z"], cd["re"], cd["pred"], cd["mean_z"], cd["sd_z"], cd["thr_re"], R.THRESHOLDS_G)      # p = NULL
    assert torch.equal(out2, out)
    return r, out.cpu()


@pytest.mark.parametrize("shape", R.OOD_SHAPES, ids=ids)
def test_ood_shapes(shape):
    check_ood(f"ood {shape}", R.ood_inputs(*shape))


def test_ood_golden_block():
    r, out = check_ood("ood golden", R.golden_ood_case(G))
    assert np.array_equal(out.numpy(), G["ood.out"])


def test_ood_each_test_alone():
    r, out = check_ood("ood split", R.ood_split_case())
    assert r["latent"].tolist() == [False, True, False, True, False] and r["rec"].tolist() == [False, False, True, True, False]
    assert out.tolist() == [0, 2, 2, 2, 1]


def test_ood_refusals():
    c = {k: v.to(DEV) for k, v in R.ood_split_case().items()}
    args = lambda **kw: [({**c, **kw})[k] for k in ("z", "re", "pred", "mean_z", "sd_z", "thr_re")]
    with pytest.raises(TypeError):
        _ops().orced_ood(*args(mean_z=c["mean_z"].float()), 0.95)
    with pytest.raises(ValueError):
        _ops().orced_ood(*args(thr_re=c["thr_re"][:1]), 0.95)
    with pytest.raises(RuntimeError):
        _ops().orced_ood(*args(z=c["z"].cpu()), 0.95)


def test_scorer_golden_block():
    """fit on the golden's training block + the rule on its test block = ORCED_ensemble_ood_detection = G["ood.out"]"""
    constants.NFEATURES = 4
    enc = models.ORCEDEncoder(3, nmax_points=16).float().to(DEV)
    sc = orced.ORCEDScorer(enc, None).fit(G["ood.re_tr"], G["ood.f_tr"], G["ood.gl"], G["ood.pl"])
    mz, sz, thr = R.ood_stats(G["ood.re_tr"], G["ood.f_tr"], G["ood.gl"], G["ood.pl"])
    assert sc.n_classes == 3
    for got, want in ((sc.mean_z, mz), (sc.sd_z, sz), (sc.thr_re, thr)):
        assert got.dtype == torch.float64 and got.is_cuda
        assert np.allclose(got.cpu().numpy(), want, rtol=1e-12, atol=0.0)      # (96 fp64 terms a class, summed in another order)
    c = R.golden_ood_case(G, DEV)
    out = sc.decide(c["pred"], c["z"], c["re"])
    assert np.array_equal(out.cpu().numpy(), G["ood.out"])
    with pytest.raises(RuntimeError):
        orced.ORCEDScorer(enc, None).decide(c["pred"], c["z"], c["re"])


def test_scorer_fit_and_score_vs_host_rule():
    """a filled OR-CED model: statistics from its outputs on a training set, ``score`` on a test batch; the labels equal
    the host rule's on the very outputs ``score`` returns"""
    K, N, C, T = 4, 16, 4, constants.NSTEPS
    constants.NFEATURES = C
    enc = models.ORCEDEncoder(K, nmax_points=N).float()
    dec = models.ORCEDDecoder(nmax_points=N).float()
    syn.deterministic_fill_(enc, 80)
    syn.deterministic_fill_(dec, 81)
    enc.to(DEV).eval(); dec.to(DEV).eval()
    sc = orced.ORCEDScorer(enc, dec, batch_size=16)
    torch.manual_seed(5)
    tr = syn.synthetic_pcs(48, T, N, C, seed=11).to(DEV).permute(0, 3, 1, 2)
    # half the test batch comes from the training set, half is an enlarged other draw: accepted and rejected samples
    te = torch.cat([tr[:12], syn.synthetic_pcs(12, T, N, C, seed=12).to(DEV).permute(0, 3, 1, 2) * 1.5]).contiguous()
    with torch.no_grad():
        _, f_tr, re_tr = sc._run(tr)
    gl = torch.arange(48) % K
    pl = torch.where(torch.arange(48) % 5 == 0, (gl + 1) % K, gl)              # every fifth sample "mispredicted"
    sc.fit(re_tr, f_tr, gl, pl)
    out, preds, fv, re = sc.score(te)                                           # two chunks of 16 and 8
    assert out.shape == (24,) and out.is_cuda and fv.shape == (24, f_tr.shape[1]) and re.shape == (24,)
    host = orced.ORCED_ensemble_ood_detection(re_tr.cpu().double().numpy(), f_tr.cpu().double().numpy(), 0.95, gl.numpy(),
                                              pl.numpy(), preds.cpu(), fv.cpu().double().numpy(), re.cpu().double().numpy())
    print("scorer labels", out.tolist(), "preds", preds.tolist())
    assert torch.equal(out.cpu(), host)
    assert 0 < int((out == K).sum()) < 24                                       # both outcomes occur
