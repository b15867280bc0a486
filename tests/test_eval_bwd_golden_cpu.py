"""The eval-mode gradient fixtures (tests/golden/eval_bwd_*.npz: the reference's own CGEncoder in ``.eval()``, fp32, CPU)
against the fp64 oracle's autograd, without a GPU: the two references the GPU tests use agree with each other at the
project's gradient gate (3e-4 of the tensor's scale; when the fixtures were made the reference sat at 3.3e-5)."""
import numpy as np
import pytest
import torch

from helpers import T, check_against_record, load_golden, make_encoder
from opensetgaitrecognition_pcaa_amd import synthetic as syn
from oracle import pcaa_oracle as O


@pytest.mark.parametrize("tag", ["eval_bwd_B2_N32_C4_K4", "eval_bwd_B3_N150_C4_K6_nohead"])
def test_oracle_eval_gradients_vs_reference_fixture(tag):
    g, m = load_golden(tag)
    B, N, C, K, head = m["B"], m["N"], m["C"], m["K"], bool(m["head"])
    enc = make_encoder(K, N, C, head, seed=m["fill_seed"])
    sd = {k: (v.detach().double() if v.is_floating_point() else v.detach()).clone() for k, v in enc.state_dict().items()}
    names = [n for n, _ in enc.named_parameters()]
    for n in names:
        sd[n].requires_grad_(True)
    buffers = {k: v.clone() for k, v in sd.items() if k not in names}
    rng = np.random.default_rng(77)
    r1 = torch.from_numpy(rng.standard_normal((B, K)).astype(np.float32)).double()
    r2 = torch.from_numpy(rng.standard_normal((B, 32)).astype(np.float32)).double()
    x = syn.synthetic_pcs(B, T, N, C, seed=m["pcs_seed"]).permute(0, 3, 1, 2).double().requires_grad_(True)
    oc, fv = O.cg_encoder_forward(x, sd, head, training=False)
    loss = (oc * r1).sum() + (fv * r2).sum()
    grads = torch.autograd.grad(loss, [x] + [sd[n] for n in names])
    assert float((oc.detach() - torch.from_numpy(g["out_classes"])).abs().max()) <= 1e-4 * float(np.abs(g["out_classes"]).max())
    assert abs(loss.item() - float(g["loss"])) <= 1e-4 * abs(float(g["loss"])) + 1e-5
    assert abs(grads[0].norm().item() - float(g["dx_l2"])) <= 2e-4 * float(g["dx_l2"])
    for n, gr in zip(names, grads[1:]):
        check_against_record(g, "grad.", n, gr, 3e-4)
    pre_bn = [gr for n, gr in zip(names, grads[1:]) if n.endswith("module.0.bias") or n.endswith("conv1d.bias")]
    assert len(pre_bn) == 10 and all(float(gr.abs().max()) > 1e-3 for gr in pre_bn), "real gradients, not rounding noise"
    for k, v in buffers.items():
        assert torch.equal(sd[k], v), f"{k} changed in eval mode"
