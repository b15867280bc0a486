#!/usr/bin/env python3
"""Golden fixtures of the REFERENCE's eval-mode gradients (eval_bwd_*.npz): its own CGEncoder in ``.eval()`` -- BatchNorm
a fixed per-channel affine map -- differentiated by torch's autograd on the CPU in fp32, with the fills, the input seed
and the probe loss of make_golden.py's encoder_case.

Run in the build container only (the reference is imported, never copied):

    python tests/golden/make_golden_eval_bwd.py

Stored, as make_golden.py stores them: the outputs, the loss, every parameter gradient (full tensors up to 2^15
elements, l2 + strided samples above) and the input gradient's l2 and samples.  The generator asserts what the fixture
cannot carry: no BatchNorm buffer changes, and the biases in front of the BatchNorms have gradients of the weights' order.
"""
import json
import os

import numpy as np
import torch

import make_golden as MG          # imports the reference (and stubs what it never uses on this path)
from make_golden import rmodels, syn, np_, T

HERE = os.path.dirname(os.path.abspath(__file__))


def eval_bwd_case(tag, B, N, C, K, head):
    MG.set_nfeatures(C)
    enc = rmodels.CGEncoder(K, nmax_points=N, use_projection_head=head).float()
    syn.deterministic_fill_(enc, seed=0)
    x = syn.synthetic_pcs(B, T, N, C, seed=1234).permute(0, 3, 1, 2).contiguous()
    rec = {"meta": np.array(json.dumps(dict(B=B, N=N, C=C, K=K, head=int(head), fill_seed=0, pcs_seed=1234)))}
    enc.eval()
    buffers = {k: v.clone() for k, v in enc.named_buffers()}
    rng = np.random.default_rng(77)
    r1 = torch.from_numpy(rng.standard_normal((B, K)).astype(np.float32))
    r2 = torch.from_numpy(rng.standard_normal((B, 32)).astype(np.float32))
    xg = x.clone().requires_grad_(True)
    oc, fv = enc(xg)
    loss = (oc * r1).sum() + (fv * r2).sum()
    loss.backward()
    for k, v in enc.named_buffers():
        assert torch.equal(v, buffers[k]), f"{k} changed in eval mode"
    rec["out_classes"] = np_(oc)
    rec["sup_fv"] = np_(fv)
    rec["loss"] = np.float64(loss.item())
    rec["dx_l2"] = np.float64(xg.grad.double().norm().item())
    rec["dx_samples"] = syn.checksum(xg.grad, 64)["samples"]
    MG.grads_record("grad.", enc.named_parameters(), rec)
    wmax = max(float(p.grad.abs().max()) for k, p in enc.named_parameters() if p.dim() > 1)
    for k, p in enc.named_parameters():
        if k.endswith("module.0.bias") or k.endswith("conv1d.bias"):
            assert float(p.grad.abs().max()) > 1e-3 * wmax, f"{k}: an eval-mode pre-BN bias gradient is not noise"
    path = os.path.join(HERE, tag + ".npz")
    np.savez_compressed(path, **rec)
    print(f"{tag}: {os.path.getsize(path) / 1024:.1f} KiB, {len(rec)} arrays")


if __name__ == "__main__":
    eval_bwd_case("eval_bwd_B2_N32_C4_K4", 2, 32, 4, 4, True)
    eval_bwd_case("eval_bwd_B3_N150_C4_K6_nohead", 3, 150, 4, 6, False)
