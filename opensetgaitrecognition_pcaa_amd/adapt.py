"""Adapting a trained encoder on site with its BatchNorm frozen.

A handful of labelled windows (a batch of 2-8) has no usable batch statistics, so the encoder stays in ``.eval()``:
BatchNorm is the fixed per-channel affine map of its running statistics, and the eval-mode module is differentiated as
such (functional.encoder_backward on an eval-mode state: one pass per BatchNorm layer, csrc/elementwise.hip
``pcaa_bn_eval_act_bwd``).  The running statistics and ``num_batches_tracked`` are never written.
"""
import torch

from .functional import cross_entropy_loss

HEADS = ("MLP_sup1", "MLP_head", "MLP_sup2")


def finetune_frozen_bn(encoder, pcs, labels, steps, lr, params="heads"):
    """``steps`` Adam steps (torch.optim.Adam, default betas) on ``cross_entropy_loss(encoder(pcs)[0], labels)`` with the
    encoder in eval mode.  ``params``: ``"heads"`` updates ``MLP_sup1`` / ``MLP_head`` / ``MLP_sup2`` only (the trunk's
    parameters receive no gradient and keep their bits), ``"all"`` every parameter -- the biases in front of the
    BatchNorms included, whose gradients are real in eval mode.  ``pcs`` [B,C,T,N] and ``labels`` [B] live on the device.
    Returns the per-step losses (floats, the loss BEFORE each update); restores the train / eval mode it found and the
    parameters' ``requires_grad`` flags."""
    if params not in ("heads", "all"):
        raise ValueError(f"finetune_frozen_bn: params must be 'heads' or 'all', got {params!r}")
    if params == "heads":
        chosen = [p for h in HEADS if hasattr(encoder, h) for p in getattr(encoder, h).parameters()]
    else:
        chosen = list(encoder.parameters())
    chosen_ids = {id(p) for p in chosen}
    flags = [(p, p.requires_grad) for p in encoder.parameters()]
    was_training = encoder.training
    opt = torch.optim.Adam(chosen, lr=lr)
    losses = []
    try:
        encoder.eval()
        for p, _ in flags:
            p.requires_grad_(id(p) in chosen_ids)
        for _ in range(int(steps)):
            opt.zero_grad(set_to_none=True)
            logits, _ = encoder(pcs)
            loss = cross_entropy_loss(logits, labels)
            loss.backward()
            opt.step()
            losses.append(loss.detach())
    finally:
        for p, f in flags:
            p.requires_grad_(f)
        encoder.train(was_training)
    return [float(l) for l in losses]
