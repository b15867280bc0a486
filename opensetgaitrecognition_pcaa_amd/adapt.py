"""Adapting a trained encoder on site with its BatchNorm frozen.

A handful of labelled windows (a batch of 2-8) has no usable batch statistics, so the encoder stays in ``.eval()``:
BatchNorm is the fixed per-channel affine map of its running statistics, and the eval-mode module is differentiated as
such (functional.encoder_backward on an eval-mode state: one pass per BatchNorm layer, csrc/elementwise.hip
``pcaa_bn_eval_act_bwd``).  The running statistics and ``num_batches_tracked`` are never written.
"""
import torch

from .functional import cross_entropy_loss, encode_track_batch, plan_tracks

HEADS = ("MLP_sup1", "MLP_head", "MLP_sup2")


def _chosen(encoder, params, who):
    if params not in ("heads", "all"):
        raise ValueError(f"{who}: params must be 'heads' or 'all', got {params!r}")
    if params == "heads":
        return [p for h in HEADS if hasattr(encoder, h) for p in getattr(encoder, h).parameters()]
    return list(encoder.parameters())


def _adam_steps(encoder, chosen, steps, lr, loss_fn):
    """``steps`` Adam steps on ``loss_fn()`` over ``chosen`` with the encoder in eval mode; the mode and the parameters'
    ``requires_grad`` flags are restored.  -> the losses before each update"""
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
            loss = loss_fn()
            loss.backward()
            opt.step()
            losses.append(loss.detach())
    finally:
        for p, f in flags:
            p.requires_grad_(f)
        encoder.train(was_training)
    return [float(l) for l in losses]


def finetune_frozen_bn(encoder, pcs, labels, steps, lr, params="heads"):
    """``steps`` Adam steps (torch.optim.Adam, default betas) on ``cross_entropy_loss(encoder(pcs)[0], labels)`` with the
    encoder in eval mode.  ``params``: ``"heads"`` updates ``MLP_sup1`` / ``MLP_head`` / ``MLP_sup2`` only (the trunk's
    parameters receive no gradient and keep their bits), ``"all"`` every parameter -- the biases in front of the
    BatchNorms included, whose gradients are real in eval mode.  ``pcs`` [B,C,T,N] and ``labels`` [B] live on the device.
    Returns the per-step losses (floats, the loss BEFORE each update); restores the train / eval mode it found and the
    parameters' ``requires_grad`` flags."""
    chosen = _chosen(encoder, params, "finetune_frozen_bn")
    return _adam_steps(encoder, chosen, steps, lr, lambda: cross_entropy_loss(encoder(pcs)[0], labels))


def finetune_frozen_bn_tracks(encoder, tracks, labels, steps, lr, params="heads", hop=None, dedup_points=False):
    """``finetune_frozen_bn`` on whole walks instead of crops: ``tracks`` is a list of processed tracks [F,N,C] (fp32, on
    the device), ``labels`` [len(tracks)] one label per walk, repeated over that track's windows (those of
    ``OpenSetScorer.embed_track``).  The loss is ``cross_entropy_loss`` over all windows of all tracks; every frame goes
    through the PointNet block once per step instead of once per window it lies in, all walks in one pass
    (``functional.cg_encoder_tracks``; ``dedup_points``: every frame's distinct detections once, found before the first
    step; ``hop``: None = CROP_STEP).  Everything else is ``finetune_frozen_bn``'s contract: eval
    mode, buffers untouched, the mode and the ``requires_grad`` flags restored, the returned floats are the losses before
    each update.  A track too short for a window raises ValueError.  Each step keeps every track's activations for the
    backward (see ``cg_encoder_tracks``): the caller bounds the walks."""
    chosen = _chosen(encoder, params, "finetune_frozen_bn_tracks")
    tracks = list(tracks)
    if len(tracks) < 1 or labels.dim() != 1 or labels.numel() != len(tracks):
        raise ValueError(f"finetune_frozen_bn_tracks: needs at least one track and labels [{len(tracks)}], got "
                         f"{tuple(labels.shape)}")
    # the tracks do not change between the steps: their frames are checked and gathered, their windows planned (a track too
    # short for one: ValueError) and (dedup_points) their distinct rows found ONCE, host copy and flag read outside the loop
    batch = plan_tracks(encoder, tracks, hop, True, dedup_points, who="finetune_frozen_bn_tracks")
    win_labels = torch.repeat_interleave(labels, torch.tensor(batch.counts, device=labels.device)).contiguous()
    return _adam_steps(encoder, chosen, steps, lr,
                       lambda: cross_entropy_loss(encode_track_batch(encoder, batch)[0], win_labels))
