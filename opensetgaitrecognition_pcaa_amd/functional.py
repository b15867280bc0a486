"""Forward/backward engines of the PCAA modules on the HIP path, and the
``torch.autograd.Function`` wrappers that make the drop-in modules of
:mod:`.models` behave like the reference's (``models.py`` of the reference;
see each function for file:line).

Layout: activations are point-major ``[rows, channels]`` (rows = B*T*N points
or B*T time steps).  The module-facing tensors keep the reference's logical
shapes (``[B,C,T,N]``, ``[B,C,T]``) as zero-copy permuted views.

Numerics modes (``set_precision``):
  * ``"fp32"``  -- fp32 storage, exact-fp32 MFMA: the parity mode (1e-4 gate).
  * ``"fp16x3"`` -- (round 3) parity-grade without the 1/16-rate fp32 MFMA: everything as in ``"fp32"`` except the
    PointNet layers' 2-4 products, whose fp32 operands are kept as [hi | lo] fp16 images (times a power of two
    that keeps them in fp16's normal range) and multiplied as hi.hi + lo.hi + hi.lo on the f16 MFMA pipe
    (pcaa_gemm_split3; fp32 accumulation, 22 mantissa bits per operand): passes the fp32 mode's 1e-4 /
    bit-exact-label / 5e-4-gradient gates unchanged (embedding error 2.0e-6 of scale against exact fp32's 2.5e-6 at
    the benchmarked size) at about half its step time.
  * ``"bf16"``  -- PointNet activations stored in bf16, PointNet GEMMs on the
    bf16 MFMA pipe with fp32 accumulation; everything else fp32.
"""
import collections
import contextlib
import functools
import math
import itertools

import numpy as np

import torch
from torch.autograd.function import once_differentiable

from . import frame_table, ops
from ._lib import ACT_ELU, ACT_NONE, KC, PCAA_BF16, PCAA_F32, RC

_PRECISION = {"mode": "fp32"}
_SYNC_BN = {"group": None}


# Optional section marks: with a list installed (set_marks), mark(name) records a timing event on the
# current stream at a few section boundaries of the step (tools/step_sections.py prints the elapsed
# times between them).  Off by default: no events, no cost.
_MARKS = None


def set_marks(lst):
    global _MARKS
    _MARKS = lst


def mark(name):
    if _MARKS is not None:
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        _MARKS.append((name, ev))


def _check_precision(mode):
    if mode not in ("fp32", "bf16", "fp16x3"):
        raise ValueError("precision must be 'fp32', 'bf16' or 'fp16x3'")
    return mode


def set_precision(mode: str):
    _PRECISION["mode"] = _check_precision(mode)


def get_precision() -> str:
    return _PRECISION["mode"]


# How the eval-mode PointNet layers 2-4 multiply in bf16 mode: "bf16" (default) or "fp8" -- e4m3 operands on the block-scaled
# MFMA (ops.gemm_fp8_affine_elu; the numerics contract is in include/pcaa_hip.h and DESIGN.md section 4).  A switch beside
# the precision mode, read at each call like it; honoured exactly where the fused bf16 epilogue route runs (_pointnet_plan),
# ignored everywhere else: training, a forward that keeps what a backward reads, fp32 and fp16x3 modes, unsupported shapes.
_EVAL_POINTNET = {"kind": "bf16"}


def _check_eval_pointnet(kind):
    if kind not in ("bf16", "fp8"):
        raise ValueError("eval_pointnet kind must be 'bf16' or 'fp8'")
    return kind


def set_eval_pointnet(kind: str):
    _EVAL_POINTNET["kind"] = _check_eval_pointnet(kind)


def get_eval_pointnet() -> str:
    return _EVAL_POINTNET["kind"]


@contextlib.contextmanager
def eval_pointnet(kind):
    """``with eval_pointnet("fp8"):`` -- the kind inside the block, the previous one restored after it"""
    prev = _EVAL_POINTNET["kind"]
    _EVAL_POINTNET["kind"] = _check_eval_pointnet(kind)
    try:
        yield
    finally:
        _EVAL_POINTNET["kind"] = prev


def set_sync_bn_group(group):
    """``None`` (per-rank BatchNorm statistics, stock DDP semantics) or a
    torch.distributed process group over which the fp64 batch statistics are
    all-reduced (SyncBN: the 8-GPU step equals the single-process global-batch
    step of the reference)."""
    _SYNC_BN["group"] = group


@contextlib.contextmanager
def sync_bn_group(group):
    """``with sync_bn_group(g):`` -- SyncBN over ``g`` inside the block, the previous setting restored after it
    (how PCAATrainer scopes its group to its own train-mode work)."""
    prev = _SYNC_BN["group"]
    _SYNC_BN["group"] = group if group is not None else prev
    try:
        yield
    finally:
        _SYNC_BN["group"] = prev


def _sync_stats(stats, count):
    g = _SYNC_BN["group"]
    if g is None:
        return count
    import torch.distributed as dist
    ev = _SYNC_BN.get("events")
    if ev is not None:
        # PCAATrainer.time_comm: these all-reduces are synchronous on the main stream -- all of their time is exposed
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dist.all_reduce(stats, group=g)
        e1.record()
        ev.append((e0, e1))
    else:
        dist.all_reduce(stats, group=g)
    _SYNC_BN["collectives"] = _SYNC_BN.get("collectives", 0) + 1          # PCAATrainer folds these into its comm record
    _SYNC_BN["payload_bytes"] = _SYNC_BN.get("payload_bytes", 0) + stats.numel() * stats.element_size()
    return count * dist.get_world_size(g)


def _sync_fn():
    """the ``sync`` argument of ops.BnTailFwd / BnTailBwd: None unless SyncBN is on (then the statistics are all-reduced
    before a stand-alone finalize; the producer cannot carry it)"""
    return _sync_stats if _SYNC_BN["group"] is not None else None


def _require_gpu(x, what):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError(f"{what}: input must live on the HIP device; this package has no CPU path "
                           "(the CPU restatement lives in oracle/ and is test infrastructure only)")
    if x.numel() == 0:
        # the reference's train-mode BatchNorm raises ValueError on an empty batch ("Expected more than 1 value per
        # channel"); its eval mode would hand back empty tensors -- here both refuse (error behaviour)
        raise ValueError(f"{what}: empty input {tuple(x.shape)}")


def _point_major(x):
    """logical [B,C,T,N] -> contiguous [B,T,N,C] storage (no copy if x already
    is a permuted view of point-major storage)."""
    xp = x.permute(0, 2, 3, 1)
    if xp.is_contiguous() and x.dtype == torch.float32:
        return xp
    return ops.pack_points(x.float() if x.dtype != torch.float32 else x)


# ======================================================================
# Linear + BatchNorm + ELU stacks (PointNetBlock models.py:82-105 and
# TemporalConvolutionBlock models.py:108-160)
# ======================================================================
class _LayerSave:
    __slots__ = ("a_in", "col", "y", "scale", "shift", "mean", "rstd", "rows", "cin", "cout", "dil", "pool_e", "mom", "wt")

    def __init__(self, a_in, col, y, scale, shift, mean, rstd, rows, cin, cout, dil, pool_e=None, mom=None, wt=None):
        self.a_in = a_in             # (one plain store per slot: ten of these are built in every forward)
        self.col = col
        self.y = y
        self.scale = scale
        self.shift = shift
        self.mean = mean
        self.rstd = rstd
        self.rows = rows
        self.cin = cin
        self.cout = cout
        self.dil = dil
        self.pool_e = pool_e
        self.mom = mom
        self.wt = wt                 # the image of W^T the layer's dgrad multiplies by, where the forward made it


class EncoderEvalConstants:
    """What an eval-mode forward derives from a FROZEN encoder alone, computed once by the kernels that compute it in every
    forward otherwise (same bits): the folded BatchNorm coefficients ``(scale, shift)`` of the ten BatchNorm layers and, in
    bf16 mode, the bf16 images of the weights of PointNet layers 2-4.  It records what it was made from -- the encoder, the
    precision mode, the eval-PointNet kind, and ``_version`` and storage address of every parameter and buffer -- and
    ``valid_for`` compares that, so a holder notices ``load_state_dict``, an optimizer step, a move to another dtype or
    device, a mode switch or ``set_eval_pointnet``.  Made under kind "fp8" (bf16 mode) it also holds ``w8``: the e4m3
    image and the folded coefficient ``scale * s`` of PointNet layers 2-4 (ops.quantize_weight_fp8).  (The
    tensors are the ones the encoder had when this was made: a Parameter OBJECT swapped for another is only noticed
    through ``encoder_eval_constants`` being called again.)  Never shared between encoders."""
    __slots__ = ("mode", "kind", "bn", "w16", "w8", "enc_id", "tensors", "stamp")

    def _stamp(self):
        return [(t._version, t.data_ptr()) for t in self.tensors]

    def valid_for(self, enc, mode):
        return (id(enc) == self.enc_id and mode == self.mode and self.kind == get_eval_pointnet()
                and self._stamp() == self.stamp)


def encoder_eval_constants(enc, mode=None):
    """-> EncoderEvalConstants of ``enc`` for ``mode`` (default: the current precision mode): ten pcaa_bn_eval_coeffs launches
    and, in bf16 mode, three weight casts, once instead of in every eval forward (``consts=`` of encoder_frame_features /
    encoder_forward_windows)."""
    mode = get_precision() if mode is None else _check_precision(mode)
    if enc.training:
        raise RuntimeError("encoder_eval_constants: the encoder is in training mode (its BatchNorm uses batch statistics)")
    c = EncoderEvalConstants()
    c.mode, c.kind, c.bn, c.w16, c.w8, c.enc_id = mode, get_eval_pointnet(), {}, {}, {}, id(enc)
    c.tensors = list(itertools.chain(enc.parameters(), enc.buffers()))
    c.stamp = c._stamp()
    with torch.no_grad():
        for li, layer in enumerate(enc.pc_block.layers()):
            conv, bn = layer.module[0], layer.module[1]
            cout, cin = conv.weight.shape[0], conv.weight.shape[1]
            c.bn[id(bn)] = ops.bn_eval_coeffs(bn, cout, conv.bias)
            if mode == "bf16" and li > 0 and cin % 8 == 0:
                c.w16[id(conv)] = ops.cast_bf16(conv.weight.view(cout, cin), True, False)[0]
                if c.kind == "fp8":
                    c.w8[id(conv)] = _quantize_layer(conv.weight.view(cout, cin), c.bn[id(bn)][0])
        for layer in enc.tc_block.layers():
            c.bn[id(layer.batch_norm)] = ops.bn_eval_coeffs(layer.batch_norm, layer.conv1d.weight.shape[0], layer.conv1d.bias)
    return c


def _eval_coeffs(consts, bn, cout, lin_bias):
    """eval-mode (scale, shift) of one BatchNorm layer: from the frozen constants when given, else computed now"""
    if consts is not None:
        return consts.bn[id(bn)]
    return ops.bn_eval_coeffs(bn, cout, lin_bias)


def _eval_w16(consts, conv, W2d):
    """the bf16 image of an eval-mode PointNet weight: from the frozen constants when given, else cast now"""
    if consts is not None:
        return consts.w16[id(conv)]
    return ops.cast_bf16(W2d, True, False)[0]


def _quantize_layer(W2d, scale):
    """(W8, scale8) of one eval-mode PointNet layer: the e4m3 image and the BatchNorm scale with the rows' weight scales
    folded in (a power of two each: the product is exact)"""
    W8, s = ops.quantize_weight_fp8(W2d)
    return W8, scale * s


def _eval_w8(consts, conv, W2d, scale):
    """(W8, scale8) from the frozen constants where they hold them (made under kind "fp8"), else quantised now"""
    if consts is not None and id(conv) in consts.w8:
        return consts.w8[id(conv)]
    return _quantize_layer(W2d, scale)


def _linear_out_dtype(mode, in_pointnet):
    """dtype of the pre-BatchNorm y of the general product: the PointNet stack stores its activations in bf16 in bf16 mode"""
    return torch.bfloat16 if (mode == "bf16" and in_pointnet) else torch.float32


def _linear_route(a_dtype, rows, cin, cout, training, mode, in_pointnet):
    """Which launch forms y[rows, cout] = a . W^T in _linear_bn.  Pure: launches and allocates nothing.  ``a_dtype``:
    ops.SplitImage.dtype for a split image; ``in_pointnet``: the caller is the PointNet stack (pointnet_forward), whose
    layer over raw points has a streaming kernel of its own and whose y is bf16 in bf16 mode."""
    if a_dtype == ops.SplitImage.dtype:
        return "split3"                  # fp16x3 mode: both operands as [hi | lo] images, three f16 MFMA passes, fp32 result
    if in_pointnet and a_dtype == torch.float32 and cin <= 8 and ops.pointnet_in_ok(cin, cout):
        return "in_store"                # raw points -> first PointNet layer: C-wide contraction, HBM-bound streaming kernel
    if mode == "bf16" and a_dtype == torch.bfloat16 and cin % 8 == 0:
        return "bf16"
    tiles = ((rows + 127) // 128) * ((cout + 127) // 128)
    sk = ops.pick_split_k(rows, cout, cin, target_blocks=512)
    if (training and _linear_out_dtype(mode, in_pointnet) == torch.float32 and tiles < 128 and sk > 1 and cout % 4 == 0
            and 256 % (cout // 4) == 0 and cout <= 1024):
        # few output tiles, long K (the temporal block): split K through slabs; the reduction
        # pass also produces the BatchNorm statistics the GEMM epilogue would have
        return "fp32_slabs"
    return "fp32"


def _linear_bn(a_in, W2d, lin_bias, bn, training, mode, in_pointnet, consts=None, conv=None, route=None):
    """y = a_in @ W2d^T (the linear bias is NOT added: it cancels in train-mode BatchNorm and
    is folded into ``shift`` in eval mode; see bn_finalize_kernel) with BatchNorm statistics;
    returns the bias-free y, the BN coefficients that apply to it and, where a train-mode launch made it beside its own
    operand, the image of W^T for the layer's dgrad (else None).  ``route``: _linear_route's answer where the caller has it."""
    rows, cin = a_in.shape
    cout = W2d.shape[0]
    if route is None:
        route = _linear_route(a_in.dtype, rows, cin, cout, training, mode, in_pointnet)
    stats = ops.new_stats(cout, a_in.device) if training else None
    # the finalize of these statistics rides on the launch that produces them where that launch can carry it
    # (csrc/bn_tail.h: its last workgroup writes the coefficients); else tail.resolve() ran the stand-alone kernel
    tail = ops.BnTailFwd(rows, lin_bias, bn, cout, sync=_sync_fn()) if training else None
    out_dtype = _linear_out_dtype(mode, in_pointnet)
    wt = None
    if route == "split3":
        w_img = ops.split_f16(W2d)
        if training:
            wt = ops.split_f16(W2d, transpose=True)
        y = ops.gemm_split3(a_in, w_img, KC, rows, cout, cin, colstats=stats, tail=tail)
    elif route == "in_store":
        y = ops.pointnet_in_fwd(a_in, W2d, None, out_dtype, stats, tail=tail)
    elif route == "bf16":
        # bf16 shadow of the weights so both operands stream by LDS-DMA (the transposed copy
        # serves the dgrad GEMM of the backward pass)
        if consts is not None and not training:
            w16 = _eval_w16(consts, conv, W2d)
        else:
            w16, wt = ops.cast_bf16(W2d, True, training)
        y = ops.gemm(a_in, KC, w16, KC, rows, cout, cin, colstats=stats, out_dtype=out_dtype, math=PCAA_BF16, tail=tail)
    elif route == "fp32_slabs":
        sk = ops.pick_split_k(rows, cout, cin, target_blocks=512)
        y = ops.gemm_slabs(a_in, KC, W2d, KC, rows, cout, cin, sk, math=PCAA_F32, colstats=stats, tail=tail)
    else:
        y = ops.gemm(a_in, KC, W2d, KC, rows, cout, cin, colstats=stats, out_dtype=out_dtype, math=PCAA_F32, tail=tail)
    if training:
        scale, shift, mean, rstd = tail.out
        count = tail.count_out
    else:
        scale, shift = _eval_coeffs(consts, bn, cout, lin_bias)
        mean = rstd = None
        count = rows
    return y, scale, shift, mean, rstd, count, wt


def _epilogue_pools(pool_rows):
    """whether the fused-epilogue GEMMs (ops.gemm_affine_elu, ops.gemm_fp8_affine_elu) take the mean over groups of
    ``pool_rows`` rows in their epilogue"""
    return pool_rows in (32, 64, 128)


_IN_RECOMPUTE = ("in_moments", "in_stats", "in_eval")


def _pointnet_plan(dims, rows, in_dtype, training, mode, pool_rows, want_bwd, last_pre_bn, kind, sync_bn, tails):
    """What pointnet_forward launches.  Pure: plain values in, launches and allocates nothing.  ``dims``: (cin, cout) of each
    layer; ``kind``: the eval-PointNet kind; ``sync_bn``: SyncBN is on; ``tails``: ops.TAILS["enabled"].
    Returns (routes, hands, finish).  ``routes[i]``: "in_moments" / "in_stats" / "in_eval" (the layer over raw points, y
    recomputed and never stored: statistics from the points' second moments, from a statistics pass, or frozen), "fp8" /
    "bf16_epilogue" (eval mode: BatchNorm + ELU in the GEMM epilogue, no stored y), or a _linear_route name (y stored).
    ``hands[i]``: dtype of what layer i hands on (ops.SplitImage.dtype for a split image).  ``finish``: what turns the last
    layer's result into the output: "done" (its launch wrote it, pooled where pool_rows), "meanpool", "act" or "pre_bn"."""
    nl = len(dims)
    infer = not training and not want_bwd            # nothing is kept for a backward: the epilogue routes are open
    from_points = in_dtype == torch.float32 and dims[0][0] <= 8 and ops.pointnet_in_ok(*dims[0])
    # fp8: the kind asks for it, the call is one the bf16 epilogue route serves, the first layer is the recompute layer (it
    # writes the e4m3 operand) and every later layer has a shape pcaa_gemm_fp8_affine_elu takes -- all or none
    fp8 = (kind == "fp8" and infer and mode == "bf16" and nl > 1 and from_points
           and (not pool_rows or (_epilogue_pools(pool_rows) and rows % pool_rows == 0))
           and all(ops.gemm_fp8_supported(rows, cout, cin) for cin, cout in dims[1:]))
    # fp16x3 mode: the activations between the layers are [hi | lo] images when every later product is one the
    # LDS-DMA kernel serves (whole 256-tiles); else the layer stack runs in exact fp32 -- all or none
    split = (mode == "fp16x3" and nl > 1 and (training or not want_bwd)
             and all(ops.gemm_split3_supported(rows, cout, cin) and cin % 256 == 0 for cin, cout in dims[1:]))
    y_dtype = _linear_out_dtype(mode, True)
    routes, hands, finish, dtype = [], [], "done", in_dtype
    for li, (cin, cout) in enumerate(dims):
        pooled = li == nl - 1 and bool(pool_rows)
        if dtype == torch.float32 and cin <= 8 and ops.pointnet_in_ok(cin, cout) and not pooled:
            # y = x.W^T costs cin FMAs per element, less than reading it back.  It is linear in the points: without SyncBN
            # the batch statistics follow from the points' C x C second moments, which the backward reuses
            route = ("in_moments" if not sync_bn and tails else "in_stats") if training else "in_eval"
            dtype = ops.FP8 if fp8 else torch.bfloat16 if mode == "bf16" else ops.SplitImage.dtype if split else torch.float32
        elif fp8:
            # layers 2 and 3 hand on e4m3, the last one bf16 rows (the ragged route's segment_weighted_mean reads them) or
            # the fp32 mean over the frame's points
            route = "fp8"
            dtype = ops.FP8 if li < nl - 1 else (torch.float32 if pooled else torch.bfloat16)
        elif (infer and mode == "bf16" and dtype == torch.bfloat16 and (not pooled or _epilogue_pools(pool_rows))
                and ops.gemm_dgrad_bn_supported(rows, cout, cin)):
            route = "bf16_epilogue"
            dtype = torch.float32 if pooled else torch.bfloat16
        else:
            route = _linear_route(dtype, rows, cin, cout, training, mode, True)
            dtype = ops.SplitImage.dtype if (split and li < nl - 1) else y_dtype
            if li == nl - 1:
                finish = "meanpool" if pooled else ("pre_bn" if last_pre_bn else "act")
        routes.append(route)
        hands.append(dtype)
    return routes, hands, finish


def _in_recompute_save(route, x, W2d, conv, bn, consts):
    """the save of a recompute first layer, its BatchNorm coefficients by ``route``: y = x.W^T is never stored"""
    rows, (cout, cin) = x.shape[0], W2d.shape
    mean = rstd = mom = None
    count = rows
    if route == "in_moments":
        # the layer's batch statistics from the points' second moments (a 4 MB read): no statistics pass over [P, cout]
        scale, shift, mean, rstd, mom = ops.pointnet_in_moment_coeffs(x, W2d, conv.bias, bn)
    elif route == "in_stats":
        stats = ops.new_stats(cout, x.device)
        tail = ops.BnTailFwd(rows, conv.bias, bn, cout, sync=_sync_fn())
        ops.pointnet_in_fwd(x, W2d, None, None, stats, tail=tail)
        scale, shift, mean, rstd = tail.out
        count = tail.count_out
    else:
        scale, shift = _eval_coeffs(consts, bn, cout, conv.bias)
    return _LayerSave(x, None, None, scale, shift, mean, rstd, count, cin, cout, 0, mom=mom)


def pointnet_forward(xp2d, layers, training, mode, pool_rows=0, consts=None, want_bwd=False, last_pre_bn=False):
    """xp2d: [P, C] fp32.  Returns (output, saves).  If pool_rows>0 the last
    layer's ELU output is mean-pooled over groups of pool_rows rows (fp32
    [P/pool_rows, ch]); else the last activation [P, ch] is returned.
    ``consts`` (eval only): the encoder's EncoderEvalConstants, used instead of recomputing them.
    ``want_bwd`` (matters in eval mode only): a backward will follow, so every layer keeps what pointnet_backward reads
    (its pre-BatchNorm ``y``: no fused-epilogue layers, no split images); off, the eval forward is unchanged.
    ``last_pre_bn`` (with pool_rows == 0): where the last layer stores its pre-BatchNorm ``y`` (every route but the
    fused-epilogue GEMM), return that ``y`` instead of ELU(BN(y)) -- the caller applies ``saves[-1].scale / .shift``
    itself (encoder_frame_features_ragged: in its pooling pass); ``saves[-1].y`` is None where the epilogue already did."""
    if consts is not None and (training or consts.mode != mode):
        raise ValueError("pointnet_forward: consts are eval-mode constants of one precision mode "
                         f"(made for {consts.mode!r}, asked for {mode!r}, training={training})")
    rows, nl = xp2d.shape[0], len(layers)
    dims = [(l.module[0].weight.shape[1], l.module[0].weight.shape[0]) for l in layers]
    routes, hands, finish = _pointnet_plan(dims, rows, xp2d.dtype, training, mode, pool_rows, want_bwd, last_pre_bn,
                                           _EVAL_POINTNET["kind"], _SYNC_BN["group"] is not None, ops.TAILS["enabled"])
    saves = []
    a = xp2d
    for li, layer in enumerate(layers):
        conv, bn = layer.module[0], layer.module[1]
        (cin, cout), route = dims[li], routes[li]
        W2d = conv.weight.view(cout, cin)
        epilogue_pool = pool_rows if li == nl - 1 else 0
        if route in _IN_RECOMPUTE:
            s = _in_recompute_save(route, a, W2d, conv, bn, consts)
            a = ops.pointnet_in_apply(a, W2d, s.scale, s.shift, hands[li])
        elif route == "fp8":
            # as the fused bf16 route below, on e4m3 operands
            scale, shift = _eval_coeffs(consts, bn, cout, conv.bias)
            W8, scale8 = _eval_w8(consts, conv, W2d, scale)
            s = _LayerSave(a, None, None, scale, shift, None, None, rows, cin, cout, 0)
            a = ops.gemm_fp8_affine_elu(a, W8, scale8, shift, epilogue_pool, hands[li])
        elif route == "bf16_epilogue":
            # eval mode: BatchNorm is a fixed per-channel affine map -> BN + ELU (and the mean over the frame's
            # points for the last layer) in the GEMM epilogue: no stored y, no separate pass
            scale, shift = _eval_coeffs(consts, bn, cout, conv.bias)
            w16 = _eval_w16(consts, conv, W2d)
            s = _LayerSave(a, None, None, scale, shift, None, None, rows, cin, cout, 0)
            a = ops.gemm_affine_elu(a, w16, scale, shift, epilogue_pool)
        else:
            y, scale, shift, mean, rstd, count, wt = _linear_bn(a, W2d, conv.bias, bn, training, mode, True, consts, conv, route)
            s = _LayerSave(a, None, y, scale, shift, mean, rstd, count, cin, cout, 0, wt=wt)
            act = ops.bn_act_fwd_split if hands[li] == ops.SplitImage.dtype else ops.bn_act_fwd
            a = act(y, scale, shift) if li < nl - 1 else y                 # (the last y: ``finish`` below)
        saves.append(s)
    if finish == "act":
        a = ops.bn_act_fwd(a, s.scale, s.shift)
    elif finish == "meanpool" and training:
        a, s.pool_e = ops.bn_act_meanpool_fwd(a, s.scale, s.shift, rows // pool_rows, pool_rows, s.mean, s.rstd)
    elif finish == "meanpool":
        a = ops.bn_act_meanpool_fwd(a, s.scale, s.shift, rows // pool_rows, pool_rows)
    return a, saves                      # ("pre_bn": the last layer's y itself; "done": its launch wrote the output)


class _FusedGrad:
    """What the fused dgrad (ops.gemm_dgrad_bn) hands to the layer below instead of da:
    dz = da * ELU'(z) and that layer's BatchNorm-backward statistics."""
    __slots__ = ("dz", "stats", "fin")

    def __init__(self, dz, stats, fin=None):
        # fin: (coef, dgamma, dbeta) of that layer when the producing launch carried its finalize (ops.BnTailBwd)
        self.dz, self.stats, self.fin = dz, stats, fin


# Side stream for the SMALL weight-gradient products (temporal block, MLP heads): they only feed the
# optimizer at the end of the step, are 10-50 us launches on a handful of CUs, and are independent of the
# dgrad that continues the chain -- run beside it they leave the backward's critical path.  Set per step by
# the trainer (set_wgrad_stream), which joins the stream before the encoder-gradient all-reduce / Adam.
_WGRAD_STREAM = None


def set_wgrad_stream(stream):
    global _WGRAD_STREAM
    _WGRAD_STREAM = stream


class _on_wgrad_stream:
    """``with _on_wgrad_stream(t1, t2, ...)``: run the body on the wgrad side stream after everything
    enqueued so far; the listed tensors (inputs allocated on the main stream) are kept alive for it."""

    def __init__(self, *tensors):
        self.tensors = tensors
        self.ctx = None

    def __enter__(self):
        st = _WGRAD_STREAM
        if st is None:
            return self
        ev = torch.cuda.Event()
        ev.record()                      # (on the current stream)
        self.ctx = ops.on_stream(st)
        self.ctx.__enter__()
        st.wait_event(ev)
        for t in self.tensors:
            if t is not None:
                t.record_stream(st)
        return self

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)
        return False


# Fusions that have an unfused fallback for the shapes their kernels do not take were A/B-ed through environment switches
# (docs/LAB_LOG.md sections 4 and 8, profiles/r03_ab_runs.txt); what was decided is plain code, with no switch left here: the slab
# reductions behind the PointNet weight gradients run on the side stream (_layer_wgrad), the first PointNet layer takes its
# statistics from the points' second moments (_pointnet_plan) and its backward reads the incoming gradient once
# (_in_bwd_route), the MLP heads and the eval-mode epilogues are fused wherever their kernels take the shape.  What still
# has a switch: _FUSE_DTC (tests toggle it; an argument of _dtc_plan), ops.TAILS / PCAA_BN_TAIL, and the library's own
# PCAA_DTC_PAIR (csrc/dtc_fused.hip reads it once; _dtc_plan asks the library, so the Python side follows it).


def _bwd_tail(save, bn, outs, ch):
    """the BatchNorm-backward finalize of ``save``'s layer, for the launch that reduces its statistics to carry"""
    return ops.BnTailBwd(save.rows, bn, save.mean, save.rstd, ch, dgamma=outs[1] if outs else None,
                         dbeta=outs[2] if outs else None, sync=_sync_fn())


def _fused_coefficients(da, s, bn, outs):
    """(coef, dgamma, dbeta) behind a _FusedGrad: finalized by the launch that produced the statistics, else (SyncBN) now"""
    if da.fin is not None:
        return da.fin
    _sync_stats(da.stats, 0)
    return ops.bn_bwd_finalize(da.stats, s.rows, bn, s.mean, s.rstd, s.cout, dgamma=outs[1] if outs else None,
                               dbeta=outs[2] if outs else None)


class _RaggedPool:
    """In the ``group_rows`` place of a ``pool=`` tuple: the pooled groups are the ragged segments ``u_off`` of the rows,
    row r counted ``weight[r]`` times out of N (ops.segment_weighted_mean) -- eval mode only."""
    __slots__ = ("weight", "u_off", "N")

    def __init__(self, weight, u_off, N):
        self.weight, self.u_off, self.N = weight, u_off, int(N)


def _bn_dy(s, bn, da, pool, lhs_split, outs, lin_bias, dbias_out, adjoint_dy=None):
    """First stage: the gradient w.r.t. the pre-BatchNorm ``s.y``, from ``da`` (tensor or _FusedGrad) or ``pool``, and the
    BatchNorm gradients.  ``lhs_split``: dy is wanted as a SplitImage; ``adjoint_dy``: the caller's adjoint when it forms dy
    itself (then d_lhs comes back too).  Returns (dy, dgamma, dbeta, dbias, d_lhs or None)."""
    y = s.y
    dpool, group_rows, pool_scale = pool if pool is not None else (None, 0, 1.0)
    if isinstance(da, torch.Tensor) and da.dtype != y.dtype:
        da = da.to(y.dtype)
    grad = dict(da=da, dpool=dpool, group_rows=group_rows, pool_scale=pool_scale)      # (unused with a _FusedGrad)
    # ---- eval-mode save: BatchNorm was the fixed map z = scale*y + shift, so no batch statistic stands between da and dy:
    # dy and the two column sums in ONE pass, then their finalize; the running statistics are only read, and no collective
    # is issued whatever the SyncBN setting
    if s.mean is None:
        emean, erstd = ops.bn_eval_moments(bn, s.cout, lin_bias)
        if isinstance(group_rows, _RaggedPool):
            # the layer's output was pooled over ragged segments with multiplicities (frame_features_ragged)
            dy, stats = ops.segment_weighted_mean_bwd(dpool, y, group_rows.weight, group_rows.u_off, group_rows.N,
                                                      s.scale, s.shift, emean, erstd)
        else:
            dy, stats = ops.bn_eval_act_bwd(y, s.scale, s.shift, emean, erstd, out=da, **grad)
        dgamma, dbeta, dbias = ops.bn_eval_bwd_finalize(stats, s.scale, s.cout, dgamma=outs[1] if outs else None,
                                                        dbeta=outs[2] if outs else None,
                                                        dbias=dbias_out if lin_bias is not None else None)
        return dy, dgamma, dbeta, dbias, None
    if isinstance(group_rows, _RaggedPool):
        raise RuntimeError("a ragged pool is an eval-mode form (train-mode BatchNorm would need weighted batch statistics)")
    # ---- fused: the dgrad above already applied ELU' and reduced the statistics
    if isinstance(da, _FusedGrad):
        coef, dgamma, dbeta = _fused_coefficients(da, s, bn, outs)
        if adjoint_dy is not None:
            # the adjoint kernel forms dy = c0*dz + c1*y + c2 while it stages its operand and hands it back
            # for the weight gradient: no separate elementwise pass
            d_lhs, dy = adjoint_dy.forming_dy(da.dz, y, coef)
            return dy, dgamma, dbeta, None, d_lhs
        if lhs_split:
            # fp16x3 mode: dz (fp32) came out of the split-operand dgrad's epilogue; dy only feeds the two products below
            dy = ops.bn_bwd_dy_split(da.dz, y, coef)
        else:
            dy = ops.bn_bwd_dy(da.dz, y, coef, out=da.dz)
        return dy, dgamma, dbeta, None, None
    # ---- plain: pass 1: statistics only (reads da/dpool and y, writes nothing); pass 2: dy directly, with
    # dz = da*ELU'(z) recomputed in registers -- dz is never materialised
    tail = _bwd_tail(s, bn, outs, s.cout)
    if dpool is not None and s.pool_e is not None:
        # mean-pooled layer: the statistics follow from the forward's per-group sums, y is not re-read
        ops.bn_pool_bwd_stats(dpool, s.pool_e, pool_scale, tail=tail)
    else:
        ops.bn_act_bwd_stats(y, s.scale, s.shift, s.mean, s.rstd, tail=tail, **grad)
    coef, dgamma, dbeta = tail.out
    if lhs_split:
        # fp16x3 mode: dy only feeds the two products below -> written as its [hi | lo] image
        dy = ops.bn_bwd_dy_fused_split(y, s.scale, s.shift, coef, **grad)
    else:
        dy = ops.bn_bwd_dy_fused(y, s.scale, s.shift, coef, out=da, **grad)
    return dy, dgamma, dbeta, None, None


def _wgrad_route(mode, dy_dtype, lhs_dtype, cout, K, has_col, addrs, deferring, has_out):
    """Which launch forms dW[cout, K] = dy^T . lhs.  Pure: launches and allocates nothing.  ``dy_dtype``: ops.SplitImage.dtype
    for a split image; ``has_col``: lhs is an im2col matrix; ``addrs``: base addresses of dy, lhs and, when given, the dW
    destination; ``deferring``: the caller collects products for a grouped launch; ``has_out``: a dW destination was given."""
    if dy_dtype == ops.SplitImage.dtype:
        return "split_slabs"
    if lhs_dtype == torch.float32 and K <= 8 and not has_col and ops.pointnet_in_ok(K, cout):
        return "pointnet_in"
    if (mode == "bf16" and dy_dtype == torch.bfloat16 and lhs_dtype == torch.bfloat16
            and cout >= 256 and K >= 128 and cout % 8 == 0 and K % 8 == 0):
        return "bf16"
    # the grouped launch stages 16-B quads of both operands: cout % 4, K % 4 and 16-B aligned bases (ADVICE round 4:
    # channel counts outside the product's own, e.g. DilTempConv1d(6, 10), keep the per-layer product)
    if (deferring and cout % 4 == 0 and K % 4 == 0 and all(a % 16 == 0 for a in addrs)
            and dy_dtype == torch.float32 and lhs_dtype == torch.float32):
        return "grouped"
    return "fp32_aside" if has_out else "fp32_inline"


def _wgrad_split_k(route, cout, K, rows):
    """split-K factor of a weight-gradient route (pure); a split image contracts over 3 * rows: hi.hi + lo.hi + hi.lo"""
    if route in ("split_slabs", "bf16"):
        return ops.pick_split_k(cout, K, 3 * rows if route == "split_slabs" else rows, target_blocks=256, bk=64, tile=256)
    return ops.pick_split_k(cout, K, rows)


def _layer_wgrad(dy, lhs, s, mode, dW_out, defer_wgrad):
    """Second stage: dW[cout, K] = dy^T . lhs (contraction over the rows: both operands row-contiguous).  ``defer_wgrad``: list
    that takes (dy, lhs, dW, split_k) of a product the caller launches together with its siblings (dtc_backward: grouped)."""
    rows, cout = s.y.shape
    K = lhs.shape[1]
    addrs = () if defer_wgrad is None else tuple(t.data_ptr() for t in (dy, lhs, dW_out) if isinstance(t, torch.Tensor))
    route = _wgrad_route(mode, dy.dtype, lhs.dtype, cout, K, s.col is not None, addrs, defer_wgrad is not None,
                         dW_out is not None)
    if route == "pointnet_in":
        return ops.pointnet_in_wgrad(dy, lhs, out=dW_out, out_is_zero=True)
    sk = _wgrad_split_k(route, cout, K, rows)
    if route == "split_slabs":
        return ops.gemm_slabs_split3(dy, lhs, cout, K, rows, sk, out=dW_out)
    if route == "bf16":
        if sk > 1:
            # the slab sum only feeds the optimizer: off the main stream (joined before the encoder's Adam)
            return ops.gemm_slabs(dy, RC, lhs, RC, cout, K, rows, sk, out=dW_out, math=PCAA_BF16,
                                  reduce_ctx=_on_wgrad_stream if dW_out is not None else None)
        return ops.gemm(dy, RC, lhs, RC, cout, K, rows, out=dW_out, math=PCAA_BF16)
    if route == "grouped":
        dW = dW_out if dW_out is not None else torch.zeros((cout, K), dtype=torch.float32, device=dy.device)
        defer_wgrad.append((dy, lhs, dW, sk))
        return dW
    if route == "fp32_aside":
        with _on_wgrad_stream(dy, lhs):
            return ops.gemm(dy, RC, lhs, RC, cout, K, rows, out=dW_out, split_k=sk, accumulate=True, math=PCAA_F32)
    return ops.gemm(dy, RC, lhs, RC, cout, K, rows, out=None, split_k=sk, accumulate=sk > 1, math=PCAA_F32)


# The dgrad by the image dy arrives in: (maker of the W^T image where the layer's save holds none; dtype of the y below that the fused
# op -- ELU' and the BatchNorm-backward statistics of the layer below in the epilogue -- takes, its predicate, that op; the plain op)
_DGRAD_IMAGE = {
    "split": (lambda W2d: ops.split_f16(W2d, transpose=True), torch.float32,
              ops.gemm_dgrad_bn_split3_supported, ops.gemm_dgrad_bn_split3,
              lambda dy, wt, rows, K, cout: ops.gemm_split3(dy, wt, KC, rows, K, cout)),
    "bf16": (lambda W2d: ops.cast_bf16(W2d, False, True)[1], torch.bfloat16,
             ops.gemm_dgrad_bn_supported, ops.gemm_dgrad_bn,
             lambda dy, wt, rows, K, cout: ops.gemm(dy, KC, wt, KC, rows, K, cout, out_dtype=torch.bfloat16,
                                                    math=PCAA_BF16)),
}


def _dgrad_route(mode, adjoint, forms_dy=False, da_fused=False, dy_dtype=None, rows=0, cout=0, K=0, below_y=None, below_has_mean=False):
    """Which launch forms d_lhs[rows, K] = dy . W.  Pure: launches and allocates nothing.  ``adjoint``: the caller has an
    adjoint of its own -- the route is then known before dy is: with ``forms_dy`` it forms dy itself from a _FusedGrad
    (``da_fused``).  Without one it follows from dy: ``below_y`` is the (shape, dtype) of the stored y of the layer that
    produced lhs, or None; ``below_has_mean``: that layer's save is a train-mode one."""
    if adjoint:
        return "adjoint_dy" if (forms_dy and da_fused) else "adjoint"
    if dy_dtype == ops.SplitImage.dtype:
        image = "split"
    elif mode == "bf16" and dy_dtype == torch.bfloat16 and cout % 8 == 0:
        image = "bf16"
    else:
        return "fp32"
    y_dtype, supported = _DGRAD_IMAGE[image][1:3]
    if (below_y is not None and below_has_mean and below_y[1] == y_dtype and tuple(below_y[0]) == (rows, K)
            and supported(rows, K, cout)):
        return image + "_bn"
    return image


def _layer_dgrad(dy, W2d, s, mode, below, adjoint):
    """Third stage: d_lhs = dy . W, through ``adjoint`` (the caller's own; temporal block: implicit col2im) if given"""
    if adjoint is not None:
        return adjoint.from_dy(dy)
    rows, cout = s.y.shape
    K = W2d.shape[1]
    bs, below_bn, below_outs = below if below is not None else (None, None, None)
    below_y = (bs.y.shape, bs.y.dtype) if bs is not None and bs.y is not None else None
    route = _dgrad_route(mode, False, dy_dtype=dy.dtype, rows=rows, cout=cout, K=K, below_y=below_y,
                         below_has_mean=bs is not None and bs.mean is not None)
    if route == "fp32":
        return ops.gemm(dy, KC, W2d, RC, rows, K, cout, out_dtype=torch.float32)
    image, _, with_bn = route.partition("_")
    make, _, _, fused_op, plain_op = _DGRAD_IMAGE[image]
    wt, s.wt = s.wt, None            # the image of W^T [K, cout] the forward made: read once, so it dies with this launch
    if wt is None:
        wt = make(W2d)
    if not with_bn:
        return plain_op(dy, wt, rows, K, cout)
    btail = _bwd_tail(bs, below_bn, below_outs, K)
    return _FusedGrad(*fused_op(dy, wt, bs.y, bs.scale, bs.shift, bs.mean, bs.rstd, tail=btail), fin=btail.out)


def _bn_layer_backward(s, bn, W2d, mode, lhs, da=None, pool=None, need_dinput=True, outs=None, below=None,
                       adjoint=None, defer_wgrad=None, lin_bias=None, dbias_out=None):
    """Backward of one (linear, BN, ELU) layer.  ``lhs`` is the GEMM's left operand ([rows, K]: the input activation or
    the im2col matrix).  ``outs`` = (dW, dgamma, dbeta) destination views (dW PRE-ZEROED: the trainer's flat gradient
    buffer) or None to allocate.  ``da`` may be a _FusedGrad (the dgrad of the layer above already applied ELU' and reduced
    the statistics); ``pool`` = (dpool, group_rows, pool_scale) instead of ``da`` when the layer's output was mean-pooled.
    ``below`` = (save, bn, outs) of the layer that produced ``lhs`` -- if it qualifies, this layer's dgrad is fused with
    the first half of ITS backward and a _FusedGrad is returned as d_lhs.  ``adjoint``: the caller's own dgrad instead
    (_DtcAdjoint: ``from_dy(dy) -> d_lhs`` and, where ``forms_dy``, ``forming_dy(dz, y, coef) -> (d_lhs, dy)``).
    With an eval-mode save (``s.mean is None``) the linear bias ``lin_bias`` in front of the BatchNorm has a gradient, dbias =
    scale*dbeta (written to ``dbias_out`` when given); in train mode dbias is None (analytically zero: the batch mean removes it).
    Returns (dW2d, dgamma, dbeta, dbias, d_lhs or None)."""
    # the caller's adjoint, where it forms dy itself, replaces the tail of the first stage; any other route follows from dy
    forms_dy = need_dinput and adjoint is not None and _dgrad_route(
        mode, True, adjoint.forms_dy, s.mean is not None and isinstance(da, _FusedGrad)) == "adjoint_dy"
    dy, dgamma, dbeta, dbias, d_lhs = _bn_dy(s, bn, da, pool, isinstance(lhs, ops.SplitImage), outs, lin_bias,
                                             dbias_out, adjoint_dy=adjoint if forms_dy else None)
    dW = _layer_wgrad(dy, lhs, s, mode, outs[0].view(s.y.shape[1], lhs.shape[1]) if outs else None, defer_wgrad)
    if need_dinput and d_lhs is None:
        d_lhs = _layer_dgrad(dy, W2d, s, mode, below, adjoint)
    return dW, dgamma, dbeta, dbias, d_lhs


_PN_NAMES = ("module.0.weight", "module.0.bias", "module.1.weight", "module.1.bias")
_DTC_NAMES = ("conv1d.weight", "conv1d.bias", "batch_norm.weight", "batch_norm.bias")


def _layer_outs(gout, prefix, names):
    """-> ((dW, dgamma, dbeta) destinations, linear-bias destination) of the layer whose parameters are ``names``"""
    if gout is None:
        return None, None
    return (gout[prefix + names[0]], gout[prefix + names[2]], gout[prefix + names[3]]), gout[prefix + names[1]]


def _layer_grads(names, conv, dW, dgamma, dbeta, dbias, bias_out):
    """one layer's {parameter-name suffix: gradient}.  The linear bias: in train mode its gradient is analytically zero
    (BatchNorm removes the mean) -- the pre-zeroed destination, or zeros; in eval mode ``dbias`` = scale * dbeta"""
    zb = dbias if dbias is not None else (bias_out if bias_out is not None else torch.zeros_like(conv.bias))
    return {names[0]: dW.view_as(conv.weight), names[1]: zb, names[2]: dgamma, names[3]: dbeta}


def _in_bwd_route(y_stored, train_save, has_da, need_in, da_fused, da_dtype, mode, dW_contiguous):
    """How pointnet_backward differentiates a layer.  Pure: launches and allocates nothing.  "general": _bn_layer_backward
    (y is stored, or the save is an eval-mode one, or the layer was pooled, or the gradient w.r.t. its input is wanted);
    else the recompute path of the first layer, which reads the incoming gradient and the points and nothing else: "fused"
    (the dgrad above already applied ELU' and reduced the statistics: one pass), "onepass" (bf16 and fp16x3 modes, a
    contiguous dW destination given: statistics and G = dz^T.x from ONE read of da, the weight gradient then a combination of
    G with the points' second moments) or "two_pass" (exact-fp32 mode: dy is formed per element before the contraction, as
    the oracle's autograd does)."""
    if y_stored or not train_save or not has_da or need_in:
        return "general"
    if da_fused:
        return "fused"
    if (da_dtype == torch.bfloat16 or (mode == "fp16x3" and da_dtype == torch.float32)) and dW_contiguous:
        return "onepass"
    return "two_pass"


def _in_recompute_backward(route, da, s, bn, W2d, outs):
    """(dW, dgamma, dbeta) of the recompute first layer by a route of _in_bwd_route other than "general" """
    dW_out = outs[0].view(s.cout, s.cin) if outs else None
    fused = route == "fused"
    if fused:
        coef, dg, db = _fused_coefficients(da, s, bn, outs)
    else:
        tail = _bwd_tail(s, bn, outs, s.cout)
        if route == "onepass":
            dW = ops.pointnet_in_bwd_onepass(da, s.a_in, W2d, s.scale, s.shift, s.mean, s.rstd, tail, mom=s.mom, out=dW_out)
            _, dg, db = tail.out
            return dW, dg, db
        ops.pointnet_in_bwd_stats(da, s.a_in, W2d, s.scale, s.shift, s.mean, s.rstd, tail=tail)
        coef, dg, db = tail.out
    dW = ops.pointnet_in_bwd_wgrad(da.dz if fused else da, s.a_in, W2d, s.scale, s.shift, coef,
                                   out=dW_out, out_is_zero=True, dz_is_pre=fused)
    return dW, dg, db


def pointnet_backward(saves, layers, mode, d_last=None, dpool=None, pool_rows=0, need_dx=False, gout=None,
                      prefix="pc_block.pointnet", ragged=None):
    """Returns ({param_name_suffix: grad} per layer list, dx2d or None).  ``gout``:
    optional {state_dict name: pre-zeroed gradient view} to write into.  ``ragged`` (a _RaggedPool, with ``dpool``; eval-mode
    saves of a ``last_pre_bn`` forward): the last layer was pooled by ops.segment_weighted_mean instead of over groups of
    ``pool_rows`` rows."""
    grads = []
    da = d_last
    for li in range(len(layers) - 1, -1, -1):
        layer, s = layers[li], saves[li]
        conv, bn = layer.module[0], layer.module[1]
        W2d = conv.weight.view(s.cout, s.cin)
        need_in = li > 0 or need_dx
        outs, bias_out = _layer_outs(gout, f"{prefix}{li + 1}.", _PN_NAMES)
        route = _in_bwd_route(s.y is not None, s.mean is not None, da is not None, need_in, isinstance(da, _FusedGrad),
                              getattr(da, "dtype", None), mode, outs is not None and outs[0].is_contiguous())
        if route != "general":
            dW, dg, db = _in_recompute_backward(route, da, s, bn, W2d, outs)
            dbias = dprev = None
        else:
            pooled = li == len(layers) - 1 and dpool is not None
            if s.y is None and not pooled:
                # recompute layer, but the caller wants the gradient w.r.t. the points, or the save is an eval-mode one
                # (which takes the general route): rebuild y from the points
                s.y = ops.pointnet_in_fwd(s.a_in, W2d, None, da.dtype)
            below = (saves[li - 1], layers[li - 1].module[1],
                     _layer_outs(gout, f"{prefix}{li}.", _PN_NAMES)[0]) if li > 0 else None
            dW, dg, db, dbias, dprev = _bn_layer_backward(s, bn, W2d, mode, s.a_in, da=None if pooled else da,
                                                          pool=((dpool, ragged, 1.0) if ragged is not None else
                                                                (dpool, pool_rows, 1.0 / pool_rows)) if pooled else None,
                                                          need_dinput=need_in, outs=outs, below=below,
                                                          lin_bias=conv.bias, dbias_out=bias_out)
        grads.append(_layer_grads(_PN_NAMES, conv, dW, dg, db, dbias, bias_out))
        da = dprev
    grads.reverse()
    return grads, da


_FUSE_DTC = True


_DtcFwd = collections.namedtuple("_DtcFwd", "fused ksplit bf16 route keep_col window")
_DtcBwd = collections.namedtuple("_DtcBwd", "fused ksplit bf16 route epilogue forms_dy")


def _dtc_launch(adjoint, mode, B, cin, cout, windowed=False):
    """(ksplit, bf16, route) of one fused launch, each the library's answer.  ``bf16`` (the _bf16 entry point) in the bf16
    throughput mode where the two-sequence kernels would take the layer at ksplit 1: exact fp32 products elsewhere"""
    ksplit = ops.dtc_conv_ksplit(adjoint, B, cin, cout)
    bf16 = mode == "bf16" and ops.dtc_conv_route(adjoint, True, B, cin, cout, 1).startswith("pair")
    return ksplit, bf16, ops.dtc_conv_route(adjoint, bf16, B, cin, cout, ksplit, windowed)


@functools.lru_cache(maxsize=None)
def _dtc_plan(dims, B, T, training, want_bwd, mode, windowed, fuse, a_dtype):
    """What dtc_forward and dtc_backward launch.  Pure: plain values in, launches and allocates nothing, and every rule is
    the library's (device-free queries; they never change within a process, hence the cache).  ``dims``: (cin, cout) of
    each layer; ``training``: train-mode BatchNorm (backward: the saves are train-mode ones); ``windowed``: the source is a
    frame table read through window rows; ``fuse``: _FUSE_DTC; ``a_dtype``: dtype of the block's input.
    Returns (fwd, bwd), one entry per layer.  _DtcFwd: ``fused`` (one launch per layer -- every layer or none; else im2col +
    _linear_bn), the launch's ``ksplit``, ``bf16`` flag and ``route`` (a name of ops.DTC_ROUTES), ``keep_col`` (the save
    holds the im2col matrix) and ``window``: None, or on the first layer of a windowed source "in_place" (its launch reads
    the table) / "gather" (the windows are written out first).  _DtcBwd: ``fused`` (the adjoint in one launch; else
    dy . W and col2im), its ``ksplit``, ``bf16`` and ``route``, ``epilogue`` (the BatchNorm backward of the layer below
    rides in it) and ``forms_dy`` (it forms dy from dz itself).
    The bf16 flag is asked at ksplit 1 but the forward's pair kernels need ksplit == 1: a wide layer with few long tiles
    (512 -> 64 channels at B = 64: ksplit 8) takes the one-sequence bf16 kernel, measured no faster than fp32
    (docs/LAB_LOG.md section 9).  No shipped block has such a layer."""
    fwd_fused = fuse and a_dtype == torch.float32 and all(ops.dtc_conv_supported(T, cin, cout) for cin, cout in dims)
    fwd, bwd = [], []
    for li, (cin, cout) in enumerate(dims):
        window = ("in_place" if fwd_fused else "gather") if windowed and li == 0 else None
        ks, bf16, route = _dtc_launch(False, mode, B, cin, cout, window is not None) if fwd_fused else (0, False, None)
        fwd.append(_DtcFwd(fwd_fused, ks, bf16, route, not fwd_fused or training or want_bwd, window))
        bwd_fused = fuse and ops.dtc_conv_dgrad_supported(T, cin, cout)
        ks, bf16, route = _dtc_launch(True, mode, B, cin, cout) if bwd_fused else (0, False, None)
        bwd.append(_DtcBwd(bwd_fused, ks, bf16, route, li > 0 and ks == 1 and training, ks == 1))
    return tuple(fwd), tuple(bwd)


def dtc_forward(a2d, B, T, layers, training, pool_time, mode="fp32", win_row=None, ring_rows=0, consts=None,
                want_bwd=False):
    """a2d: [B*T, Cin] fp32 rows (b,t).  Causal dilated conv = (implicit) im2col + contraction.
    ``win_row`` (ops.WindowRows, eval only): a2d is a frame-feature table [table_rows, Cin] instead and sequence b is
    its T rows from win_row[b] on (modulo ``ring_rows`` if > 0).  Only the first layer reads the table: fused, through
    the windowed form of its launch; otherwise the windows are written out with one gather and today's path runs.
    ``consts`` (eval only): the encoder's EncoderEvalConstants, used instead of recomputing the BatchNorm coefficients.
    ``want_bwd`` (matters in eval mode only): a backward will follow, so the fused launch also writes the im2col matrix
    dtc_backward contracts with; off, the eval forward is unchanged."""
    if consts is not None and training:
        raise ValueError("dtc_forward: consts are eval-mode constants")
    if win_row is not None and want_bwd:
        raise ValueError("dtc_forward: the windowed form has no backward")
    saves = []
    a = a2d
    nl = len(layers)
    dims = tuple((l.conv1d.weight.shape[1], l.conv1d.weight.shape[0]) for l in layers)
    plan = _dtc_plan(dims, B, T, training, want_bwd, mode, win_row is not None, _FUSE_DTC, a2d.dtype)[0]
    if win_row is not None:
        if training:
            raise ValueError("dtc_forward: win_row is an eval-mode form (train-mode BatchNorm needs every row's statistics)")
        if ring_rows != win_row.ring_rows or len(win_row) != B or win_row.T != T or win_row.table_rows != a2d.shape[0]:
            raise ValueError("dtc_forward: win_row does not describe B windows of T rows of this table / ring_rows")
        if plan[0].window == "gather":
            a = ops.gather_frames(a2d.contiguous(), win_row.row_index())
    prev = None          # (scale, shift) of the layer whose bias-free output `a` is (fused path)
    for li, (layer, p) in enumerate(zip(layers, plan)):
        conv, bn = layer.conv1d, layer.batch_norm
        cin, cout = dims[li]
        W2d = conv.weight.view(cout, cin * 3)
        if p.fused:
            # one launch: implicit im2col + BN/ELU of the previous layer on load + contraction + statistics
            stats = ops.new_stats(cout, a.device) if training else None
            tail = ops.BnTailFwd(a.shape[0], conv.bias, bn, cout, sync=_sync_fn()) if training else None
            y, col = ops.dtc_conv_fwd(a, prev[0] if prev else None, prev[1] if prev else None, W2d, B, T,
                                      layer.dilation, stats=stats, want_col=p.keep_col, tail=tail, bf16=p.bf16,
                                      win_row=win_row if p.window == "in_place" else None, ksplit=p.ksplit)
            if training:
                scale, shift, mean, rstd = tail.out
                count = tail.count_out
            else:
                scale, shift = _eval_coeffs(consts, bn, cout, conv.bias)
                mean = rstd = None
                count = y.shape[0]
            a_in = None
        else:
            col = ops.dtc_im2col(a, B, T, cin, layer.dilation)
            y, scale, shift, mean, rstd, count, _ = _linear_bn(col, W2d, conv.bias, bn, training, "fp32", False,
                                                               consts if not training else None)
            a_in = a
        s = _LayerSave(a_in, col, y, scale, shift, mean, rstd, count, cin, cout, layer.dilation)
        saves.append(s)
        if li == nl - 1 and pool_time:
            if training:
                out, s.pool_e = ops.bn_act_meanpool_fwd(y, scale, shift, B, T, mean, rstd)
                return out, saves
            return ops.bn_act_meanpool_fwd(y, scale, shift, B, T), saves
        if p.fused and li < nl - 1:
            a, prev = y, (scale, shift)
        else:
            a = ops.bn_act_fwd(y, scale, shift)
    return a, saves


class _DtcAdjoint:
    """The adjoint of one fused temporal layer w.r.t. its input in one launch (implicit col2im), as its _DtcBwd plans it.
    With ``sb`` / ``btail`` (save and finalize of the layer below) the first half of that layer's BatchNorm+ELU backward
    rides in the epilogue -- dz and the two column sums: it then starts at bn_bwd_finalize -- and d_lhs is a _FusedGrad."""
    __slots__ = ("forms_dy", "btail", "launch")

    def __init__(self, p, W2d, B, T, s, sb, btail):
        self.forms_dy, self.btail = p.forms_dy, btail
        self.launch = functools.partial(ops.dtc_conv_dgrad, W2d=W2d, B=B, T=T, cin=s.cin, dilation=s.dil, tail=btail,
                                        below=(sb.y, sb.scale, sb.shift, sb.mean, sb.rstd) if sb else None,
                                        bf16=p.bf16, ksplit=p.ksplit)

    def forming_dy(self, dz, y, coef):
        """dy = c0*dz + c1*y + c2 formed while the operand is staged, and handed back -> (d_lhs, dy)"""
        return self._run(None, dz=dz, y=y, coef=coef, want_dy=True)

    def from_dy(self, dy):
        return self._run(dy)[0]

    def _run(self, dy, **formed):
        out, stats, dy = self.launch(dy, **formed)
        return (out if self.btail is None else _FusedGrad(out, stats, fin=self.btail.out)), dy


def dtc_backward(saves, layers, B, T, d_last=None, dpool=None, need_dx=True, gout=None, prefix="tc_block.dtc", mode="fp32"):
    grads = []
    defer = []
    da = d_last
    plan = _dtc_plan(tuple((s.cin, s.cout) for s in saves), B, T, saves[0].mean is not None, True, mode, False, _FUSE_DTC,
                     torch.float32)[1]
    for li in range(len(layers) - 1, -1, -1):
        layer, s, p = layers[li], saves[li], plan[li]
        conv, bn = layer.conv1d, layer.batch_norm
        W2d = conv.weight.view(s.cout, s.cin * 3)
        need_in = li > 0 or need_dx
        outs, bias_out = _layer_outs(gout, f"{prefix}{li + 1}.", _DTC_NAMES)
        adjoint = None                      # else dcol = dy . W, then col2im
        if p.fused:
            sb = saves[li - 1] if p.epilogue else None
            btail = _bwd_tail(sb, layers[li - 1].batch_norm, _layer_outs(gout, f"{prefix}{li}.", _DTC_NAMES)[0],
                              s.cin) if p.epilogue else None
            adjoint = _DtcAdjoint(p, W2d, B, T, s, sb, btail)
        pooled = li == len(layers) - 1 and dpool is not None
        dW, dg, db, dbias, dcol = _bn_layer_backward(s, bn, W2d, "fp32", s.col, da=None if pooled else da,
                                                     pool=(dpool, T, 1.0 / T) if pooled else None, need_dinput=need_in,
                                                     outs=outs, adjoint=adjoint, defer_wgrad=defer, lin_bias=conv.bias,
                                                     dbias_out=bias_out)
        grads.append(_layer_grads(_DTC_NAMES, conv, dW, dg, db, dbias, bias_out))
        if not need_in:
            da = None
        elif p.fused:
            da = dcol                       # already the gradient w.r.t. the layer's input
        else:
            da = ops.dtc_col2im(dcol, B, T, s.cin, s.dil)
    if defer:
        # the block's weight gradients dW_l = dy_l^T . col_l, all in one launch behind the dgrad chain (round 4: they were
        # six launches of 26-47 us in a chain beside it; measured without them the N = 32 step was 0.17 ms shorter)
        # (exact fp32: bf16 operands on the 256x256-tile kernel measured no better in round 4 -- N=32 2.16 against 2.11 ms)
        tensors = [t for d in defer for t in d[:3]]
        for k in range(0, len(defer), 8):
            with _on_wgrad_stream(*tensors):
                ops.gemm_group_rc_f32(defer[k:k + 8])
    grads.reverse()
    return grads, da


# ======================================================================
# small dense layers (Linear + ELU): MLP heads, projection heads, decoder
# ======================================================================
def _wide_bf16(mode, M, N, K):
    """Route a dense layer through the 256x256-tile bf16 MFMA kernel: only the
    weight-streaming decoder layers qualify (bf16 throughput mode, wide, 8-aligned)."""
    return mode == "bf16" and N >= 512 and K >= 512 and N % 8 == 0 and K % 8 == 0 and M % 8 == 0


def _skinny(mode, M, N, K):
    """Batch-skinny streaming kernels (gemm_skinny.hip): bf16 throughput mode, M <= 64 rows."""
    return mode == "bf16" and ops.skinny_supported(M, N, K)


def _skinny_exact(mode, M, N, K):
    """The same kernels with fp32 products (the parity modes): round 3 -- before, those modes ran the decoder on the
    128x128-tile fp32 GEMM (half of every tile padding; the weight gradient, a 64-deep contraction, 2-3 ms per step)."""
    return mode in ("fp32", "fp16x3") and ops.skinny_supported(M, N, K)


def linear_act_forward(x, lin, act, mode="fp32", W16=None):
    """act(x @ W^T + b); x [M,K] fp32 -> [M,N] fp32.  fp32 MFMA, or (bf16 mode,
    wide layers) bf16 MFMA with fp32 accumulation: the layer is bound by
    streaming W from HBM either way, the bf16 pipe just keeps the MFMA time out
    of the way of the stream."""
    M, K = x.shape
    N = lin.weight.shape[0]
    if _skinny(mode, M, N, K):
        # W16: the weight's bf16 image, passed by a caller that vouches for it (PCAATrainer._refresh_w16): same result
        return ops.skinny_linear_fwd(x, lin.weight, lin.bias, act, W16=W16)
    if _skinny_exact(mode, M, N, K):
        return ops.skinny_linear_fwd(x, lin.weight, lin.bias, act, exact=True)
    if _wide_bf16(mode, M, N, K):
        sk = ops.pick_split_k(M, N, K, target_blocks=256, bk=64, tile=256)
        y = ops.gemm(x, KC, lin.weight, KC, M, N, K, split_k=sk, accumulate=True, math=PCAA_BF16)
        return ops.bias_act_(y, lin.bias, act)
    sk = ops.pick_split_k(M, N, K)
    if sk > 1:
        y = ops.gemm(x, KC, lin.weight, KC, M, N, K, split_k=sk, accumulate=True)
        return ops.bias_act_(y, lin.bias, act)
    y = ops.gemm(x, KC, lin.weight, KC, M, N, K, bias=lin.bias if act == ACT_NONE else None)
    if act != ACT_NONE:
        ops.bias_act_(y, lin.bias, act)
    return y


def linear_act_backward(x, a_out, lin, act, d_out, need_dx=True, dW_out=None, db_out=None, dx_init=None,
                        mode="fp32", d_is_pre=False, fuse_elu_in=False, update=None, W16=None, defer_db=None):
    """d_out is the gradient w.r.t. the layer output (d_is_pre: already w.r.t. its
    pre-activation).  Returns (dW, db, dx).  fuse_elu_in (skinny path only, x = ELU output of
    the layer below): dx is multiplied by ELU'(x), i.e. it is the gradient w.r.t. that layer's
    pre-activation -- the caller passes it on with d_is_pre=True.
    ``update`` (skinny path only): callable ``update(dz, x)`` that forms the weight gradient AND applies the
    optimizer to the weight in one kernel (ops.skinny_linear_wgrad_adam_) LATER -- the callback itself must not touch the
    weight: it is called before the layer's dgrad, which reads it -- and dW is returned as None.
    ``defer_db`` (a list; with ``update`` and a ``db_out`` destination): the bias gradient's column sum is not launched here
    but noted as (dz, db_out) for the caller to launch later (decoder_backward: all of them behind ONE hand-over to the
    weight-gradient stream -- every hand-over is an event record on this stream, ~7 us of idle queue between two kernels)."""
    M, K = x.shape
    N = lin.weight.shape[0]
    dz = ops.elu_bwd_from_out(d_out, a_out) if (act == ACT_ELU and not d_is_pre) else d_out
    dz2 = dz.view(M, N)
    if update is not None:
        if not (_skinny(mode, M, N, K) or _skinny_exact(mode, M, N, K)):
            raise RuntimeError("linear_act_backward: a fused weight update is only served by the skinny path")
        if defer_db is not None and db_out is not None and _WGRAD_STREAM is not None:
            defer_db.append(((dz2,), lambda dz2=dz2, db_out=db_out: ops.colsum(dz2, out=db_out)))
            db = db_out
        else:
            with _on_wgrad_stream(dz2):
                db = ops.colsum(dz2, out=db_out)
        # the callback only NOTES the operands (single process: the kernels run later, on the Adam side stream, once the whole
        # decoder backward -- whose dgrads read the weights they overwrite -- is enqueued) or packs and sends them (data
        # parallel); nothing in it writes the weight, so it runs ahead of this layer's dgrad and the pack + all-gather of
        # the data-parallel step leave while the dgrad streams the weight
        update(dz2, x)
        dx = None
        if need_dx:
            dx = ops.skinny_linear_dgrad(dz2, lin.weight, a_prev=x if fuse_elu_in else None, out=dx_init,
                                         accumulate=dx_init is not None, exact=_skinny_exact(mode, M, N, K),
                                         W16=W16)
        return None, db, dx
    exact = _skinny_exact(mode, M, N, K)
    if _skinny(mode, M, N, K) or exact:
        if dW_out is not None and db_out is not None and defer_db is not None and _WGRAD_STREAM is not None:
            # (decoder_backward's one hand-over to the weight-gradient stream takes this layer's two products as well)
            def both(dz2=dz2, x=x, db_out=db_out, dW_out=dW_out, exact=exact):
                ops.colsum(dz2, out=db_out)
                ops.skinny_linear_wgrad(dz2, x, out=dW_out, exact=exact)
            defer_db.append(((dz2, x), both))
            db, dW = db_out, dW_out
        elif dW_out is not None and db_out is not None:
            # the weight-gradient write stream (and the bias gradient) beside the dgrad read stream of the same layer
            with _on_wgrad_stream(dz2, x):
                db = ops.colsum(dz2, out=db_out)
                dW = ops.skinny_linear_wgrad(dz2, x, out=dW_out, exact=exact)
        else:
            db = ops.colsum(dz2, out=db_out)
            dW = ops.skinny_linear_wgrad(dz2, x, out=dW_out, exact=exact)
        dx = None
        if need_dx:
            dx = ops.skinny_linear_dgrad(dz2, lin.weight, a_prev=x if fuse_elu_in else None, out=dx_init,
                                         accumulate=dx_init is not None, exact=exact, W16=W16)
        return dW, db, dx
    if fuse_elu_in:
        raise RuntimeError("linear_act_backward: fuse_elu_in is only served by the skinny path")
    db = ops.colsum(dz2, out=db_out)
    wide = _wide_bf16(mode, M, N, K)
    if dW_out is not None and not wide:
        with _on_wgrad_stream(dz2, x):
            dW = ops.gemm(dz2, RC, x, RC, N, K, M, out=dW_out, math=PCAA_F32)
    else:
        dW = ops.gemm(dz2, RC, x, RC, N, K, M, out=dW_out, math=PCAA_BF16 if wide else PCAA_F32)
    dx = None
    if need_dx:
        if wide:
            sk = ops.pick_split_k(M, K, N, target_blocks=256, bk=64, tile=256)
            math = PCAA_BF16
        else:
            sk = ops.pick_split_k(M, K, N)
            math = PCAA_F32
        if dx_init is not None:
            dx = ops.gemm(dz2, KC, lin.weight, RC, M, K, N, out=dx_init, split_k=sk, accumulate=True, math=math)
        else:
            dx = ops.gemm(dz2, KC, lin.weight, RC, M, K, N, split_k=sk, accumulate=sk > 1 or wide, math=math)
    return dW, db, dx


# ======================================================================
# CGEncoder (models.py:232-292)
# ======================================================================
class EncoderState:
    pass


def _heads_mods(enc, gph):
    l1 = enc.MLP_sup1[0]
    lh = enc.MLP_head[0] if enc.use_projection_head else None
    l2 = enc.MLP_sup2[0]
    lg = gph[0] if gph is not None else None
    return l1, lh, l2, lg


def _heads_fusable(enc, gph, B, backward):
    l1, lh, l2, lg = _heads_mods(enc, gph)
    return ops.heads_supported(B, l2.weight.shape[0], l1.weight.shape[1], l1.weight.shape[0],
                               lh.weight.shape[0] if lh is not None else 0,
                               lg.weight.shape[0] if lg is not None else 0, backward) and \
        l2.weight.shape[1] == (lh.weight.shape[0] if lh is not None else l1.weight.shape[0]) and \
        (lg is None or lg.weight.shape[1] == l1.weight.shape[0]) and \
        (lh is None or lh.weight.shape[1] == l1.weight.shape[0])


def _check_encoder_input(enc, C, N):
    """C features per point and N points per frame are the ones ``enc`` was built for"""
    cin = enc.pc_block.pointnet1.module[0].weight.shape[1]
    if C != cin:
        raise RuntimeError(f"CGEncoder: input has {C} features, first layer expects {cin}")
    if N != enc.nmax_points:
        raise RuntimeError(f"CGEncoder: N={N} points but nmax_points={enc.nmax_points} "
                           "(the reference's AvgPool2d((1,nmax_points)) would emit >1 column)")


def _check_encoder_frames(enc, frames, who):
    """point-major frames [n,N,C] on the device (frame_table.check_frames, none empty) of the shape ``enc`` was built for"""
    frame_table.check_frames(frames, who, empty_ok=False)
    _check_encoder_input(enc, frames.shape[2], frames.shape[1])


def _check_encoder_ragged(enc, rows, weight, u_off, n, N, who):
    """a compact table (frame_table.check_ragged) of the shape ``enc`` was built for"""
    _, C = frame_table.check_ragged(rows, weight, u_off, n, N, who)
    _check_encoder_input(enc, C, int(N))


def encoder_forward(enc, x, training, mode=None, gph=None, want_bwd=False):
    """``gph``: optional decoder projection head ``Sequential(Linear(32,64), ELU)`` evaluated in the
    same launch as the MLP heads (``st.hproj``).  ``want_bwd``: encoder_backward will follow -- in eval mode the two
    blocks then keep what it reads (pointnet_forward / dtc_forward); a train-mode forward always does."""
    mode = get_precision() if mode is None else mode
    frame_table.check_crops(x, "CGEncoder", empty_ok=False)
    B, C, T, N = x.shape
    _check_encoder_input(enc, C, N)
    st = EncoderState()
    st.B, st.C, st.T, st.N, st.mode, st.training, st.want_bwd = B, C, T, N, mode, training, training or want_bwd
    xp = _point_major(x).view(B * T * N, C)
    st.xp = xp
    mark("enc_fwd.begin")
    x2, st.pn = pointnet_forward(xp, enc.pc_block.layers(), training, mode, pool_rows=N, want_bwd=want_bwd)   # [B*T, 1024]
    st.x2 = x2
    mark("enc_fwd.pointnet")
    x4, st.dtc = dtc_forward(x2, B, T, enc.tc_block.layers(), training, pool_time=True, mode=mode,
                             want_bwd=want_bwd)                                                        # [B, 512]
    st.x4 = x4
    mark("enc_fwd.dtc")
    return _encoder_heads(enc, st, x4, gph)


def _encoder_heads(enc, st, x4, gph=None):
    """x4 [B, 512] -> the MLP heads (models.py:252-277, 284-292); fills st, returns (logits, sup_fv, st)."""
    B = x4.shape[0]
    st.h = st.hproj = None
    if _heads_fusable(enc, gph, B, False):
        m1, mh, m2, mg = _heads_mods(enc, gph)
        st.sup_fv, st.h, st.logits, st.hproj = ops.heads_fwd(
            x4, m1.weight, m1.bias, mh.weight if mh is not None else None, mh.bias if mh is not None else None,
            m2.weight, m2.bias, mg.weight if mg is not None else None, mg.bias if mg is not None else None)
        return st.logits, st.sup_fv, st
    st.sup_fv = linear_act_forward(x4, enc.MLP_sup1[0], ACT_ELU)
    h = st.sup_fv
    if enc.use_projection_head:
        st.h = linear_act_forward(st.sup_fv, enc.MLP_head[0], ACT_ELU)
        h = st.h
    st.logits = linear_act_forward(h, enc.MLP_sup2[0], ACT_ELU)
    if gph is not None:
        st.hproj = linear_act_forward(st.sup_fv, gph[0], ACT_ELU)
    return st.logits, st.sup_fv, st


def frame_pad_quantum(N, mode=None):
    """Frames per chunk must be a multiple of this for the eval PointNet to stay on the fused-epilogue GEMM in bf16 mode
    (pcaa_gemm_affine_elu takes whole 256-row tiles: U * N % 256 == 0); 1 where that path does not apply."""
    mode = get_precision() if mode is None else mode
    if not (mode == "bf16" and _epilogue_pools(N)):
        return 1
    return 256 // math.gcd(N, 256)


def encoder_frame_features(enc, frames, mode=None, consts=None):
    """Eval-mode PointNet block + mean over the points, frame by frame (models.py:82-105, 242-243, 279-282): point-major
    frames [U, N, C] fp32 -> ([U, 1024] fp32, saves).  A frame's features do not depend on its neighbours, which is what
    lets overlapping crops share them.  ``consts``: ``encoder_eval_constants(enc, mode)`` of a frozen encoder (same bits,
    the constants are not recomputed); None: they are computed in this call."""
    mode = get_precision() if mode is None else mode
    _check_encoder_frames(enc, frames, "encoder_frame_features")
    U, N, C = frames.shape
    return pointnet_forward(frames.view(U * N, C), enc.pc_block.layers(), False, mode, pool_rows=N, consts=consts)


def encoder_frame_features_ragged(enc, rows, weight, u_off, n, N, mode=None, consts=None):
    """``encoder_frame_features`` of n padded frames from their DISTINCT points (``ops.frames_from_raw_unique``): ``rows``
    [M, C] fp32, ``weight`` fp32 [M] (how often a row's point occurs in its padded frame), ``u_off`` int32 [n + 1] (frame
    f owns rows ``u_off[f] .. u_off[f + 1] - 1``) -> ([n, 1024] fp32, saves).  In eval mode the per-point network f is a
    pure function of the point, so the mean over a frame's N padded rows of f(row) is (1 / N) sum_i weight_i f(row_i): the
    eval PointNet layers run on the M compact rows with no pooling in the last layer, then ``ops.segment_weighted_mean``
    pools (and applies BatchNorm + ELU itself where the last layer left its pre-BatchNorm y: fp32 and fp16x3 modes).
    Eval mode and no gradient only: the saves do not serve pointnet_backward."""
    mode = get_precision() if mode is None else mode
    _check_track_eval(enc, "encoder_frame_features_ragged")
    _check_encoder_ragged(enc, rows, weight, u_off, n, N, "encoder_frame_features_ragged")
    if torch.is_grad_enabled() and (rows.requires_grad or any(p.requires_grad for p in enc.parameters())):
        raise RuntimeError("encoder_frame_features_ragged: forward only -- a backward is wanted (autograd is on and the "
                           "rows or the encoder's parameters require a gradient); call it under torch.no_grad(), or "
                           "differentiate encoder_frame_features on the padded frames")
    N = int(N)
    with torch.no_grad():
        a, saves = pointnet_forward(rows, enc.pc_block.layers(), False, mode, pool_rows=0, consts=consts, last_pre_bn=True)
        last = saves[-1]
        if last.y is not None:
            return ops.segment_weighted_mean(a, weight, u_off, N, last.scale, last.shift), saves
        return ops.segment_weighted_mean(a, weight, u_off, N), saves


def encoder_forward_windows(enc, table, win_row, T, mode=None, consts=None):
    """Eval-mode temporal block, mean over T and heads on windows of a frame-feature table [table_rows, 1024]
    (encoder_frame_features): window b = rows win_row[b] .. + T - 1 (an ops.WindowRows; its ring_rows > 0: modulo, its
    segments > 0: modulo inside the ring the window starts in).  ``consts``: as for encoder_frame_features.
    Returns (logits, sup_fv, st) as encoder_forward does for the materialised crops."""
    mode = get_precision() if mode is None else mode
    _require_gpu(table, "CGEncoder")
    B = len(win_row)
    st = EncoderState()
    st.B, st.T, st.mode, st.training = B, T, mode, False
    x4, st.dtc = dtc_forward(table, B, T, enc.tc_block.layers(), False, pool_time=True, mode=mode, win_row=win_row,
                             ring_rows=win_row.ring_rows, consts=consts)
    st.x4 = x4
    return _encoder_heads(enc, st, x4)


def encoder_backward(enc, st, d_logits, d_supfv, need_dx=False, gout=None,
                     gph=None, d_hproj=None, gph_gout=None, after_heads=None):
    """Returns ({state_dict-style name: grad}, dx [B,C,T,N] view or None).
    ``gout``: optional {name: gradient view}; split-K products accumulate into
    them, so they must arrive ZEROED (the trainer zeroes its flat buffer once).
    ``gph`` / ``d_hproj`` / ``gph_gout``: the decoder projection head evaluated by encoder_forward(gph=...),
    the gradient w.r.t. its output and optional (dW, db) destinations: its backward runs in the heads'
    launch; its gradients are returned under "GPH.0.weight" / "GPH.0.bias".
    An eval-mode state (encoder_forward(..., training=False, want_bwd=True)) differentiates the frozen-BatchNorm encoder:
    the running statistics are read, never written, and the biases in front of the BatchNorms get real gradients."""
    if not getattr(st, "want_bwd", st.training):
        raise RuntimeError("encoder_backward: this eval-mode forward kept nothing for a backward -- "
                           "call encoder_forward(..., want_bwd=True)")
    B, T, N = st.B, st.T, st.N
    g, dx4 = _encoder_heads_backward(enc, st, d_logits, d_supfv, gout, gph, d_hproj, gph_gout)
    mark("enc_bwd.heads")
    if after_heads is not None:
        after_heads()            # trainer hook: the heads' backward is enqueued, the temporal block follows
    dg, dx2 = dtc_backward(st.dtc, enc.tc_block.layers(), B, T, dpool=dx4, need_dx=True, gout=gout, mode=st.mode)
    mark("enc_bwd.dtc")
    for i, d in enumerate(dg, start=1):
        for k, v in d.items():
            g[f"tc_block.dtc{i}.{k}"] = v
    pg, dxp = pointnet_backward(st.pn, enc.pc_block.layers(), st.mode, dpool=dx2, pool_rows=N, need_dx=need_dx,
                                gout=gout)
    for i, d in enumerate(pg, start=1):
        for k, v in d.items():
            g[f"pc_block.pointnet{i}.{k}"] = v
    mark("enc_bwd.pointnet")
    dx = None
    if need_dx:
        dx = dxp.float().view(B, T, N, st.C).permute(0, 3, 1, 2)
    return g, dx


def _encoder_heads_backward(enc, st, d_logits, d_supfv, gout=None, gph=None, d_hproj=None, gph_gout=None):
    """The MLP heads' part of encoder_backward (arguments as there) -> ({name: grad}, dx4 [B, 512])"""
    g = {}
    B = st.B

    def dst(name):
        return (gout[name + ".weight"], gout[name + ".bias"]) if gout is not None else (None, None)

    if d_hproj is not None and (gph is None or st.hproj is None):
        raise RuntimeError("encoder_backward: d_hproj needs the head passed to encoder_forward(gph=...)")
    if _heads_fusable(enc, gph if d_hproj is not None else None, B, True):
        m1, mh, m2, mg = _heads_mods(enc, gph if d_hproj is not None else None)
        outs = {}
        outs["dW1"], outs["db1"] = dst("MLP_sup1.0")
        outs["dW2"], outs["db2"] = dst("MLP_sup2.0")
        if mh is not None:
            outs["dWh"], outs["dbh"] = dst("MLP_head.0")
        if mg is not None and gph_gout is not None:
            outs["dWg"], outs["dbg"] = gph_gout
        outs, dx4 = ops.heads_bwd(
            st.x4, st.sup_fv, st.h, st.logits, st.hproj if mg is not None else None, m1.weight,
            mh.weight if mh is not None else None, m2.weight, mg.weight if mg is not None else None,
            d_logits.contiguous() if d_logits is not None else None,
            d_supfv.contiguous() if d_supfv is not None else None,
            d_hproj.contiguous() if mg is not None else None, outs)
        g["MLP_sup1.0.weight"], g["MLP_sup1.0.bias"] = outs["dW1"], outs["db1"]
        g["MLP_sup2.0.weight"], g["MLP_sup2.0.bias"] = outs["dW2"], outs["db2"]
        if mh is not None:
            g["MLP_head.0.weight"], g["MLP_head.0.bias"] = outs["dWh"], outs["dbh"]
        if mg is not None:
            g["GPH.0.weight"], g["GPH.0.bias"] = outs["dWg"], outs["dbg"]
    else:
        dsup = d_supfv.contiguous().clone() if d_supfv is not None else torch.zeros_like(st.sup_fv)
        if d_hproj is not None:
            gw, gb = gph_gout if gph_gout is not None else (None, None)
            dW, db, dsup = linear_act_backward(st.sup_fv, st.hproj, gph[0], ACT_ELU, d_hproj.contiguous(),
                                               dx_init=dsup, dW_out=gw, db_out=gb)
            g["GPH.0.weight"], g["GPH.0.bias"] = dW, db
        if d_logits is not None:
            h = st.h if enc.use_projection_head else st.sup_fv
            w_o, b_o = dst("MLP_sup2.0")
            if enc.use_projection_head:
                dW, db, dh = linear_act_backward(h, st.logits, enc.MLP_sup2[0], ACT_ELU, d_logits.contiguous(),
                                                 dW_out=w_o, db_out=b_o)
                g["MLP_sup2.0.weight"], g["MLP_sup2.0.bias"] = dW, db
                w_o, b_o = dst("MLP_head.0")
                dW, db, dsup = linear_act_backward(st.sup_fv, st.h, enc.MLP_head[0], ACT_ELU, dh, dx_init=dsup,
                                                   dW_out=w_o, db_out=b_o)
                g["MLP_head.0.weight"], g["MLP_head.0.bias"] = dW, db
            else:
                dW, db, dsup = linear_act_backward(h, st.logits, enc.MLP_sup2[0], ACT_ELU, d_logits.contiguous(),
                                                   dx_init=dsup, dW_out=w_o, db_out=b_o)
                g["MLP_sup2.0.weight"], g["MLP_sup2.0.bias"] = dW, db
        else:
            for nm in ("MLP_sup2.0", "MLP_head.0"):
                mod = getattr(enc, nm.split(".")[0], None)
                if mod is not None:
                    g[nm + ".weight"] = gout[nm + ".weight"] if gout is not None else torch.zeros_like(mod[0].weight)
                    g[nm + ".bias"] = gout[nm + ".bias"] if gout is not None else torch.zeros_like(mod[0].bias)
        w_o, b_o = dst("MLP_sup1.0")
        dW, db, dx4 = linear_act_backward(st.x4, st.sup_fv, enc.MLP_sup1[0], ACT_ELU, dsup, dW_out=w_o, db_out=b_o)
        g["MLP_sup1.0.weight"], g["MLP_sup1.0.bias"] = dW, db
    return g, dx4


class _EncoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, enc, x, *params):
        # (cg_encoder only comes here when a gradient is wanted)
        logits, sup_fv, st = encoder_forward(enc, x, enc.training, want_bwd=True)
        ctx.enc, ctx.st = enc, st
        ctx.need_dx = x.requires_grad
        ctx.names = [n for n, _ in enc.named_parameters()]
        # the state keeps logits and sup_fv for the heads' backward: hand out aliases, or the outputs (whose grad_fn is
        # this node) and the node (whose state holds them) keep each other, and a step's activations, alive
        return logits.detach(), sup_fv.detach()

    @staticmethod
    @once_differentiable
    def backward(ctx, d_logits, d_supfv):
        g, dx = encoder_backward(ctx.enc, ctx.st, d_logits, d_supfv, need_dx=ctx.need_dx)
        return (None, dx) + tuple(g.get(n) for n in ctx.names)


def cg_encoder(enc, x):
    _require_gpu(x, "CGEncoder")
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in enc.parameters())):
        return _EncoderFn.apply(enc, x, *enc.parameters())
    logits, sup_fv, _ = encoder_forward(enc, x, enc.training)
    return logits, sup_fv


def _want_bwd(x, params):
    """the "a backward will follow" switch of an eval-mode forward, decided where autograd's state can still be seen
    (inside Function.forward grad mode is off): the condition cg_encoder tests"""
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))


# ---------------------------------------------------------------- the track routes, differentiable in eval mode
# A deployment's data arrives as tracks: every frame goes through the PointNet block ONCE (frame_features; from its
# distinct detections with their multiplicities: frame_features_ragged) into a frame-feature table, and the temporal
# block and the heads read windows of that table (windows_forward).  The three pieces are autograd Functions that chain:
# the window gradients are overlap-added into the table's gradient (ops.gather_sum_rows), which is the pooled gradient
# the PointNet backward starts from.  Eval mode only: BatchNorm is the fixed map of its running statistics, which are
# read and never written.  The host-side rules (which windows a track has, where they start in the table, the padding
# of a chunk to whole GEMM row tiles, the refusals, the raw-detection step) are frame_table.py's, shared with the scorers.
def _check_track_eval(enc, who):
    if enc.training:
        raise RuntimeError(f"{who}: the encoder is in training mode (batch statistics would need weighted moments); "
                           "call encoder.eval()")


def _pointnet_param_grads(enc, grads):
    """pointnet_backward's per-layer dicts -> the gradients in the order of enc.pc_block.named_parameters()"""
    g = {f"pointnet{i}.{k}": v for i, d in enumerate(grads, start=1) for k, v in d.items()}
    return tuple(g.get(n) for n, _ in enc.pc_block.named_parameters())


class _FrameFeaturesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, enc, x, ragged, *params):
        # (frame_features / frame_features_ragged only come here when a gradient is wanted)
        mode = get_precision()
        layers = enc.pc_block.layers()
        if ragged is None:
            U, N, C = x.shape
            out, saves = pointnet_forward(x.view(U * N, C), layers, False, mode, pool_rows=N, want_bwd=True)
        else:
            y, saves = pointnet_forward(x, layers, False, mode, pool_rows=0, want_bwd=True, last_pre_bn=True)
            last = saves[-1]
            if last.y is None:
                raise RuntimeError("frame_features_ragged: the last PointNet layer kept no pre-BatchNorm y")
            out = ops.segment_weighted_mean(y, ragged.weight, ragged.u_off, ragged.N, last.scale, last.shift)
        ctx.enc, ctx.saves, ctx.mode, ctx.ragged = enc, saves, mode, ragged
        ctx.x_shape, ctx.need_dx = tuple(x.shape), x.requires_grad
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dfeats):
        enc, ragged = ctx.enc, ctx.ragged
        N = ragged.N if ragged is not None else ctx.x_shape[1]
        grads, dxp = pointnet_backward(ctx.saves, enc.pc_block.layers(), ctx.mode, dpool=dfeats.contiguous(), pool_rows=N,
                                       need_dx=ctx.need_dx, ragged=ragged)
        dx = dxp.float().view(ctx.x_shape) if ctx.need_dx else None
        return (None, dx, None) + _pointnet_param_grads(enc, grads)


def frame_features(enc, frames):
    """Eval-mode PointNet block + mean over the points, frame by frame: point-major ``frames`` [U, N, C] fp32 -> [U, 1024]
    fp32.  With no gradient wanted this is ``encoder_frame_features`` (same bits); with one (autograd on, ``frames`` or a
    parameter of the PointNet block requires it) the forward keeps every layer's pre-BatchNorm y and the backward is ``pointnet_backward`` on the
    eval-mode saves: parameter gradients (the biases in front of the BatchNorms included) and, when ``frames`` requires
    it, the gradient w.r.t. the frames.  No BatchNorm buffer is written.  Raises in training mode."""
    _check_track_eval(enc, "frame_features")
    if not _want_bwd(frames, enc.pc_block.parameters()):
        return encoder_frame_features(enc, frames)[0]
    _check_encoder_frames(enc, frames, "frame_features")         # (without a gradient encoder_frame_features checks)
    return _FrameFeaturesFn.apply(enc, frames, None, *enc.pc_block.parameters())


def frame_features_ragged(enc, rows, weight, u_off, n, N):
    """``frame_features`` of n padded frames from their DISTINCT points (arguments of ``encoder_frame_features_ragged``):
    ``rows`` [M, C] fp32, ``weight`` fp32 [M], ``u_off`` int32 [n + 1] -> [n, 1024] fp32.  With no gradient wanted this is
    ``encoder_frame_features_ragged`` (same bits).  With one, the PointNet layers run on the M compact rows and keep their
    pre-BatchNorm y, ``ops.segment_weighted_mean`` pools; the backward starts with its adjoint
    (``ops.segment_weighted_mean_bwd``: dy of the last layer and its BatchNorm statistics in one pass over the M rows) and
    continues as ``pointnet_backward`` does on M rows.  ``rows.requires_grad`` gives ``rows.grad``: ONE value per distinct
    detection -- the sum of the padded route's gradients over the copies of that point.  Raises in training mode."""
    _check_track_eval(enc, "frame_features_ragged")
    if not _want_bwd(rows, enc.pc_block.parameters()):
        with torch.no_grad():
            return encoder_frame_features_ragged(enc, rows, weight, u_off, n, N)[0]
    _check_encoder_ragged(enc, rows, weight, u_off, n, N, "frame_features_ragged")   # (without: the call above checks)
    return _FrameFeaturesFn.apply(enc, rows, _RaggedPool(weight, u_off, int(N)), *enc.pc_block.parameters())


class _WindowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, enc, table, win_row, T, *params):
        # (windows_forward only comes here when a gradient is wanted)
        mode = get_precision()
        B = len(win_row)
        st = EncoderState()
        st.B, st.T, st.mode, st.training, st.want_bwd = B, T, mode, False, True
        a = ops.gather_frames(table, win_row.row_index())                       # the windows, written out: [B*T, 1024]
        x4, st.dtc = dtc_forward(a, B, T, enc.tc_block.layers(), False, pool_time=True, mode=mode, want_bwd=True)
        st.x4 = x4
        logits, sup_fv, _ = _encoder_heads(enc, st, x4)
        ctx.enc, ctx.st, ctx.need_dtable = enc, st, table.requires_grad
        ctx.csr = None
        if ctx.need_dtable:
            # the plan transposed on the host, uploaded once
            off, idx = win_row.csr()
            ctx.csr = (torch.from_numpy(off).to(table.device), torch.from_numpy(idx).to(table.device))
        return logits.detach(), sup_fv.detach()            # aliases: see _EncoderFn.forward

    @staticmethod
    @once_differentiable
    def backward(ctx, d_logits, d_supfv):
        enc, st = ctx.enc, ctx.st
        g, dx4 = _encoder_heads_backward(enc, st, d_logits, d_supfv)
        dg, da = dtc_backward(st.dtc, enc.tc_block.layers(), st.B, st.T, dpool=dx4, need_dx=ctx.need_dtable, mode=st.mode)
        for i, d in enumerate(dg, start=1):
            for k, v in d.items():
                g[f"tc_block.dtc{i}.{k}"] = v
        dtable = ops.gather_sum_rows(da.contiguous(), *ctx.csr) if ctx.need_dtable else None
        return (None, dtable, None, None) + tuple(g.get(n) for n, _ in enc.named_parameters())


def windows_forward(enc, table, win_row, T):
    """Eval-mode temporal block, mean over T and heads on windows of a frame-feature table [table_rows, 1024] fp32
    (``win_row``: an ops.WindowRows -- flat, ring or segmented rings) -> (logits, sup_fv).  With no gradient wanted this is
    ``encoder_forward_windows`` (same bits: the first layer reads the table through its windowed launch).  With one, the
    windows are written out with one gather (``ops.gather_frames(table, win_row.row_index())``) and go the eval-backward
    route of the materialised crops; the backward runs the heads, ``dtc_backward`` and, when ``table`` requires a
    gradient, the overlap-add of the window gradients into the table's (``ops.gather_sum_rows``: fixed order, no atomics).
    Raises in training mode."""
    _check_track_eval(enc, "windows_forward")
    _require_gpu(table, "CGEncoder")
    if not _want_bwd(table, enc.parameters()):
        return encoder_forward_windows(enc, table, win_row, T)[:2]
    if table.dim() != 2 or table.dtype != torch.float32 or not table.is_contiguous():
        raise ValueError(f"windows_forward expects a contiguous fp32 table [rows, ch], got {tuple(table.shape)} {table.dtype}")
    if win_row.T != T or win_row.table_rows != table.shape[0] or len(win_row) < 1:
        raise ValueError("windows_forward: win_row does not describe at least one window of T rows of this table")
    return _WindowsFn.apply(enc, table, win_row, int(T), *enc.parameters())


track_windows = frame_table.track_windows      # (n_frames, T, hop, drop_last_aligned=True) -> (W, U): kept under this name


class TrackBatch:
    """What ``plan_tracks`` derives from tracks that do not change between calls, so that a loop over the same tracks
    (adapt.finetune_frozen_bn_tracks) does it once: the frames any window uses (``frames`` [U, N, C]; ``spare``: the
    tensor they are the first U frames of), with ``dedup_points`` their compact table (``rows`` [M, C], ``weight`` [M],
    ``u_off`` [U + 1]), the windows' plan (an ops.WindowRows over the U table rows), each track's windows (``counts``)."""
    __slots__ = ("frames", "spare", "U", "N", "rows", "weight", "u_off", "plan", "T", "counts")


def plan_tracks(enc, tracks, hop=None, drop_last_aligned=True, dedup_points=False, who="cg_encoder_tracks"):
    """-> the TrackBatch of a list of processed tracks [F_i, N, C] (arguments of ``cg_encoder_tracks``).  With
    ``dedup_points`` this is where the distinct rows are found (``ops.frames_unique_offsets`` / ``ops.frames_unique``: the one
    host copy of the offsets and the read of the error flag); nothing here is differentiated."""
    from . import constants
    tracks = list(tracks)
    if not tracks:
        raise ValueError(f"{who}: no track")
    T, hop = constants.NSTEPS, constants.CROP_STEP if hop is None else int(hop)
    for track in tracks:
        _check_encoder_frames(enc, track, who)
    wp = frame_table.plan_track_windows([t.shape[0] for t in tracks], T, hop, drop_last_aligned, who)
    if dedup_points and torch.is_grad_enabled() and any(t.requires_grad for t in tracks):
        raise RuntimeError(f"{who}: with dedup_points the padded frames have no gradient of their own (a repeated "
                           "detection is one row); call it without dedup_points, or differentiate frame_features_ragged "
                           "for one gradient per distinct detection")
    tb = TrackBatch()
    tb.U, tb.N, tb.T, tb.counts = wp.U, tracks[0].shape[1], T, wp.counts
    tb.spare = tracks[0] if len(tracks) == 1 else torch.cat([t[:u] for t, u in zip(tracks, wp.used)])
    tb.frames = tb.spare[:tb.U]
    tb.rows = tb.weight = tb.u_off = None
    if dedup_points:
        with torch.no_grad():
            u_off = ops.frames_unique_offsets(tb.frames)
            err = torch.zeros(1, dtype=torch.int32, device=tb.frames.device)
            M = ops.unique_chunk_rows(int(u_off.cpu()[-1]))                    # the one host copy
            tb.rows, tb.weight, tb.u_off = ops.frames_unique(tb.frames, u_off, 0, tb.U, M, err_flag=err)
        if err.item():
            raise RuntimeError(f"{who}: ops.frames_unique met a segment that is not its frame's")
    tb.plan = ops.WindowRows(wp.starts, T, tb.U, device=tb.frames.device)
    return tb


def encode_track_batch(enc, tb):
    """A planned batch of tracks through the eval-mode encoder -> (logits [W, K], sup_fv [W, 32]): ``cg_encoder_tracks``
    behind its plan.  Launches only: no host copy, no read of a device flag."""
    _check_track_eval(enc, "cg_encoder_tracks")
    if tb.rows is not None:
        table = frame_features_ragged(enc, tb.rows, tb.weight, tb.u_off, tb.U, tb.N)
    elif _want_bwd(tb.frames, enc.pc_block.parameters()):
        table = frame_features(enc, tb.frames)
    else:
        # no gradient: whole GEMM row tiles (frame_table.pad_chunk); the extra frames' features are dropped
        table = frame_features(enc, frame_table.pad_chunk(tb.spare, 0, tb.U, frame_pad_quantum(tb.N))[0])[:tb.U]
    return windows_forward(enc, table, tb.plan, tb.T)


def cg_encoder_tracks(enc, tracks, hop=None, drop_last_aligned=True, dedup_points=False, who="cg_encoder_tracks"):
    """The eval-mode encoder on the windows of processed tracks, differentiable: ``tracks`` is a list of [F_i, N, C] fp32
    device tensors -> (logits [W, K], sup_fv [W, 32]) for their W = sum W_i windows of NSTEPS frames, track after track --
    the windows ``OpenSetScorer.embed_track`` scores (``inference.window_count``; track i's windows use its first
    ``U_i = (W_i - 1) * hop + NSTEPS`` frames).  Every frame goes through the PointNet block once and no crop is written
    out; the tracks share ONE PointNet pass and ONE temporal pass (one frame-feature table, a window never leaves its
    track's rows), so the launches do not grow with the number of tracks.  ``dedup_points``: every frame's DISTINCT rows
    once, pooled with their multiplicities (``ops.frames_unique_offsets`` / ``ops.frames_unique``: one host copy of the
    offsets, the table rounded to 256-row tiles).  ``hop``: None = CROP_STEP.  A caller that passes the same tracks again
    and again plans them once (``plan_tracks``) and calls ``encode_track_batch``.

    With a gradient wanted (autograd on; a parameter or a track requires it) nothing is chunked and the backward reads what
    the forward kept -- the caller bounds the tracks.  Kept per point row (sum U_i * N rows, with ``dedup_points`` the
    distinct rows): the pre-BatchNorm y of PointNet layers 2-4 and the three activations between the layers (layer 1's y
    is recomputed from the points), 4 608 values = 18 KB in fp32 mode, 9 KB in bf16 mode.  Kept per window: its NSTEPS rows
    of the table written out (120 KB), the six temporal layers' im2col matrices (3 * (1024 + 16 + 32 + 64 + 128 + 256)
    values per step: 534 KB) and their pre-BatchNorm y (118 KB), all fp32.  A track's ``requires_grad`` is served without
    ``dedup_points``; with it this raises -- ``frame_features_ragged`` gives the gradient per distinct detection.  Raises
    in training mode and (ValueError) for a track too short for a window.  No BatchNorm buffer is written."""
    _check_track_eval(enc, who)
    return encode_track_batch(enc, plan_tracks(enc, tracks, hop, drop_last_aligned, dedup_points, who))


def cg_encoder_track(enc, track, hop=None, drop_last_aligned=True, dedup_points=False):
    """``cg_encoder_tracks`` of one processed track [F, N, C] -> (logits [W, K], sup_fv [W, 32]).  With no gradient wanted
    the outputs are the bits ``OpenSetScorer.embed_track`` scores.  ``hop``: None = CROP_STEP.  Memory kept for a backward:
    see ``cg_encoder_tracks``."""
    return cg_encoder_tracks(enc, [track], hop, drop_last_aligned, dedup_points, who="cg_encoder_track")


def cg_encoder_raw_track(enc, points, offsets, pick=None, seed=0, track_key=0, hop=None, drop_last_aligned=True,
                         dedup_points=False):
    """``cg_encoder_track`` from the radar's detections (arguments of ``OpenSetScorer.embed_raw_track``): ``points`` [P, 5]
    fp32 / fp64 and ``offsets`` int32 [F + 1] on the device -> ``ops.frames_from_raw`` (centred, not divided by std) -> the
    track route; ``dedup_points``: ``ops.frames_from_raw_unique`` -> ``frame_features_ragged``, the padded frames never
    written.  ``pick`` int32 [F, N]: host-drawn picks; None: drawn on the device, frame f under the key ``(track_key, f)``
    and ``seed``.  Parameter gradients only: the frame preparation (centring, dB) is not differentiated, and
    ``points.requires_grad`` raises.  Memory kept for the backward: as ``cg_encoder_tracks``.  A frame that could not be
    processed (``ops.frames_from_raw``'s rule) raises."""
    from . import constants
    _check_track_eval(enc, "cg_encoder_raw_track")
    N, C = enc.nmax_points, enc.pc_block.pointnet1.module[0].weight.shape[1]
    F = frame_table.check_raw(points, offsets, pick, N, "cg_encoder_raw_track")
    if points.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("cg_encoder_raw_track: no gradient w.r.t. the raw detections (the frame preparation is not "
                           "differentiated); detach the points")
    T, hop = constants.NSTEPS, constants.CROP_STEP if hop is None else int(hop)
    wp = frame_table.plan_track_windows([F], T, hop, drop_last_aligned, "cg_encoder_raw_track")
    dev = points.device
    keys = frame_table.frame_keys(track_key, 0, F, dev) if pick is None else None
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.no_grad():              # dedup_points: the frames any window uses; without: all (cg_encoder_track cuts)
        raw = frame_table.raw_frames(points, offsets, N, C, pick, seed, keys, err, 0, wp.U if dedup_points else None,
                                     dedup_points)
    if err.item():
        raise RuntimeError("cg_encoder_raw_track: a frame could not be processed (ops.frames_from_raw's rule)")
    if not dedup_points:
        return cg_encoder_track(enc, raw, hop, drop_last_aligned)
    table = frame_features_ragged(enc, *raw, wp.U, N)
    return windows_forward(enc, table, ops.WindowRows(wp.starts, T, table.shape[0], device=dev), T)


# ---------------------------------------------------------------- encoder trunk (OR-CED baseline, models.py:446-505)
class _TrunkFn(torch.autograd.Function):
    """PointNetBlock -> mean over the points -> TemporalConvolutionBlock -> mean over time: x [B,C,T,N] -> x4 [B,512],
    the part ORCEDEncoder shares with CGEncoder, on the same kernels (its three Linear heads follow in torch)."""

    @staticmethod
    def forward(ctx, enc, want_bwd, x, *params):
        B, C, T, N = x.shape
        mode = get_precision()
        xp = _point_major(x).view(B * T * N, C)
        x2, pn = pointnet_forward(xp, enc.pc_block.layers(), enc.training, mode, pool_rows=N, want_bwd=want_bwd)
        x4, dtc = dtc_forward(x2, B, T, enc.tc_block.layers(), enc.training, pool_time=True, want_bwd=want_bwd)
        ctx.enc, ctx.pn, ctx.dtc, ctx.shape, ctx.mode, ctx.training = enc, pn, dtc, (B, C, T, N), mode, enc.training
        ctx.names = [n for n, _ in itertools.chain(enc.pc_block.named_parameters(prefix="pc_block"),
                                                   enc.tc_block.named_parameters(prefix="tc_block"))]
        return x4

    @staticmethod
    @once_differentiable
    def backward(ctx, dx4):
        B, C, T, N = ctx.shape
        enc = ctx.enc
        g = {}
        dg, dx2 = dtc_backward(ctx.dtc, enc.tc_block.layers(), B, T, dpool=dx4.contiguous().float(), need_dx=True)
        for i, d in enumerate(dg, start=1):
            for k, v in d.items():
                g[f"tc_block.dtc{i}.{k}"] = v
        pg, _ = pointnet_backward(ctx.pn, enc.pc_block.layers(), ctx.mode, dpool=dx2, pool_rows=N, need_dx=False)
        for i, d in enumerate(pg, start=1):
            for k, v in d.items():
                g[f"pc_block.pointnet{i}.{k}"] = v
        return (None, None, None) + tuple(g.get(n) for n in ctx.names)


class _OrcedHeadsFn(torch.autograd.Function):
    """ORCEDEncoder's MLP_mu / MLP_logvar, the reparametrisation and MLP_classification (models.py:489-505) in one
    launch (csrc/orced.hip); backward in two."""

    @staticmethod
    def forward(ctx, x4, eps, Wmu, bmu, Wlv, blv, Wc, bc):
        x4, eps = x4.contiguous(), eps.contiguous().float()
        logits, sup, mu, logvar = ops.orced_heads_fwd(x4, Wmu, bmu, Wlv, blv, eps, Wc, bc)
        ctx.save_for_backward(x4, eps, logvar, sup, Wmu, Wlv, Wc)
        return logits, sup, mu, logvar

    @staticmethod
    @once_differentiable
    def backward(ctx, d_logits, d_sup, d_mu, d_logvar):
        x4, eps, logvar, sup, Wmu, Wlv, Wc = ctx.saved_tensors
        c = lambda t: None if t is None else t.contiguous().float()
        dx4, dWmu, dbmu, dWlv, dblv, dWc, dbc = ops.orced_heads_bwd(x4, eps, logvar, sup, Wmu, Wlv, Wc, c(d_logits), c(d_sup),
                                                                    c(d_mu), c(d_logvar), need_dx=ctx.needs_input_grad[0])
        return dx4, None, dWmu, dbmu, dWlv, dblv, dWc, dbc


def orced_heads(enc, x4, eps):
    """(logits, sup_fv, vae_mu, vae_logvar) of an ORCEDEncoder from its trunk output and the caller's eps draw"""
    _require_gpu(x4, "ORCEDEncoder heads")
    lm, ll, lc = enc.MLP_mu[0], enc.MLP_logvar[0], enc.MLP_classification[0]
    return _OrcedHeadsFn.apply(x4, eps, lm.weight, lm.bias, ll.weight, ll.bias, lc.weight, lc.bias)


class _KlFn(torch.autograd.Function):
    """CG_kl_divergence (utils.py:72-85): forward and the three gradients in one launch each."""

    @staticmethod
    def forward(ctx, mu, logvar, mu_k):
        mu, logvar, mu_k = mu.contiguous().float(), logvar.contiguous().float(), mu_k.contiguous().float()
        # loss and the three UNSCALED gradients from the one launch (as _CeFn): the backward multiplies by the upstream
        # gradient on the device -- no host read of a device scalar (round-3 advisor finding: float(g) synchronised
        # every step and cannot be captured into a hipGraph)
        loss, grads = ops.orced_kl(mu, logvar, mu_k, want_loss=True, gscale=1.0)
        ctx.save_for_backward(*grads)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        dm, dl, dk = ctx.saved_tensors
        return dm * g, dl * g, dk * g


def cg_kl_divergence(mu, logvar, mu_k):
    _require_gpu(mu, "CG_kl_divergence")
    return _KlFn.apply(mu, logvar, mu_k)


class _TripletFn(torch.autograd.Function):
    """OR-CED's triplet term (MultiSimilarityMiner + TripletMarginLoss, train_ORCED.py:9,30,34) in dense form: loss and
    the UNSCALED gradient from the one launch sequence (pcaa_orced_triplet), as _KlFn; nothing is read on the host."""

    @staticmethod
    def forward(ctx, x, labels, epsilon, margin):
        loss, dx = ops.orced_triplet(x.contiguous().float(), labels.contiguous(), epsilon, margin, gscale=1.0)
        ctx.save_for_backward(dx)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        return dx * g, None, None, None


def orced_triplet_loss(x, labels, epsilon=0.1, margin=0.5):
    """``triplet_margin_loss(x, labels, multi_similarity_miner(x, labels, epsilon), margin)`` of orced.py on the device
    kernels; ``margin`` defaults to the reference's TRIPLET_MARGIN (train_ORCED.py:324).  Raises on unsupported shapes."""
    _require_gpu(x, "orced_triplet_loss")
    return _TripletFn.apply(x, labels, float(epsilon), float(margin))


class _CeFn(torch.autograd.Function):
    """torch.nn.functional.cross_entropy (mean) on the device kernel of the PCAA step (pcaa_cross_entropy: loss and
    softmax - onehot gradient in the same launch)."""

    @staticmethod
    def forward(ctx, logits, target):
        logits = logits.contiguous().float()
        loss, dl, _ = ops.cross_entropy(logits, target, want_loss=True, want_grad=True, grad_scale=1.0)
        ctx.save_for_backward(dl)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return dl * g, None


def cross_entropy_loss(logits, target):
    _require_gpu(logits, "cross_entropy_loss")
    return _CeFn.apply(logits, target)


def encoder_trunk(enc, x):
    _require_gpu(x, "ORCEDEncoder")
    if x.dim() != 4 or x.shape[3] != enc.nmax_points:
        raise RuntimeError(f"ORCEDEncoder expects [B,C,T,{enc.nmax_points}], got {tuple(x.shape)}")
    params = list(enc.pc_block.parameters()) + list(enc.tc_block.parameters())
    return _TrunkFn.apply(enc, _want_bwd(x, params), x, *params)


# ---------------------------------------------------------------- standalone blocks
class _PointNetStackFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, layers, training, want_bwd, x, *params):
        B, C, T, N = x.shape
        xp = _point_major(x).view(B * T * N, C)
        a, saves = pointnet_forward(xp, layers, training, "fp32", want_bwd=want_bwd)
        ctx.layers, ctx.saves, ctx.shape = layers, saves, (B, C, T, N)
        ctx.need_dx = x.requires_grad
        ctx.training = training
        return a.view(B, T, N, -1).permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        B, C, T, N = ctx.shape
        d = gout.permute(0, 2, 3, 1).contiguous().view(B * T * N, -1)
        grads, dxp = pointnet_backward(ctx.saves, ctx.layers, "fp32", d_last=d, need_dx=ctx.need_dx)
        flat = []
        for gd in grads:
            flat += [gd["module.0.weight"], gd["module.0.bias"], gd["module.1.weight"], gd["module.1.bias"]]
        dx = dxp.view(B, T, N, C).permute(0, 3, 1, 2) if ctx.need_dx else None
        return (None, None, None, dx) + tuple(flat)


def pointnet_stack(x, layers, training):
    _require_gpu(x, "PointNet")
    params = []
    for l in layers:
        params += [l.module[0].weight, l.module[0].bias, l.module[1].weight, l.module[1].bias]
    return _PointNetStackFn.apply(layers, training, _want_bwd(x, params), x, *params)


class _DtcStackFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, layers, training, want_bwd, x, *params):
        B, C, T = x.shape
        a2d = x.permute(0, 2, 1).contiguous().view(B * T, C)
        a, saves = dtc_forward(a2d, B, T, layers, training, pool_time=False, want_bwd=want_bwd)
        ctx.layers, ctx.saves, ctx.shape, ctx.training = layers, saves, (B, C, T), training
        return a.view(B, T, -1).permute(0, 2, 1)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        B, C, T = ctx.shape
        d = gout.permute(0, 2, 1).contiguous().view(B * T, -1)
        grads, dx2d = dtc_backward(ctx.saves, ctx.layers, B, T, d_last=d, need_dx=True)
        flat = []
        for gd in grads:
            flat += [gd["conv1d.weight"], gd["conv1d.bias"], gd["batch_norm.weight"], gd["batch_norm.bias"]]
        return (None, None, None, dx2d.view(B, T, C).permute(0, 2, 1)) + tuple(flat)


def dtc_stack(x, layers, training):
    _require_gpu(x, "DilTempConv1d")
    params = []
    for l in layers:
        params += [l.conv1d.weight, l.conv1d.bias, l.batch_norm.weight, l.batch_norm.bias]
    return _DtcStackFn.apply(layers, training, _want_bwd(x, params), x.float(), *params)


# ======================================================================
# CGDecoder (models.py:340-385)
# ======================================================================
def decoder_forward(dec, z, mode=None, images=None):
    """``images`` {layer number: bf16 image of that layer's weight}: streamed instead of the fp32 matrix by the bf16
    mode's weight-streaming kernels (same rounding, same result); only a caller that keeps them current passes them."""
    mode = get_precision() if mode is None else mode
    _require_gpu(z, "CGDecoder")
    if z.dim() != 2 or z.shape[1] != dec.dense1.weight.shape[1]:
        raise RuntimeError(f"CGDecoder: expected [B,{dec.dense1.weight.shape[1]}], got {tuple(z.shape)}")
    acts = [z.contiguous().float()]
    # _pcaa_pad (set by PCAATrainer.finalize for ragged widths): the layers as zero-padded [Np,Kp] weights;
    # the chain then runs in the padded widths (padded activations are exactly 0) and the output is cut back
    layers = getattr(dec, "_pcaa_pad", None) or dec.dense_layers()
    for i, lin in enumerate(layers):
        acts.append(linear_act_forward(acts[-1], lin, ACT_ELU if i < 4 else ACT_NONE, mode,
                                       W16=(images or {}).get(i + 1)))
    out = acts[-1]
    S = dec.dense5.weight.shape[0]
    if out.shape[1] != S:
        out = out[:, :S].contiguous()
    return out, acts


def decoder_backward(dec, acts, d_out, need_dz=True, grads_out=None, dz_init=None, mode=None, after_layer=None,
                     updates=None, images=None):
    """``grads_out`` {"denseI.weight"/"denseI.bias": destination}: for a padded decoder (see decoder_forward)
    these are the PADDED gradient tensors; without grads_out the returned gradients are cut to the parameter
    shapes.  ``updates`` {layer number: update(dz, x)}: those layers' weight gradients are formed and consumed by
    the caller's fused optimizer kernel (linear_act_backward) and come back as None."""
    mode = get_precision() if mode is None else mode
    padded = getattr(dec, "_pcaa_pad", None)
    layers = padded or dec.dense_layers()
    g = {}
    d = d_out.contiguous().view(d_out.shape[0], -1)
    if d.shape[1] != acts[-1].shape[1]:
        dp = torch.zeros_like(acts[-1])                  # padded output columns carry no gradient
        dp[:, :d.shape[1]].copy_(d)
        d = dp
    pre = False           # d is w.r.t. the layer's pre-activation (ELU' already applied by the dgrad above)
    defer_db = []         # (dz, db destination) of the layers whose update is fused: their column sums leave together below
    for i in range(4, -1, -1):
        lin = layers[i]
        nm = f"dense{i + 1}"
        dW_out = grads_out[nm + ".weight"] if grads_out else None
        db_out = grads_out[nm + ".bias"] if grads_out else None
        M, K = acts[i].shape
        fuse = i > 0 and (_skinny(mode, M, lin.weight.shape[0], K) or _skinny_exact(mode, M, lin.weight.shape[0], K))    # acts[i] is an ELU output for i >= 1
        dW, db, d = linear_act_backward(acts[i], acts[i + 1], lin, ACT_ELU if i < 4 else ACT_NONE, d,
                                        need_dx=(i > 0 or need_dz), dW_out=dW_out, db_out=db_out,
                                        dx_init=dz_init if i == 0 else None, mode=mode, d_is_pre=pre,
                                        fuse_elu_in=fuse, update=(updates or {}).get(i + 1), W16=(images or {}).get(i + 1),
                                        defer_db=defer_db if ((updates or {}).get(i + 1) is not None or after_layer is None) else None)
        pre = fuse
        if after_layer is not None:
            after_layer(i + 1)       # trainer hook: layer i+1's weight / bias gradients are enqueued
        dW = dW.view_as(lin.weight) if dW is not None else None
        if padded and grads_out is None:
            ref = dec.dense_layers()[i]                  # cut the padding off: gradients in the parameter shapes
            db = db[:ref.bias.shape[0]]
            dW = dW[:ref.weight.shape[0], :ref.weight.shape[1]] if dW is not None else None
        g[nm + ".weight"], g[nm + ".bias"] = dW, db
    if defer_db:
        with _on_wgrad_stream(*[t for ts, _ in defer_db for t in ts]):
            for _, launch in defer_db:
                launch()
    return g, d


class _DecoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dec, z, *params):
        out, acts = decoder_forward(dec, z)
        ctx.dec, ctx.acts, ctx.need_dz = dec, acts, z.requires_grad
        ctx.names = [n for n, _ in dec.named_parameters()]
        return out.view(-1, dec.n_features, dec.n_steps, dec.nmax_points)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        g, dz = decoder_backward(ctx.dec, ctx.acts, gout.contiguous(), need_dz=ctx.need_dz)
        return (None, dz) + tuple(g.get(n) for n in ctx.names)   # bn1..4: None (unused, like the reference)


def cg_decoder(dec, z):
    _require_gpu(z, "CGDecoder")
    return _DecoderFn.apply(dec, z, *dec.parameters())


# ======================================================================
# CGDiscriminator (models.py:405-421).  Twice differentiable: the reference's D-step differentiates THROUGH
# torch.autograd.grad(D(interp), interp, create_graph=True) (PCAA_ablation.py:955-976), so the backward of this
# Function is itself a Function (_DiscBwdFn) whose backward is the closed-form second-order kernel
# (pcaa_disc_backward_backward).  The fused trainer does not go through autograd at all
# (ops.disc_wgan_gp); this is what lets the reference's own loop body drive the drop-in module unchanged.
# ======================================================================
class _DiscBwdFn(torch.autograd.Function):
    """(x, label, gout, params) -> (dx, dlabel, dparams...) = the first-order backward, as a differentiable op.
    Its own backward supports an incoming gradient w.r.t. ``dx`` (the gradient-penalty use)."""

    @staticmethod
    def forward(ctx, disc, want, x, label, gout, *params):
        ctx.set_materialize_grads(False)
        dx, dl, grads = ops.disc_backward(x, label, list(params), gout, want_dx=want[0], want_dlabel=want[1],
                                          want_params=want[2])
        ctx.save_for_backward(x, label, gout, *params)
        outs = (dx, dl) + (tuple(grads) if grads is not None else (None,) * 6)
        ctx.mark_non_differentiable(*[o for o in outs[1:] if o is not None])
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, g_dx, *g_rest):
        if any(g is not None for g in g_rest):
            raise NotImplementedError("CGDiscriminator: only the input gradient dD/dx can be differentiated again "
                                      "(the WGAN-GP penalty); gradients of parameter gradients are not implemented")
        if g_dx is None:
            return (None,) * (5 + 6)
        x, label, gout, *params = ctx.saved_tensors
        need = ctx.needs_input_grad        # (disc, want, x, label, gout, *params)
        dx2, dl2, dgo, grads = ops.disc_backward_backward(
            x, label, params, gout, g_dx.contiguous().float(), want_dx=need[2], want_dlabel=need[3],
            want_dgout=need[4], want_params=any(need[5:]))
        return (None, None, dx2, dl2, dgo) + (tuple(grads) if grads is not None else (None,) * 6)


class _DiscFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disc, x, label, *params):
        ctx.disc = disc
        ctx.save_for_backward(x, label, *params)       # the inputs themselves: they keep their place in the graph
        ctx.need = (ctx.needs_input_grad[1], ctx.needs_input_grad[2], any(ctx.needs_input_grad[3:]))
        return ops.disc_forward(x, label, list(params))

    @staticmethod
    def backward(ctx, gout):
        x, label, *params = ctx.saved_tensors
        gout = gout.contiguous().view(-1)
        if torch.is_grad_enabled():
            # create_graph=True: the input gradient stays attached to (x, gout, parameters)
            outs = _DiscBwdFn.apply(ctx.disc, ctx.need, x, label, gout, *params)
            return (None,) + tuple(outs)
        dx, dl, grads = ops.disc_backward(x, label, params, gout, want_dx=ctx.need[0], want_dlabel=ctx.need[1],
                                          want_params=ctx.need[2])
        return (None, dx, dl) + (tuple(grads) if grads is not None else (None,) * 6)


def cg_discriminator(disc, x, label):
    _require_gpu(x, "CGDiscriminator")
    # (conversions happen out here, under autograd, so that what the Function saves are its own inputs)
    return _DiscFn.apply(disc, x.contiguous().float(), label.contiguous().float(), *ops._disc_params(disc))


# ======================================================================
# GaussianMeanLearner (models.py:424-443): Linear+BN1d+ELU x3, Linear
# ======================================================================
class _GmlFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gml, x, *params):
        m = gml.model
        x = x.contiguous().float()
        saves = []
        a = x
        for lin_i, bn_i in ((0, 1), (3, 4), (6, 7)):
            lin, bn = m[lin_i], m[bn_i]
            y, scale, shift, mean, rstd, count, _ = _linear_bn(a, lin.weight, lin.bias, bn, gml.training, "fp32", False)
            saves.append(_LayerSave(a, None, y, scale, shift, mean, rstd, count, lin.weight.shape[1], lin.weight.shape[0], 0))
            a = ops.bn_act_fwd(y, scale, shift)
        out = linear_act_forward(a, m[9], ACT_NONE)
        ctx.gml, ctx.saves, ctx.a_last, ctx.training = gml, saves, a, gml.training
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        m = ctx.gml.model
        dW9, db9, da = linear_act_backward(ctx.a_last, None, m[9], ACT_NONE, gout.contiguous())
        out = []
        for (lin_i, bn_i), s in reversed(list(zip(((0, 1), (3, 4), (6, 7)), ctx.saves))):
            lin, bn = m[lin_i], m[bn_i]
            dW, dg, db, dbias, da = _bn_layer_backward(s, bn, lin.weight, "fp32", s.a_in, da=da, lin_bias=lin.bias)
            out = [dW, dbias if dbias is not None else torch.zeros_like(lin.bias), dg, db] + out
        return (None, da) + tuple(out) + (dW9, db9)


def gaussian_mean_learner(gml, x):
    _require_gpu(x, "GaussianMeanLearner")
    return _GmlFn.apply(gml, x, *gml.parameters())


# ======================================================================
# SeqChamferLoss (utils.py:88-132)
# ======================================================================
class _ChamferFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, preds, gts, avg_out):
        B, C, T, N = preds.shape
        want = preds.requires_grad
        scale = 1.0 / (B * T) if avg_out else 1.0 / T
        fl, dp = ops.chamfer(preds.float(), gts.float(), want_grad=want, grad_scale=scale)
        ctx.dp, ctx.avg_out, ctx.B = dp, avg_out, B
        if avg_out:
            return ops.total(fl, scale)
        return ops.rowsum(fl, scale)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        if ctx.dp is None:
            return None, None, None
        gout = gout.contiguous().float()
        if ctx.avg_out:
            return ops.scale_by_device_scalar(ctx.dp, gout), None, None
        return ops.scale_rows(ctx.dp, gout), None, None


def seq_chamfer_loss(preds, gts, avg_out=True):
    _require_gpu(preds, "SeqChamferLoss")
    _require_gpu(gts, "SeqChamferLoss")
    return _ChamferFn.apply(preds, gts, bool(avg_out))
