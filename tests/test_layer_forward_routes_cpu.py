"""The route choices of the PointNet forward (functional._pointnet_plan, _linear_route) and of the first layer's backward
(functional._in_bwd_route), pinned without a GPU against tables written out by hand from the code they replaced: one case on
each side of every boundary.  The functions are pure -- they launch nothing and allocate nothing -- and the ``*_supported``
predicates behind the epilogue and split-image routes are library calls that need no device (by hand: tests/gemm_ref.py
``dgrad_bn_supported`` / ``split3_supported``; the fp8 product takes N % 256 == 0 and K a multiple of 128).
"""
import math

import pytest
import torch

from opensetgaitrecognition_pcaa_amd import _lib, functional as F, ops

F32, BF16, SPLIT, FP8 = torch.float32, torch.bfloat16, ops.SplitImage.dtype, ops.FP8
ENC = ((4, 512), (512, 512), (512, 1024), (1024, 1024))            # the encoder's PointNet block at C = 4
MID384 = ((4, 512), (512, 512), (512, 384), (384, 512))            # 384 output channels: no epilogue GEMM takes the third layer


def plan(dims=ENC, rows=1024, in_dtype=F32, training=False, mode="fp32", pool_rows=32, want_bwd=False, last_pre_bn=False,
         kind="bf16", sync_bn=False, tails=True):
    """the arguments of _pointnet_plan, in its order: the defaults are a no-grad eval forward of 32 frames of 32 points"""
    return (dims, rows, in_dtype, training, mode, pool_rows, want_bwd, last_pre_bn, kind, sync_bn, tails)


# arguments -> (route of each layer, dtype each layer hands on, finish)
PLAN = [
    # ---- fp32 mode.  16384 rows: 128 row tiles, so no layer meets the slab rule's "fewer than 128 output tiles"
    (plan(rows=16384, training=True), (["in_moments", "fp32", "fp32", "fp32"], [F32] * 4, "meanpool")),
    (plan(rows=16384, training=True, sync_bn=True), (["in_stats", "fp32", "fp32", "fp32"], [F32] * 4, "meanpool")),
    (plan(rows=16384, training=True, tails=False), (["in_stats", "fp32", "fp32", "fp32"], [F32] * 4, "meanpool")),
    (plan(rows=16384), (["in_eval", "fp32", "fp32", "fp32"], [F32] * 4, "meanpool")),
    (plan(rows=16384, want_bwd=True, kind="fp8"), (["in_eval", "fp32", "fp32", "fp32"], [F32] * 4, "meanpool")),
    # 1024 rows in training: 32 / 64 / 64 output tiles and K >= 512 -> split-K 4, 4, 8: slabs
    (plan(training=True), (["in_moments", "fp32_slabs", "fp32_slabs", "fp32_slabs"], [F32] * 4, "meanpool")),
    (plan(), (["in_eval", "fp32", "fp32", "fp32"], [F32] * 4, "meanpool")),
    # the layer over raw points: cin <= 8 against 9, pointnet_in_ok (256 % (24 // 4) != 0)
    (plan(dims=((8, 512), (512, 512)), rows=16384, training=True), (["in_moments", "fp32"], [F32] * 2, "meanpool")),
    (plan(dims=((9, 512), (512, 512)), rows=16384, training=True), (["fp32", "fp32"], [F32] * 2, "meanpool")),
    (plan(dims=((4, 24), (24, 512)), rows=16384, training=True), (["fp32", "fp32"], [F32] * 2, "meanpool")),
    (plan(dims=((4, 24), (24, 512)), rows=16384, training=True, mode="bf16"), (["fp32", "bf16"], [BF16] * 2, "meanpool")),
    # ... which is whatever layer reads fp32 rows of at most 8 channels: the second one too in fp32 mode, not in bf16 mode
    (plan(dims=((4, 8), (8, 512)), training=True, pool_rows=0), (["in_moments", "in_moments"], [F32] * 2, "done")),
    (plan(dims=((4, 8), (8, 512)), training=True, pool_rows=0, mode="bf16"), (["in_moments", "bf16"], [BF16] * 2, "act")),
    # a single-layer stack: pooled, it must store y for the pooling pass; not pooled, it recomputes
    (plan(dims=((4, 512),), training=True), (["in_store"], [F32], "meanpool")),
    (plan(dims=((4, 512),), training=True, mode="bf16"), (["in_store"], [BF16], "meanpool")),
    (plan(dims=((4, 512),), training=True, pool_rows=0), (["in_moments"], [F32], "done")),
    (plan(dims=((4, 512),), training=True, pool_rows=0, mode="fp16x3"), (["in_moments"], [F32], "done")),
    (plan(dims=((4, 512),), pool_rows=0, last_pre_bn=True), (["in_eval"], [F32], "done")),
    # last_pre_bn (pool_rows == 0): the stored y where there is one
    (plan(pool_rows=0), (["in_eval", "fp32", "fp32", "fp32"], [F32] * 4, "act")),
    (plan(pool_rows=0, last_pre_bn=True), (["in_eval", "fp32", "fp32", "fp32"], [F32] * 4, "pre_bn")),
    (plan(pool_rows=0, last_pre_bn=True, mode="bf16"), (["in_eval"] + ["bf16_epilogue"] * 3, [BF16] * 4, "done")),
    (plan(pool_rows=0, last_pre_bn=True, mode="bf16", kind="fp8", rows=1000),
     (["in_eval", "fp8", "fp8", "fp8"], [FP8, FP8, FP8, BF16], "done")),
    (plan(pool_rows=0, last_pre_bn=True, mode="bf16", want_bwd=True), (["in_eval", "bf16", "bf16", "bf16"], [BF16] * 4, "pre_bn")),
    # ---- bf16 mode
    (plan(training=True, mode="bf16"), (["in_moments", "bf16", "bf16", "bf16"], [BF16] * 4, "meanpool")),
    (plan(training=True, mode="bf16", sync_bn=True), (["in_stats", "bf16", "bf16", "bf16"], [BF16] * 4, "meanpool")),
    # eval: the epilogue GEMMs, unless a backward will follow
    (plan(mode="bf16"), (["in_eval"] + ["bf16_epilogue"] * 3, [BF16, BF16, BF16, F32], "done")),
    (plan(mode="bf16", want_bwd=True), (["in_eval", "bf16", "bf16", "bf16"], [BF16] * 4, "meanpool")),
    (plan(mode="bf16", want_bwd=True, kind="fp8"), (["in_eval", "bf16", "bf16", "bf16"], [BF16] * 4, "meanpool")),
    # the pooled last layer rides in the epilogue for groups of 32, 64 or 128 rows only (the layers before it stay)
    (plan(mode="bf16", pool_rows=64), (["in_eval"] + ["bf16_epilogue"] * 3, [BF16, BF16, BF16, F32], "done")),
    (plan(mode="bf16", pool_rows=128), (["in_eval"] + ["bf16_epilogue"] * 3, [BF16, BF16, BF16, F32], "done")),
    (plan(mode="bf16", pool_rows=16), (["in_eval", "bf16_epilogue", "bf16_epilogue", "bf16"], [BF16] * 4, "meanpool")),
    (plan(mode="bf16", pool_rows=256), (["in_eval", "bf16_epilogue", "bf16_epilogue", "bf16"], [BF16] * 4, "meanpool")),
    (plan(mode="bf16", pool_rows=50, rows=1000), (["in_eval", "bf16_epilogue", "bf16_epilogue", "bf16"], [BF16] * 4, "meanpool")),
    # rows that are no whole number of 256-row tiles: both epilogue GEMMs serve a partial last tile
    (plan(mode="bf16", rows=1056), (["in_eval"] + ["bf16_epilogue"] * 3, [BF16, BF16, BF16, F32], "done")),
    # a layer no epilogue GEMM takes (384 output channels) leaves the bf16 epilogue route alone, layer by layer
    (plan(dims=MID384, mode="bf16"), (["in_eval", "bf16_epilogue", "bf16", "bf16_epilogue"], [BF16, BF16, BF16, F32], "done")),
    # ---- kind "fp8": where the bf16 epilogue route runs, all layers or none
    (plan(mode="bf16", kind="fp8"), (["in_eval", "fp8", "fp8", "fp8"], [FP8, FP8, FP8, F32], "done")),
    (plan(mode="bf16", kind="fp8", rows=1056), (["in_eval", "fp8", "fp8", "fp8"], [FP8, FP8, FP8, F32], "done")),
    (plan(mode="bf16", kind="fp8", pool_rows=0), (["in_eval", "fp8", "fp8", "fp8"], [FP8, FP8, FP8, BF16], "done")),
    (plan(dims=MID384, mode="bf16", kind="fp8"),
     (["in_eval", "bf16_epilogue", "bf16", "bf16_epilogue"], [BF16, BF16, BF16, F32], "done")),
    (plan(mode="bf16", kind="fp8", pool_rows=16), (["in_eval", "bf16_epilogue", "bf16_epilogue", "bf16"], [BF16] * 4, "meanpool")),
    # rows % pool_rows: the fp8 route asks for whole groups; the bf16 epilogue route it falls back to never did
    (plan(mode="bf16", kind="fp8", rows=1000), (["in_eval"] + ["bf16_epilogue"] * 3, [BF16, BF16, BF16, F32], "done")),
    (plan(mode="bf16", kind="fp8", training=True), (["in_moments", "bf16", "bf16", "bf16"], [BF16] * 4, "meanpool")),
    (plan(mode="fp32", kind="fp8"), (["in_eval", "fp32", "fp32", "fp32"], [F32] * 4, "meanpool")),
    # the first layer must be the recompute layer (it writes the e4m3 operand)
    (plan(dims=((9, 512), (512, 512)), mode="bf16", kind="fp8"), (["fp32", "bf16_epilogue"], [BF16, F32], "done")),
    (plan(dims=((4, 512),), mode="bf16", kind="fp8", pool_rows=0), (["in_eval"], [BF16], "done")),
    # ---- fp16x3 mode: split images between the layers, all later layers or none
    (plan(training=True, mode="fp16x3"), (["in_moments", "split3", "split3", "split3"], [SPLIT, SPLIT, SPLIT, F32], "meanpool")),
    (plan(mode="fp16x3"), (["in_eval", "split3", "split3", "split3"], [SPLIT, SPLIT, SPLIT, F32], "meanpool")),
    (plan(mode="fp16x3", want_bwd=True), (["in_eval", "fp32", "fp32", "fp32"], [F32] * 4, "meanpool")),
    (plan(mode="fp16x3", pool_rows=0, last_pre_bn=True), (["in_eval", "split3", "split3", "split3"], [SPLIT, SPLIT, SPLIT, F32], "pre_bn")),
    # a later layer over 128 channels: the product would take it (3 * 128 >= 320), the rule cin % 256 == 0 does not
    (plan(dims=((4, 256), (256, 256), (256, 256)), rows=16384, training=True, mode="fp16x3"),
     (["in_moments", "split3", "split3"], [SPLIT, SPLIT, F32], "meanpool")),
    (plan(dims=((4, 128), (128, 256), (256, 256)), rows=16384, training=True, mode="fp16x3"),
     (["in_moments", "fp32", "fp32"], [F32] * 3, "meanpool")),
    # a later layer the product does not take (384 output channels)
    (plan(dims=MID384, mode="fp16x3"), (["in_eval", "fp32", "fp32", "fp32"], [F32] * 4, "meanpool")),
    # rows that are no whole number of 256-row tiles: served from a contraction of 320 on only
    (plan(dims=((4, 256), (256, 256)), rows=1024, mode="fp16x3", pool_rows=0), (["in_eval", "split3"], [SPLIT, F32], "act")),
    (plan(dims=((4, 256), (256, 256)), rows=1000, mode="fp16x3", pool_rows=0), (["in_eval", "fp32"], [F32] * 2, "act")),
    (plan(rows=1000, mode="fp16x3", pool_rows=0), (["in_eval", "split3", "split3", "split3"], [SPLIT, SPLIT, SPLIT, F32], "act")),
]

# (dtype of a, rows, cin, cout, training, mode, caller is the PointNet stack) -> route
LINEAR = [
    ((SPLIT, 1024, 512, 512, True, "fp16x3", True), "split3"),
    ((SPLIT, 1024, 512, 512, False, "fp16x3", True), "split3"),
    # fp32 rows of at most 8 channels, in the PointNet stack: the streaming kernel with y stored
    ((F32, 1024, 8, 512, True, "fp32", True), "in_store"),
    ((F32, 1024, 8, 512, False, "bf16", True), "in_store"),
    ((F32, 1024, 9, 512, True, "fp32", True), "fp32"),
    ((F32, 1024, 8, 512, True, "fp32", False), "fp32"),
    ((F32, 1024, 4, 24, True, "fp32", True), "fp32"),
    ((BF16, 1024, 8, 512, True, "bf16", True), "bf16"),
    # bf16 rows in bf16 mode, cin % 8 == 0
    ((BF16, 1024, 512, 512, True, "bf16", True), "bf16"),
    ((BF16, 1024, 512, 512, False, "bf16", True), "bf16"),
    ((BF16, 1024, 516, 512, True, "bf16", True), "fp32"),
    ((BF16, 1024, 512, 512, False, "fp32", True), "fp32"),
    ((F32, 1024, 512, 512, True, "bf16", True), "fp32"),
    # the slab rule, term by term.  The temporal block at B * T = 64 rows: one row tile
    ((F32, 64, 3072, 512, True, "fp32", False), "fp32_slabs"),
    ((F32, 64, 3072, 512, False, "fp32", False), "fp32"),                   # training
    ((F32, 1024, 512, 512, True, "bf16", False), "fp32_slabs"),             # fp32 output: outside the PointNet stack ...
    ((F32, 1024, 512, 512, True, "fp32", True), "fp32_slabs"),              # ... or in it in fp32 mode, not in bf16 mode (above)
    ((F32, 3968, 3072, 512, True, "fp32", False), "fp32_slabs"),            # 31 x 4 = 124 output tiles
    ((F32, 4096, 3072, 512, True, "fp32", False), "fp32"),                  # 32 x 4 = 128
    ((F32, 64, 256, 512, True, "fp32", False), "fp32_slabs"),               # split-K 256 // 128 = 2
    ((F32, 64, 255, 512, True, "fp32", False), "fp32"),                     # split-K 1
    ((F32, 64, 3072, 510, True, "fp32", False), "fp32"),                    # cout % 4
    ((F32, 64, 3072, 32, True, "fp32", False), "fp32_slabs"),               # 256 % (32 // 4) == 0
    ((F32, 64, 3072, 24, True, "fp32", False), "fp32"),                     # 256 % (24 // 4) != 0
    ((F32, 64, 3072, 1024, True, "fp32", False), "fp32_slabs"),
    ((F32, 64, 3072, 2048, True, "fp32", False), "fp32"),                   # cout <= 1024
]

# (y is stored, the save is a train-mode one, an incoming gradient is given, the gradient w.r.t. the input is wanted, it is a
# _FusedGrad, its dtype, mode, a contiguous dW destination is given) -> route
IN_BWD = [
    ((False, True, True, False, True, None, "bf16", True), "fused"),
    ((False, True, True, False, True, None, "fp32", False), "fused"),
    ((False, True, True, False, False, BF16, "bf16", True), "onepass"),
    ((False, True, True, False, False, F32, "fp16x3", True), "onepass"),
    ((False, True, True, False, False, F32, "fp32", True), "two_pass"),
    ((False, True, True, False, False, F32, "bf16", True), "two_pass"),
    ((False, True, True, False, False, BF16, "bf16", False), "two_pass"),
    ((False, True, True, False, False, F32, "fp16x3", False), "two_pass"),
    ((True, True, True, False, False, BF16, "bf16", True), "general"),
    ((False, False, True, False, False, BF16, "bf16", True), "general"),
    ((False, True, False, False, False, None, "bf16", True), "general"),
    ((False, True, True, True, False, BF16, "bf16", True), "general"),
    ((False, True, True, True, True, None, "bf16", True), "general"),
]

# frames per chunk that keep the eval PointNet of ENC on the epilogue GEMMs
QUANTUM = {("bf16", 32): 8, ("bf16", 64): 4, ("bf16", 128): 2}


@pytest.fixture(scope="module", autouse=True)
def _tile_loops_on():
    _lib.load().pcaa_gemm_v2_enable(1)           # the library's default; the epilogue and split-image predicates depend on it


@pytest.mark.parametrize("args,want", PLAN)
def test_pointnet_plan(args, want):
    routes, hands, finish = F._pointnet_plan(*args)
    assert (list(routes), list(hands), finish) == want


@pytest.mark.parametrize("args,route", LINEAR)
def test_linear_route(args, route):
    assert F._linear_route(*args) == route


@pytest.mark.parametrize("args,route", IN_BWD)
def test_in_bwd_route(args, route):
    assert F._in_bwd_route(*args) == route


def test_every_route_has_a_case():
    linear = {"split3", "in_store", "bf16", "fp32_slabs", "fp32"}
    assert {r for _, r in LINEAR} == linear
    assert {r for _, (routes, _, _) in PLAN for r in routes} == linear | {"in_moments", "in_stats", "in_eval", "fp8", "bf16_epilogue"}
    assert {h for _, (_, hands, _) in PLAN for h in hands} == {F32, BF16, SPLIT, FP8}
    assert {f for _, (_, _, f) in PLAN} == {"done", "meanpool", "act", "pre_bn"}
    assert {r for _, r in IN_BWD} == {"fused", "onepass", "two_pass", "general"}


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16x3"])
@pytest.mark.parametrize("N", [16, 32, 64, 128, 150, 256])
def test_frame_pad_quantum_is_where_the_plan_pools_in_the_epilogue(N, mode):
    """a chunk of whole 256-row tiles of N-point frames: the quantum differs from 1 exactly where the plan keeps every later
    layer of such a chunk, the pooled one included, on the bf16 epilogue route"""
    q = F.frame_pad_quantum(N, mode)
    assert q == QUANTUM.get((mode, N), 1)
    rows = N * (256 // math.gcd(N, 256))
    routes, _, finish = F._pointnet_plan(*plan(rows=rows, mode=mode, pool_rows=N))
    on_epilogue = all(r == "bf16_epilogue" for r in routes[1:])
    assert (q != 1) == on_epilogue
    assert (finish == "done") == on_epilogue
    if on_epilogue:
        assert (q * N) % 256 == 0 and F._epilogue_pools(N)
