"""The route choices of the (linear, BatchNorm, ELU) layer backward (functional._wgrad_route, _wgrad_split_k, _dgrad_route),
pinned without a GPU against tables written out by hand: one case on each side of every boundary.  The functions are pure --
they launch nothing and allocate nothing -- and the ``*_supported`` predicates behind the fused dgrads are library calls that
need no device.
"""
import pytest
import torch

from opensetgaitrecognition_pcaa_amd import _lib, functional as F, ops

F32, BF16, SPLIT = torch.float32, torch.bfloat16, ops.SplitImage.dtype
A = 1 << 20                                   # made-up 16-B aligned base addresses: dy at A, lhs at 2A, dW at 3A
ALIGNED, NO_OUT, DW_PLUS_4 = (A, 2 * A, 3 * A), (A, 2 * A), (A, 2 * A, 3 * A + 4)

# (mode, dy dtype, lhs dtype, cout, K, lhs is an im2col matrix, addresses, defer list given, dW_out given) -> route
WGRAD = [
    # a split-image dy: slabs, whatever else holds
    (("fp16x3", SPLIT, SPLIT, 256, 128, False, (), False, True), "split_slabs"),
    (("fp16x3", SPLIT, SPLIT, 256, 128, False, (), False, False), "split_slabs"),
    # fp32 lhs of at most 8 channels that is no im2col matrix: the first PointNet layer's streaming kernel
    (("fp32", F32, F32, 64, 8, False, (), False, True), "pointnet_in"),
    (("bf16", F32, F32, 64, 8, False, (), False, False), "pointnet_in"),
    (("fp32", F32, F32, 64, 9, False, (), False, True), "fp32_aside"),
    (("fp32", F32, F32, 64, 8, True, (), False, True), "fp32_aside"),
    (("fp32", F32, F32, 64, 8, True, ALIGNED, True, True), "grouped"),
    (("fp32", F32, F32, 6, 8, False, (), False, True), "fp32_aside"),
    (("fp32", F32, F32, 6, 8, False, (), False, False), "fp32_inline"),
    (("fp32", F32, F32, 6, 9, False, (), False, False), "fp32_inline"),
    # bf16 operands: the 256 x 256-tile kernel from cout = 256, K = 128 on, both multiples of 8
    (("bf16", BF16, BF16, 256, 128, False, (), False, True), "bf16"),
    (("bf16", BF16, BF16, 256, 128, False, (), False, False), "bf16"),
    (("bf16", BF16, BF16, 248, 128, False, (), False, True), "fp32_aside"),
    (("bf16", BF16, BF16, 256, 120, False, (), False, True), "fp32_aside"),
    (("bf16", BF16, BF16, 256, 132, False, (), False, True), "fp32_aside"),
    (("bf16", BF16, BF16, 260, 128, False, (), False, True), "fp32_aside"),
    (("bf16", F32, BF16, 256, 128, False, (), False, True), "fp32_aside"),
    (("fp32", BF16, BF16, 256, 128, False, (), False, True), "fp32_aside"),
    # fp32 with a defer list: the grouped launch takes cout % 4 == 0, K % 4 == 0 and 16-B aligned bases
    (("fp32", F32, F32, 32, 12, True, ALIGNED, True, True), "grouped"),
    (("fp32", F32, F32, 32, 12, True, NO_OUT, True, False), "grouped"),
    (("fp32", F32, F32, 10, 18, True, ALIGNED, True, True), "fp32_aside"),
    (("fp32", F32, F32, 10, 18, True, NO_OUT, True, False), "fp32_inline"),
    (("fp32", F32, F32, 32, 12, True, DW_PLUS_4, True, True), "fp32_aside"),
    (("fp32", F32, F32, 32, 12, True, (A + 4, 2 * A, 3 * A), True, True), "fp32_aside"),
    (("fp32", BF16, F32, 32, 12, True, ALIGNED, True, True), "fp32_aside"),
    # ... and without one
    (("fp32", F32, F32, 32, 12, True, (), False, True), "fp32_aside"),
    (("fp32", F32, F32, 32, 12, True, (), False, False), "fp32_inline"),
]

# (route, cout, K, rows) -> split-K factor.  pick_split_k by hand: one output tile in each case, so the factor is
# min(target_blocks, depth // (4 * bk)) -- 256 and bk = 64 for the 256-tile routes, 1024 and bk = 32 otherwise
SPLIT_K = [
    (("split_slabs", 256, 128, 4096), 48),         # the contraction is 3 * rows = 12288 deep: 12288 // 256
    (("bf16", 256, 128, 4096), 16),                # 4096 // 256
    (("fp32_aside", 32, 12, 2048), 16),            # 2048 // 128
    (("grouped", 32, 12, 2048), 16),
    (("fp32_inline", 32, 12, 64), 1),              # shallower than 4 * bk
]

Y_SPLIT, Y_BF16 = ((512, 256), F32), ((512, 256), BF16)
# (mode, adjoint, forms_dy, da is a _FusedGrad, dy dtype, rows, cout, K, (shape, dtype) of the y below, below has batch
# statistics) -> route.  The fused forms take rows x K outputs with K % 256 == 0 and a contraction (cout) that is a multiple
# of 64 and >= 320 (bf16) / >= 107 (split: three passes) -- tests/gemm_ref.py dgrad_bn_supported, split3_supported
DGRAD = [
    (("fp32", True, True, True), "adjoint_dy"),
    (("fp32", True, False, True), "adjoint"),
    (("fp32", True, True, False), "adjoint"),
    (("bf16", True, False, False, F32, 512, 512, 256, Y_BF16, True), "adjoint"),
    (("fp16x3", False, False, False, SPLIT, 512, 128, 256, Y_SPLIT, True), "split_bn"),
    (("fp16x3", False, False, True, SPLIT, 512, 128, 256, Y_SPLIT, True), "split_bn"),
    (("fp16x3", False, False, False, SPLIT, 512, 128, 256, None, False), "split"),
    (("fp16x3", False, False, False, SPLIT, 512, 128, 256, Y_SPLIT, False), "split"),
    (("fp16x3", False, False, False, SPLIT, 512, 128, 256, Y_BF16, True), "split"),
    (("fp16x3", False, False, False, SPLIT, 512, 128, 256, ((512, 128), F32), True), "split"),
    (("fp16x3", False, False, False, SPLIT, 512, 128, 128, ((512, 128), F32), True), "split"),     # K % 256: refused
    (("bf16", False, False, False, BF16, 512, 512, 256, Y_BF16, True), "bf16_bn"),
    (("bf16", False, False, False, BF16, 512, 512, 256, None, False), "bf16"),
    (("bf16", False, False, False, BF16, 512, 512, 256, Y_BF16, False), "bf16"),
    (("bf16", False, False, False, BF16, 512, 512, 256, Y_SPLIT, True), "bf16"),
    (("bf16", False, False, False, BF16, 512, 512, 256, ((256, 256), BF16), True), "bf16"),
    (("bf16", False, False, False, BF16, 512, 256, 256, Y_BF16, True), "bf16"),                   # cout < 320: refused
    (("bf16", False, False, False, BF16, 512, 516, 256, Y_BF16, True), "fp32"),                   # cout % 8 != 0
    (("bf16", False, False, False, F32, 512, 512, 256, Y_BF16, True), "fp32"),
    (("fp32", False, False, False, BF16, 512, 512, 256, Y_BF16, True), "fp32"),
    (("fp32", False, False, False, F32, 512, 512, 256, None, False), "fp32"),
]


@pytest.fixture(scope="module", autouse=True)
def _tile_loops_on():
    _lib.load().pcaa_gemm_v2_enable(1)           # the library's default; the fused forms' predicates depend on it


@pytest.mark.parametrize("args,route", WGRAD)
def test_wgrad_route(args, route):
    assert F._wgrad_route(*args) == route


@pytest.mark.parametrize("args,sk", SPLIT_K)
def test_wgrad_split_k(args, sk):
    assert F._wgrad_split_k(*args) == sk


@pytest.mark.parametrize("args,route", DGRAD)
def test_dgrad_route(args, route):
    assert F._dgrad_route(*args) == route


def test_every_route_has_a_case():
    assert {r for _, r in WGRAD} == {"split_slabs", "pointnet_in", "bf16", "grouped", "fp32_aside", "fp32_inline"}
    assert {a[0] for a, _ in SPLIT_K} == {r for _, r in WGRAD} - {"pointnet_in"}     # (that kernel has no split-K)
    assert {r for _, r in DGRAD} == {"adjoint_dy", "adjoint", "split_bn", "split", "bf16_bn", "bf16", "fp32"}
