"""What the temporal block launches (functional._dtc_plan), pinned without a GPU against a table written out by hand: the
plan's full answer per case -- per layer and direction: fused or not, the library's ksplit, the bf16 flag, the route
pcaa_dtc_conv_route names for exactly those arguments, and what rides along (the im2col matrix, the window, the epilogue of
the layer below, dy formed on load).  The plan is pure: it launches and allocates nothing, and its rules are library calls
that need no device.  Every route and ksplit of the table is also what the restatement of tests/dtc_ref.py gives, and over
the predicate grid of tests/test_dtc_gates_cpu.py the bf16 flag is ``mode == "bf16" and pair_takes(kc, nc, 1, adj)``.
"""
import pytest
import torch

import dtc_ref as D
from opensetgaitrecognition_pcaa_amd import functional as F, ops

F32, BF16 = torch.float32, torch.bfloat16
BLOCK = ((1024, 16), (16, 32), (32, 64), (64, 128), (128, 256), (256, 512))       # the shipped block, T = 30
WIDE_FIRST = ((256, 64), (64, 128))           # a first layer the two-sequence kernels would take
ODD = ((16, 6), (6, 10), (10, 16))            # DilTempConv1d(6, 10) and its neighbours
COUT20 = ((16, 20), (20, 32))                 # cout % 16 != 0: no fused forward; cin % 4 == cout % 4 == 0: the adjoints are
TO_1024 = ((16, 64), (64, 1024))              # an adjoint over 1024 channels: two splits
MODES = ("fp32", "bf16", "fp16x3")


def plan(dims=BLOCK, B=4, T=30, training=True, want_bwd=False, mode="fp32", windowed=False, fuse=True, a_dtype=F32):
    """the arguments of _dtc_plan, in its order: the defaults are a train-mode pass over 4 sequences of the shipped block"""
    return (dims, B, T, training, want_bwd, mode, windowed, fuse, a_dtype)


def f(ksplit=1, bf16=False, route="one_f32", col=True, window=None):
    return (True, ksplit, bf16, route, col, window)


def b(ksplit=1, bf16=False, route="one_f32", ep=True, dy=True):
    return (True, ksplit, bf16, route, ep, dy)


def nf(window=None):
    return (False, 0, False, None, True, window)        # im2col + _linear_bn: the save always holds the im2col matrix


NB = (False, 0, False, None, False, False)
P32, P64 = dict(bf16=True, route="pair32_bf16"), dict(bf16=True, route="pair64_bf16")
F32_32, F32_64 = dict(route="pair32_f32"), dict(route="pair64_f32")      # the same kernels' exact-fp32 forms: flag off


def block(ks1, fwd5, fwd6, adj4, adj5, adj6, col=True, ep=True):
    """the shipped block: layer 1 splits its 1024 channels, layers 2-4 (forward) / 1-3 (adjoint) are narrow"""
    return ([f(ks1, col=col), f(col=col), f(col=col), f(col=col), f(col=col, **fwd5), f(col=col, **fwd6)],
            [b(ep=False), b(ep=ep), b(ep=ep), b(ep=ep, **adj4), b(ep=ep, **adj5), b(ep=ep, **adj6)])


# arguments -> (the forward plan of each layer, the backward plan of each layer)
PLAN = [
    # ---- the shipped block in bf16 mode: the pair kernels from 128 contraction channels and 64 output channels on (forward:
    # layers 5, 6; adjoint: 4, 5, 6), 64 columns where (B + 1) // 2 * (nc // 64) >= 192.  Layer 1: few long tiles -> ksplit 8
    (plan(mode="bf16"), block(8, P32, P32, P32, P32, P32)),
    (plan(mode="bf16", B=64), block(8, P32, P64, P32, P32, P32)),                 # forward layer 6: 32 * 8 = 256 workgroups
    (plan(mode="bf16", B=65), block(8, P32, P64, P32, P32, P32)),
    (plan(mode="bf16", B=1024), block(4, P64, P64, P64, P64, P64)),               # 1024 // 256 = 4: enough workgroups
    # ---- fp32 and fp16x3 modes: the same ksplits and kernel families, no flag
    (plan(), block(8, F32_32, F32_32, F32_32, F32_32, F32_32)),
    (plan(B=64), block(8, F32_32, F32_64, F32_32, F32_32, F32_32)),
    (plan(mode="fp16x3", B=1024), block(4, F32_64, F32_64, F32_64, F32_64, F32_64)),
    (plan(mode="fp16x3"), block(8, F32_32, F32_32, F32_32, F32_32, F32_32)),
    # ---- eval mode: the im2col matrix only where a backward will follow; eval saves: no epilogue for the layer below
    (plan(training=False, mode="bf16"), block(8, P32, P32, P32, P32, P32, col=False, ep=False)),
    (plan(training=False, want_bwd=True, mode="bf16"), block(8, P32, P32, P32, P32, P32, ep=False)),
    (plan(training=False, want_bwd=True), block(8, F32_32, F32_32, F32_32, F32_32, F32_32, ep=False)),
    # ---- a windowed source (eval): layer 1 reads the table in place, on a one-sequence kernel whatever its shape
    (plan(training=False, mode="bf16", windowed=True),
     ([f(8, col=False, window="in_place")] + block(8, P32, P32, P32, P32, P32, col=False, ep=False)[0][1:],
      block(8, P32, P32, P32, P32, P32, ep=False)[1])),
    (plan(WIDE_FIRST, training=False, mode="bf16", windowed=True),
     ([f(1, True, "one_bf16", col=False, window="in_place"), f(col=False)], [b(ep=False), b(ep=False, **P32)])),
    (plan(WIDE_FIRST, training=False, mode="bf16"),
     ([f(col=False, **P32), f(col=False)], [b(ep=False), b(ep=False, **P32)])),
    (plan(WIDE_FIRST, training=False, windowed=True),
     ([f(col=False, window="in_place"), f(col=False)], [b(ep=False), b(ep=False, **F32_32)])),
    # ... and with the fusion off it is gathered first; nothing is fused in either direction
    (plan(training=False, mode="bf16", windowed=True, fuse=False), ([nf("gather")] + [nf()] * 5, [NB] * 6)),
    (plan(mode="bf16", fuse=False), ([nf()] * 6, [NB] * 6)),
    # ---- shapes the kernels do not take.  The forward is fused for every layer or none; the adjoint layer by layer
    (plan(ODD), ([nf()] * 3, [NB] * 3)),
    (plan(ODD, mode="bf16"), ([nf()] * 3, [NB] * 3)),
    (plan(COUT20), ([nf()] * 2, [b(ep=False), b()])),
    (plan(T=33, mode="bf16"), ([nf()] * 6, [NB] * 6)),
    (plan(T=32, mode="bf16"), block(8, P32, P32, P32, P32, P32)),
    (plan(a_dtype=BF16, mode="bf16"), ([nf()] * 6, block(8, P32, P32, P32, P32, P32)[1])),
    # ---- an adjoint over 1024 channels: dgrad ksplit 2 -- partial products in slabs, so no epilogue for the layer below
    # and dy is not formed on load; the pair kernels need ksplit == 1, the flag is asked at ksplit 1
    (plan(TO_1024), ([f(), f()], [b(ep=False), b(2, ep=False, dy=False)])),
    (plan(TO_1024, mode="bf16"), ([f(), f()], [b(ep=False), b(2, True, "one_bf16", ep=False, dy=False)])),
    # ---- the same in the forward: 512 -> 64 channels at B = 64 is few long tiles (ksplit 8) of a pair shape: flag on, the
    # one-sequence bf16 kernel (no shipped block has such a layer; _dtc_plan's docstring)
    (plan(((512, 64),), B=64, mode="bf16"), ([f(8, True, "one_bf16")], [b(ep=False)])),
    (plan(((512, 64),), B=64), ([f(8)], [b(ep=False)])),
    (plan(((512, 64),), B=65, mode="bf16"), ([f(2, True, "one_bf16")], [b(ep=False)])),       # 130 workgroups: 512 // 256
]


@pytest.mark.parametrize("args,want", PLAN)
def test_dtc_plan(args, want):
    fwd, bwd = F._dtc_plan(*args)
    assert ([tuple(p) for p in fwd], [tuple(p) for p in bwd]) == want
    assert all(p._fields == ("fused", "ksplit", "bf16", "route", "keep_col", "window") for p in fwd)
    assert all(p._fields == ("fused", "ksplit", "bf16", "route", "epilogue", "forms_dy") for p in bwd)


@pytest.mark.parametrize("args,want", PLAN)
def test_the_table_is_what_the_restatement_gives(args, want):
    """ksplit and route of every fused launch of the table, from tests/dtc_ref.py with the table's own flag"""
    dims, B = args[0], args[1]
    assert ops.DTC_ROUTES == D.ROUTES
    for (cin, cout), fw, bw in zip(dims, *want):
        if fw[0]:
            assert fw[1] == D.fwd_ksplit(B, cin, cout)
            assert fw[3] == D.ROUTES[D.route(False, fw[2], B, cin, cout, fw[1], fw[5] is not None)]
        if bw[0]:
            assert bw[1] == D.dgrad_ksplit(B, cin, cout)
            assert bw[3] == D.ROUTES[D.route(True, bw[2], B, cin, cout, bw[1])]


def test_every_value_of_every_field_has_a_case():
    fwd = [p for _, (fw, _) in PLAN for p in fw]
    bwd = [p for _, (_, bw) in PLAN for p in bw]
    col = lambda rows, i: {r[i] for r in rows}
    assert col(fwd, 0) == col(bwd, 0) == {True, False}
    assert col(fwd, 1) == {0, 1, 2, 4, 8} and col(bwd, 1) == {0, 1, 2}
    assert col(fwd, 2) == col(bwd, 2) == {True, False}
    assert col(fwd, 3) == col(bwd, 3) == {None} | set(D.ROUTES)
    assert col(fwd, 4) == {True, False} and col(fwd, 5) == {None, "in_place", "gather"}
    assert col(bwd, 4) == col(bwd, 5) == {True, False}
    args = [a for a, _ in PLAN]
    assert {a[5] for a in args} == set(MODES) and {a[3] for a in args} == {a[4] for a in args} == {True, False}
    assert {a[6] for a in args} == {a[7] for a in args} == {True, False} and {a[8] for a in args} == {F32, BF16}


def test_the_flag_is_the_librarys_pair_rule_at_ksplit_1():
    """over the predicate grid: the flag of a launch, and of a one-layer plan wherever the plan fuses the layer"""
    hit = set()
    for B, cin, cout in D.grid():
        for adj in (False, True):
            kc, nc = (cout, cin) if adj else (cin, cout)
            for mode in MODES:
                want = mode == "bf16" and D.pair_takes(kc, nc, 1, adj)
                ks, flag, route = F._dtc_launch(adj, mode, B, cin, cout)
                assert flag == want, (adj, mode, B, cin, cout)
                assert ks == (D.dgrad_ksplit if adj else D.fwd_ksplit)(B, cin, cout)
                assert route == D.ROUTES[D.route(adj, flag, B, cin, cout, ks)]
                p = F._dtc_plan(((cin, cout),), B, 30, True, False, mode, False, True, F32)[int(adj)][0]
                assert p.fused == bool(cin % 4 == 0 and cout % 4 == 0 if adj else D.supported(30, cin, cout))
                assert tuple(p[:4]) == ((True, ks, flag, route) if p.fused else (False, 0, False, None))
                hit.add((adj, flag, p.fused))
    # (an adjoint the pair kernels take has cin % 4 == 0 and cout % 32 == 0: it is always fused)
    assert hit == {(a, fl, fu) for a in (False, True) for fl in (False, True) for fu in (False, True)} - {(True, True, False)}


def test_the_plan_launches_nothing():
    """plain values in, tuples of plain values out: no tensor, and the same object for the same question"""
    fwd, bwd = F._dtc_plan(*plan(mode="bf16"))
    assert all(isinstance(v, (bool, int, str, type(None))) for p in fwd + bwd for v in p)
    assert F._dtc_plan(*plan(mode="bf16")) is F._dtc_plan(*plan(mode="bf16"))
    assert F._dtc_plan(*plan(mode="bf16", fuse=False)) != F._dtc_plan(*plan(mode="bf16"))
