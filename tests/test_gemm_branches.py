"""Every dispatch branch of the GEMM launchers (csrc/gemm.hip, csrc/gemm_bf16.hip, csrc/gemm_v2.h) against fp64.

References, gates, the route table and the case lists: tests/gemm_ref.py; the gates are shown reference-safe and
defect-sensitive, and the case lists complete, by tests/test_gemm_gates_cpu.py.  Every case names the route it means to
reach (``gemm_ref.route`` restates the launchers; the library reports the kernel it plans -- pcaa_gemm_route, asked
before every product launch -- and the one the launch started -- pcaa_gemm_last_kernel, asked after it: both must be the
kernel the route name implies; a carried BatchNorm tail, which only the LDS-DMA loops take, is asserted too), computes the result, the
fp64 reference of the same stored operands and the gate, asserts |got - want| <= gate for EVERY element and prints the
worst ratio (pytest -rP).  Operands live inside NaN-filled allocations (leading-dimension padding, the element in front
of a misaligned base, the memory behind the last row); outputs inside sentinel-filled ones that must come back
bit-identical outside the logical window.

    test                                     entry points and branches
    ---------------------------------------  ------------------------------------------------------------------------
    test_product[...]                        pcaa_gemm / ops.gemm, pcaa_gemm_slabs + ops.splitk_reduce (+ ops.gemm_slabs,
                                             ops.gemm_slabs_part), ops.gemm_split3, ops.gemm_slabs_split3: gemm_ref.gemm_cases
    test_fused[...]                          ops.gemm_dgrad_bn, ops.gemm_dgrad_bn_split3 (and their ABI with ld > N),
                                             ops.gemm_affine_elu with pool_rows 0 / 32 / 64 / 128: gemm_ref.fused_cases
    test_group_launch                        ops.gemm_group_rc_f32 (slabs) and pcaa_gemm_group_rc_f32 (atomics): 1, 3, 8 products
    test_ticket_counters_return_to_zero      two launches over the CU count on one stream, a third on another
    test_split_fast_against_...              the split_fast product against the same product on the ordinary grid
    test_refusals, test_abi_refusals         one call per PCAA_CHECK_ARG of csrc/gemm.hip (gemm_ref.REFUSALS, ABI_REFUSALS): the
                                             error code, the message, an untouched output
    test_supported_predicates                pcaa_gemm_*_supported against the entry points' verdicts, v2 on and off
    test_lab_switches_in_a_child_process     PCAA_GEMM_TICKETS=0 (the fixed-share walk) and PCAA_GEMM_V2_RC=0; one timed launch
                                             per event kind of ops.LaunchTimer (TIMED)
Not covered: operands beyond 4 GiB (flat addressing, the 4 GiB refusals), more than 128 streams, a stream capture as the
first launch of a device (capture-time slot allocation).
"""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

import elementwise_ref as E
import gemm_ref as G
from gemm_ref import BF16, F32, KC, RC

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 7.0


def _ops():
    from opensetgaitrecognition_pcaa_amd import _lib, ops
    return _lib.load(), ops


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


WORST = {}


def check(name, got, want, gate, route=None):
    err = (got.double() - want).abs() / gate.clamp_min(1e-300)
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    r = float(err.max()) if err.numel() else 0.0
    print(f"[gemm] {name}: worst |err| / gate = {r:.3f}" + (f"   route {route}" if route else ""))
    if route:
        WORST[route] = max(WORST.get(route, 0.0), r)
    if not r <= 1.0:
        at = [int(i) for i in torch.unravel_index(err.argmax(), err.shape)]
        over = (err > 1.0).nonzero()
        print(f"[gemm] {name}: worst at {at}; {over.shape[0]} of {err.numel()} over the gate, first {over[:8].tolist()}")
    assert r <= 1.0, (name, r)
    return r


def dt(t):
    return 1 if t == BF16 else 0        # PCAA_BF16 / PCAA_F32


def ptr(t):
    return None if t is None else t.data_ptr()


class Out:
    """an [M, N] output window (row stride ldc, one element off a 16-B boundary on request) inside a sentinel-filled buffer"""

    def __init__(self, M, N, dtype, ldc=None, off=0, init=None, tail=4096):
        ldc = N if ldc is None else ldc
        self.buf = torch.full((off + M * ldc + tail,), SENT, dtype=dtype, device=DEV)
        self.win = self.buf[off:off + M * ldc].view(M, ldc)[:, :N]
        self.ldc = ldc
        if init is not None:
            self.win.copy_(init)

    def take(self):
        """-> the window's contents; asserts everything around it is bit-identical to the sentinel"""
        torch.cuda.synchronize()
        got = self.win.clone()
        self.win.fill_(SENT)
        assert bool((self.buf == SENT).all()), "memory outside the output window was written"
        return got


def bn_module(N):
    bn = torch.nn.BatchNorm1d(N).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(G.uniform(N, 11, DEV, 0.7, 1.3).float())
        bn.bias.copy_(G.uniform(N, 12, DEV, -0.5, 0.5).float())
        bn.running_mean.copy_(G.uniform(N, 13, DEV, -0.3, 0.3).float())
        bn.running_var.copy_(G.uniform(N, 14, DEV, 0.5, 1.5).float())
    return bn


def check_fwd_tail(name, ops, tail, stats, bn, rm0, rv0, count, expect_taken, taken0):
    """the finalize a launch carried (or the stand-alone one it fell back to) against fp64 of the launch's own statistics"""
    torch.cuda.synchronize()
    assert (ops.TAILS["taken"] - taken0 == 1) == expect_taken, (name, "BatchNorm tail carried by the launch", expect_taken)
    mom = ops.BN_MOMENTUM if bn.momentum is None else bn.momentum
    ref = E.bn_finalize_ref(stats, count, None, bn.weight, bn.bias, rm0, rv0, mom, bn.eps)
    for k, t in zip(("scale", "shift", "mean", "rstd"), tail.out):
        check(f"{name} tail {k}", t, *ref[k])
    check(f"{name} tail running_mean", bn.running_mean, *ref["running_mean"])
    check(f"{name} tail running_var", bn.running_var, *ref["running_var"])


# ===================================================================================================== products
def launch_product(c, bt, out, stats, lib, ops, tail=None, via_ops=True):
    """one launch of a product case into ``out`` (slab cases: into the slab buffer ``out``); -> the return code"""
    A, B = bt["A"], bt["B"]
    M, N, K = bt["M"], bt["N"], c["K"]
    if c["split3"]:
        sa, sb = G.SPLIT_SCALES
        if c["slabs"]:
            return lib.pcaa_gemm_slabs_split3(ptr(A), ptr(B), c["alay"], A.stride(0), B.stride(0), ptr(out.win), M * N, M, N, K,
                                              c["split_k"], 1.0 / (sa * sb), ops._s())
        if via_ops and out.ldc == N and not c["misaligned"]:
            ia = ops.SplitImage(A, *((M, K) if c["alay"] == KC else (K, M)), sa)
            ib = ops.SplitImage(B, *((N, K) if c["blay"] == KC else (K, N)), sb)
            ops.gemm_split3(ia, ib, c["alay"], M, N, K, colstats=stats, tail=tail, out=out.win)
            return 0
        return lib.pcaa_gemm_split3(ptr(A), ptr(B), c["alay"], A.stride(0), B.stride(0), ptr(out.win), out.ldc, M, N, K, ptr(stats),
                                    c["nrep"], 1.0 / (sa * sb), ops._s())
    if c["slabs"]:
        return lib.pcaa_gemm_slabs(c["math"], ptr(A), dt(A.dtype), c["alay"], A.stride(0), ptr(B), dt(B.dtype), c["blay"], B.stride(0),
                                   ptr(out.win), M * N, M, N, K, c["split_k"], ops._s())
    dense = A.is_contiguous() and B.is_contiguous() and out.ldc == N and c["nrep"] == 16
    if via_ops and dense:
        ops.gemm(A, c["alay"], B, c["blay"], M, N, K, out=out.win, bias=bt["bias"], colstats=stats, split_k=c["split_k"],
                 accumulate=c["accumulate"], math=c["math"], tail=tail)
        return 0
    if tail is not None:
        tail.arm(stats)
    rc = lib.pcaa_gemm(c["math"], ptr(A), dt(A.dtype), c["alay"], A.stride(0), ptr(B), dt(B.dtype), c["blay"], B.stride(0), ptr(out.win),
                       dt(c["cdt"]), out.ldc, M, N, K, ptr(bt["bias"]), ptr(stats), c["nrep"], c["split_k"], int(c["accumulate"]),
                       ops._s())
    if tail is not None:
        tail.resolve(stats)
    return rc


def planned_kernel(c, bt, out, stats, lib):
    """pcaa_gemm_route / pcaa_gemm_split3_route for the call launch_product is about to make"""
    A, B = bt["A"], bt["B"]
    M, N, K = bt["M"], bt["N"], c["K"]
    stride = M * N if c["slabs"] else 0
    if c["split3"]:
        return lib.pcaa_gemm_split3_route(ptr(A), ptr(B), c["alay"], A.stride(0), B.stride(0), ptr(out.win), N if c["slabs"] else out.ldc,
                                          M, N, K, ptr(stats), c["nrep"], c["split_k"], stride, 1.0)
    return lib.pcaa_gemm_route(c["math"], ptr(A), dt(A.dtype), c["alay"], A.stride(0), ptr(B), dt(B.dtype), c["blay"], B.stride(0),
                               ptr(out.win), dt(c["cdt"]), out.ldc, M, N, K, ptr(bt["bias"]), ptr(stats), c["nrep"], c["split_k"],
                               int(c["accumulate"]), stride)


def new_out(c, bt, ns=1):
    M, N = bt["M"], bt["N"]
    if c["slabs"]:
        return Out(ns, M * N, F32)
    atomic = c["split_k"] > 1 or c["accumulate"]
    init = bt["out0"] if c["accumulate"] else (torch.zeros((M, N), device=DEV) if atomic else None)
    return Out(M, N, c["cdt"], c["ldc"], 1 if "C" in c["misaligned"] else 0, init)


def run_product(c, tickets=True, rc_on=True):
    lib, ops = _ops()
    route = G.case_route(c, n_cu(), tickets=tickets, rc_on=rc_on)
    if tickets and rc_on:
        assert route == c["route"], (c["id"], "the case means to reach", c["route"], "the launchers' rules give", route)
    ops.gemm_v2_enable(c["v2_on"])
    try:
        bt = G.build(c, DEV)
        p = G.reference(dict(c, route=route), bt)
        M, N, K = c["M"], c["N"], c["K"]
        ns = len(p["slabs"]) if c["slabs"] else 1
        if c["slabs"]:
            want_ns = lib.pcaa_gemm_split3_num_splits(K, c["split_k"]) if c["split3"] else lib.pcaa_gemm_num_splits(c["math"], K, c["split_k"])
            assert ns == want_ns
        out = new_out(c, bt, ns)
        stats = tail = bn = None
        if c["colstats"]:
            stats = ops.new_stats(N, DEV) if c["nrep"] == 16 else torch.zeros((c["nrep"], 2, N), dtype=torch.float64, device=DEV)
        if c["tail"]:
            bn = bn_module(N)
            rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
            tail = ops.BnTailFwd(M, None, bn, N)
            taken0 = ops.TAILS["taken"]
        planned = planned_kernel(c, bt, out, stats, lib)
        rc = launch_product(c, bt, out, stats, lib, ops, tail)
        assert rc == 0, (c["id"], rc, lib.pcaa_last_error())
        assert lib.pcaa_gemm_last_kernel() == G.kernel_id(route) == planned, (c["id"], route, planned, lib.pcaa_gemm_last_kernel())
        got = out.take()
        for buf in bt["bufs"]:
            assert bool(torch.isnan(buf[-64:].float()).all())
        if c["slabs"]:
            for s, (w, g) in enumerate(p["slabs"]):
                check(f"{c['id']} slab {s}", got[s].view(M, N), w, g, route)
            red = Out(M, N, F32)
            ops.splitk_reduce(got.reshape(-1), ns, M, N, red.win)
            res = red.take()
            check(f"{c['id']} reduced", res, p["want"], p["gate"], route)
            if bt["A"].is_contiguous() and bt["B"].is_contiguous():     # the ops-level entry points give the same bits
                if c["split3"]:
                    ia = ops.SplitImage(bt["A"], K, M, G.SPLIT_SCALES[0])
                    ib = ops.SplitImage(bt["B"], K, N, G.SPLIT_SCALES[1])
                    assert torch.equal(ops.gemm_slabs_split3(ia, ib, M, N, K, c["split_k"]), res)
                else:
                    assert torch.equal(ops.gemm_slabs(bt["A"], c["alay"], bt["B"], c["blay"], M, N, K, c["split_k"], math=c["math"]), res)
                    if c["alay"] == RC and c["blay"] == RC:
                        part = torch.empty(ns * M * N, dtype=F32, device=DEV)
                        assert ops.gemm_slabs_part(bt["A"], bt["B"], M, N, K, c["split_k"], part, math=c["math"]) == ns
                        assert torch.equal(part.view(ns, M * N), got)
        else:
            check(c["id"], got, p["want"], p["gate"], route)
        if c["colstats"]:
            check(f"{c['id']} colstats", stats, p["stats"], p["stats_gate"], route)
        if c["tail"]:
            check_fwd_tail(c["id"], ops, tail, stats, bn, rm0, rv0, M, route.startswith("v2/") and route.endswith("/tail"), taken0)
    finally:
        ops.gemm_v2_enable(True)


CASES = G.gemm_cases(n_cu())


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_product(c):
    run_product(c)


# ===================================================================================================== fused epilogues
def run_fused(c):
    lib, ops = _ops()
    M, N, K = c["M"], c["N"], c["K"]
    ld = c["ld"] or N
    need = 2 * K if c["split3"] else K
    assert G.route_fused(c["epi"], M, N, K, need, need, ld, True, n_cu(), split3=c["split3"], pool_rows=c["pool_rows"],
                         tail=c["tail"]) == c["route"]
    bt = G.fused_inputs(c, DEV)
    ref = G.fused_reference(c, bt)
    A, B = bt["A"], bt["B"]
    if c["epi"] == "affine":
        got = ops.gemm_affine_elu(A, B, bt["scale"], bt["shift"], c["pool_rows"])
        assert lib.pcaa_gemm_last_kernel() == G.kernel_id(c["route"]), (c["id"], c["route"], lib.pcaa_gemm_last_kernel())
        torch.cuda.synchronize()
        check(c["id"], got, ref["want"], ref["gate"], c["route"])
        return
    stats = ops.new_stats(N, DEV)
    tail = None
    if c["tail"]:
        bn = bn_module(N)
        tail = ops.BnTailBwd(M, bn, bt["mean"], bt["rstd"], N)
        taken0 = ops.TAILS["taken"]
    ydt = F32 if c["split3"] else BF16
    dz = Out(M, N, ydt, ld)
    if tail is not None:
        tail.arm(stats)
    sc = (ptr(bt["scale"]), ptr(bt["shift"]), ptr(bt["mean"]), ptr(bt["rstd"]), ptr(stats), 16, M, N, K)
    if c["split3"]:
        rc = lib.pcaa_gemm_dgrad_bn_split3(ptr(A), A.stride(0), ptr(B), B.stride(0), ptr(bt["y"]), ptr(dz.win), ld, *sc,
                                           1.0 / (G.SPLIT_SCALES[0] * G.SPLIT_SCALES[1]), ops._s())
    else:
        rc = lib.pcaa_gemm_dgrad_bn(ptr(A), A.stride(0), ptr(B), B.stride(0), ptr(bt["y"]), ptr(dz.win), ld, *sc, None, 0, None, ops._s())
    assert rc == 0, (c["id"], lib.pcaa_last_error())
    assert lib.pcaa_gemm_last_kernel() == G.kernel_id(c["route"]), (c["id"], c["route"], lib.pcaa_gemm_last_kernel())
    if tail is not None:
        tail.resolve(stats)
    got = dz.take()
    check(f"{c['id']} dz", got, ref["dz"], ref["dz_gate"], c["route"])
    check(f"{c['id']} stats", stats, ref["stats"], ref["stats_gate"], c["route"])
    if tail is not None:
        assert ops.TAILS["taken"] - taken0 == 1, "the fused dgrad carries the backward finalize"
        fin = E.bn_bwd_finalize_ref(stats, M, bn.weight, bt["mean"], bt["rstd"])
        coef, dgamma, dbeta = tail.out
        for k, t in (("coef0", coef[0]), ("coef1", coef[1]), ("coef2", coef[2]), ("dgamma", dgamma), ("dbeta", dbeta)):
            check(f"{c['id']} tail {k}", t, *fin[k])
    if ld == N:                                    # the ops-level entry point: the same bits
        y = bt["y"]
        if c["split3"]:
            ia, ib = ops.SplitImage(A, M, K, G.SPLIT_SCALES[0]), ops.SplitImage(B, N, K, G.SPLIT_SCALES[1])
            dz2, st2 = ops.gemm_dgrad_bn_split3(ia, ib, y, bt["scale"], bt["shift"], bt["mean"], bt["rstd"])
        else:
            dz2, st2 = ops.gemm_dgrad_bn(A, B, y, bt["scale"], bt["shift"], bt["mean"], bt["rstd"])
        assert torch.equal(dz2, got)
        check(f"{c['id']} stats (ops)", st2, ref["stats"], ref["stats_gate"], c["route"])


FUSED = G.fused_cases(n_cu())


@pytest.mark.parametrize("c", FUSED, ids=[c["id"] for c in FUSED])
def test_fused(c):
    run_fused(c)


# ===================================================================================================== group launch
GROUPS = {1: [(132, 136, 100, 3)],
          3: [(4, 8, 33, 1), (260, 132, 64, 2), (128, 128, 200, 9)],
          8: [(4 * (i + 1), 136 - 8 * i, 40 + 37 * i, 1 + i) for i in range(8)]}


@pytest.mark.parametrize("n", [1, 3, 8])
@pytest.mark.parametrize("form", ["slabs", "atomics"])
def test_group_launch(n, form):
    lib, ops = _ops()
    prods, refs = [], []
    for i, (M, N, K, sk) in enumerate(GROUPS[n]):
        xa, xb = G.logical(M, K, G.seed_of(M, N, K, 20), DEV), G.logical(N, K, G.seed_of(M, N, K, 21), DEV, (3.0 / K) ** 0.5)
        (_, A), (_, B) = G.operand(xa, F32, RC), G.operand(xb, F32, RC)
        c0 = G.uniform(M * N, G.seed_of(M, N, K, 22), DEV, -1.0, 1.0).float().view(M, N)
        out = Out(M, N, F32, init=c0)
        prods.append((A, B, out, sk))
        refs.append(G.product_ref(G.widen(A, RC, 0), G.widen(B, RC, 0), exact=False, math=G.M_F32, split_k=sk, out0=c0, tile=128))
    if form == "slabs":
        ops.gemm_group_rc_f32([(A, B, o.win, sk) for A, B, o, sk in prods])
    else:
        arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
        ints = lambda vs: (ctypes.c_int * n)(*[int(v) for v in vs])
        rc = lib.pcaa_gemm_group_rc_f32(n, arr([p[0] for p in prods]), arr([p[1] for p in prods]), arr([p[2].win for p in prods]),
                                        ints([p[0].shape[1] for p in prods]), ints([p[1].shape[1] for p in prods]),
                                        ints([p[0].shape[0] for p in prods]), ints([p[3] for p in prods]), ops._s())
        assert rc == 0, lib.pcaa_last_error()
    for i, ((A, B, o, sk), p) in enumerate(zip(prods, refs)):
        ns = G.num_splits(G.M_F32, A.shape[0], sk)[0]
        check(f"group of {n} ({form}) product {i} {tuple(GROUPS[n][i])}, {ns} ranges", o.take(), p["want"], p["gate"], f"group/{form}")


# ===================================================================================================== ticket counters
def test_ticket_counters_return_to_zero():
    """two launches over the CU count back to back on one stream (the second starts from the counters the first left:
    they must be back at zero), then a third on another stream (its own slot)"""
    lib, ops = _ops()
    c = next(c for c in CASES if c["id"] == "v2-tickets-r77-bf16-nobias-nostats")
    bt = G.build(c, DEV)
    p = G.reference(c, bt)
    outs = [new_out(c, bt) for _ in range(3)]
    for o in outs[:2]:
        assert launch_product(c, bt, o, None, lib, ops) == 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert launch_product(c, bt, outs[2], None, lib, ops) == 0
    torch.cuda.current_stream().wait_stream(side)
    got = [o.take() for o in outs]
    for i, g in enumerate(got):
        check(f"ticket draw, launch {i}", g, p["want"], p["gate"], c["route"])
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])


def test_split_fast_against_the_same_product_in_fewer_ranges():
    """split_fast (8 ranges, 256 workgroups, every tile of one range on one XCD) and the same product asked for 7 ranges (4,
    the ordinary grid): each within its gate of fp64 (test_product), and of each other within the two gates together"""
    lib, ops = _ops()
    res = {}
    for cid in ("v2rc-split-fast-8", "v2rc-not-split-fast-7"):
        c = next(c for c in CASES if c["id"] == cid)
        bt = G.build(c, DEV)
        p = G.reference(c, bt)
        res[cid] = (ops.gemm_slabs(bt["A"], RC, bt["B"], RC, c["M"], c["N"], c["K"], c["split_k"]), p)
    (fast, pf), (slow, ps) = res["v2rc-split-fast-8"], res["v2rc-not-split-fast-7"]
    assert len(pf["slabs"]) == 8 and len(ps["slabs"]) == 4
    check("split_fast against 4 ranges", fast, slow.double(), pf["gate"] + ps["gate"])


# ===================================================================================================== refusals
@pytest.mark.parametrize("reason", [r for r, v in G.REFUSALS.items() if v is not None])
def test_refusals(reason):
    """every refusal the route table names: PCAA_ERR_INVALID_ARG with that check's message, before anything is launched"""
    lib, ops = _ops()
    c = G.refusal_case(reason)
    if "epi" in c:
        M, N, K = c["M"], c["N"], c["K"]
        ld = c["ld"] or N
        assert G.refusal_route(c, n_cu()) == "refused/" + reason
        a = torch.zeros(M * K + 8, dtype=BF16, device=DEV)[(1 if "A" in c["misaligned"] else 0):]
        w = torch.zeros(N * K + 8, dtype=BF16, device=DEV)
        v = torch.zeros(N, device=DEV)
        out = Out(M, N, BF16, ld)
        if c["epi"] == "dgrad":
            st = ops.new_stats(N, DEV)
            rc = lib.pcaa_gemm_dgrad_bn(ptr(a), K, ptr(w), K, ptr(out.buf), ptr(out.win), ld, ptr(v), ptr(v), ptr(v), ptr(v), ptr(st), 16,
                                        M, N, K, None, 0, None, ops._s())
        else:
            rc = lib.pcaa_gemm_affine_elu(ptr(a), K, ptr(w), K, ptr(out.win), ld, ptr(v), ptr(v), M, N, K, c["pool_rows"], ops._s())
        refused(lib, rc, reason)
        out.take()
        return
    assert G.refusal_route(c, n_cu()) == "refused/" + reason
    K = c["K"]
    c_build = dict(c, K=max(K, 8), lda=None, ldb=None)
    bt = G.build(c_build, DEV)
    if c["lda"]:                                   # a leading dimension the operand does not have: the call must not get that far
        bt["A"] = bt["A"].as_strided(bt["A"].shape, (c["lda"], 1))
    out = new_out(c, bt)
    stats = torch.zeros((16, 2, c["N"]), dtype=torch.float64, device=DEV) if c["colstats"] else None
    rc = launch_product(c, bt, out, stats, lib, ops, via_ops=False)
    refused(lib, rc, reason)
    out.take()
    assert stats is None or not bool(stats.any())


ABI_ARGS = {
    "gemm": "math=1 A a_dtype=1 a_layout=0 lda=K B b_dtype=1 b_layout=0 ldb=K C c_dtype=0 ldc=N M N K bias=NULL colstats=NULL nrep=16 "
            "split_k=1 accumulate=0",
    "slabs": "math=1 A a_dtype=1 a_layout=1 lda=M B b_dtype=1 b_layout=1 ldb=N slabs slab_stride=MN M N K split_k=2",
    "slabs_split3": "A B layout=1 lda=2M ldb=2N slabs slab_stride=MN M N K split_k=2 out_scale=1.0",
    "split3": "A B layout=0 lda=2K ldb=2K C ldc=N M N K colstats=NULL nrep=16 out_scale=1.0",
    "dgrad": "dy lddy=K Wt ldw=K y dz ld=N scale shift mean rstd stats nrep=16 M N K x=NULL xc=0 W1=NULL",
    "dgrad_split3": "dy lddy=2K Wt ldw=2K y dz ld=N scale shift mean rstd stats nrep=16 M N K out_scale=1.0",
    "affine": "A lda=K W ldw=K out ldo=N scale shift M N K pool_rows=0",
}
ABI_FN = {"gemm": "pcaa_gemm", "slabs": "pcaa_gemm_slabs", "slabs_split3": "pcaa_gemm_slabs_split3", "split3": "pcaa_gemm_split3",
          "dgrad": "pcaa_gemm_dgrad_bn", "dgrad_split3": "pcaa_gemm_dgrad_bn_split3", "affine": "pcaa_gemm_affine_elu"}
OUTPUTS = ("C", "slabs", "dz", "out")


def refused(lib, rc, reason, prefix=None, frag=None):
    """PCAA_ERR_INVALID_ARG (1) with the message of that check: a shape that got past the checks and failed at launch (2) is no refusal"""
    if prefix is None:
        prefix, frag = G.REFUSAL_MESSAGES[reason]
    msg = (lib.pcaa_last_error() or b"").decode()
    assert rc == 1, (reason, rc, msg)
    assert msg.startswith(prefix) and frag in msg, (reason, msg)


@pytest.mark.parametrize("i", range(len(G.ABI_REFUSALS)), ids=[f"{e}-{f.replace(' ', '_')}-{'-'.join(o)}" for e, _, f, o in G.ABI_REFUSALS])
def test_abi_refusals(i):
    """the argument checks the route table does not name (null pointers, dtype / layout codes, slab strides, the group launch,
    each fused entry point's own copy of the shape, leading-dimension, ragged-output and alignment checks): a valid call with
    ONE argument changed is refused with PCAA_ERR_INVALID_ARG and that check's message, and writes nothing"""
    lib, ops = _ops()
    entry, prefix, frag, over = G.ABI_REFUSALS[i]
    zeros = lambda n, dtype=F32: torch.zeros(n, dtype=dtype, device=DEV)
    out = Out(1, 1 << 20, F32)
    stats = zeros(16 * 2 * 1024, torch.float64)
    if entry == "group":
        n, M0, K0 = over.get("n", 1), over.get("M0", 132), over.get("K0", 40)
        a, b = zeros(1 << 16), zeros(1 << 16)
        m = max(n, 1)
        arr = lambda p: (ctypes.c_void_p * m)(*[p] * m)
        ints = lambda v: (ctypes.c_int * m)(*[v] * m)
        rc = lib.pcaa_gemm_group_rc_f32(n, arr(a.data_ptr() + (4 if over.get("A0") else 0)), arr(b.data_ptr()), arr(out.win.data_ptr()),
                                        ints(M0), ints(136), ints(K0), ints(1), ops._s())
    else:
        dims = {k: over.get(k, v) for k, v in (("M", 256), ("N", 256), ("K", 320))}
        M, N, K = dims["M"], dims["N"], dims["K"]
        sym = {"K": K, "N": N, "M": M, "2K": 2 * K, "2M": 2 * M, "2N": 2 * N, "MN": M * N, "NULL": None}
        bufs = {}
        args = []
        for tok in ABI_ARGS[entry].split():
            name, _, default = tok.partition("=")
            if name in dims:
                val = dims[name]
            elif default:
                val = sym[default] if default in sym else (float(default) if "." in default else int(default))
            else:
                bufs[name] = out.win if name in OUTPUTS else (stats if name == "stats" else zeros(1 << 20))
                val = bufs[name].data_ptr()
            if name in over and name not in dims:
                o = over[name]
                val = None if o == "NULL" else (val + 4 if o == "+4" else (stats.data_ptr() if o == "stats" else
                                                                           (zeros(64).data_ptr() if o == "vec" else o)))
            args.append(val)
        rc = getattr(lib, ABI_FN[entry])(*args, ops._s())
    refused(lib, rc, entry, prefix, frag)
    out.take()
    assert not bool(stats.any())


def test_supported_predicates():
    """pcaa_gemm_split3_supported / pcaa_gemm_dgrad_bn_supported agree with gemm_ref's restatement and with the verdict
    of the entry points themselves, with the 4-wave loops on and off"""
    lib, ops = _ops()
    try:
        for v2 in (True, False):
            ops.gemm_v2_enable(v2)
            for M in (256, 300):
                for N in (256, 260):
                    for K in (64, 128, 256, 320):
                        s3, dg = bool(lib.pcaa_gemm_split3_supported(M, N, K)), bool(lib.pcaa_gemm_dgrad_bn_supported(M, N, K))
                        assert s3 == G.split3_supported(M, N, K, v2) and dg == G.dgrad_bn_supported(M, N, K, v2), (M, N, K, v2)
                        c = G._c("p", None, M, N, K, split3=True, v2_on=v2)
                        bt = G.build(c, DEV)
                        out = new_out(c, bt)
                        rc = launch_product(c, bt, out, None, lib, ops, via_ops=False)
                        assert (rc == 0) == s3, (M, N, K, v2, "pcaa_gemm_split3")
                        out.take() if rc else torch.cuda.synchronize()
                        fc = dict(id="p", epi="dgrad", M=M, N=N, K=K, ld=None, tail=False, split3=False, pool_rows=0, route="")
                        fb = G.fused_inputs(fc, DEV)
                        dz, st = Out(M, N, BF16), ops.new_stats(N, DEV)
                        rc = lib.pcaa_gemm_dgrad_bn(ptr(fb["A"]), K, ptr(fb["B"]), K, ptr(fb["y"]), ptr(dz.win), N, ptr(fb["scale"]),
                                                    ptr(fb["shift"]), ptr(fb["mean"]), ptr(fb["rstd"]), ptr(st), 16, M, N, K, None, 0,
                                                    None, ops._s())
                        assert (rc == 0) == dg, (M, N, K, v2, "pcaa_gemm_dgrad_bn")
                        torch.cuda.synchronize()
    finally:
        ops.gemm_v2_enable(True)


# ===================================================================================================== lab switches
CHILD_IDS = ("v2-tickets-r0-bf16-nobias-stats-tail", "v2-tickets-r77-f32-bias-stats", "split3-tickets-r77-stats", "v2rc-one-pass",
             "v2rc-slabs-one-step-each", "v2rc-split-fast-8")


# the smallest shapes that reach each event kind of ops.LaunchTimer: (case, key, kernel-exact events)
TIMED = [(G._c("timed-v2-kc", "v2/plain/whole/one_tile_each/nobias/nostats/notail", 256, 256, 320, cdt=BF16), "gemm_bf16_v2_kernel<bf16,plain>", True),
         (G._c("timed-staged", "bf16_staged/bf16,bf16,f32,KC,KC", 256, 256, 64), "gemm_bf16_big_kernel<f32,KC,KC>", False)]


def run_timed(c, key, kernel_exact):
    """one ops.gemm under a LaunchTimer: exactly one record, under the key of the kernel the library names, with a valid,
    positive time from the right kind of events; the result within its gate as untimed"""
    lib, ops = _ops()
    assert G.case_route(c, n_cu()) == c["route"]
    bt = G.build(c, DEV)
    p = G.reference(c, bt)
    out = new_out(c, bt)
    timer = ops.LaunchTimer()
    ops.set_timer(timer)
    try:
        assert launch_product(c, bt, out, None, lib, ops) == 0
    finally:
        ops.set_timer(None)
    assert lib.pcaa_gemm_last_kernel() == G.kernel_id(c["route"])
    check(c["id"], out.take(), p["want"], p["gate"], c["route"])
    assert [r[0] for r in timer.records] == [key], (c["id"], [r[0] for r in timer.records])
    ev = timer.records[0][3]
    assert isinstance(ev, ops._KernelEvents if kernel_exact else ops._TorchEvents), (c["id"], type(ev))
    assert ev.valid() and ev.elapsed_ms() > 0.0, (c["id"], ev.valid())
    assert timer.summary()[key]["launches"] == 1


def child():
    """PCAA_GEMM_TICKETS=0, PCAA_GEMM_V2_RC=0 (both read once per process): the fixed-share walk a declined ticket slot
    falls back to, and the register-staged kernel under the whole-tile weight gradients; then the timed launches"""
    assert os.environ["PCAA_GEMM_TICKETS"] == "0" and os.environ["PCAA_GEMM_V2_RC"] == "0"
    for c in CASES:
        if c["id"] in CHILD_IDS:
            run_product(c, tickets=False, rc_on=False)
    for c, key, kernel_exact in TIMED:
        run_timed(c, key, kernel_exact)
    res = dict(WORST)
    print("CHILD_RESULT " + json.dumps(res))


def test_lab_switches_in_a_child_process():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""), PCAA_GEMM_TICKETS="0", PCAA_GEMM_V2_RC="0")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], capture_output=True, text=True, timeout=300, cwd=root,
                         env=env)
    print(res.stdout[-4000:])
    assert res.returncode == 0, res.stderr[-4000:]
    line = [l for l in res.stdout.splitlines() if l.startswith("CHILD_RESULT ")][-1]
    worst = json.loads(line[len("CHILD_RESULT "):])
    assert any(r.startswith("v2/plain/whole/one_tile_each") for r in worst), worst       # the over-CU-count cases, without the draw
    assert any(r.startswith("bf16_staged/bf16,bf16,f32,RC,RC") for r in worst), worst
    assert all(v <= 1.0 for v in worst.values()), worst


if __name__ == "__main__":
    if sys.argv[1:] == ["child"]:
        child()
