"""The streaming route of the element-wise passes (csrc/ew_stream.h) against the classic grid-stride route, on the same
inputs, by the library's own switch (pcaa_ew_stream_set): every element the ported passes write -- ``a`` of bn_act_fwd,
``dy`` of bn_bwd_dy out of place and in place over dz -- must be BITWISE equal, and is also held to fp64 by the gates the
classic route is held to (tests/elementwise_ref.py, tests/test_elementwise_branches.py).  The ported passes reduce
nothing, so there is no statistic to compare.

Shapes: with r = 256 / (ch / 8) rows per trip, R the pass's ring depth and G its persistent grid (workgroups per CU x
CUs, both asked from the library / the device):

    rows in {1, r-1, r, r+1, R r - 1, R r, R r + 1, 3 R r + 5}   fewer trips than the grid has workgroups: the grid shrinks
                                                                 to one workgroup per trip and only the predicated tail runs
    G R r, G R r + 1                                             every workgroup runs the main loop exactly once; the second
                                                                 with a partial trip behind it
    2 G R r + G r + 3                                            two batches, then a tail with one whole stage and a partial one
    G (R-1) r + 5                                                the full grid, but no whole batch: tail only
    ch in {8 (the smallest the route takes), 512, 1024} for bn_bwd_dy; {1024, 2048} for bn_act_fwd, which streams from
    1024 channels on

The inputs sit at the front of a larger allocation whose rest is NaN-pattern garbage (0xffff): the clamped loads of rows
past the end may read rows below the end, never beyond it, and what they return must not reach any output; the outputs
sit in front of a guard region that must come back untouched."""
import pytest
import torch

import elementwise_ref as R
from opensetgaitrecognition_pcaa_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
ACT_FWD, BWD_DY = 0, 1                        # PCAA_EW_ACT_FWD, PCAA_EW_BWD_DY
PCAA_BF16 = 1
GUARD = 4096                                  # elements of garbage / guard behind every tensor
CASES = ["1", "r-1", "r", "r+1", "Rr-1", "Rr", "Rr+1", "3Rr+5", "GRr", "GRr+1", "2GRr+Gr+3", "G(R-1)r+5"]


def rows_of(case, kind, ch):
    lib = _lib.load()
    r = 256 // (ch // 8)
    Rd = lib.pcaa_ew_ring_depth(kind)
    G = lib.pcaa_ew_wgs_per_cu(kind) * torch.cuda.get_device_properties(0).multi_processor_count
    assert Rd >= 1 and G >= 1
    return {"1": 1, "r-1": r - 1, "r": r, "r+1": r + 1, "Rr-1": Rd * r - 1, "Rr": Rd * r, "Rr+1": Rd * r + 1,
            "3Rr+5": 3 * Rd * r + 5, "GRr": G * Rd * r, "GRr+1": G * Rd * r + 1, "2GRr+Gr+3": 2 * G * Rd * r + G * r + 3,
            "G(R-1)r+5": G * (Rd - 1) * r + 5}[case]


def fenced(t):
    """a copy of t at the front of an allocation whose remaining GUARD elements are 0xffff (a bf16 NaN)"""
    buf = torch.full((t.numel() + GUARD,), -1, dtype=torch.int16, device=DEV).view(BF16)
    view = buf[:t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def fence_intact(buf, n):
    return bool((buf[n:].view(torch.int16) == -1).all())


class Route:
    """run with the streaming route switched on or off; the previous setting comes back"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.was = _lib.load().pcaa_ew_stream_set(self.on)

    def __exit__(self, *exc):
        _lib.load().pcaa_ew_stream_set(self.was)


def bits(t):
    return t.contiguous().view(torch.int16)


def held_to_fp64(name, got, want, gate):
    r = R.ratio(got, want, gate)
    print(f"[ew_stream] {name}: worst |err| / gate = {r:.3f}")
    assert r <= 1.0, (name, r)


@pytest.mark.parametrize("ch", [1024, 2048])       # bn_act_fwd streams from 1024 channels on: the smallest, and r = 1
@pytest.mark.parametrize("case", CASES)
def test_bn_act_fwd_stream_equals_classic(case, ch):
    rows = max(1, rows_of(case, ACT_FWD, ch))                   # r - 1 = 0 at ch = 2048: one row again
    lib = _lib.load()
    seed = R.seed_of(ch, rows)
    sc, sh, _, _ = R.bn_vectors(ch, seed, DEV)
    ybuf, y = fenced(R.activations(rows, ch, BF16, seed, DEV))
    n = rows * ch
    with Route(1):
        assert lib.pcaa_ew_route(ACT_FWD, PCAA_BF16, rows, ch, 1) == b"stream"
        abuf, a = fenced(torch.zeros(rows, ch, dtype=BF16, device=DEV))
        check_call = lib.pcaa_bn_act_fwd(y.data_ptr(), a.data_ptr(), PCAA_BF16, sc.data_ptr(), sh.data_ptr(), rows, ch,
                                         torch.cuda.current_stream().cuda_stream)
        assert check_call == 0, lib.pcaa_last_error()
        torch.cuda.synchronize()
        assert fence_intact(abuf, n), "the stream route wrote behind the end of a"
        assert fence_intact(ybuf, n)
    with Route(0):
        assert lib.pcaa_ew_route(ACT_FWD, PCAA_BF16, rows, ch, 1) == b"classic"
        classic = ops.bn_act_fwd(y, sc, sh)
    assert torch.equal(bits(a), bits(classic)), f"bn_act_fwd rows={rows} ch={ch}: stream and classic differ bitwise"
    assert not torch.isnan(a).any()
    want, gate = R.bn_act_fwd_ref(y, sc, sh)
    held_to_fp64(f"bn_act_fwd stream rows={rows} ch={ch}", a, want, R.out_gate(gate, want, BF16))


@pytest.mark.parametrize("ch", [8, 512, 1024])
@pytest.mark.parametrize("case", CASES)
def test_bn_bwd_dy_stream_equals_classic_in_place_and_out_of_place(case, ch):
    rows = rows_of(case, BWD_DY, ch)
    assert rows >= 1
    lib = _lib.load()
    seed = R.seed_of(ch, rows)
    coef = R.coef_vectors(ch, seed, DEV)
    ybuf, y = fenced(R.activations(rows, ch, BF16, seed, DEV))
    dz0 = R.gradient(rows, ch, BF16, seed, DEV)
    n = rows * ch
    with Route(0):
        classic = ops.bn_bwd_dy(dz0, y, coef)
        classic_in_place = dz0.clone()
        ops.bn_bwd_dy(classic_in_place, y, coef, out=classic_in_place)
    assert torch.equal(bits(classic), bits(classic_in_place))
    with Route(1):
        assert lib.pcaa_ew_route(BWD_DY, PCAA_BF16, rows, ch, 1) == b"stream"
        dzbuf, dz = fenced(dz0)
        outbuf, out = fenced(torch.zeros(rows, ch, dtype=BF16, device=DEV))
        ops.bn_bwd_dy(dz, y, coef, out=out)                     # out of place
        torch.cuda.synchronize()
        assert fence_intact(outbuf, n), "the stream route wrote behind the end of dy"
        assert torch.equal(bits(dz), bits(dz0)), "the out-of-place call changed dz"
        ops.bn_bwd_dy(dz, y, coef, out=dz)                      # in place over dz, as functional._bn_dy calls it
        torch.cuda.synchronize()
        assert fence_intact(dzbuf, n), "the in-place stream route wrote behind the end of dz"
        assert fence_intact(ybuf, n)
    assert torch.equal(bits(out), bits(classic)), f"bn_bwd_dy rows={rows} ch={ch}: stream and classic differ bitwise"
    assert torch.equal(bits(dz), bits(classic)), f"bn_bwd_dy in place rows={rows} ch={ch}: stream and classic differ bitwise"
    assert not torch.isnan(out).any()
    want, gate = R.bn_bwd_dy_ref(dz0, y, coef)
    held_to_fp64(f"bn_bwd_dy stream rows={rows} ch={ch}", out, want, R.out_gate(gate, want, BF16))


def test_a_tensor_that_is_not_16_byte_aligned_takes_the_classic_kernel_and_still_agrees():
    rows, ch = 37, 512
    seed = R.seed_of(ch, rows)
    sc, sh, _, _ = R.bn_vectors(ch, seed, DEV)
    y0 = R.activations(rows, ch, BF16, seed, DEV)
    buf = torch.zeros(rows * ch + 8, dtype=BF16, device=DEV)
    y = buf[4:4 + rows * ch].view(rows, ch)                     # 8 bytes off a 16-byte boundary
    y.copy_(y0)
    assert y.data_ptr() % 16 == 8
    with Route(1):
        a = ops.bn_act_fwd(y, sc, sh)
        b = ops.bn_act_fwd(y0, sc, sh)
    assert torch.equal(bits(a), bits(b))
