#!/usr/bin/env python3
"""The HBM-bound passes of the PointNet block alone on the GPU: ms and TB/s of the bytes each moves, at the bench
shape.  python tools/elementwise_lab.py        (profiles/r03_elementwise_unroll_lab.txt is this lab on a scratch build
whose column-invariant kernels took 1 / 2 / 4 / 8 quads per thread and trip; the switch was not kept)
python tools/elementwise_lab.py --routes    the passes with a streaming kernel, both routes alternating, 9 rounds
(profiles/ew_stream.txt)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from opensetgaitrecognition_pcaa_amd import ops
P, dev = 245760, "cuda"


def timed(fn, reps=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def routes_ab(rounds=9):
    """the passes that have a streaming kernel (csrc/ew_stream.h), stream and classic alternating on this box"""
    from opensetgaitrecognition_pcaa_amd import _lib
    lib = _lib.load()

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    print(f"# {rounds} rounds, stream and classic alternating; us: median (min-max); a pass ships on the stream route only")
    print("# if its median beats the classic median by more than the classic route's own min-max spread")
    for ch in (512, 1024):
        y = (torch.randn(P, ch, device=dev) * 0.7).bfloat16()
        sc = torch.rand(ch, device=dev) + 0.5
        sh = torch.randn(ch, device=dev) * 0.1
        coef = torch.randn(3, ch, device=dev) * 0.3
        coef[0] = 0.5                                            # the in-place iteration stays bounded
        dz = (torch.randn(P, ch, device=dev) * 0.1).bfloat16()
        out = torch.empty_like(y)
        nb = P * ch * 2
        passes = [("bn_act_fwd", 2, lambda: ops.bn_act_fwd(y, sc, sh)),
                  ("bn_bwd_dy (out of place)", 3, lambda: ops.bn_bwd_dy(dz, y, coef, out=out)),
                  ("bn_bwd_dy (in place)", 3, lambda: ops.bn_bwd_dy(dz, y, coef, out=dz))]
        for name, nt, fn in passes:
            ts = {0: [], 1: []}
            for on in (1, 0):
                lib.pcaa_ew_stream_set(on); fn(); fn()
            torch.cuda.synchronize()
            for _ in range(rounds):
                for on in (1, 0):
                    lib.pcaa_ew_stream_set(on)
                    ts[on].append(once(fn))
            lib.pcaa_ew_stream_set(1)
            st = {on: (sorted(v)[len(v) // 2], min(v), max(v)) for on, v in ts.items()}
            wins = st[0][0] - st[1][0] > st[0][2] - st[0][1]
            print(f"[{ch}] {name:26s} stream {st[1][0]:7.1f} ({st[1][1]:6.1f}-{st[1][2]:6.1f}) {nt * nb / st[1][0] / 1e6:5.2f} TB/s | "
                  f"classic {st[0][0]:7.1f} ({st[0][1]:6.1f}-{st[0][2]:6.1f}) {nt * nb / st[0][0] / 1e6:5.2f} TB/s | "
                  f"{'stream wins' if wins else 'inside the spread: stays classic'}")


if "--routes" in sys.argv:
    routes_ab()
    sys.exit(0)

for ch in (512, 1024):
    y = (torch.randn(P, ch, device=dev) * 0.7).bfloat16()
    sc = torch.rand(ch, device=dev) + 0.5
    sh = torch.randn(ch, device=dev) * 0.1
    mu = torch.randn(ch, device=dev) * 0.1
    rs = torch.rand(ch, device=dev) + 0.5
    nb = P * ch * 2
    t = timed(lambda: ops.bn_act_fwd(y, sc, sh))
    print(f"[{ch}] bn_act_fwd            {t:.3f} ms  {2 * nb / t / 1e9:.2f} TB/s (read + write)")
    t = timed(lambda: ops.bn_act_meanpool_fwd(y, sc, sh, P // 128, 128, mu, rs))
    print(f"[{ch}] bn_act_meanpool (train) {t:.3f} ms  {nb / t / 1e9:.2f} TB/s (read)")
    coef = torch.randn(3, ch, device=dev) * 0.3
    dzt = (torch.randn(P, ch, device=dev) * 0.1).bfloat16()
    outt = torch.empty_like(y)
    t = timed(lambda: ops.bn_bwd_dy(dzt, y, coef, out=outt))
    print(f"[{ch}] bn_bwd_dy             {t:.3f} ms  {3 * nb / t / 1e9:.2f} TB/s (2 reads + write)")
    t = timed(lambda: ops.bn_bwd_dy_fused(y, sc, sh, coef, da=dzt, out=outt))
    print(f"[{ch}] bn_bwd_dy_fused (da)  {t:.3f} ms  {3 * nb / t / 1e9:.2f} TB/s (2 reads + write)")
    dpool = torch.randn(P // 128, ch, device=dev) * 0.1
    t = timed(lambda: ops.bn_bwd_dy_fused(y, sc, sh, coef, dpool=dpool, group_rows=128, pool_scale=1 / 128, out=outt))
    print(f"[{ch}] bn_bwd_dy_fused (pool) {t:.3f} ms  {2 * nb / t / 1e9:.2f} TB/s (read + write)")
    del dzt, outt
    z = torch.empty_like(y)
    t = timed(lambda: z.copy_(y))
    print(f"[{ch}] torch copy            {t:.3f} ms  {2 * nb / t / 1e9:.2f} TB/s (read + write)")
    t = timed(lambda: y.sum(dim=0))
    print(f"[{ch}] torch column sum      {t:.3f} ms  {nb / t / 1e9:.2f} TB/s (read)")
x = torch.randn(P, 4, device=dev)
W = torch.randn(512, 4, device=dev) * 0.3
da = (torch.randn(P, 512, device=dev) * 0.1).bfloat16()
sc = torch.rand(512, device=dev) + 0.5; sh = torch.randn(512, device=dev) * 0.1
mu = torch.randn(512, device=dev) * 0.1; rs = torch.rand(512, device=dev) + 0.5
t = timed(lambda: ops.pointnet_in_bwd_stats(da, x, W, sc, sh, mu, rs))
print(f"pointnet_in_bwd_stats      {t:.3f} ms  {P * 512 * 2 / t / 1e9:.2f} TB/s (read)")
t = timed(lambda: ops.pointnet_in_apply(x, W, sc, sh, torch.bfloat16))
print(f"pointnet_in_apply          {t:.3f} ms  {P * 512 * 2 / t / 1e9:.2f} TB/s (write)")


class _Bn:
    weight = torch.rand(512, device=dev) + 0.5


def onepass():
    tail = ops.BnTailBwd(P, _Bn, mu, rs, 512)
    return ops.pointnet_in_bwd_onepass(da, x, W, sc, sh, mu, rs, tail, mom=mom)


mom = ops.points_moments(x)
t = timed(onepass)
print(f"pointnet_in_bwd_onepass    {t:.3f} ms  {P * 512 * 2 / t / 1e9:.2f} TB/s (read; + the small launches around it)")
