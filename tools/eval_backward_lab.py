#!/usr/bin/env python3
"""What the eval-mode backward costs on the GPU (reported, not gated; profiles/eval_backward.txt is this tool's output).

1. CGEncoder forward + backward at B=64, N=128, C=4 in eval mode (frozen BatchNorm: functional.encoder_forward(...,
   want_bwd=True) + encoder_backward) and in train mode, in fp32 and bf16.
2. The one-pass kernel alone (pcaa_bn_eval_act_bwd) at [245 760, 1024] bf16 beside the two train-mode passes it replaces
   (the statistics pass pcaa_bn_act_bwd_dz(dz=NULL) + pcaa_bn_bwd_dy_fused), in the da form and in the pooled form, with
   the bytes each moves (computed from the shapes) and the fraction of the 8.0 TB/s HBM peak.

HIP events around each window; every configuration is warmed up, then timed in several windows whose configurations
alternate, so a drift of the shared machine lands on all of them; the median and the min-max spread are printed.

    python tools/eval_backward_lab.py [--windows 5] [--iters 20]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from opensetgaitrecognition_pcaa_amd import constants, functional as F_hip, models, ops, synthetic as syn

DEV = "cuda"
HBM_PEAK = 8.0e12          # bytes/s, MI355X HBM3E specification


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(fns, windows, iters):
    """{name: fn} -> {name: sorted per-call ms of each window}; windows of the configurations alternate"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            out[k].append(window(fn, iters))
    return {k: sorted(v) for k, v in out.items()}


def show(name, ts, nbytes=None):
    med = ts[len(ts) // 2]
    line = f"{name:58s} {med:8.3f} ms  (min {ts[0]:.3f}, max {ts[-1]:.3f}, {len(ts)} windows)"
    if nbytes is not None:
        rate = nbytes / (med * 1e-3)
        line += f"  {nbytes / 1e9:6.3f} GB  {rate / 1e12:5.2f} TB/s = {rate / HBM_PEAK:5.1%} of HBM peak"
    print(line, flush=True)
    return med


def encoder_part(windows, iters):
    B, N, C, K, T = 64, 128, 4, 8, constants.NSTEPS
    constants.NFEATURES = C
    enc = models.CGEncoder(K, nmax_points=N, use_projection_head=True).float()
    syn.deterministic_fill_(enc, 0)
    enc = enc.to(DEV)
    x = syn.synthetic_pcs(B, T, N, C, seed=1234).to(DEV).permute(0, 3, 1, 2)
    d1 = torch.randn(B, K, device=DEV)
    d2 = torch.randn(B, 32, device=DEV)
    buffers = {k: v.clone() for k, v in enc.named_buffers()}          # the train-mode runs move the running statistics

    def run(training, mode):
        def fn():
            with torch.no_grad():
                _, _, st = F_hip.encoder_forward(enc, x, training, mode, want_bwd=True)
                F_hip.encoder_backward(enc, st, d1, d2)
        return fn

    print(f"CGEncoder forward + backward, B={B} N={N} C={C} T={T} ({B * T * N} points), per call")
    fns = {f"{'train' if tr else 'eval '} {mode}": run(tr, mode) for mode in ("fp32", "bf16") for tr in (False, True)}
    res = measure(fns, windows, iters)
    med = {k: show("  encoder fwd + bwd, " + k, v) for k, v in res.items()}
    for mode in ("fp32", "bf16"):
        print(f"  {mode}: eval / train = {med['eval  ' + mode] / med['train ' + mode]:.3f}")
    with torch.no_grad():
        for k, v in enc.named_buffers():
            v.copy_(buffers[k])


def kernel_part(windows, iters):
    P, ch, G = 245760, 1024, 128
    y = (torch.randn(P, ch, device=DEV) * 0.7).bfloat16()
    da = (torch.randn(P, ch, device=DEV) * 0.1).bfloat16()
    dpool = torch.randn(P // G, ch, device=DEV) * 0.1
    out = torch.empty_like(y)
    sc, sh = torch.rand(ch, device=DEV) + 0.5, torch.randn(ch, device=DEV) * 0.1
    mu, rs = torch.randn(ch, device=DEV) * 0.1, torch.rand(ch, device=DEV) + 0.5
    coef = torch.randn(3, ch, device=DEV) * 0.3
    nb = P * ch * 2          # bytes of one [P, ch] bf16 tensor
    pool = dict(dpool=dpool, group_rows=G, pool_scale=1.0 / G)
    print(f"\nthe BatchNorm + ELU backward of one layer alone, [{P}, {ch}] bf16 (one tensor = {nb / 1e9:.3f} GB)")
    fns = {
        "eval  one pass, da form (reads da, y; writes dy)": lambda: ops.bn_eval_act_bwd(y, sc, sh, mu, rs, da=da, out=out),
        "train pass 1: statistics, da form (reads da, y)": lambda: ops.bn_act_bwd_stats(y, sc, sh, mu, rs, da=da),
        "train pass 2: bn_bwd_dy_fused, da form (reads da, y; writes dy)": lambda: ops.bn_bwd_dy_fused(y, sc, sh, coef, da=da, out=out),
        "eval  one pass, pooled form (reads y; writes dy)": lambda: ops.bn_eval_act_bwd(y, sc, sh, mu, rs, out=out, **pool),
        "train pass 1: statistics, pooled form (reads y)": lambda: ops.bn_act_bwd_stats(y, sc, sh, mu, rs, **pool),
        "train pass 2: bn_bwd_dy_fused, pooled form (reads y; writes dy)": lambda: ops.bn_bwd_dy_fused(y, sc, sh, coef, out=out, **pool),
    }
    nbytes = dict(zip(fns, (3 * nb, 2 * nb, 3 * nb, 2 * nb, nb, 2 * nb)))
    res = measure(fns, windows, iters)
    med = {k: show("  " + k, v, nbytes[k]) for k, v in res.items()}
    keys = list(fns)
    for form, (e, p1, p2) in (("da form", keys[0:3]), ("pooled form", keys[3:6])):
        two = med[p1] + med[p2]
        print(f"  {form}: one eval pass {med[e]:.3f} ms against {two:.3f} ms for the two train-mode passes "
              f"({med[e] / two:.2f} x; bytes {nbytes[e] / 1e9:.2f} GB against {(nbytes[p1] + nbytes[p2]) / 1e9:.2f} GB)")
    print("  (the trainer's pooled layer takes its statistics from the forward's per-group sums instead of pass 1: "
          "ops.bn_pool_bwd_stats)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--part", choices=["all", "encoder", "kernel"], default="all")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_backward_lab: no GPU -- a time is only measured on one")
    print(f"device: {torch.cuda.get_device_name(0)}; windows {a.windows} x {a.iters} calls, configurations alternating")
    if a.part in ("all", "encoder"):
        encoder_part(a.windows, a.iters)
    if a.part in ("all", "kernel"):
        kernel_part(a.windows, a.iters)


if __name__ == "__main__":
    main()
