"""The eval-mode PointNet layers in fp8 (``functional.set_eval_pointnet("fp8")``) against the bf16 route, in one process.

    python tools/fp8_pointnet_bench.py [--legs 1,2,3,4,5,6,7] [--out profiles/fp8_pointnet.txt]

N = 128, C = 4, K = 8, bf16 mode.  Legs, each as a bf16 leg and an fp8 leg, alternated window by window:
  1  the three GEMM launches of PointNet layers 2-4 alone at 786 432 rows (6 144 frames x 128), the last with the mean over
     the frame's points: ops.gemm_affine_elu against ops.gemm_fp8_affine_elu on operands made once
  2  ``OpenSetScorer.embed_track``, 1 024 windows
  3  the same with ``dedup_points`` on a synthetic raw track of 3-40 detections per frame
  4  ``OpenSetScorer.embed`` on the 1 024 crops
  5  one ``MultiStreamScorer`` tick at S = 64 (launch-bound: no gain expected; recorded, not tuned against)
  6  no timing: ``naive_sequential_procedure_tensors`` on the synthetic procedure data of tests/golden/procedures.npz (its raw
     data set regenerated in a temporary folder, N = 16, the golden's encoder fill and centroids) in both kinds, k in 1, 2, 4, 6:
     agreement of the votes between the kinds.  N = 16 has no pooled epilogue, so the padded route ignores the kind (both
     runs launch the same kernels); with ``dedup_points`` the ragged route runs in fp8
  7  no timing: the accumulator error of ``pcaa_gemm_fp8_affine_elu`` against fp64 on exact e4m3 operands -- the measurement the
     in-instruction term of tests/fp8_ref.py (``C_IN``) is taken from.  One non-zero row per pooled group of 32 and shift 0,
     so 32 x the fp32 output is ELU(scale8 acc) of that row exactly; elements with z > 0 (there the epilogue rounds by
     3 u |z|, taken off); K = 128 / 512 / 1024; operands uniform of both signs, all products positive, and |a| spread over
     nine binades.  u = 2^-24, S = sum |a w|, pmax = the largest |a w| of an element inside one 64-wide step
WARMUP calls per leg, then WINDOWS windows of CALLS calls each between two HIP events; the median over the windows, per
call, and the spread ((max - min) / median).  Per scorer leg also: label agreement of the fp8 leg with the bf16 leg, the
largest ``sup_fv`` difference between them over the largest ``|sup_fv|``, and the distance of both legs' frame features
from the fp64 oracle (tests/fp8_ref.py ``emulate(quant=False)`` on the leg's first 64 frames, through
``encoder_frame_features``) over the features' maximum, and the share of the e4m3 activations of those frames (the outputs
of layers 1-3) that sit at the clamp (+-448): what the contract records in place of activation scales.  Synthetic encoder
and data: what a trained checkpoint on the real data set loses is NOT measured here.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fp8_ref  # noqa: E402
from crop_dedup_bench import distinct_data, raw_data  # noqa: E402
from multi_stream_bench import KVOTE, Bed, C, K, N, make_encoder  # noqa: E402
from opensetgaitrecognition_pcaa_amd import functional as F_hip, inference, ops  # noqa: E402

WARMUP, WINDOWS, CALLS = 3, 5, 20
ROWS = 6144 * 128
KINDS = ("bf16", "fp8")


def window_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def measure(legs, calls=CALLS):
    """{kind: callable} -> {kind: (median ms per call, spread)}; the kinds alternate window by window"""
    for kind, fn in legs.items():
        with F_hip.eval_pointnet(kind):
            for _ in range(WARMUP):
                fn()
    rec = {k: [] for k in legs}
    for _ in range(WINDOWS):
        for kind, fn in legs.items():
            with F_hip.eval_pointnet(kind):
                rec[kind].append(window_ms(fn, calls))
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for k, v in rec.items()}


def report(say, name, res, extra=""):
    (tb, sb), (t8, s8) = res["bf16"], res["fp8"]
    say(f"  leg [{name}] bf16 {tb:.3f} ms (spread {100 * sb:.1f} %)  fp8 {t8:.3f} ms (spread {100 * s8:.1f} %)  "
        f"bf16 / fp8 = {tb / t8:.2f}x{extra}")


def oracle_distance(enc, frames):
    """frame features of both kinds on ``frames`` [n, N, C] against the fp64 oracle, of the features' maximum, and the share
    of the fp8 kind's e4m3 activations at the clamp -> the report line"""
    frames = frames.contiguous()
    sd = {k: v for k, v in enc.state_dict().items()}
    want = fp8_ref.emulate(sd, frames.reshape(-1, frames.shape[2]), frames.shape[1], quant=False)
    out = {}
    for kind in KINDS:
        with torch.no_grad(), F_hip.eval_pointnet(kind):
            got, saves = F_hip.encoder_frame_features(enc, frames)
        out[kind] = float((got.double() - want).abs().max() / want.abs().max())
    acts = [s.a_in.view(torch.uint8) for s in saves[1:]]
    assert all(s.a_in.dtype == ops.FP8 for s in saves[1:]), "the fp8 route must be the one that ran"
    clamp = sum(int(((a & 0x7F) == 0x7E).sum()) for a in acts) / sum(a.numel() for a in acts)
    return (f"  frame features from the fp64 oracle, of their maximum: bf16 {out['bf16']:.2e}, fp8 {out['fp8']:.2e}; e4m3 "
            f"activations at the clamp: {100 * clamp:.4f} %")


def agreement(run):
    """run(kind) -> (preds, sup_fv, lik): label agreement and the sup_fv difference of scale between the kinds"""
    res = {}
    for kind in KINDS:
        with F_hip.eval_pointnet(kind):
            res[kind] = run()
    (pb, fb, _), (p8, f8, _) = res["bf16"], res["fp8"]
    return (f"  labels equal {int((pb == p8).sum())} / {pb.numel()}, max |sup_fv(fp8) - sup_fv(bf16)| / max |sup_fv| = "
            f"{float((f8.double() - fb.double()).abs().max() / fb.double().abs().max()):.2e}")


def leg1(say):
    gen = torch.Generator(device="cuda").manual_seed(3)
    shapes = ((512, 512, 0), (1024, 512, 0), (1024, 1024, 128))
    a0 = torch.randn((ROWS, 512), device="cuda", generator=gen).clamp(-1.0, 8.0)
    w = [torch.randn((n, k), device="cuda", generator=gen) * (1.5 / k ** 0.5) for n, k, _ in shapes]
    sc = [torch.rand(n, device="cuda", generator=gen) * 0.6 + 0.7 for n, _, _ in shapes]
    sh = [torch.rand(n, device="cuda", generator=gen) - 0.5 for n, _, _ in shapes]
    w16 = [ops.cast_bf16(x, True, False)[0] for x in w]
    w8 = [ops.quantize_weight_fp8(x) for x in w]
    sc8 = [s * q[1] for s, q in zip(sc, w8)]
    a16 = a0.bfloat16()
    a8 = torch.empty((ROWS, 512), dtype=torch.uint8, device="cuda")
    for r0 in range(0, ROWS, 65536):                      # (the e4m3 image of the first operand: torch's cast on the host)
        a8[r0:r0 + 65536] = fp8_ref.q8(a0[r0:r0 + 65536])
    a8 = a8.view(ops.FP8)
    del a0
    keep = {}

    def run16():
        a = a16
        for i, (_, _, pool) in enumerate(shapes):
            a = ops.gemm_affine_elu(a, w16[i], sc[i], sh[i], pool)
        keep["bf16"] = a

    def run8():
        a = a8
        for i, (_, _, pool) in enumerate(shapes):
            a = ops.gemm_fp8_affine_elu(a, w8[i][0], sc8[i], sh[i], pool)
            if i == 1:
                keep["a3"] = a
        keep["fp8"] = a
    res = measure({"bf16": run16, "fp8": run8})
    flop = sum(2.0 * ROWS * n * k for n, k, _ in shapes)
    clamp = float(((keep["a3"].view(torch.uint8) & 0x7F) == 0x7E).float().mean())
    d = float((keep["fp8"] - keep["bf16"]).abs().max() / keep["bf16"].abs().max())
    report(say, f"three GEMM launches, {ROWS} rows", res,
           f"  ({flop / res['bf16'][0] * 1e-9:.0f} / {flop / res['fp8'][0] * 1e-9:.0f} TFLOP/s; {res['fp8'][0] * 1e6 / ROWS:.2f} ns per row)")
    say(f"  pooled outputs differ by {d:.2e} of their maximum; layer-3 activations (of random operands) at the clamp: {100 * clamp:.4f} %")
    for i, (n, k, pool) in enumerate(shapes):               # the three launches one by one
        x16 = torch.randn((ROWS, k), device="cuda", generator=gen).bfloat16()
        x8 = torch.randint(0, 0x70, (ROWS, k), dtype=torch.uint8, device="cuda", generator=gen).view(ops.FP8)
        r = measure({"bf16": lambda: ops.gemm_affine_elu(x16, w16[i], sc[i], sh[i], pool),
                     "fp8": lambda: ops.gemm_fp8_affine_elu(x8, w8[i][0], sc8[i], sh[i], pool)})
        f = 2.0 * ROWS * n * k
        report(say, f"layer {i + 2}: {k} -> {n}" + (f", mean over {pool}" if pool else ""), r,
               f"  ({f / r['bf16'][0] * 1e-9:.0f} / {f / r['fp8'][0] * 1e-9:.0f} TFLOP/s)")


def leg5_agreement(enc, means, bed):
    """the windows of one tick of two fresh MultiStreamScorers, one per kind, fed the bed's tracks"""
    res = {}
    S, hop, warm = bed.S, bed.hop, bed.warm
    for kind in KINDS:
        with F_hip.eval_pointnet(kind):
            ms = inference.MultiStreamScorer(enc, means, 0.0, KVOTE, K, max_streams=S)
            sids = [ms.open() for _ in range(S)]
            for a in range(0, warm, 32):
                b = min(a + 32, warm)
                ms.push(sids, [b - a] * S, torch.cat([t[a:b] for t in bed.tracks]))
            tick = ms.push(sids, [hop] * S, bed.ticks_b[0])
            res[kind] = (tick.preds, tick.sup_fv, tick.lik)
    (pb, fb, _), (p8, f8, _) = res["bf16"], res["fp8"]
    return (f"  labels equal {int((pb == p8).sum())} / {pb.numel()}, max |sup_fv(fp8) - sup_fv(bf16)| / max |sup_fv| = "
            f"{float((f8.double() - fb.double()).abs().max() / fb.double().abs().max()):.2e}")


def leg7(say):
    import gemm_ref as G
    U, Nc, groups = 2.0 ** -24, 256, 512
    say("  accumulator error of pcaa_gemm_fp8_affine_elu against fp64 (leg 7); 'fp32 model': against tests/gemm_ref.py's "
        f"accumulator gate alone; 'gate': against the gate of tests/fp8_ref.py (that model plus C_IN = {fp8_ref.C_IN:g} times the last column's unit)")
    for Kc in (128, 512, 1024):
        for kind in ("both signs", "positive", "spread"):
            xa = G.logical(groups, Kc, 7 + Kc, "cuda")
            xw = G.logical(Nc, Kc, 8 + Kc, "cuda", (3.0 / Kc) ** 0.5).float()
            if kind == "positive":
                xa, xw = xa.abs(), xw.abs()
            if kind == "spread":
                xa = xa * torch.exp2(torch.floor(G.uniform(groups * Kc, 9, "cuda", -6.0, 3.0)).view(groups, Kc))
            W8, s = fp8_ref.weight_rule(xw)
            a8 = torch.zeros((32 * groups, Kc), dtype=torch.uint8, device="cuda")
            a8[::32] = fp8_ref.q8(xa)
            scale8 = (torch.ones(Nc, device="cuda") * s).contiguous()
            out = ops.gemm_fp8_affine_elu(a8.view(ops.FP8), W8.view(ops.FP8), scale8, torch.zeros(Nc, device="cuda"), 32)
            a, w = fp8_ref.dq(a8[::32]), fp8_ref.dq(W8)
            r = G.acc_ref(a, w, True)
            unit = fp8_ref.instr_gate(a, w) / fp8_ref.C_IN              # u sqrt(sum_steps pmax^2)
            sc = scale8.double().expand_as(r["acc"])
            z = r["acc"] * sc
            pos = z > 0
            err = ((out.double() * 32 - z) / sc)[pos]                   # in accumulator units
            mag = (err.abs() - 3 * U * r["acc"][pos].abs()).clamp_min(0)
            S = r["S"][pos]
            say(f"    K={Kc:4d} {kind:10s} n={err.numel():6d}  |err|/(u S): max {float((mag / (U * S)).max()):7.2f} mean "
                f"{float((mag / (U * S)).mean()):6.2f}, signed mean {float((err / (U * S)).mean()):+7.2f};  fp32 model: max "
                f"{float((mag / G.acc_gate(r)[pos]).max()):6.2f};  gate: max {float((mag / (G.acc_gate(r) + fp8_ref.C_IN * unit)[pos]).max()):5.3f};  "
                f"|err|/(u sqrt(sum pmax^2)): max {float((mag / unit[pos]).max()):7.1f} p99.9 {float((mag / unit[pos]).quantile(0.999)):7.1f}")


def leg6(say):
    import json
    import pickle
    import tempfile

    import numpy as np

    from opensetgaitrecognition_pcaa_amd import constants, datasets, models, synthetic as syn
    g = np.load(os.path.join(ROOT, "tests", "golden", "procedures.npz"), allow_pickle=False)
    meta = json.loads(str(g["meta"]))
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        data, gen = os.path.join(tmp, "raw"), os.path.join(tmp, "gen")
        for subj in range(10):
            for si, scen in enumerate(("free_walk", "hands_in_pockets", "smartphone")):
                d = os.path.join(data, f"target{subj}", scen)
                os.makedirs(d, exist_ok=True)
                for t in range(10):
                    with open(os.path.join(d, f"pc_tr{t}{si}.obj"), "wb") as f:
                        pickle.dump(syn.synthetic_raw_track(1000 + subj * 100 + si * 10 + t, 38 + ((subj + t) % 3) * 6), f)
        os.chdir(tmp)
        try:
            constants.DATA_PATH, constants.GEN_DATA_PATH, constants.NFEATURES = data, gen, 4
            np.random.seed(meta["np_seed_splits"])
            datasets.generate_splits(train_classes=meta["train_classes"], seed=0, nmax_points=meta["nmax"], verbose=False)
            known = inference._sequential_split_on_device(constants.SPLIT.TEST, constants.TRAIN_SCENARIOS, "cuda")
            unseen = inference._sequential_split_on_device(constants.SPLIT.UNSEEN, constants.TRAIN_SCENARIOS, "cuda")
        finally:
            os.chdir(cwd)
    enc = models.CGEncoder(len(meta["train_classes"]), nmax_points=meta["nmax"], use_projection_head=True).float()
    syn.deterministic_fill_(enc, meta["enc_fill_seed"])
    enc = enc.cuda().eval()
    means = torch.from_numpy(g["infer.means"]).cuda()
    say(f"  procedures.npz (N = {meta['nmax']}, {known[0].shape[0]} known and {unseen[0].shape[0]} unseen crops), votes of the fp8 kind "
        "against the bf16 kind:")
    for dedup in (False, True):
        for k in (1, 2, 4, 6):
            res = {}
            for kind in KINDS:
                with F_hip.eval_pointnet(kind):
                    res[kind] = inference.naive_sequential_procedure_tensors(k, enc, means, known[0], known[1], unseen[0], unseen[1],
                                                                             seed=0, unseen_valid_ratio=0.2, dedup_points=dedup)
            (pb, lb, tb), (p8, l8, t8) = res["bf16"], res["fp8"]
            same = float((np.asarray(pb) == np.asarray(p8)).mean()) if np.shape(pb) == np.shape(p8) else float("nan")
            acc = [float((np.asarray(p) == np.asarray(l)).mean()) for p, l in ((pb, lb), (p8, l8))]
            say(f"    dedup_points={int(dedup)} k={k}: votes equal {same:.4f} of {np.size(pb)}; accuracy bf16 {acc[0]:.4f} fp8 {acc[1]:.4f}; "
                f"threshold bf16 {float(tb):.4e} fp8 {float(t8):.4e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="1,2,3,4,5,6,7")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    legs = {int(x) for x in args.legs.split(",")}
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    F_hip.set_precision("bf16")
    enc, means = make_encoder()
    sc = inference.OpenSetScorer(enc, means)
    say(f"fp8_pointnet_bench: N={N} C={C} K={K}, bf16 mode, {torch.cuda.get_device_name(0)}; {WARMUP} warm-up calls, then the "
        f"median of {WINDOWS} windows of {CALLS} calls between HIP events, bf16 and fp8 legs alternated; spread = (max - min) "
        "/ median.  Synthetic encoder and data; trained models on the real data set: not measured.")
    if 1 in legs:
        leg1(say)
    if legs & {2, 4}:
        _, track, crops, _ = distinct_data()
        if 2 in legs:
            report(say, "embed_track, 1024 windows", measure({k: (lambda: sc.embed_track(track)) for k in KINDS}))
            say(agreement(lambda: sc.embed_track(track)))
            say(oracle_distance(enc, track[:64]))
        if 4 in legs:
            report(say, "embed, 1024 crops", measure({k: (lambda: sc.embed(crops)) for k in KINDS}, calls=5))
            say(agreement(lambda: sc.embed(crops)))
            say(oracle_distance(enc, F_hip._point_major(crops).view(-1, N, C)[:64]))
        del track, crops
    if 3 in legs:
        _, track, _, share = raw_data(40)
        report(say, f"embed_track dedup_points, 1024 windows, 3-40 detections per frame (duplicate share {100 * share:.0f} %)",
               measure({k: (lambda: sc.embed_track(track, dedup_points=True)) for k in KINDS}))
        say(agreement(lambda: sc.embed_track(track, dedup_points=True)))
        say(oracle_distance(enc, track[:64]))
        del track
    if 5 in legs:
        bed = Bed(enc, means, 64, 3 + (WARMUP + WINDOWS * CALLS) * 2 + 4)
        res = measure({k: bed.tick_b for k in KINDS})
        report(say, "MultiStreamScorer tick, S = 64", res)
        say(leg5_agreement(enc, means, bed))
        say(oracle_distance(enc, bed.ticks_b[0][:64]))
    if 6 in legs:
        leg6(say)
    if 7 in legs:
        leg7(say)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
