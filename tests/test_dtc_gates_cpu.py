"""The gates, the dispatch restatement and the case lists of tests/dtc_ref.py, checked on the CPU at the inputs the GPU
tests use (tests/test_dtc_branches.py takes its cases from the same lists; the largest case is 47 sequences of 4 steps,
so every case is evaluated whole).

* NOT TOO TIGHT: float32 torch evaluations of the kernels' formulation -- not the kernels -- stay within HALF of every
  gate, in several orders of summation: tap-major inside 32-channel chunks as one chain; the four waves' partial tiles
  (group gg = tap * 4 + channel / 8 of a chunk goes to wave gg / 3) combined as (p0 + p1) + (p2 + p3); the two k-halves of
  the 32-column pair kernel (wave gg / 6) combined; for the bf16 kernels the 16-deep MFMA steps summed exactly and rounded
  once, as one chain and as two halves; per K range for the slabs, then added in order.  The staged operand is evaluated as
  the kernels form it (fma, the polynomial / exp(z) - 1 ELU, (k0 dz + k1 y) + k2), the statistics in the kernels' row lanes
  and with the rows in order.  Evaluated once per distinct arithmetic (``sig``): the four kinds of windowed source stage
  the same values through different addresses, so one kind per shape is evaluated.
* NOT VACUOUS: every planted defect, at the case meant to catch it, moves at least 80 % of the elements it touches by more
  than 10 x the gate.
* INPUT CONDITIONS: every operand's |mean| is below 0.05 of its rms (or 3 / sqrt(n) of it, the sampling noise of n values); the share of staged elements whose bf16 rounding
  interval straddles a boundary (the size of the flip term) is printed.
* COVERAGE: every code pcaa_dtc_conv_route can return is the target of a forward and of an adjoint case, the library's
  answer equals the restatement and the case's own claim; every condition of pair_takes, wide and the ksplit functions is
  taken both ways (by the cases where a valid call can, by the predicate grid otherwise); every PCAA_CHECK_ARG message of
  csrc/dtc_fused.hip is the target of a refusal case; every defect has a case.
"""
import os
import re

import pytest
import torch

import dtc_ref as D
from dtc_ref import U

BF = torch.bfloat16
LISTS = {"fwd": D.fwd_cases(), "adj": D.adj_cases(), "win": D.window_cases()}


def fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def half_gate(name, got, want, gate, bound=0.5):
    r = D.ratio(got, want, gate)
    assert r <= bound, (name, r)
    return r


# ------------------------------------------------------------------------------------------------ fp32 evaluations
def elu_stage32(z):
    poly = z * (1 + z * (0.5 + z * (1 / 6 + z * (1 / 24 + z * (1 / 120 + z * (1 / 720))))))
    return torch.where(z > 0, z, torch.where(z > -0.25, poly, torch.exp(z) - 1))


def stage32(c, inp):
    if not c["adj"]:
        x = D.materialise(c, inp) if c.get("win") else inp["src"]
        return elu_stage32(fma(inp["scale"], x, inp["shift"])) if c["act"] else x
    if c["form"] == 0:
        return inp["dy"]
    k0, k1, k2 = inp["coef"].unbind(0)
    return (k0 * inp["dz"] + k1 * inp["y"]) + k2


def korder(kc, c0, c1):
    """the kernels' order of the contraction over channels [c0, c1): (column of X, fp32 group gg, bf16 step st, chunk)"""
    return [(tap * kc + ci, tap * 4 + (ci - ch0) // 8, tap * 2 + (ci - ch0) // 16, ch0)
            for ch0 in range(c0, c1, 32) for tap in range(3) for ci in range(ch0, min(ch0 + 32, c1))]


def chain(X, Wm, cols):
    acc = torch.zeros(X.shape[0], Wm.shape[0])
    for k in cols:
        acc = acc + X[:, k:k + 1] * Wm[:, k]
    return acc


def steps_exact(X, Wm, blocks):
    acc = torch.zeros(X.shape[0], Wm.shape[0])
    for blk in blocks:
        acc = (acc.double() + X[:, blk].double() @ Wm[:, blk].double().t()).float()
    return acc


def orders(X, Wm, kc, c0, c1, bf16):
    ko = korder(kc, c0, c1)
    if not ko:
        return {"empty": torch.zeros(X.shape[0], Wm.shape[0])}
    cols = [k for k, *_ in ko]
    if not bf16:
        w4 = [chain(X, Wm, [k for k, gg, _, _ in ko if gg // 3 == w]) for w in range(4)]
        w2 = [chain(X, Wm, [k for k, gg, _, _ in ko if gg // 6 == w]) for w in range(2)]
        return {"one chain": chain(X, Wm, cols), "four partial tiles": (w4[0] + w4[1]) + (w4[2] + w4[3]), "two k-halves": w2[0] + w2[1]}
    blocks = {}
    for k, _, st, ch0 in ko:
        blocks.setdefault((ch0, st), []).append(k)
    halves = [steps_exact(X, Wm, [b for (ch0, st), b in blocks.items() if st // 3 == w]) for w in range(2)]
    return {"one chain": chain(X, Wm, cols), "16-deep steps": steps_exact(X, Wm, list(blocks.values())), "two k-halves of steps": halves[0] + halves[1]}


def stats32(v1, v2, c, fam, bf16):
    """the two statistics' fp32 summands [B*T, ch] -> {order: [nrep, 2, ch] fp64}"""
    B, T, nrep = c["B"], c["T"], c["nrep"]
    pos, lanes = D.slice_positions(fam, bf16, T)
    seqs = 2 if fam == "pair32" else 1
    R = seqs * T
    out = {}
    for name, lists in (("row lanes", [[p for p in pos[l::lanes] if p >= 0] for l in range(lanes)]), ("rows in order", [list(range(R))])):
        tot = torch.zeros(nrep, 2, v1.shape[1], dtype=torch.float64)
        for s in range(D.cdiv(B, seqs)):
            rep = (s if fam != "pair64" else s // 2) % nrep
            for k, v in enumerate((v1, v2)):
                lane_sums = []
                for rows in lists:
                    a = torch.zeros(v.shape[1])
                    for r in rows:
                        if s * R + r < B * T:
                            a = a + v[s * R + r]
                    lane_sums.append(a)
                t = lane_sums[0]
                for x in lane_sums[1:]:
                    t = t + x
                tot[rep, k] += t.double()
        out[name] = tot
    return out


def eval32(c, inp, bf16, staged64=False, nudge=0):
    """-> {output: {order: fp32 / fp64 tensor}}; staged64: the bf16 operands rounded from the fp64 staged values; nudge = +-1:
    from the fp64 staged values moved to that edge of their own gate, a + nudge gate(a) -- a staged fp32 value may sit there,
    and wherever the interval straddles a bf16 boundary on that side the rounding flips"""
    T, kc, ks, adj = c["T"], c["kc"], c["ks"], c["adj"]
    fam = D.family(c, bf16)
    a = stage32(c, inp)
    W = inp["W"]
    a_op, W_op = (a.to(BF).float(), W.to(BF).float()) if bf16 else (a, W)
    if staged64:
        a_op = D.rb(D.stage(c, inp)[0]).float()
    if nudge:
        a64, ga = D.stage(c, inp)
        a_op = D.rb(a64 + nudge * ga).float()
    X = D.im2col(a_op.double(), T, c["d"], adj).float()
    Wm = D.wmat(W_op, c["cin"], c["cout"], adj).float()
    name = "out" if adj else "y"
    res = {}
    if ks == 1:
        res[name] = orders(X, Wm, kc, 0, kc, bf16)
    else:
        slabs = [orders(X, Wm, kc, k0, k1, bf16) for k0, k1 in D.split_ranges(kc, ks)]
        for z, s in enumerate(slabs):
            res[f"slab{z}"] = s
        first = [next(iter(s.values())) for s in slabs]
        total = first[0]
        for s in first[1:]:
            total = total + s
        res[name] = {"slabs added in order": total}
    if not adj:
        if c["col"]:
            res["col"] = {"staged": D.col_layout(D.im2col(a.double(), T, c["d"], False), kc).float()}
        if c["stats"]:
            res["stats"] = {}
            for o, v in res["y"].items():
                for so, t in stats32(v, v * v, c, fam, bf16).items():
                    res["stats"][f"{o}, {so}"] = t
        return res
    if c["form"] >= 2:
        res["dy_out"] = {"staged": a}
    if c["form"] == 3:
        z = fma(inp["ep_y"], inp["ep_scale"], inp["ep_shift"])
        e = torch.where(z > 0, torch.ones_like(z), torch.exp(z))
        yh = (inp["ep_y"] - inp["ep_mean"]) * inp["ep_rstd"]
        res["out"] = {o: v * e for o, v in res["out"].items()}
        res["stats"] = {}
        for o, v in res["out"].items():
            for so, t in stats32(v, v * yh, c, fam, bf16).items():
                res["stats"][f"{o}, {so}"] = t
    return res


def sig(which, c, bf16):
    return (which, bf16, c["B"], c["T"], c["cin"], c["cout"], c["d"], c["act"], c["form"], c["ks"], c["col"], c["nrep"])


def _distinct():
    seen, out = set(), []
    for which, cases in LISTS.items():
        for c in cases:
            for bf16 in (False, True):
                if sig(which, c, bf16) not in seen:
                    seen.add(sig(which, c, bf16))
                    out.append(pytest.param(which, c, bf16, id=f"{which}-{c['id']}-{'bf16' if bf16 else 'f32'}"))
    return out


@pytest.mark.parametrize("which,c,bf16", _distinct())
def test_fp32_evaluations_stay_within_half_of_every_gate(which, c, bf16):
    inp = D.inputs(c)
    # a flipped bf16 rounding of a staged element realises the whole of its term by itself: the evaluation that rounds the
    # reference's own fp64 staged values is held to half of the gates without that term, the one that rounds its fp32
    # staged values to the whole gates (the convention of the bf16 outputs in tests/test_gemm_gates_cpu.py)
    staged = bf16 and (c["act"] or c["form"] > 0)
    worst, no_flip = {}, {}
    for flip, bound in ((False, 0.5), (True, 1.0)) if staged else ((True, 0.5),):
        ref = D.reference(c, inp, bf16, flip=flip)
        ev = eval32(c, inp, bf16, staged64=staged and not flip)
        assert set(ev) | {k for k in ref if k.endswith("_sum")} == set(ref), (sorted(ev), sorted(ref))
        for name, by_order in ev.items():
            want, gate = ref[name]
            for o, got in by_order.items():
                r = half_gate(f"{c['id']} {name} ({o})", got, want, gate, bound)
                if name == "stats":
                    half_gate(f"{c['id']} stats summed ({o})", got.sum(0), *ref["stats_sum"], bound)
                if bound == 0.5:
                    worst[name] = max(worst.get(name, 0.0), r)
                    no_flip[name] = gate
                elif bool((gate == no_flip[name]).any()):       # the elements no flip can reach keep the half rule
                    m = gate == no_flip[name]
                    half_gate(f"{c['id']} {name} ({o}), elements without a flip term", got[m], want[m], gate[m], 0.5)
    top = max(worst.values())
    print(f"[dtc gate cpu] {which} {c['id']} {'bf16' if bf16 else 'f32'}: worst fp32-evaluation |err| / gate = "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items() if not k.startswith("slab") or v == top))
    assert top <= 0.5


FLIP_CASES = [("adj", "t32_w36/formed+dy_out+epilogue"), ("adj", "wg2"), ("fwd", "t32_w36"), ("fwd", "pair32_odd_quads")]


@pytest.mark.parametrize("which,cid", FLIP_CASES)
def test_a_realised_flip_fits_the_gates_and_exceeds_the_issues_form_of_the_statistics_gate(which, cid):
    """The bf16 operands rounded from a +- gate(a): every staged element whose interval straddles a bf16 boundary on that side
    flips.  The outputs and the statistics must stay within the WHOLE gate (a flip is its term); the statistics gate in the
    issue's starting form, with the operands' term inside min(., C_STAT u sqrt(.)), is exceeded -- the measurement, against
    the fp64 reference and without any kernel, that dtc_ref's docstring quotes for the CHANGED form."""
    c = D.case_of(which, cid)
    inp = D.inputs(c)
    ref, old = D.reference(c, inp, True), D.reference(c, inp, True, own_in_min=True)
    name = "out" if c["adj"] else "y"
    new_worst, old_worst, flips = {}, 0.0, 0
    a, ga = D.stage(c, inp)
    for nudge in (1, -1):
        flips += int((D.rb(a + nudge * ga) != D.rb(a)).sum())
        ev = eval32(c, inp, True, nudge=nudge)
        for k in (name, "stats"):
            for o, got in ev[k].items():
                new_worst[k] = max(new_worst.get(k, 0.0), half_gate(f"{cid} {k} ({o}), nudge {nudge}", got, *ref[k], 1.0))
                if k == "stats":
                    half_gate(f"{cid} stats summed ({o}), nudge {nudge}", got.sum(0), *ref["stats_sum"], 1.0)
                    old_worst = max(old_worst, D.ratio(got, *old[k]))
    print(f"[dtc gate cpu] {which} {cid} bf16, {flips} realised flips of {a.numel()} staged elements: {name} {new_worst[name]:.3f}, "
          f"statistics {new_worst['stats']:.3f} of the gate; {old_worst:.2f} of the issue's form of the statistics gate")
    assert flips > 0
    if (which, cid) == FLIP_CASES[0]:
        assert old_worst > 1.0, "the case the CHANGED note quotes"


# ------------------------------------------------------------------------------------------------ not vacuous
@pytest.mark.parametrize("defect", sorted(D.DEFECTS))
def test_every_defect_is_seen(defect):
    which, cid, bf16, out = D.DEFECTS[defect]
    c = D.case_of(which, cid)
    inp = D.inputs(c)
    good = D.reference(c, inp, bf16)
    bad = D.reference(c, inp, bf16, defect=defect)
    want, gate = good[out]
    mask = D.defect_mask(c, inp, defect, bf16)
    if mask is not None:
        assert bool(mask.any()), "the defect must touch something at its case"
    share = D.moved(want, bad[out][0], gate, mask)
    print(f"[dtc gate cpu] defect {defect} at {which} {cid} ({'bf16' if bf16 else 'f32'}), output {out}: "
          f"{100 * share:.1f} % of the touched elements moved by more than 10 x the gate")
    assert share >= 0.8, (defect, share)


def test_every_defect_has_a_case():
    for defect, (which, cid, bf16, out) in D.DEFECTS.items():
        c = D.case_of(which, cid)
        assert out in D.reference(c, D.inputs(c), bf16), (defect, out)


# ------------------------------------------------------------------------------------------------ input conditions
def test_operands_are_zero_mean_and_the_flip_share_is_small():
    shares = []
    for which, cases in LISTS.items():
        for c in cases:
            inp = D.inputs(c)
            for k in ("W", "src", "dy", "dz", "y", "ep_y"):
                if k in inp:
                    t = inp[k].double()
                    # (the mean of n independent values scatters by rms / sqrt(n): a few hundred elements cannot show less)
                    assert abs(float(t.mean())) < max(0.05, 3.0 / t.numel() ** 0.5) * float(t.pow(2).mean().sqrt()), (c["id"], k)
            a, ga = D.stage(c, inp)
            flip = float((D.rb(a - ga) != D.rb(a + ga)).double().mean())
            shares.append(flip)
            if c["act"] or c["form"]:
                print(f"[dtc gate cpu] {which} {c['id']}: {100 * flip:.4f} % of the staged elements straddle a bf16 boundary")
            else:
                assert flip == 0.0, "an operand used as stored has no rounding interval"
    assert max(shares) < 0.01


# ------------------------------------------------------------------------------------------------ coverage
def _lib():
    from opensetgaitrecognition_pcaa_amd import _lib
    return _lib.load()


def test_every_route_is_the_target_of_a_forward_and_an_adjoint_case_and_the_library_agrees():
    lib = _lib()
    for which in ("fwd", "adj"):
        hit = set()
        for c in LISTS[which]:
            for bf16 in (False, True):
                want = D.ROUTES.index(f"{c['fam']}_{'bf16' if bf16 else 'f32'}")
                assert D.route(c["adj"], bf16, c["B"], c["cin"], c["cout"], c["ks"]) == want, c["id"]
                assert lib.pcaa_dtc_conv_route(int(c["adj"]), int(bf16), c["B"], c["cin"], c["cout"], c["ks"], 0) == want, c["id"]
                hit.add(want)
        assert hit == set(range(6)), (which, hit)
    for c in LISTS["win"]:
        for bf16 in (False, True):
            assert lib.pcaa_dtc_conv_route(0, int(bf16), c["B"], c["cin"], c["cout"], c["ks"], 1) == int(bf16) == D.route(False, bf16, c["B"], c["cin"], c["cout"], c["ks"], True)
    c = D.case_of("win", "plain_overlap/pair_shape")
    assert D.route(False, False, c["B"], c["cin"], c["cout"], 1, False) == 2, "a pair shape: only the window keeps it on the one-sequence kernel"


def test_conditions_are_taken_both_ways_and_the_predicates_match_their_restatements():
    lib = _lib()
    seen = {}

    def note(name, v):
        seen.setdefault(name, set()).add(bool(v))
    for B, cin, cout in D.grid():          # (tests/test_dtc_plan_cpu.py walks the same grid)
        for adj in (False, True):
            kc, nc = (cout, cin) if adj else (cin, cout)
            for ks in (1, 2):
                for bf16 in (0, 1):
                    assert lib.pcaa_dtc_conv_route(int(adj), bf16, B, cin, cout, ks, 0) == D.route(adj, bf16, B, cin, cout, ks), (adj, B, cin, cout, ks)
                note("ksplit == 1", ks == 1)
            note("kc >= 128", kc >= 128), note("kc % 32 == 0", kc % 32 == 0), note("nc >= 64", nc >= 64), note("nc % 4 == 0", nc % 4 == 0)
            if D.pair_takes(kc, nc, 1, adj):
                note("wide: workgroups >= 192", (B + 1) // 2 * (nc // 64) >= 192)
                if (B + 1) // 2 * (nc // 64) >= 192:
                    note("wide: nc % 64 == 0", nc % 64 == 0)
        ks = lib.pcaa_dtc_conv_ksplit(B, cin, cout)
        assert ks == D.fwd_ksplit(B, cin, cout), (B, cin, cout, ks)
        chunks = D.cdiv(cin, 32)
        note("few workgroups", B * D.cdiv(cout, 32) <= 128), note("chunks >= 16", chunks >= 16)
        if B * D.cdiv(cout, 32) <= 128 and chunks >= 16:
            note("ks > 8", D.cdiv(cin, 256) > 8)
        note("ks < chunks", D.cdiv(cin, 256) < chunks)
        assert lib.pcaa_dtc_conv_dgrad_ksplit(B, cin, cout) == D.dgrad_ksplit(B, cin, cout)
        assert lib.pcaa_dtc_conv_supported(30, cin, cout) == D.supported(30, cin, cout)
    for T in (0, 1, 32, 33):
        for cin, cout in ((4, 16), (2, 16), (6, 16), (4, 8), (4, 24)):
            assert lib.pcaa_dtc_conv_supported(T, cin, cout) == D.supported(T, cin, cout)
    missing = {k: v for k, v in seen.items() if v != {True, False}}
    assert not missing, missing
    # the cases themselves: everything a valid call can reach
    by_case = {}
    for which in ("fwd", "adj"):
        for c in LISTS[which]:
            kc, nc = c["kc"], c["nc"]
            for k, v in (("ksplit == 1", c["ks"] == 1), ("kc >= 128", kc >= 128), ("kc % 32 == 0", kc % 32 == 0), ("nc >= 64", nc >= 64)):
                by_case.setdefault((which, k), set()).add(v)
            if D.pair_takes(kc, nc, c["ks"], c["adj"]):
                by_case.setdefault((which, "wide"), set()).add(D.wide(c["B"], nc))
            if c.get("lib_ks"):
                own = D.dgrad_ksplit(c["B"], c["cin"], c["cout"]) if c["adj"] else D.fwd_ksplit(c["B"], c["cin"], c["cout"])
                assert own == c["ks"], (c["id"], own)
    assert all(v == {True, False} for v in by_case.values()), by_case


def test_every_argument_check_of_the_file_has_a_refusal_case():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opensetgaitrecognition_pcaa_amd", "csrc", "dtc_fused.hip")
    with open(path) as f:
        src = f.read()
    msgs = ["".join(re.findall(r'"((?:[^"\\]|\\.)*)"', m.group(1))) for m in re.finditer(r"PCAA_CHECK_ARG\((.*?)\);\n", src, re.S)]
    assert len(msgs) >= 16
    frags = [f for _, _, f in D.REFUSALS.values()]
    for m in msgs:
        assert any(f in m for f in frags), f"no refusal case ends at: {m}"
    for f in frags:
        assert any(f in m for m in msgs), f"no PCAA_CHECK_ARG says: {f}"
    print(f"[dtc gate cpu] {len(msgs)} argument checks, {len(D.REFUSALS)} refusal cases")


def test_split_ranges_of_the_ksplit_cases():
    """the cases meant to have an empty split, one chunk per split and uneven splits have them"""
    rg = D.split_ranges(544, 8)
    assert rg[5] == (480, 544) and rg[6] == rg[7] == (544, 544)
    assert D.split_ranges(96, 3) == [(0, 32), (32, 64), (64, 96)]
    assert D.split_ranges(160, 2) == [(0, 96), (96, 160)]
    assert D.split_ranges(160, 4) == [(0, 64), (64, 128), (128, 160), (160, 160)]
    assert D.split_ranges(1024, 2) == [(0, 512), (512, 1024)]
