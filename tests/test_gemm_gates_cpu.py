"""The gates, the route table and the case lists of tests/gemm_ref.py, checked on the CPU at the inputs the GPU tests use
(tests/test_gemm_branches.py takes its cases from the same lists; a case larger than 640 x 264 is evaluated on its first
rows and columns, which the hash generator makes a prefix of the full operands).

* NOT TOO TIGHT: float32 torch evaluations of the kernels' formulation -- not the kernels -- in several orders of
  summation (k-sequential; blocked by the MFMA depth, the block summed exactly and rounded once as the matrix pipe does;
  blocked by the 64-deep step; split by K range, then added, forwards and backwards) stay within HALF of every gate.
  For a bf16 output the value before the rounding stays within half the fp32 part, the rounded value within the gate.
  Evaluated once per distinct arithmetic: the cases are de-duplicated by ``sig`` (math, the three dtypes, K, the split
  count and form, accumulate, bias, statistics, split operands, the kernel family whose statistics slices apply, nrep,
  ragged or whole M) -- M, N and the layouts beyond that do not change what is summed, only where it is stored, and the
  first case of each signature is the one evaluated (its id is in the test's name).
* NOT VACUOUS: every planted defect, substituted for the reference at the shape of the case meant to catch it, moves at
  least 80 % of the elements it touches by more than 10 x the gate.
* INPUT CONDITIONS: every operand's |mean| is below 0.05 of its rms; the share of fp16-subnormal lo halves is printed.
* COVERAGE: every name ``route`` / ``route_fused`` can return is the target of a GPU case, every refusal reason of a
  refusal case, every defect of a case, and every condition of the launchers is taken both ways by the cases.
"""
import inspect
import re

import pytest
import torch

import gemm_ref as G
from gemm_ref import BF16, F32, KC, RC, U

ROWS, COLS = 640, 264
LN2 = 0.6931471805599453
CASES = G.gemm_cases(256)
FUSED = G.fused_cases(256)


def f32c(x):
    return torch.tensor(x, dtype=F32)


def fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def half_gate(name, got, want, gate, bound=0.5):
    r = G.ratio(got, want, gate)
    print(f"[gemm gate cpu] {name}: fp32 evaluation worst |err| / gate = {r:.3f}")
    assert r <= bound, (name, r)
    return r


# ------------------------------------------------------------------------------------------------ fp32 evaluations
def seq(a, b, k0=0, k1=None):
    k1 = a.shape[1] if k1 is None else k1
    acc = torch.zeros(a.shape[0], b.shape[0])
    for k in range(k0, k1):
        acc = acc + a[:, k:k + 1] * b[:, k]
    return acc


def blocked_exact(a, b, d, k0=0, k1=None):
    """blocks of d products summed exactly, rounded once, added to the fp32 accumulator (the MFMA's own depth)"""
    k1 = a.shape[1] if k1 is None else k1
    acc = torch.zeros(a.shape[0], b.shape[0])
    for k in range(k0, k1, d):
        e = min(k1, k + d)
        acc = (acc.double() + a[:, k:e].double() @ b[:, k:e].double().t()).float()
    return acc


def blocked_step(a, b, d, k0=0, k1=None):
    """every d-deep step summed on its own in fp32, then added"""
    k1 = a.shape[1] if k1 is None else k1
    acc = torch.zeros(a.shape[0], b.shape[0])
    for k in range(k0, k1, d):
        acc = acc + seq(a, b, k, min(k1, k + d))
    return acc


def orders(a, b, mfma_depth, ranges=None):
    """-> {name: fp32 accumulator} of one pass over K (ranges None) or of the given K ranges added forwards / backwards"""
    K = a.shape[1]
    if ranges is None or len(ranges) == 1:
        thirds = [(i * K // 3, (i + 1) * K // 3) for i in range(3)]
        parts = [seq(a, b, k0, k1) for k0, k1 in thirds if k1 > k0]
        return {"k-sequential": seq(a, b), f"blocked by {mfma_depth} (exact blocks)": blocked_exact(a, b, mfma_depth),
                "blocked by the 64-deep step": blocked_step(a, b, 64), "three K ranges, added": sum(parts[1:], parts[0])}
    return None


def stored32(win, layout, math):
    """the stored window as fp32 values the kernel multiplies, logical [rows, K]"""
    return G.widen(win, layout, math).float()


def slices32(v, h, lanes):
    """fp32 column sums of the slices of h rows in two orders: rows in order; row r on lane r % lanes, lanes then added"""
    rows, ch = v.shape
    nb = G.cdiv(rows, h)
    pv = torch.zeros(nb * h, ch)
    pv[:rows] = v
    pv = pv.view(nb, h, ch)
    s_seq = torch.zeros(nb, ch)
    lane = [torch.zeros(nb, ch) for _ in range(lanes)]
    for r in range(h):
        s_seq = s_seq + pv[:, r]
        lane[r % lanes] = lane[r % lanes] + pv[:, r]
    s_lane = lane[0]
    for l in lane[1:]:
        s_lane = s_lane + l
    return s_seq, s_lane


def replicas(s, kernel, nrep):
    tile, h, _ = G.SLICES[kernel]
    rep = (torch.arange(s.shape[0]) // (tile // h)) % nrep
    return torch.zeros(nrep, s.shape[1], dtype=torch.float64).index_add_(0, rep, s.double())


def stats32(name, v1, v2, kernel, nrep, want, gate):
    """v1, v2: the fp32 summands of the two statistics [rows, ch]"""
    _, h, lanes = G.SLICES[kernel]
    for which, (a, b) in zip(("rows in order", "row lanes"), zip(slices32(v1, h, lanes), slices32(v2, h, lanes))):
        got = torch.stack([replicas(a, kernel, nrep), replicas(b, kernel, nrep)], 1)
        half_gate(f"{name} statistics, {which}", got, want, gate)


# ------------------------------------------------------------------------------------------------ not too tight
def sig(c):
    return (c["math"], c["adt"], c["bdt"], c["cdt"], c["K"], c["split_k"], c["slabs"], c["accumulate"], c["bias"], c["colstats"],
            c["split3"], G.kernel_of(c["route"]), c["nrep"], min(c["M"], ROWS) % 256 != 0)


def distinct(cases):
    seen, out = set(), []
    for c in cases:
        if sig(c) not in seen:
            seen.add(sig(c))
            out.append(c)
    return out


DISTINCT = distinct(CASES)


def operands32(c, bt):
    """-> (a, b [fp32, logical], depth, scale): the values the matrix pipe multiplies (split: the 3 K long walk of the images)"""
    if c["split3"]:
        sa, sb = G.SPLIT_SCALES
        ha, la = G.split_halves(bt["A"], 1.0, c["alay"])
        hb, lb = G.split_halves(bt["B"], 1.0, c["blay"])
        return torch.cat([ha, la, ha], 1).float(), torch.cat([hb, hb, lb], 1).float(), 32, 1.0 / (sa * sb)
    return stored32(bt["A"], c["alay"], c["math"]), stored32(bt["B"], c["blay"], c["math"]), (2 if c["math"] == G.M_F32 else 16), 1.0


@pytest.mark.parametrize("c", DISTINCT, ids=[c["id"] for c in DISTINCT])
def test_fp32_evaluations_stay_within_half_the_gate(c):
    bt = G.build(c, "cpu", ROWS, COLS)
    p = G.reference(c, bt)
    a, b, depth, os_ = operands32(c, bt)
    name = c["id"]
    K = a.shape[1]
    kern = G.kernel_of(c["route"])
    ns = len(p["slabs"])
    multi = (c["split_k"] > 1 or c["slabs"]) and ns > 1
    if not multi:
        for oname, acc in orders(a, b, depth).items():
            acc = acc * f32c(os_)
            out = acc
            if c["accumulate"]:
                out = bt["out0"] + out
            if c["bias"]:
                out = out + bt["bias"]
            half_gate(f"{name} [{oname}]", out, p["want"], p["gate32"])
            if c["cdt"] == BF16:
                half_gate(f"{name} [{oname}] rounded to bf16", out.to(BF16), p["want"], p["gate"], bound=1.0)
            if c["colstats"] and oname in ("k-sequential", "blocked by the 64-deep step"):
                stats32(f"{name} [{oname}]", acc, acc * acc, kern, c["nrep"], p["stats"], p["stats_gate"])
        return
    rg = G.k_ranges(G.M_BF16 if c["split3"] else c["math"], K, c["split_k"])
    assert len(rg) == ns
    parts = []
    for s, (k0, k1) in enumerate(rg):
        for oname, fn in (("k-sequential", lambda: seq(a, b, k0, k1)), ("exact blocks", lambda: blocked_exact(a, b, depth, k0, k1))):
            part = fn() * f32c(os_)
            half_gate(f"{name} slab {s} [{oname}]", part, *p["slabs"][s])
        parts.append(part)
    for oname, order in (("forwards", parts), ("backwards", parts[::-1])):
        out = bt["out0"].clone() if c["accumulate"] else torch.zeros_like(parts[0])
        for i, part in enumerate(order):
            out = out + (part + bt["bias"] if (c["bias"] and i == 0) else part)
        half_gate(f"{name} ranges added {oname}", out, p["want"], p["gate32"])


FUSED_DISTINCT = [c for c in FUSED if not c.get("big")]


@pytest.mark.parametrize("c", FUSED_DISTINCT, ids=[c["id"] for c in FUSED_DISTINCT])
def test_fused_epilogues_in_fp32_stay_within_half_the_gate(c):
    bt = G.fused_inputs(c, "cpu", ROWS)
    ref = G.fused_reference(c, bt)
    a, b, depth, os_ = operands32(bt["case"], bt)
    l2 = f32c(G.LOG2E)
    sc, sh, mu, rs = bt["scale"], bt["shift"], bt["mean"], bt["rstd"]
    for oname, acc in orders(a, b, depth).items():
        acc = acc * f32c(os_)
        name = f"{c['id']} [{oname}]"
        if c["epi"] == "dgrad":
            y = bt["y"].float()
            if c["split3"]:
                z = y * sc + sh
                g = torch.where(z > 0, torch.ones_like(z), torch.exp(z))
            else:
                g = torch.exp2(fma(y, sc * l2, sh * l2)).clamp(0.0, 1.0)
            dz = acc * g
            half_gate(name + " dz", dz, ref["dz"], ref["dz_gate32"])
            if not c["split3"]:
                half_gate(name + " dz rounded to bf16", dz.to(BF16), ref["dz"], ref["dz_gate"], bound=1.0)
            if oname in ("k-sequential", "blocked by the 64-deep step"):
                stats32(name, dz, dz * fma(y, rs, -mu * rs), "v2", 16, ref["stats"], ref["stats_gate"])
            continue
        z2 = fma(acc, sc * l2, sh * l2)
        e = torch.exp2(z2).clamp(0.0, 1.0)
        act = fma(z2.clamp_min(0.0), f32c(LN2), e - 1)
        R = c["pool_rows"]
        if not R:
            half_gate(name, act, ref["want"], ref["gate32"])
            half_gate(name + " rounded to bf16", act.to(BF16), ref["want"], ref["gate"], bound=1.0)
            continue
        v = act.view(-1, R, act.shape[1])
        s = torch.zeros(v.shape[0], v.shape[2])
        for r in range(R):
            s = s + v[:, r]
        half_gate(name + f" mean of {R} rows", s * f32c(1.0 / R), ref["want"], ref["gate"])


# ------------------------------------------------------------------------------------------------ not vacuous
STATS_DEFECTS = ("stats_wrong_replica_lost", "stats_from_rounded", "ragged_rows_in_stats")
DEFECT_CASES = [(c, d) for c in CASES for d in c["defects"]]
FUSED_DEFECT_CASES = [(c, d) for c in FUSED for d in c["defects"]]


def defect_moves(name, want, bad, gate, mask=None):
    f = G.moved(want, bad, gate, mask)
    print(f"[gemm gate cpu] {name}: moved {f:.1%}")
    assert f >= 0.8, (name, f)


@pytest.mark.parametrize("c,defect", DEFECT_CASES, ids=[f"{c['id']}-{d}" for c, d in DEFECT_CASES])
def test_planted_defects_exceed_the_gate(c, defect):
    bt = G.build(c, "cpu", ROWS, COLS)
    good, bad = G.reference(c, bt), G.reference(c, bt, defect)
    if defect in STATS_DEFECTS:
        defect_moves(f"{c['id']} {defect}", good["stats"], bad["stats"], good["stats_gate"])
    elif defect == "split_lo_swapped":
        # Looked for in the SLABS of a split product, which the GPU file gates one by one: the slabs of the hi.lo segment
        # hold small terms only.  In a whole product (K = 128, the routes' minimum) the 2 K small terms are added to the
        # finished hi.hi sum, whose roundings the gate has to admit: there the defect moved 77.5 % of the elements.
        stack = lambda r, i: torch.stack([s[i] for s in r["slabs"]])
        defect_moves(f"{c['id']} {defect} (slabs)", stack(good, 0), stack(bad, 0), stack(good, 1))
    else:
        defect_moves(f"{c['id']} {defect}", good["want"], bad["want"], good["gate"])


@pytest.mark.parametrize("c,defect", FUSED_DEFECT_CASES, ids=[f"{c['id']}-{d}" for c, d in FUSED_DEFECT_CASES])
def test_planted_defects_of_the_fused_epilogues(c, defect):
    bt = G.fused_inputs(c, "cpu", ROWS)
    good, bad = G.fused_reference(c, bt), G.fused_reference(c, bt, defect)
    if c["epi"] == "affine":
        defect_moves(f"{c['id']} {defect}", good["want"], bad["want"], good["gate"])
    elif defect in STATS_DEFECTS:
        defect_moves(f"{c['id']} {defect}", good["stats"], bad["stats"], good["stats_gate"])
    else:
        defect_moves(f"{c['id']} {defect} dz", good["dz"], bad["dz"], good["dz_gate"])
        defect_moves(f"{c['id']} {defect} statistics", good["stats"], bad["stats"], good["stats_gate"])


def test_every_defect_has_a_case():
    used = {d for _, d in DEFECT_CASES} | {d for _, d in FUSED_DEFECT_CASES}
    assert used == set(G.DEFECTS), (set(G.DEFECTS) - used, used - set(G.DEFECTS))


# ------------------------------------------------------------------------------------------------ input conditions
def test_operands_are_zero_mean_and_the_subnormal_share_is_known():
    worst, shares = 0.0, []
    for c in DISTINCT + [f for f in FUSED_DISTINCT]:
        bt = G.build(c, "cpu", ROWS, COLS) if "epi" not in c else G.fused_inputs(c, "cpu", ROWS)
        cc = bt.get("case", c)
        if cc["split3"]:
            ops_ = [sum(G.split_halves(bt["A"], 1.0, cc["alay"])), sum(G.split_halves(bt["B"], 1.0, cc["blay"]))]
            shares += [G.subnormal_lo_share(bt["A"]), G.subnormal_lo_share(bt["B"])]
            for img in (bt["A"], bt["B"]):
                hi = img[:, :img.shape[1] // 2].double().abs()
                assert float(hi.min()) >= 16.0 and float(hi.max()) <= 2048.0
        else:
            ops_ = [G.widen(bt["A"], cc["alay"], cc["math"]), G.widen(bt["B"], cc["blay"], cc["math"])]
        for x in ops_:
            if x.numel() >= 4096:           # (a 4 x 33 operand has no mean to speak of: its gate is the worst-case term)
                worst = max(worst, float(x.mean().abs() / x.pow(2).mean().sqrt()))
        if "y" in bt:                       # fused cases: z = y scale + shift has both signs in every column
            z = bt["y"].double() * bt["scale"].double() + bt["shift"].double()
            assert bool(((z > 0).any(0) & (z < 0).any(0)).all()), c["id"]
    print(f"[gemm gate cpu] worst |mean| / rms over the operands: {worst:.4f}")
    print(f"[gemm gate cpu] fp16-subnormal lo halves: mean share {sum(shares) / len(shares):.4%}, largest {max(shares):.4%}")
    assert worst < 0.05
    assert max(shares) > 0.0, "the split operands are meant to contain subnormal lo halves"


# ------------------------------------------------------------------------------------------------ coverage
def test_every_route_is_the_target_of_a_case():
    targets = {c["route"] for c in CASES}
    for c in CASES:
        assert G.case_route(c, 256) == c["route"], (c["id"], c["route"], G.case_route(c, 256))
    missing = G.all_routes(256) - targets
    print("[gemm gate cpu] routes:", *sorted(targets), sep="\n    ")
    assert not missing, sorted(missing)
    assert not {t for t in targets - G.all_routes(256)}, sorted(targets - G.all_routes(256))
    ftargets = {c["route"] for c in FUSED}
    print("[gemm gate cpu] fused routes:", *sorted(ftargets), sep="\n    ")
    assert G.all_fused_routes(256) == ftargets, (sorted(G.all_fused_routes(256) - ftargets), sorted(ftargets - G.all_fused_routes(256)))
    for n in (104, 256, 304):               # the over-CU-count cases follow the device's CU count
        assert {c["route"] for c in G.gemm_cases(n)} >= G.all_routes(n)


def test_every_refusal_reason_has_a_case():
    src = inspect.getsource(G.route) + inspect.getsource(G._route_split3) + inspect.getsource(G.route_fused)
    reasons = set(re.findall(r'"refused/(\w+)"', src))
    print("[gemm gate cpu] refusal reasons:", *sorted(reasons), sep="\n    ")
    assert reasons == set(G.REFUSALS), (reasons - set(G.REFUSALS), set(G.REFUSALS) - reasons)
    for reason, kw in G.REFUSALS.items():
        if kw is not None:
            assert G.refusal_route(G.refusal_case(reason)) == "refused/" + reason, (reason, G.refusal_route(G.refusal_case(reason)))


def test_every_argument_check_of_the_entry_points_has_a_refusal_case():
    """against the source, not against gemm_ref's own names: every PCAA_CHECK_ARG of csrc/gemm.hip is the end of a refusal
    case (REFUSAL_MESSAGES, ABI_REFUSALS: message prefix + fragment) or is listed as out of reach"""
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opensetgaitrecognition_pcaa_amd", "csrc", "gemm.hip")
    with open(path) as f:
        src = f.read()
    msgs = ["".join(re.findall(r'"((?:[^"\\]|\\.)*)"', m.group(1))) for m in re.finditer(r"PCAA_CHECK_ARG\((.*?)\);\n", src, re.S)]
    assert len(msgs) >= 40
    have = list(G.REFUSAL_MESSAGES.values()) + [(p, f) for _, p, f, _ in G.ABI_REFUSALS]
    assert set(G.REFUSAL_MESSAGES) == {r for r, v in G.REFUSALS.items() if v is not None}
    for msg in msgs:
        hit = any(msg.startswith(p) and f in msg for p, f in have)
        skipped = any(msg.startswith(p) and f in msg for p, f in G.OUT_OF_REACH)
        assert hit or skipped, ("no refusal case ends in this check", msg)
    for p, f in have + G.OUT_OF_REACH:
        assert any(msg.startswith(p) and f in msg for msg in msgs) or f == "unsupported dtype combination", ("no such check", p, f)


def conditions(c):
    """the booleans of gemm_impl / pcaa_launch_gemm_bf16_big / launch_dma for a product case"""
    lda, ldb, ldc = G.case_lds(c)
    M, N, K = c["M"], c["N"], c["K"] * (3 if c["split3"] else 1)
    math = G.M_BF16 if c["split3"] else c["math"]
    ns, kps = G.num_splits(math, K, max(c["split_k"], 1)) if K > 0 else (1, 64)
    atomic = not c["slabs"] and (c["split_k"] > 1 or c["accumulate"])
    ntiles = G.cdiv(M, 256) * G.cdiv(N, 256)
    al = lambda x: x not in c["misaligned"]
    d = {"math is bf16": math == G.M_BF16, "atomic": atomic, "slabs": c["slabs"], "bias": c["bias"], "colstats": c["colstats"],
         "C is fp32": c["cdt"] == F32, "split operands": c["split3"], "fewer ranges than asked": ns < c["split_k"],
         "last range partial": K % kps != 0}
    if math == G.M_F32:
        d.update({"f32: A aligned": al("A"), "f32: B aligned": al("B"), "f32: lda % 4": lda % 4 == 0, "f32: ldb % 4": ldb % 4 == 0,
                  "f32: K % 4": K % 4 == 0, "f32: A is KC": c["alay"] == KC, "f32: B is KC": c["blay"] == KC,
                  "f32: M % 4": M % 4 == 0, "f32: N % 4": N % 4 == 0})
        return d
    d.update({"N < 128": N < 128, "A, B aligned": al("A") and al("B"), "K % 8": K % 8 == 0, "A is KC": c["alay"] == KC,
              "layouts equal": c["alay"] == c["blay"], "A is bf16": c["adt"] == BF16, "B is bf16": c["bdt"] == BF16,
              "M % 256": M % 256 == 0, "N % 256": N % 256 == 0, "K % 64": K % 64 == 0,
              "v2 enabled": c["v2_on"], "one K range": ns == 1, "at least five steps": K // 64 >= 5, "ldc % 8": ldc % 8 == 0,
              "C aligned": al("C"), "split_fast": bool(c["slabs"]) and ns >= 8 and ns % 8 == 0 and ntiles * ns >= 256,
              "nsplit % 8 with slabs": bool(c["slabs"]) and ns % 8 == 0, "more tiles than CUs": ntiles > 256,
              "tile count % 8": ntiles % 8 == 0, "tail": c["tail"], "lda padded": bool(c["lda"]), "ldc padded": bool(c["ldc"])})
    return d


def test_every_condition_is_taken_both_ways():
    seen = {}
    allc = CASES + [G.refusal_case(r) for r, v in G.REFUSALS.items() if v is not None and "fused" not in v]
    for c in allc:
        for k, v in conditions(c).items():
            seen.setdefault(k, set()).add(bool(v))
    one_way = sorted(k for k, v in seen.items() if len(v) < 2)
    assert not one_way, one_way
