"""The gates of tests/skinny_ref.py, checked on the CPU: what tests/test_skinny_branches.py asserts of the kernels of
csrc/gemm_skinny.hip is reference-safe (an fp32 evaluation in the kernel's order stays within HALF of every gate),
defect-sensitive (every planted defect moves >= 80 % of the elements it touches by more than 10 gates) and complete
(every route, every defect and every PCAA_CHECK_ARG of the file has a case).  Figures: pytest -rP.

The fp32 evaluation: operands as the MFMA sees them (bf16-rounded or unrounded, held as fp32), one fp32 matmul per
chunk of 64 added to the accumulator in chunk order, the splits' ranges, the slabs summed in order, bias, expm1 in fp32;
the gathered forms chunk by chunk of rows; Adam in torch.float32 arithmetic, expression for expression.  A long N (the
shapes that reach 2 and 4 column steps per wave) is evaluated at its first 640 rows: the generators make them a prefix,
and no gate depends on N.
"""
import os
import re

import pytest
import torch

import elementwise_ref as E
import skinny_ref as R

F32, BF16 = torch.float32, torch.bfloat16
N_MAX = 640
CASES = R.cases()
BY_ID = {R.case_id(c): c for c in CASES}


def _as32(t, variant):
    return R.widen(t, variant).float()


def _chunked(a, b, k0, k1):
    acc = torch.zeros((a.shape[0], b.shape[0]), dtype=F32)
    for k in range(k0, k1, 64):
        acc = acc + a[:, k:k + 64] @ b[:, k:k + 64].t()
    return acc


def fwd_f32(c, bt):
    a, b = _as32(bt["x"].win, c["variant"]), _as32(bt["W"].win, c["variant"])
    slabs = [_chunked(a, b, k0, k1) for k0, k1 in R.split_ranges(c["K"] // 64, R.case_nsplit(c))]
    v = slabs[0]
    for s in slabs[1:]:
        v = v + s
    if bt["bias"] is not None:
        v = v + bt["bias"]
    return torch.where(v > 0, v, torch.expm1(v)) if c["act"] else v


def dgrad_f32(c, bt):
    a, b = _as32(bt["dz"].win, c["variant"]), _as32(bt["W"].win, c["variant"]).t().contiguous()
    slabs = [_chunked(a, b, n0, n1) for n0, n1 in R.split_ranges(c["N"] // 64, R.case_nsplit(c))]
    v = slabs[0]
    for s in slabs[1:]:
        v = v + s
    if bt["a_prev"] is not None:
        ap = bt["a_prev"]
        v = v * torch.where(ap > 0, torch.ones_like(ap), ap + 1.0)
    return v + bt["out0"] if c["accumulate"] else v


def grad_f32(c, bt, P=None, cs=None):
    """the fused forms' accumulator: one fp32 product per 64-row chunk, added in chunk order"""
    N, K = bt["N"], c["K"]
    acc = torch.zeros((N, K), dtype=F32)
    if c["entry"] == "t16":
        for ch in range(c["chunks"]):
            img = P[ch * cs:ch * cs + (N + K) * 64].view(N + K, 64).float()
            acc = acc + img[:N] @ img[N:].t()
        return acc
    variant = "exact" if c["variant"] == "exact" else "bf16"
    dz, x = bt["dz"].rows(c["M"]), bt["x"].rows(c["M"])
    for r in range(0, c["M"], 64):
        acc = acc + _as32(dz[r:r + 64], variant).t() @ _as32(x[r:r + 64], variant)
    return acc


def adam_f32(p, m, v, acc, coef, hp=R.HP):
    """common.h::adam_update in torch.float32"""
    t = lambda x: torch.tensor(x, dtype=F32)
    b1, b2, eps, gs, ss, ibc = t(hp["b1"]), t(hp["b2"]), t(hp["eps"]), t(hp["gs"]), t(coef[0]), t(coef[1])
    g = acc * gs
    m1 = b1 * m + (1 - b1) * g
    v1 = b2 * v + ((1 - b2) * g) * g
    denom = torch.sqrt(v1) * ibc + eps
    return p - ss * (m1 / denom), m1, v1


def _note(worst, key, r):
    worst[key] = max(worst.get(key, 0.0), r)


def _report(worst, what):
    for k in sorted(worst):
        print(f"[skinny-cpu] {what} {k}: fp32 evaluation / gate = {worst[k]:.3f}")
    assert worst and max(worst.values()) <= 0.5, {k: v for k, v in worst.items() if v > 0.5}


# ===================================================================================================== the half rule
@pytest.mark.parametrize("variant", R.FWD_VARIANTS)
def test_half_rule_forward(variant):
    worst = {}
    for c in CASES:
        if c["entry"] == "fwd" and c["variant"] == variant:
            bt = R.build(c)
            ref = R.reference(c, bt)
            _note(worst, R.case_route(c), R.ratio(fwd_f32(c, bt), ref["want"], ref["gate"]))
    _report(worst, "forward")


@pytest.mark.parametrize("form", R.DGRAD_FORMS)
def test_half_rule_dgrad(form):
    worst = {}
    for c in CASES:
        if c["entry"] == "dgrad" and c["form"] == form:
            bt = R.build(c)
            ref = R.reference(c, bt)
            _note(worst, R.case_route(c), R.ratio(dgrad_f32(c, bt), ref["want"], ref["gate"]))
    _report(worst, "dgrad")


@pytest.mark.parametrize("variant", R.WG_VARIANTS)
def test_half_rule_wgrad(variant):
    """a bf16 output: the value before the rounding within half of the fp32 part, the rounded value within the whole gate
    (the rounding reaches the whole of its own term by itself, as in elementwise_ref)"""
    worst, rounded = {}, 0.0
    for c in CASES:
        if c["entry"] == "wgrad" and c["variant"] == variant:
            bt = R.build(c)
            ref = R.reference(c, bt)
            got = grad_f32(dict(c, variant="exact" if variant == "exact" else "bf16"), bt)
            gate32 = ref["gate"] - (R.BF16_ROUND * ref["want"].abs() if variant == "bf16" else 0.0)
            _note(worst, R.case_route(c), R.ratio(got, ref["want"], gate32))
            if variant == "bf16":
                rounded = max(rounded, R.ratio(got.to(BF16), ref["want"], ref["gate"]))
    if variant == "bf16":
        print(f"[skinny-cpu] wgrad bf16: rounded fp32 evaluation / whole gate = {rounded:.3f}")
        assert rounded <= 1.0
    _report(worst, "wgrad")


def _update_case(c, worst):
    """two steps (one from zero moments) of a fused-update case in fp32 against the reference from the same state"""
    n_max = N_MAX if c["N"] > 4096 else None
    frames = R.state(c, n_max=n_max, ldw=c["K"] + 3)
    cs = (min(c["N"], n_max or c["N"]) + c["K"]) * 64 + 64
    JL, NB = R.ring_of(c)
    for step in ((1,) if c["zero"] else (1, 2)):
        bt = R.build(c, n_max=n_max, step=step)
        P = R.packed(c, bt, bt["N"], cs) if c["entry"] == "t16" else None
        coef = R.coef_ref(step)
        p, m, v = (f.win.clone() for f in frames)
        ref = R.wgrad_adam_ref(R.gradient(c, bt, P=P, chunk_stride=cs), p, m, v, step, coef, JL, NB)
        got = adam_f32(p, m, v, grad_f32(c, bt, P, cs), coef)
        for name, g in zip("pmv", got):
            _note(worst, f"{R.case_route(c)} {name}", R.ratio(g, *ref[name]))
        for f, g in zip(frames, got):
            f.win.copy_(g)


@pytest.mark.parametrize("entry", ["adam", "rows", "t16"])
def test_half_rule_fused_update(entry):
    worst = {}
    for c in CASES:
        if c["entry"] == entry:
            _update_case(c, worst)
    _report(worst, "fused update")


def test_stored_coefficients_and_adam_ref_agree():
    """the wanted values are formed with the stored fp32 coefficients, the gates by elementwise_ref.adam_ref from lr and
    the step: the two differ by the coefficients' fp32 rounding, a small share of the gate"""
    c = BY_ID["adam-bf16-33x130x96-zero0"]
    bt, frames = R.build(c), R.state(c)
    p, m, v = (f.win for f in frames)
    r = R.gradient(c, bt)
    ref = R.wgrad_adam_ref(r, p, m, v, 2, R.coef_ref(2))
    e = E.adam_ref(p, r["acc"], m, v, R.HP["lr"], R.HP["b1"], R.HP["b2"], R.HP["eps"], 2, R.HP["gs"])
    for k in "pmv":
        assert R.ratio(e[k][0], *ref[k]) <= 0.25, k


# ===================================================================================================== planted defects
def _defect_share(defect):
    c = dict(BY_ID[R.DEFECT_CASE[defect]], rows_extra=1)
    if c["entry"] in ("fwd", "dgrad", "wgrad"):
        bt = R.build(c, tail="finite")
        out = bt.get("y") or bt.get("dx") or R.Framed(torch.full((c["N"], c["K"]), R.SENTINEL["dW"]), c["K"] + 2)
        want = R.reference(c, bt)
        bad = R.reference(c, bt, defect=defect, before=out.win)
        mask = bad.get("touched")
        if defect == "reduce_second_trip_skipped":
            mask = (torch.arange(want["want"].numel()) >= 4 * R.REDUCE_QUADS).view(want["want"].shape)
        if defect == "col_clamp_dup":
            mask = torch.zeros(want["want"].shape, dtype=torch.bool)
            mask[:, -1] = True
        return {"out": R.moved(want["want"], bad["want"], want["gate"], mask)}
    bt = R.build(c, tail="finite")
    frames = R.state(c, ldw=c["K"] + 3)
    cs = (c["N"] + c["K"]) * 64 + 64
    P = R.packed(c, bt, c["N"], cs) if c["entry"] == "t16" else None
    JL, NB = R.ring_of(c)
    p, m, v = (f.win for f in frames)
    grad_defect = defect if defect in ("chunk_dropped", "dz_rows_unmasked", "kslot_mismatch", "truncating_bf16") else None
    want = R.wgrad_adam_ref(R.gradient(c, bt, P=P, chunk_stride=cs), p, m, v, 1, R.coef_ref(1), JL, NB)
    bad = R.wgrad_adam_ref(R.gradient(c, bt, grad_defect, P, cs), p, m, v, 1, R.coef_ref(1), JL, NB,
                           defect=None if grad_defect else defect, frames=frames)
    return {k: R.moved(want[k][0], bad[k][0], want[k][1], bad["touched"]) for k in "pmv"}


def test_every_planted_defect_moves_what_it_touches():
    """>= 80 % of the touched elements by more than 10 gates.  A forward / dgrad / plain-gradient defect is looked for in
    the output; a defect of the fused update in exp_avg (the gradient enters it linearly: no cancellation against the
    state as in W, no square as in exp_avg_sq) -- the shares of W and exp_avg_sq are printed beside it."""
    for d in R.DEFECTS:
        s = _defect_share(d)
        key = "out" if "out" in s else "m"
        print(f"[skinny-cpu] defect {d} at {R.DEFECT_CASE[d]}: moved " + ", ".join(f"{k} {100 * v:.1f} %" for k, v in s.items()))
        assert s[key] >= 0.8, (d, s)


# ===================================================================================================== coverage
def test_every_route_and_every_defect_has_a_case():
    targeted = {R.case_route(c) for c in CASES}
    assert "refused" not in targeted
    every = set(R.all_routes())
    assert targeted == every, sorted(every ^ targeted)
    assert set(R.DEFECT_CASE) == set(R.DEFECTS)
    for d, cid in R.DEFECT_CASE.items():
        assert cid in BY_ID, (d, cid)
    print(f"[skinny-cpu] {len(CASES)} cases, {len(targeted)} of {len(every)} routes targeted, {len(R.DEFECTS)} defects")
    # the column steps of the shapes that exist for them: wave 0 full, wave 1 ragged, waves 2 - 3 without work
    assert R.wave_steps(160, 4) == [(0, 4), (128, 1)] and R.wave_steps(288, 2) == [(0, 2), (64, 2), (128, 2), (192, 2), (256, 1)]
    for (N, K), jl in R.WIDE_JL.items():
        assert R.cols_per_wave(N, K) == jl
    for (N, K), jl in R.T16_DEEP_JL.items():
        assert R.cols_per_wave(N, K, 384) == jl and R.cols_per_wave(N, K) == 1
    for c in CASES:
        if c["entry"] in ("adam", "rows", "t16") and (c["N"], c["K"]) not in R.WIDE_JL and (c["N"], c["K"]) not in R.T16_DEEP_JL:
            assert R.ring_of(c)[0] == 1


def test_split_counts_of_the_cases():
    """the forward shapes take the paths they exist for: one chunk / one split of several chunks (the kernel's own
    epilogue), slabs with cps dividing the chunks and not (7 chunks in 3 splits: 3 + 3 + 1)"""
    assert [R.splits(0, N, K) for N, K in R.FWD_NK] == [1, 1, 1, 2, 3]
    assert R.split_ranges(7, 3) == [(0, 192), (192, 384), (384, 448)]
    assert [R.splits(1, N, 64) for N in R.DGRAD_N] == [1, 1, 3]
    M, N, K, ns = R.BIG_REDUCE
    assert M * N // 4 > R.REDUCE_QUADS and K // 64 == ns


def test_every_argument_check_of_the_file_has_a_refusal_case():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opensetgaitrecognition_pcaa_amd", "csrc",
                        "gemm_skinny.hip")
    with open(path) as f:
        src = f.read()
    msgs = ["".join(re.findall(r'"((?:[^"\\]|\\.)*)"', m.group(1))) for m in re.finditer(r"PCAA_CHECK_ARG\((.*?)\);\n", src, re.S)]
    assert len(msgs) >= 30
    have = [(p, f) for _, p, f, _ in R.REFUSALS]
    for msg in msgs:
        hit = any(msg.startswith(p) and f in msg for p, f in have)
        skipped = any(msg.startswith(p) and f in msg for p, f in R.OUT_OF_REACH)
        assert hit or skipped, ("no refusal case ends in this check", msg)
    for p, f in have + R.OUT_OF_REACH:
        assert any(msg.startswith(p) and f in msg for msg in msgs), ("no such check", p, f)
    print(f"[skinny-cpu] {len(msgs)} PCAA_CHECK_ARG, {len(R.REFUSALS)} refusal cases, {len(R.OUT_OF_REACH)} out of reach")


# ===================================================================================================== input conditions
def test_input_conditions():
    """zero-mean operands (|mean| / rms <= 0.05) and exp_avg_sq >= 1e-4 (denom is not eps) in every nonzero-moment case"""
    seen, worst, count = set(), 0.0, 0
    for c in CASES:
        key = (c["entry"], c["N"], c["K"], c["M"])
        if key in seen:
            continue
        seen.add(key)
        n_max = N_MAX if c["N"] > 4096 else None
        bt = R.build(c, n_max=n_max)
        ops_ = [bt[name].rows(min(c["M"], bt[name].r)) if name != "W" else bt[name].win for name in ("x", "dz", "W") if name in bt]
        ops_ += [t for pair in bt.get("chunks", []) for t in pair]
        for t in ops_:
            r = R.mean_over_rms(t)
            if r is not None:
                worst, count = max(worst, r), count + 1
        if c["entry"] in ("adam", "rows", "t16") and not c["zero"]:
            _, m, v = R.state(c, n_max=n_max)
            assert float(v.win.min()) >= 1e-4 and float(m.win.abs().max()) > 0
    print(f"[skinny-cpu] worst |mean| / rms over the {count} operands of >= 4096 values: {worst:.4f}")
    assert worst <= 0.05


def test_pack_ref_is_the_transposed_image():
    dz, x = R.mat(9, 5, 3), R.mat(9, 4, 4)
    img = R.pack_ref(dz, x, 9)
    assert img.shape == (9, 64) and torch.equal(img[:5, :9], dz.t().to(BF16)) and not bool(img[:, 9:].any())
    assert sorted(R.kslot_perm().tolist()) == list(range(64)) and R.kslot_perm()[8] == 32
