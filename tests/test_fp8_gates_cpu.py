"""The gates, input conditions and planted defects of tests/fp8_ref.py, on the CPU (no GPU needed), plus the ABI side of
the fp8 route: header and library agree on version 29 and the library exports the new entry points.

Every figure is printed before it is asserted (pytest -s shows them)."""
import ctypes
import os
import re

import pytest
import torch

import fp8_ref as R
import gemm_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c["id"]: c for c in R.cases(256) if not c["big"]}
_BUILT = {}


def built(cid):
    if cid not in _BUILT:
        c = CASES[cid]
        bt = R.build(c)
        _BUILT[cid] = (c, bt, R.reference(c, bt))
    return _BUILT[cid]


# the share of a case's outputs a defect must move beyond the gate (of the elements it touches at all where that is a
# subset: the clamp only matters in the two large-scale columns, the group shift in one row of 32)
SHARE = {"truncate": 0.3, "no_saturate": 0.2, "scale_unfolded": 0.9, "fnuz_bias": 0.9, "drop_last_kstep": 0.9, "khalf_crossed": 0.9,
         "coef_shift_col": 0.9, "pool_group_shift": 0.9}
# ... and on e4m3 OUTPUTS a defect of the accumulator or of the coefficients shows only where the output responds: the
# columns with a negative shift (half of them, |shift| >= 1.5) sit on ELU's flat branch, slope below 0.22 against e4m3's
# spacing of 1/16 there, so half the outputs is what such a defect is asked to move; the bf16 case asks the full share
E4M3_SHARE = {d: 0.5 for d in ("scale_unfolded", "fnuz_bias", "drop_last_kstep", "khalf_crossed", "coef_shift_col")}
DEFECT_CASES = [(cid, d) for cid, c in CASES.items() for d in c["defects"]]


def test_every_defect_is_planted_somewhere():
    assert {d for _, d in DEFECT_CASES} == set(R.DEFECTS)


@pytest.mark.parametrize("cid,defect", DEFECT_CASES, ids=[f"{a}-{b}" for a, b in DEFECT_CASES])
def test_defect_leaves_the_gate(cid, defect):
    c, bt, ref = built(cid)
    bad = R.stored(c, R.reference(c, bt, defect), defect)
    good = R.stored(c, ref)
    out = R.outside(c, bad, ref)
    touched = torch.ones_like(out)
    if defect == "no_saturate":
        touched = ref["want"].abs() > R.E4M3_MAX
    share = float(out[touched & ~torch.isnan(ref["want"])].double().mean())
    asked = E4M3_SHARE.get(defect, SHARE[defect]) if c["out"] == "e4m3" else SHARE[defect]
    print(f"[fp8 gates] {cid} {defect}: {share:.3f} of the outputs outside the gate (asked {asked})")
    assert not bool(R.outside(c, good, ref).any()), "the reference's own stored values pass"
    assert share >= asked


@pytest.mark.parametrize("cid", list(CASES))
def test_fp32_evaluation_inside_half_the_gate_and_ends_rarely_differ(cid):
    c, bt, ref = built(cid)
    a, w = R.dq(bt["A"]).float(), R.dq(bt["W"]).float()
    z = (a @ w.t()) * bt["scale8"] + bt["shift"]
    v = torch.where(z > 0, z, torch.expm1(z))
    if c["pool_rows"]:
        v = v.view(-1, c["pool_rows"], v.shape[1]).mean(1)
    ok = ~torch.isnan(ref["want"])
    assert bool(torch.isnan(v)[~ok].all()) and not bool(torch.isnan(v)[ok].any()), "the NaN reaches exactly its own row"
    assert int((~ok).any(1).sum()) == 1 and bool((~ok)[5 // (c["pool_rows"] or 1)].all())
    r = float(((v.double() - ref["want"]).abs() / ref["gate32"])[ok].max())
    print(f"[fp8 gates] {cid}: fp32 evaluation at {r:.3f} of the fp32 gate")
    assert r <= 0.5
    if c["out"] == "e4m3":
        share = R.ends_differ(ref["want"], ref["gate"])
        print(f"[fp8 gates] {cid}: the ends of the e4m3 interval differ for {share:.2e} of the elements")
        assert share < 0.01
        # the corners are there: clamped outputs and outputs in the subnormal range (below 2^-6)
        assert int((ref["want"][ok].abs() > R.E4M3_MAX).sum()) > 0
        sub = (ref["want"].abs() < 2.0 ** -6) & (ref["want"] != 0) & ok
        assert int(sub.sum()) > 0


def test_weight_rule_invariants():
    W = G.logical(64, 512, 77, amp=0.3).float()
    W[3] = 0.0
    W[4, 7] = float("inf")
    W[5, 9] = float("nan")
    W[6] = 0.0
    W[6, 1] = 3.0e38
    W[7] *= 1e-30
    W8, s = R.weight_rule(W)
    v = R.dq(W8)
    fin = torch.ones(64, dtype=torch.bool)
    fin[4] = fin[5] = False
    assert float(v[fin].abs().max()) <= 256.0
    m, e = torch.frexp(s)
    assert bool((m == 0.5).all()), "s is a power of two"
    assert float(s[3]) == 1.0 and float(s[4]) == 1.0 and float(s[5]) == 1.0 and bool((v[3] == 0).all())
    assert float(v[4, 7]) == 448.0 and bool(torch.isnan(v[5, 9])) and int(torch.isnan(v).sum()) == 1
    # W8 s within half an e4m3 ulp of W: ulp(x) = 2^(floor(log2 |x|) - 3) for a normal e4m3 (>= 2^-6), 2^-9 below
    x = (W.double() / s.double()[:, None])[fin]
    ulp = torch.where(x.abs() >= 2.0 ** -6, torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(1e-300))) - 3), torch.full_like(x, 2.0 ** -9))
    assert bool(((v[fin] - x).abs() <= ulp / 2).all())
    # a row's largest element lands in [128, 256): all of e4m3's precision is used
    rows = fin.clone()
    rows[3] = False
    assert bool((v[rows].abs().amax(1) >= 128).all())


def test_q8_clamps_and_keeps_nan():
    x = torch.tensor([500.0, -1e9, 448.0, 463.9, float("nan"), 2.0 ** -10, 2.0 ** -9, 0.0, float("inf")])
    v = R.q8v(x)
    assert v[:4].tolist() == [448.0, -448.0, 448.0, 448.0] and bool(torch.isnan(v[4]))
    assert v[5:].tolist() == [0.0, 2.0 ** -9, 0.0, 448.0]
    assert R.dq(R.truncate8(torch.tensor([1.9, -1.9, 1.0]))).tolist() == [1.875, -1.875, 1.0]


def test_accumulator_precision_does_not_decide_the_end_to_end_gate():
    from helpers import make_encoder
    from opensetgaitrecognition_pcaa_amd import synthetic as syn
    enc = make_encoder(8, 32, 4, False).eval()
    sd = enc.state_dict()
    rows = syn.synthetic_pcs(4, 30, 32, 4).reshape(-1, 4)
    f64 = R.emulate(sd, rows, 32)
    f32 = R.emulate(sd, rows, 32, acc_dtype=torch.float32)
    oracle = R.emulate(sd, rows, 32, quant=False)
    top = float(oracle.abs().max())
    d_acc, d_or = float((f64 - f32).abs().max()) / top, float((f64 - oracle).abs().max()) / top
    print(f"[fp8 gates] emulation: fp32 vs fp64 accumulators {d_acc:.2e} of the features' maximum; distance from the fp64 "
          f"oracle {d_or:.2e}")
    assert d_acc <= 1e-3 * d_or
    assert 1e-3 < d_or < 0.2


def test_abi_29_and_exports():
    with open(os.path.join(ROOT, "include", "pcaa_hip.h")) as f:
        hdr = f.read()
    declared = int(re.search(r"#define\s+PCAA_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert declared == 29
    assert re.search(r"#define\s+PCAA_FP8_E4M3\s+3\b", hdr)
    from opensetgaitrecognition_pcaa_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert lib.pcaa_abi_version() == declared == _lib.ABI_VERSION
    for name in ("pcaa_quantize_weight_fp8", "pcaa_gemm_fp8_supported", "pcaa_gemm_fp8_affine_elu"):
        assert hasattr(lib, name), name
    protos = _lib.parse_header()
    assert len(protos["pcaa_gemm_fp8_affine_elu"][1]) == 14 and len(protos["pcaa_quantize_weight_fp8"][1]) == 6
    assert lib.pcaa_gemm_fp8_supported(300, 256, R.K_MIN) == 1 and lib.pcaa_gemm_fp8_supported(300, 256, 64) == 0
    assert lib.pcaa_gemm_fp8_supported(300, 260, 512) == 0 and lib.pcaa_gemm_fp8_supported(300, 256, 192) == 0
