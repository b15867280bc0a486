"""The gates of tests/eval_bwd_ref.py, checked on the CPU at the inputs tests/test_eval_bwd_branches.py uses on the GPU
(same seeds, same shapes), as tests/test_elementwise_gates_cpu.py does for the train-mode kernels:

* NOT TOO TIGHT: a float32 torch evaluation of the same expressions, in the kernel's order (row lanes per 128-row
  workgroup in fp32, workgroups in fp64), stays inside every gate; the largest fraction reached is printed.
* NOT VACUOUS: every planted defect, applied to the fp64 restatement, moves at least 80 % of the output elements it
  touches by more than 10 x the gate.

Plus, without a GPU: the library built from this tree exports the new entry points, the header declares them, and the
ABI versions agree.
"""
import ctypes
import os
import re

import pytest
import torch

import elementwise_ref as R
import eval_bwd_ref as E

F32, BF16 = torch.float32, torch.bfloat16
WORST = {}


def f32c(x):
    return torch.tensor(x, dtype=F32)


def e_of(z, fast):
    """ELU'(z) in fp32: expf, or the bf16-storage kernels' fast exponential"""
    ex = torch.exp2(torch.minimum(z, f32c(0.0)) * f32c(1.4426950408889634)) if fast else torch.exp(torch.minimum(z, f32c(0.0)))
    return torch.where(z > 0, torch.ones_like(z), ex)


def inside(name, got, want, gate):
    r = R.ratio(got, want, gate)
    key = name.split(":")[0]
    WORST[key] = max(WORST.get(key, 0.0), r)
    print(f"[eval-bwd gate cpu] {name}: fp32 evaluation worst |err| / gate = {r:.3f}")
    assert r <= 1.0, (name, r)


def defect_moves(name, want, bad, gate, mask=None):
    f = R.moved(want, bad, gate, mask)
    print(f"[eval-bwd gate cpu] {name}: moved {f:.1%}")
    assert f >= 0.8, (name, f)


def case_inputs(rows, ch, gr, dtype, pooled):
    """the inputs of one case: tests/test_eval_bwd_branches.py builds the same ones on the device"""
    seed = R.seed_of(ch, rows * 1009 + gr)
    y = R.activations(rows, ch, dtype, seed)
    sc, sh, mu, rs = R.bn_vectors(ch, seed)
    kw = ({"dpool": R.gradient(E.pooled_groups(rows, gr), ch, F32, seed), "group_rows": gr, "pool_scale": 1.0 / gr}
          if pooled else {"da": R.gradient(rows, ch, dtype, seed)})
    return y, sc, sh, mu, rs, kw


CASES = [(rows, ch) for rows in (1, 127, 129, 300) for ch in (4, 64, 512, 1024)]


@pytest.mark.parametrize("gr", [0, 1, 30, 32, 150])          # 0: the da form
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("rows,ch", CASES)
def test_eval_act_bwd_gates(rows, ch, dtype, gr):
    pooled = gr > 0
    y, sc, sh, mu, rs, kw = case_inputs(rows, ch, gr, dtype, pooled)
    ref = E.bn_eval_act_bwd_ref(y, sc, sh, mu, rs, **kw)
    fast = dtype == BF16
    if pooled:
        g = (kw["dpool"] * f32c(1.0 / gr)).repeat_interleave(gr, 0)[:rows]
    else:
        g = kw["da"].float()
    d = g * e_of(y.float() * sc + sh, fast)
    dy = sc * d
    tag = f"ch={ch} rows={rows} gr={gr} {dtype}"
    inside(f"dy: {tag}", dy, ref["dy"], ref["dy_gate"])
    if dtype == BF16:
        inside(f"dy bf16: {tag}", dy.to(BF16), ref["dy"], R.out_gate(ref["dy_gate"], ref["dy"], BF16))
    rl = 256 // (ch // 4)
    t = torch.stack([d, d * ((y.float() - mu) * rs)])
    stats = torch.zeros(2, ch, dtype=torch.float64)
    for r0 in range(0, rows, 128):
        blk = t[:, r0:r0 + 128]
        for lane in range(min(rl, blk.shape[1])):
            acc = torch.zeros(2, ch)
            for r in range(lane, blk.shape[1], rl):
                acc = acc + blk[:, r]
            stats += acc.double()
    inside(f"stats: {tag}", stats, ref["stats"], ref["stats_gate"])

    gate = R.out_gate(ref["dy_gate"], ref["dy"], dtype)
    defects = ["drop_last_row"] + (["swap_quads"] if ch >= 8 else []) + (["next_group_grad"] if pooled and rows > 2 * gr else []) \
        + (["batch_stats"] if rows >= 127 else [])
    for df in defects:
        bad = E.bn_eval_act_bwd_ref(y, sc, sh, mu, rs, defect=df, **kw)
        if df in ("swap_quads", "next_group_grad"):
            mask = R.swapped_channels(ch) if df == "swap_quads" else R.last_rows_with_next(rows, gr)
            defect_moves(f"{tag} dy {df}", ref["dy"], bad["dy"], gate, mask)
        if df == "batch_stats":
            assert torch.equal(bad["dy"], ref["dy"]) and torch.equal(bad["stats"][0], ref["stats"][0])
            defect_moves(f"{tag} dgamma {df}", ref["stats"][1], bad["stats"][1], ref["stats_gate"][1])
        elif df != "next_group_grad":
            defect_moves(f"{tag} stats {df}", ref["stats"], bad["stats"], ref["stats_gate"],
                         R.swapped_channels(ch) if df == "swap_quads" else None)


@pytest.mark.parametrize("ch", [4, 64, 512, 1024])
def test_eval_bwd_finalize_gates(ch):
    rows = 300
    y, sc, sh, mu, rs, kw = case_inputs(rows, ch, 0, F32, False)
    sums = E.bn_eval_act_bwd_ref(y, sc, sh, mu, rs, **kw)["stats"]
    stats = E.spread_stats(sums, seed=ch)
    ref = E.bn_eval_bwd_finalize_ref(stats, sc)
    s1, s2 = torch.zeros(ch, dtype=torch.float64), torch.zeros(ch, dtype=torch.float64)
    for r in range(stats.shape[0]):          # the kernel's order, in fp64, rounded once
        s1, s2 = s1 + stats[r, 0], s2 + stats[r, 1]
    got = {"dbeta": s1.float(), "dgamma": s2.float(), "dbias": (sc.double() * s1).float()}
    for k, v in got.items():
        inside(f"finalize {k}: ch={ch}", v, *ref[k])
    bad = E.bn_eval_bwd_finalize_ref(stats, sc, defect="zero_bias_grad")
    defect_moves(f"finalize ch={ch} zero_bias_grad", ref["dbias"][0], bad["dbias"][0], ref["dbias"][1])
    # the bias gradient is a real one: of the order of dbeta, not rounding noise
    assert float(ref["dbias"][0].abs().max()) > 0.5 * float(ref["dbeta"][0].abs().max())


def test_report_worst_fractions():
    """prints the largest fraction of each gate the fp32 evaluation reached in this session (pytest -s / -rP)"""
    for k in sorted(WORST):
        print(f"[eval-bwd gate cpu] largest fraction of the {k} gate reached: {WORST[k]:.3f}")
    assert all(v <= 1.0 for v in WORST.values())


# ------------------------------------------------------------------------------------------------ the C ABI, no GPU needed
NEW_ENTRY_POINTS = ("pcaa_bn_eval_act_bwd", "pcaa_bn_eval_bwd_finalize", "pcaa_bn_eval_moments")


def test_library_exports_and_header_declares_the_eval_backward():
    from opensetgaitrecognition_pcaa_amd import _lib
    protos = _lib.parse_header()
    for name in NEW_ENTRY_POINTS:
        assert name in protos, f"include/pcaa_hip.h does not declare {name}"
    ret, args = protos["pcaa_bn_eval_act_bwd"]
    assert ret is ctypes.c_int and len(args) == 16
    assert len(protos["pcaa_bn_eval_bwd_finalize"][1]) == 8
    assert os.path.exists(_lib.LIB_PATH), "libpcaa_hip.so has not been built (python -m opensetgaitrecognition_pcaa_amd.build)"
    lib = _lib.load()                         # dlopen and prototypes only: no HIP call is made
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name), f"libpcaa_hip.so does not export {name}"
    with open(_lib.HEADER) as f:
        declared = int(re.search(r"#define\s+PCAA_ABI_VERSION\s+(\d+)", f.read()).group(1))
    assert lib.pcaa_abi_version() == declared == _lib.ABI_VERSION >= 23
