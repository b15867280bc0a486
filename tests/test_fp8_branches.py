"""The fp8 eval-mode PointNet kernels of csrc/gemm_fp8.hip on the GPU, branch by branch, against tests/fp8_ref.py:
pcaa_gemm_fp8_affine_elu on exact e4m3 operands (every output kind x M x K, more tiles than compute units, N = 512, padded
leading dimensions), pcaa_quantize_weight_fp8 against the weight rule bit for bit, the first layer's e4m3 output, and every
refusal with its message before any launch.  The gates are fp8_ref's; each figure is printed before it is asserted."""
import pytest
import torch

import elementwise_ref as E
import fp8_ref as R
import gemm_ref as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 0x55


def _ops():
    from opensetgaitrecognition_pcaa_amd import _lib, ops
    return _lib.load(), ops


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


CASES = R.cases(n_cu())
_BIG = {}
CODE = {"e4m3": 3, "bf16": 1, "f32": 0}
ODT = {"e4m3": torch.uint8, "bf16": torch.bfloat16, "f32": torch.float32}


def launch(lib, ops, c, bt):
    """the raw entry point into a sentinel-filled window -> (rc, got [rows, N] in the output's storage dtype)"""
    M, N, K = c["M"], c["N"], c["K"]
    rows = M // c["pool_rows"] if c["pool_rows"] else M
    ldo = c["ldo"] or N
    dt = ODT[c["out"]]
    sent = SENT if dt == torch.uint8 else 7.0
    buf = torch.full((c["off"] + rows * ldo + 4096,), sent, dtype=dt, device=DEV)
    win = buf[c["off"]:c["off"] + rows * ldo].view(rows, ldo)[:, :N]
    rc = lib.pcaa_gemm_fp8_affine_elu(bt["A"].data_ptr(), bt["A"].stride(0), bt["W"].data_ptr(), bt["W"].stride(0), win.data_ptr(),
                                      CODE[c["out"]], ldo, bt["scale8"].data_ptr(), bt["shift"].data_ptr(), M, N, K, c["pool_rows"],
                                      ops._s())
    torch.cuda.synchronize()
    got = win.clone()
    win.fill_(sent)
    assert bool((buf == sent).all()), "memory outside the output window was written"
    return rc, got


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_gemm_fp8_affine_elu(c):
    lib, ops = _ops()
    bt = R.build(c, DEV)
    acc = None
    if c["big"]:                    # the two over-CU-count cases share their operands and accumulators
        if "acc" not in _BIG:
            _BIG["acc"] = G.acc_ref(R.dq(bt["A"]), R.dq(bt["W"]), True)
            _BIG["acc"]["g_in"] = R.instr_gate(R.dq(bt["A"]), R.dq(bt["W"]))
        acc = _BIG["acc"]
    ref = R.reference(c, bt, acc=acc)
    rc, got = launch(lib, ops, c, bt)
    assert rc == 0, lib.pcaa_last_error()
    val = R.dq(got) if c["out"] == "e4m3" else got.double()
    out = R.outside(c, val, ref)
    ok = ~torch.isnan(ref["want"])
    if c["out"] != "e4m3":
        r = float(((val - ref["want"]).abs() / ref["gate"])[ok].max())
        print(f"[fp8] {c['id']}: worst |err| / gate = {r:.3f}")
    else:
        exact = float((val == R.q8v(ref["want"]))[ok].double().mean())
        print(f"[fp8] {c['id']}: {int(out.sum())} of {out.numel()} outside the interval; {exact:.6f} equal to q8(want)")
    if bool(out.any()):
        idx = out.nonzero()
        print(f"[fp8] {c['id']}: misses in rows {sorted(set(idx[:, 0].tolist()))[:12]}, columns {sorted(set(idx[:, 1].tolist()))[:12]}")
        for i, j in idx[:8].tolist():
            print(f"[fp8]   [{i}, {j}] got {float(val[i, j])!r} want {float(ref['want'][i, j])!r} gate {float(ref['gate'][i, j]):.3e}")
    assert not bool(out.any())
    if c["ldo"] is None and c["off"] == 0:          # the ops-level entry point: the same bits
        odt = {"e4m3": None, "bf16": torch.bfloat16, "f32": None}[c["out"]]
        o2 = ops.gemm_fp8_affine_elu(bt["A"].view(R.FP8), bt["W"].view(R.FP8), bt["scale8"], bt["shift"], c["pool_rows"], odt) \
            if bt["A"].is_contiguous() else None
        if o2 is not None:
            a, b = (o2.view(torch.uint8), got) if c["out"] == "e4m3" else (o2, got)
            assert torch.equal(torch.nan_to_num(a.float(), nan=-1.0), torch.nan_to_num(b.float(), nan=-1.0))


def test_c_layout_with_asymmetric_operands():
    """A = one-hot rows against an asymmetric W (W[n][k] = small integers that differ in n and k): every output element
    names its own (row, column) -- a transposed or permuted accumulator block cannot pass"""
    lib, ops = _ops()
    M, N, K = 256, 256, 128
    k_of = (torch.arange(M, device=DEV) * 5 + 3) % K
    a = torch.zeros((M, K), dtype=torch.float64, device=DEV)
    a[torch.arange(M, device=DEV), k_of] = 1.0
    w = ((torch.arange(N, device=DEV)[:, None] * 3 + torch.arange(K, device=DEV)[None, :] * 7) % 13).double()
    c = dict(M=M, N=N, K=K, pool_rows=0, out="bf16", ldo=None, off=0)
    bt = {"A": R.q8(a), "W": R.q8(w), "scale8": torch.ones(N, device=DEV), "shift": torch.zeros(N, device=DEV)}
    rc, got = launch(lib, ops, c, bt)
    assert rc == 0, lib.pcaa_last_error()
    want = E.elu(a @ w.t()).to(torch.bfloat16)
    assert torch.equal(got, want)


@pytest.mark.parametrize("shape", [(256, 512), (1024, 1024), (37, 130)])
def test_quantize_weight_fp8_is_the_rule(shape):
    _, ops = _ops()
    R_, C = shape
    W = G.logical(R_, C, 5 + R_, DEV, (3.0 / C) ** 0.5).float()
    W[2] = 0.0
    W[3] = 0.0
    W[3, C // 3] = 2.5e38
    W[4] *= 1e-20
    W8, s = ops.quantize_weight_fp8(W)
    w8, s_ref = R.weight_rule(W)
    torch.cuda.synchronize()
    bad = (s != s_ref).nonzero().flatten().tolist()
    for r in bad[:4]:
        print(f"[fp8] quantize row {r}: s {float(s[r])!r} rule {float(s_ref[r])!r} absmax {float(W[r].abs().max())!r}")
    assert torch.equal(s, s_ref)
    assert torch.equal(W8.view(torch.uint8), w8)
    assert float(s[2]) == 1.0 and 128.0 <= float(R.dq(W8)[3, C // 3]) < 256.0


@pytest.mark.parametrize("P,C,cout", [(300, 4, 512), (129, 5, 512)])
def test_pointnet_in_apply_e4m3(P, C, cout):
    _, ops = _ops()
    x = G.logical(P, C, 9, DEV, 2.0).float()
    x[7, 1] = 3000.0                                  # a point far out: outputs beyond 448 before the clamp
    W = G.logical(cout, C, 10, DEV, 1.0).float()
    scale = R.uniform(cout, 11, DEV, 0.7, 1.3).float()
    shift = R.uniform(cout, 12, DEV, -0.5, 0.5).float()
    a32 = ops.pointnet_in_apply(x, W, scale, shift, torch.float32)
    a8 = ops.pointnet_in_apply(x, W, scale, shift, R.FP8)
    torch.cuda.synchronize()
    assert a8.dtype == R.FP8 and tuple(a8.shape) == (P, cout)
    y = x.double() @ W.double().t()
    _, gate = E.bn_act_fwd_ref(y, scale, shift)
    gate = gate + 4 * E.U * C * (x.double().abs() @ W.double().abs().t()) * scale.double().abs()      # y itself: C fp32 fmas
    assert int((a32.abs() > R.E4M3_MAX).sum()) > 0
    ok = R.in_interval(a8, a32.double(), gate)
    print(f"[fp8] pointnet_in_apply e4m3 [{P}, {cout}]: {int((~ok).sum())} of {ok.numel()} outside the interval")
    assert bool(ok.all())


REFUSALS = [
    ("N must be a multiple of 256", dict(N=260)),
    ("N must be a multiple of 256", dict(K=192)),
    ("N must be a multiple of 256", dict(K=64)),
    ("16-B alignment", dict(A="+4")),
    ("16-B alignment", dict(out="+4")),
    ("16-B alignment", dict(shift="+4")),
    ("bad leading dimension", dict(lda=520)),
    ("bad leading dimension", dict(ldo=260, out_dtype=3)),
    ("pool_rows must be", dict(pool_rows=16)),
    ("bad out_dtype", dict(out_dtype=0)),
    ("bad out_dtype", dict(out_dtype=1, pool_rows=32)),
    ("M must be a multiple of pool_rows", dict(M=300, pool_rows=32, out_dtype=0)),
    ("null pointer", dict(W=None)),
    ("null pointer", dict(scale8=None)),
]


@pytest.mark.parametrize("frag,kw", REFUSALS, ids=[f"{i}-{f[:12]}" for i, (f, _) in enumerate(REFUSALS)])
def test_refused_before_any_launch(frag, kw):
    lib, ops = _ops()
    a = dict(M=256, N=256, K=512, lda=512, ldw=512, ldo=256, out_dtype=3, pool_rows=0)
    a.update({k: v for k, v in kw.items() if k in a})
    bufs = {"A": torch.zeros(512 * 1024, dtype=torch.uint8, device=DEV), "W": torch.zeros(512 * 1024, dtype=torch.uint8, device=DEV),
            "out": torch.full((512 * 1024,), SENT, dtype=torch.uint8, device=DEV), "scale8": torch.ones(1024, device=DEV),
            "shift": torch.zeros(1024, device=DEV)}
    ptrs = {k: v.data_ptr() for k, v in bufs.items()}
    for k in ptrs:
        if k in kw:
            ptrs[k] = None if kw[k] is None else ptrs[k] + 4
    rc = lib.pcaa_gemm_fp8_affine_elu(ptrs["A"], a["lda"], ptrs["W"], a["ldw"], ptrs["out"], a["out_dtype"], a["ldo"], ptrs["scale8"],
                                      ptrs["shift"], a["M"], a["N"], a["K"], a["pool_rows"], ops._s())
    msg = lib.pcaa_last_error().decode()
    torch.cuda.synchronize()
    assert rc == 1 and msg.startswith("pcaa_gemm_fp8_affine_elu:") and frag in msg, (rc, msg)
    assert bool((bufs["out"] == SENT).all()), "a refused call wrote"


def test_ops_level_refusals():
    _, ops = _ops()
    a = torch.zeros((256, 512), dtype=torch.uint8, device=DEV).view(R.FP8)
    w = torch.zeros((256, 512), dtype=torch.uint8, device=DEV).view(R.FP8)
    v = torch.ones(256, device=DEV)
    with pytest.raises(ValueError):
        ops.gemm_fp8_affine_elu(a, w, v, v, pool_rows=16)
    with pytest.raises(TypeError):
        ops.gemm_fp8_affine_elu(a, w, v, v, out_dtype=torch.float32)
    with pytest.raises(TypeError):
        ops.gemm_fp8_affine_elu(a.view(torch.uint8), w, v, v)
    assert ops.gemm_fp8_supported(300, 256, 128) and not ops.gemm_fp8_supported(300, 256, 320)
