"""Every launcher branch of csrc/gemm_skinny.hip against fp64, through the C ABI (references, gates, route table, cases
and planted defects: tests/skinny_ref.py; the gates themselves are shown reference-safe and defect-sensitive, and the
coverage of routes and argument checks complete, by tests/test_skinny_gates_cpu.py).

Every comparison prints ``worst |err| / gate`` with its route (``[skinny] ...``, pytest -rP) and asserts ``<= 1``
element-wise.  Operands sit in NaN-framed allocations with leading dimensions above the width; outputs and the Adam
state in sentinel-framed ones that must come back bit-identical outside the logical window.

    branch of the launcher                                              test
    ------------------------------------------------------------------  -----------------------------------------------
    pcaa_skinny_splits: every (N, K) of the cases, the four kinds       test_split_counts_match_the_library
    forward bf16 / exact / w16: the kernel's own epilogue (one chunk,   test_forward
      two, three; a ragged column group) / slabs + reduction (cps
      dividing the chunks and not), bias / none, ELU / none, ldx, ldw
    forward with nsplit chosen by the caller (2, 4, 7 of 7 chunks)      test_forward_with_split_counts_of_the_callers_choice
    the reduction's grid-stride second trip (bias, ELU)                 test_forward_reduction_takes_a_second_trip
    dgrad: dgrad2 / dgrad1 by an odd ldw / dgrad1 by a base 4 bytes     test_dgrad
      off / dgrad2_exact / dgrad2_w16; K % 256, K % 128 both ways
      (lanes with col >= K); one slab / three; a_prev, accumulate
    plain gradient f32 / exact / bf16: full / ragged row panel, odd N,  test_wgrad
      N = 1, 128 k -+ 1 (the bf16 pair store), jn = 1, 3, 4, lddw > K
    fused update bf16 / exact, JL = 1: the same shapes, ldw > K,        test_wgrad_adam
      two steps from nonzero moments
    fused update, JL = 4 and 2 with a ragged last column step           test_wgrad_adam_wide_waves
    gathered rows: MC = 1, 2, 4, 8 full and ragged, rows_alloc at and   test_wgrad_adam_rows
      above 64 MC, x rows behind M = 1e30
    gathered rows at JL = 4 and 2, MC = 1, 2, 4, 8                      test_wgrad_adam_rows_wide_waves
    pack_rows_t16: rows 1 .. 64, strided sources, bitwise               test_pack_rows_t16
    packed update: chunks 1 .. 8 (NB = 2 / 4), chunk_stride at and      test_wgrad_adam_t16
      above (N + K) 64, NaN chunk behind the last
    packed update at JL = 4 and 2: the 384-tile rule (chunks >= 4)      test_wgrad_adam_t16_wide_waves
      and the 1024-tile one (chunks = 2)
    the dynamic-LDS limit raised, then left alone                       test_wgrad_adam_t16_lds_limit_is_raised_once
    the first step (zero moments) of each fused kernel                  test_fused_update_first_step_from_zero_moments
    every reachable PCAA_CHECK_ARG: PCAA_ERR_INVALID_ARG, its message,  test_refusals
      every buffer bit-identical
"""
import pytest
import torch

import skinny_ref as R
from opensetgaitrecognition_pcaa_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
CASES = R.cases()
HP = R.HP

FN = {("fwd", "bf16"): "pcaa_skinny_linear_fwd", ("fwd", "exact"): "pcaa_skinny_linear_fwd_exact",
      ("fwd", "w16"): "pcaa_skinny_linear_fwd_w16", ("dgrad", "bf16"): "pcaa_skinny_linear_dgrad",
      ("dgrad", "exact"): "pcaa_skinny_linear_dgrad_exact", ("dgrad", "w16"): "pcaa_skinny_linear_dgrad_w16",
      ("wgrad", "f32"): "pcaa_skinny_linear_wgrad", ("wgrad", "exact"): "pcaa_skinny_linear_wgrad_exact",
      ("wgrad", "bf16"): "pcaa_skinny_linear_wgrad_bf16", ("adam", "bf16"): "pcaa_skinny_linear_wgrad_adam",
      ("adam", "exact"): "pcaa_skinny_linear_wgrad_adam_exact", ("rows", "bf16"): "pcaa_skinny_linear_wgrad_adam_rows",
      ("t16", "bf16"): "pcaa_skinny_linear_wgrad_adam_t16"}


def fn(entry, variant):
    return getattr(_lib.load(), FN[(entry, variant)])


def stream():
    return torch.cuda.current_stream().cuda_stream


def check(name, got, want, gate, worst):
    err = (got.double() - want).abs() / gate.clamp_min(1e-300)
    r = float(err.max())
    worst[name] = max(worst.get(name, 0.0), r)
    if not r <= 1.0:
        at = [int(i) for i in torch.unravel_index(err.argmax(), err.shape)]
        over = (~(err <= 1.0)).nonzero()
        print(f"[skinny] {name}: worst at {at}; {over.shape[0]} of {err.numel()} over the gate, first {over[:8].tolist()}")
    assert r <= 1.0, (name, r)


def report(worst):
    for k in sorted(worst):
        print(f"[skinny] {k}: worst |err| / gate = {worst[k]:.3f}")


def pick(entry, **kw):
    return [c for c in CASES if c["entry"] == entry and all(c.get(k) == v for k, v in kw.items())]


# ===================================================================================================== split counts
def test_split_counts_match_the_library():
    lib = _lib.load()
    shapes = {(c["N"], c["K"]) for c in CASES if c["entry"] in ("fwd", "dgrad")} | {(15360, 7680), (7680, 15360), (960, 64)}
    for N, K in sorted(shapes):
        for kind in range(4):
            assert lib.pcaa_skinny_splits(kind, 64, N, K) == R.splits(kind, N, K), (kind, N, K)


# ===================================================================================================== forward
def run_forward(c, worst):
    M, N, K = c["M"], c["N"], c["K"]
    bt = R.build(c, DEV)
    ns = R.case_nsplit(c)
    if c["nsplit"] is None:
        assert _lib.load().pcaa_skinny_splits(2 if c["variant"] == "exact" else 0, M, N, K) == ns
    ws = torch.full((ns * M * N,), R.NAN, dtype=F32, device=DEV)
    y, x, W, bias = bt["y"], bt["x"], bt["W"], bt["bias"]
    before = y.snapshot()
    rc = fn("fwd", c["variant"])(x.ptr(), x.ld, W.ptr(), W.ld, None if bias is None else bias.data_ptr(), c["act"], y.ptr(),
                                 ws.data_ptr(), ws.numel(), M, N, K, ns, stream())
    _lib.check(rc, R.case_id(c))
    ref = R.reference(c, bt)
    check(R.case_route(c), y.win, ref["want"], ref["gate"], worst)
    assert y.intact(before), R.case_id(c)


@pytest.mark.parametrize("N,K", R.FWD_NK)
@pytest.mark.parametrize("variant", R.FWD_VARIANTS)
def test_forward(variant, N, K):
    worst = {}
    for c in pick("fwd", variant=variant, N=N, K=K, nsplit=None):
        run_forward(c, worst)
    report(worst)


def test_forward_with_split_counts_of_the_callers_choice():
    """nsplit is the caller's: every count that leaves no split empty is served (7 chunks as 4 + 3, 2 + 2 + 2 + 1, 7 x 1)"""
    worst = {}
    for ns in R.FWD_CALLER_SPLITS:
        (c,) = pick("fwd", N=320, K=448, nsplit=ns)
        run_forward(c, worst)
    report(worst)


def test_forward_reduction_takes_a_second_trip():
    """M N / 4 quads above the reduction's 4096 x 256-thread grid: the last 4096 outputs come from the loop's second trip,
    with their bias column (q % qpr) and the ELU.  (Forward with two chunks and nsplit = 2: one chunk admits one split,
    and one split has no reduction launch.)"""
    M, N, K, ns = R.BIG_REDUCE
    assert M * N // 4 > R.REDUCE_QUADS
    worst = {}
    for c in pick("fwd", N=N, K=K):
        run_forward(c, worst)
    report(worst)


# ===================================================================================================== dgrad
def run_dgrad(c, worst):
    M, N, K = c["M"], c["N"], c["K"]
    bt = R.build(c, DEV)
    ns = R.case_nsplit(c)
    assert _lib.load().pcaa_skinny_splits(3 if c["variant"] == "exact" else 1, M, N, K) == ns
    ws = torch.full((ns * M * K,), R.NAN, dtype=F32, device=DEV)
    dz, W, dx, ap = bt["dz"], bt["W"], bt["dx"], bt["a_prev"]
    before = dx.snapshot()
    rc = fn("dgrad", c["variant"])(dz.ptr(), dz.ld, W.ptr(), W.ld, dx.ptr(), None if ap is None else ap.data_ptr(),
                                   int(c["accumulate"]), ws.data_ptr(), ws.numel(), M, N, K, ns, stream())
    _lib.check(rc, R.case_id(c))
    ref = R.reference(c, bt)
    check(R.case_route(c), dx.win, ref["want"], ref["gate"], worst)
    assert dx.intact(before), R.case_id(c)


@pytest.mark.parametrize("K", R.DGRAD_K)
@pytest.mark.parametrize("form", R.DGRAD_FORMS)
def test_dgrad(form, K):
    worst = {}
    want = {"dgrad2": "dgrad2", "dgrad1_ld": "dgrad1", "dgrad1_off": "dgrad1", "dgrad2_exact": "dgrad2_exact", "dgrad2_w16": "dgrad2_w16"}
    for c in pick("dgrad", form=form, K=K):
        assert R.case_route(c) == want[form]
        run_dgrad(c, worst)
    report(worst)


# ===================================================================================================== plain gradient
@pytest.mark.parametrize("K", R.WG_K)
@pytest.mark.parametrize("variant", R.WG_VARIANTS)
def test_wgrad(variant, K):
    worst = {}
    odt = BF16 if variant == "bf16" else F32
    for c in pick("wgrad", variant=variant, K=K):
        M, N = c["M"], c["N"]
        bt = R.build(c, DEV)
        dW = R.Framed(torch.full((N, K), R.SENTINEL["dW"], dtype=odt, device=DEV), K + (6 if variant == "bf16" else 3),
                      fill=R.SENTINEL["dW"])
        before = dW.snapshot()
        dz, x = bt["dz"], bt["x"]
        _lib.check(fn("wgrad", variant)(dz.ptr(), dz.ld, x.ptr(), x.ld, dW.ptr(), dW.ld, M, N, K, stream()), R.case_id(c))
        ref = R.reference(c, bt)
        check(R.case_route(c), dW.win, ref["want"], ref["gate"], worst)
        assert dW.intact(before), R.case_id(c)
    report(worst)


# ===================================================================================================== fused updates
def run_update(c, worst, rows_extra=0, cs_pad=64, ldw_pad=3, frames=None, steps=None):
    """one or two steps of a fused-update case: every step from the fp32 state the kernel left, against the fp64 update
    of that state with the fp64 gradient; W / exp_avg / exp_avg_sq bit-identical outside [N, K]"""
    e, M, N, K = c["entry"], c["M"], c["N"], c["K"]
    JL, NB = R.ring_of(c)
    frames = frames or R.state(c, DEV, ldw=K + ldw_pad)
    step_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    coef_dev = torch.zeros(2, dtype=F32, device=DEV)
    hp = (HP["b1"], HP["b2"], HP["eps"], HP["gs"])
    route = R.case_route(c)
    steps = steps or ((1,) if c["zero"] else (1, 2))
    step_dev.fill_(steps[0] - 1)
    for step in steps:
        ops.adam_advance_(step_dev, coef_dev, HP["lr"], HP["b1"], HP["b2"])
        coef = coef_dev.tolist()
        bt = R.build(dict(c, rows_extra=rows_extra), DEV, step=step)
        snaps = [f.snapshot() for f in frames]
        p, m, v = (f.win.clone() for f in frames)
        Wf, mf, vf = frames
        P, cs = None, (N + K) * 64 + cs_pad
        if e == "t16":
            P = R.packed(c, bt, N, cs, DEV)
            rc = fn(e, "bf16")(P.data_ptr(), cs, c["chunks"], Wf.ptr(), mf.ptr(), vf.ptr(), Wf.ld, N, K, *hp, coef_dev.data_ptr(),
                               stream())
        else:
            dz, x = bt["dz"], bt["x"]
            tail = (x.r, stream()) if e == "rows" else (stream(),)
            rc = fn(e, c["variant"])(dz.ptr(), dz.ld, x.ptr(), x.ld, Wf.ptr(), mf.ptr(), vf.ptr(), Wf.ld, M, N, K, *hp,
                                     coef_dev.data_ptr(), *tail)
        _lib.check(rc, R.case_id(c))
        ref = R.wgrad_adam_ref(R.gradient(c, bt, P=P, chunk_stride=cs), p, m, v, step, coef, JL, NB)
        for name, f in zip("pmv", frames):
            check(f"{route} {name}", f.win, *ref[name], worst)
        for f, s in zip(frames, snaps):
            assert f.intact(s), (R.case_id(c), step)
        del ref, bt, snaps, P
    return frames


@pytest.mark.parametrize("K", R.WG_K)
@pytest.mark.parametrize("variant", R.ADAM_VARIANTS)
def test_wgrad_adam(variant, K):
    worst = {}
    for c in pick("adam", variant=variant, K=K, zero=False):
        if (c["N"], K) not in R.WIDE_JL:
            assert R.ring_of(c) == (1, 2)
            run_update(c, worst)
    report(worst)


@pytest.mark.parametrize("N,K", list(R.WIDE_JL))
@pytest.mark.parametrize("variant", R.ADAM_VARIANTS)
def test_wgrad_adam_wide_waves(variant, N, K):
    """JL = 4 at K = 160 (wave 0: four column steps, wave 1: one, waves 2 - 3: none) and JL = 2 at K = 288 (the fifth
    wave: one step); N = 128 k and 128 k - 122 (6 live rows in the last panel)"""
    worst = {}
    (c,) = pick("adam", variant=variant, N=N, K=K)
    assert R.ring_of(c) == (R.WIDE_JL[(N, K)], 2)
    run_update(c, worst, ldw_pad=0)
    report(worst)


@pytest.mark.parametrize("N,K", R.ROWS_NK)
def test_wgrad_adam_rows(N, K):
    worst = {}
    for i, c in enumerate(pick("rows", N=N, K=K, zero=False)):
        assert R.ring_of(c) == (1, 2)
        run_update(c, worst, rows_extra=64 * (i & 1))
    assert {k.split("/")[1] for k in worst} == {"MC1", "MC2", "MC4", "MC8"}
    report(worst)


@pytest.mark.parametrize("N,K", list(R.WIDE_JL))
def test_wgrad_adam_rows_wide_waves(N, K):
    worst = {}
    for c in pick("rows", N=N, K=K):
        assert R.ring_of(c) == (R.WIDE_JL[(N, K)], 2)
        run_update(c, worst, ldw_pad=0)
    assert {k.split("/")[1] for k in worst} == {"MC1", "MC2", "MC4", "MC8"}
    report(worst)


@pytest.mark.parametrize("rows", R.PACK_ROWS)
def test_pack_rows_t16(rows):
    for N, K in R.ROWS_NK:
        bt = R.build(dict(entry="pack", M=rows, N=N, K=K), DEV)
        out = R.Framed(torch.full((N + K, 64), R.SENTINEL["P"], dtype=BF16, device=DEV), fill=R.SENTINEL["P"])
        before = out.snapshot()
        dz, x = bt["dz"], bt["x"]
        _lib.check(_lib.load().pcaa_pack_rows_t16(dz.ptr(), dz.ld, N, x.ptr(), x.ld, K, rows, out.ptr(), stream()), "pack")
        assert torch.equal(out.win, R.pack_ref(dz.win, x.win, rows)), (rows, N, K)
        assert out.intact(before)
        assert _lib.load().pcaa_packed_chunk_elems(N, K) == (N + K) * 64


@pytest.mark.parametrize("N,K", R.ROWS_NK)
def test_wgrad_adam_t16(N, K):
    worst = {}
    for i, c in enumerate(pick("t16", N=N, K=K, zero=False)):
        assert R.ring_of(c) == (1, 4 if c["chunks"] >= 4 else 2)
        run_update(c, worst, cs_pad=64 * (i & 1))
    assert {k.split("/")[1] for k in worst} == {"NB2", "NB4"}
    report(worst)


@pytest.mark.parametrize("N,K,chunks", [(N, K, 4) for N, K in R.T16_DEEP_JL] + [(N, K, 2) for N, K in R.WIDE_JL])
def test_wgrad_adam_t16_wide_waves(N, K, chunks):
    worst = {}
    (c,) = pick("t16", N=N, K=K, chunks=chunks)
    jl = R.T16_DEEP_JL[(N, K)] if chunks >= 4 else R.WIDE_JL[(N, K)]
    assert R.ring_of(c) == (jl, 4 if chunks >= 4 else 2)
    run_update(c, worst, ldw_pad=0)
    report(worst)


def test_wgrad_adam_t16_lds_limit_is_raised_once():
    """the dynamic dz panel of one instantiation grows, then shrinks: the limit is raised for the larger panel and left
    alone for the smaller.  Ring of 2 (chunks < 4): 1, 3, 1 chunks; ring of 4: 4, 8, 4.  (1, 8, 1 would be two
    instantiations: the ring depth is a template argument chosen by the chunk count.)"""
    worst = {}
    for seq in ((1, 3, 1), (4, 8, 4)):
        frames = None
        for i, ch in enumerate(seq):
            c = dict(entry="t16", variant="bf16", chunks=ch, M=37, N=130, K=96, zero=False)
            frames = run_update(c, worst, frames=frames, steps=(i + 1,))
    report(worst)


@pytest.mark.parametrize("entry", ["adam", "rows", "t16"])
def test_fused_update_first_step_from_zero_moments(entry):
    worst = {}
    cs = pick(entry, zero=True)
    assert len(cs) == (2 if entry == "adam" else 1)
    for c in cs:
        run_update(c, worst)
    report(worst)


# ===================================================================================================== refusals
VALID = {
    "fwd": dict(x="a", ldx=256, W="b", ldw=256, bias="c", act=1, y="o", ws="w", ws_floats=8 * 128 * 4, M=8, N=128, K=256, nsplit=1),
    "dgrad": dict(dz="a", lddz=256, W="b", ldw=128, dx="o", a_prev="c", accumulate=0, ws="w", ws_floats=8 * 128 * 4, M=8, N=256,
                  K=128, nsplit=1),
    "wgrad": dict(dz="a", lddz=256, x="b", ldx=128, dW="o", lddw=128, M=8, N=256, K=128),
    "adam": dict(dz="a", lddz=256, x="b", ldx=128, W="o", m="p", v="q", ldw=128, M=8, N=256, K=128, b1=0.9, b2=0.99, eps=1e-8,
                 gs=1.0, coef="c"),
    "pack": dict(dz="a", lddz=256, N=256, x="b", ldx=128, K=128, rows=8, chunk="o"),
    "t16": dict(P="a", cs=(256 + 128) * 64, chunks=1, W="o", m="p", v="q", ldw=128, N=256, K=128, b1=0.9, b2=0.99, eps=1e-8,
                gs=1.0, coef="c"),
}
VALID["rows"] = dict(VALID["adam"], rows_alloc=64)
ENTRY = {"fwd": ("fwd", "pcaa_skinny_linear_fwd"), "fwd_exact": ("fwd", "pcaa_skinny_linear_fwd_exact"),
         "fwd_w16": ("fwd", "pcaa_skinny_linear_fwd_w16"), "dgrad": ("dgrad", "pcaa_skinny_linear_dgrad"),
         "dgrad_exact": ("dgrad", "pcaa_skinny_linear_dgrad_exact"), "dgrad_w16": ("dgrad", "pcaa_skinny_linear_dgrad_w16"),
         "wgrad": ("wgrad", "pcaa_skinny_linear_wgrad"), "wgrad_exact": ("wgrad", "pcaa_skinny_linear_wgrad_exact"),
         "wgrad_bf16": ("wgrad", "pcaa_skinny_linear_wgrad_bf16"), "adam": ("adam", "pcaa_skinny_linear_wgrad_adam"),
         "adam_exact": ("adam", "pcaa_skinny_linear_wgrad_adam_exact"), "rows": ("rows", "pcaa_skinny_linear_wgrad_adam_rows"),
         "pack": ("pack", "pcaa_pack_rows_t16"), "t16": ("t16", "pcaa_skinny_linear_wgrad_adam_t16")}
# the name a weight-gradient entry point's "%s:" messages carry (the exact forms share their bf16 sibling's)
WG_NAME = {"wgrad": "pcaa_skinny_linear_wgrad:", "wgrad_exact": "pcaa_skinny_linear_wgrad:", "wgrad_bf16": "pcaa_skinny_linear_wgrad_bf16:",
           "adam": "pcaa_skinny_linear_wgrad_adam:", "adam_exact": "pcaa_skinny_linear_wgrad_adam:",
           "rows": "pcaa_skinny_linear_wgrad_adam_rows:"}


def refusal_args(key, over, ptr):
    """the argument tuple of a valid call of entry point ``key`` with ``over`` applied; ptr: buffer letter -> address"""
    args = dict(VALID[ENTRY[key][0]])
    args.update(over)
    out = []
    for k, v in args.items():
        if isinstance(v, str):
            v = None if v == "NULL" else ptr[VALID[ENTRY[key][0]][k]] + int(v[1:]) if v.startswith("+") else ptr[v]
        out.append(v)
    return out


def test_refusals():
    """every reachable PCAA_CHECK_ARG: PCAA_ERR_INVALID_ARG, the check's message under the entry point's name, and no
    buffer touched.  The checks run before any launch: the 32-bit-offset refusals pass leading dimensions only, nothing
    of that size is allocated."""
    lib = _lib.load()
    bufs = {k: torch.full((64 * 512,), 1.0 + i, dtype=F32, device=DEV) for i, k in enumerate("abcopqw")}
    ptr = {k: t.data_ptr() for k, t in bufs.items()}
    before = {k: t.clone() for k, t in bufs.items()}
    for key, prefix, frag, over in R.REFUSALS:
        rc = getattr(lib, ENTRY[key][1])(*refusal_args(key, over, ptr), stream())
        msg = lib.pcaa_last_error().decode()
        assert rc == 1, (key, over, rc, msg)
        assert msg.startswith(WG_NAME[key] if prefix == "%s:" else prefix) and frag in msg, (key, over, msg)
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert torch.equal(t, before[k]), k
    # the valid calls themselves are accepted (the overrides above are what is refused)
    for key in ("fwd", "dgrad", "wgrad", "adam", "rows", "pack", "t16"):
        assert getattr(lib, ENTRY[key][1])(*refusal_args(key, {}, ptr), stream()) == 0, (key, lib.pcaa_last_error())
    torch.cuda.synchronize()
