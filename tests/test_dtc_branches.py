"""Every dispatch branch of csrc/dtc_fused.hip against the fp64 restatements of tests/dtc_ref.py, on the GPU.

Operands live inside NaN-filled allocations (32 rows of their own width in front and behind), every output -- y / out, the slabs with the gap
between them, col, dy_out, the fp64 statistics -- inside a sentinel-filled one that must come back bit-identical outside the
logical window.  The library is asked for its route first (pcaa_dtc_conv_route) and must name the kernel the case means to
reach; then |got - want| <= gate for every element of every output (the gates: module docstring of tests/dtc_ref.py, checked
on the CPU by tests/test_dtc_gates_cpu.py).  The calls go through ctypes on the C ABI: ops.dtc_conv_fwd / dtc_conv_dgrad
allocate their own outputs (no sentinel can surround them) and choose ksplit, slab_stride and nrep themselves; they are what
test_carried_finalize drives.

  test                         entry points                                         branches
  ---------------------------  ---------------------------------------------------  -----------------------------------------
  test_forward[case-dtype]     pcaa_dtc_conv_fwd, _fwd_bf16, pcaa_splitk_reduce      dtc_fwd_one_kernel<false>, <true> (second
                                                                                    128-column workgroup with one live wave,
                                                                                    ragged chunk, ragged column tile, T = 1,
                                                                                    T = 32, d >= T, 2d >= T), dtc_pair_kernel
                                                                                    <fwd, f32|bf16, 32|64> (odd batch, per-quad
                                                                                    reload, second staging pass, the wide
                                                                                    boundary from both sides), ksplit > 1 (empty
                                                                                    splits, one chunk per split, uneven, stride
                                                                                    > slab, col under a split), nrep 1 and > B
  test_adjoint[case-dtype]     pcaa_dtc_conv_dgrad, _dgrad_bf16, pcaa_splitk_reduce  dtc_dgrad_one_kernel<false>, <true>,
                                                                                    dtc_pair_kernel<adj, ...>; dy given / formed /
                                                                                    + dy_out / + epilogue and its statistics;
                                                                                    ksplit > 1 with dy_out slices per split
  test_windowed[case-dtype]    pcaa_dtc_conv_fwd_win(_bf16), _fwd_seg(_bf16)         dtc_src_row0 / dtc_src_row: plain table, ring
                                                                                    == T, ring > T (start at ring - 1 and 0),
                                                                                    segmented; a pair shape kept on the one-
                                                                                    sequence kernels; the library's own ksplit
  test_refusals[reason]        all of the above                                     every PCAA_CHECK_ARG of the file
  test_carried_finalize        ops.dtc_conv_fwd / ops.dtc_conv_dgrad + BnTail*       bn_tail_run of the four kernel families
  test_pair_switch_in_a_child  PCAA_DTC_PAIR = 0 | fwd | adj                         pair_takes' switch; the one-sequence kernels at
                                                                                    the pair widths with statistics and col
  test_supported_and_ksplit    pcaa_dtc_conv_supported, _ksplit, _dgrad_ksplit      both sides of every boundary; every returned
                                                                                    ksplit launched

The pad of the bf16 one-sequence kernels' staged rows (cvt8 reads it when the width is 4 mod 8): the cases of width 36 are
preceded by one launch of the same entry point on all-NaN operands, 256 channels wide and four sequences per CU, which
leaves NaN bit patterns in the LDS the next launch is given.  That is best effort -- nothing can force uninitialised LDS to
hold a NaN -- and the fix (one zero quad per staged row) rests on reading the kernels, not on this step.  (On an MI355X
the build without the pad stores failed 8 of these 9 bf16 cases with NaN outputs: docs/LAB_LOG.md.)

test_supported_and_ksplit_predicates launches every supported (B, cin, cout) of its grid with the library's own ksplit, both
dtypes, forward and adjoint, and checks that the call is accepted; the values are compared on a sample of nine shapes.

Not covered: B*T*cout beyond 2^31 (the index arithmetic is long, no case allocates that much); the hipFuncSetAttribute
failure paths; PCAA_DTC_TRACE builds; nc % 4 != 0 and nc % 64 != 0 at >= 192 workgroups in pair_takes / wide (no valid call
of this size reaches them: the predicate grid of the CPU file does); the unfused pcaa_dtc_im2col / pcaa_dtc_col2im.
"""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dtc_ref as D  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
_E = os.environ.get("PCAA_DTC_PAIR")
SWITCH = "both" if _E is None else {"0": "0", "f": "fwd", "a": "adj"}.get(_E[:1], "both")
WORST = {}          # route name -> {output: worst |err| / gate}
PAD_ROWS = 32       # guard rows on either side: a whole missing sequence (T <= 32), and more than 2 d rows in front


def pad_of(width):
    return max(64, PAD_ROWS * width)


def lib():
    from opensetgaitrecognition_pcaa_amd import _lib
    return _lib.load()


def ptr(t, byte_off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + byte_off)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def nan_op(t):
    """an operand inside a NaN-filled allocation, PAD_ROWS rows of its own width in front and behind -> the window"""
    if t is None:
        return None
    pad = pad_of(t.shape[-1])
    buf = torch.full((pad + t.numel() + pad,), float("nan"), dtype=t.dtype, device=DEV)
    win = buf[pad:pad + t.numel()].view(t.shape)
    win.copy_(t)
    return win


class Out:
    """n elements (rows of ``width``) inside a sentinel-filled allocation, PAD_ROWS rows in front and behind; ``keep``: the
    (offset, length) windows the call may write"""

    def __init__(self, n, width=1, dtype=torch.float32, zero=False, keep=None):
        self.n, self.keep, self.pad = n, keep or [(0, n)], pad_of(width)
        self.buf = torch.full((self.pad + n + self.pad,), D.SENTINEL, dtype=dtype, device=DEV)
        self.win = self.buf[self.pad:self.pad + n]
        if zero:
            for o, l in self.keep:
                self.win[o:o + l] = 0
        self.before = self.buf.clone()

    def check(self, what):
        mask = torch.ones_like(self.buf, dtype=torch.bool)
        for o, l in self.keep:
            mask[self.pad + o:self.pad + o + l] = False
        a, b = self.buf[mask], self.before[mask]
        assert torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int64),
                           b.view(torch.int32 if b.dtype == torch.float32 else torch.int64)), f"{what}: a store outside the logical window"

    def untouched(self):
        return torch.equal(self.buf, self.before)


def dev_inputs(c):
    return {k: nan_op(v.to(DEV)) for k, v in D.inputs(c).items()}, {k: v.to(DEV) for k, v in D.inputs(c).items()}


def expect_route(c, bf16):
    L = lib()
    got = L.pcaa_dtc_conv_route(int(c["adj"]), int(bf16), c["B"], c["cin"], c["cout"], c["ks"], int(c.get("win") is not None))
    want = D.route(c["adj"], bf16, c["B"], c["cin"], c["cout"], c["ks"], c.get("win") is not None, SWITCH)
    assert got == want, (c["id"], D.ROUTES[got], D.ROUTES[want])
    if SWITCH == "both":
        assert D.ROUTES[got] == f"{c['fam']}_{'bf16' if bf16 else 'f32'}", (c["id"], D.ROUTES[got])
    return D.ROUTES[got]


def poison(c, bf16):
    """best effort (module docstring): NaN bit patterns into the LDS of every CU, through the same entry point"""
    if not (c["poison"] and bf16):
        return
    L = lib()
    B, T = 4 * torch.cuda.get_device_properties(0).multi_processor_count, 32
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    if c["adj"]:
        dy, W, out = nan(B * T, 256), nan(256, 12), torch.empty(B * T, 4, device=DEV)
        rc = L.pcaa_dtc_conv_dgrad_bf16(ptr(dy), None, None, None, None, ptr(W), ptr(out), None, None, None, None, None, None, 1,
                                        B, T, 4, 256, 1, 1, 0, stream())
    else:
        src, W, y = nan(B * T, 256), nan(16, 768), torch.empty(B * T, 16, device=DEV)
        if c.get("win"):
            rows = torch.arange(B, dtype=torch.int32, device=DEV) * T
            rc = L.pcaa_dtc_conv_fwd_win_bf16(ptr(src), None, None, ptr(W), ptr(y), None, None, 1, B, T, 256, 16, 1, 1, 0, ptr(rows), B * T, 0, stream())
        else:
            rc = L.pcaa_dtc_conv_fwd_bf16(ptr(src), None, None, ptr(W), ptr(y), None, None, 1, B, T, 256, 16, 1, 1, 0, stream())
    assert rc == 0, L.pcaa_last_error()


def slab_out(rows, width, ks, pad):
    slab = rows * width
    stride = slab + pad if ks > 1 else 0
    return Out((ks - 1) * stride + slab, width, keep=[(z * stride, slab) for z in range(ks)]), slab, stride


def reduce_slabs(o, ks, stride, slab, rows, width, got, name):
    L = lib()
    red = Out(slab, width)
    assert L.pcaa_splitk_reduce(ptr(o.win), ks, stride, slab, ptr(red.win), 0, stream()) == 0, L.pcaa_last_error()
    torch.cuda.synchronize()
    red.check("reduced " + name)
    for z in range(ks):
        got[f"slab{z}"] = o.win[z * stride:z * stride + slab].view(rows, width)
    got[name] = red.win.view(rows, width)


def run_fwd(c, dv, bf16, table=None, win=None):
    """-> {output: tensor}; ``win``: (kind, win_row tensor, table_rows, ring, seg) for the windowed entry points"""
    L = lib()
    B, T, cin, cout, d, ks, nrep = c["B"], c["T"], c["cin"], c["cout"], c["d"], c["ks"], c["nrep"]
    rows = B * T
    y, slab, stride = slab_out(rows, cout, ks, c["stride_pad"])
    col = Out(rows * cin * 3, cin * 3) if c["col"] else None
    st = Out(nrep * 2 * cout, cout, torch.float64, zero=True) if c["stats"] else None
    src = dv["src"] if table is None else table
    head = (ptr(src), ptr(dv.get("scale")), ptr(dv.get("shift")), ptr(dv["W"]), ptr(y.win))
    shape = (B, T, cin, cout, d, ks, stride)
    sfx = "_bf16" if bf16 else ""
    if win is None:
        rc = getattr(L, "pcaa_dtc_conv_fwd" + sfx)(*head, ptr(col.win) if col else None, ptr(st.win) if st else None, nrep, *shape, stream())
    elif not win["seg"]:
        rc = getattr(L, "pcaa_dtc_conv_fwd_win" + sfx)(*head, None, None, nrep, *shape, ptr(win["dev"]), win["table_rows"], win["ring"], stream())
    else:
        rc = getattr(L, "pcaa_dtc_conv_fwd_seg" + sfx)(*head, *shape, ptr(win["dev"]), win["seg"], win["ring"], stream())
    assert rc == 0, L.pcaa_last_error()
    torch.cuda.synchronize()
    got = {}
    if ks == 1:
        got["y"] = y.win.view(rows, cout)
    else:
        reduce_slabs(y, ks, stride, slab, rows, cout, got, "y")
    y.check("y")
    if col:
        col.check("col")
        got["col"] = col.win.view(rows, cin * 3)
    if st:
        st.check("stats")
        got["stats"] = st.win.view(nrep, 2, cout)
        got["stats_sum"] = got["stats"].sum(0)
    return got


def run_adj(c, dv, bf16):
    L = lib()
    B, T, cin, cout, d, ks, nrep, form = c["B"], c["T"], c["cin"], c["cout"], c["d"], c["ks"], c["nrep"], c["form"]
    rows = B * T
    out, slab, stride = slab_out(rows, cin, ks, c["stride_pad"])
    dyo = Out(rows * cout, cout) if form >= 2 else None
    st = Out(nrep * 2 * cin, cin, torch.float64, zero=True) if form == 3 else None
    ep = [ptr(dv.get(k)) for k in ("ep_y", "ep_scale", "ep_shift", "ep_mean", "ep_rstd")]
    fn = L.pcaa_dtc_conv_dgrad_bf16 if bf16 else L.pcaa_dtc_conv_dgrad
    rc = fn(ptr(dv.get("dy")), ptr(dv.get("dz")), ptr(dv.get("y")), ptr(dv.get("coef")), ptr(dyo.win) if dyo else None, ptr(dv["W"]),
            ptr(out.win), *ep, ptr(st.win) if st else None, nrep, B, T, cin, cout, d, ks, stride, stream())
    assert rc == 0, L.pcaa_last_error()
    torch.cuda.synchronize()
    got = {}
    if ks == 1:
        got["out"] = out.win.view(rows, cin)
    else:
        reduce_slabs(out, ks, stride, slab, rows, cin, got, "out")
    out.check("out")
    if dyo:
        dyo.check("dy_out")
        got["dy_out"] = dyo.win.view(rows, cout)
    if st:
        st.check("ep_stats")
        got["stats"] = st.win.view(nrep, 2, cin)
        got["stats_sum"] = got["stats"].sum(0)
    return got


def compare(c, route_name, got, ref):
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    w = WORST.setdefault(route_name, {})
    bad = {}
    for name, (want, gate) in ref.items():
        r = D.ratio(got[name], want, gate)
        key = "slab" if name.startswith("slab") else name
        if not r <= w.get(key, 0.0):
            w[key] = r
        if not r <= 1.0:
            bad[name] = r
    line = ", ".join(f"{k} {v:.3f}" for k, v in sorted(w.items()))
    print(f"[dtc] {c['id']}: route {route_name}; worst |err| / gate of the route so far: {line}")
    assert not bad, (c["id"], route_name, bad)


def ids(cases):
    return [pytest.param(c, bf16, id=f"{c['id']}-{'bf16' if bf16 else 'f32'}") for c in cases for bf16 in (False, True)]


def one_case(c, bf16):
    r = expect_route(c, bf16)
    dv, raw = dev_inputs(c)
    ref = D.reference(c, raw, bf16, switch=SWITCH)
    poison(c, bf16)
    got = run_adj(c, dv, bf16) if c["adj"] else run_fwd(c, dv, bf16)
    compare(c, r, got, ref)
    return r


@pytest.mark.parametrize("c,bf16", ids(D.fwd_cases()))
def test_forward(c, bf16):
    if c.get("lib_ks"):
        assert lib().pcaa_dtc_conv_ksplit(c["B"], c["cin"], c["cout"]) == c["ks"]
    one_case(c, bf16)


@pytest.mark.parametrize("c,bf16", ids(D.adj_cases()))
def test_adjoint(c, bf16):
    if c.get("lib_ks"):
        assert lib().pcaa_dtc_conv_dgrad_ksplit(c["B"], c["cin"], c["cout"]) == c["ks"]
    one_case(c, bf16)


@pytest.mark.parametrize("c,bf16", ids(D.window_cases()))
def test_windowed(c, bf16):
    assert lib().pcaa_dtc_conv_ksplit(c["B"], c["cin"], c["cout"]) == c["ks"]
    r = expect_route(c, bf16)
    assert r == ("one_bf16" if bf16 else "one_f32")
    dv, raw = dev_inputs(c)
    w = dict(c["win"], dev=torch.tensor(c["win"]["rows"], dtype=torch.int32, device=DEV))
    ref = D.reference(c, raw, bf16)
    if w["ring"] and not w["seg"]:
        dv["src"][w["ring"]:] = float("nan")          # table rows behind the ring are never read
    poison(c, bf16)
    got = run_fwd(c, dv, bf16, win=w)
    compare(c, r + " (windowed)", got, ref)
    # the same entry point on the materialised windows: same values staged, same instruction sequence
    mat = nan_op(D.materialise(c, raw))
    ident = dict(kind="plain", seg=0, ring=0, table_rows=c["B"] * c["T"],
                 dev=torch.arange(c["B"], dtype=torch.int32, device=DEV) * c["T"])
    again = run_fwd(c, dv, bf16, table=mat, win=ident)
    for k in got:
        assert torch.equal(got[k], again[k]), (c["id"], k, "differs from the run on the materialised windows")


# ------------------------------------------------------------------------------------------------ refusals
def _refusal_call(entry, kw):
    """a valid small call of ``entry`` with ``kw`` changed -> (rc, the output allocation)"""
    L = lib()
    a = dict(B=2, T=6, cin=32 if entry != "adj" else 16, cout=16 if entry != "adj" else 32, d=1, ks=1, nrep=2, stats=entry == "fwd", col=False,
             ring=0, n_seg=2, ep=False, both=False, null=[], misalign=None, stride=None)
    a.update(kw)
    big = lambda dt=torch.float32: torch.zeros(1 << 16, dtype=dt, device=DEV)
    t = {k: big() for k in ("src", "scale", "shift", "W", "dy", "dz", "y", "coef", "ep_y", "ep_scale", "ep_shift", "ep_mean", "ep_rstd", "col")}
    t["stats"] = big(torch.float64)
    out = Out(1 << 14)
    p = {k: (None if k in a["null"] else ptr(v, 4 if a["misalign"] == k else 0)) for k, v in t.items()}
    B, T, cin, cout = a["B"], a["T"], a["cin"], a["cout"]
    width = cin if entry == "adj" else cout
    stride = 0 if a["ks"] == 1 else B * T * width + (a["stride"] or 0)
    shape = (B, T, cin, cout, a["d"], a["ks"], stride)
    rows = torch.zeros(B, dtype=torch.int32, device=DEV)
    if entry == "fwd":
        rc = L.pcaa_dtc_conv_fwd(p["src"], p["scale"], p["shift"], p["W"], ptr(out.win), p["col"] if a["col"] else None,
                                 p["stats"] if a["stats"] else None, a["nrep"], *shape, stream())
    elif entry == "win":
        rc = L.pcaa_dtc_conv_fwd_win_bf16(p["src"], p["scale"], p["shift"], p["W"], ptr(out.win), p["col"] if a["col"] else None,
                                          p["stats"] if a["stats"] else None, a["nrep"], *shape, ptr(rows), 12, a["ring"], stream())
    elif entry == "seg":
        rc = L.pcaa_dtc_conv_fwd_seg(p["src"], p["scale"], p["shift"], p["W"], ptr(out.win), *shape, ptr(rows), a["n_seg"], 6, stream())
    else:
        formed = a["both"]
        ep = [p[k] if a["ep"] else None for k in ("ep_y", "ep_scale", "ep_shift", "ep_mean", "ep_rstd")]
        rc = L.pcaa_dtc_conv_dgrad(p["dy"], p["dz"] if formed else None, p["y"] if formed else None, p["coef"] if formed else None, None,
                                   p["W"], ptr(out.win), *ep, p["stats"] if a["ep"] else None, a["nrep"], *shape, stream())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("reason", sorted(D.REFUSALS))
def test_refusals(reason):
    entry, kw, fragment = D.REFUSALS[reason]
    L = lib()
    rc, out = _refusal_call(entry, kw)
    msg = L.pcaa_last_error().decode()
    assert rc == 1 and fragment in msg, (reason, rc, msg)
    assert out.untouched(), "a refused call wrote to its output"
    assert L.pcaa_bn_tail_pending() == 0
    rc, out = _refusal_call(entry, {})
    assert rc == 0 and not out.untouched(), (reason, "the unchanged call must be accepted", L.pcaa_last_error())


# ------------------------------------------------------------------------------------------------ carried finalize
@pytest.mark.parametrize("family", ["one_f32", "one_bf16", "pair_fwd", "pair_adj"])
def test_carried_finalize(family):
    from opensetgaitrecognition_pcaa_amd import ops, synthetic as syn

    def bn(ch, seed):
        m = torch.nn.BatchNorm1d(ch).to(DEV)
        syn.deterministic_fill_(m, seed)
        return m
    adj = family == "pair_adj"
    B, T, cin, cout, d = (4, 7, 160, 80, 2) if family == "pair_fwd" else ((4, 7, 80, 160, 2) if adj else (4, 9, 36, 48, 2))
    c = D._c(family, adj, B, T, cin, cout, d, "pair32" if family.startswith("pair") else "one", act=True, form=3 if adj else 0)
    raw = {k: v.to(DEV) for k, v in D.inputs(c).items()}
    bf16 = family == "one_bf16"
    assert D.ROUTES[lib().pcaa_dtc_conv_route(int(adj), int(bf16), B, cin, cout, 1, 0)] == ("pair32_f32" if family.startswith("pair") else family)
    taken0 = ops.TAILS["taken"]
    if not adj:
        bias = D.uniform(cout, 5, DEV, -0.1, 0.1).float()
        bn_a, bn_b = bn(cout, 7), bn(cout, 7)
        stats = ops.new_stats(cout, DEV)
        tail = ops.BnTailFwd(B * T, bias, bn_a, cout)
        ops.dtc_conv_fwd(raw["src"], raw["scale"], raw["shift"], raw["W"], B, T, d, stats=stats, tail=tail, bf16=bf16)
        ref = ops.bn_finalize(stats, B * T, bias, bn_b, cout)
        torch.cuda.synchronize()
        for a, b, nm in zip(tail.out, ref, ("scale", "shift", "mean", "rstd")):
            assert torch.allclose(a, b, rtol=1e-6, atol=1e-7), (nm, (a - b).abs().max().item())
        assert torch.allclose(bn_a.running_var, bn_b.running_var, rtol=1e-6, atol=1e-7)
    else:
        bn_a, bn_b = bn(cin, 9), bn(cin, 9)
        below = (raw["ep_y"], raw["ep_scale"], raw["ep_shift"], raw["ep_mean"], raw["ep_rstd"])
        tail = ops.BnTailBwd(B * T, bn_a, raw["ep_mean"], raw["ep_rstd"], cin)
        _, st, _ = ops.dtc_conv_dgrad(None, raw["W"], B, T, cin, d, dz=raw["dz"], y=raw["y"], coef=raw["coef"], below=below, tail=tail)
        ref = ops.bn_bwd_finalize(st, B * T, bn_b, raw["ep_mean"], raw["ep_rstd"], cin)
        torch.cuda.synchronize()
        for a, b in zip(tail.out, ref):
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), (a - b).abs().max().item()
    assert ops.TAILS["taken"] - taken0 == 1, "the launch must have carried its finalize"


# ------------------------------------------------------------------------------------------------ PCAA_DTC_PAIR
def child():
    """the pair-shaped cases under this process's PCAA_DTC_PAIR -> CHILD_RESULT {route: worst ratio}, CHILD_CASES {case: route}"""
    routes = {}
    for which, cases in (("fwd", D.fwd_cases()), ("adj", D.adj_cases())):
        for c in cases:
            if c["fam"] == "one":
                continue
            for bf16 in (False, True):
                fam = D.family(c, bf16, SWITCH)
                if fam == "one" and c["kc"] > (D.DG_MAX_CR if c["adj"] else D.MAX_CR):
                    continue        # a one-sequence workgroup cannot keep this many channels: the entry point refuses
                routes[f"{which}/{c['id']}/{'bf16' if bf16 else 'f32'}"] = one_case(c, bf16)
    print("CHILD_CASES " + json.dumps(routes))
    print("CHILD_RESULT " + json.dumps({r: max(v.values()) for r, v in WORST.items()}))


def test_pair_switch_in_a_child_process():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for value in ("0", "fwd", "adj"):
        env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""), PCAA_DTC_PAIR=value)
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], capture_output=True, text=True, timeout=300, cwd=root, env=env)
        assert res.returncode == 0, (value, res.stdout[-3000:], res.stderr[-3000:])
        take = lambda tag: json.loads([l for l in res.stdout.splitlines() if l.startswith(tag + " ")][-1][len(tag) + 1:])
        cases, worst = take("CHILD_CASES"), take("CHILD_RESULT")
        print(f"[dtc] PCAA_DTC_PAIR={value}: " + ", ".join(f"{r} {v:.3f}" for r, v in sorted(worst.items())))
        assert all(v <= 1.0 for v in worst.values()), (value, worst)
        for name, r in cases.items():
            off = value == "0" or (value == "fwd") == name.startswith("adj/")
            assert r.startswith("one_") == off, (value, name, r)
        if value == "0":
            assert cases["fwd/pair32_odd_quads/f32"] == "one_f32" and cases["adj/two_pass_512/bf16"] == "one_bf16", cases


# ------------------------------------------------------------------------------------------------ predicates
def test_supported_and_ksplit_predicates():
    L = lib()
    for B in (1, 2, 8, 9, 64):
        for cin in (4, 96, 256, 257, 258, 259, 260, 480, 512, 516, 544, 1024, 2080):
            for cout in (16, 32, 64, 512, 516):
                assert L.pcaa_dtc_conv_supported(30, cin, cout) == D.supported(30, cin, cout), (cin, cout)
                assert L.pcaa_dtc_conv_ksplit(B, cin, cout) == D.fwd_ksplit(B, cin, cout), (B, cin, cout)
                assert L.pcaa_dtc_conv_dgrad_ksplit(B, cin, cout) == D.dgrad_ksplit(B, cin, cout), (B, cin, cout)
    for T in (0, 1, 32, 33):
        assert L.pcaa_dtc_conv_supported(T, 4, 16) == D.supported(T, 4, 16)
    # every ksplit the library returns is accepted by the entry point it is for: every supported point of the grid, both
    # dtypes, launched at T = 2 on zero operands (the values are checked on the sample below)
    z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=DEV)
    big, small = z(8 << 20), z(1 << 20)
    for B in (1, 2, 8, 9, 64):
        for cin in (4, 96, 256, 260, 480, 512, 516, 544, 1024, 2080):
            for cout in (16, 32, 64, 512, 516):
                for bf16 in (False, True):
                    sfx = "_bf16" if bf16 else ""
                    if D.supported(2, cin, cout):
                        ks = L.pcaa_dtc_conv_ksplit(B, cin, cout)
                        rc = getattr(L, "pcaa_dtc_conv_fwd" + sfx)(ptr(small), None, None, ptr(big), ptr(big, 4 << 22), None, None, 1, B, 2, cin, cout, 1,
                                                                   ks, B * 2 * cout if ks > 1 else 0, stream())
                        assert rc == 0, ("fwd", B, cin, cout, ks, L.pcaa_last_error())
                    ks = L.pcaa_dtc_conv_dgrad_ksplit(B, cin, cout)
                    rc = getattr(L, "pcaa_dtc_conv_dgrad" + sfx)(ptr(small), None, None, None, None, ptr(big), ptr(big, 4 << 22), None, None, None, None,
                                                                 None, None, 1, B, 2, cin, cout, 1, ks, B * 2 * cin if ks > 1 else 0, stream())
                    assert rc == 0, ("adj", B, cin, cout, ks, L.pcaa_last_error())
    torch.cuda.synchronize()
    # a sample of them with the values compared, the forward in fp32 and the adjoint in bf16
    for B, cin, cout in ((1, 260, 16), (9, 512, 16), (2, 516, 16), (1, 2080, 16), (8, 480, 16), (9, 544, 64)):
        c = D._c(f"ksplit {B},{cin},{cout}", False, B, 2, cin, cout, 1, "one", ks=D.fwd_ksplit(B, cin, cout))
        dv, raw = dev_inputs(c)
        compare(c, expect_route(dict(c, fam=D.family(c, False)), False), run_fwd(c, dv, False), D.reference(c, raw, False))
    for B, cin, cout in ((2, 16, 512), (2, 16, 516), (1, 64, 1028)):
        c = D._c(f"dgrad ksplit {B},{cin},{cout}", True, B, 2, cin, cout, 1, "one", ks=D.dgrad_ksplit(B, cin, cout))
        dv, raw = dev_inputs(c)
        compare(c, expect_route(dict(c, fam=D.family(c, True)), True), run_adj(c, dv, True), D.reference(c, raw, True))


def test_worst_ratio_per_route():
    """the summary line per route of everything this process ran (empty when the test is run alone)"""
    for r, w in sorted(WORST.items()):
        print(f"[dtc] route {r}: worst |err| / gate = {max(w.values()):.3f}  (" + ", ".join(f"{k} {v:.3f}" for k, v in sorted(w.items())) + ")")
        assert max(w.values()) <= 1.0


if __name__ == "__main__":
    if sys.argv[1:] == ["child"]:
        child()
