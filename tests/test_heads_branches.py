"""Every branch of csrc/heads.hip (pcaa_heads_fwd, pcaa_heads_bwd), of their wrappers ops.heads_fwd / ops.heads_bwd and
of the two routes of functional._encoder_heads_backward against fp64 (references, gates, inputs and cases:
tests/heads_ref.py; the gates themselves are shown reference-safe and defect-sensitive by tests/test_heads_gates_cpu.py).

Every comparison prints ``worst |err| / gate`` of its case (pytest -rP); the numbers are reported, the assertion is
``<= 1``.  No element is excluded.

    branch                                                              test
    ------------------------------------------------------------------  ------------------------------------------------
    forward: projection head on / off (W2 at pitch 16 / 32), decoder    test_forward (every case of HEADS_CASES)
      head on / off; B = 1, 3, 5 (partial last workgroup), 4, 64, 65,
      130; K = 1 .. 70: the second trip of the q < 4 K loop at K >= 65
    backward: head on / off (ds from dh . Wh or from dl . W2), proj on  test_backward (every case of HEADS_BWD_CASES x
      / off, d_logits / d_sup / d_hproj each alone, all, none; B = 1      HEADS_USES), from the reference's forward
      .. 64, K = 1 .. 8; the job spread of the small gradients over      values rounded once (a) and from the kernel's
      the 16 workgroups with 2 .. 7 jobs                                  own forward outputs (b)
    backward: no upstream gradient -> every output exactly 0;           test_backward
      d_logits None -> dW2, db2, dWh, dbh exactly 0
    backward: Wg given, d_hproj None -> no dWg / dbg, the bits of the   test_backward
      call without the decoder head
    extents of every output (NaN-filled guard bands on both sides),     test_extents
      the launchers called directly: B = 1, 3, 5, 64
    a forward row's bits do not depend on B or on its slot; a dx4       test_rows_do_not_depend_on_the_batch
      row's bits do not depend on the other rows
    two identical calls give identical bits                             test_identical_calls_identical_bits
    ``outs`` destinations are written in place, nothing between them    test_outs_are_written_in_place
    ops.heads_fwd / heads_bwd refuse before any launch: every wrong     test_wrong_shapes_are_refused,
      shape, Wh without bh, Wg without bg, B = 65 / K = 9 backward,       test_unsupported_sizes_and_bad_tensors_are_refused
      misaligned x4, CPU tensor, non-contiguous tensor
    functional: (64, 8) takes the fused backward, (65, 8) and (8, 9)    test_routes
      the layer-by-layer one; head on / off, decoder head + d_hproj +
      gph_gout on / off, gout views on / off, d_logits None
"""
import copy

import pytest
import torch

import heads_ref as R
from helpers import make_encoder, make_head
from opensetgaitrecognition_pcaa_amd import _lib, functional as F_hip, ops
from opensetgaitrecognition_pcaa_amd._lib import PcaaError
from test_eval_bwd_modules import DXTOL, GTOL, TOL, _close, _rel_l2

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32
WORST = {}                      # (output, form) -> largest |err| / gate of the kernels


def check(name, key, form, got, want, gate):
    got = got.double().reshape(want.shape)
    assert bool(torch.isfinite(got).all()), (name, "non-finite output")
    err = (got - want).abs() / gate.clamp_min(1e-300)
    r = float(err.max()) if err.numel() else 0.0
    WORST[(key, form)] = max(WORST.get((key, form), 0.0), r)
    print(f"[heads] {name}: worst |err| / gate = {r:.3f}")
    if not r <= 1.0:
        at = [int(i) for i in torch.unravel_index(err.argmax(), err.shape)]
        print(f"[heads] {name}: worst at {at}; {int((err > 1.0).sum())} of {err.numel()} over the gate")
    assert r <= 1.0, (name, r)


def fwd(c):
    return ops.heads_fwd(c["x4"], c["W1"], c["b1"], c.get("Wh"), c.get("bh"), c["W2"], c["b2"], c.get("Wg"), c.get("bg"))


def bwd(c, acts, use, outs=None, with_proj=True):
    """acts: (sup_fv, h, logits, hproj) fp32 as heads_fwd returns them; with_proj False: the call without the decoder head"""
    s, h, lg, hp = acts
    up = [c[k] if k in use else None for k in ("d_logits", "d_sup", "d_hproj")]
    return ops.heads_bwd(c["x4"], s, h, lg, hp if with_proj else None, c["W1"], c.get("Wh"), c["W2"],
                         c.get("Wg") if with_proj else None, *up, outs=outs)


def _named(acts):
    return {k: v for k, v in zip(R.FWD_KEYS, acts) if v is not None}


# ====================================================================================================== values
@pytest.mark.parametrize("case", R.HEADS_CASES, ids=R.case_id)
def test_forward(case):
    B, K, head, proj = case
    c = R.heads_case(*case, DEV)
    want, en = R.heads_fwd_ref(c), R.heads_fwd_en(c)
    s, h, lg, hp = got = fwd(c)
    assert (h is None) == (not head) and (hp is None) == (not proj)
    assert tuple(s.shape) == (B, 32) and tuple(lg.shape) == (B, K)
    assert set(_named(got)) == set(want)
    for k, g in _named(got).items():
        assert g.dtype == F32 and g.is_contiguous() and tuple(g.shape) == tuple(want[k].shape)
        check(f"{R.case_id(case)} fwd {k}", k, "a", g, want[k], R.gate_of(en[k]))


@pytest.mark.parametrize("case", R.HEADS_BWD_CASES, ids=R.case_id)
def test_backward(case):
    B, K, head, proj = case
    c = R.heads_case(*case, DEV)
    tag = R.case_id(case)
    want_f = R.heads_fwd_ref(c)
    own = fwd(c)
    rounded = tuple(want_f[k].float().contiguous() if k in want_f else None for k in R.FWD_KEYS)
    forms = {"a": (R.acts_rounded(want_f), rounded), "b": (R.acts_from_fwd(c), own)}
    for use in R.HEADS_USES:
        use = R.use_of(use, proj)
        want = R.heads_bwd_ref(c, use)
        for form, (en_acts, acts) in forms.items():
            en = R.heads_bwd_en(c, use, en_acts)
            outs, dx4 = bwd(c, acts, use)
            got = dict(outs, dx4=dx4)
            assert set(got) == set(want) == set(en), (tag, use, sorted(got))
            for k in R.BWD_KEYS:
                if k in got:
                    assert tuple(got[k].shape) == tuple(want[k].shape)
                    check(f"{tag} bwd ({form}) {'+'.join(use) or 'none'} {k}", k, form, got[k], want[k], R.gate_of(en[k]))
            if not use:
                assert all(not bool(v.any()) for v in got.values()), (tag, "no upstream gradient: every output is exactly 0")
            if "d_logits" not in use:
                assert all(not bool(got[k].any()) for k in ("dW2", "db2", "dWh", "dbh") if k in got), (tag, use)
            if proj and "d_hproj" not in use:
                # Wg and hproj were given: nothing of the decoder head may show
                assert "dWg" not in got and "dbg" not in got
                outs0, dx0 = bwd(c, acts, use, with_proj=False)
                assert set(outs0) == set(outs) and torch.equal(dx0, dx4), (tag, use)
                assert all(torch.equal(outs0[k], outs[k]) for k in outs), (tag, use)


def test_print_largest_ratios():
    """after the cases above (file order): the table that stands in the docstring of heads_ref"""
    for k in R.FWD_KEYS + R.BWD_KEYS:
        a, b = WORST.get((k, "a")), WORST.get((k, "b"))
        if a is not None:
            print(f"[heads] largest kernel ratio {k:7s} fwd / (a) {a:.3f}" + (f"   (b) {b:.3f}" if b is not None else ""))
    assert all(v <= 1.0 for v in WORST.values())


# ====================================================================================================== extents
GUARD = 64                      # floats on either side: a multiple of 4, so the slice keeps the allocation's 16-byte alignment


def _guarded(*shape):
    n = int(torch.Size(shape).numel())
    big = torch.full((n + 2 * GUARD,), float("nan"), dtype=F32, device=DEV)
    view = big[GUARD:GUARD + n].view(*shape)
    assert view.data_ptr() % 16 == 0
    return big, view


def _assert_extent(name, big, view):
    n = view.numel()
    assert not bool(torch.isnan(view).any()), (name, "an element of the output was not written")
    assert bool(torch.isnan(big[:GUARD]).all()) and bool(torch.isnan(big[GUARD + n:]).all()), (name, "written outside its extent")


@pytest.mark.parametrize("B,K,head,proj", [(1, 1, True, True), (3, 8, False, False), (5, 2, True, True), (5, 8, False, True),
                                           (64, 8, True, True), (64, 1, True, False)])
def test_extents(B, K, head, proj):
    c = R.heads_case(B, K, head, proj, DEV)
    lib = _lib.load()
    p = lambda t: None if t is None else t.data_ptr()
    shapes = {"sup_fv": (B, 32), "logits": (B, K)}
    if head:
        shapes["h"] = (B, 16)
    if proj:
        shapes["hproj"] = (B, 64)
    f = {k: _guarded(*s) for k, s in shapes.items()}
    v = lambda d, k: d[k][1] if k in d else None
    rc = lib.pcaa_heads_fwd(p(c["x4"]), p(c["W1"]), p(c["b1"]), p(c.get("Wh")), p(c.get("bh")), p(c["W2"]), p(c["b2"]),
                            p(c.get("Wg")), p(c.get("bg")), p(v(f, "sup_fv")), p(v(f, "h")), p(v(f, "logits")), p(v(f, "hproj")),
                            B, K, ops._s())
    _lib.check(rc, "pcaa_heads_fwd")
    torch.cuda.synchronize()
    for k, (big, view) in f.items():
        _assert_extent(f"fwd {k}", big, view)
    ref = _named(fwd(c))
    assert all(torch.equal(f[k][1], ref[k]) for k in f)
    din2 = 16 if head else 32
    gshapes = {"dx4": (B, 512), "dW1": (32, 512), "db1": (32,), "dW2": (K, din2), "db2": (K,)}
    if head:
        gshapes.update(dWh=(16, 32), dbh=(16,))
    if proj:
        gshapes.update(dWg=(64, 32), dbg=(64,))
    g = {k: _guarded(*s) for k, s in gshapes.items()}
    rc = lib.pcaa_heads_bwd(p(c["x4"]), p(v(f, "sup_fv")), p(v(f, "h")), p(v(f, "logits")), p(v(f, "hproj")), p(c["W1"]),
                            p(c.get("Wh")), p(c["W2"]), p(c.get("Wg")), p(c["d_logits"]), p(c["d_sup"]), p(c.get("d_hproj")),
                            p(v(g, "dW1")), p(v(g, "db1")), p(v(g, "dWh")), p(v(g, "dbh")), p(v(g, "dW2")), p(v(g, "db2")),
                            p(v(g, "dWg")), p(v(g, "dbg")), p(v(g, "dx4")), B, K, ops._s())
    _lib.check(rc, "pcaa_heads_bwd")
    torch.cuda.synchronize()
    for k, (big, view) in g.items():
        _assert_extent(f"bwd {k}", big, view)
    outs, dx4 = bwd(c, tuple(ref.get(k) for k in R.FWD_KEYS), R.use_of(R.HEADS_USES[3], proj))
    assert all(torch.equal(g[k][1], dict(outs, dx4=dx4)[k]) for k in g)


# ====================================================================================================== bit-level properties
def _rows(c, idx):
    """the case with its batch rows taken at ``idx``"""
    per_row = ("x4", "d_logits", "d_sup", "d_hproj")
    return {k: (v[idx].contiguous() if k in per_row else v) for k, v in c.items()}


@pytest.mark.parametrize("head,proj", [(True, True), (False, False)])
def test_rows_do_not_depend_on_the_batch(head, proj):
    B, K = 64, 8
    c = R.heads_case(B, K, head, proj, DEV)
    use = R.use_of(R.HEADS_USES[3], proj)
    acts = fwd(c)
    _, dx4 = bwd(c, acts, use)
    perm = torch.tensor([(37 * i + 11) % B for i in range(B)], device=DEV)          # 37 is prime to 64: a permutation
    assert sorted(perm.tolist()) == list(range(B)) and bool((perm % 4 != torch.arange(B, device=DEV) % 4).any())
    cp = _rows(c, perm)
    acts_p = fwd(cp)
    for k, a, b in zip(R.FWD_KEYS, acts, acts_p):
        if a is not None:
            assert torch.equal(b, a[perm]), (k, "a forward row depends on its slot")
    _, dx4_p = bwd(cp, acts_p, use)
    assert torch.equal(dx4_p, dx4[perm]), "a dx4 row depends on the other rows' slots"
    for r in (0, 5, 63):
        one = _rows(c, torch.tensor([r], device=DEV))
        acts_1 = fwd(one)
        for k, a, b in zip(R.FWD_KEYS, acts, acts_1):
            if a is not None:
                assert torch.equal(b, a[r:r + 1]), (k, r, "a forward row depends on B")
        _, dx4_1 = bwd(one, acts_1, use)
        assert torch.equal(dx4_1, dx4[r:r + 1]), (r, "a dx4 row depends on the other rows")


@pytest.mark.parametrize("case", [(5, 2, True, True), (64, 8, True, True), (3, 8, False, False)], ids=R.case_id)
def test_identical_calls_identical_bits(case):
    c = R.heads_case(*case, DEV)
    use = R.use_of(R.HEADS_USES[3], case[3])
    a1, a2 = fwd(c), fwd(c)
    assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a1, a2))
    (o1, d1), (o2, d2) = bwd(c, a1, use), bwd(c, a1, use)
    assert torch.equal(d1, d2) and set(o1) == set(o2) and all(torch.equal(o1[k], o2[k]) for k in o1)


@pytest.mark.parametrize("case", [(5, 2, True, True), (64, 8, False, True)], ids=R.case_id)
def test_outs_are_written_in_place(case):
    B, K, head, proj = case
    c = R.heads_case(*case, DEV)
    use = R.use_of(R.HEADS_USES[3], proj)
    acts = fwd(c)
    ref, _ = bwd(c, acts, use)
    GAP, MARK = 12, 7.0                                                          # at least 12 marked floats between destinations
    flat = torch.full((sum(v.numel() + GAP + 4 for v in ref.values()) + GAP,), MARK, dtype=F32, device=DEV)
    outs, gaps, at = {}, torch.ones_like(flat, dtype=torch.bool), GAP
    for k, v in ref.items():
        outs[k] = flat[at:at + v.numel()].view(v.shape).zero_()
        gaps[at:at + v.numel()] = False
        at = (at + v.numel() + GAP + 3) // 4 * 4
    ptrs = {k: v.data_ptr() for k, v in outs.items()}
    got, _ = bwd(c, acts, use, outs=outs)
    assert set(got) == set(ref)
    for k in ref:
        assert got[k].data_ptr() == ptrs[k] and torch.equal(got[k], ref[k]) and torch.equal(outs[k], ref[k]), k
    assert bool((flat[gaps] == MARK).all()), "the bytes between the destinations changed"


# ====================================================================================================== refusals
class _Arena:
    """Wrong-shaped tensors are views at the start of one large allocation the test owns: were a check missing, the kernel
    would read or write past the view's end inside this allocation, not in foreign memory."""

    def __init__(self):
        self.buf = torch.zeros(1 << 20, dtype=F32, device=DEV)              # 4 MiB: beyond anything the kernels address

    def view(self, *shape, offset=0):
        n = int(torch.Size(shape).numel())
        return self.buf[offset:offset + n].view(*shape)


def _spy(monkeypatch):
    """records the return code of every launcher call ops makes"""
    seen, real = [], ops.check

    def check(rc, what=""):
        seen.append(rc)
        return real(rc, what)

    monkeypatch.setattr(ops, "check", check)
    return seen


def _fwd_args(c):
    return {k: c.get(k) for k in ("x4", "W1", "b1", "Wh", "bh", "W2", "b2", "Wg", "bg")}


def _bwd_args(c, acts):
    s, h, lg, hp = acts
    return {"x4": c["x4"], "sup_fv": s, "h": h, "logits": lg, "hproj": hp, "W1": c["W1"], "Wh": c.get("Wh"), "W2": c["W2"],
            "Wg": c.get("Wg"), "d_logits": c["d_logits"], "d_sup": c["d_sup"], "d_hproj": c.get("d_hproj")}


def test_wrong_shapes_are_refused(monkeypatch):
    B, K = 5, 4
    arena = _Arena()
    cases = [(head, R.heads_case(B, K, head, True, DEV)) for head in (True, False)]
    cases = [(head, c, fwd(c)) for head, c in cases]
    seen = _spy(monkeypatch)
    for head, c, acts in cases:
        d2 = 16 if head else 32
        wrong = {"W1": [(16, 512), (32, 256), (32, 513)], "b1": [(31,), (1, 32)], "W2": [(K, 48 - d2), (K, d2 - 1), (K * d2,)],
                 "b2": [(K - 1,), (K + 1,)], "Wg": [(32, 32), (64, 16), (63, 32)], "bg": [(63,), (32,)]}
        if head:
            wrong.update(Wh=[(8, 32), (16, 16), (32, 16)], bh=[(15,), (8,)])
        for nm, shapes in wrong.items():
            for shape in shapes:
                with pytest.raises(ValueError, match=rf"heads_fwd\.{nm}\b"):
                    ops.heads_fwd(**dict(_fwd_args(c), **{nm: arena.view(*shape)}))
        wrong_b = {"sup_fv": [(B, 16), (B - 1, 32)], "logits": [(B, K + 1), (B, K - 1), (B - 1, K)], "hproj": [(B, 32), (B - 1, 64)],
                   "W1": wrong["W1"], "W2": [(K, 48 - d2), (K, d2 - 1)], "Wg": wrong["Wg"],
                   "d_logits": [(B, K - 1), (B - 1, K)], "d_sup": [(B, 16), (B - 1, 32)], "d_hproj": [(B, 32), (B - 1, 64)]}
        if head:
            wrong_b.update(h=[(B, 8), (B - 1, 16)], Wh=wrong["Wh"])
        for nm, shapes in wrong_b.items():
            for shape in shapes:
                with pytest.raises(ValueError, match=rf"heads_bwd\.{nm}\b"):
                    ops.heads_bwd(**dict(_bwd_args(c, acts), **{nm: arena.view(*shape)}))
        dests = {"dW1": [(32, 256), (16, 512)], "db1": [(16,), (31,)], "dW2": [(K - 1, d2), (K, d2 - 1)], "db2": [(K - 1,)],
                 "dWg": [(32, 32), (64, 16)], "dbg": [(63,)]}
        if head:
            dests.update(dWh=[(8, 32), (16, 16)], dbh=[(15,)])
        for nm, shapes in dests.items():
            for shape in shapes:
                with pytest.raises(ValueError, match=rf"heads_bwd\.{nm}\b"):
                    ops.heads_bwd(**_bwd_args(c, acts), outs={nm: arena.view(*shape)})
        # one of a pair
        for nm, other in (("bh", "Wh"), ("Wh", "bh"), ("bg", "Wg"), ("Wg", "bg")):
            if nm in c:
                with pytest.raises(ValueError, match=other):
                    ops.heads_fwd(**dict(_fwd_args(c), **{nm: None}))
    assert seen == [], "a refused call reached a launcher"
    assert not bool(arena.buf.any())


def test_unsupported_sizes_and_bad_tensors_are_refused(monkeypatch):
    arena = _Arena()
    c = dict(R.heads_case(5, 4, True, True, DEV))
    acts = fwd(c)
    seen = _spy(monkeypatch)
    # the backward's limits: B <= 64, K <= 8 -- every other tensor has the shape that B and K ask for
    for B, K, names in ((65, 8, "x4"), (8, 9, "W2"), (65, 9, "x4")):
        big = {"x4": arena.view(B, 512), "sup_fv": arena.view(B, 32), "h": arena.view(B, 16), "logits": arena.view(B, K),
               "hproj": arena.view(B, 64), "W1": c["W1"], "Wh": c["Wh"], "W2": arena.view(K, 16), "Wg": c["Wg"],
               "d_logits": arena.view(B, K), "d_sup": arena.view(B, 32), "d_hproj": arena.view(B, 64)}
        assert not ops.heads_supported(B, K, 512, 32, 16, 64, True) and ops.heads_supported(B, K, 512, 32, 16, 64, False)
        with pytest.raises(ValueError, match=rf"heads_bwd: .*{names}"):
            ops.heads_bwd(**big)
    with pytest.raises(ValueError, match="heads_fwd: .*x4"):
        ops.heads_fwd(**dict(_fwd_args(c), x4=arena.view(5, 256)))
    with pytest.raises(ValueError, match="heads_fwd: .*x4"):
        ops.heads_fwd(**dict(_fwd_args(c), x4=arena.view(0, 512)))
    with pytest.raises(ValueError, match=r"heads_fwd\.x4"):
        ops.heads_fwd(**dict(_fwd_args(c), x4=arena.view(5 * 512)))
    # as _chk refuses them: a CPU tensor, a wrong dtype, a non-contiguous tensor
    for fn, args in (("heads_fwd", _fwd_args(c)), ("heads_bwd", _bwd_args(c, acts))):
        call = getattr(ops, fn)
        for nm in ("x4", "W1", "W2", "Wh", "Wg") + (("b1", "bg") if fn == "heads_fwd" else ("sup_fv", "h", "logits", "hproj", "d_sup")):
            with pytest.raises(RuntimeError, match=rf"{fn}\.{nm}: expected a tensor on the HIP device"):
                call(**dict(args, **{nm: args[nm].cpu()}))
            with pytest.raises(TypeError, match=rf"{fn}\.{nm}\b"):
                call(**dict(args, **{nm: args[nm].double()}))
            if args[nm].dim() == 2:
                r, w = args[nm].shape
                with pytest.raises(ValueError, match=rf"{fn}\.{nm}: must be contiguous"):
                    call(**dict(args, **{nm: arena.view(w, r).t()}))
    with pytest.raises(ValueError, match=r"heads_bwd\.dW1: must be contiguous"):
        ops.heads_bwd(**_bwd_args(c, acts), outs={"dW1": arena.view(512, 32).t()})
    with pytest.raises(RuntimeError, match=r"heads_bwd\.db1: expected a tensor on the HIP device"):
        ops.heads_bwd(**_bwd_args(c, acts), outs={"db1": torch.zeros(32)})
    assert seen == [], "a refused call reached a launcher"
    # a misaligned x4 is the launcher's to refuse: it returns from its argument checks
    odd = arena.view(5, 512, offset=1)
    odd.copy_(c["x4"])
    assert odd.data_ptr() % 16 == 4 and odd.is_contiguous()
    with pytest.raises(PcaaError, match="pcaa_heads_fwd: x4"):
        ops.heads_fwd(**dict(_fwd_args(c), x4=odd))
    with pytest.raises(PcaaError, match="pcaa_heads_bwd: x4"):
        ops.heads_bwd(**dict(_bwd_args(c, acts), x4=odd))
    assert seen == [1, 1], "PCAA_ERR_INVALID_ARG: the launcher returned before its launch"
    torch.cuda.synchronize()


# ====================================================================================================== the two routes
def _route_names(head, with_gph):
    names = ["MLP_sup1.0", "MLP_sup2.0"] + (["MLP_head.0"] if head else []) + (["GPH.0"] if with_gph else [])
    return {f"{n}.{p}" for n in names for p in ("weight", "bias")}


_KERNEL_KEY = {"MLP_sup1.0.weight": "dW1", "MLP_sup1.0.bias": "db1", "MLP_sup2.0.weight": "dW2", "MLP_sup2.0.bias": "db2",
               "MLP_head.0.weight": "dWh", "MLP_head.0.bias": "dbh", "GPH.0.weight": "dWg", "GPH.0.bias": "dbg"}


@pytest.mark.parametrize("with_gout", [False, True], ids=["alloc", "gout"])
@pytest.mark.parametrize("with_gph", [False, True], ids=["nogph", "gph"])
@pytest.mark.parametrize("head", [False, True], ids=["nohead", "head"])
@pytest.mark.parametrize("B,K,fused", [(64, 8, True), (65, 8, False), (8, 9, False)])
def test_routes(monkeypatch, B, K, fused, head, with_gph, with_gout):
    enc = make_encoder(K, 8, 4, head, seed=3).to(DEV)
    gph = make_head(32, 64, seed=5).to(DEV) if with_gph else None
    seed = R.seed_of(B, K)
    r = lambda s, a, *shape: R.uniform(int(torch.Size(shape).numel()), seed + s, DEV, -a, a).view(*shape).float().contiguous()
    x4, d_logits, d_sup = r(0, 1.7, B, 512), r(1, 1.0, B, K), r(2, 1.0, B, 32)
    d_hproj = r(3, 1.0, B, 64) if with_gph else None
    mods = {"MLP_sup1.0": enc.MLP_sup1[0], "MLP_sup2.0": enc.MLP_sup2[0]}
    if head:
        mods["MLP_head.0"] = enc.MLP_head[0]
    if with_gph:
        mods["GPH.0"] = gph[0]
    calls = []
    real = ops.heads_bwd
    monkeypatch.setattr(ops, "heads_bwd", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def run(d_lg):
        st = F_hip.EncoderState()
        st.B, st.x4 = B, x4
        with torch.no_grad():
            logits, sup_fv, _ = F_hip._encoder_heads(enc, st, x4, gph)
        gout = gph_gout = flat = None
        if with_gout:
            flat = torch.zeros(sum(p.numel() for m in mods.values() for p in m.parameters()), dtype=F32, device=DEV)
            views, at = {}, 0
            for n, m in mods.items():
                for pn, p in (("weight", m.weight), ("bias", m.bias)):
                    views[f"{n}.{pn}"] = flat[at:at + p.numel()].view(p.shape)
                    at += p.numel()
            gout = {k: v for k, v in views.items() if not k.startswith("GPH")}
            gph_gout = (views["GPH.0.weight"], views["GPH.0.bias"]) if with_gph else None
        before = len(calls)
        with torch.no_grad():
            g, dx4 = F_hip._encoder_heads_backward(enc, st, d_lg, d_sup, gout, gph, d_hproj, gph_gout)
        torch.cuda.synchronize()
        assert (len(calls) - before == 1) == fused, "the route: fused exactly when pcaa_heads_supported takes the backward"
        assert set(g) == _route_names(head, with_gph)
        if with_gout:
            views = dict(gout, **({"GPH.0.weight": gph_gout[0], "GPH.0.bias": gph_gout[1]} if with_gph else {}))
            assert all(g[k].data_ptr() == views[k].data_ptr() for k in g), "the gradients are the caller's views"
        return st, g, dx4

    # fp64 autograd of the same Linear modules
    m64 = {n: copy.deepcopy(m).double() for n, m in mods.items()}
    xr = x4.double().requires_grad_(True)
    elu = torch.nn.functional.elu
    sup_r = elu(m64["MLP_sup1.0"](xr))
    h_r = elu(m64["MLP_head.0"](sup_r)) if head else sup_r
    log_r = elu(m64["MLP_sup2.0"](h_r))
    obj = (log_r * d_logits.double()).sum() + (sup_r * d_sup.double()).sum()
    if with_gph:
        hp_r = elu(m64["GPH.0"](sup_r))
        obj = obj + (hp_r * d_hproj.double()).sum()
    obj.backward()
    want = {f"{n}.{pn}": getattr(m, pn).grad for n, m in m64.items() for pn in ("weight", "bias")}

    st, g, dx4 = run(d_logits)
    tag = f"route B{B} K{K} head{int(head)} gph{int(with_gph)} gout{int(with_gout)}"
    if fused:
        # the kernel gates of heads_ref, form (b): the backward read the forward kernel's own outputs
        c = {"x4": x4, "W1": enc.MLP_sup1[0].weight.detach(), "b1": enc.MLP_sup1[0].bias.detach(),
             "W2": enc.MLP_sup2[0].weight.detach(), "b2": enc.MLP_sup2[0].bias.detach(), "d_logits": d_logits, "d_sup": d_sup}
        if head:
            c.update(Wh=enc.MLP_head[0].weight.detach(), bh=enc.MLP_head[0].bias.detach())
        if with_gph:
            c.update(Wg=gph[0].weight.detach(), bg=gph[0].bias.detach(), d_hproj=d_hproj)
        fen = R.heads_fwd_en(c)
        for k, got, ref in (("sup_fv", st.sup_fv, sup_r), ("logits", st.logits, log_r)) + \
                ((("h", st.h, h_r),) if head else ()) + ((("hproj", st.hproj, hp_r),) if with_gph else ()):
            check(f"{tag} {k}", k, "route", got, ref.detach(), R.gate_of(fen[k]))
        en = R.heads_bwd_en(c, R.use_of(R.HEADS_USES[3], with_gph), R.acts_from_fwd(c))
        check(f"{tag} dx4", "dx4", "route", dx4, xr.grad, R.gate_of(en["dx4"]))
        for k in g:
            check(f"{tag} {k}", _KERNEL_KEY[k], "route", g[k], want[k], R.gate_of(en[_KERNEL_KEY[k]]))
    else:
        _close(st.sup_fv, sup_r, TOL, what=f"{tag} sup_fv")
        _close(st.logits, log_r, TOL, what=f"{tag} logits")
        for k in g:
            _close(g[k], want[k], GTOL, what=f"{tag} d{k}")
        assert _rel_l2(dx4, xr.grad) <= DXTOL, f"{tag}: dx4 rel-l2 {_rel_l2(dx4, xr.grad):.3e}"

    # d_logits None: MLP_sup2 / MLP_head get exactly zero on either route, the same key set
    _, g0, _ = run(None)
    for k in g0:
        if k.startswith(("MLP_sup2", "MLP_head")):
            assert not bool(g0[k].any()), (tag, k)
