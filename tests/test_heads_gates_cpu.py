"""The gates of tests/heads_ref.py themselves, on the CPU, at the inputs tests/test_heads_branches.py uses:

* a plain-fp32 torch restatement of both kernels (the trees of heads_ref evaluated in float32) stays within every gate
  on the whole case list, forward, backward (a) -- from the reference's forward values rounded once -- and backward
  (b) -- from the restatement's own forward outputs.  The rounding counts of the rule are the ones the docstring of
  heads_ref derives from the kernel's text; none had to be corrected: the largest figure is printed per output;
* the closed forms the gates are propagated through equal fp64 autograd;
* the input condition (every ELU layer's pre-activations O(1), both signs) holds on every case with B >= 4;
* every planted defect moves every output it touches by more than 10 x the gate (the worst element), and >= 80 % of the
  elements it touches by that much, as the sibling files ask;
* pcaa_heads_supported's truth table, and the argument checks of pcaa_heads_fwd / pcaa_heads_bwd that return before any
  launch.  Only combinations that must be refused are passed: nothing here starts anything on a device.

Each check prints its figure (pytest -rP)."""
import itertools

import numpy as np
import pytest
import torch

import heads_ref as R
from opensetgaitrecognition_pcaa_amd import _lib

F32 = torch.float32
WORST = {}                      # (output, form) -> largest |err| / gate of the fp32 restatement


def within(name, key, form, got, want, gate):
    r = R.ratio(got, want, gate) if want.numel() else 0.0
    WORST[(key, form)] = max(WORST.get((key, form), 0.0), r)
    print(f"[heads gates] {name}: fp32 restatement, worst |err| / gate = {r:.4f}")
    assert r <= 1.0, (name, r)


def _same(name, en_v, auto):
    err = float((en_v.double().reshape(auto.shape) - auto).abs().max())
    assert err <= 1e-11 * (1 + float(auto.abs().max())), (name, err)


def bites(name, want, bad, gate):
    touched = int((bad != want).sum())
    assert touched > 0, (name, "the defect touches nothing at this case")
    worst, m = R.ratio(bad, want.double(), gate), R.moved(want, bad, gate)
    print(f"[heads gates] {name}: worst move {worst:.3g} x gate; {100 * m:.1f} % of the {touched} touched elements by > 10 x gate")
    assert worst > 10.0, (name, worst)
    assert m >= 0.8, (name, m)


@pytest.mark.parametrize("case", R.HEADS_CASES, ids=R.case_id)
def test_input_condition(case):
    c = R.heads_case(*case)
    ok, info = R.pre_condition(c)
    print(f"[heads gates] {R.case_id(case)}: " + ", ".join(f"{k}: rms {r:.2f} max {m:.2f}" for k, (_, r, m) in info.items()))
    if case[0] >= 4:
        assert ok, info
    assert (set(c) >= {"Wh", "bh"}) == case[2] and (set(c) >= {"Wg", "bg", "d_hproj"}) == case[3]


@pytest.mark.parametrize("case", R.HEADS_CASES, ids=R.case_id)
def test_fp32_restatement_within_gates(case):
    B, K, head, proj = case
    c = R.heads_case(*case)
    tag = R.case_id(case)
    want = R.heads_fwd_ref(c)
    en, lo = R.heads_fwd_en(c), R.heads_fwd_en(c, F32)
    assert set(en) == set(want) == {"sup_fv", "logits"} | ({"h"} if head else set()) | ({"hproj"} if proj else set())
    for k in en:
        _same(f"{tag} {k}", en[k].v, want[k])
        within(f"{tag} fwd {k}", k, "a", lo[k].v, want[k], R.gate_of(en[k]))
    if case not in R.HEADS_BWD_CASES:
        return
    forms = {"a": (R.acts_rounded(want), {k: R.EN(v.float()) for k, v in want.items()}),
             "b": (R.acts_from_fwd(c), {k: R.EN(v.v) for k, v in lo.items()})}
    for use in R.HEADS_USES:
        use = R.use_of(use, proj)
        ref = R.heads_bwd_ref(c, use)
        for form, (acts, acts32) in forms.items():
            en, lo32 = R.heads_bwd_en(c, use, acts), R.heads_bwd_en(c, use, acts32, dtype=F32)
            assert set(en) == set(ref) == set(lo32)
            for k in en:
                _same(f"{tag} {k}", en[k].v, ref[k])
                within(f"{tag} bwd ({form}) {'+'.join(use) or 'none'} {k}", k, form, lo32[k].v, ref[k], R.gate_of(en[k]))
                if not use or (k in ("dW2", "db2", "dWh", "dbh") and "d_logits" not in use):
                    assert not bool(lo32[k].v.any()) and not bool(ref[k].any()), (tag, use, k)


def test_print_largest_ratios():
    """after the cases above (file order): the table that stands in the docstring of heads_ref"""
    for k in R.FWD_KEYS + R.BWD_KEYS:
        a, b = WORST.get((k, "a")), WORST.get((k, "b"))
        if a is not None:
            print(f"[heads gates] largest fp32-restatement ratio {k:7s} fwd / (a) {a:.3f}" + (f"   (b) {b:.3f}" if b is not None else ""))
    assert all(v <= 1.0 for v in WORST.values())


DEFECT_CASES = [(d, c) for d in R.HEADS_DEFECTS for c in R.HEADS_BWD_CASES + R.HEADS_FWD_ONLY_CASES[:4]
                if R.defect_applies(d, c) and (d in R.HEADS_FWD_DEFECTS or c in R.HEADS_BWD_CASES)]


def test_every_defect_and_every_output_is_covered():
    assert {d for d, _ in DEFECT_CASES} == set(R.HEADS_DEFECTS)
    touched = {k for d in R.HEADS_DEFECTS for k in R.HEADS_DEFECT_TOUCHES[d][0]}
    assert touched == set(R.FWD_KEYS + R.BWD_KEYS)


@pytest.mark.parametrize("defect,case", DEFECT_CASES, ids=lambda v: v if isinstance(v, str) else R.case_id(v))
def test_defects_bite(defect, case):
    c = R.heads_case(*case)
    tag = f"{R.case_id(case)} defect {defect}"
    keys = R.HEADS_DEFECT_TOUCHES[defect][0]
    if defect in R.HEADS_FWD_DEFECTS:
        good, bad = R.heads_fwd_en(c), R.heads_fwd_en(c, defect=defect)
    else:
        use = R.use_of(R.HEADS_USES[3], case[3])
        acts = R.acts_rounded(R.heads_fwd_ref(c))
        good, bad = R.heads_bwd_en(c, use, acts), R.heads_bwd_en(c, use, acts, defect=defect)
    for k in keys:
        if k in good:
            bites(f"{tag} {k}", good[k].v, bad[k].v, R.gate_of(good[k]))
    for k in set(good) - set(keys):
        assert torch.equal(good[k].v, bad[k].v), (tag, k, "a defect moves only the outputs it names")


# ====================================================================================================== the C side, host only
def test_heads_supported_truth_table():
    sup = _lib.load().pcaa_heads_supported
    for d_in, d_sup, d_head, d_proj in itertools.product((256, 511, 512, 513, 1024), (16, 31, 32, 33, 64), (0, 8, 15, 16, 17, 32),
                                                         (0, 32, 63, 64, 65, 128)):
        want = d_in == 512 and d_sup == 32 and d_head in (0, 16) and d_proj in (0, 64)
        for bwd in (0, 1):
            assert bool(sup(4, 4, d_in, d_sup, d_head, d_proj, bwd)) == want, (d_in, d_sup, d_head, d_proj, bwd)
    for d_head, d_proj in itertools.product((0, 16), (0, 64)):
        for bwd in (0, 1):
            for B, K in ((0, 4), (-1, 4), (4, 0), (4, -1), (0, 0)):
                assert not sup(B, K, 512, 32, d_head, d_proj, bwd), (B, K, bwd)
            assert sup(1, 1, 512, 32, d_head, d_proj, bwd) and sup(64, 8, 512, 32, d_head, d_proj, bwd)
        assert sup(64, 1, 512, 32, d_head, d_proj, 1) and not sup(65, 1, 512, 32, d_head, d_proj, 1)
        assert sup(1, 8, 512, 32, d_head, d_proj, 1) and not sup(1, 9, 512, 32, d_head, d_proj, 1)
        assert sup(65, 70, 512, 32, d_head, d_proj, 0) and sup(130, 9, 512, 32, d_head, d_proj, 0)


INVALID_ARG = 1                 # PCAA_ERR_INVALID_ARG: the launcher returned from its argument checks
FWD_ARGS = ("x4", "W1", "b1", "Wh", "bh", "W2", "b2", "Wg", "bg", "sup_fv", "h", "logits", "hproj")
BWD_ARGS = ("x4", "sup_fv", "h", "logits", "hproj", "W1", "Wh", "W2", "Wg", "d_logits", "d_sup", "d_hproj", "dW1", "db1", "dWh",
            "dbh", "dW2", "db2", "dWg", "dbg", "dx4")
FWD_REQUIRED = ("x4", "W1", "b1", "W2", "b2", "sup_fv", "logits")
BWD_REQUIRED = ("x4", "sup_fv", "logits", "W1", "W2", "dW1", "db1", "dW2", "db2", "dx4")


def _mixed(group):
    """every way to give some but not all of ``group``"""
    return [s for n in range(1, len(group)) for s in itertools.combinations(group, n)]


def test_launchers_refuse_before_any_launch():
    """Host memory stands in for every pointer: an argument check never reads through one, and every call below must
    end in one (return code PCAA_ERR_INVALID_ARG, the message of that check)."""
    lib = _lib.load()
    host = np.zeros(64, dtype=np.float32)
    ptr = (host.ctypes.data + 15) // 16 * 16

    def refused(fn, names, given, B, K, why, odd=()):
        args = [None if n not in given else ptr + (4 if n in odd else 0) for n in names]
        rc = getattr(lib, fn)(*args, B, K, None)
        msg = (lib.pcaa_last_error() or b"").decode()
        assert rc == INVALID_ARG and fn in msg and why in msg, (fn, sorted(set(names) - set(given)), B, K, rc, msg)

    # ---- forward
    for missing in FWD_REQUIRED:
        refused("pcaa_heads_fwd", FWD_ARGS, set(FWD_REQUIRED) - {missing}, 4, 4, "bad args")
    for B, K in ((0, 4), (4, 0), (-3, 4)):
        refused("pcaa_heads_fwd", FWD_ARGS, set(FWD_REQUIRED), B, K, "bad args")
    for some in _mixed(("Wh", "bh", "h")):
        refused("pcaa_heads_fwd", FWD_ARGS, set(FWD_REQUIRED) | set(some), 4, 4, "Wh, bh and h go together")
    for some in _mixed(("Wg", "bg", "hproj")):
        refused("pcaa_heads_fwd", FWD_ARGS, set(FWD_REQUIRED) | set(some), 4, 4, "Wg, bg and hproj go together")
    for odd in ("x4", "W1"):
        refused("pcaa_heads_fwd", FWD_ARGS, set(FWD_ARGS), 4, 4, "16-B aligned", odd=(odd,))
    # ---- backward
    for missing in BWD_REQUIRED:
        refused("pcaa_heads_bwd", BWD_ARGS, set(BWD_REQUIRED) - {missing}, 4, 4, "bad args")
    for B, K in ((65, 8), (64, 9), (0, 4), (4, 0), (1024, 2)):
        refused("pcaa_heads_bwd", BWD_ARGS, set(BWD_ARGS), B, K, "B <= 64 and K <= 8")
    for some in _mixed(("Wh", "h", "dWh", "dbh")):
        refused("pcaa_heads_bwd", BWD_ARGS, set(BWD_REQUIRED) | set(some), 4, 4, "Wh, h, dWh and dbh go together")
    for some in [()] + _mixed(("Wg", "hproj", "dWg", "dbg")):
        refused("pcaa_heads_bwd", BWD_ARGS, set(BWD_REQUIRED) | {"d_hproj"} | set(some), 4, 4, "d_hproj needs")
    refused("pcaa_heads_bwd", BWD_ARGS, set(BWD_ARGS), 4, 4, "16-B aligned", odd=("x4",))
