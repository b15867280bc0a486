"""fp64 restatement of csrc/heads.hip (pcaa_heads_fwd / pcaa_heads_bwd), the gate of every output, the input condition
the gates need, and planted defects.

Used by tests/test_heads_branches.py (the kernels, on the GPU) and tests/test_heads_gates_cpu.py (the gates themselves,
on the CPU).  Plain torch, device-agnostic: a reference runs where its inputs live, in float64.  Inputs come from
``elementwise_ref.uniform``: the same bits on the CPU and on the device.  Kernel and reference get the SAME stored fp32
values, so only the kernel's arithmetic separates them.  u = 2^-24 throughout.

    x4 [B, 512] -> sup_fv = ELU(x4 W1^T + b1) [B, 32] -> h = ELU(sup_fv Wh^T + bh) [B, 16]   (projection head, optional)
                -> logits = ELU((h | sup_fv) W2^T + b2) [B, K];   hproj = ELU(sup_fv Wg^T + bg) [B, 64]   (optional)

Inputs (``heads_case``)
-----------------------
x4 in +-1.7, W1 in +-1.5 / sqrt 512, Wh, Wg in +-2 / sqrt 32, W2 in +-2 / sqrt(its row length), biases in +-0.3, upstream
gradients in +-1.  The condition on the reference, asserted here for every case with B >= 4 and re-checked on the whole case
list by the CPU file: in each of the (up to) four ELU layers the fp64 pre-activations have both signs, a root mean square
inside HEADS_PRE_RMS = [0.25, 2] and no magnitude above HEADS_PRE_MAX = 8 (O(1): neither a layer that is linear for every
row nor one whose ELU' is 1 or 0 everywhere).  A case draws its tensors under successive salts and keeps the first draw that
satisfies it (as ``critic_loss_ref.disc_case`` keeps rows).

Reference (``heads_ref``)
-------------------------
fp64 torch autograd of ELU(x W^T + b) layer by layer; the objective is the sum of <output, upstream gradient> over the
upstream gradients that are present.

Gate
----
The running error analysis of tests/critic_loss_ref.py (``EN``: value, worst-case bound f, sum of squares q; gate
u min(2 f, LAMBDA sqrt q) with that module's LAMBDA = 8; no new number), through the kernels' own expression trees:

* forward (``heads_fwd_en``): sup1 is two chains of 256 fmas (the two k-halves, each from 0) met by one addition, then
  the bias is added (one rounding), then ELU; h, logits and hproj are chains of 32 (16 for the logits behind the
  projection head) fmas that start from the bias, then ELU.
* backward (``heads_bwd_en``): ELU' comes from the STORED output (out > 0 ? 1 : out + 1).  It is 1-Lipschitz in the
  stored value, so it inherits that value's f and q wherever the value is not safely positive (out <= 2 u f_out), and
  adds one rounding of its own (out + 1) where out <= 0.  dl = d_logits ELU'(logits), dg = d_hproj ELU'(hproj): one
  product.  dh = (a chain of K fmas from 0) ELU'(h).  ds starts from d_sup (or 0), then the chain of 16 fmas dh . Wh
  (or K fmas dl . W2), then the chain of 64 fmas dg . Wg, then times ELU'(sup_fv).  dx4 = ds . W1: 32 fmas from 0.
  The bias gradients add the B rows in ascending order in fp32 (B roundings); dW* are chains of B fmas.
* (a) the backward receives the reference's forward values rounded once to fp32: those leaves carry f = |v|, q = v^2
  (``acts_rounded``).  (b) the backward receives the kernel's own forward outputs: the same tree, with those leaves
  carrying the f and q of ``heads_fwd_en`` (``acts_from_fwd``).  No element is excluded from any comparison.

Measured: largest |err| / gate per output over HEADS_CASES (backward: over HEADS_USES and both forms)
--------------------------------------------------------------------------------------------------------
``fp32 restatement`` is the plain-fp32 torch evaluation of the same trees by tests/test_heads_gates_cpu.py, measured on
the CPU; ``kernel`` is csrc/heads.hip against fp64, measured on the device (MI355X) by tests/test_heads_branches.py.

    output     fp32 restatement, measured on the CPU     kernel, measured on the device
               fwd / (a)     (b)                         fwd / (a)     (b)
    sup_fv     0.025                                     0.025
    h          0.019                                     0.019
    logits     0.016                                     0.017
    hproj      0.015                                     0.015
    dx4        0.100         0.047                       0.100         0.047
    dW1        0.265         0.163                       0.344         0.163
    db1        0.202         0.070                       0.249         0.070
    dW2        0.285         0.011                       0.285         0.012
    db2        0.223         0.076                       0.223         0.076
    dWh        0.246         0.013                       0.246         0.016
    dbh        0.203         0.081                       0.203         0.081
    dWg        0.290         0.014                       0.290         0.016
    dbg        0.198         0.102                       0.198         0.102

(The forward figures are small, for the kernel as for the restatement: the rule charges each of a chain's n roundings
against the sum of the magnitudes, and the partial sums of 256 products of mixed sign stay far below it.  The planted
forward defects still move their outputs by hundreds of gates at the least (the CPU file prints each).  (b) is wider than (a) for the weight gradients: the
forward tree's f and q ride on every stored activation.)

Planted defects (``HEADS_DEFECTS``)
-----------------------------------
``defect=`` makes the trees return what a subtly wrong kernel would have produced; HEADS_DEFECT_TOUCHES names the outputs
each one must move (the CPU file: by more than 10 x the gate).

    sup1_half_dropped       only the kh = 0 half of the 512-long dot product reaches sup_fv
    logits_from_sup         the logits are formed from sup_fv[:, :16] although the projection head is on
    w2_pitch_32             W2 [K, 16] is read at pitch 32 (what is read past its end: 0)
    fwd_rows_read_row0      batch rows >= 4 read the x4 rows of workgroup 0 (row r reads row r % 4)
    elu_grad_wrong_side     out > 0 ? out + 1 : 1
    d_sup_not_added         ds starts from 0
    dg_wg_missing           the dg . Wg chain is missing from ds
    bias_last_row_missing   the column sums stop at row B - 2
    slice_next_wg           workgroup i stages W1 and x4 at workgroup i + 1's 32 columns (the last one wraps)
    dwg_rows_48_missing     rows 48..63 of dWg are not written (the destination keeps its zeros)
"""
import functools

import torch

from critic_loss_ref import EN, LAMBDA, add, colsum, en_elu, en_rounded, gate_of, mm, mul, tmm  # noqa: F401
from elementwise_ref import U, moved, ratio, seed_of, uniform  # noqa: F401  (re-exported for the two test files)

D_IN, D_SUP, D_HEAD, D_PROJ = 512, 32, 16, 64
HEADS_PRE_RMS = (0.25, 2.0)
HEADS_PRE_MAX = 8.0
_SALTS = 16

FWD_KEYS = ("sup_fv", "h", "logits", "hproj")
BWD_KEYS = ("dx4", "dW1", "db1", "dW2", "db2", "dWh", "dbh", "dWg", "dbg")
_PARAM_OF = {"dW1": "W1", "db1": "b1", "dW2": "W2", "db2": "b2", "dWh": "Wh", "dbh": "bh", "dWg": "Wg", "dbg": "bg", "dx4": "x4"}

HEADS_DEFECTS = ("sup1_half_dropped", "logits_from_sup", "w2_pitch_32", "fwd_rows_read_row0", "elu_grad_wrong_side",
                 "d_sup_not_added", "dg_wg_missing", "bias_last_row_missing", "slice_next_wg", "dwg_rows_48_missing")
HEADS_FWD_DEFECTS = HEADS_DEFECTS[:4]
# the outputs a defect must move, and what a case needs for the defect to be visible: (outputs, head, proj, min B, min K)
HEADS_DEFECT_TOUCHES = {
    "sup1_half_dropped": (("sup_fv", "h", "logits", "hproj"), True, True, 1, 1),
    "logits_from_sup": (("logits",), True, None, 1, 1),
    "w2_pitch_32": (("logits",), True, None, 1, 2),
    "fwd_rows_read_row0": (("sup_fv", "h", "logits", "hproj"), True, True, 5, 1),
    "elu_grad_wrong_side": (("dx4", "dW1", "db1", "dW2", "db2", "dWh", "dbh", "dWg", "dbg"), True, True, 1, 1),
    "d_sup_not_added": (("dx4", "dW1", "db1"), None, None, 1, 1),
    "dg_wg_missing": (("dx4", "dW1", "db1"), None, True, 1, 1),
    "bias_last_row_missing": (("db1", "db2", "dbh", "dbg"), True, True, 2, 1),
    "slice_next_wg": (("dx4", "dW1"), None, None, 1, 1),
    "dwg_rows_48_missing": (("dWg",), None, True, 1, 1),
}

HEADS_USES = [("d_logits",), ("d_sup",), ("d_hproj",), ("d_logits", "d_sup", "d_hproj"), ()]


def _cases():
    """(B, K, head, proj).  Backward: for each of the four (head, proj) every B of {1, 3, 4, 5, 64} and every K of
    {1, 2, 8} (the pairing rotates with (head, proj), so the four together hold 12 of the 15 (B, K) pairs) plus the two
    corners (1, 1) and (64, 8).  Forward only: B of {65, 130} x K of {9, 70} under every (head, proj)."""
    bwd, fwd = [], []
    for n, (head, proj) in enumerate(((False, False), (False, True), (True, False), (True, True))):
        for i, B in enumerate((1, 3, 4, 5, 64)):
            bwd.append((B, (1, 2, 8)[(i + n) % 3], head, proj))
        bwd += [c for c in ((1, 1, head, proj), (64, 8, head, proj)) if c not in bwd]
        fwd += [(65, 70, head, proj), (130, 9, head, proj), (65 if n % 2 else 130, 9 if n % 2 else 70, head, proj)]
    return bwd, [c for i, c in enumerate(fwd) if c not in fwd[:i]]


HEADS_BWD_CASES, HEADS_FWD_ONLY_CASES = _cases()
HEADS_CASES = HEADS_BWD_CASES + HEADS_FWD_ONLY_CASES


def case_id(c):
    return f"B{c[0]}-K{c[1]}-head{int(c[2])}-proj{int(c[3])}"


def use_of(use, proj):
    """the upstream set a case can take: d_hproj exists only with the decoder head"""
    return tuple(k for k in use if proj or k != "d_hproj")


# ====================================================================================================== inputs, reference
def _draw(B, K, head, proj, salt, device):
    seed = seed_of(B * 7 + K, 2 * int(head) + int(proj) + 10 * salt)
    r = lambda s, a, *shape: uniform(int(torch.Size(shape).numel()), seed + s, device, -a, a).view(*shape).float().contiguous()
    din2 = D_HEAD if head else D_SUP
    c = {"x4": r(0, 1.7, B, D_IN), "W1": r(1, 1.5 / D_IN ** 0.5, D_SUP, D_IN), "b1": r(2, 0.3, D_SUP),
         "W2": r(3, 2.0 / din2 ** 0.5, K, din2), "b2": r(4, 0.3, K),
         "d_logits": r(9, 1.0, B, K), "d_sup": r(10, 1.0, B, D_SUP)}
    if head:
        c.update(Wh=r(5, 2.0 / D_SUP ** 0.5, D_HEAD, D_SUP), bh=r(6, 0.3, D_HEAD))
    if proj:
        c.update(Wg=r(7, 2.0 / D_SUP ** 0.5, D_PROJ, D_SUP), bg=r(8, 0.3, D_PROJ), d_hproj=r(11, 1.0, B, D_PROJ))
    return c


def _elu(a):
    return torch.where(a > 0, a, torch.expm1(a))


def _forward64(c, lv=None):
    """-> (outputs dict, pre-activations dict) in fp64 from the leaves ``lv`` (default: the case's tensors cast up)"""
    p = {k: v.double() for k, v in c.items()} if lv is None else lv
    pre = {"sup_fv": p["x4"] @ p["W1"].t() + p["b1"]}
    out = {"sup_fv": _elu(pre["sup_fv"])}
    last = out["sup_fv"]
    if "Wh" in p:
        pre["h"] = out["sup_fv"] @ p["Wh"].t() + p["bh"]
        last = out["h"] = _elu(pre["h"])
    pre["logits"] = last @ p["W2"].t() + p["b2"]
    out["logits"] = _elu(pre["logits"])
    if "Wg" in p:
        pre["hproj"] = out["sup_fv"] @ p["Wg"].t() + p["bg"]
        out["hproj"] = _elu(pre["hproj"])
    return out, pre


def pre_condition(c):
    """-> (holds, {layer: (has both signs, rms, max |pre|)}) on the fp64 reference"""
    _, pre = _forward64(c)
    info = {k: (bool((a > 0).any()) and bool((a < 0).any()), float((a * a).mean().sqrt()), float(a.abs().max()))
            for k, a in pre.items()}
    ok = all(s and HEADS_PRE_RMS[0] <= r <= HEADS_PRE_RMS[1] and m <= HEADS_PRE_MAX for s, r, m in info.values())
    return ok, info


@functools.lru_cache(maxsize=None)
def heads_case(B, K, head, proj, device="cpu"):
    """the case's fp32 tensors (a dict; shared between the tests: read only).  B >= 4: the first draw that satisfies the
    input condition, asserted; smaller batches (too few pre-activations to ask for both signs) take the first draw"""
    if B < 4:
        return _draw(B, K, head, proj, 0, device)
    for salt in range(_SALTS):
        c = _draw(B, K, head, proj, salt, device)
        if pre_condition(c)[0]:
            return c
    raise AssertionError(f"heads_case {(B, K, head, proj)}: no draw keeps every layer's pre-activations O(1) with both signs")


def _leaf_names(c):
    return [k for k in ("x4", "W1", "b1", "Wh", "bh", "W2", "b2", "Wg", "bg") if k in c]


def heads_fwd_ref(c):
    """fp64 outputs {sup_fv, h, logits, hproj} (detached; absent heads are absent)"""
    return {k: v.detach() for k, v in _forward64(c)[0].items()}


def heads_bwd_ref(c, use):
    """``use``: which of d_logits, d_sup, d_hproj are present -> dict of fp64 gradients (BWD_KEYS that exist for the case;
    dWg / dbg only when d_hproj is present, as the kernel returns them)"""
    names = _leaf_names(c)
    lv = {k: c[k].detach().double().clone().requires_grad_(True) for k in names}
    out, _ = _forward64(c, lv)
    tot = out["sup_fv"].sum() * 0.0
    for up, o in (("d_logits", "logits"), ("d_sup", "sup_fv"), ("d_hproj", "hproj")):
        if up in use:
            tot = tot + (out[o] * c[up].double()).sum()
    g = dict(zip(names, torch.autograd.grad(tot, [lv[k] for k in names], allow_unused=True)))
    res = {}
    for key in BWD_KEYS:
        nm = _PARAM_OF[key]
        if nm not in lv or (nm in ("Wg", "bg") and "d_hproj" not in use):
            continue
        res[key] = torch.zeros_like(lv[nm]) if g[nm] is None else g[nm]
    return res


# ====================================================================================================== the kernels' trees
def _row(b):
    return EN(b.v.view(1, -1), b.f.view(1, -1), b.q.view(1, -1))


def _bad_pitch(W2):
    """W2 [K, 16] stored at pitch 16, rows read at pitch 32 (what is read past the end: 0)"""
    K, n = W2.shape
    flat = torch.cat([W2.reshape(-1), torch.zeros(K * n, dtype=W2.dtype, device=W2.device)])
    idx = torch.arange(K, device=W2.device).view(K, 1) * (2 * n) + torch.arange(n, device=W2.device).view(1, n)
    return flat[idx]


def heads_fwd_en(c, dtype=torch.float64, defect=None):
    """heads_fwd_kernel's expression tree -> {sup_fv, h, logits, hproj} as EN nodes (dtype float32: a plain fp32 evaluation)"""
    e = {k: EN(v.to(dtype)) for k, v in c.items()}
    head, proj = "Wh" in c, "Wg" in c
    x = e["x4"]
    if defect == "fwd_rows_read_row0":
        x = EN(x.v[torch.arange(x.v.shape[0], device=x.v.device) % 4])
    half = D_IN // 2
    lo = mm(x[:, :half], e["W1"][:, :half].T, n=half)
    hi = mm(x[:, half:], e["W1"][:, half:].T, n=half)
    acc = lo if defect == "sup1_half_dropped" else add(lo, hi)
    out = {"sup_fv": en_elu(add(acc, _row(e["b1"])))[0]}
    sup = last = out["sup_fv"]
    if head:
        last = out["h"] = en_elu(mm(sup, e["Wh"].T, n=D_SUP, bias=_row(e["bh"])))[0]
    W2 = e["W2"]
    if head and defect == "w2_pitch_32":
        W2 = EN(_bad_pitch(W2.v))
    if head and defect == "logits_from_sup":
        last = sup[:, :D_HEAD]
    out["logits"] = en_elu(mm(last, W2.T, n=D_HEAD if head else D_SUP, bias=_row(e["b2"])))[0]
    if proj:
        out["hproj"] = en_elu(mm(sup, e["Wg"].T, n=D_SUP, bias=_row(e["bg"])))[0]
    return out


def acts_rounded(fwd_ref):
    """form (a): the reference's forward values, rounded once to fp32 on their way to the kernel"""
    return {k: en_rounded(v) for k, v in fwd_ref.items()}


def acts_from_fwd(c):
    """form (b): the forward kernel's own outputs -- the reference's values with the forward tree's f and q"""
    return heads_fwd_en(c)


def _elu_grad_from_out(out, wrong_side=False):
    """out > 0 ? 1 : out + 1 of a stored ELU output (module docstring)"""
    v = out.v
    pos = v > 0
    one = torch.ones_like(v)
    g = torch.where(pos, v + 1, one) if wrong_side else torch.where(pos, one, v + 1)
    inherits = (v <= 2 * U * out.f).to(v.dtype)
    own = torch.where(pos, torch.zeros_like(v), g.abs())
    return EN(g, inherits * out.f + own, inherits * out.q + own ** 2)


def heads_bwd_en(c, use, acts, dtype=torch.float64, defect=None):
    """heads_bwd_kernel's expression tree.  ``acts``: the stored forward outputs the kernel receives, as EN nodes
    (``acts_rounded`` / ``acts_from_fwd``; an fp32 evaluation passes EN(fp32 values)) -> dict of EN nodes, keys as
    ``heads_bwd_ref``"""
    e = {k: EN(v.to(dtype)) for k, v in c.items()}
    head = "Wh" in c
    proj = "Wg" in c and "d_hproj" in use
    B = c["x4"].shape[0]
    K = c["W2"].shape[0]
    dev = c["x4"].device
    zeros = lambda *s: EN(torch.zeros(s, dtype=dtype, device=dev))
    eg = lambda k: _elu_grad_from_out(acts[k], defect == "elu_grad_wrong_side")
    sup = acts["sup_fv"]
    dl = mul(e["d_logits"], eg("logits")) if "d_logits" in use else zeros(B, K)
    acc = e["d_sup"] if ("d_sup" in use and defect != "d_sup_not_added") else zeros(B, D_SUP)
    if head:
        dh = mul(mm(dl, e["W2"], n=K), eg("h"))
        acc = mm(dh, e["Wh"], n=D_HEAD, bias=acc)
    else:
        acc = mm(dl, e["W2"], n=K, bias=acc)
    if proj:
        dg = mul(e["d_hproj"], eg("hproj"))
        if defect != "dg_wg_missing":
            acc = mm(dg, e["Wg"], n=D_PROJ, bias=acc)
    ds = mul(acc, eg("sup_fv"))
    W1, x4 = e["W1"], e["x4"]
    if defect == "slice_next_wg":
        W1, x4 = EN(W1.v.roll(-32, dims=1)), EN(x4.v.roll(-32, dims=1))
    rows = (lambda a: a[: B - 1]) if defect == "bias_last_row_missing" else (lambda a: a)
    out = {"dx4": mm(ds, W1, n=D_SUP), "dW1": tmm(ds, x4, n=B), "db1": colsum(rows(ds), n=B),
           "dW2": tmm(dl, acts["h"] if head else sup, n=B), "db2": colsum(rows(dl), n=B)}
    if head:
        out["dWh"], out["dbh"] = tmm(dh, sup, n=B), colsum(rows(dh), n=B)
    if proj:
        out["dWg"], out["dbg"] = tmm(dg, sup, n=B), colsum(rows(dg), n=B)
        if defect == "dwg_rows_48_missing":
            w = out["dWg"]
            keep = (torch.arange(D_PROJ, device=dev) < 48).to(dtype).view(-1, 1)
            out["dWg"] = EN(w.v * keep, w.f, w.q)
    return out


def defect_applies(defect, case):
    """whether ``defect`` can show at ``case`` (HEADS_DEFECT_TOUCHES)"""
    B, K, head, proj = case
    _, need_head, need_proj, min_b, min_k = HEADS_DEFECT_TOUCHES[defect]
    return (need_head is None or head == need_head) and (need_proj is None or proj == need_proj) and B >= min_b and K >= min_k
