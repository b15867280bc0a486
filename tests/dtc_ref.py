"""fp64 restatements of the fused temporal convolution of csrc/dtc_fused.hip (forward, adjoint, the two-sequence "pair"
kernels, windowed sources), the gate of each output, the dispatch as plain Python, the case lists and planted defects.

Used by tests/test_dtc_branches.py (the kernels, on the GPU) and tests/test_dtc_gates_cpu.py (the gates, the coverage and
the input conditions, on the CPU).  Plain torch, device-agnostic.  ``uniform``, ``sum_gate``, ``ratio``, ``moved``, ``U``,
``BF16_ROUND`` and the ELU / ELU' gates come from tests/elementwise_ref.py; the fp32-accumulator gate (``acc_ref`` /
``acc_gate``) and the statistical carried form from tests/gemm_ref.py.  (``operand`` / ``logical`` of gemm_ref lay a matrix
out with a leading dimension and 64 NaN elements behind it; the temporal entry points take contiguous tensors and want whole
NaN ROWS on both sides, so the GPU file places its operands itself: ``nan_op`` there.)

The operation
-------------
forward   y[b,t,co]  = sum_{ci,tap} W[co, ci*3+tap] a[b, t-(2-tap)d, ci]       rows < 0 are zero
          a = ELU(scale src + shift), or src where scale is null;  col[(b,t), ci*3+tap] = a[b, t-(2-tap)d, ci]
adjoint   da[b,t,ci] = sum_{co,tap} dy[b, t+(2-tap)d, co] W[co, ci*3+tap]      rows >= T are zero
          dy given, or formed as c0 dz + c1 y + c2 (and written out as dy_out)
epilogue  dz_below = da ELU'(ep_y scale + shift), statistics {sum dz_below, sum dz_below (ep_y - mean) rstd}
Both are one contraction over n = 3 kc terms, kc = the contraction channels (forward cin, adjoint cout): ``im2col`` lays
the shifted rows out as X [B T, 3 kc] (column tap kc + c), ``wmat`` the weights as [nc, 3 kc], and the product is X Wm^T.
ksplit > 1: split z owns channels [z per_z, min(kc, (z+1) per_z)), per_z = ceil(chunks / ksplit) 32, chunks = ceil(kc / 32);
the range may be empty and its slab is then exactly zero.  Source rows: plain b T + t; windowed win_row[b] + t (modulo
ring_rows when > 0); segmented: base = (win_row[b] // ring_rows) ring_rows, row base + (win_row[b] - base + t) % ring_rows.

Gates, u = 2^-24, per output element
------------------------------------
* fp32 kernels: the fp32-accumulator gate of gemm_ref over n = 3 kc terms with every product rounding (c_n = 2 n), plus
  sum_k |w_k| gate(a_k), gate(a_k) the error of the staged operand: the ELU gate of elementwise_ref (ELU_STAGE_C u (T + [z<=0])
  + [z<=0] u |z|) for an activated forward operand, DY_C u (|c0 dz| + |c1 y| + |c2|) for a formed dy, zero for an operand
  used as stored.
* DY_C = 8.  CHANGED from the issue's 3: the three roundings that 3 u (...) counts are the worst case itself, so an
  evaluation that realises it sits at the whole gate, not at half: the fp32 torch evaluation (k0 dz + k1 y) + k2 of the CPU
  file reached 0.82 of the gate with 3 (dy_out of the (47,2,512,128,1) adjoint; 0.77 at (3,32,48,36,4)) and 0.31 with 8.  8 is the constant elementwise_ref uses for
  the same expression (``bn_bwd_dy``), for the same reason.
* ELU on load (``elu_stage``: a degree-6 polynomial on |z| < 0.25, __expf(z) - 1 elsewhere): ELU_STAGE_C = 4, the gate of
  ``bn_act_fwd`` unchanged; the GPU file prints the ratio of the col output (the activation alone) against fp64.
* bf16 kernels: the reference rounds the fp64 operands to bf16 (the weights always, the staged tile after the activation /
  after dy is formed); products are then exact, c_n = n - 1.  A staged element whose rounding interval straddles a bf16
  boundary (round(a - gate(a)) != round(a + gate(a))) adds |w16_k| |hi16 - lo16| to the outputs it feeds.  dy_out and col
  are fp32 by contract: the fp32 operand gate.
* epilogue: the fused-dgrad gate of gemm_ref, (gate(da) + |da| (rel_e + 2u)) e.
* statistics: fp32 inside a workgroup's slice of rows, fp64 atomics across.  ``sum_gate`` per slice with the kernel's row
  lanes, plus the summands' own errors in the statistical form of gemm_ref (min of the added worst cases and C_STAT u
  sqrt(sum n P2)).  CHANGED from the issue's form ("the summands' errors carried in the statistical form"): the staged
  operands' part of a summand's gate -- sum_k |w_k| gate(a_k) and the bf16 flip term -- is added up on top instead (``extra``
  of ``stat_sums``).  A flipped rounding of one staged element moves up to three rows of every column by its whole term, one
  way: a bias, not rounding noise, and the sqrt branch of the min drops it.  Measured without a kernel, against the fp64
  reference: the CPU file rounds the bf16 operands from a +- gate(a), where a staged fp32 value may sit; the 4 flips this
  realises in the (3,32,48,36,4) epilogue adjoint put its statistics at 53.3 x the issue's form (forward (3,32,36,48,4): 130 x,
  2 flips) and at 0.98 of the gate as it is now.  Slices, lanes and the replica a slice lands in, read from the kernels:
      one-sequence fp32  slice = one sequence, row r on lane r % 8 (lanes met in fp64),      replica b % nrep
      one-sequence bf16  slice = one sequence, row r on lane (r >> 2) & 1 (the half-wave),   replica b % nrep
      pair, 32 columns   slice = the pair's two sequences, row r of either on lane r % 8,    replica (b // 2) % nrep
      pair, 64 columns   slice = one sequence, lane (r >> 2) & 1,                            replica (b // 2) % nrep
  Compared per replica and summed over the replicas.
* slabs: each its own product gate over its own range; the reduced output adds ks u sum |slab| (``splitk_reduce``).
No output element is left out of a comparison.

Planted defects: ``DEFECTS``; ``defect=`` of a reference returns what a subtly wrong kernel would have produced.
"quad_not_reloaded" restates the pair kernels' staging: thread tid handles the quads q = tid + 256 i of the pass's 2 T rows
x q4 = kr / 4 quads, quad q being (pair row R = q // q4, channel quad cq = q % q4); its first quad's channel quad is
cq0 = tid % q4, and without the reload every later quad takes the vectors of channels 4 cq0 .. 4 cq0 + 3.
"""
import torch

import elementwise_ref as E
import gemm_ref as G
from elementwise_ref import BF16_ROUND, U, moved, ratio, sum_gate, uniform  # noqa: F401  (re-exported)
from gemm_ref import C_STAT

BF = torch.bfloat16
ROWS, CC, MAX_CR, DG_MAX_CR, PAIR_KC = 32, 32, 256, 512, 256
ELU_STAGE_C = 4.0
DY_C = 8.0
SENTINEL = -12345.671875            # exact in fp32
ROUTES = ("one_f32", "one_bf16", "pair32_f32", "pair32_bf16", "pair64_f32", "pair64_bf16")   # PCAA_DTC_ROUTE_*
FORMS = ("given", "formed", "formed+dy_out", "formed+dy_out+epilogue")

DEFECTS = {  # name: (list, case id, bf16, the output it is judged on)
    "taps_reversed": ("fwd", "pair32_odd_quads", False, "y"),
    "tap_shift": ("adj", "pair32_odd_quads", False, "out"),
    "edge_neighbour": ("fwd", "2d_ge_T", False, "y"),
    "edge_neighbour_adj": ("adj", "2d_ge_T", True, "out"),
    "drop_last_chunk": ("fwd", "t32_w36", True, "y"),
    "pass2_stale": ("fwd", "two_pass", False, "y"),
    "pass2_stale_adj": ("adj", "two_pass", True, "out"),
    "quad_not_reloaded": ("fwd", "pair32_odd_quads", True, "y"),
    "quad_not_reloaded_adj": ("adj", "pair32_odd_quads", False, "out"),
    "pair_second_gets_first": ("fwd", "pair64_edge", False, "y"),
    "odd_last_missing": ("adj", "pair64_edge", True, "out"),
    "empty_split_unwritten": ("fwd", "ks8_empty", False, "slab7"),
    "ring_wrap_off_by_one": ("win", "ring_gt_T/pair_shape", False, "y"),
    "seg_wraps_into_next": ("win", "segmented/w36", True, "y"),
    "c2_dropped": ("adj", "t32_w36/formed", False, "out"),
    "epilogue_cols_local": ("adj", "t32_w36/formed+dy_out+epilogue", False, "out"),
    "stats_rows_lt16": ("fwd", "t32_w36", False, "stats"),
    "stats_wrong_replica": ("adj", "pair32_odd_quads", True, "stats"),
    "f32_on_bf16": ("fwd", "wg2", False, "y"),
}


def cdiv(a, b):
    return -(-a // b)


def rb(x):
    """fp64 -> the nearest bf16, as fp64"""
    return x.to(BF).double()


# ------------------------------------------------------------------------------------------------ dispatch, restated
def pair_takes(kc, nc, ksplit, adj, switch="both"):
    on = {"both": True, "0": False, "fwd": not adj, "adj": adj}[switch]
    return on and ksplit == 1 and kc >= 128 and kc % CC == 0 and nc >= 64 and nc % 4 == 0


def wide(B, nc):
    return (B + 1) // 2 * (nc // 64) >= 192 and nc % 64 == 0


def route(adj, bf16, B, cin, cout, ksplit=1, windowed=False, switch="both"):
    """the restatement of pcaa_dtc_conv_route -> an index into ROUTES"""
    kc, nc = (cout, cin) if adj else (cin, cout)
    fam = 0
    if not windowed and pair_takes(kc, nc, ksplit, adj, switch):
        fam = 2 if wide(B, nc) else 1
    return fam * 2 + int(bool(bf16))


def supported(T, cin, cout):
    return int(1 <= T <= ROWS and cin >= 4 and cin % 4 == 0 and cout >= 16 and cout % 16 == 0)


def fwd_ksplit(B, cin, cout):
    chunks = cdiv(cin, CC)
    ks = cdiv(cin, MAX_CR)
    if B * cdiv(cout, 32) <= 128 and chunks >= 16:
        ks = max(ks, 8)
    return min(ks, chunks)


def dgrad_ksplit(B, cin, cout):
    return max(1, cdiv(cout, DG_MAX_CR))


def grid():
    """(B, cin, cout) with both sides of every boundary of the predicates"""
    Bs = (1, 2, 4, 8, 9, 45, 47, 64, 383)
    cins = (4, 32, 96, 128, 132, 160, 256, 260, 288, 480, 512, 516, 544, 1024, 2080, 2304, 2560)
    couts = (16, 32, 48, 64, 80, 128, 256, 512, 516, 1024)
    # (2, 128, 66): forward nc % 4 != 0 with every other condition of pair_takes true -- no entry point accepts it, the route
    # function takes any integers; (383, 128, 80): >= 192 workgroups with nc % 64 != 0
    return [(B, ci, co) for B in Bs for ci in cins for co in couts] + [(2, 128, 66), (383, 128, 80)]


def split_ranges(kc, ks):
    per_z = cdiv(cdiv(kc, CC), ks) * CC
    return [(min(kc, z * per_z), min(kc, (z + 1) * per_z)) for z in range(ks)]


def family(c, bf16, switch="both"):
    """'one' / 'pair32' / 'pair64' of a case"""
    r = route(c["adj"], bf16, c["B"], c["cin"], c["cout"], c["ks"], c.get("win") is not None, switch)
    return ("one", "pair32", "pair64")[r // 2]


def tile_cols(fam, bf16):
    return {"one": 128 if bf16 else 32, "pair32": 32, "pair64": 64}[fam]


# ------------------------------------------------------------------------------------------------ cases
def _c(id, adj, B, T, cin, cout, d, fam, **kw):
    c = dict(id=id, adj=adj, B=B, T=T, cin=cin, cout=cout, d=d, fam=fam, act=False, col=False, ks=1, stride_pad=0, nrep=3,
             form=0, only=None, poison=False)
    c.update(kw)
    c["kc"], c["nc"] = (cout, cin) if adj else (cin, cout)
    c["stats"] = (c["ks"] == 1) if not adj else c["form"] == 3
    return c


def fwd_cases():
    f = lambda id, *a, **kw: _c(id, False, *a, **kw)
    return [
        f("t1", 1, 1, 4, 16, 1, "one", col=True, nrep=1),
        f("t32_w36", 3, 32, 36, 48, 4, "one", act=True, col=True, poison=True),
        f("d_ge_T", 2, 5, 32, 32, 7, "one", act=True, nrep=4),
        f("2d_ge_T", 2, 5, 32, 32, 3, "one", col=True),
        f("wg2", 2, 9, 96, 144, 2, "one", act=True, col=True),
        f("takes_cout48", 2, 6, 128, 48, 1, "one", act=True),
        f("takes_cout64", 2, 6, 128, 64, 1, "pair32", col=True),
        f("takes_cin96", 3, 6, 96, 64, 1, "one", col=True),
        f("takes_cin132", 2, 6, 132, 64, 1, "one", act=True),
        f("pair32_odd_quads", 3, 7, 160, 80, 2, "pair32", act=True, col=True),
        f("two_pass", 2, 30, 288, 64, 1, "pair32", act=True),
        f("two_pass_512", 1, 3, 512, 64, 2, "pair32", act=True, col=True, nrep=1),
        f("pair64_edge", 47, 4, 128, 512, 1, "pair64", nrep=26),
        f("pair64_under", 45, 4, 128, 512, 1, "pair32", act=True),
        f("pair64_two_pass", 47, 2, 320, 512, 1, "pair64", act=True, col=True),
        f("ks8_empty", 2, 6, 544, 16, 1, "one", ks=8, act=True, lib_ks=True),
        f("ks8_1024", 2, 30, 1024, 16, 1, "one", ks=8, lib_ks=True),
        f("ks3_one_chunk", 2, 9, 96, 32, 2, "one", ks=3, act=True, stride_pad=52),
        f("ks2_uneven_col", 2, 9, 160, 32, 2, "one", ks=2, act=True, col=True),
    ]


def adj_cases():
    a = lambda id, *x, **kw: _c(id, True, *x, **kw)
    out = [a("t1", 1, 1, 4, 4, 1, "one", form=0)]
    out += [a("t32_w36/" + FORMS[f], 3, 32, 48, 36, 4, "one", form=f, poison=True) for f in range(4)]
    out += [
        a("d_ge_T", 2, 5, 32, 32, 7, "one", form=1),
        a("2d_ge_T", 2, 5, 32, 32, 3, "one", form=2),
        a("wg2", 2, 9, 144, 96, 2, "one", form=3, nrep=4),
        a("takes_cin48", 2, 6, 48, 128, 1, "one", form=0),
        a("takes_cin64", 2, 6, 64, 128, 1, "pair32", form=1),
        a("takes_cout96", 3, 6, 64, 96, 1, "one", form=2),
        a("takes_cout132", 2, 6, 64, 132, 1, "one", form=3, nrep=1),
        a("pair32_odd_quads", 3, 7, 80, 160, 2, "pair32", form=3),
        a("two_pass", 2, 30, 64, 288, 1, "pair32", form=1),
        a("two_pass_512", 1, 3, 64, 512, 2, "pair32", form=3, nrep=1),
        a("three_pass_544", 1, 3, 64, 544, 2, "pair32", form=1),
        a("pair64_edge", 47, 4, 512, 128, 1, "pair64", form=0),
        a("pair64_under", 45, 4, 512, 128, 1, "pair32", form=2),
        a("pair64_two_pass", 47, 2, 512, 320, 1, "pair64", form=1),
        a("pair64_epilogue", 47, 2, 512, 128, 1, "pair64", form=3, nrep=26),
        a("ks2_1024", 2, 6, 16, 1024, 1, "one", ks=2, form=2, lib_ks=True),
        a("ks4_empty", 2, 9, 32, 160, 2, "one", ks=4, form=2, stride_pad=20),
        a("ks3_one_chunk", 2, 9, 32, 96, 2, "one", ks=3, form=2),
    ]
    return out


WINDOW_SHAPES = {"pair_shape": (4, 6, 256, 64, 2), "lib_ks": (3, 30, 1024, 16, 1), "w36": (2, 32, 36, 48, 4)}


def window_cases():
    out = []
    for sname, (B, T, cin, cout, d) in WINDOW_SHAPES.items():
        ks = fwd_ksplit(B, cin, cout)
        for kind in ("plain_overlap", "ring_eq_T", "ring_gt_T", "segmented"):
            if kind == "plain_overlap":
                table_rows, ring, seg = T + B + 1, 0, 0
                rows = [min(2 * b, table_rows - T) for b in range(B)]
                rows[-1] = table_rows - T
            elif kind == "ring_eq_T":
                table_rows, ring, seg = T, T, 0
                rows = [(b * (T - 1)) % T for b in range(B)]
            elif kind == "ring_gt_T":
                ring, seg = T + 3, 0
                table_rows = ring + 2
                rows = ([ring - 1, 0, 4, ring - 2] * B)[:B]
            else:
                ring, seg = T + 2, 3
                table_rows = ring * seg
                rows = ([ring - 1, ring, 2 * ring + 3, 2 * ring - 2] * B)[:B]
            out.append(_c(f"{kind}/{sname}", False, B, T, cin, cout, d, "one", act=True, ks=ks, lib_ks=True, poison=(sname == "w36"),
                          win=dict(kind=kind, rows=rows, table_rows=table_rows, ring=ring, seg=seg)))
            out[-1]["stats"] = False
    return out


def case_of(which, id):
    return next(c for c in {"fwd": fwd_cases, "adj": adj_cases, "win": window_cases}[which]() if c["id"] == id)


# reason -> (entry point, the arguments changed from a valid small call, a fragment of the PCAA_CHECK_ARG message)
REFUSALS = {
    "fwd_null_src": ("fwd", dict(null=["src"]), "pcaa_dtc_conv_fwd: bad args"),
    "fwd_T33": ("fwd", dict(T=33), "pcaa_dtc_conv_fwd: needs T <="),
    "fwd_cin6": ("fwd", dict(cin=6), "pcaa_dtc_conv_fwd: needs T <="),
    "fwd_cout24": ("fwd", dict(cout=24), "pcaa_dtc_conv_fwd: needs T <="),
    "fwd_scale_without_shift": ("fwd", dict(null=["shift"]), "scale and shift go together"),
    "fwd_nrep0": ("fwd", dict(nrep=0), "pcaa_dtc_conv_fwd: nrep"),
    "fwd_misaligned": ("fwd", dict(misalign="src"), "must be 16-B aligned"),
    "fwd_ksplit_gt_chunks": ("fwd", dict(ks=2, stats=False), "pcaa_dtc_conv_fwd: ksplit must keep <="),
    "fwd_over_256_channels": ("fwd", dict(cin=288), "pcaa_dtc_conv_fwd: ksplit must keep <="),
    "fwd_stats_with_ksplit": ("fwd", dict(cin=64, ks=2), "ksplit > 1 writes slabs (no statistics)"),
    "fwd_slab_stride_small": ("fwd", dict(cin=64, ks=2, stats=False, stride=-1), "ksplit > 1 writes slabs (no statistics)"),
    "win_col": ("win", dict(col=True), "pcaa_dtc_conv_fwd_win: eval form only"),
    "win_stats": ("win", dict(stats=True), "pcaa_dtc_conv_fwd_win: eval form only"),
    "win_ring_below_T": ("win", dict(ring=3), "pcaa_dtc_conv_fwd_win: needs win_row"),
    "win_ring_over_table": ("win", dict(ring=1000), "pcaa_dtc_conv_fwd_win: needs win_row"),
    "seg_n_seg0": ("seg", dict(n_seg=0), "pcaa_dtc_conv_fwd_seg: needs win_row"),
    "adj_null_W": ("adj", dict(null=["W"]), "pcaa_dtc_conv_dgrad: bad args"),
    "adj_dy_and_dz": ("adj", dict(both=True), "either dy, or dz + y + coef"),
    "adj_neither": ("adj", dict(null=["dy"]), "either dy, or dz + y + coef"),
    "adj_T33": ("adj", dict(T=33), "pcaa_dtc_conv_dgrad: needs T <="),
    "adj_misaligned": ("adj", dict(misalign="dy"), "pcaa_dtc_conv_dgrad: 16-B alignment"),
    "adj_ksplit_gt_chunks": ("adj", dict(ks=2), "pcaa_dtc_conv_dgrad: ksplit must keep <="),
    "adj_over_512_channels": ("adj", dict(cout=544), "pcaa_dtc_conv_dgrad: ksplit must keep <="),
    "adj_slab_stride_small": ("adj", dict(cout=64, ks=2, stride=-1), "pcaa_dtc_conv_dgrad: slab_stride >="),
    "adj_epilogue_with_ksplit": ("adj", dict(cout=64, ks=2, ep=True), "the epilogue needs ksplit == 1"),
    "adj_epilogue_missing_vector": ("adj", dict(ep=True, null=["ep_mean"]), "the epilogue needs ksplit == 1"),
}


# ------------------------------------------------------------------------------------------------ inputs
def seed_of(c, which):
    return 1 + (c["B"] * 7919 + c["T"] * 4099 + c["cin"] * 31 + c["cout"] * 131 + c["d"] * 17 + which * 1009 + c["adj"] * 7) % 1000003


def inputs(c, device="cpu"):
    """the fp32 operands of a case (the logical tensors; the GPU file places them inside NaN-filled allocations)"""
    B, T, cin, cout, kc, nc = c["B"], c["T"], c["cin"], c["cout"], c["kc"], c["nc"]
    rows = B * T
    amp = 3.0 ** 0.5
    inp = {"W": uniform(cout * cin * 3, seed_of(c, 0), device, -1.0, 1.0).mul((3.0 / (3 * kc)) ** 0.5 * amp).view(cout, cin * 3).float()}
    if not c["adj"]:
        w = c.get("win")
        n = w["table_rows"] if w else rows
        inp["src"] = uniform(n * cin, seed_of(c, 1), device, -amp, amp).view(n, cin).float()
        if c["act"]:
            inp["scale"], inp["shift"], _, _ = E.bn_vectors(cin, seed_of(c, 2), device)
        return inp
    if c["form"] == 0:
        inp["dy"] = uniform(rows * cout, seed_of(c, 1), device, -amp, amp).view(rows, cout).float()
    else:
        inp["dz"] = uniform(rows * cout, seed_of(c, 1), device, -amp, amp).view(rows, cout).float()
        inp["y"] = uniform(rows * cout, seed_of(c, 3), device, -amp, amp).view(rows, cout).float()
        inp["coef"] = E.coef_vectors(cout, seed_of(c, 4), device)
    if c["form"] == 3:
        inp["ep_y"] = uniform(rows * cin, seed_of(c, 5), device, -amp, amp).view(rows, cin).float()
        inp["ep_scale"], inp["ep_shift"], inp["ep_mean"], inp["ep_rstd"] = E.bn_vectors(cin, seed_of(c, 6), device)
    return inp


def window_rows(c, defect=None):
    """[B, T] table rows of a windowed case (python ints -> a list of lists)"""
    w, T = c["win"], c["T"]
    out = []
    for r0 in w["rows"]:
        seq = []
        for t in range(T):
            if w["seg"]:
                base = r0 // w["ring"] * w["ring"]
                row = base + (r0 - base + t) % w["ring"]
                if defect == "seg_wraps_into_next":
                    row = r0 + t
            elif w["ring"]:
                row = (r0 % w["ring"] + t)
                if row >= w["ring"]:
                    row = row - w["ring"] + (1 if defect == "ring_wrap_off_by_one" else 0)
            else:
                row = r0 + t
            seq.append(row)
        out.append(seq)
    return out


def materialise(c, inp, defect=None):
    idx = torch.tensor(window_rows(c, defect), device=inp["src"].device).view(-1)
    return inp["src"][idx]


# ------------------------------------------------------------------------------------------------ the contraction
def shifted(a, T, sh, adj, neighbour=False):
    """a [B*T, k] -> row (b, t) holds row t + sh (adjoint) or t - sh (forward) of its sequence, zero outside it"""
    n = a.shape[0]
    r = torch.arange(n, device=a.device)
    t = r % T
    src = r + sh if adj else r - sh
    ok = (src >= 0) & (src < n) if neighbour else ((t + sh < T) if adj else (t - sh >= 0))
    return a[src.clamp(0, n - 1)] * ok.view(-1, 1).to(a.dtype)


def im2col(a, T, d, adj, defect=None):
    """-> X [B*T, 3 k], column tap * k + c"""
    cols = []
    for tap in range(3):
        sh = (2 - tap) * d
        if defect == "tap_shift" and tap == 0:
            sh = (1 - tap) * d
        cols.append(shifted(a, T, sh, adj, defect == "edge_neighbour"))
    return torch.cat(cols, 1)


def wmat(W, cin, cout, adj, defect=None):
    """W [cout, cin*3] (k = ci*3 + tap) -> [nc, 3 kc] with column tap * kc + c"""
    w = W.double().view(cout, cin, 3)
    if defect == "taps_reversed":
        w = w.flip(2)
    return (w.permute(1, 2, 0).reshape(cin, 3 * cout) if adj else w.permute(0, 2, 1).reshape(cout, 3 * cin)).contiguous()


def col_layout(X, k):
    """X [rows, 3 k] (tap-major) -> the col matrix [rows, k*3], column c*3 + tap"""
    return X.view(X.shape[0], 3, k).permute(0, 2, 1).reshape(X.shape[0], 3 * k)


def _quad_map(c, B, T, kc, device):
    """[B*T, kc] channel whose vectors the element takes when the per-quad reload is missing (module docstring)"""
    b = torch.arange(B, device=device).view(B, 1, 1)
    t = torch.arange(T, device=device).view(1, T, 1)
    ch = torch.arange(kc, device=device).view(1, 1, kc)
    k0 = ch // PAIR_KC * PAIR_KC
    q4 = (kc - k0).clamp_max(PAIR_KC) // 4
    q = ((b % 2) * T + t) * q4 + (ch - k0) // 4
    return (k0 + 4 * ((q % 256) % q4) + ch % 4).view(B * T, kc)


def _vectors(c, vs, defect, B, T, device):
    """per-channel vectors [kc] -> what each staged element [B*T, kc] takes"""
    kc = c["kc"]
    idx = torch.arange(kc, device=device).view(1, kc).expand(B * T, kc)
    if defect == "pass2_stale":
        idx = torch.where(idx >= PAIR_KC, idx - PAIR_KC, idx)
    if defect == "quad_not_reloaded":
        idx = _quad_map(c, B, T, kc, device)
    return [v.double()[idx] for v in vs]


def stage(c, inp, defect=None):
    """-> (a [B*T, kc] fp64, gate): the tile the kernels keep in LDS"""
    B, T = c["B"], c["T"]
    if not c["adj"]:
        x = (materialise(c, inp, defect) if c.get("win") else inp["src"]).double()
        if not c["act"]:
            return x, torch.zeros_like(x)
        scale, shift = _vectors(c, (inp["scale"], inp["shift"]), defect, B, T, x.device)
        z = x * scale + shift
        Tm, neg = (x * scale).abs() + shift.abs(), (z <= 0).double()
        return E.elu(z), ELU_STAGE_C * U * (Tm + neg) + neg * U * z.abs()
    if c["form"] == 0:
        x = inp["dy"].double()
        return x, torch.zeros_like(x)
    k0, k1, k2 = _vectors(c, inp["coef"].unbind(0), defect, B, T, inp["dz"].device)
    if defect == "c2_dropped":
        k2 = torch.zeros_like(k2)
    t0, t1 = k0 * inp["dz"].double(), k1 * inp["y"].double()
    return t0 + t1 + k2, DY_C * U * (t0.abs() + t1.abs() + k2.abs())


def product(c, a, ga, W, bf16, defect=None, crange=None, flip=True):
    """the contraction of the staged tile a (gate ga) -> dict(want, gate, r, own) over all channels or ``crange``"""
    B, T, kc, adj = c["B"], c["T"], c["kc"], c["adj"]
    fl = torch.zeros_like(a)
    Wd = W.double()
    if defect == "pair_second_gets_first":
        a = a.view(B, T, kc).clone()
        a[1::2] = a[0::2][:a[1::2].shape[0]]
        a = a.view(B * T, kc)
    if bf16 or defect == "f32_on_bf16":
        lo, hi = rb(a - ga), rb(a + ga)
        fl, a, ga, Wd = (hi - lo).abs() * float(flip), rb(a), torch.zeros_like(a), rb(Wd)
    c0, c1 = crange if crange is not None else (0, kc)
    if defect == "drop_last_chunk":
        c1 = (kc - 1) // CC * CC
    keep = torch.zeros(kc, dtype=torch.float64, device=a.device)
    keep[c0:c1] = 1.0
    X, GX, FX = (im2col(t * keep, T, c["d"], adj, defect) for t in (a, ga, fl))
    Wm = wmat(Wd, c["cin"], c["cout"], adj, defect)
    r = G.acc_ref(X, Wm, bool(bf16), n=max(1, 3 * (c1 - c0)))
    own = (FX if bf16 else GX) @ Wm.abs().t()
    want = r["acc"]
    if defect == "odd_last_missing":
        want = want.clone()
        want[(B - 1) * T:] = 0.0
    return {"want": want, "gate": G.acc_gate(r) + own, "r": r, "own": own, "X": X}


# ------------------------------------------------------------------------------------------------ statistics
def _lane_of(fam, bf16):
    return (lambda r: (r >> 2) & 1) if (fam == "pair64" or (fam == "one" and bf16)) else (lambda r: r % 8)


def slice_positions(fam, bf16, T):
    """(positions, lanes): position p of a slice holds row positions[p] (-1: none) and sits on lane p % lanes of sum_gate"""
    lane = _lane_of(fam, bf16)
    seqs = 2 if fam == "pair32" else 1
    nl = 2 if (fam == "pair64" or (fam == "one" and bf16)) else 8
    per = [[s * T + r for s in range(seqs) for r in range(T) if lane(r) == l] for l in range(nl)]
    per = [p for p in per if p]
    depth = max(len(p) for p in per)
    pos = [per[l][i] if i < len(per[l]) else -1 for i in range(depth) for l in range(len(per))]
    return pos, len(per)


def stat_sums(x, mag, cw, cq, fam, bf16, B, T, nrep, extra=None, defect=None):
    """column sums of the summands x [B*T, ch] per replica -> (want [nrep, ch], gate [nrep, ch]); mag bounds |x|, cw / cq the
    summands' own worst-case error and n P2 (gemm_ref), extra: per-summand errors that are added up, not carried in the
    statistical form: further roundings, and the staged operands' part of a summand's gate -- a flipped bf16 rounding of one
    staged element moves up to three rows of every column by the whole of its term, one way: it is a bias, not a rounding
    noise, and min(., C_STAT u sqrt(.)) would drop it (module docstring: CHANGED, with the CPU measurement)"""
    ch = x.shape[1]
    seqs = 2 if fam == "pair32" else 1
    ns = cdiv(B, seqs)
    R = seqs * T

    def sl(v):
        p = torch.zeros((ns * R + 1, ch), dtype=torch.float64, device=x.device)        # + a zero row for position -1
        p[:B * T] = v
        return p
    pos, lanes = slice_positions(fam, bf16, T)
    pos = torch.tensor(pos, device=x.device)
    base = torch.arange(ns, device=x.device).view(ns, 1) * R
    gidx = torch.where(pos.view(1, -1) >= 0, base + pos.view(1, -1), torch.full_like(base, ns * R))
    g_sum = sum_gate(sl(x)[gidx], sl(mag)[gidx], lanes)
    xs = x
    if defect == "stats_rows_lt16":
        xs = x * (torch.arange(B * T, device=x.device) % T < 16).view(-1, 1)
    tot = lambda v: sl(v)[:ns * R].view(ns, R, ch).sum(1)
    s = torch.arange(ns, device=x.device)
    rep = (s if fam == "pair32" else (s if fam == "one" else s // 2)) % nrep
    if defect == "stats_wrong_replica":
        rep = (rep + 1) % nrep
    z = lambda: torch.zeros((nrep, ch), dtype=torch.float64, device=x.device)
    want = z().index_add_(0, rep, tot(xs))
    gate = z().index_add_(0, rep, g_sum + (tot(extra) if extra is not None else 0.0))
    cws, cqs = z().index_add_(0, rep, tot(cw)), z().index_add_(0, rep, tot(cq))
    return want, gate + torch.minimum(cws, C_STAT * U * torch.sqrt(cqs)) + 1e-300


def _with_sum(name, want, gate, out):
    out[name] = (want, gate)
    out[name + "_sum"] = (want.sum(0), gate.sum(0))


# ------------------------------------------------------------------------------------------------ whole cases
def reference(c, inp, bf16, defect=None, switch="both", flip=True, own_in_min=False):
    """-> {output name: (want, gate)}: y / out (ks > 1: slab0 .. and the reduced y / out), col, dy_out, stats [nrep, 2, ch] and
    stats_sum [2, ch].  flip=False leaves the rounding-flip term out of the bf16 gates (for an evaluation that rounds the same
    fp64 staged values as the reference does); own_in_min=True is the statistics gate in the issue's starting form (the staged
    operands' term carried inside the min, see the module docstring), kept for the CPU file's demonstration"""
    d0 = defect[:-4] if defect and defect.endswith("_adj") else defect
    B, T, kc, ks = c["B"], c["T"], c["kc"], c["ks"]
    fam = family(c, bf16, switch)
    a, ga = stage(c, inp, d0)
    name = "out" if c["adj"] else "y"
    res = {}
    if ks == 1:
        p = product(c, a, ga, inp["W"], bf16, d0, flip=flip)
    else:
        slabs = [product(c, a, ga, inp["W"], bf16, d0, crange=rg, flip=flip) for rg in split_ranges(kc, ks)]
        for z, (s, (k0, k1)) in enumerate(zip(slabs, split_ranges(kc, ks))):
            empty = k1 <= k0
            want = torch.zeros_like(s["want"]) if empty else s["want"]
            if empty and d0 == "empty_split_unwritten":
                want = torch.full_like(want, SENTINEL)
            res[f"slab{z}"] = (want, torch.zeros_like(want) if empty else s["gate"])
        terms = torch.stack([res[f"slab{z}"][0] for z in range(ks)])
        p = {"want": terms.sum(0), "gate": ks * U * terms.abs().sum(0) + sum(res[f"slab{z}"][1] for z in range(ks))}
    if not c["adj"]:
        res["y"] = (p["want"], p["gate"])
        if c["col"]:
            res["col"] = (col_layout(im2col(a, T, c["d"], False), kc), col_layout(im2col(ga, T, c["d"], False), kc))
        if c["stats"]:
            v, r = p["want"], p["r"]
            cw, own = r["worst"], p["own"]          # own: the staged operands' errors and bf16 flips, added up (see stat_sums)
            if own_in_min:
                cw, own = cw + own, torch.zeros_like(own)
            w1, g1 = stat_sums(v, v.abs(), cw, r["nq"], fam, bf16, B, T, c["nrep"], extra=own, defect=d0)
            w2, g2 = stat_sums(v * v, v * v, 2 * v.abs() * cw, 4 * v * v * r["nq"], fam, bf16, B, T, c["nrep"],
                               extra=U * v * v + 2 * v.abs() * own, defect=d0)
            _with_sum("stats", torch.stack([w1, w2], 1), torch.stack([g1, g2], 1), res)
        return res
    if c["form"] >= 2:
        res["dy_out"] = (a, ga)
    if c["form"] == 3:
        vs = [inp[k].double() for k in ("ep_scale", "ep_shift", "ep_mean", "ep_rstd")]
        if d0 == "epilogue_cols_local":
            tc = tile_cols(fam, bf16)
            vs = [v[torch.arange(v.numel(), device=v.device) % tc] for v in vs]
        scale, shift, mean, rstd = vs
        yd = inp["ep_y"].double()
        z = yd * scale + shift
        Tm, neg = (yd * scale).abs() + shift.abs(), (z <= 0).double()
        e = E.elu_grad(z)
        rel = E._rel_e(z, Tm, neg) + 2 * U
        da, r = p["want"], p["r"]
        dz = da * e
        res["out"] = (dz, (p["gate"] + da.abs() * rel) * e)
        yh, yh_mag = (yd - mean) * rstd, (yd.abs() + mean.abs()) * rstd
        cw, cq, own = r["worst"] * e + da.abs() * rel * e, r["nq"] * e * e, p["own"] * e
        if own_in_min:
            cw, own = cw + own, torch.zeros_like(own)
        w1, g1 = stat_sums(dz, dz.abs(), cw, cq, fam, bf16, B, T, c["nrep"], extra=own, defect=d0)
        m2 = dz.abs() * yh_mag
        w2, g2 = stat_sums(dz * yh, m2, cw * yh_mag, cq * yh_mag * yh_mag, fam, bf16, B, T, c["nrep"],
                           extra=4 * U * m2 + own * yh_mag, defect=d0)
        _with_sum("stats", torch.stack([w1, w2], 1), torch.stack([g1, g2], 1), res)
    else:
        res["out"] = (p["want"], p["gate"])
    return res


def touched_rows(c, inp, defect):
    """bool [B*T, 1]: output rows fed by a staged row the defect changes (for ``moved``'s mask)"""
    d0 = defect[:-4] if defect.endswith("_adj") else defect
    good, _ = stage(c, inp)
    bad, _ = stage(c, inp, d0)
    if d0 == "pair_second_gets_first":
        ch = (torch.arange(c["B"] * c["T"]) // c["T"] % 2 == 1).view(-1, 1).double()
    else:
        ch = (good != bad).any(1, keepdim=True).double()
    return im2col(ch, c["T"], c["d"], c["adj"]).sum(1, keepdim=True) > 0


def defect_mask(c, inp, defect, bf16):
    """the elements of DEFECTS[defect]'s output the defect is judged on, or None for all of them"""
    d0 = defect[:-4] if defect.endswith("_adj") else defect
    B, T, d = c["B"], c["T"], c["d"]
    t = (torch.arange(B * T) % T).view(-1, 1)
    b = (torch.arange(B * T) // T).view(-1, 1)
    if d0 in ("quad_not_reloaded", "pair_second_gets_first", "ring_wrap_off_by_one", "seg_wraps_into_next"):
        return touched_rows(c, inp, defect)
    if d0 == "tap_shift":
        return (t + d < T) if c["adj"] else (t >= d)
    if d0 == "edge_neighbour":
        return ((t + 2 * d >= T) & (b < B - 1)) if c["adj"] else ((t < 2 * d) & (b > 0))
    if d0 == "odd_last_missing":
        return b == B - 1
    if d0 == "epilogue_cols_local":
        return (torch.arange(c["nc"]) >= tile_cols(family(c, bf16), bf16)).view(1, -1)
    return None
