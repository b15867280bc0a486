"""The gates of tests/track_bwd_ref.py, on the CPU: the clean restatement of each kernel passes its gate on the case list
of tests/test_track_bwd_branches.py, every planted defect fails it; the identity the track routes' backward rests on,
in fp64 with the oracle's autograd; and the ABI of the two new entry points.  No GPU."""
import re

import numpy as np
import pytest
import torch

import track_bwd_ref as R
from helpers import T, make_encoder
from opensetgaitrecognition_pcaa_amd import _lib, constants
from oracle import pcaa_oracle as O

HOP = constants.CROP_STEP


# ------------------------------------------------------------------------------------------------ the segment backward
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("ch", R.CHANNELS)
def test_segment_bwd_gate_passes_the_clean_evaluation_and_fails_every_defect(ch, dtype):
    case = R.segment_case(ch, dtype)
    ref = R.segment_bwd_ref(**case)
    dy, stats = R.segment_bwd_fp32(**case)
    r_dy = R.ratio(dy, ref["dy"], ref["dy_gate"])
    r_st = R.ratio(stats, ref["stats"], ref["stats_gate"])
    print(f"[track-bwd gates] ch={ch} {dtype}: clean dy {r_dy:.3f}, statistics {r_st:.3f} of the gate")
    assert r_dy <= 1.0 and r_st <= 1.0
    assert not dy[case["M"] - R.TAIL:].any(), "rows no segment owns are zeros"
    for defect in R.SEGMENT_DEFECTS:
        bad = R.segment_bwd_ref(defect=defect, **case)
        which = "stats" if defect == "batch_stats" else "dy"
        r = R.ratio(bad[which], ref[which], ref[which + "_gate"])
        print(f"[track-bwd gates] ch={ch} {dtype}: {defect} moves {which} to {r:.3g} of the gate")
        assert r > 10.0, defect
        if defect not in ("batch_stats", "tail_unwritten"):         # a wrong gradient shows in the statistics too
            assert R.ratio(bad["stats"], ref["stats"], ref["stats_gate"]) > 10.0, defect


def test_a_bad_segment_owns_no_row():
    case = R.segment_case(8, torch.float32)
    M = case["M"]
    u = case["u_off"].clone()
    u[3] = M + 4                                   # segment 2 ends past the table, segment 3 runs backwards
    bad = dict(case, u_off=u)
    ref = R.segment_bwd_ref(**bad)
    clean = R.segment_bwd_ref(**case)
    lo, hi = int(case["u_off"][2]), int(case["u_off"][4])
    assert not ref["dy"][lo:hi].any() and torch.equal(ref["dy"][hi:], clean["dy"][hi:])
    dy, _ = R.segment_bwd_fp32(**bad)
    assert R.ratio(dy, ref["dy"], ref["dy_gate"]) <= 1.0


# ------------------------------------------------------------------------------------------------ the overlap-add
PLANS = [("flat W=1", [0], 30, 0, 0), ("flat W=4", [0, 6, 12, 18], 48, 0, 0), ("flat, idle rows", [3, 40], 80, 0, 0),
         ("ring that wraps", [20, 26, 0], 32, 32, 0), ("two rings", [31, 40, 70], 80, 40, 2)]


@pytest.mark.parametrize("name,starts,rows,ring,segs", PLANS)
def test_overlap_add_is_the_adjoint_of_the_gather_and_defects_show(name, starts, rows, ring, segs):
    from opensetgaitrecognition_pcaa_amd import ops
    idx = R.row_index_ref(starts, T, rows, ring, segs)
    off, cidx = R.csr_of(idx, rows)
    # the package's host plan is this restatement (WindowRows needs no device for its host half)
    plan = ops.WindowRows.__new__(ops.WindowRows)
    plan.host, plan.T, plan.table_rows, plan.ring_rows, plan.segments = np.asarray(starts, np.int64), T, rows, ring, segs
    assert np.array_equal(plan.row_index_host(), idx)
    poff, pidx = plan.csr()
    assert np.array_equal(poff, off) and np.array_equal(pidx, cidx) and poff.dtype == pidx.dtype == np.int32
    rng = np.random.default_rng(5)
    src = rng.standard_normal((len(idx), 6)).astype(np.float32)
    got = R.gather_sum_rows_ref(src, off, cidx)
    # adjoint: <gather(t), s> == <t, gather_sum(s)> in fp64, and the fp32 sum is within its few roundings of the fp64 one
    t = rng.standard_normal((rows, 6))
    assert np.isclose((t[idx] * src).sum(), (t * got.astype(np.float64)).sum(), rtol=1e-6)
    want64 = np.zeros((rows, 6))
    np.add.at(want64, idx, src.astype(np.float64))
    assert np.abs(got - want64).max() <= 8 * 2.0 ** -24 * np.abs(src).max() * 5
    assert not got[np.bincount(idx, minlength=rows) == 0].any(), "a row without contributors is zero"
    for defect in R.OVERLAP_DEFECTS:
        assert not np.array_equal(R.gather_sum_rows_ref(src, off, cidx, defect=defect), got), (name, defect)


def test_overlap_add_skips_an_index_outside_the_source():
    src = np.arange(12, dtype=np.float32).reshape(3, 4)
    off, idx = np.array([0, 2, 3], np.int32), np.array([0, 7, -1], np.int32)
    got = R.gather_sum_rows_ref(src, off, idx)
    assert np.array_equal(got[0], src[0]) and not got[1].any()


# ------------------------------------------------------------------------------------------------ the identity, fp64
def _sd(enc):
    sd = {k: (v.detach().double() if v.is_floating_point() else v.detach()).clone() for k, v in enc.state_dict().items()}
    names = [n for n, _ in enc.named_parameters()]
    for n in names:
        sd[n].requires_grad_(True)
    return sd, names


@pytest.mark.parametrize("seed,n_frames,C,head", [(1, 49, 4, True), (2, 43, 4, False), (3, 37, 5, True)])
def test_three_routes_give_one_gradient_in_fp64(seed, n_frames, C, head):
    """d(window loss) / d(every encoder parameter) through (a) the padded crops, (b) the frame table and the overlap-add of
    the window gradients, (c) the compact rows and the weighted pool: equal to 1e-12 relative, in fp64."""
    N, K = 32, 4
    _, _, track = R.make_track(n_frames, N, C, seed)
    W = len(range(0, n_frames - T, HOP))
    U = (W - 1) * HOP + T
    sd, names = _sd(make_encoder(K, N, C, head, seed=seed))
    rng = np.random.default_rng(seed)
    r1, r2 = torch.from_numpy(rng.standard_normal((W, K))), torch.from_numpy(rng.standard_normal((W, 32)))
    params = [sd[n] for n in names]

    def loss_of(logits, fv):
        return (logits * r1).sum() + (fv * r2).sum()

    # (a) the materialised crops [W, C, T, N]
    crops = torch.from_numpy(R.crops_of(track, T, HOP, W)).double().permute(0, 3, 1, 2)
    ga = torch.autograd.grad(loss_of(*O.cg_encoder_forward(crops, sd, head, training=False, update_stats=False)), params)

    # (b) every frame once -> table; windows gathered; the window gradients overlap-added by the CSR; then the PointNet
    frames = torch.from_numpy(track[:U]).double()
    table = R.oracle_point_net(sd, frames.reshape(U * N, C)).reshape(U, N, -1).mean(dim=1)
    idx = R.row_index_ref(HOP * np.arange(W), T, U)
    win = table.detach()[torch.from_numpy(idx)].requires_grad_(True)
    tc_names = [n for n in names if not n.startswith("pc_block.")]
    g2 = torch.autograd.grad(loss_of(*R.oracle_windows(sd, win.view(W, T, -1), head)), [win] + [sd[n] for n in tc_names])
    off, cidx = R.csr_of(idx, U)
    dtable = torch.zeros_like(table)
    for u in range(U):
        for k in range(off[u], off[u + 1]):
            dtable[u] = dtable[u] + g2[0][cidx[k]]
    pc_names = [n for n in names if n.startswith("pc_block.")]
    g1 = torch.autograd.grad(table, [sd[n] for n in pc_names], grad_outputs=dtable)
    gb = dict(zip(tc_names, g2[1:]))
    gb.update(zip(pc_names, g1))

    # (c) the distinct rows of every frame once, pooled with their multiplicities
    rows, weight, u_off, _ = R.compact_of(track[:U])
    assert len(rows) < U * N, "the track repeats detections"
    f = R.oracle_point_net(sd, torch.from_numpy(rows).double())
    wf = f * torch.from_numpy(weight)[:, None]
    table_c = torch.stack([wf[u_off[i]:u_off[i + 1]].sum(0) for i in range(U)]) / N
    gc = torch.autograd.grad(loss_of(*R.oracle_windows(sd, table_c[torch.from_numpy(idx)].view(W, T, -1), head)), params)

    worst = 0.0
    for n, a, c in zip(names, ga, gc):
        scale = float(a.abs().max()) + 1e-300
        worst = max(worst, float((gb[n] - a).abs().max()) / scale, float((c - a).abs().max()) / scale)
    print(f"[track-bwd identity] F={n_frames} C={C} head={head}: W={W}, rows {len(rows)} of {U * N}, largest deviation "
          f"between the three routes {worst:.2e} of a tensor's scale")
    assert worst <= 1e-12


# ------------------------------------------------------------------------------------------------ the ABI
def test_abi_27_and_the_two_entry_points():
    with open(_lib.HEADER) as f:
        declared = int(re.search(r"#define\s+PCAA_ABI_VERSION\s+(\d+)", f.read()).group(1))
    assert declared >= 27 and _lib.ABI_VERSION == declared
    protos = _lib.parse_header()
    assert len(protos["pcaa_segment_weighted_mean_bwd"][1]) == 19 and len(protos["pcaa_gather_sum_rows"][1]) == 10
    lib = _lib.load()                               # raises with build instructions when the library is not there
    assert lib.pcaa_abi_version() == declared
    for name in ("pcaa_segment_weighted_mean_bwd", "pcaa_gather_sum_rows"):
        assert hasattr(lib, name)
    # the refusals need no device: null pointers, ch % 8, a leading dimension below ch or off 8, misalignment
    a = 4096                                                            # a 16-B aligned stand-in address, never dereferenced
    ok = dict(dpool=a, y=a, dy=2 * a, dtype=0, lda=8, weight=a, u_off=a, n=1, M=8, ch=8, N=32, scale=a, shift=a, mean=a,
              rstd=a, stats=a, nrep=16, err=None, stream=None)

    def seg(**kw):
        return lib.pcaa_segment_weighted_mean_bwd(*dict(ok, **kw).values())

    for kw in (dict(dpool=None), dict(y=None), dict(dy=None), dict(stats=None), dict(mean=None), dict(ch=12), dict(ch=4),
               dict(lda=4), dict(lda=12, ch=8), dict(y=a + 8), dict(dy=2 * a + 4), dict(dpool=a + 4), dict(dy=a),
               dict(dtype=2), dict(n=0), dict(N=0), dict(nrep=0)):
        assert seg(**kw) != 0, kw
    assert lib.pcaa_gather_sum_rows(None, 1, 4, a, a, 1, a, 1, None, None) != 0
    assert lib.pcaa_gather_sum_rows(a, 1, 4, None, a, 1, 2 * a, 1, None, None) != 0
    assert lib.pcaa_gather_sum_rows(a, 1, 4, a, None, 1, 2 * a, 1, None, None) != 0
    assert lib.pcaa_gather_sum_rows(a, 1, 0, a, a, 1, 2 * a, 1, None, None) != 0
    assert lib.pcaa_gather_sum_rows(a, 1, 4, a, a, 1, a, 1, None, None) != 0          # dst aliases src
    assert lib.pcaa_gather_sum_rows(a + 2, 1, 4, a, a, 1, 2 * a, 1, None, None) != 0
