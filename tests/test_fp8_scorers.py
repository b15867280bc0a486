"""The fp8 eval-PointNet kind (``functional.set_eval_pointnet("fp8")``) through the entry points, on the GPU: frame features
against the fp64 emulation of the numerics contract (tests/fp8_ref.py ``emulate``), a frame's independence of its neighbours,
the entry points that share a frame table, ``sup_fv`` of ``embed_track``, and the switch itself (back to "bf16": the bits
from before; autograd, training, fp32 mode and N = 150: the kind is ignored).

The end-to-end gate: with d(a, b) the largest absolute difference over the features' maximum,
d(device, emulation) <= 0.1 d(emulation, fp64 oracle), all three computed here.  The right-hand side is the reference's own
quantisation error (4.0e-2 on the CPU); a wrong rounding mode, a missing fold or a missing clamp shifts the result by a
quantity of that size, summation order and rare rounding flips sit orders of magnitude below (test_fp8_gates_cpu.py)."""
import numpy as np
import pytest
import torch

import fp8_ref as R
from helpers import T, load_golden, make_encoder
from opensetgaitrecognition_pcaa_amd import constants, synthetic as syn

pytestmark = pytest.mark.gpu
HOP = constants.CROP_STEP
K, C = 8, 4


def _F():
    from opensetgaitrecognition_pcaa_amd import functional as F_hip
    F_hip.set_precision("bf16")
    return F_hip


def _enc(N):
    return make_encoder(K, N, C, False).cuda().eval()


def _sd(enc):
    return {k: v.detach() for k, v in enc.state_dict().items()}


def _d(a, b, top):
    return float((a.double() - b.double()).abs().max()) / top


def _means():
    return torch.from_numpy(load_golden("misc")[0]["means_K4"]).float().repeat(2, 1) * torch.tensor([[1.0], [-1.0]]).repeat_interleave(4, 0)


@pytest.mark.parametrize("N,U", [(32, 64), (128, 8)])
def test_frame_features_against_the_emulation(N, U):
    F_hip = _F()
    enc = _enc(N)
    frames = syn.synthetic_pcs(1, U, N, C, seed=11)[0].contiguous().cuda()
    with torch.no_grad(), F_hip.eval_pointnet("fp8"):
        got, saves = F_hip.encoder_frame_features(enc, frames)
    assert [s.a_in.dtype for s in saves] == [torch.float32] + [torch.float8_e4m3fn] * 3
    emu = R.emulate(_sd(enc), frames.view(U * N, C), N)
    oracle = R.emulate(_sd(enc), frames.view(U * N, C), N, quant=False)
    top = float(oracle.abs().max())
    d_dev, d_q = _d(got, emu, top), _d(emu, oracle, top)
    print(f"[fp8 scorers] N={N}: d(device, emulation) = {d_dev:.2e}, d(emulation, oracle) = {d_q:.2e}")
    assert d_dev <= 0.1 * d_q


def test_ragged_frame_features_against_the_emulation():
    F_hip = _F()
    from opensetgaitrecognition_pcaa_amd import ops
    N, n = 32, 24
    enc = _enc(N)
    rng = np.random.default_rng(5)
    base = syn.synthetic_pcs(1, n, N, C, seed=12)[0].numpy()
    frames = np.stack([base[f][rng.integers(0, int(rng.integers(3, N + 1)), size=N)] for f in range(n)])     # padded by repetition
    frames = torch.from_numpy(frames).contiguous().cuda()
    u_off = ops.frames_unique_offsets(frames)
    rows, weight, seg = ops.frames_unique(frames, u_off)
    with torch.no_grad(), F_hip.eval_pointnet("fp8"):
        got, saves = F_hip.encoder_frame_features_ragged(enc, rows, weight, seg, n, N)
    assert [s.a_in.dtype for s in saves] == [torch.float32] + [torch.float8_e4m3fn] * 3 and saves[-1].y is None
    seg_h = seg.cpu().tolist()
    frame_of = torch.zeros(rows.shape[0], dtype=torch.long, device="cuda")
    for f in range(n):
        frame_of[seg_h[f]:seg_h[f + 1]] = f

    def pooled(a):
        return torch.zeros((n, a.shape[1]), dtype=torch.float64, device="cuda").index_add_(0, frame_of, a * weight.double()[:, None]) / N
    emu = pooled(R.emulate(_sd(enc), rows, 0))
    oracle = pooled(R.emulate(_sd(enc), rows, 0, quant=False))
    top = float(oracle.abs().max())
    d_dev, d_q = _d(got, emu, top), _d(emu, oracle, top)
    print(f"[fp8 scorers] ragged N={N}: d(device, emulation) = {d_dev:.2e}, d(emulation, oracle) = {d_q:.2e}")
    assert d_dev <= 0.1 * d_q
    # and the padded frames give the same features up to the pooling order
    with torch.no_grad(), F_hip.eval_pointnet("fp8"):
        padded, _ = F_hip.encoder_frame_features(enc, frames)
    assert _d(padded, got, top) <= 0.1 * d_q


def test_a_frame_does_not_depend_on_its_neighbours():
    F_hip = _F()
    N = 32
    enc = _enc(N)
    frames = syn.synthetic_pcs(1, 40, N, C, seed=13)[0].contiguous().cuda()
    q = F_hip.frame_pad_quantum(N)
    with torch.no_grad(), F_hip.eval_pointnet("fp8"):
        among, _ = F_hip.encoder_frame_features(enc, frames)
        for f in (0, 17, 39):
            alone = torch.zeros((q, N, C), device="cuda")
            alone[0] = frames[f]
            got, saves = F_hip.encoder_frame_features(enc, alone)
            assert saves[1].a_in.dtype == torch.float8_e4m3fn
            assert torch.equal(got[0], among[f]), f


def _triples(inference, enc, means, track, thr=0.0):
    crops = torch.stack([track[s:s + T] for s in np.arange(track.shape[0] - T, step=HOP)]).permute(0, 3, 1, 2)
    sc = inference.OpenSetScorer(enc, means)
    out = {"dedup": sc.embed(crops, dedup_frames=True), "track": sc.embed_track(track)}
    st = inference.StreamingScorer(enc, means, thr, 4, K, max_push=64)
    parts = [st.push(track[a:a + 16]) for a in range(0, track.shape[0], 16)]
    W = out["track"][0].shape[0]
    out["stream"] = tuple(torch.cat([p[i] for p in parts])[:W] for i in range(3))
    out["saves"] = sc.last_pointnet_saves
    return out


def test_entry_points_that_share_a_frame_table_stay_consistent_and_the_switch_restores_the_bits():
    F_hip = _F()
    from opensetgaitrecognition_pcaa_amd import inference
    N = 32
    enc = _enc(N)
    means = _means().cuda()
    track = syn.synthetic_pcs(1, 66, N, C, seed=14)[0].contiguous().cuda()
    before = _triples(inference, enc, means, track)
    assert before["saves"][1].a_in.dtype == torch.bfloat16
    with F_hip.eval_pointnet("fp8"):
        assert F_hip.get_eval_pointnet() == "fp8"
        f8 = _triples(inference, enc, means, track)
    assert F_hip.get_eval_pointnet() == "bf16"
    assert f8["saves"][1].a_in.dtype == torch.float8_e4m3fn
    after = _triples(inference, enc, means, track)
    ran = []
    for a, b in (("dedup", "track"), ("track", "stream")):
        for i in range(3):
            if torch.equal(before[a][i], before[b][i]):          # wherever the bf16 route is bit-equal, the fp8 route is
                assert torch.equal(f8[a][i], f8[b][i]), (a, b, i)
                ran.append((a, b, ("preds", "sup_fv", "lik")[i]))
    print(f"[fp8 scorers] bit-equality held in bf16 and asserted in fp8 for {len(ran)} of 6 comparisons: {ran}")
    # the two frame-table routes of OpenSetScorer agree bit for bit in bf16 today: their whole triple is always checked
    assert all(("dedup", "track", n) in ran for n in ("preds", "sup_fv", "lik")), ran
    for name in ("dedup", "track", "stream"):
        for i in range(3):
            assert torch.equal(before[name][i], after[name][i]), (name, i)
    assert not torch.equal(before["track"][1], f8["track"][1])
    with pytest.raises(ValueError):
        F_hip.set_eval_pointnet("fp4")


def test_sup_fv_of_embed_track():
    F_hip = _F()
    from opensetgaitrecognition_pcaa_amd import inference
    from oracle import pcaa_oracle as O
    N = 32
    enc = _enc(N)
    means = _means().cuda()
    track = syn.synthetic_pcs(1, 66, N, C, seed=15)[0].contiguous().cuda()
    sc = inference.OpenSetScorer(enc, means)
    fv16 = sc.embed_track(track)[1]
    with F_hip.eval_pointnet("fp8"):
        fv8 = sc.embed_track(track)[1]
    sd = {k: v.detach().double().cpu() for k, v in enc.state_dict().items()}
    W = fv8.shape[0]

    def tail(feats):
        x2 = torch.stack([feats[HOP * j:HOP * j + T] for j in range(W)]).permute(0, 2, 1).cpu()      # [W, 1024, T]
        x4 = O.temporal_block(x2, sd, "tc_block.", False).mean(dim=2)
        return O.elu(O.linear(x4, sd["MLP_sup1.0.weight"], sd["MLP_sup1.0.bias"]))
    rows = track.view(-1, C)
    want8 = tail(R.emulate(_sd(enc), rows, N))
    want = tail(R.emulate(_sd(enc), rows, N, quant=False))
    top = float(want.abs().max())
    d_q, d_16, d_8 = _d(want8, want, top), _d(fv16.cpu(), want, top), _d(fv8.cpu(), want8, top)
    print(f"[fp8 scorers] sup_fv: d(fp8 device, emulation + fp64 tail) = {d_8:.2e}; d(emulation, oracle) = {d_q:.2e}; "
          f"d(bf16 device, oracle) = {d_16:.2e}")
    assert d_8 <= 0.1 * d_q + d_16


def test_multi_stream_scorer_after_a_toggle_equals_a_fresh_one():
    F_hip = _F()
    from opensetgaitrecognition_pcaa_amd import inference
    N = 32
    enc = _enc(N)
    means = _means().cuda()
    track = syn.synthetic_pcs(1, 48, N, C, seed=16)[0].contiguous().cuda()

    def run(ms, sid):
        return [ms.push([sid], [16], track[a:a + 16]) for a in (0, 16, 32)][-1]
    ms = inference.MultiStreamScorer(enc, means, 0.0, 4, K, max_streams=2)
    sid = ms.open()
    first = run(ms, sid)
    assert ms.last_pointnet_saves[1].a_in.dtype == torch.bfloat16
    consts16 = ms._consts
    with F_hip.eval_pointnet("fp8"):
        ms.push([sid], [6], track[:6])
        assert ms.last_pointnet_saves[1].a_in.dtype == torch.float8_e4m3fn
        assert ms._consts is not consts16 and ms._consts.kind == "fp8" and len(ms._consts.w8) == 3
        assert not consts16.valid_for(enc, "bf16")
    fresh = inference.MultiStreamScorer(enc, means, 0.0, 4, K, max_streams=2)
    sid2 = fresh.open()
    want = run(fresh, sid2)
    ms.close(sid)
    sid = ms.open()
    got = run(ms, sid)
    assert ms.last_pointnet_saves[1].a_in.dtype == torch.bfloat16 and ms._consts.kind == "bf16" and not ms._consts.w8
    for name in ("preds", "sup_fv", "lik"):
        assert torch.equal(getattr(got, name), getattr(want, name)) and torch.equal(getattr(got, name), getattr(first, name)), name


def test_the_kind_is_ignored_where_the_fused_route_does_not_run():
    F_hip = _F()
    N = 32
    enc = _enc(N)
    frames = syn.synthetic_pcs(1, 16, N, C, seed=17)[0].contiguous().cuda()
    with F_hip.eval_pointnet("fp8"):
        # under autograd with a parameter that requires a gradient: the bf16 route, and its backward works
        p = enc.pc_block.pointnet2.module[0].weight
        assert p.requires_grad and torch.is_grad_enabled()
        feats = F_hip.frame_features(enc, frames)
        feats.square().sum().backward()
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
        p.grad = None
        # fp32 mode
        with torch.no_grad():
            _, saves = F_hip.encoder_frame_features(enc, frames, mode="fp32")
            assert all(s.a_in.dtype == torch.float32 for s in saves)
            # training mode
            x = frames.view(1, 16, N, C).permute(0, 3, 1, 2)
            _, _, st = F_hip.encoder_forward(enc, x, True, mode="bf16")
            assert [s.a_in.dtype for s in st.pn[1:]] == [torch.bfloat16] * 3
            enc.eval()
            # N = 150: no pooled epilogue of that size, the whole block falls back
            enc150 = _enc(150)
            f150 = syn.synthetic_pcs(1, 4, 150, C, seed=18)[0].contiguous().cuda()
            _, saves = F_hip.encoder_frame_features(enc150, f150)
            assert [s.a_in.dtype for s in saves[1:]] == [torch.bfloat16] * 3
            # and with the kind honoured again
            _, saves = F_hip.encoder_frame_features(enc, frames)
            assert [s.a_in.dtype for s in saves[1:]] == [torch.float8_e4m3fn] * 3
