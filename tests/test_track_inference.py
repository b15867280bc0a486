"""Frame-deduplicated open-set inference: the overlap mask, the host plan, the windowed first layer of the temporal
block, ``OpenSetScorer.embed(dedup_frames=True)`` / ``embed_track`` and ``StreamingScorer``.

Crops are cut with NSTEPS = 30 and CROP_STEP = 6 out of tracks whose frames were standardised one by one, so consecutive
crops of a track share 24 frames bit for bit, and the eval-mode PointNet block is a function of one frame: every frame
needs encoding once.  The CPU tests pin the cropping rule and the plan; the GPU tests compare the new paths with the
existing entry points (bit-exact where the same instructions run on the same values), with the reference's procedure
(tests/golden/procedures.npz) and with the CPU oracle."""
import json
import pickle

import numpy as np
import pytest
import torch

from helpers import T, load_golden, make_encoder
from opensetgaitrecognition_pcaa_amd import constants, datasets, synthetic as syn

G, META = load_golden("procedures")
HOP = constants.CROP_STEP
UNIQUE_FRAMES = {"test": 504, "unseen": 7524}       # of 1 080 / 16 020 crop frames (36 / 534 crops in 12 / 180 runs)


def _raw_and_splits(tmp_path, monkeypatch):
    """The golden's raw dataset (10 subjects x 3 scenarios x 10 tracks) and its splits, regenerated here (the same recipe
    as tests/test_procedures.py)."""
    data, gen = tmp_path / "raw", tmp_path / "gen"
    for subj in range(10):
        for si, scen in enumerate(("free_walk", "hands_in_pockets", "smartphone")):
            d = data / f"target{subj}" / scen
            d.mkdir(parents=True, exist_ok=True)
            for t in range(10):
                with open(d / f"pc_tr{t}{si}.obj", "wb") as f:
                    pickle.dump(syn.synthetic_raw_track(1000 + subj * 100 + si * 10 + t, 38 + ((subj + t) % 3) * 6), f)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(constants, "DATA_PATH", str(data))
    monkeypatch.setattr(constants, "GEN_DATA_PATH", str(gen))
    monkeypatch.setattr(constants, "NFEATURES", 4)
    np.random.seed(META["np_seed_splits"])
    datasets.generate_splits(train_classes=META["train_classes"], seed=0, nmax_points=META["nmax"], verbose=False)


def _packed_sequential(split, tmp_path):
    """-> (crops [M,T,N,C] fp32 as the packed store keeps them, file names in sequential order)"""
    from opensetgaitrecognition_pcaa_amd.batcher import PackedCrops, pack_split
    ds = datasets.MSRadarDataset(split, sequential=True)
    cache = str(tmp_path / f"packed_{split.value}")
    pack_split(ds, cache)
    return np.array(PackedCrops(cache).crops), list(ds.filenames)


def _numpy_mask(crops, hop=HOP):
    """same[i]: the first T - hop frames of crop i + 1 equal the last T - hop frames of crop i as 32-bit words"""
    w = np.ascontiguousarray(crops).view(np.uint32)
    return np.array([np.array_equal(w[i, hop:], w[i + 1, :w.shape[1] - hop]) for i in range(len(w) - 1)], dtype=np.int32)


def _names_mask(names):
    """same track, crop index + 1"""
    key = [(datasets.filename2subj(f), datasets.filename2scenario(f), datasets.filename2track(f)) for f in names]
    crop = [datasets.filename2crop(f) for f in names]
    return np.array([key[i] == key[i + 1] and crop[i + 1] == crop[i] + 1 for i in range(len(names) - 1)], dtype=np.int32)


def _host_crops(track, hop=HOP):
    """the reference's cropping rule on a [F,N,C] track -> [W,T,N,C]"""
    return torch.stack([track[s:s + T] for s in np.arange(track.shape[0] - T, step=hop)])


# ---------------------------------------------------------------------------------------------------- CPU
def test_window_count_is_the_reference_rule():
    from opensetgaitrecognition_pcaa_amd import inference
    for hop in (1, 5, 6, 30):
        for F in range(0, 201):
            assert inference.window_count(F, 30, hop) == len(np.arange(F - 30, step=hop)), (F, hop)
    assert inference.window_count(30) == 0 and inference.window_count(36) == 1 and inference.window_count(37) == 2
    assert inference.window_count(273) == 41


def test_plan_frames_reproduces_every_crop(tmp_path, monkeypatch):
    from opensetgaitrecognition_pcaa_amd import inference
    _raw_and_splits(tmp_path, monkeypatch)
    for split in (constants.SPLIT.TEST, constants.SPLIT.UNSEEN):
        crops, names = _packed_sequential(split, tmp_path)
        M = len(crops)
        same = _numpy_mask(crops)
        assert np.array_equal(same, _names_mask(names)), split
        frame_src, win_row = inference.plan_frames(same, M, T, HOP)
        assert len(frame_src) == UNIQUE_FRAMES[split.value] and len(win_row) == M
        assert len(np.unique(frame_src)) == len(frame_src)
        words = crops.view(np.uint32).reshape(M * T, -1)
        table = words[frame_src]
        for i in range(M):
            assert np.array_equal(table[win_row[i]:win_row[i] + T], words[i * T:(i + 1) * T]), (split, i)
        # nothing shared: the identity plan
        frame_src, win_row = inference.plan_frames(np.zeros(M - 1, np.int32), M, T, HOP)
        assert np.array_equal(frame_src, np.arange(M * T)) and np.array_equal(win_row, np.arange(M) * T)
    fs, wr = inference.plan_frames(np.zeros(0, np.int32), 1, T, HOP)
    assert np.array_equal(fs, np.arange(T)) and np.array_equal(wr, [0])
    with pytest.raises(ValueError):
        inference.plan_frames(np.zeros(3, np.int32), 3, T, HOP)


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_crop_overlap_kernel(tmp_path, monkeypatch):
    from opensetgaitrecognition_pcaa_amd import ops
    _raw_and_splits(tmp_path, monkeypatch)
    for split in (constants.SPLIT.TEST, constants.SPLIT.UNSEEN):
        crops, _ = _packed_sequential(split, tmp_path)
        got = ops.crop_overlap(torch.from_numpy(crops).cuda(), HOP)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), _numpy_mask(crops)), split

    def chain(F, N, C, seed):
        return _host_crops(syn.synthetic_pcs(1, F, N, C, seed=seed)[0]).contiguous()

    base = chain(30 + 6 * 5 + 1, 32, 4, 3)                             # 6 chained crops, 16-byte path
    assert ops.crop_overlap_vec_bytes(base.cuda()) == 16
    assert ops.crop_overlap(base.cuda(), HOP).cpu().tolist() == [1] * 5
    # one low mantissa bit in the last shared frame of crop 2 (its frame T - hop - 1): pair (1, 2) breaks, and so does
    # pair (2, 3), whose overlap holds the same frame
    x = base.clone()
    x.view(torch.int32)[2, T - HOP - 1, -1, -1] ^= 1
    assert ops.crop_overlap(x.cuda(), HOP).cpu().tolist() == [1, 0, 0, 1, 1]
    # the last word of the overlap only: frame T - 1 of crop 1 against frame T - hop - 1 of crop 2
    x = base.clone()
    x.view(torch.int32)[1, T - 1, -1, -1] ^= 1
    assert ops.crop_overlap(x.cuda(), HOP).cpu().tolist() == [1, 0, 1, 1, 1]
    # the first word
    x = base.clone()
    x.view(torch.int32)[4, 0, 0, 0] ^= 1
    assert ops.crop_overlap(x.cuda(), HOP).cpu().tolist() == [1, 1, 1, 0, 1]
    # -0.0 against +0.0 are different words; a frame outside the overlap does not matter
    x = base.clone()
    x[0, HOP + 2, 5, 1] = 0.0
    x[1, 2, 5, 1] = -0.0
    x[0, 0, 0, 0] = 123.0
    assert ops.crop_overlap(x.cuda(), HOP).cpu().tolist() == [0, 1, 1, 1, 1]
    # identical NaN bits are equal words
    x = base.clone()
    nan_bits = 0x7FC01234
    x.view(torch.int32)[0, HOP + 2, 5, 1] = nan_bits
    x.view(torch.int32)[1, 2, 5, 1] = nan_bits
    assert ops.crop_overlap(x.cuda(), HOP).cpu().tolist() == [1, 1, 1, 1, 1]
    x.view(torch.int32)[1, 2, 5, 1] = nan_bits + 1
    assert ops.crop_overlap(x.cuda(), HOP).cpu().tolist() == [0, 1, 1, 1, 1]
    # a frame of 150 x 5 floats = 3 000 bytes: the 4-byte path
    odd = chain(30 + 6 * 3 + 2, 150, 5, 4)
    assert ops.crop_overlap_vec_bytes(odd.cuda()) == 4
    assert ops.crop_overlap(odd.cuda(), HOP).cpu().tolist() == [1, 1, 1]
    x = odd.clone()
    x.view(torch.int32)[1, T - 1, -1, -1] ^= 1
    assert ops.crop_overlap(x.cuda(), HOP).cpu().tolist() == [1, 0, 1]
    # other hops, unrelated crops
    assert ops.crop_overlap(base.cuda(), 5).cpu().tolist() == [0] * 5
    assert ops.crop_overlap(syn.synthetic_pcs(4, T, 32, 4, seed=9).cuda(), HOP).cpu().tolist() == [0, 0, 0]
    # one crop: nothing to compare, nothing launched
    assert ops.crop_overlap(base[:1].cuda(), HOP).numel() == 0
    # the 4-byte gather that goes with such frames
    src = torch.arange(7 * 750, dtype=torch.float32).view(7, 750).cuda()
    idx = torch.tensor([6, 0, 3, 3], dtype=torch.int64).cuda()
    assert torch.equal(ops.gather_frames(src, idx), src[idx])
    assert torch.equal(ops.gather_frames(src[:, :748].contiguous(), idx), src[idx][:, :748])


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [False, True])
def test_windowed_temporal_layer_is_bit_exact(bf16):
    """The windowed entry point against the existing one on the MATERIALISED windows: the same instructions on the same
    values, so ``torch.equal``."""
    from opensetgaitrecognition_pcaa_amd import ops
    gen = torch.Generator().manual_seed(11)
    for W, cin, cout, dil, act in ((40, 1024, 16, 1, False), (200, 1024, 16, 1, False), (40, 16, 32, 2, True),
                                   (133, 16, 32, 2, True)):
        Wt = (torch.randn(cout, cin * 3, generator=gen) / np.sqrt(3 * cin)).cuda()
        scale = (torch.rand(cin, generator=gen) + 0.5).cuda() if act else None
        shift = (torch.randn(cin, generator=gen) * 0.3).cuda() if act else None
        cases = []
        rows = HOP * (W - 1) + T
        table = torch.randn(rows, cin, generator=gen).cuda()
        starts = HOP * np.arange(W)
        cases.append(("track", table, starts, 0))
        cases.append(("shuffled", table, np.random.default_rng(W).permutation(starts), 0))
        ring = 47                                                       # windows wrap: 6 j mod 47 passes 47 - 30 often
        cases.append(("ring", torch.randn(ring, cin, generator=gen).cuda(), (HOP * np.arange(W)) % ring, ring))
        for name, tab, st, ring_rows in cases:
            plan = ops.WindowRows(st, T, tab.shape[0], ring_rows, device="cuda")
            assert not ring_rows or (st + T > ring_rows).any(), "the ring case must wrap"
            idx = torch.from_numpy((st[:, None] + np.arange(T)[None, :]) % (ring_rows or tab.shape[0])).cuda().reshape(-1)
            mat = tab[idx].contiguous()
            assert torch.equal(plan.row_index(), idx)
            want, _ = ops.dtc_conv_fwd(mat, scale, shift, Wt, W, T, dil, bf16=bf16)
            got, _ = ops.dtc_conv_fwd(tab, scale, shift, Wt, W, T, dil, bf16=bf16, win_row=plan)
            assert got.shape == want.shape == (W * T, cout)
            assert torch.equal(got, want), (name, W, cin, cout, bf16, (got - want).abs().max().item())
    # the range check runs on the host copy of the plan
    with pytest.raises(ValueError):
        ops.WindowRows([0, 7], T, 36, device="cuda")
    with pytest.raises(ValueError):
        ops.WindowRows([-1], T, 36, device="cuda")
    with pytest.raises(ValueError):
        ops.WindowRows([47], T, 47, 47, device="cuda")


@pytest.mark.gpu
def test_dtc_forward_windowed_equals_materialised_and_refuses_training():
    """functional.dtc_forward with win_row: fused path == the same block on the written-out windows (bit for bit: only
    layer 0 differs, and only in its addressing); the unfused fallback (one gather, then today's path) likewise; training
    raises."""
    from opensetgaitrecognition_pcaa_amd import functional as F_hip, ops
    enc = make_encoder(4, 32, 4, True, seed=0).cuda().eval()
    layers = enc.tc_block.layers()
    W = 21
    table = torch.randn(HOP * (W - 1) + T, 1024, generator=torch.Generator().manual_seed(5)).cuda()
    plan = ops.WindowRows(HOP * np.arange(W), T, table.shape[0], device="cuda")
    mat = table[plan.row_index()].contiguous()
    with torch.no_grad():
        want, _ = F_hip.dtc_forward(mat, W, T, layers, False, True)
        got, _ = F_hip.dtc_forward(table, W, T, layers, False, True, win_row=plan)
        assert torch.equal(got, want)
        F_hip._FUSE_DTC = False
        try:
            slow_w, _ = F_hip.dtc_forward(mat, W, T, layers, False, True)
            slow, _ = F_hip.dtc_forward(table, W, T, layers, False, True, win_row=plan)
        finally:
            F_hip._FUSE_DTC = True
        assert torch.equal(slow, slow_w)
    with pytest.raises(ValueError):
        F_hip.dtc_forward(table, W, T, layers, True, True, win_row=plan)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_naive_sequential_procedure_dedup_vs_reference(tmp_path, monkeypatch):
    """The deduplicated path under the gates test_naive_sequential_procedure_vs_reference applies to the crop path:
    labels equal, share of differing votes <= 0.02 (a cap on votes that sit on the threshold), metrics within 0.03."""
    from sklearn.metrics import f1_score
    from opensetgaitrecognition_pcaa_amd import functional as F_hip, inference
    _raw_and_splits(tmp_path, monkeypatch)
    F_hip.set_precision("fp32")
    K = len(META["train_classes"])
    enc = make_encoder(K, META["nmax"], 4, True, seed=META["enc_fill_seed"]).to("cuda").eval()
    means = torch.from_numpy(G["infer.means"]).to("cuda")
    known_pcs, known_labels = inference._sequential_split_on_device(constants.SPLIT.TEST, constants.TRAIN_SCENARIOS, "cuda")
    unseen_pcs, unseen_labels = inference._sequential_split_on_device(constants.SPLIT.UNSEEN, constants.TRAIN_SCENARIOS, "cuda")
    encoded = []
    plain_embed = inference.OpenSetScorer.embed

    def recording_embed(self, pcs, dedup_frames=False, **kw):
        self.last_frames_encoded = None
        out = plain_embed(self, pcs, dedup_frames=dedup_frames, **kw)
        encoded.append((bool(dedup_frames), pcs.shape[0], self.last_frames_encoded))
        return out
    monkeypatch.setattr(inference.OpenSetScorer, "embed", recording_embed)
    for k in (1, 2, 4, 6):
        ref = G[f"infer.k{k}.preds"]
        share = {}
        for dedup in (False, True):
            del encoded[:]
            preds, labels, thr = inference.naive_sequential_procedure(k, enc, means, known_pcs, known_labels, unseen_pcs,
                                                                      unseen_labels, seed=0, unseen_valid_ratio=0.2,
                                                                      dedup_frames=dedup)
            share[dedup] = float((preds != ref).mean()) if preds.shape == ref.shape else float("nan")
            if dedup:
                # the deduplicated path really ran: unique frames encoded, before any padding
                assert encoded == [(True, known_pcs.shape[0], UNIQUE_FRAMES["test"]),
                                   (True, unseen_pcs.shape[0], UNIQUE_FRAMES["unseen"])], encoded
            else:
                assert encoded == [(False, known_pcs.shape[0], None), (False, unseen_pcs.shape[0], None)], encoded
        print(f"k={k}: share of votes that differ from the reference's: crop path {share[False]:.4f}, "
              f"deduplicated path {share[True]:.4f}")
        assert np.array_equal(labels.astype(np.int64), G[f"infer.k{k}.labels"]), k
        assert preds.shape == ref.shape and (preds != ref).mean() <= 0.02, (k, (preds != ref).mean())
        m = G[f"infer.k{k}.metrics"]
        got = [np.equal(labels, preds).mean(), f1_score(labels, preds, average="micro"),
               f1_score(labels, preds, average="macro"), f1_score(labels, preds, average="weighted")]
        assert np.allclose(got, m, atol=0.03), (k, got, m)


def _same_encoder_gates(got, want, what):
    """tests/test_inference.py:55-57: same encoder, different batch composition"""
    assert torch.equal(got[0], want[0]), what
    assert torch.allclose(got[1], want[1], rtol=1e-5, atol=1e-6), (what, (got[1] - want[1]).abs().max().item())
    assert torch.allclose(got[2], want[2], rtol=1e-3), (what, ((got[2] - want[2]).abs() / want[2].abs()).max().item())


F_TRACK = 30 + 6 * 40 + 3


def _track_setup():
    K, N, C = 4, 32, 4
    enc = make_encoder(K, N, C, True, seed=0).cuda().eval()
    means = torch.from_numpy(load_golden("misc")[0]["means_K4"]).float()
    track = syn.synthetic_pcs(1, F_TRACK, N, C, seed=21)[0].contiguous()
    return K, enc, means, track


@pytest.mark.gpu
def test_track_and_crop_paths_agree_fp32():
    from opensetgaitrecognition_pcaa_amd import inference
    K, enc, means, track = _track_setup()
    crops = _host_crops(track).cuda().permute(0, 3, 1, 2)              # [W,C,T,N] view of point-major storage
    W = crops.shape[0]
    assert W == inference.window_count(F_TRACK) == 41
    for bs in (1024, 16):
        scorer = inference.OpenSetScorer(enc, means, batch_size=bs)
        plain = scorer.embed(crops)
        assert scorer.last_frames_encoded is None
        dedup = scorer.embed(crops, dedup_frames=True)
        assert scorer.last_frames_encoded == 30 + 6 * 40
        trk = scorer.embed_track(track.cuda())
        assert scorer.last_frames_encoded == 30 + 6 * 40
        for name, got in (("dedup", dedup), ("track", trk)):
            assert got[0].shape == (W,) and got[1].shape == (W, 32) and got[2].shape == (W,) and got[2].dtype == torch.float64
            _same_encoder_gates(got, plain, (name, bs))
    # unrelated crops: nothing merged, same result
    scorer = inference.OpenSetScorer(enc, means)
    loose = syn.synthetic_pcs(7, T, 32, 4, seed=2).cuda().permute(0, 3, 1, 2)
    _same_encoder_gates(scorer.embed(loose, dedup_frames=True), scorer.embed(loose), "loose")
    assert scorer.last_frames_encoded == 7 * T
    # no window: empty tensors, no launch; the aligned last window is the reference's to drop
    for F in (0, 7, 30):
        p, f, l = scorer.embed_track(track[:F].cuda())
        assert p.shape == (0,) and f.shape == (0, 32) and l.shape == (0,) and l.dtype == torch.float64
    assert scorer.embed_track(track[:36].cuda())[0].shape == (1,)
    assert scorer.embed_track(track[:36].cuda(), drop_last_aligned=False)[0].shape == (2,)
    assert scorer.embed_track(track[:30].cuda(), drop_last_aligned=False)[0].shape == (1,)


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_track_path_bf16_vs_oracle():
    """bf16 mode at N = 128, C = 4, K = 8 on a track of 256 windows: ``embed_track`` (and the streaming form, whose odd
    pushes need the padding to whole GEMM row tiles) against the CPU oracle's eval forward on every 8th window, under the
    gates of test_config4_bf16_eval_encoder_vs_oracle_on_64_of_1024."""
    from opensetgaitrecognition_pcaa_amd import functional as F_hip, inference
    from oracle import pcaa_oracle as O
    N, C, K, W = 128, 4, 8, 256
    enc = make_encoder(K, N, C, True, seed=0).cuda().eval()
    means = O.sample_distant_points(32, K, 10, 10).float()
    track = syn.synthetic_pcs(1, 30 + 6 * (W - 1) + 1, N, C, seed=5)[0].contiguous()
    assert inference.window_count(track.shape[0]) == W
    F_hip.set_precision("bf16")
    scorer = inference.OpenSetScorer(enc, means, batch_size=64)        # several chunks of frames and of windows
    preds, fv, lik = scorer.embed_track(track.cuda())
    assert [s.y is None for s in scorer.last_pointnet_saves] == [True] * 4, "the fused-epilogue path must be the one that ran"
    assert scorer.last_frames_encoded == 30 + 6 * (W - 1)
    idx = torch.arange(0, W, 8)
    sd = {k: v.detach().cpu().clone() for k, v in enc.state_dict().items()}
    with torch.no_grad():
        ref_oc, ref_fv = O.cg_encoder_forward(torch.stack([track[6 * j:6 * j + T] for j in idx.tolist()])
                                              .permute(0, 3, 1, 2).contiguous(), sd, True, training=False)
    scale = ref_fv.abs().max().item()
    err = (fv.cpu()[idx] - ref_fv).abs().max().item()
    agree = (preds.cpu()[idx] == O.predicted_labels(ref_oc)).float().mean().item()
    print(f"bf16 embed_track vs ORACLE on {len(idx)} of {W} windows: label agreement {agree:.4f}, "
          f"embedding err {err / scale:.2e} of scale")
    assert err <= 5e-2 * scale
    assert agree >= 0.95
    # an odd hop leaves an odd number of frames: a chunk is filled up to whole GEMM row tiles with the track's next frame,
    # the one before it, or zeros.  Windows 0 / 6 under hop 5 hold the frames of windows 0 / 5 under hop 6 (another batch
    # composition of the same bf16 path: the bf16 gate on the embeddings)
    one = inference.OpenSetScorer(enc, means, batch_size=1)
    for sc, trk in ((scorer, track[:30 + 5 * 9 + 2]), (scorer, track[:30 + 5 * 9]), (one, track[:30 + 5 * 9])):
        p5, f5, _ = sc.embed_track(trk.cuda(), hop=5, drop_last_aligned=False)
        assert sc.last_frames_encoded == 30 + 5 * 9 and p5.shape == (10,)
        assert [s.y is None for s in sc.last_pointnet_saves] == [True] * 4
        assert (f5[[0, 6]] - fv[[0, 5]]).abs().max().item() <= 5e-2 * scale
    # the deduplicated crop path on the same windows
    crops = _host_crops(track).cuda().permute(0, 3, 1, 2)
    p2, f2, _ = scorer.embed(crops, dedup_frames=True)
    assert scorer.last_frames_encoded == 30 + 6 * (W - 1)
    assert [s.y is None for s in scorer.last_pointnet_saves] == [True] * 4
    err2 = (f2.cpu()[idx] - ref_fv).abs().max().item()
    agree2 = (p2.cpu()[idx] == O.predicted_labels(ref_oc)).float().mean().item()
    print(f"bf16 embed(dedup_frames=True): label agreement {agree2:.4f}, embedding err {err2 / scale:.2e} of scale")
    assert err2 <= 5e-2 * scale and agree2 >= 0.95
    # streaming, pushes of odd sizes
    stream = inference.StreamingScorer(enc, means, float(lik.median()), 4, K)
    outs, pos = [], 0
    for n in (7, 13, 1, 64) * 1000:
        if pos >= track.shape[0]:
            break
        outs.append(stream.push(track[pos:pos + n].cuda()))
        assert [s.y is None for s in stream.last_pointnet_saves] == [True] * 4
        pos += n
    p3, f3 = torch.cat([o[0] for o in outs])[:W], torch.cat([o[1] for o in outs])[:W]
    err3 = (f3.cpu()[idx] - ref_fv).abs().max().item()
    agree3 = (p3.cpu()[idx] == O.predicted_labels(ref_oc)).float().mean().item()
    print(f"bf16 StreamingScorer: label agreement {agree3:.4f}, embedding err {err3 / scale:.2e} of scale")
    assert err3 <= 5e-2 * scale and agree3 >= 0.95


@pytest.mark.gpu
def test_streaming_scorer():
    from opensetgaitrecognition_pcaa_amd import inference
    K, enc, means, track = _track_setup()
    dev_track = track.cuda()
    scorer = inference.OpenSetScorer(enc, means)
    want = scorer.embed_track(dev_track)
    W = want[0].shape[0]
    thr, k = float(want[2].median()), 4
    stream = inference.StreamingScorer(enc, means, thr, k, K, max_push=64)
    assert stream.ring_rows == T + 64 and F_TRACK > 2 * stream.ring_rows          # the ring wraps several times

    def run(trk):
        outs, pos, emitted = [], 0, 0
        for n in (1, 6, 7, 13, 30, 64) * 100:
            if pos >= trk.shape[0]:
                break
            out = stream.push(trk[pos:pos + n])
            pos = min(pos + n, trk.shape[0])
            emitted += out[0].shape[0]
            # window j comes back from the very push that delivers frame T + j * hop - 1
            assert emitted == (0 if pos < T else (pos - T) // HOP + 1), (pos, emitted)
            assert out[1].shape == (out[0].shape[0], 32) and out[2].shape == out[0].shape
            outs.append(out)
        return tuple(torch.cat([o[i] for o in outs]) for i in range(3))

    got = run(dev_track)
    assert got[0].shape[0] == W == inference.window_count(F_TRACK)                # (F - T) % hop = 3: nothing extra
    _same_encoder_gates(got, want, "stream")
    votes = stream.votes()
    assert torch.equal(votes, inference.k_vote(got[2][:W // k * k].contiguous(), got[0][:W // k * k].contiguous(), thr, k, K,
                                               n_classes=K))
    assert votes.shape == (W // k,)
    # a second track after reset(); (F - T) % hop == 0: the stream emits the aligned last window, the reference's rule drops it
    stream.reset()
    assert stream.votes().numel() == 0
    second = syn.synthetic_pcs(1, 30 + 6 * 5, 32, 4, seed=22)[0].contiguous().cuda()
    want2 = scorer.embed_track(second)
    got2 = run(second)
    assert want2[0].shape[0] == inference.window_count(60) == 5 and got2[0].shape[0] == 6
    _same_encoder_gates(tuple(t[:5] for t in got2), want2, "second track")
    _same_encoder_gates(got2, scorer.embed_track(second, drop_last_aligned=False), "second track, aligned window kept")
    assert torch.equal(stream.votes(), inference.k_vote(got2[2][:4].contiguous(), got2[0][:4].contiguous(), thr, k, K,
                                                        n_classes=K))
    # one push longer than max_push is cut into several
    stream.reset()
    _same_encoder_gates(stream.push(dev_track), want, "one long push")
    # a training-mode encoder is refused
    enc.train()
    try:
        with pytest.raises(RuntimeError):
            stream.push(dev_track[:6])
        with pytest.raises(RuntimeError):
            inference.StreamingScorer(enc, means, thr, k, K)
    finally:
        enc.eval()
    with pytest.raises(ValueError):
        inference.StreamingScorer(enc, means, thr, k, K, max_push=64, ring_rows=64)
