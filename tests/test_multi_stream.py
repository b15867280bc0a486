"""MultiStreamScorer: many live tracks scored in one batched tick.

CPU: the tick plan (``inference.plan_tick``) against a brute-force simulation, the new exports.  GPU: the segmented
windowed temporal layer, ``scatter_rows``, ``stream_score`` and the frozen eval constants against the existing entry
points (bit for bit), the scorer end to end against ``OpenSetScorer.embed_track`` (fp32) and the CPU oracle (bf16 at the
timed shape), and its refusals.  The gates are the ones tests/test_track_inference.py applies to ``StreamingScorer``."""
import numpy as np
import pytest
import torch

from helpers import T, load_golden, make_encoder
from opensetgaitrecognition_pcaa_amd import _lib, constants, synthetic as syn

HOP = constants.CROP_STEP


# ---------------------------------------------------------------------------------------------------------------- CPU
def _simulate_tick(frames_of, windows_of, sids, counts, ring_rows, k, hop=HOP):
    """one tick, one frame and one window at a time, on plain Python ints"""
    dst, win = [], []
    for s, c in zip(sids, counts):
        for _ in range(c):
            dst.append(s * ring_rows + frames_of[s] % ring_rows)
            frames_of[s] += 1
        n = frames_of[s]
        done = 0 if n < T else (n - T) // hop + 1
        while windows_of[s] < done:
            j = windows_of[s]
            win.append((s, j, s * ring_rows + (j * hop) % ring_rows))
            windows_of[s] += 1
    votes = [(s, j // k) for s, j, _ in win if j % k == k - 1]
    return dst, win, votes


def test_plan_tick_against_brute_force():
    from opensetgaitrecognition_pcaa_amd.inference import plan_tick
    n_slots, ring_rows, k, pad_to, max_count = 5, 41, 4, 4, 8
    rng = np.random.default_rng(7)
    n_frames, n_windows = np.zeros(n_slots, np.int64), np.zeros(n_slots, np.int64)
    frames_of, windows_of = [0] * n_slots, [0] * n_slots
    opened = [0, 1, 2]                                  # slot 3 opens late, slot 1 is closed and handed out again
    seen_zero = seen_pad = seen_multi = 0
    total_votes = 0
    for tick in range(90):
        if tick == 20:
            opened.append(3)
        if tick == 45:                                  # close slot 1 ... and reopen it for a new track: counters restart
            n_frames[1] = n_windows[1] = 0
            frames_of[1] = windows_of[1] = 0
        if tick == 50:
            opened.append(4)
        sids = [int(s) for s in rng.permutation(opened)[:rng.integers(1, len(opened) + 1)]]
        counts = [int(c) for c in rng.integers(0, max_count + 1, len(sids))]
        if tick % 9 == 0:
            counts[0] = 0
        plan = plan_tick(n_frames, n_windows, sids, counts, T, HOP, k, ring_rows, pad_to)
        dst, win, votes = _simulate_tick(frames_of, windows_of, sids, counts, ring_rows, k)
        total = sum(counts)
        # frames: ring row of every frame, the padding marked "skip", no destination twice
        assert plan.dst_row.dtype == np.int32 and plan.dst_row.size == total + (-total) % pad_to
        assert plan.dst_row[:total].tolist() == dst
        assert (plan.dst_row[total:] == -1).all()
        assert len(set(dst)) == len(dst)
        # windows: stream, index within the stream, start row, ordered by stream position then ascending
        assert plan.win_stream.tolist() == [w[0] for w in win]
        assert plan.win_j.tolist() == [w[1] for w in win]
        assert plan.win_row.tolist() == [w[2] for w in win]
        # group completions and where their votes go
        assert list(zip(plan.vote_stream.tolist(), plan.vote_group.tolist())) == votes
        want_pos, g = [], 0
        for _, j, _ in win:
            want_pos.append(g if j % k == k - 1 else -1)
            g += j % k == k - 1
        assert plan.vote_pos.tolist() == want_pos
        # runs: one per stream that completes a window
        runs = plan.run_start.tolist()
        assert runs[0] == 0 and runs[-1] == len(win) and all(a < b for a, b in zip(runs, runs[1:]))
        for a, b in zip(runs, runs[1:]):
            assert len(set(plan.win_stream[a:b].tolist())) == 1
            assert b == len(win) or plan.win_stream[b] != plan.win_stream[a]
        # counters after the tick, and the one packed buffer
        assert plan.n_frames.tolist() == [frames_of[s] for s in sids]
        assert plan.n_windows.tolist() == [windows_of[s] for s in sids]
        assert plan.packed.dtype == np.int32
        for name, (a, b) in plan.offsets.items():
            assert np.array_equal(plan.packed[a:b], getattr(plan, name)), name
        assert sum(b - a for a, b in plan.offsets.values()) == plan.packed.size
        n_frames[sids], n_windows[sids] = plan.n_frames, plan.n_windows
        seen_zero += 0 in counts
        seen_pad += bool(total % pad_to)
        seen_multi += any(b - a > 1 for a, b in zip(runs, runs[1:]))
        total_votes += len(votes)
    assert seen_zero and seen_pad and seen_multi and total_votes > 10
    assert max(frames_of) > 3 * ring_rows, "every ring must wrap several times"
    # argument errors
    nf, nw = np.zeros(3, np.int64), np.zeros(3, np.int64)
    for sids, counts in (([0, 0], [1, 1]), ([3], [1]), ([-1], [1]), ([0], [1, 2]), ([0], [-1]), ([0], [ring_rows - T + 1])):
        with pytest.raises(ValueError):
            plan_tick(nf, nw, sids, counts, T, HOP, k, ring_rows, 1)
    with pytest.raises(ValueError):
        plan_tick(nf, nw, [0], [1], T, HOP, k, T - 1, 1)
    with pytest.raises(ValueError):
        plan_tick(nf, nw, [0], [1], T, T + 1, k, ring_rows, 1)
    empty = plan_tick(nf, nw, [], [], T, HOP, k, ring_rows, 4)
    assert empty.dst_row.size == 0 and empty.win_row.size == 0 and empty.run_start.tolist() == [0]


def test_library_exports_the_multi_stream_entry_points():
    protos = _lib.parse_header()
    lib = _lib.load()
    for name in ("pcaa_dtc_conv_fwd_seg", "pcaa_dtc_conv_fwd_seg_bf16", "pcaa_scatter_rows", "pcaa_stream_score"):
        assert name in protos and hasattr(lib, name), name
    assert lib.pcaa_abi_version() >= 19
    # argument checks run on the host: ring_rows >= T, n_seg >= 1, non-null win_row
    assert lib.pcaa_dtc_conv_fwd_seg(1, None, None, 1, 1, 1, 30, 1024, 16, 1, 1, 0, None, 1, 64, None) != 0
    assert lib.pcaa_scatter_rows(None, None, 1, 1, None, 1, None, None) != 0


def test_window_rows_segments_are_range_checked_on_the_host():
    from opensetgaitrecognition_pcaa_amd import ops
    dev = torch.zeros(1, dtype=torch.int32)
    for host, table_rows, ring_rows, segments, why in (([0], 100, 47, 2, "segments="), ([94], 94, 47, 2, "window starts"),
                                                       ([-1], 94, 47, 2, "window starts"), ([0], 94, 20, 2, "segments="),
                                                       ([0], 94, 47, -1, "segments=")):
        with pytest.raises(ValueError, match=why):
            ops.WindowRows(host, T, table_rows, ring_rows, dev=dev, segments=segments)
    with pytest.raises(ValueError, match="dev must be"):         # in range: only the host copy of ``dev`` is objected to
        ops.WindowRows([93], T, 94, 47, dev=dev, segments=2)


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [False, True])
def test_segmented_temporal_layer_is_bit_exact(bf16):
    """pcaa_dtc_conv_fwd_seg against pcaa_dtc_conv_fwd on the MATERIALISED windows: the same instructions on the same
    values, so ``torch.equal``; with one segment it is the ``_win`` call."""
    from opensetgaitrecognition_pcaa_amd import ops
    gen = torch.Generator().manual_seed(13)
    ring, n_seg = 47, 4
    local = np.array([0, 5, 17, 18, 30, 46, 46, 23, 40, 16, 46, 1, 33])
    seg = np.array([0, 0, 1, 1, 2, 2, 0, 3, 3, 3, 3, 1, 2])
    starts = seg * ring + local
    assert len(set(seg.tolist())) >= 3 and (local + T > ring).any() and ((local == ring - 1) & (seg < n_seg - 1)).any()
    assert (seg == n_seg - 1).any() and ((seg == n_seg - 1) & (local + T > ring)).any()
    W = len(starts)
    idx_np = (seg * ring)[:, None] + (local[:, None] + np.arange(T)[None, :]) % ring
    idx = torch.from_numpy(idx_np).cuda().reshape(-1)
    for cin, cout, dil, act in ((1024, 16, 1, False), (16, 32, 2, True)):
        Wt = (torch.randn(cout, cin * 3, generator=gen) / np.sqrt(3 * cin)).cuda()
        scale = (torch.rand(cin, generator=gen) + 0.5).cuda() if act else None
        shift = (torch.randn(cin, generator=gen) * 0.3).cuda() if act else None
        table = torch.randn(n_seg * ring, cin, generator=gen).cuda()
        plan = ops.WindowRows(starts, T, table.shape[0], ring, device="cuda", segments=n_seg)
        assert torch.equal(plan.row_index(), idx)
        mat = table[idx].contiguous()
        want, _ = ops.dtc_conv_fwd(mat, scale, shift, Wt, W, T, dil, bf16=bf16)
        got, _ = ops.dtc_conv_fwd(table, scale, shift, Wt, W, T, dil, bf16=bf16, win_row=plan)
        assert got.shape == want.shape == (W * T, cout)
        assert torch.equal(got, want), (cin, cout, bf16, (got - want).abs().max().item())
        part = plan.slice(3, 9)
        got_part, _ = ops.dtc_conv_fwd(table, scale, shift, Wt, 6, T, dil, bf16=bf16, win_row=part)
        assert torch.equal(got_part, want[3 * T:9 * T])
        # one segment: the ring form of the previous entry point, bit for bit
        one = table[:ring].contiguous()
        st1 = (HOP * np.arange(40)) % ring
        a, _ = ops.dtc_conv_fwd(one, scale, shift, Wt, 40, T, dil, bf16=bf16,
                                win_row=ops.WindowRows(st1, T, ring, ring, device="cuda", segments=1))
        b, _ = ops.dtc_conv_fwd(one, scale, shift, Wt, 40, T, dil, bf16=bf16,
                                win_row=ops.WindowRows(st1, T, ring, ring, device="cuda"))
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_dtc_forward_and_encoder_windows_take_segments():
    """functional.dtc_forward / encoder_forward_windows pass a segmented plan through; the one-gather fallback honours it"""
    from opensetgaitrecognition_pcaa_amd import functional as F_hip, ops
    enc = make_encoder(4, 32, 4, True, seed=0).cuda().eval()
    layers = enc.tc_block.layers()
    ring, n_seg = 38, 3
    starts = np.array([0, 37, 38 + 20, 38 + 9, 76 + 37, 76 + 8, 76 + 30])
    W = len(starts)
    table = torch.randn(ring * n_seg, 1024, generator=torch.Generator().manual_seed(6)).cuda()
    plan = ops.WindowRows(starts, T, table.shape[0], ring, device="cuda", segments=n_seg)
    mat = table[plan.row_index()].contiguous()
    with torch.no_grad():
        want, _ = F_hip.dtc_forward(mat, W, T, layers, False, True)
        got, _ = F_hip.dtc_forward(table, W, T, layers, False, True, win_row=plan, ring_rows=ring)
        assert torch.equal(got, want)
        F_hip._FUSE_DTC = False
        try:
            slow_w, _ = F_hip.dtc_forward(mat, W, T, layers, False, True)
            slow, _ = F_hip.dtc_forward(table, W, T, layers, False, True, win_row=plan, ring_rows=ring)
        finally:
            F_hip._FUSE_DTC = True
        assert torch.equal(slow, slow_w)
        lg, fv, _ = F_hip.encoder_forward_windows(enc, table, plan, T)
        x4 = want
        st = F_hip.EncoderState()
        lg_w, fv_w, _ = F_hip._encoder_heads(enc, st, x4)
        assert torch.equal(lg, lg_w) and torch.equal(fv, fv_w)


@pytest.mark.gpu
def test_scatter_rows():
    from opensetgaitrecognition_pcaa_amd import ops
    gen = torch.Generator().manual_seed(3)
    for width, dtype in ((1024, torch.float32), (6, torch.float32), (7, torch.float32), (16, torch.bfloat16)):
        n_dst, n = 300, 70
        src = torch.randn(n, width, generator=gen).to(dtype).cuda()
        before = torch.randn(n_dst, width, generator=gen).to(dtype).cuda()
        rows = torch.randperm(n_dst, generator=gen)[:n].to(torch.int32)
        rows[[3, 17, 69]] = -1                               # padding: skipped
        keep = rows >= 0
        want = before.clone()
        want.index_copy_(0, rows[keep].long().cuda(), src[keep.cuda()])
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        got = before.clone()
        out = ops.scatter_rows(src, rows.cuda(), got, err_flag=err)
        assert out is got and torch.equal(got, want), (width, dtype)
        assert err.item() == 0
        untouched = torch.ones(n_dst, dtype=torch.bool)
        untouched[rows[keep].long()] = False
        assert torch.equal(got[untouched.cuda()], before[untouched.cuda()])
        # fewer destinations than source rows: only the first ones are taken
        got2 = before.clone()
        ops.scatter_rows(src, rows[:10].cuda(), got2)
        want2 = before.clone()
        k10 = rows[:10] >= 0
        want2.index_copy_(0, rows[:10][k10].long().cuda(), src[:10][k10.cuda()])
        assert torch.equal(got2, want2)
        # a destination out of range: flagged, nothing of it written (the rest is)
        bad = rows.clone()
        bad[5] = n_dst
        bad[6] = n_dst + 1000
        keep_b = (bad >= 0) & (bad < n_dst)
        want3 = before.clone()
        want3.index_copy_(0, bad[keep_b].long().cuda(), src[keep_b.cuda()])
        got3 = before.clone()
        ops.scatter_rows(src, bad.cuda(), got3, err_flag=err)
        assert err.item() == 1 and torch.equal(got3, want3)
    # a misaligned view takes the 4-byte copies
    base = torch.zeros(40 * 8 + 1, device="cuda")
    dst = base[1:].view(40, 8)
    src = torch.randn(5, 8, generator=gen).cuda()
    ops.scatter_rows(src, torch.tensor([4, -1, 0, 39, 7], dtype=torch.int32).cuda(), dst)
    want = torch.zeros(40, 8, device="cuda")
    want[[4, 0, 39, 7]] = src[[0, 2, 3, 4]]
    assert torch.equal(dst, want)
    with pytest.raises(ValueError):
        ops.scatter_rows(src, torch.zeros(6, dtype=torch.int32).cuda(), dst)
    with pytest.raises(ValueError):
        ops.scatter_rows(src, torch.zeros(2, dtype=torch.int32).cuda(), torch.zeros(4, 9).cuda())
    with pytest.raises(RuntimeError):
        ops.scatter_rows(src.cpu(), torch.zeros(2, dtype=torch.int32).cuda(), dst)


@pytest.mark.gpu
def test_stream_score_against_the_single_stream_kernels():
    """preds / lik equal ops.cross_entropy(want_preds) / joint_likelihood bit for bit, votes equal k_vote over each stream's
    own windows; history over several launches, ticks of k + 1 and 2k + 1 windows of one stream, exact ties in the logits."""
    from opensetgaitrecognition_pcaa_amd import inference, ops
    K, D, k, n_slots = 4, 32, 3, 4
    gen = torch.Generator().manual_seed(17)
    means = torch.from_numpy(load_golden("misc")[0]["means_K4"]).float().cuda()
    per_tick = {0: [1, k + 1, 0, 2 * k + 1, 1, 2, 3 * k, 1],
                2: [2, 2, 2, 2, 2, 2, 2, 2],
                3: [0, 1, 5, 0, k, 1, 0, k - 1]}
    n_win = {s: sum(c) for s, c in per_tick.items()}
    logits, fvs = {}, {}
    for s, n in n_win.items():
        x = torch.nn.functional.elu(torch.randn(n, K, generator=gen) * 12)       # ELU saturates to exactly -1: ties
        x[1] = -1.0
        x[2, 1] = x[2, 3] = x[2].max() + 0.5                                    # two equal maxima: the first wins
        assert ((x == -1).sum(1) >= 2).any()
        logits[s] = x.cuda()
        fvs[s] = (means[torch.randint(0, K, (n,), generator=gen).cuda()] + torch.randn(n, D, generator=gen).cuda() * 0.9)
    lik_ref = {s: inference.joint_likelihood(fvs[s].contiguous(), means) for s in n_win}
    pred_ref = {s: ops.cross_entropy(logits[s], None, want_loss=False, want_preds=True)[2] for s in n_win}
    thr = float(torch.cat(list(lik_ref.values())).median())
    vote_ref = {s: inference.k_vote(lik_ref[s][:n_win[s] // k * k].contiguous(), pred_ref[s][:n_win[s] // k * k].contiguous(),
                                    thr, k, K, n_classes=K) for s in n_win}
    assert any(0 < v.eq(K).sum() < v.numel() for v in vote_ref.values()), "known and unknown votes must both occur"
    hist_lik = torch.full((n_slots, k), float("nan"), dtype=torch.float64, device="cuda")
    hist_pred = torch.full((n_slots, k), -7, dtype=torch.int64, device="cuda")
    nf, nw = np.zeros(n_slots, np.int64), np.zeros(n_slots, np.int64)
    got = {s: ([], [], {}) for s in n_win}
    for tick in range(8):
        order = [3, 0, 2] if tick % 2 else [2, 3, 0]
        counts = [per_tick[s][tick] for s in order]
        plan = inference.plan_tick(nf, nw, order, counts, 1, 1, k, 16, 1)         # T = hop = 1: one window per frame
        lg = torch.cat([logits[s][nw[s]:nw[s] + c] for s, c in zip(order, counts)])
        fv = torch.cat([fvs[s][nw[s]:nw[s] + c] for s, c in zip(order, counts)]).contiguous()
        nf[order], nw[order] = plan.n_frames, plan.n_windows
        assert plan.win_stream.size == lg.shape[0]
        preds, lik, votes = ops.stream_score(
            lg.contiguous(), fv, means, *(torch.from_numpy(a).cuda() for a in (plan.run_start, plan.win_stream, plan.win_j,
                                                                              plan.vote_pos)),
            plan.vote_group.size, thr, k, K, K, hist_lik, hist_pred)
        assert preds.dtype == torch.int64 and lik.dtype == torch.float64 and votes.shape == (plan.vote_group.size,)
        for s in n_win:
            m = torch.from_numpy(plan.win_stream == s).cuda()
            got[s][0].append(preds[m])
            got[s][1].append(lik[m])
        for v, s, g in zip(votes.tolist(), plan.vote_stream.tolist(), plan.vote_group.tolist()):
            assert g not in got[s][2]
            got[s][2][g] = v
    for s in n_win:
        assert torch.equal(torch.cat(got[s][0]), pred_ref[s]), s
        assert torch.equal(torch.cat(got[s][1]), lik_ref[s]), s
        assert sorted(got[s][2]) == list(range(n_win[s] // k)), s
        assert [got[s][2][g] for g in range(n_win[s] // k)] == vote_ref[s].tolist(), s
    assert torch.isnan(hist_lik[1]).all() and (hist_pred[1] == -7).all(), "a stream that was not in any tick keeps its state"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_frozen_constants_give_the_same_bits(mode):
    from opensetgaitrecognition_pcaa_amd import functional as F_hip, ops
    F_hip.set_precision(mode)
    enc = make_encoder(4, 32, 4, True, seed=0).cuda().eval()
    frames = syn.synthetic_pcs(1, 64, 32, 4, seed=9)[0].contiguous().cuda()
    with torch.no_grad():
        consts = F_hip.encoder_eval_constants(enc)
        assert consts.mode == mode and len(consts.bn) == 10 and len(consts.w16) == (3 if mode == "bf16" else 0)
        assert consts.valid_for(enc, mode) and not consts.valid_for(enc, "fp16x3")
        want, saves_w = F_hip.encoder_frame_features(enc, frames)
        got, saves = F_hip.encoder_frame_features(enc, frames, consts=consts)
        assert torch.equal(got, want)
        assert [s.y is None for s in saves] == [s.y is None for s in saves_w]
        if mode == "bf16":
            assert [s.y is None for s in saves] == [True] * 4, "the fused-epilogue path must be the one that ran"
        for a, b in zip(saves, saves_w):
            assert torch.equal(a.scale, b.scale) and torch.equal(a.shift, b.shift)
        plan = ops.WindowRows(HOP * np.arange(6), T, 64, device="cuda")
        lw, fw, _ = F_hip.encoder_forward_windows(enc, want, plan, T)
        lg, fg, _ = F_hip.encoder_forward_windows(enc, want, plan, T, consts=consts)
        assert torch.equal(lg, lw) and torch.equal(fg, fw)
        # made for another precision mode, or asked for in training mode: refused
        other = F_hip.encoder_eval_constants(enc, "fp16x3" if mode == "fp32" else "fp32")
        with pytest.raises(ValueError):
            F_hip.encoder_frame_features(enc, frames, consts=other)
        enc.train()
        try:
            with pytest.raises(RuntimeError):
                F_hip.encoder_eval_constants(enc)
        finally:
            enc.eval()
        # a changed parameter or buffer is noticed
        enc.pc_block.pointnet2.module[1].running_var.mul_(1.5)
        assert not consts.valid_for(enc, mode)


def _track_setup():
    """tests/test_track_inference.py::_track_setup"""
    K, N, C = 4, 32, 4
    enc = make_encoder(K, N, C, True, seed=0).cuda().eval()
    means = torch.from_numpy(load_golden("misc")[0]["means_K4"]).float()
    return K, enc, means


def _same_encoder_gates(got, want, what):
    """tests/test_inference.py:55-57: same encoder, different batch composition"""
    assert torch.equal(got[0], want[0]), what
    assert torch.allclose(got[1], want[1], rtol=1e-5, atol=1e-6), (what, (got[1] - want[1]).abs().max().item())
    assert torch.allclose(got[2], want[2], rtol=1e-3), (what, ((got[2] - want[2]).abs() / want[2].abs()).max().item())


class _Collector:
    """per track: what the ticks returned for it, in order"""

    def __init__(self):
        self.preds, self.fv, self.lik, self.votes, self.next_window, self.next_group = [], [], [], [], 0, 0

    def take(self, tick, sid):
        m = tick.stream == sid
        if m.any():
            assert tick.window[m].tolist() == list(range(self.next_window, self.next_window + int(m.sum())))
            self.next_window += int(m.sum())
            md = torch.from_numpy(m).cuda()
            self.preds.append(tick.preds[md])
            self.fv.append(tick.sup_fv[md])
            self.lik.append(tick.lik[md])
        v = tick.vote_stream == sid
        if v.any():
            assert tick.vote_group[v].tolist() == list(range(self.next_group, self.next_group + int(v.sum())))
            self.next_group += int(v.sum())
            self.votes.append(tick.votes[torch.from_numpy(v).cuda()])

    def result(self):
        return torch.cat(self.preds), torch.cat(self.fv), torch.cat(self.lik)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_multi_stream_scorer_end_to_end_fp32():
    """4 tracks through 3 slots (one opened late, one slot reused after close), ragged ticks of at most 8 frames per
    stream so that every ring wraps many times: per track the concatenated ticks equal ``embed_track`` under the gate for
    "same encoder, different batch composition"; votes equal k_vote over the scorer's own per-stream results."""
    from opensetgaitrecognition_pcaa_amd import inference
    K, enc, means = _track_setup()
    lengths = (273, 150, 281, 266)
    tracks = [syn.synthetic_pcs(1, F, 32, 4, seed=21 + i)[0].contiguous().cuda() for i, F in enumerate(lengths)]
    ref = inference.OpenSetScorer(enc, means)
    want = [ref.embed_track(t, drop_last_aligned=False) for t in tracks]
    thr, k = float(want[0][2].median()), 4
    ms = inference.MultiStreamScorer(enc, means, thr, k, K, max_streams=3, max_push=8)
    assert ms.ring_rows == T + 8 and min(lengths) > 3 * ms.ring_rows
    assert ms.ring.shape == (3 * ms.ring_rows, 1024)
    rng = np.random.default_rng(5)
    slot_of, pos, col = {}, [0] * 4, [_Collector() for _ in range(4)]
    slot_of[0], slot_of[1] = ms.open(), ms.open()
    assert (slot_of[0], slot_of[1]) == (0, 1)
    waiting = [2, 3]                                   # track 2 opens late; track 3 takes the slot track 1 leaves
    n_ticks = n_empty = 0
    while slot_of or waiting:
        if n_ticks == 12:
            slot_of[2] = ms.open()
            waiting.remove(2)
            assert slot_of[2] == 2
            with pytest.raises(ValueError):
                ms.open()
        live = [int(t) for t in rng.permutation(list(slot_of))]
        if n_ticks % 7 == 3 and len(live) > 1:
            live = live[:-1]                           # a stream that gets nothing this tick by absence ...
        counts = [int(min(rng.integers(0, 9), lengths[t] - pos[t])) for t in live]     # ... or by a zero count
        frames = torch.cat([tracks[t][pos[t]:pos[t] + c] for t, c in zip(live, counts)])
        tick = ms.push([slot_of[t] for t in live], counts, frames)
        n_ticks += 1
        n_empty += len(tick) == 0
        assert tick.preds.shape == (len(tick),) and tick.sup_fv.shape == (len(tick), 32) and tick.lik.shape == (len(tick),)
        assert tick.preds.dtype == torch.int64 and tick.lik.dtype == torch.float64 and tick.votes.dtype == torch.int64
        assert tick.votes.shape == (tick.vote_group.size,) and tick.stream.dtype == np.int64
        expect = []
        for t, c in zip(live, counts):
            before = 0 if pos[t] < T else (pos[t] - T) // HOP + 1
            pos[t] += c
            expect += [slot_of[t]] * ((0 if pos[t] < T else (pos[t] - T) // HOP + 1) - before)
            col[t].take(tick, slot_of[t])
        assert tick.stream.tolist() == expect          # eager windows, ordered by the position of the stream in sids
        for t in live:
            if pos[t] == lengths[t]:
                ms.close(slot_of.pop(t))
                if t == 1:
                    slot_of[3] = ms.open()
                    waiting.remove(3)
                    assert slot_of[3] == 1, "the lowest free slot is handed out again"
    assert n_empty > 0 and n_ticks > 60
    for t in range(4):
        got = col[t].result()
        W = (lengths[t] - T) // HOP + 1
        assert got[0].shape == (W,) == want[t][0].shape
        _same_encoder_gates(got, want[t], f"track {t}")
        votes = torch.cat(col[t].votes)
        n = W // k * k
        assert torch.equal(votes, inference.k_vote(got[2][:n].contiguous(), got[0][:n].contiguous(), thr, k, K, n_classes=K))
    assert ms.scatter_err.item() == 0


@pytest.mark.gpu
def test_multi_stream_chunks_long_ticks_and_follows_the_encoder():
    """more windows than ``batch_size`` in one tick are scored in chunks; after ``load_state_dict`` of a differently seeded
    encoder (and after a precision switch) the next push equals a fresh scorer's"""
    from opensetgaitrecognition_pcaa_amd import functional as F_hip, inference
    K, enc, means = _track_setup()
    tracks = [syn.synthetic_pcs(1, 30 + 6 * 9, 32, 4, seed=31 + i)[0].contiguous().cuda() for i in range(3)]
    ref = inference.OpenSetScorer(enc, means)
    want = [ref.embed_track(t, drop_last_aligned=False) for t in tracks]
    ms = inference.MultiStreamScorer(enc, means, 1e-20, 2, K, max_streams=4, max_push=64, batch_size=4)
    sids = [ms.open() for _ in range(3)]
    tick = ms.push(sids, [64, 64, 64], torch.cat([t[:64] for t in tracks]))      # 6 windows per stream, chunks of 4
    assert len(tick) == 18 and tick.votes.shape == (9,)
    for i in range(3):
        m = torch.from_numpy(tick.stream == sids[i]).cuda()
        _same_encoder_gates((tick.preds[m], tick.sup_fv[m], tick.lik[m]), tuple(w[:6] for w in want[i]), f"chunked {i}")
    # another encoder's weights arrive in place: the folded constants must not be reused
    other = make_encoder(K, 32, 4, True, seed=3).cuda().eval()
    enc.load_state_dict(other.state_dict())
    for sid in sids:
        ms.close(sid)
    sid = ms.open()
    fresh = inference.MultiStreamScorer(enc, means, 1e-20, 2, K, max_streams=4, max_push=64, batch_size=4)
    fsid = fresh.open()
    a = ms.push([sid], [40], tracks[0][:40])
    b = fresh.push([fsid], [40], tracks[0][:40])
    assert len(a) == len(b) == 2
    after = inference.OpenSetScorer(enc, means).embed_track(tracks[0][:40], drop_last_aligned=False)
    _same_encoder_gates((a.preds, a.sup_fv, a.lik), after, "after load_state_dict")
    assert not torch.allclose(a.sup_fv, want[0][1][:2], rtol=1e-3, atol=1e-4), "the two encoders must differ"
    for x, y in ((a.preds, b.preds), (a.sup_fv, b.sup_fv), (a.lik, b.lik), (a.votes, b.votes)):
        assert torch.equal(x, y)
    # a precision switch between ticks is picked up the same way
    F_hip.set_precision("bf16")
    a = ms.push([sid], [12], tracks[0][40:52])
    b = fresh.push([fsid], [12], tracks[0][40:52])
    assert len(a) == 2 and torch.equal(a.sup_fv, b.sup_fv) and torch.equal(a.lik, b.lik) and torch.equal(a.preds, b.preds)
    assert ms._consts.mode == "bf16" and len(ms._consts.w16) == 3


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_multi_stream_bf16_vs_oracle():
    """bf16 mode at the timed shape (N = 128, C = 4, K = 8): 3 streams cut from the seed-5 track of
    test_track_path_bf16_vs_oracle, odd counts per tick (the tick is padded to whole GEMM row tiles), every 8th window
    against the CPU oracle's eval forward under that test's gates."""
    from opensetgaitrecognition_pcaa_amd import functional as F_hip, inference
    from oracle import pcaa_oracle as O
    N, C, K = 128, 4, 8
    enc = make_encoder(K, N, C, True, seed=0).cuda().eval()
    means = O.sample_distant_points(32, K, 10, 10).float()
    track = syn.synthetic_pcs(1, 30 + 6 * 255 + 1, N, C, seed=5)[0].contiguous()
    F_len = 520
    cuts = [track[i * F_len:(i + 1) * F_len] for i in range(3)]
    W = (F_len - T) // HOP + 1
    F_hip.set_precision("bf16")
    ms = inference.MultiStreamScorer(enc, means, 1e-30, 4, K, max_streams=3, max_push=64)
    sids = [ms.open() for _ in range(3)]
    dev = [c.cuda() for c in cuts]
    col, pos = [_Collector() for _ in range(3)], [0, 0, 0]
    cycle, step, padded = (7, 13, 1, 5, 3, 9, 11), 0, 0
    while min(pos) < F_len:
        counts = [min(cycle[(step + 2 * i) % len(cycle)], F_len - pos[i]) for i in range(3)]
        padded += sum(counts) % 2
        tick = ms.push(sids, counts, torch.cat([dev[i][pos[i]:pos[i] + c] for i, c in enumerate(counts)]))
        assert [s.y is None for s in ms.last_pointnet_saves] == [True] * 4, "the fused-epilogue path must be the one that ran"
        for i in range(3):
            pos[i] += counts[i]
            col[i].take(tick, sids[i])
        step += 1
    assert padded > 10, "odd ticks must occur: the padding to the row-tile quantum is what this exercises"
    idx = torch.arange(0, W, 8)
    sd = {k: v.detach().cpu().clone() for k, v in enc.state_dict().items()}
    got_p, got_f, ref_p, ref_f = [], [], [], []
    for i in range(3):
        p, f, _ = col[i].result()
        assert p.shape == (W,)
        with torch.no_grad():
            oc, fv = O.cg_encoder_forward(torch.stack([cuts[i][6 * j:6 * j + T] for j in idx.tolist()])
                                          .permute(0, 3, 1, 2).contiguous(), sd, True, training=False)
        got_p.append(p.cpu()[idx]), got_f.append(f.cpu()[idx]), ref_p.append(O.predicted_labels(oc)), ref_f.append(fv)
    got_p, got_f, ref_p, ref_f = torch.cat(got_p), torch.cat(got_f), torch.cat(ref_p), torch.cat(ref_f)
    scale = ref_f.abs().max().item()
    err = (got_f - ref_f).abs().max().item()
    agree = (got_p == ref_p).float().mean().item()
    print(f"bf16 MultiStreamScorer vs ORACLE on {len(got_p)} of {3 * W} windows: label agreement {agree:.4f}, "
          f"embedding err {err / scale:.2e} of scale")
    assert err <= 5e-2 * scale
    assert agree >= 0.95
    assert ms.scatter_err.item() == 0


@pytest.mark.gpu
def test_multi_stream_scorer_refusals():
    from opensetgaitrecognition_pcaa_amd import inference
    K, enc, means = _track_setup()
    frames = syn.synthetic_pcs(1, 12, 32, 4, seed=1)[0].contiguous().cuda()
    with pytest.raises(ValueError):
        inference.MultiStreamScorer(enc, means, 0.0, 4, K, max_push=64, ring_rows=64)       # < NSTEPS + max_push
    ms = inference.MultiStreamScorer(enc, means, 0.0, 4, K, max_streams=2, max_push=8)
    a, b = ms.open(), ms.open()
    with pytest.raises(ValueError):
        ms.open()                                                                           # beyond max_streams
    for sids, counts, fr in (([a, a], [6, 6], frames),                   # duplicate
                             ([5], [6], frames[:6]),                     # unknown
                             ([a], [9], frames[:9]),                     # more than max_push
                             ([a, b], [6, 5], frames),                   # sum(counts) != frames
                             ([a], [6, 6], frames),                      # one count per sid
                             ([a], [6], frames[:6].double()),            # dtype
                             ([a], [6], frames[:12:2]),                  # layout
                             ([a], [6], frames[:6].reshape(6, -1)),      # rank
                             ([a], [-1], frames[:0]),
                             ([0.5], [6], frames[:6])):
        with pytest.raises(ValueError):
            ms.push(sids, counts, fr)
    with pytest.raises(RuntimeError):
        ms.push([a], [6], frames[:6].cpu())
    ms.close(b)
    with pytest.raises(ValueError):
        ms.push([b], [6], frames[:6])                                                       # closed
    with pytest.raises(ValueError):
        ms.close(b)
    assert ms.n_frames.tolist() == [0, 0], "a refused push changes nothing"
    # no window yet: empty tensors of the right dtypes, and a tick without frames
    for tick in (ms.push([a], [6], frames[:6]), ms.push([a], [0], frames[:0]), ms.push([], [], frames[:0])):
        assert len(tick) == 0 and tick.preds.shape == (0,) and tick.preds.dtype == torch.int64
        assert tick.sup_fv.shape == (0, 32) and tick.lik.shape == (0,) and tick.lik.dtype == torch.float64
        assert tick.votes.shape == (0,) and tick.votes.dtype == torch.int64
    assert ms.n_frames.tolist() == [6, 0]
    enc.train()
    try:
        with pytest.raises(RuntimeError):
            ms.push([a], [6], frames[:6])
        with pytest.raises(RuntimeError):
            inference.MultiStreamScorer(enc, means, 0.0, 4, K)
    finally:
        enc.eval()
