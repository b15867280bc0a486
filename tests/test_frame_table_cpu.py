"""The host-side rules of frame_table.py, each tested where it is written: the window rule, the plan of several tracks'
windows, the padding of a chunk of frames to whole GEMM row tiles, the refusals.  No device."""
import itertools

import numpy as np
import pytest
import torch

from opensetgaitrecognition_pcaa_amd import frame_table as ft
from opensetgaitrecognition_pcaa_amd import functional as F_hip, inference

T = 30


def test_window_rule():
    n = np.arange(101, dtype=np.int64)
    for hop in range(1, 31):
        eager = ft.eager_window_count(n, T, hop)                          # the whole array in one call
        assert isinstance(eager, np.ndarray) and eager.dtype == np.int64
        for F in range(101):
            want_eager = 0 if F < T else (F - T) // hop + 1
            want_ref = len(np.arange(F - T, step=hop))
            assert ft.eager_window_count(F, T, hop) == want_eager == eager[F], (F, hop)
            W, U = ft.track_windows(F, T, hop)
            assert W == want_ref and U == ((W - 1) * hop + T if W else 0), (F, hop)
            assert ft.track_windows(F, T, hop, drop_last_aligned=False) == (want_eager, (want_eager - 1) * hop + T if want_eager else 0)
            # the reference's rule drops exactly the aligned last window
            assert want_eager - want_ref == (1 if F >= T and (F - T) % hop == 0 else 0), (F, hop)
            # the names the callers know the rule under
            assert inference.window_count(F, T, hop) == want_ref
            assert F_hip.track_windows(F, T, hop) == (W, U)
    with pytest.raises(ValueError):
        ft.track_windows(40, T, 0)


def test_track_plan():
    hop, frames = 6, [41, 61, 36]
    plan = ft.plan_track_windows(frames, T, hop)
    assert plan.counts == [2, 6, 1] and plan.used == [36, 60, 30] and plan.U == 126
    base, first, want = 0, 0, []
    for F, W, U in zip(frames, plan.counts, plan.used):
        assert (W, U) == ft.track_windows(F, T, hop)
        want.append(base + hop * np.arange(W))
        mine = plan.starts[first:first + W]
        assert mine.min() >= base and mine.max() + T <= base + U          # a window never leaves its track's rows
        base, first = base + U, first + W
    assert plan.starts.dtype == np.int64 and np.array_equal(plan.starts, np.concatenate(want))
    eager = ft.plan_track_windows([36, 66], T, hop, drop_last_aligned=False)
    assert eager.counts == [2, 7] and eager.used == [36, 66] and eager.starts.tolist() == [0, 6] + list(range(36, 78, 6))
    with pytest.raises(ValueError, match="track 1 of 30 frames has no window"):
        ft.plan_track_windows([41, 30], T, hop, who="somebody")
    empty = ft.plan_track_windows([30], T, hop, allow_empty=True)
    assert empty.counts == [0] and empty.U == 0 and empty.starts.size == 0


def test_padding_rule():
    for F in range(1, 21):
        src = torch.arange(F * 6, dtype=torch.float32).view(F, 3, 2) + 1           # no zero in it
        for a, b in itertools.combinations(range(F + 1), 2):
            for q in (1, 4, 8):
                pad = (a - b) % q
                chunk, lo = ft.pad_chunk(src, a, b, q)
                assert chunk.shape[0] == b - a + pad and chunk.shape[1:] == src.shape[1:], (F, a, b, q)
                assert torch.equal(chunk[lo:lo + b - a], src[a:b]), (F, a, b, q)
                view = chunk.untyped_storage().data_ptr() == src.untyped_storage().data_ptr()
                assert view == (b + pad <= F or a >= pad), (F, a, b, q)
                if b + pad <= F:                                            # trailing neighbours, also where both apply
                    assert lo == 0 and torch.equal(chunk, src[a:b + pad])
                elif a >= pad:                                              # leading neighbours
                    assert lo == pad and torch.equal(chunk, src[a - pad:b])
                else:                                                       # zeros behind the frames
                    assert lo == 0 and not chunk[b - a:].any()


def test_join_rows():
    a, b = torch.ones(2, 3), torch.zeros(1, 3)
    assert ft.join_rows([a]) is a
    assert torch.equal(ft.join_rows([a, b]), torch.cat([a, b]))


def _raises(kind, fn, *args):
    with pytest.raises(kind, match="somebody"):
        fn(*args, "somebody")


def test_checks_refuse_host_tensors_first():
    # no device here: a well-formed host tensor gets as far as the device refusal and no further
    _raises(RuntimeError, ft.check_frames, torch.zeros(2, 32, 4))
    _raises(RuntimeError, ft.check_frames, np.zeros((2, 32, 4), np.float32))
    _raises(RuntimeError, ft.check_crops, torch.zeros(2, 4, 30, 32))
    _raises(RuntimeError, ft.check_raw, torch.zeros(9, 5), torch.zeros(3, dtype=torch.int32), None, 32)
    _raises(RuntimeError, ft.check_ragged, torch.zeros(9, 4), torch.zeros(9), torch.zeros(3, dtype=torch.int32), 2, 32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ft.check_frames(torch.zeros(2, 32, 4), "somebody")


def test_checks_refuse_each_defect(monkeypatch):
    # what follows the device refusal, reached on host tensors by letting them pass for device tensors
    monkeypatch.setattr(torch.Tensor, "is_cuda", True)
    frames = torch.zeros(4, 32, 4)
    ft.check_frames(frames, "somebody")
    ft.check_frames(frames[:0], "somebody")
    for bad in (frames.view(4, -1), frames.double(), frames[::2], frames[:, :, :2]):     # rank, dtype, layout twice
        _raises(ValueError, ft.check_frames, bad)
    with pytest.raises(ValueError, match="empty"):
        ft.check_frames(frames[:0], "somebody", empty_ok=False)

    ft.check_crops(torch.zeros(0, 4, 30, 32), "somebody")
    _raises(ValueError, ft.check_crops, torch.zeros(2, 4, 30))
    with pytest.raises(ValueError, match="empty"):
        ft.check_crops(torch.zeros(0, 4, 30, 32), "somebody", empty_ok=False)

    points, offsets, pick = torch.zeros(9, 5), torch.tensor([0, 4, 9], dtype=torch.int32), torch.zeros(2, 32, dtype=torch.int32)
    assert ft.check_raw(points, offsets, None, 32, "somebody") == 2 == ft.check_raw(points.double(), offsets, pick, 32, "somebody")
    assert ft.check_raw(points[:0], offsets[:1], pick[:0], 32, "somebody") == 0
    for p, o, k in ((points[:, :4], offsets, None), (points.view(-1), offsets, None), (points.half(), offsets, None),
                    (points, offsets.long(), None), (points, offsets.view(1, 3), None), (points, offsets[:0], None),
                    (points, offsets, pick.long()), (points, offsets, pick[:1]), (points, offsets, pick[:, :31]),
                    (points, offsets, pick.view(-1))):
        _raises(ValueError, ft.check_raw, p, o, k, 32)

    rows, weight, u_off = torch.zeros(9, 4), torch.zeros(9), torch.tensor([0, 4, 9], dtype=torch.int32)
    assert ft.check_ragged(rows, weight, u_off, 2, 32, "somebody") == (9, 4)
    for r, w, u, n in ((rows.view(-1), weight, u_off, 2), (rows.double(), weight, u_off, 2), (rows[:, :2], weight, u_off, 2),
                       (rows[:0], weight[:0], u_off, 2), (rows, weight[:-1], u_off, 2), (rows, weight.double(), u_off, 2),
                       (rows, weight, u_off[:-1], 2), (rows, weight, u_off.long(), 2), (rows, weight, u_off, 3)):
        _raises(ValueError, ft.check_ragged, r, w, u, n, 32)
