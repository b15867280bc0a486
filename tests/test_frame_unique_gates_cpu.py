"""The reference and the cases of tests/frame_unique_ref.py on the CPU: the case frames expose every planted defect, the
host planner cuts the chunks it promises, the ABI declares the new entry points, and the scorer scenario's cap holds for
the fp64 oracle alone.  No kernel runs here; tests/test_frame_unique_branches.py holds the GPU side."""
import numpy as np
import pytest

import frame_unique_ref as FU
import raw_unique_ref as R
from helpers import T, make_encoder
from opensetgaitrecognition_pcaa_amd import constants


def test_unique_rows_first_orders_by_first_occurrence():
    b = FU.bits(np.array([[5, 1], [2, 1], [5, 1], [9, 1], [2, 1], [5, 1]], np.float32))
    first, mult = FU.unique_rows_first(b)
    assert first.tolist() == [0, 1, 3] and mult.tolist() == [3, 2, 1]
    u_off, weight, rows = FU.table(b[None])
    assert u_off.tolist() == [0, 3] and weight[:4].tolist() == [3, 2, 1, 0] and rows.shape == (256, 2)
    assert np.array_equal(rows[:3], b[[0, 1, 3]]) and not rows[3:].any() and not weight[3:].any()


def test_bits_decide_not_values():
    """-0.0 and +0.0 are two points; NaNs of one payload are one point, of another payload another"""
    z = FU.bits(np.array([[0.0], [-0.0], [0.0]], np.float32))
    assert FU.unique_rows_first(z)[1].tolist() == [2, 1]
    nan = np.array([[0x7FC00000], [0x7FC00001], [0x7FC00000]], np.int32)
    assert FU.unique_rows_first(nan)[1].tolist() == [2, 1]


@pytest.mark.parametrize("defect", FU.DEFECTS)
def test_the_case_frames_expose_the_defect(defect):
    """what the GPU file compares exactly (u_off, weight, the rows) differs under the defect at some listed (N, C)"""
    seen = []
    for N, C in FU.SHAPES:
        b = FU.bits(FU.case_frames(N, C))
        u_off, weight, rows = FU.table(b)
        assert (np.add.reduceat(weight[:u_off[-1]], u_off[:-1]) == N).all()
        M = max(weight.size, FU.table_rows(FU.table(b, defect=defect)[0][-1]))
        good, bad = FU.table(b, M=M), FU.table(b, M=M, defect=defect)
        if not all(np.array_equal(g, w) for g, w in zip(good, bad)):
            seen.append((N, C))
    print(f"[frame unique] {defect}: seen at {seen}")
    assert seen, defect
    if defect == "first_four_words":
        assert all(C == 5 for _, C in seen)
    if defect == "wave_local":
        assert all(N >= 65 for N, _ in seen)


def test_plan_unique_chunks_against_hand_written_tables():
    from opensetgaitrecognition_pcaa_amd import ops
    plan = ops.plan_unique_chunks
    assert plan([0], 100) == []                                         # n = 0
    assert plan([0, 40, 70, 100], 100) == [(0, 3, 256)]                 # the budget exactly met
    assert plan([0, 40, 70, 101], 100) == [(0, 2, 256), (2, 3, 256)]    # one row over
    assert plan([0, 32], 32) == [(0, 1, 256)]                           # a single frame of N rows equal to the budget
    assert plan([0, 32, 64, 96], 32) == [(0, 1, 256), (1, 2, 256), (2, 3, 256)]
    # the M rounding: 256 rows stay 256, 257 become 512
    assert plan([0, 200, 256, 457, 513], 300) == [(0, 2, 256), (2, 4, 512)]
    assert ops.unique_chunk_rows(0) == 256 and ops.unique_chunk_rows(256) == 256 and ops.unique_chunk_rows(257) == 512
    assert ops.unique_chunk_rows(256) == ops.UNIQUE_ROW_QUANTUM == FU.QUANTUM
    # every chunk within the budget, the chunks cover the frames in order
    rng = np.random.default_rng(0)
    u = np.concatenate([[0], np.cumsum(rng.integers(1, 33, 500))])
    chunks = plan(u, 700)
    assert chunks[0][0] == 0 and chunks[-1][1] == 500 and all(x[1] == y[0] for x, y in zip(chunks, chunks[1:]))
    for a, b, M in chunks:
        assert a < b and u[b] - u[a] <= 700 and M == FU.table_rows(u[b] - u[a])
        assert b == 500 or u[b + 1] - u[a] > 700                       # and no chunk could have taken one frame more
    with pytest.raises(ValueError):
        plan([0, 33], 32)                                               # a frame above the budget
    with pytest.raises(ValueError):
        plan([0, 5, 3], 32)


def test_the_abi_declares_the_entry_points():
    from opensetgaitrecognition_pcaa_amd import _lib
    protos = _lib.parse_header()
    lib = _lib.load()
    for name in ("pcaa_frames_unique_offsets", "pcaa_frames_unique"):
        assert name in protos and hasattr(lib, name), name
    assert lib.pcaa_abi_version() == _lib.ABI_VERSION >= 26
    # argument checks run on the host, before any launch
    ok = dict(frames=16, n=1, N=8, C=4, u_off=16, stream=None)
    for change in (dict(N=1025), dict(N=0), dict(C=6), dict(C=0), dict(n=-1), dict(u_off=None), dict(frames=None),
                   dict(frames=18), dict(n=2 ** 21, N=1024)):
        assert lib.pcaa_frames_unique_offsets(*{**ok, **change}.values()) != 0, change
        assert lib.pcaa_last_error().startswith(b"pcaa_frames_unique_offsets") and b"launch" not in lib.pcaa_last_error()
    ok = dict(frames=16, n=4, N=8, C=4, u_off=16, a=0, b=4, rows=16, weight=16, M=256, seg_off=16, err=None, stream=None)
    for change in (dict(N=1025), dict(C=6), dict(C=0), dict(M=0), dict(M=2 ** 31), dict(rows=None), dict(weight=None),
                   dict(u_off=None), dict(seg_off=None), dict(frames=None), dict(a=-1), dict(a=3, b=2), dict(b=5),
                   dict(rows=18), dict(n=2 ** 21, N=1024)):
        assert lib.pcaa_frames_unique(*{**ok, **change}.values()) != 0, change
        assert lib.pcaa_last_error().startswith(b"pcaa_frames_unique:") and b"launch" not in lib.pcaa_last_error()


def test_the_scorer_scenario_leaves_the_oracle_enough_safe_windows():
    """the cap of the GPU scorer tests (at most 10 % of the windows under the margin rule) holds for the fp64 oracle alone,
    and the scenario's padded frames do repeat points"""
    frames, cards = FU.scenario_track()
    N, C = FU.SCENARIO_N, FU.SCENARIO_C
    assert frames.shape == (131, N, C)
    distinct = int(FU.table(FU.bits(frames))[0][-1])
    assert distinct == int(np.minimum(cards, N).sum()) < 131 * N
    enc = make_encoder(FU.SCENARIO_K, N, C, True, seed=0).eval()
    sd = R.sd64(enc)
    logits = R.oracle_window_logits(sd, R.oracle_frame_features(sd, frames), T, constants.CROP_STEP, True)
    assert logits.shape[0] == 17
    for mode in ("fp32", "bf16"):
        excluded = int((~R.safe_windows(logits, mode)).sum())
        print(f"[frame unique] scenario {mode}: {excluded} of 17 windows excluded; {distinct} distinct rows of {131 * N}")
        assert excluded <= R.MAX_EXCLUDED * 17
