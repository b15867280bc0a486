"""Host reference, case frames and planted defects of the distinct-row front for PADDED frames: ``ops.frames_unique_offsets``
and ``ops.frames_unique`` (csrc/frame_unique.hip) and the scorers' ``dedup_points`` on stored crops and processed tracks.
Used by tests/test_frame_unique_branches.py (the kernels, on the GPU) and tests/test_frame_unique_gates_cpu.py (the power
of the cases, on the CPU).  numpy on the host only.

The table
---------
Two rows of a frame are the same point iff all their C 32-bit words are equal as BITS, so the reference works on the int32
view of the frames: ``np.unique(axis=0, return_index, return_counts)`` re-ordered by the index gives the first positions
and the multiplicities (``unique_rows_first``).  Frame f owns rows ``u_off[f] .. u_off[f + 1] - 1`` of the table: its
distinct rows in order of first occurrence, weight = the multiplicity; the rows behind ``u_off[n]`` are zero with weight 0
(``table``).  Everything is compared EXACTLY (the rows as int32 bits): the kernel uses integer operations only, so there is
no gate to derive.  The scorer gates are those of tests/raw_unique_ref.py.

Planted defects: ``DEFECTS``; ``defect=`` of ``unique_rows_first`` / ``table`` returns what a subtly wrong kernel gives.
"""
import numpy as np

import raw_unique_ref as R
from opensetgaitrecognition_pcaa_amd import datasets

QUANTUM = 256                 # ops.UNIQUE_ROW_QUANTUM
DEFECTS = ("value_order", "float_equality", "first_four_words", "mult_off_by_one", "wave_local")
SHAPES = ((1, 4), (2, 1), (24, 5), (32, 4), (64, 4), (65, 3), (150, 5), (256, 4), (300, 2), (1024, 4))
MIN_INT32 = np.int32(-2 ** 31)            # the bits of -0.0


def bits(frames):
    """float32 [..., C] -> the same words as int32"""
    return np.ascontiguousarray(frames, dtype=np.float32).view(np.int32)


def unique_rows_first(frame_bits, defect=None):
    """int32 [N, C] -> (positions of the first occurrences, ascending; the multiplicity of the row at each)"""
    b = np.asarray(frame_bits)
    assert b.dtype == np.int32 and b.ndim == 2
    key = b
    if defect == "float_equality":
        # +0.0 == -0.0 as floats; a NaN equals nothing, itself included: a row that holds one gets a key of its own
        key = np.where(b == MIN_INT32, 0, b)
        nan = np.isnan(b.view(np.float32)).any(axis=1)
        key = np.concatenate([key, np.where(nan, np.arange(b.shape[0]), -1)[:, None].astype(np.int32)], axis=1)
    elif defect == "first_four_words":
        key = b[:, :4]
    elif defect == "wave_local":
        key = np.concatenate([b, (np.arange(b.shape[0]) // 64)[:, None].astype(np.int32)], axis=1)
    _, index, counts = np.unique(key, axis=0, return_index=True, return_counts=True)
    if defect != "value_order":
        order = np.argsort(index)
        index, counts = index[order], counts[order]
    if defect == "mult_off_by_one":
        counts = counts.copy()
        counts[-1] += 1
    return index, counts


def table_rows(need):
    """rows of a table that holds ``need`` distinct rows: whole quanta, at least one (ops.unique_chunk_rows)"""
    return max((int(need) + QUANTUM - 1) // QUANTUM, 1) * QUANTUM


def table(frames_bits, M=None, defect=None):
    """int32 [n, N, C] -> ``(u_off int32 [n + 1], weight fp32 [M], rows int32 [M, C])``; M defaults to ``table_rows``"""
    frames_bits = np.asarray(frames_bits)
    n, N, C = frames_bits.shape
    parts = [unique_rows_first(frames_bits[f], defect) for f in range(n)]
    u_off = np.concatenate([[0], np.cumsum([p[0].size for p in parts])]).astype(np.int64)
    M = table_rows(u_off[-1]) if M is None else int(M)
    assert u_off[-1] <= M
    weight = np.zeros(M, dtype=np.float32)
    rows = np.zeros((M, C), dtype=np.int32)
    for f, (first, mult) in enumerate(parts):
        rows[u_off[f]:u_off[f + 1]] = frames_bits[f][first]
        weight[u_off[f]:u_off[f + 1]] = mult
    return u_off.astype(np.int32), weight, rows


def distinct_frame(rng, N, C):
    """a frame whose N rows are all different"""
    fr = rng.standard_normal((N, C)).astype(np.float32)
    assert np.unique(bits(fr), axis=0).shape[0] == N
    return fr


def padded_frames(cards, N, C, seed):
    """frames of the given cardinalities padded (card < N) or subsampled (card > N) as ``process_track`` does it:
    ``datasets.draw_picks`` and ``datasets.frames_from_picks``, rounded to fp32 -> [len(cards), N, C]"""
    rng = np.random.default_rng(seed)
    raw = [R.make_frame(rng, c) for c in cards]
    np.random.seed(seed)
    picks = datasets.draw_picks(np.asarray(cards), N)
    return datasets.frames_from_picks(raw, picks, C).astype(np.float32)


def case_frames(N, C):
    """the frames every (N, C) is tested on -> float32 [n, N, C]; the docstring of each block says what it is there for"""
    rng = np.random.default_rng(1000 * N + C)
    out = [distinct_frame(rng, N, C),                                   # all rows distinct: every weight 1
           np.tile(distinct_frame(rng, 1, C), (N, 1)),                  # all rows equal: one row of weight N
           np.zeros((N, C), np.float32)]                                # the all-zero frame
    cards = sorted({c for c in (1, 2, N - 1, N, N + 1) if c >= 1})
    out += list(padded_frames(cards, N, C, seed=N + C))                 # repeat-padded / whole / subsampled frames
    if N >= 65:                                                         # first occurrence >= 64 rows earlier: another wave
        fr = distinct_frame(rng, N, C)
        fr[N - 1] = fr[0]
        fr[64] = fr[63]                                                 # and one right across the boundary
        out.append(fr)
    if N >= 257:                                                        # >= 256 rows earlier: another block of the rank scan
        fr = distinct_frame(rng, N, C)
        fr[N - 2] = fr[1]
        fr[256] = fr[255]
        out.append(fr)
    if N >= 2:
        fr = distinct_frame(rng, N, C)                                  # the lowest mantissa bit of the LAST feature differs
        b = bits(fr)
        b[1] = b[0]
        b[1, C - 1] ^= 1
        out.append(b.view(np.float32))
        fr = distinct_frame(rng, N, C)                                  # a +0.0 row and a -0.0 row: different points
        fr[0] = 0.0
        fr[N - 1] = -0.0
        out.append(fr)
    if N >= 3:
        b = bits(distinct_frame(rng, N, C))                             # two NaN rows of one payload, one of another
        b[0] = b[N - 1] = 0x7FC00000
        b[N // 2] = 0x7FC00001
        out.append(b.view(np.float32))
    return np.stack(out)


# ----------------------------------------------------------------------------------------------- the scorer scenario
SCENARIO_N, SCENARIO_C, SCENARIO_K = 32, 4, 4


def scenario_track():
    """the track of the scorer tests: ``synthetic_raw_track(41, 131, max_points=60)`` padded to N = 32 with the reference's
    draws -> (frames fp32 [131, 32, 4], the cardinalities)"""
    from opensetgaitrecognition_pcaa_amd import synthetic as syn
    raw = syn.synthetic_raw_track(41, 131, max_points=60)
    cards = R.cards_of(raw)
    np.random.seed(19)
    picks = datasets.draw_picks(cards, SCENARIO_N)
    return datasets.frames_from_picks(raw, picks, SCENARIO_C).astype(np.float32), cards
