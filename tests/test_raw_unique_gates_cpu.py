"""The references and gates of tests/raw_unique_ref.py on the CPU: they reproduce the identity the padding-free raw path
rests on, and they reject planted defects.  No kernel runs here; tests/test_raw_unique_branches.py holds the GPU side."""
import numpy as np
import pytest
import torch

import raw_unique_ref as R
from helpers import make_encoder
from opensetgaitrecognition_pcaa_amd import datasets, synthetic as syn

N, C = 32, 4


@pytest.fixture(scope="module")
def case():
    """three synthetic tracks' frames, their picks, the oracle's per-point activations on the padded frames"""
    enc = make_encoder(4, N, C, True, seed=0).eval()
    sd = R.sd64(enc)
    raw = [fr for s in (300, 301, 302) for fr in syn.synthetic_raw_track(s, 14, max_points=60)]
    raw.append(R.make_frame(np.random.default_rng(1), 1))
    cards = R.cards_of(raw)
    np.random.seed(3)
    picks = datasets.draw_picks(cards, N)
    offsets = np.concatenate([[0], np.cumsum(cards)])
    padded = R.padded_frames64(raw, picks, C)
    M = int(np.minimum(cards, N).sum()) + 5
    return dict(sd=sd, raw=raw, cards=cards, picks=picks, offsets=offsets, padded=padded, M=M, P=int(cards.sum()),
                want=R.oracle_frame_features(sd, padded))


def _ragged(case, defect=None, picks=None, offsets=None, pool_defect=None, bad_as_zero=False):
    picks = case["picks"] if picks is None else picks
    offsets = case["offsets"] if offsets is None else offsets
    u_off, weight, src = R.compact_plan(offsets, case["P"], picks, N, case["M"], defect=defect)
    rows = R.gather_rows(case["padded"], src)
    if pool_defect is None:
        return R.oracle_ragged_features(case["sd"], rows, weight, u_off, N, bad_as_zero=bad_as_zero), (u_off, weight, src)
    return R.weighted_pool(R.oracle_point_features(case["sd"], rows), weight, u_off, N, defect=pool_defect)[0], (u_off, weight, src)


def test_the_identity_in_fp64(case):
    """the weighted pool of the per-point activations on the distinct rows = the padded mean, to 1e-12 of scale"""
    got, (u_off, weight, src) = _ragged(case)
    scale = np.abs(case["want"]).max()
    err = np.abs(got - case["want"]).max() / scale
    rows_padded, rows_ragged = case["cards"].size * N, int(u_off[-1])
    print(f"[raw unique] identity: {err:.2e} of scale; network rows {rows_ragged} against {rows_padded} padded")
    assert err <= 1e-12
    assert rows_ragged == int(np.minimum(case["cards"], N).sum()) < rows_padded
    # every frame's weights add up to N, the rows behind u_off[n] carry none
    sums = np.add.reduceat(weight[:u_off[-1]], u_off[:-1])
    assert (sums == N).all() and not weight[u_off[-1]:].any() and (src[u_off[-1]:] == -1).all()


def test_unique_first_orders_by_first_occurrence():
    first, mult = R.unique_first([5, 2, 5, 9, 2, 5])
    assert first.tolist() == [0, 1, 3] and mult.tolist() == [3, 2, 1]
    first, mult = R.unique_first([7])
    assert first.tolist() == [0] and mult.tolist() == [1]


@pytest.mark.parametrize("defect", ["mult_off_by_one", "raw_order"])
def test_the_table_comparison_rejects_a_wrong_layout(case, defect):
    """what the GPU file compares exactly (u_off, weight, the rows) differs under the defect -- and for the multiplicity the
    pooled feature leaves the fp32 parity gate"""
    u_off, weight, src = R.compact_plan(case["offsets"], case["P"], case["picks"], N, case["M"])
    u2, w2, s2 = R.compact_plan(case["offsets"], case["P"], case["picks"], N, case["M"], defect=defect)
    assert np.array_equal(u_off, u2)
    if defect == "mult_off_by_one":
        assert not np.array_equal(weight, w2)
        got, _ = _ragged(case, defect=defect)
        assert np.abs(got - case["want"]).max() > R.MODE_GATE["fp32"] * np.abs(case["want"]).max()
    else:
        # only frames with card >= N are re-ordered, and they are: their rows differ, their pooled feature does not (a
        # sum does not see the order) -- which is why the rows are compared, not only the features
        changed = np.flatnonzero(src != s2)
        frames = np.unique(np.searchsorted(u_off, changed, side="right") - 1)
        assert frames.size and (case["cards"][frames] >= N).all()
        assert not np.array_equal(R.gather_rows(case["padded"], src), R.gather_rows(case["padded"], s2))


def test_the_pool_gate_rejects_a_dropped_inv_n(case):
    u_off, weight, src = R.compact_plan(case["offsets"], case["P"], case["picks"], N, case["M"])
    a = R.oracle_point_features(case["sd"], R.gather_rows(case["padded"], src)).astype(np.float32)
    want, gate = R.weighted_pool(a, weight, u_off, N)
    wrong, _ = R.weighted_pool(a, weight, u_off, N, defect="no_inv_n")
    assert R.ratio(wrong, want, gate) > 1e3
    # while an fp32 evaluation in another order stays inside it
    got = np.stack([(weight[u_off[f]:u_off[f + 1], None] * a[u_off[f]:u_off[f + 1]])[::-1].sum(axis=0, dtype=np.float32)
                    / np.float32(N) for f in range(u_off.size - 1)])
    assert R.ratio(got, want, gate) <= 1.0


def test_the_pool_gate_with_the_affine_map(case):
    """v = ELU(y scale + shift) evaluated in fp32 stays inside the gate; with the shift's sign flipped it does not"""
    rng = np.random.default_rng(5)
    M, ch = 90, 16
    y = rng.standard_normal((M, ch)).astype(np.float32) * 3
    scale, shift = (rng.standard_normal(ch) * 0.7).astype(np.float32), rng.standard_normal(ch).astype(np.float32)
    weight = rng.integers(1, 6, M).astype(np.float32)
    u_off = np.array([0, 1, 3, 66, 90], dtype=np.int32)
    want, gate = R.weighted_pool(y, weight, u_off, 32, scale, shift)
    z = torch.from_numpy(y) * torch.from_numpy(scale) + torch.from_numpy(shift)
    v = torch.nn.functional.elu(z).numpy()
    got = np.stack([(weight[a:b, None] * v[a:b]).sum(axis=0, dtype=np.float32) / np.float32(32)
                    for a, b in zip(u_off[:-1], u_off[1:])])
    assert R.ratio(got, want, gate) <= 1.0
    wrong, _ = R.weighted_pool(y, weight, u_off, 32, scale, -shift)
    assert R.ratio(wrong, want, gate) > 1e3


def test_a_bad_frame_pools_to_f_of_zero_not_to_zero(case):
    """a frame with an out-of-range pick and one with no detections: one zero row of weight N each, pooled f(0), which is
    what the oracle makes of the padded path's all-zero frame; pooled as 0 it misses by the whole feature"""
    picks = case["picks"].copy()
    picks[4, 7] = case["cards"][4]                      # one past the frame's last detection
    offsets = case["offsets"].copy()
    offsets[9:] -= case["cards"][8]                     # frame 8 loses its detections: card 0
    padded = case["padded"].copy()
    padded[[4, 8]] = 0.0                                # what frames_from_raw writes for them
    want = R.oracle_frame_features(case["sd"], padded[[3, 4, 8]])
    u_off, weight, src = R.compact_plan(offsets, case["P"], picks, N, case["M"])
    assert u_off[9] - u_off[8] == 1 and weight[u_off[4]] == N and weight[u_off[8]] == N
    assert not weight[u_off[4] + 1:u_off[5]].any() and (src[u_off[4]:u_off[5]] == -1).all()
    rows = R.gather_rows(padded, src)
    got = R.oracle_ragged_features(case["sd"], rows, weight, u_off, N)[[3, 4, 8]]
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= 1e-12 * scale
    assert np.abs(want[1]).max() > 0.01 * scale         # f(0) is not small
    wrong = R.oracle_ragged_features(case["sd"], rows, weight, u_off, N, bad_as_zero=True)[[3, 4, 8]]
    assert np.abs(wrong - want).max() > R.MODE_GATE["bf16"] * scale


def test_lik_bound_covers_a_moved_embedding():
    """the relative likelihood bound holds for embeddings moved by up to g per component, and is not vacuous"""
    from oracle import pcaa_oracle as O
    rng = np.random.default_rng(2)
    means = rng.standard_normal((4, 32)) * 3
    x = rng.standard_normal((50, 32))
    for g in (1e-5, 1e-3):
        moved = x + rng.uniform(-g, g, x.shape)
        lik, lik2 = O.joint_likelihood(x, means), O.joint_likelihood(moved, means)
        bound = R.lik_rel_bound(x, means, g)
        assert (np.abs(lik2 - lik) <= bound * lik).all()
        assert bound.max() < 1.0 and (np.abs(O.joint_likelihood(x + 50 * g, means) - lik) > bound * lik).any()


def test_the_abi_declares_the_entry_points():
    from opensetgaitrecognition_pcaa_amd import _lib
    protos = _lib.parse_header()
    lib = _lib.load()
    for name in ("pcaa_frames_from_raw_unique", "pcaa_segment_weighted_mean"):
        assert name in protos and hasattr(lib, name), name
    assert lib.pcaa_abi_version() == _lib.ABI_VERSION >= 25
    # argument checks run on the host, before any launch: null pointers, ch % 8, the leading dimension, N above the cap
    assert lib.pcaa_segment_weighted_mean(None, 0, 8, None, None, 1, 8, 8, 32, None, None, None, None, None) != 0
    assert b"null" in lib.pcaa_last_error()
    for ch, lda in ((12, 12), (8, 4), (16, 12)):
        assert lib.pcaa_segment_weighted_mean(16, 0, lda, 16, 16, 1, 8, ch, 32, None, None, 16, None, None) != 0, (ch, lda)
    assert lib.pcaa_segment_weighted_mean(16, 0, 8, 16, 16, 1, 8, 8, 32, 16, None, 16, None, None) != 0     # scale alone
    assert lib.pcaa_segment_weighted_mean(16, 1, 8, 16, 16, 1, 8, 8, 32, None, None, 24, None, None) != 0   # out misaligned
    ok = dict(points=None, f64=0, P=0, offsets=None, n=0, pick=None, key=None, seed=0, N=8, C=4, st=1, div=0, rows=16,
              weight=16, u_off=16, M=256, pick_out=None, err=None, stream=None)
    for change in (dict(N=1025), dict(C=6), dict(C=0), dict(M=0), dict(rows=None), dict(weight=None), dict(u_off=None),
                   dict(n=1, offsets=16, points=16), dict(n=2 ** 21)):
        assert lib.pcaa_frames_from_raw_unique(*{**ok, **change}.values()) != 0, change
