"""References, gates, input generators and planted defects of the run-time enrolment kernels (csrc/gallery.hip), written
from the rule alone: used by tests/test_gallery_branches.py and tests/test_gallery_scorers.py on the
GPU and shown to be sharp by tests/test_gallery_gates_cpu.py on the CPU.  No GPU needed to import.

The rule
--------
A gallery is ``centroids`` fp32 [E, D] with ``counts`` int32 [E]; slot e with count > 0 is a live mode and identity e.
For a window x with the classifier's prediction p, against the prior means [Kc, D]:
    lik   = (sum over the Kc prior modes + sum over the live slots of exp(-0.5 (D log 2pi + |x - m|^2))) / Kc
    near  = the mode of smallest squared distance among 0 .. Kc + E - 1 (live ones), the lowest index on exact ties
    label = p if near < Kc else n_labels + 1 + (near - Kc)
``gallery_score_ref`` evaluates it in np.longdouble where that is wider than double, else with math.fsum over exact
products, as ``critic_loss_ref.joint_likelihood_ref`` does.

The gate of lik
---------------
The derivation of ``critic_loss_ref`` (Scoring) carries over with n = Kc + E_live terms and the divisor Kc: every term's
argument a_m is off by at most (D + 4) 2^-53 |a_m|, exp adds 4 2^-53 relative, the n positive terms add in ANY order with
at most n 2^-53 relative, the division rounds once, denormal terms sit on a grid of 2^-1074:
    gate = sum_m t_m ((D + 4) |a_m| + 4) 2^-53 / Kc + (n + 1) 2^-53 lik + (n + 2) 2^-1074.
``near``, ``labels`` and the votes are integers and must be equal.

Conditions on the inputs (asserted here, on the reference; no row is excluded)
-----------------------------------------------------------------------------
* every row's best and second-best squared distance differ by more than 2^-40 relative in the wide arithmetic, or are
  an exact planted tie (``check_separation``);
* no likelihood lies within 10 gates of the threshold used for a vote (``check_threshold``).

The vote: known iff #(lik > thr) > k/2, then argmax(bincount(labels)), else n_labels (``gallery_vote_ref``).
The centroid: np.float32(cumsum_in_float64[-1] / count) (``centroid_ref``).
"""
import itertools
import math

import numpy as np
import torch

import critic_loss_ref as R
from critic_loss_ref import U64, WIDE

GALLERY_DEFECTS = ("divisor_kc_plus_e", "empty_slot_at_zero", "highest_on_ties", "gallery_beats_prior_on_ties",
                   "label_n_labels_plus_slot", "fp32_distance")
VOTE_DEFECTS = ("vote_below_n_classes",)

# (B, Kc, D, E, which slots are empty)
CASES = [(1, 1, 1, 0, None), (1, 4, 32, 1, None), (127, 1, 1, 63, None), (128, 8, 33, 64, None), (129, 4, 32, 65, None),
         (300, 8, 32, 300, "third"), (64, 8, 32, 1024, None)]
ACC_M = (1, 2, 65, 257)


def case_id(c):
    return "x".join(str(v) for v in c if v is not None)


# ------------------------------------------------------------------------------------------------ inputs
def gallery_case(B, Kc, D, E, empty=None, device="cpu"):
    """-> dict: ``x`` fp32 [B, D], ``preds`` int64 [B], ``means`` fp32 [Kc, D], ``centroids`` fp32 [max(E, 1), D], ``counts``
    int32 [max(E, 1)], ``E``, ``n_labels`` (= Kc), ``tie_pairs`` (the pairs of mode indices planted at equal distance), ``mid_row``.  Rows sit at
    squared distance 0, 50, the denormal boundary (1460 - D log 2pi) and 1600 from a live mode in turn, the modes taken in
    turn too, as ``critic_loss_ref.likelihood_inputs`` does.  ``empty="third"``: every third slot has count 0 and a zero
    centroid (what ``Gallery.remove`` leaves).  Where D >= 32, planted ties: the first two live slots hold bit-equal
    centroids (E_live >= 3), and the last row lies exactly midway between the last prior mean and the last live slot."""
    seed = R.seed_of(B, 10 * Kc + D) + 7 * E
    means = R.uniform(Kc * D, seed, "cpu", -2.0, 2.0).view(Kc, D).float()
    Eb = max(E, 1)
    cent = torch.zeros(Eb, D)
    counts = np.zeros(Eb, np.int32)
    if E:
        cent = R.uniform(E * D, seed + 2, "cpu", -2.0, 2.0).view(E, D).float()
        counts = (1 + np.arange(E) % 3).astype(np.int32)
        if empty == "third":
            counts[2::3] = 0
            cent[2::3] = 0.0
    live = np.flatnonzero(counts > 0) if E else np.zeros(0, np.int64)
    plant = D >= 32 and live.size >= 1
    sgn = torch.where(R.uniform(D, seed + 3, "cpu") < 0.5, -1.0, 1.0).float()
    if plant and live.size >= 3:
        cent[live[1]] = cent[live[0]]
    if plant:                                   # the grid 2^-10 makes mean +- 1/4 and mean +- 1/2 exact in fp32
        means[Kc - 1] = torch.round(means[Kc - 1] * 1024.0) / 1024.0
        cent[live[-1]] = means[Kc - 1] + 0.5 * sgn
    modes = torch.cat([means, cent[live]]).double()
    n = modes.shape[0]
    b = torch.arange(B)
    d2 = torch.tensor([0.0, 50.0, 1460.0 - D * R.LOG2PI, 1600.0], dtype=torch.float64)[(b + b // n) % 4]
    sign = torch.where(R.uniform(B * D, seed + 1, "cpu").view(B, D) < 0.5, -1.0, 1.0)
    x = (modes[b % n] + sign * torch.sqrt(d2 / D).view(B, 1)).float()
    pairs = set()
    if plant:
        x[B - 1] = means[Kc - 1] + 0.25 * sgn
        pairs.add((Kc - 1, Kc + int(live[-1])))
        if live.size >= 3:                      # every row sees the twin slots at the same distance
            pairs.add((Kc + int(live[0]), Kc + int(live[1])))
    preds = ((b * 5 + 1) % Kc).long()
    dev = torch.device(device)
    return {"x": x.contiguous().to(dev), "preds": preds.to(dev), "means": means.contiguous().to(dev),
            "centroids": cent.contiguous().to(dev), "counts": torch.from_numpy(counts).to(dev), "E": E, "n_labels": Kc,
            "tie_pairs": pairs, "mid_row": B - 1 if plant else None}


# ------------------------------------------------------------------------------------------------ the score
def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _maha(x, modes, wide, fp32=False):
    """|x_b - m|^2 for every pair -> [B, n] in the wide type (fp32: the defect's float32 running sum)"""
    d64 = x.astype(np.float64)[:, None, :] - modes.astype(np.float64)[None]          # exact
    if fp32:
        d32 = d64.astype(np.float32)
        return np.cumsum(d32 * d32, axis=-1, dtype=np.float32)[..., -1].astype(np.longdouble if wide else np.float64)
    if wide:
        return (d64.astype(np.longdouble) ** 2).sum(-1)
    hi = np.float64(134217729.0) * d64                                               # Veltkamp split, as joint_likelihood_ref
    a = hi - (hi - d64)
    b_ = d64 - a
    return np.array([[math.fsum(np.concatenate([a[i, k] * a[i, k], 2 * a[i, k] * b_[i, k], b_[i, k] * b_[i, k]]))
                      for k in range(modes.shape[0])] for i in range(x.shape[0])])


def gallery_score_ref(x, preds, means, centroids, counts, E, n_labels, defect=None, wide=None):
    """-> dict of numpy: ``lik`` / ``gate`` float64 [B], ``near`` int32 [B], ``labels`` int64 [B], ``d2`` [B, Kc + E] in the
    wide arithmetic (inf at an empty slot)"""
    x, preds, mu = _np(x), _np(preds).astype(np.int64), _np(means)
    cent, cnt = _np(centroids)[:E], _np(counts)[:E]
    B, D = x.shape
    Kc = mu.shape[0]
    wide = WIDE if wide is None else wide
    ld = np.longdouble if wide else np.float64
    live = np.concatenate([np.ones(Kc, bool), cnt > 0 if defect != "empty_slot_at_zero" else np.ones(E, bool)])
    maha = _maha(x, np.concatenate([mu, cent.reshape(E, D)]), wide, fp32=defect == "fp32_distance").astype(ld)
    arg = ld(-0.5) * (ld(D) * np.log(ld(2) * ld(np.pi)) + maha)
    terms = np.where(live[None], np.exp(arg), ld(0))
    n = int(live.sum())
    lik = terms.sum(1) / (n if defect == "divisor_kc_plus_e" else Kc)
    a, t = np.abs(arg).astype(np.float64), terms.astype(np.float64)
    lik64 = lik.astype(np.float64)
    gate = (t * ((D + 4) * a + 4)).sum(1) * U64 / Kc + (n + 1) * U64 * lik64 + (n + 2) * 2.0 ** -1074
    d2 = np.where(live[None], maha, ld(np.inf))
    best = d2.min(1, keepdims=True)
    at = d2 == best
    if defect == "highest_on_ties":
        near = (Kc + E - 1 - np.argmax(at[:, ::-1], axis=1)).astype(np.int32)
    elif defect == "gallery_beats_prior_on_ties":
        in_gal = at[:, Kc:].any(1)
        near = np.where(in_gal, Kc + np.argmax(at[:, Kc:], axis=1) if E else 0, np.argmax(at, axis=1)).astype(np.int32)
    else:
        near = np.argmax(at, axis=1).astype(np.int32)
    off = n_labels if defect == "label_n_labels_plus_slot" else n_labels + 1
    labels = np.where(near < Kc, preds, off + (near.astype(np.int64) - Kc))
    return {"lik": lik64, "gate": gate, "near": near, "labels": labels, "d2": d2}


def check_separation(ref, tie_pairs=()):
    """the first condition: best and second-best squared distance apart by more than 2^-40 relative, or an exact tie
    between the two modes of a planted pair -> bool [B]: the rows that sit on such a tie"""
    d2 = ref["d2"]
    if d2.shape[1] < 2:
        return np.zeros(d2.shape[0], bool)
    order = np.argsort(d2, axis=1, kind="stable")[:, :2]
    two = np.take_along_axis(d2, order, axis=1)
    apart = (two[:, 1] - two[:, 0]) > 2.0 ** -40 * two[:, 1]
    planted = np.array([(int(a), int(b)) in tie_pairs for a, b in order])
    tie = (two[:, 1] == two[:, 0]) & planted
    bad = ~(apart | tie)
    assert not bad.any(), f"rows {np.flatnonzero(bad)[:8].tolist()}: best and second-best distance too close: {two[bad][:4]}"
    return tie


def check_threshold(lik, gate, thr):
    """the second condition: no likelihood within 10 gates of a vote's threshold"""
    close = np.abs(np.asarray(lik) - thr) <= 10 * np.asarray(gate)
    assert not close.any(), f"{int(close.sum())} likelihoods within 10 gates of the threshold {thr!r}"


def mid_threshold(lik, at=0.5):
    """the midpoint of two adjacent values of the distinct likelihoods, ``at`` of the way up (default: the two middle
    ones): both outcomes occur"""
    v = np.unique(np.asarray(lik, dtype=np.float64))
    assert v.size >= 2
    i = min(max(int(v.size * at), 1), v.size - 1)
    return float(0.5 * (v[i - 1] + v[i]))


# ------------------------------------------------------------------------------------------------ the vote
def gallery_vote_ref(lik, labels, thr, k, n_labels, defect=None, n_classes=None):
    lik, labels = np.asarray(lik, dtype=np.float64), np.asarray(labels, dtype=np.int64)
    nwin = len(labels) // k
    out = np.empty(nwin, dtype=np.int64)
    for w in range(nwin):
        lk, lb = lik[w * k:(w + 1) * k], labels[w * k:(w + 1) * k]
        if 2 * int(np.sum(lk > thr)) <= k:
            out[w] = n_labels
        elif defect == "vote_below_n_classes":
            out[w] = int(np.argmax(np.bincount(lb[lb < n_classes], minlength=n_classes)))
        else:
            out[w] = int(np.argmax(np.bincount(lb)))
    return out


def vote_exhaustive(label_set, ks=(1, 2, 3, 4), thr=0.5):
    """the patterns of ``critic_loss_ref.kvote_exhaustive`` over ``label_set``: every label tuple x every above / not above
    tuple -> {k: (lik, labels)}"""
    out = {}
    for k in ks:
        lik, labels = [], []
        for pr in itertools.product(range(len(label_set)), repeat=k):
            for ab in itertools.product((0, 1), repeat=k):
                labels.extend(label_set[i] for i in pr)
                lik.extend([2 * thr if a else (thr if (i + sum(pr)) % 2 else thr / 2) for i, a in enumerate(ab)])
        out[k] = (np.array(lik, dtype=np.float64), np.array(labels, dtype=np.int64))
    return out


# ------------------------------------------------------------------------------------------------ the centroid
def accumulate_inputs(n, D, seed=5, device="cpu"):
    """fp32 rows whose fp64 running sum rounds (magnitudes spread over 2^+-20: a sum in another order has other bits)"""
    v = R.uniform(n * D, seed, "cpu", -1.0, 1.0) * torch.exp2(torch.floor(R.uniform(n * D, seed + 1, "cpu", -20.0, 20.0)))
    return v.view(n, D).float().contiguous().to(device)


def centroid_ref(fv, rows=None, sums=None, count=0):
    """the host expression: ``np.float32(cumsum_in_float64[-1] / count)``, continuing ``sums`` / ``count`` -> (centroid
    fp32 [D], sums fp64 [D], count).  ``rows``: which rows in which order; an index out of range is skipped."""
    fv = _np(fv)
    rows = np.arange(fv.shape[0]) if rows is None else np.asarray(rows)
    rows = rows[(rows >= 0) & (rows < fv.shape[0])]
    start = np.zeros((1, fv.shape[1])) if sums is None or count == 0 else np.asarray(sums, dtype=np.float64).reshape(1, -1)
    run = np.cumsum(np.concatenate([start, fv[rows].astype(np.float64)]), axis=0, dtype=np.float64)[-1]
    total = int(count) + len(rows)
    return np.float32(run / total), run, total


# ------------------------------------------------------------------------------------------------ host bookkeeping
def ring_rows_brute(windows_per_tick, H, m, stream):
    """``fv_hist`` rows of a stream's last m windows, oldest first, by replaying every write into a list"""
    ring, j = [None] * H, 0
    for n in windows_per_tick:
        for _ in range(n):
            ring[j % H] = j
            j += 1
    want = list(range(j - m, j))
    assert all(w in ring for w in want)
    return [stream * H + ring.index(w) for w in want]


def accumulate_host(fv, slot, sums, counts, centroids, rows=None, err_flag=None):
    """``ops.gallery_accumulate`` restated on host tensors (the CPU file swaps it in to exercise ``Gallery``'s bookkeeping)"""
    c, s, n = centroid_ref(fv, None if rows is None else _np(rows), sums[slot].numpy(), int(counts[slot]))
    m = fv.shape[0] if rows is None else rows.numel()
    if err_flag is not None and n - int(counts[slot]) != m:
        err_flag.fill_(1)
    sums[slot] = torch.from_numpy(s)
    counts[slot] = n
    centroids[slot] = torch.from_numpy(np.asarray(c))


# ------------------------------------------------------------------------------------------------ the stream scenario
STREAM_KS = (1, 3)


def stream_scenario(k, device="cpu"):
    """One stream (slot 2 of 3) over four ticks of k + 1, 2k + 1, 0 and 2H + 1 windows with H = 3; slot 0 rides along in the
    first and the last tick, slot 1 never appears.  Identity 0 (a person the model was not trained on) is in the gallery
    from the start; identity 1 is enrolled between the second and the third tick from the stream's last H windows.
    Everything the GPU test compares against is computed here, on the host: per window the score against the gallery
    as it stood when the window was scored (a stored label is never recomputed), the votes over all windows, the
    threshold (the midpoint of two adjacent likelihoods a quarter of the way up).  The input conditions are asserted."""
    Kc, D, H, n_slots, nl = 4, 32, 3, 3, 4
    ticks = [k + 1, 2 * k + 1, 0, 2 * H + 1]
    n = sum(ticks)
    means = R.uniform(Kc * D, 71, "cpu", -2.0, 2.0).view(Kc, D).float()
    person = R.uniform(2 * D, 72, "cpu", -2.0, 2.0).view(2, D).float()
    i = torch.arange(n)
    enrol_after = ticks[0] + ticks[1]
    who = (i // k) % 3                                              # vote groups of: a trained class, person 0, person 1
    who[max(enrol_after - H, 0):enrol_after] = 2                    # (the windows the enrolment takes: person 1's)
    centre = torch.where((who == 0).view(n, 1), means[i % Kc], person[(who - 1).clamp_min(0)])
    fv = (centre.double() + R.uniform(n * D, 73, "cpu", -0.6, 0.6).view(n, D)).float().contiguous()
    logits = R.ce_inputs(n, Kc, 4.0, "cpu")[0]
    preds = R.ce_ref(logits)["preds"].cpu().numpy()
    other = (means[torch.arange(5) % Kc].double() + R.uniform(5 * D, 74, "cpu", -0.6, 0.6).view(5, D)).float().contiguous()
    other_logits = R.ce_inputs(5, Kc, 4.0, "cpu")[0]
    m = min(H, enrol_after)
    cent = np.zeros((2, D), np.float32)
    cent[0] = centroid_ref(person[:1])[0]
    counts = np.array([1, 0], np.int32)
    before = (cent.copy(), counts.copy(), 1)
    cent[1], counts[1] = centroid_ref(fv[enrol_after - m:enrol_after])[0], m
    after = (cent.copy(), counts.copy(), 2)
    parts = [gallery_score_ref(fv[a:b], preds[a:b], means, *state, nl)
             for a, b, state in ((0, enrol_after, before), (enrol_after, n, after))]
    for p in parts:
        check_separation(p)
    ref = {key: np.concatenate([p[key] for p in parts]) for key in ("lik", "gate", "labels")}
    thr = mid_threshold(ref["lik"], 0.25)
    check_threshold(ref["lik"], ref["gate"], thr)
    votes = gallery_vote_ref(ref["lik"], ref["labels"], thr, k, nl)
    lab = ref["labels"]
    assert (lab == nl + 1).any() and (lab == nl + 2).any() and (lab < nl).any()
    assert (lab[:enrol_after] != nl + 2).all() and (votes == nl).any() and (votes != nl).any()
    dev = torch.device(device)
    return {"Kc": Kc, "D": D, "H": H, "n_slots": n_slots, "n_labels": nl, "ticks": ticks, "n": n, "k": k, "thr": thr,
            "means": means.to(dev), "person": person.to(dev), "fv": fv.to(dev), "logits": logits.to(dev),
            "other": other.to(dev), "other_logits": other_logits.to(dev), "enrol_after": enrol_after, "m": m,
            "before": before, "after": after, "lik": ref["lik"], "gate": ref["gate"], "labels": lab, "votes": votes}
