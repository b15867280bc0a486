"""Open-set inference of the PCAA path on the HIP device (reference
``inference_PCAA.py``: ``CGAAE_inference_setup`` :34-114, ``naive_sequential_procedure``
:117-347, ``CGAAE_inference`` :382-469).

The reference evaluates the encoder one crop at a time (batch 1) and scores each embedding
with scipy on the host.  Here the eval-mode encoder runs batched (BatchNorm uses running
statistics, so every sequence is independent: the batched result equals the per-crop one),
the float64 mixture likelihood and the k-window vote run as HIP kernels, and only the ROC /
Youden threshold (a sort over a few thousand scores) stays on the host.  F1 / confusion
matrix plotting is reporting and out of scope.
"""
import ctypes
import os
import pickle

import numpy as np
import torch

from . import _lib, constants, frame_table
from . import functional as F_hip
from . import ops
from ._lib import check
from .datasets import RawPrep
from .models import CGEncoder


def joint_likelihood(sup_fv: torch.Tensor, means: torch.Tensor) -> torch.Tensor:
    """[B,32] fp32 embeddings, [K,32] fp32 centroids -> [B] float64 likelihoods."""
    ops._chk(sup_fv, "joint_likelihood.x", torch.float32, 2)
    ops._chk(means, "joint_likelihood.means", torch.float32, 2)
    B, D = sup_fv.shape
    K = means.shape[0]
    if means.shape[1] != D:
        raise ValueError("joint_likelihood: dimension mismatch")
    out = torch.empty(B, dtype=torch.float64, device=sup_fv.device)
    check(_lib.load().pcaa_joint_likelihood(ops._p(sup_fv), ops._p(means), B, K, D, ops._p(out), ops._s()),
          "pcaa_joint_likelihood")
    return out


def k_vote(lik: torch.Tensor, preds: torch.Tensor, threshold: float, k: int, n_labels: int,
           n_classes: int = None) -> torch.Tensor:
    """Windows of k consecutive crops (trailing partial window dropped, like DataLoader
    drop_last=True) -> [n_windows] int64 open-set predictions.  ``n_labels`` is the "unknown" id (the number
    of distinct labels in the known test split); the majority is taken over the encoder's ``n_classes``
    outputs (``np.argmax(np.bincount(preds))``, inference_PCAA.py:265-266) -- a test split that lacks a trained
    class must not drop the votes for it.  Default ``n_classes = n_labels``."""
    ops._chk(lik, "k_vote.lik", torch.float64, 1)
    ops._chk(preds, "k_vote.preds", torch.int64, 1)
    n_classes = int(n_labels if n_classes is None else n_classes)
    nwin = lik.numel() // k
    out = torch.empty(nwin, dtype=torch.int64, device=lik.device)
    if nwin:
        check(_lib.load().pcaa_kvote(ops._p(lik), ops._p(preds), ctypes.c_double(float(threshold)), int(k),
                                     int(n_labels), n_classes, nwin, ops._p(out), ops._s()), "pcaa_kvote")
    return out


def youden_threshold(known_mask: np.ndarray, scores: np.ndarray) -> float:
    """``thresholds[argmax(tpr - fpr)]`` of ``sklearn.metrics.roc_curve`` (default
    ``drop_intermediate=True``) as used at inference_PCAA.py:230-231: scores sorted
    descending (stable), one candidate per distinct score, collinear points dropped,
    (0,0) with threshold +inf prepended.  Host numpy: a sort of a few thousand float64."""
    y = np.asarray(known_mask, dtype=np.float64)
    s = np.asarray(scores, dtype=np.float64)
    order = np.argsort(s, kind="mergesort")[::-1]
    s, y = s[order], y[order]
    idx = np.r_[np.where(np.diff(s))[0], y.size - 1]
    tps = np.cumsum(y)[idx]
    fps = 1 + idx - tps
    thr = s[idx]
    if len(fps) > 2:
        keep = np.where(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])[0]
        fps, tps, thr = fps[keep], tps[keep], thr[keep]
    tps, fps, thr = np.r_[0, tps], np.r_[0, fps], np.r_[np.inf, thr]
    return float(thr[np.argmax(tps / tps[-1] - fps / fps[-1])])


def window_count(n_frames, T=constants.NSTEPS, hop=constants.CROP_STEP):
    """Number of crops the reference cuts out of a processed track of ``n_frames`` frames (its ``crop_with_step``,
    datasets.py:16-25, 297-302): one per start in ``arange(n_frames - T, step=hop)``.  The rule drops the last aligned
    window when ``(n_frames - T) % hop == 0`` and gives none for ``n_frames == T`` (``frame_table.track_windows``)."""
    return frame_table.track_windows(n_frames, T, hop)[0]


def plan_frames(same, M, T=constants.NSTEPS, hop=constants.CROP_STEP):
    """Host plan of the deduplicated pass over M sequentially ordered crops.  ``same`` [M - 1]: nonzero where crop i + 1
    starts with the last T - hop frames of crop i (``ops.crop_overlap``).  Returns ``(frame_src, win_row)``:
    ``frame_src`` int64 [U]: for every unique frame its index (crop * T + t) in the flat [M * T] frame array -- a run of
    L chained crops gives the first crop's T frames and the last ``hop`` frames of each later one;
    ``win_row`` int64 [M]: the row of the unique-frame table where crop i's window of T rows starts."""
    M, T, hop = int(M), int(T), int(hop)
    same = np.asarray(same).reshape(-1) != 0
    if M < 0 or same.size != max(M - 1, 0) or not 1 <= hop <= T:
        raise ValueError(f"plan_frames: needs a mask of M - 1 = {max(M - 1, 0)} entries and 1 <= hop <= T")
    if M == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    new = np.full(M, T, np.int64)
    new[1:][same] = hop                                   # frames crop i adds to the table
    ends = np.cumsum(new)                                 # table row after crop i's last frame
    win_row = ends - T
    # crop i's new frames are its LAST new[i] ones: t = T - new[i] .. T - 1
    first_t = np.repeat(np.arange(M, dtype=np.int64) * T + (T - new), new)
    within = np.arange(int(ends[-1]), dtype=np.int64) - np.repeat(ends - new, new)
    return first_t + within, win_row


def _ragged_features(enc, points, offsets, N, C, pick, seed, keys, err_flag, a=0, b=None, mode=None, consts=None, prep=None):
    """raw frames (``b``: frames a .. b - 1 of them; ``prep``: thinned and moved first) -> their distinct
    points and multiplicities -> (their [n, 1024] frame features, the PointNet layer records, rows of the compact table): the ``dedup_points``
    route of the raw entries"""
    rows, weight, u_off = frame_table.raw_frames(points, offsets, N, C, pick, seed, keys, err_flag, a, b, dedup_points=True,
                                                 prep=prep)
    feats, saves = F_hip.encoder_frame_features_ragged(enc, rows, weight, u_off, u_off.numel() - 1, N, mode, consts=consts)
    return feats, saves, rows.shape[0]


class _Rule:
    """The open-set rule of a scorer, decided once in its constructor: under the prior's modes alone (``gallery=None``),
    or with the identities a ``gallery.Gallery`` of the embedding width enrolled at run time beside them -- labels are
    then the extended ones (``preds`` where a prior mode is closest, ``n_labels + 1 + identity`` otherwise)."""

    def __init__(self, means, n_labels, n_classes, gallery, who):
        self.means, self.n_classes, self.gallery = means, int(n_classes), gallery
        self.n_labels = None if n_labels is None else int(n_labels)
        if gallery is None:
            return
        from .gallery import Gallery
        if not isinstance(gallery, Gallery) or gallery.D != int(means.shape[1]):
            raise ValueError(f"{who}: gallery must be a gallery.Gallery of width {int(means.shape[1])}")
        if self.n_labels is None or self.n_labels < 1:
            raise ValueError(f"{who}: a gallery needs n_labels >= 1 (the \"unknown\" id its labels are counted from)")

    def score(self, sup_fv, preds):
        """embeddings and the classifier's predictions -> (labels, likelihood)"""
        if self.gallery is None:
            return preds, joint_likelihood(sup_fv, self.means)
        lik, labels, _ = self.gallery.score(sup_fv, preds, self.means, self.n_labels)
        return labels, lik

    def vote(self, lik, labels, threshold, k, n_labels):
        if self.gallery is None:
            return k_vote(lik, labels, threshold, k, n_labels, n_classes=self.n_classes)
        return ops.gallery_vote(lik, labels, threshold, k, n_labels)

    def tick(self, logits, sup_fv, part, n_votes, threshold, k, hist_lik, hist_label, fv_hist):
        """one scoring launch for a tick's windows (``part``: its plan on the device) -> what ``_tick`` takes after the plan"""
        args = (logits, sup_fv, self.means, part["run_start"], part["win_stream"], part["win_j"], part["vote_pos"], n_votes,
                threshold, k, self.n_labels)
        if self.gallery is None:
            labels, lik, votes = ops.stream_score(*args, self.n_classes, hist_lik, hist_label)
        else:
            g = self.gallery
            labels, lik, _, votes = ops.stream_score_gallery(*args, g.centroids, g.counts, g.high_water, hist_lik, hist_label,
                                                             fv_hist)
        return labels, sup_fv, lik, votes


def _empty_triple(D, dev):
    """(preds, sup_fv, likelihood) of no window at all"""
    return (torch.empty(0, dtype=torch.int64, device=dev), torch.empty((0, D), dtype=torch.float32, device=dev),
            torch.empty(0, dtype=torch.float64, device=dev))


class OpenSetScorer:
    """Encoder + centroids -> predictions, likelihoods, threshold, k-window votes."""

    def __init__(self, encoder: CGEncoder, discriminator_means: torch.Tensor, batch_size: int = 1024, gallery=None,
                 n_labels: int = None):
        """``gallery`` (a ``gallery.Gallery``, with ``n_labels``, the "unknown" id): the identities enrolled at run time
        are scored beside the prior's modes -- every embed route then returns the extended labels (``preds`` where a
        prior mode is closest, ``n_labels + 1 + identity`` otherwise) in place of ``preds`` and the extended likelihood,
        and ``vote`` takes the majority over those labels.  Without one nothing changes."""
        self.last_preds = None               # with a gallery: the classifier's own predictions of the last embed
        self.encoder = encoder.eval()
        dev = next(encoder.parameters()).device
        self.means = discriminator_means.float().to(dev).contiguous()
        self._rule = _Rule(self.means, n_labels, encoder.MLP_sup2[0].weight.shape[0], gallery, "OpenSetScorer")
        self.gallery, self.n_labels = gallery, self._rule.n_labels
        self.batch_size = batch_size
        self.threshold = None
        self.last_frames_encoded = None      # unique frames the last deduplicated embed / embed_track encoded (no padding)
        self.last_pointnet_saves = None      # the PointNet layer records of its last chunk (which path ran)
        self.last_rows_encoded = None        # dedup_points=True: rows of the compact tables the last call ran
        self.raw_err = torch.zeros(1, dtype=torch.int32, device=dev)     # set by a raw frame that could not be processed
        self.unique_err = torch.zeros(1, dtype=torch.int32, device=dev)  # set by ops.frames_unique: a segment not its frame's

    @torch.no_grad()
    def embed(self, pcs: torch.Tensor, dedup_frames: bool = False, hop: int = constants.CROP_STEP,
              dedup_points: bool = False):
        """pcs [M,C,T,N] on the device -> (preds [M] int64, sup_fv [M,32], likelihood [M] f64).
        ``dedup_frames``: for sequentially ordered crops (cut with ``hop``), encode every frame that consecutive crops
        share bit for bit once (``_embed_frames``); same triple, same order, one entry per crop.
        ``dedup_points``: the stored crops carry their padding written out (``process_track`` repeats detections, every
        copy bit-equal); every frame's DISTINCT rows go through the PointNet block once and are pooled with their
        multiplicities (``ops.frames_unique_offsets`` / ``ops.frames_unique``,
        ``functional.encoder_frame_features_ragged``): the same features up to fp32 summation order.  One small copy to
        the host per call (the offsets, to plan the chunks); ``last_rows_encoded`` is the number of table rows it ran.
        The two options multiply."""
        if dedup_points or dedup_frames:
            return self._embed_frames(pcs, hop, dedup_frames, dedup_points)
        return self._score(F_hip.encoder_forward(self.encoder, pcs[i:i + self.batch_size], False)[:2]
                           for i in range(0, pcs.shape[0], self.batch_size))

    def _score(self, batches):
        """(logits, sup_fv) of one batch after the other -> the triple ``embed`` returns"""
        preds, fvs = [], []
        for logits, sup_fv in batches:
            _, _, p = ops.cross_entropy(logits, None, want_loss=False, want_preds=True)
            preds.append(p)
            fvs.append(sup_fv)
        preds, fvs = torch.cat(preds), torch.cat(fvs)
        if self.gallery is not None:
            self.last_preds = preds
        labels, lik = self._rule.score(fvs.contiguous(), preds)
        return labels, fvs, lik

    def _unique_features(self, frames):
        """padded frames [U, N, C] -> the chunks of their [U, 1024] feature table from their distinct rows: one offsets
        pass, ONE copy of the offsets to the host, chunks of at most the rows a padded chunk runs"""
        U, N, C = frames.shape
        u_off = ops.frames_unique_offsets(frames)

        def chunk(a, b, M):
            rows, weight, seg_off = ops.frames_unique(frames, u_off, a, b, M, err_flag=self.unique_err)
            return F_hip.encoder_frame_features_ragged(self.encoder, rows, weight, seg_off, b - a, N) + (M,)
        feats = self._chunk_features(ops.plan_unique_chunks(u_off.cpu().numpy(), self.batch_size * constants.NSTEPS * N), chunk)
        if self.unique_err.item():                     # u_off came from these very frames: an internal inconsistency
            self.unique_err.zero_()
            raise RuntimeError("OpenSetScorer: ops.frames_unique met a segment that is not its frame's (unique_err)")
        return feats

    def _chunk_features(self, chunks, features):
        """``dedup_points``: ``features(*chunk)`` -> (its frames' features, the PointNet records, its compact table's rows),
        chunk after chunk -> the chunks of the feature table; counts ``last_rows_encoded``"""
        feats, self.last_rows_encoded = [], 0
        for chunk in chunks:
            f, self.last_pointnet_saves, M = features(*chunk)
            self.last_rows_encoded += M
            feats.append(f)
        return feats

    def _embed_frames(self, pcs, hop, dedup_frames, dedup_points):
        """``embed`` with an option: the crops' frames -- with ``dedup_frames`` those that consecutive crops do not share
        (overlap mask: one launch, one small copy to the host; ``plan_frames``), gathered once -- through the PointNet block,
        with ``dedup_points`` their distinct rows only -> windows of the feature table through the temporal block and heads"""
        frame_table.check_crops(pcs, "CGEncoder", empty_ok=dedup_points)
        M, C, T, N = pcs.shape
        if M == 0:
            self.last_rows_encoded = 0
            return _empty_triple(self.encoder.MLP_sup1[0].weight.shape[0], pcs.device)
        xp = F_hip._point_major(pcs)                                       # [M, T, N, C] storage
        frames, win_row = xp.view(M * T, N * C), T * np.arange(M, dtype=np.int64)
        if dedup_frames:
            same = ops.crop_overlap(xp, hop).cpu().numpy() if M > 1 else np.zeros(0, np.int32)
            frame_src, win_row = plan_frames(same, M, T, hop)
            self.last_frames_encoded = len(frame_src)
        if dedup_points:
            if dedup_frames:
                frames = ops.gather_frames(frames, torch.from_numpy(frame_src).to(pcs.device))
            feats = self._unique_features(frames.view(-1, N, C))
        else:
            # the index form of frame_table.pad_chunk: whole GEMM row tiles, the padding gathers frame 0; features dropped
            q = F_hip.frame_pad_quantum(N)
            idx = torch.from_numpy(np.concatenate([frame_src, np.zeros((-len(frame_src)) % q, np.int64)])).to(pcs.device)
            step = max(self.batch_size * T // q, 1) * q
            feats = []
            for a in range(0, idx.numel(), step):
                rows = ops.gather_frames(frames, idx[a:a + step].contiguous())
                f, self.last_pointnet_saves = F_hip.encoder_frame_features(self.encoder, rows.view(-1, N, C))
                feats.append(f)
        table = frame_table.join_rows(feats)
        return self._score_windows(table, ops.WindowRows(win_row, T, table.shape[0], device=pcs.device), T)

    def _score_windows(self, table, plan, T):
        """windows of a frame-feature table, ``batch_size`` at a time -> the triple ``embed`` returns"""
        return self._score(F_hip.encoder_forward_windows(self.encoder, table, plan.slice(i, i + self.batch_size), T)[:2]
                           for i in range(0, len(plan), self.batch_size))

    @torch.no_grad()
    def embed_track(self, track: torch.Tensor, hop: int = constants.CROP_STEP, drop_last_aligned: bool = True,
                    dedup_points: bool = False):
        """track [F,N,C] fp32 on the device (a processed track as the packed store keeps it) -> the triple of ``embed``
        for its ``window_count(F)`` windows of NSTEPS frames, as if ``embed`` had been called on the reference's crops
        of it -- every frame encoded once, no crop ever written out.  ``drop_last_aligned=False`` also takes the
        aligned last window the reference's rule drops when ``(F - NSTEPS) % hop == 0``.  ``dedup_points``: as in
        ``embed`` -- the distinct rows of every frame once, pooled with their multiplicities."""
        frame_table.check_frames(track, "embed_track")
        F, N, C = track.shape

        def features(U):
            if dedup_points:
                return self._unique_features(track[:U])
            q = F_hip.frame_pad_quantum(N)
            step = max(self.batch_size * constants.NSTEPS // q, 1) * q
            feats = []
            for a in range(0, U, step):
                b = min(a + step, U)
                chunk, lo = frame_table.pad_chunk(track, a, b, q)          # whole GEMM row tiles
                f, self.last_pointnet_saves = F_hip.encoder_frame_features(self.encoder, chunk)
                feats.append(f[lo:lo + b - a])
            return feats
        return self._score_track(F, hop, drop_last_aligned, dedup_points, track.device, features)

    def _score_track(self, F, hop, drop_last_aligned, dedup_points, dev, features):
        """a track of F frames -> the triple of its windows; ``features(U)``: the chunks of the feature table of its first
        U frames, the frames any window uses"""
        T, hop = constants.NSTEPS, int(hop)
        plan = frame_table.plan_track_windows([F], T, hop, drop_last_aligned, allow_empty=True)
        W, self.last_frames_encoded = plan.counts[0], plan.U
        if W == 0:
            if dedup_points:
                self.last_rows_encoded = 0
            return _empty_triple(self.encoder.MLP_sup1[0].weight.shape[0], dev)
        table = frame_table.join_rows(features(plan.U))
        rows = ops.WindowRows(plan.starts, T, table.shape[0], device=dev,
                              dev=torch.arange(0, W * hop, hop, dtype=torch.int32, device=dev))
        return self._score_windows(table, rows, T)

    @torch.no_grad()
    def embed_raw_track(self, points: torch.Tensor, offsets: torch.Tensor, pick: torch.Tensor = None, seed: int = 0,
                        track_key: int = 0, hop: int = constants.CROP_STEP, drop_last_aligned: bool = True,
                        dedup_points: bool = False, keep_points=0, keep_rule: str = "first", augment=None):
        """``embed_track`` from the radar's detections: ``points`` [P,5] fp32 / fp64 and ``offsets`` int32 [F + 1] on the
        device (``datasets.pack_raw_frames``) -> one ``ops.frames_from_raw`` launch for the whole track (centred, not
        divided by std, as ``generate_splits`` prepares the crops) -> exactly ``embed_track`` on those frames.  ``pick``
        int32 [F, N]: host-drawn picks (``datasets.draw_picks``); None: drawn on the device, frame f under the key
        ``(track_key, f)`` and ``seed``.  ``raw_err`` (int32 [1], device) is set by a frame that could not be processed.
        ``dedup_points``: the padded frames are never written; every frame's DISTINCT picked detections go through the
        PointNet block once and are pooled with their multiplicities (``ops.frames_from_raw_unique``,
        ``functional.encoder_frame_features_ragged``): the same features up to fp32 summation order, from
        ``sum(min(card, N))`` rows instead of ``F * N``.  ``last_rows_encoded`` is the number of table rows it ran.
        ``keep_points`` / ``keep_rule`` / ``augment`` (``datasets.RawPrep``): the track as a sparser radar, a person at
        another azimuth, of another size or pace, or a noisier sensor would deliver it, by the same launch on both routes;
        the draws come from ``seed`` and the keys ``(track_key, f)``, those of ``augment`` with supplied ``pick`` too.  With
        ``keep_points`` and ``dedup_points`` the table holds at most ``F * min(k, N)`` rows (in whole GEMM tiles)."""
        enc = self.encoder
        N, C = enc.nmax_points, enc.pc_block.pointnet1.module[0].weight.shape[1]
        F = frame_table.check_raw(points, offsets, pick, N, "embed_raw_track")
        prep = RawPrep.of(keep_points, None, keep_rule, augment, "embed_raw_track")
        keys = frame_table.frame_keys(track_key, 0, F, points.device) if prep.needs_keys(pick) and F else None
        if not dedup_points:
            frames = frame_table.raw_frames(points, offsets, N, C, pick, seed, keys, self.raw_err, prep=prep)
            return self.embed_track(frames, hop, drop_last_aligned)
        step = max(self.batch_size * constants.NSTEPS, 1)

        def features(U):
            return self._chunk_features(((a, min(a + step, U)) for a in range(0, U, step)), lambda a, b: _ragged_features(
                enc, points, offsets, N, C, pick, seed, keys, self.raw_err, a, b, prep=prep))
        return self._score_track(F, hop, drop_last_aligned, True, points.device, features)

    def _enrol(self, triple, ident, windows, who):
        if self.gallery is None:
            raise RuntimeError(f"OpenSetScorer.{who}: the scorer was built without a gallery")
        return self.gallery.enrol(triple[1].contiguous(), ident, windows)

    def enrol_track(self, track: torch.Tensor, ident=None, windows=None, **how):
        """``embed_track(track, **how)``, then ``gallery.enrol`` of its windows (``windows``: which, host ints in the
        order they are added; None: all) -> the identity"""
        return self._enrol(self.embed_track(track, **how), ident, windows, "enrol_track")

    def enrol_raw_track(self, points: torch.Tensor, offsets: torch.Tensor, ident=None, windows=None, **how):
        """``embed_raw_track(points, offsets, **how)``, then ``gallery.enrol`` of its windows -> the identity"""
        return self._enrol(self.embed_raw_track(points, offsets, **how), ident, windows, "enrol_raw_track")

    def fit_threshold(self, known_lik: torch.Tensor, unseen_valid_lik: torch.Tensor) -> float:
        """ROC-optimal (Youden J) separation of known-test vs held-out-unseen likelihoods
        (inference_PCAA.py:225-231: unseen first with label 0, known with label 1)."""
        scores = np.concatenate([unseen_valid_lik.cpu().numpy(), known_lik.cpu().numpy()])
        labels = np.concatenate([np.zeros(unseen_valid_lik.numel()), np.ones(known_lik.numel())])
        self.threshold = youden_threshold(labels, scores)
        return self.threshold

    def vote(self, lik: torch.Tensor, preds: torch.Tensor, k: int, n_labels: int) -> torch.Tensor:
        if self.threshold is None:
            raise RuntimeError("fit_threshold() first")
        return self._rule.vote(lik, preds, self.threshold, k, n_labels)


def _variation_uses_head(variation, model_name=""):
    """Projection head on the encoder for variants 1, 2 and 4 (inference_PCAA.py:75-84); ``variation`` may be
    the reference's VARIATION enum, its name ("V1"...), True/False, or be inferred from the model name's
    ``...V4`` suffix (:402-414)."""
    if variation is True:
        return True
    name = getattr(variation, "name", variation) if variation else model_name.split(".")[0][-2:]
    return str(name).upper() in ("V1", "V2", "V4")


def CGAAE_inference_setup(model_name, loaders_batch_size=1, variation=False, generate_dataset=True,
                          force_pc_subsampling=0, device=None):
    """Load ``models/<name>/config.pkl``, ``<name>_E.pt`` and ``discriminator_means.pt``
    (checkpoint format of the reference) -> (encoder.eval(), means on the device); with
    ``generate_dataset`` the splits are regenerated from the raw tracks first for the model's
    TRAIN_CLASSES / NMAX (inference_PCAA.py:66-72)."""
    folder = os.path.join("models", model_name)
    with open(os.path.join(folder, "config.pkl"), "rb") as f:
        config = pickle.load(f)
    if generate_dataset:
        from .datasets import generate_splits
        generate_splits(train_classes=config["TRAIN_CLASSES"], seed=0, force_pc_subsampling=force_pc_subsampling,
                        nmax_points=config["NMAX"], verbose=False)
    dev = torch.device(device or constants.DEVICE)
    enc = CGEncoder(n_out_labels=len(config["TRAIN_CLASSES"]),
                    use_projection_head=_variation_uses_head(variation, model_name),
                    nmax_points=config["NMAX"]).to(dev).float()
    enc.load_state_dict(torch.load(os.path.join(folder, f"{model_name}_E.pt"), map_location=dev))
    means = torch.load(os.path.join(folder, "discriminator_means.pt"), map_location=dev)
    return enc.eval(), means


def naive_sequential_procedure(k, encoder, discriminator_means, *args, **kwargs):
    """Two call forms.

    The REFERENCE's (inference_PCAA.py:117-125), taken when the fourth argument is a path:
    ``naive_sequential_procedure(k, encoder, discriminator_means, figures_folder, model_folder,
    scenarios_list=constants.TRAIN_SCENARIOS, seed=0, unseen_valid_ratio=0.2, force_pc_subsampling=0)``
    (and the opt-in ``dedup_frames`` / ``dedup_points`` of ``OpenSetScorer.embed``)
    -> ``(out_log, final_preds, final_labels)``: the sequentially ordered TEST / UNSEEN splits are read from the generated
    dataset (packed once into an HBM-resident store), the procedure runs on the device, and ``naive_seq_log_{k}*.json`` is
    written into ``model_folder`` under the reference's three file names.  Not reproduced: the confusion-matrix PNG in
    ``figures_folder`` (plotting is out of scope; the folder is only created).

    The in-memory form the drivers and tests use: ``naive_sequential_procedure_tensors`` below (crops already on the device)
    -> ``(final_preds, final_labels, threshold)``."""
    if args and isinstance(args[0], (str, os.PathLike)) or "figures_folder" in kwargs:
        return _naive_sequential_procedure_files(k, encoder, discriminator_means, *args, **kwargs)
    return naive_sequential_procedure_tensors(k, encoder, discriminator_means, *args, **kwargs)


def _metrics(k, preds, labels):
    """the ``naive_seq_log_{k}*.json`` record: accuracy and F1 micro / macro / weighted of the open-set votes"""
    from sklearn.metrics import f1_score
    return {"n_steps": k, "accuracy": float(np.equal(labels, preds).sum() / max(len(labels), 1)),
            "f1_micro": float(f1_score(labels, preds, average="micro")),
            "f1_macro": float(f1_score(labels, preds, average="macro")),
            "f1_weighted": float(f1_score(labels, preds, average="weighted"))}


def _file_suffix(force_pc_subsampling, scenarios_list):
    """what the reference appends to its output file names: ``_subsampled{n}`` or ``_scenarios...`` when ONE of the two
    differs from its default, nothing when neither does; None when both do (the reference has no name for that)"""
    default_scen = list(scenarios_list) == list(constants.TRAIN_SCENARIOS)
    if force_pc_subsampling and not default_scen:
        return None
    if force_pc_subsampling:
        return f"_subsampled{force_pc_subsampling}"
    return "" if default_scen else "_scenarios" + "_".join(sc.value for sc in scenarios_list)


def _naive_sequential_procedure_files(k, encoder, discriminator_means, figures_folder, model_folder,
                                      scenarios_list=None, seed=0, unseen_valid_ratio=0.2, force_pc_subsampling=0,
                                      dedup_frames=False, dedup_points=False):
    import json
    from .constants import SPLIT
    scenarios_list = constants.TRAIN_SCENARIOS if scenarios_list is None else scenarios_list
    dev = next(encoder.parameters()).device
    os.makedirs(figures_folder, exist_ok=True)
    known_pcs, known_labels = _sequential_split_on_device(SPLIT.TEST, scenarios_list, dev)
    unseen_pcs, unseen_labels = _sequential_split_on_device(SPLIT.UNSEEN, scenarios_list, dev)
    preds, labels, _ = naive_sequential_procedure_tensors(k, encoder, discriminator_means, known_pcs, known_labels, unseen_pcs,
                                                          unseen_labels, seed=seed, unseen_valid_ratio=unseen_valid_ratio,
                                                          dedup_frames=dedup_frames, dedup_points=dedup_points)
    labels = labels.astype(int)
    out_log = _metrics(k, preds, labels)
    name = f"naive_seq_log_{k}{_file_suffix(force_pc_subsampling, scenarios_list) or ''}.json"    # both given: the plain name
    with open(os.path.join(model_folder, name), "w") as f:
        json.dump(out_log, f)
    return out_log, preds, labels


def naive_sequential_procedure_tensors(k, encoder, discriminator_means, known_pcs, known_labels, unseen_pcs,
                                       unseen_labels, seed=0, unseen_valid_ratio=0.2, batch_size=1024,
                                       dedup_frames=False, dedup_points=False):
    """The reference's procedure on in-memory, temporally ordered crops: (1) likelihoods of
    known-test and unseen crops, 20 % of the unseen SUBJECTS (rng seed 0) held out to pick the
    threshold; (2) k-window votes on the known test set and on the remaining unseen subjects.
    Returns (open-set predictions, open-set labels, threshold).  ``dedup_frames``: frames that
    consecutive crops share are encoded once; ``dedup_points``: the points that padding repeated
    inside a frame are encoded once (both: ``OpenSetScorer.embed``)."""
    scorer = OpenSetScorer(encoder, discriminator_means, batch_size)
    k_preds, _, k_lik = scorer.embed(known_pcs, dedup_frames=dedup_frames, dedup_points=dedup_points)
    u_preds, _, u_lik = scorer.embed(unseen_pcs, dedup_frames=dedup_frames, dedup_points=dedup_points)
    return _sequential_votes(k, scorer, (k_preds, k_lik), known_labels, (u_preds, u_lik), unseen_labels, seed,
                             unseen_valid_ratio)


def _sequential_votes(k, scorer, known, known_labels, unseen, unseen_labels, seed=0, unseen_valid_ratio=0.2,
                      threshold=None):
    """steps (1) and (2) of the procedure on crops that are embedded already: ``known`` / ``unseen`` = (preds,
    likelihood) of the sequential TEST / UNSEEN crops -> (open-set predictions, open-set labels, threshold).  The
    threshold is refit from these likelihoods; one embedding serves every k (``point_sweep``).  ``threshold``: used as it
    is instead (a deployed threshold; ``perturbation_sweep``): nothing is fitted, the validation subjects are held out
    all the same."""
    (k_preds, k_lik), (u_preds, u_lik) = known, unseen
    n_labels = int(len(np.unique(known_labels.cpu().numpy())))
    u_lab = unseen_labels.cpu().numpy()
    val_subjects = _validation_subjects(u_lab, np.random.default_rng(seed), unseen_valid_ratio)
    vm = torch.from_numpy(np.isin(u_lab, val_subjects)).to(u_lik.device)
    if threshold is None:
        thr = scorer.fit_threshold(k_lik, u_lik[vm])
    else:
        thr = scorer.threshold = float(threshold)
    preds, labels = [], []
    for lik, pr, lab, unknown in ((k_lik, k_preds, known_labels, False), (u_lik, u_preds, unseen_labels, True)):
        voted, truth = _voted_windows(
            k, lab.cpu().numpy(), lambda n: scorer.vote(lik[:n].contiguous(), pr[:n].contiguous(), k, n_labels),
            val_subjects, unknown, (lambda s: n_labels) if unknown else (lambda s: s))
        preds += voted
        labels += truth
    return np.asarray(preds), np.asarray(labels), thr


def _validation_subjects(u_lab, rng, ratio):
    """the unseen subjects held out to choose the threshold: ``ceil(ratio * n)`` of them, the FIRST draw of ``rng``"""
    subjects = np.unique(u_lab)
    return rng.choice(subjects, size=int(np.ceil(ratio * len(subjects))), replace=False)


def _voted_windows(k, lab, vote, val_subjects, unknown, label_of):
    """The window loop of the sequential procedure over one split.  ``lab``: the subject of every crop, in order (numpy);
    ``vote(n)``: the votes of the ``n // k`` groups of its first n crops, on the device; ``label_of(subject)``: the
    open-set label of a group.  Windows are cut over the WHOLE sequential set, as the reference's DataLoader(batch_size=k)
    does -> (votes, labels) of the windows that count, as lists."""
    n = (len(lab) // k) * k
    votes = vote(n).cpu().numpy()
    preds, labels = [], []
    for w in range(n // k):
        seg = lab[w * k:(w + 1) * k]
        if len(np.unique(seg)) != 1:
            continue                           # windows straddling two subjects are skipped (:243-245)
        if unknown and seg[0] in val_subjects:
            continue                           # validation subjects only chose the threshold (:286)
        preds.append(int(votes[w]))
        labels.append(label_of(int(seg[0])))
    return preds, labels


def _sequential_split_on_device(split, scenarios_list, device):
    """A split's crops in the sequential order of ``MSRadarDataset(sequential=True)`` as device tensors
    ([M,C,T,N] view of the packed point-major store, labels [M])."""
    from .batcher import PackedCrops, pack_split
    from .datasets import MSRadarDataset
    ds = MSRadarDataset(split, scenarios=scenarios_list, sequential=True)
    cache = str(ds.dataset_dir).rstrip("/") + "_packed_seq"
    pack_split(ds, cache)
    crops, labels = PackedCrops(cache).to_device(device)
    return crops.permute(0, 3, 1, 2), labels


def _sequential_split_from_store(store, split, scenarios_list, N, seed=0, **how):
    """The same tensors from a ``datasets.RawTrackStore`` (already assigned and on the device): the split's crops in
    sequential order, written out by one ``pcaa_crops_from_raw`` launch under the fixed draws of ``seed``; no files.
    ``how``: ``prep=`` (or the keywords it is built from) of ``RawCrops.materialize``: the frames thinned and moved by the
    same launch; ``seed``: of the picks and of those draws alike."""
    return store.crops(split, N=N, C=constants.NFEATURES, order="sequential", scenarios=scenarios_list).materialize(
        seed=seed, **how)


def _sweep_scorer(encoder, means, store, who):
    """the scorer of a sweep over ``store``, refused before anything is built when the store is not on the device"""
    if store.device is None:
        raise RuntimeError(f"{who}: call store.to_device() first; there is no CPU path")
    return OpenSetScorer(encoder, means)


def _embed_splits(scorer, store, scenarios_list, N, seed, prep, dedup_points):
    """What every sweep does per point: the sequential TEST and UNSEEN crops of ``store`` (a ``datasets.RawTrackStore``
    with its splits assigned, on the device) built under ``seed`` and ``prep``, embedded ONCE each with
    ``dedup_frames=True``, the crops freed before the next split -> per split (preds, sup_fv, likelihood, labels)."""
    from .constants import SPLIT
    scenarios_list = constants.TRAIN_SCENARIOS if scenarios_list is None else scenarios_list
    out = []
    for split in (SPLIT.TEST, SPLIT.UNSEEN):
        pcs, labels = _sequential_split_from_store(store, split, scenarios_list, N, seed, prep=prep)
        out.append(scorer.embed(pcs, dedup_frames=True, dedup_points=dedup_points) + (labels,))
        del pcs
    return out


def _vote_sets(emb):
    """``_embed_splits``' result as the four arguments ``_sequential_votes`` takes after the scorer"""
    return [x for preds, _, lik, labels in emb for x in ((preds, lik), labels)]


def point_sweep(encoder, means, store, keeps, ks, N, scenarios_list=None, dedup_points=True, keep_rule="first"):
    """The paper's robustness curve -- open-set accuracy against the detections a frame keeps -- from one resident store:
    ``store`` a ``datasets.RawTrackStore`` with its splits assigned, on the device -> ``{keep: {k: metrics}}``, ``metrics``
    the record ``CGAAE_inference`` writes as ``naive_seq_log_{k}_subsampled{keep}.json`` (accuracy, F1 micro / macro /
    weighted of the votes over k windows).  Per ``keep`` (k points, ``(lo, hi)``, or 0 for the frames as they are) the
    sequential TEST / UNSEEN crops are built thinned on the device (seed 0) and embedded ONCE -- every frame that
    consecutive crops share once, and with ``dedup_points`` (default) its distinct points only, so a sweep point costs
    PointNet rows proportional to ``min(keep, N)`` -- then the threshold is refit and the votes are taken for every k of
    ``ks``.  Writes no file."""
    scorer = _sweep_scorer(encoder, means, store, "point_sweep")
    out = {}
    for keep in keeps:
        sets = _vote_sets(_embed_splits(scorer, store, scenarios_list, N, 0, RawPrep.of(keep, None, keep_rule, who="point_sweep"),
                                        dedup_points))
        out[keep] = {}
        for k in ks:
            preds, labels, _ = _sequential_votes(k, scorer, *sets)
            out[keep][k] = _metrics(k, preds, labels.astype(int))
    return out


def perturbation_sweep(encoder, means, store, augments, ks, N, seed=0, refit=False, scenarios_list=None,
                       dedup_points=True):
    """The sibling of ``point_sweep`` for the ways a deployed radar degrades or differs other than by losing points:
    position and Doppler noise, people at other azimuths, of other sizes and paces.  ``augments``: a dict from a name to an
    augment (``datasets.augment_arguments``: yaw, mirror, scale, speed, noise; None or ``{}``: the crops as they are) ->
    ``{name: {k: metrics}}``, ``metrics`` as in ``point_sweep``.  Per entry the sequential TEST / UNSEEN crops are built
    augmented on the device under ``seed`` (one ``pcaa_crops_from_raw_aug`` launch per split) and embedded ONCE with
    ``dedup_frames=True`` (and ``dedup_points``, default).  ``refit=False``: the votes use the threshold fitted on the
    UN-augmented crops (built and embedded once, first) -- a deployed threshold meeting a degraded sensor; ``refit=True``:
    the threshold is refit on each entry's own likelihoods, as ``point_sweep`` does per ``keep``.  Writes no file."""
    scorer = _sweep_scorer(encoder, means, store, "perturbation_sweep")

    def embedded(augment):
        return _vote_sets(_embed_splits(scorer, store, scenarios_list, N, seed,
                                        RawPrep.of(augment=augment, who="perturbation_sweep"), dedup_points))

    # the threshold does not depend on k: one fit on the crops as they are (same seed: the same picks)
    clean = None if refit else _sequential_votes(ks[0], scorer, *embedded(None))[2]
    out = {}
    for name, augment in augments.items():
        sets = embedded(augment)
        out[name] = {}
        for k in ks:
            preds, labels, _ = _sequential_votes(k, scorer, *sets, threshold=clean)
            out[name][k] = _metrics(k, preds, labels.astype(int))
    return out


def plan_enrolment(unseen_labels, shots, seed=0, unseen_valid_ratio=0.2, enrol_ratio=0.5):
    """Host plan of one ``enrolment_sweep`` point, numpy only.  ``unseen_labels``: the subject of every sequential UNSEEN
    crop.  The validation subjects are the draw ``_sequential_votes`` makes (``_validation_subjects``: same generator, first
    draw); of the others ``ceil(enrol_ratio * n)`` are drawn next and numbered 0, 1, ... in ascending subject order.
    A drawn subject is enrolled from its first ``shots`` crops when it has more than ``shots`` of them (something must be
    left to evaluate) and ``shots > 0``.  -> (val_subjects, {subject: identity} of the enrolled, {subject: its enrolment
    rows}, keep mask over the crops: False on the enrolment rows)."""
    u_lab = np.asarray(unseen_labels)
    rng = np.random.default_rng(seed)
    subjects = np.unique(u_lab)
    val_subjects = _validation_subjects(u_lab, rng, unseen_valid_ratio)
    rest = subjects[~np.isin(subjects, val_subjects)]
    if not 0.0 <= enrol_ratio <= 1.0 or int(shots) < 0:
        raise ValueError("plan_enrolment: needs 0 <= enrol_ratio <= 1 and shots >= 0")
    drawn = np.sort(rng.choice(rest, size=int(np.ceil(enrol_ratio * len(rest))), replace=False)) if len(rest) else rest
    idents, rows, keep = {}, {}, np.ones(len(u_lab), bool)
    for s in drawn:
        at = np.flatnonzero(u_lab == s)
        if 0 < int(shots) < at.size:
            idents[int(s)] = len(idents)
            rows[int(s)] = at[:int(shots)]
            keep[at[:int(shots)]] = False
    return val_subjects, idents, rows, keep


def enrolment_sweep(encoder, means, store, shots, ks, N, enrol_ratio=0.5, seed=0, scenarios_list=None, dedup_points=True,
                    unseen_valid_ratio=0.2):
    """Open-set accuracy against the windows a new person is enrolled from, the sibling of ``point_sweep``: ``store`` a
    ``datasets.RawTrackStore`` with its splits assigned, on the device -> ``{shots: {k: metrics}}``, ``metrics`` what
    ``_metrics`` returns.  The sequential TEST / UNSEEN crops are built and embedded ONCE, as ``point_sweep`` does for
    ``keep = 0``.  The threshold is fitted first, with an empty gallery, as ``_sequential_votes`` fits it; the held-out
    validation subjects are never enrolled.  Per entry of ``shots`` a fresh ``gallery.Gallery`` enrols the subjects
    ``plan_enrolment`` draws under ``seed`` from their first ``shots`` windows; those windows are left out of the
    evaluation, every other window is scored against prior and gallery (``ops.gallery_score``), and the votes over k
    windows (``ops.gallery_vote``) carry ``n_labels + 1 + identity`` for an enrolled subject and ``n_labels`` for every
    other unseen one.  With nobody enrolled an entry is ``point_sweep``'s record for ``keep = 0``.  Writes no file."""
    from .gallery import Gallery
    scorer = _sweep_scorer(encoder, means, store, "enrolment_sweep")
    (k_preds, k_fv, k_lik, k_lab), (u_preds, u_fv, u_lik, u_lab) = (
        (preds, fv.contiguous(), lik, labels.cpu().numpy()) for preds, fv, lik, labels in _embed_splits(
            scorer, store, scenarios_list, N, 0, RawPrep.of(0, None, "first", who="enrolment_sweep"), dedup_points))
    n_labels = int(len(np.unique(k_lab)))
    dev = k_fv.device
    out = {}
    for n_shots in shots:
        val_subjects, idents, rows, keep = plan_enrolment(u_lab, n_shots, seed, unseen_valid_ratio, enrol_ratio)
        thr = scorer.fit_threshold(k_lik, u_lik[torch.from_numpy(np.isin(u_lab, val_subjects)).to(dev)])
        gal = Gallery(k_fv.shape[1], max(len(idents), 1), dev)
        for s, ident in idents.items():                                   # (ascending subjects: identity = slot)
            gal.enrol(u_fv, ident, rows[s])
        kept = torch.from_numpy(np.flatnonzero(keep)).to(dev)
        sets = ((k_preds, k_fv, k_lab, False), (u_preds[kept], u_fv[kept].contiguous(), u_lab[keep], True))
        scored = [gal.score(fv, pr.contiguous(), scorer.means, n_labels)[:2] + (lab, unknown) for pr, fv, lab, unknown in sets]
        out[n_shots] = {}
        for k in ks:
            preds, labels = [], []
            for lik, ext, lab, unknown in scored:
                voted, truth = _voted_windows(
                    k, lab, lambda n: ops.gallery_vote(lik[:n].contiguous(), ext[:n].contiguous(), thr, k, n_labels),
                    val_subjects, unknown,
                    (lambda s: n_labels + 1 + idents[s] if s in idents else n_labels) if unknown else (lambda s: s))
                preds += voted
                labels += truth
            out[n_shots][k] = _metrics(k, np.asarray(preds), np.asarray(labels).astype(int))
    return out


def CGAAE_inference(model_names, ks, force_pc_subsampling=0, scenarios_list=None, variation=False,
                    generate_dataset=True, device=None, dedup_frames=False, dedup_points=False, raw_store=None,
                    keep_points=0, keep_rule="first"):
    """Open-set evaluation driver with the reference's call surface and output files
    (inference_PCAA.py:382-469): for every model and k, the naive sequential procedure on the sequentially
    ordered test / unseen splits; writes ``naive_seq_log_{k}*.json`` (accuracy, F1 micro / macro / weighted),
    ``final_preds_{k}*.npy`` / ``final_labels_{k}*.npy`` and ``naive_seq_log_subsampled{n}.json`` under
    ``models/<name>/``.  Not reproduced: the confusion-matrix PNG (plotting).  The splits are regenerated once per
    call (the reference regenerates them for every (model, k) with identical arguments).  ``dedup_frames`` (opt-in):
    every frame that consecutive crops of the sequential splits share is encoded once.  ``dedup_points`` (opt-in): every
    point that the stored crops' padding repeats inside a frame is encoded once (it pays most with
    ``force_pc_subsampling``, which pads from fewer points).  ``raw_store`` (a ``datasets.RawTrackStore`` of the raw
    tracks): nothing is generated or read from crop files -- per model the store's tracks are assigned as
    ``generate_splits(TRAIN_CLASSES, seed=0)`` assigns them and the sequential TEST / UNSEEN crops are built on the device
    at the model's NMAX (device draws of seed 0; ``force_pc_subsampling`` is a property of generated files and is refused).
    ``keep_points=k`` (with ``raw_store``; ``keep_rule`` "first" / "random") is the sweep over detections per frame
    without crop files: the crops are built thinned to at most k detections a frame on the device, the threshold is refit
    as the reference's rerun refits it, and the files carry the reference's ``_subsampled{k}`` names.  ``point_sweep``
    returns the whole curve and writes nothing."""
    import json
    from .constants import SPLIT
    scenarios_list = constants.TRAIN_SCENARIOS if scenarios_list is None else scenarios_list
    if keep_points:
        if raw_store is None:
            raise ValueError("CGAAE_inference: keep_points thins raw detections on the device and needs raw_store; crop "
                             "files are thinned when they are generated (force_pc_subsampling)")
        if isinstance(keep_points, (tuple, list)) or isinstance(keep_points, bool) or int(keep_points) != keep_points:
            raise ValueError("CGAAE_inference: keep_points is one count k (the files are named _subsampled{k}); "
                             "point_sweep takes ranges")
        if force_pc_subsampling:
            raise ValueError("CGAAE_inference: keep_points and force_pc_subsampling are the same sweep on two routes; give one")
        keep_points = int(keep_points)
    prep = RawPrep.of(keep_points, None, keep_rule, who="CGAAE_inference") if raw_store is not None else None
    subsampled = keep_points or force_pc_subsampling
    suffix = _file_suffix(subsampled, scenarios_list)
    if suffix is None:
        raise ValueError("force_pc_subsampling / keep_points and scenarios_list cannot be both different from default")
    if raw_store is not None and force_pc_subsampling:
        raise ValueError("CGAAE_inference: force_pc_subsampling needs generated crop files; it cannot be combined with raw_store")
    dev = torch.device(device or constants.DEVICE)
    out_log = {}
    generated = not generate_dataset
    for model_name in model_names:
        folder = os.path.join("models", model_name)
        os.makedirs(os.path.join("figures", model_name), exist_ok=True)
        enc, means = CGAAE_inference_setup(model_name, 32, variation,
                                           generate_dataset=not generated and raw_store is None,
                                           force_pc_subsampling=force_pc_subsampling, device=dev)
        generated = True
        if raw_store is not None:
            with open(os.path.join(folder, "config.pkl"), "rb") as f:
                config = pickle.load(f)
            raw_store.assign_like_generate_splits(config["TRAIN_CLASSES"], seed=0).to_device(dev)
            known_pcs, known_labels = _sequential_split_from_store(raw_store, SPLIT.TEST, scenarios_list, config["NMAX"],
                                                                   prep=prep)
            unseen_pcs, unseen_labels = _sequential_split_from_store(raw_store, SPLIT.UNSEEN, scenarios_list, config["NMAX"],
                                                                     prep=prep)
        else:
            known_pcs, known_labels = _sequential_split_on_device(SPLIT.TEST, scenarios_list, dev)
            unseen_pcs, unseen_labels = _sequential_split_on_device(SPLIT.UNSEEN, scenarios_list, dev)
        for k in ks:
            preds, labels, thr = naive_sequential_procedure(k, enc, means, known_pcs, known_labels, unseen_pcs,
                                                            unseen_labels, seed=0, unseen_valid_ratio=0.2,
                                                            dedup_frames=dedup_frames, dedup_points=dedup_points)
            labels = labels.astype(int)
            metrics = _metrics(k, preds, labels)
            with open(os.path.join(folder, f"naive_seq_log_{k}{suffix}.json"), "w") as f:
                json.dump(metrics, f)
            np.save(os.path.join(folder, f"final_preds_{k}{suffix}.npy"), preds)
            np.save(os.path.join(folder, f"final_labels_{k}{suffix}.npy"), labels)
            out_log[k] = {m: metrics[m] for m in ("f1_micro", "f1_macro", "f1_weighted")}
        with open(os.path.join(folder, f"naive_seq_log_subsampled{subsampled}.json"), "w") as f:
            json.dump(out_log, f)
    return out_log


class _LiveScorer:
    """What the two live scorers are built from: the window rule's arguments checked, the ring sized
    (``ring_rows >= NSTEPS + max_push``), the centroids on the encoder's device, the encoder's widths."""

    def __init__(self, encoder, means, threshold, k, n_labels, hop, max_push, ring_rows, gallery):
        self.encoder = encoder
        self._check_eval()
        who = type(self).__name__
        self.T, self.hop, self.k, self.n_labels = constants.NSTEPS, int(hop), int(k), int(n_labels)
        self.threshold, self.max_push = float(threshold), int(max_push)
        if not 1 <= self.hop <= self.T or self.max_push < 1 or self.k < 1:
            raise ValueError(f"{who}: needs 1 <= hop <= NSTEPS, max_push >= 1, k >= 1")
        need = self.T + self.max_push
        self.ring_rows = need if ring_rows is None else int(ring_rows)
        if self.ring_rows < need:
            raise ValueError(f"{who}: ring_rows={self.ring_rows} < NSTEPS + max_push = {need}")
        self.means = means.float().to(next(encoder.parameters()).device).contiguous()
        self.n_classes = encoder.MLP_sup2[0].weight.shape[0]
        self._D = encoder.MLP_sup1[0].weight.shape[0]                          # embedding width
        # run-time enrolment: with a gallery windows are scored against it too and carry extended labels (OpenSetScorer)
        self._rule = _Rule(self.means, n_labels, self.n_classes, gallery, who)
        self.gallery = gallery
        self._width = encoder.tc_block.layers()[0].conv1d.weight.shape[1]      # frame-feature width: a ring row
        self._N, self._C = encoder.nmax_points, encoder.pc_block.pointnet1.module[0].weight.shape[1]   # a raw frame becomes [N, C]
        self.last_pointnet_saves = None

    def _set_keep(self, keep_points, keep_rule):
        """``push_raw`` scores the stream as a sparser radar would deliver it: every frame keeps at most ``keep_points``
        detections under ``keep_rule`` before it is padded to N (``datasets.RawPrep``, built here once)"""
        self.prep = RawPrep.of(keep_points, None, keep_rule, who=type(self).__name__)    # refused here, not at the first push
        self.keep_points, self.keep_rule = keep_points, keep_rule

    def _check_eval(self):
        if self.encoder.training:
            raise RuntimeError(f"{type(self).__name__}: the encoder is in training mode (train-mode BatchNorm mixes the "
                               "frames of a batch: a frame's features would depend on its neighbours); call encoder.eval()")


class StreamingScorer(_LiveScorer):
    """Open-set scoring of a live track: frames arrive a few at a time, a decision is due every ``hop`` frames.

    A device ring keeps the PointNet features of the last ``ring_rows >= NSTEPS + max_push`` frames.  ``push`` encodes the
    new frames once, writes them into the ring (a push that wraps is two writes) and runs the temporal block, in its
    windowed form over the ring, for every window whose last frame has now arrived: window j (frames ``j*hop .. j*hop +
    NSTEPS - 1``) is returned by the very push that brings the track to ``NSTEPS + j*hop`` frames.  Windows are emitted
    EAGERLY: for a track of F frames ``OpenSetScorer.embed_track`` under the reference's cropping rule holds one window
    fewer when ``(F - NSTEPS) % hop == 0`` (``window_count``); the first ``window_count(F)`` windows are the same.
    ``votes()`` is ``k_vote`` over the completed groups of k windows so far, ``reset()`` starts a new track.  The
    precision mode (``functional.get_precision()``) is read at every push, as ``OpenSetScorer.embed`` does.

    One object serves ONE track, and it keeps the predictions and likelihoods of every past window (``votes()`` recomputes
    all groups), so its memory grows for as long as the track lives.  ``MultiStreamScorer`` scores many concurrent tracks
    in one batched tick with O(k) state per track."""

    def __init__(self, encoder: CGEncoder, means: torch.Tensor, threshold: float, k: int, n_labels: int,
                 hop: int = constants.CROP_STEP, max_push: int = 64, ring_rows: int = None, seed: int = 0,
                 dedup_points: bool = False, keep_points=0, keep_rule: str = "first", gallery=None):
        super().__init__(encoder, means, threshold, k, n_labels, hop, max_push, ring_rows, gallery)
        dev = self.means.device
        self.ring = torch.zeros((self.ring_rows, self._width), dtype=torch.float32, device=dev)
        self.dedup_points = bool(dedup_points)           # push_raw: distinct points once, pooled with their multiplicities
        self._set_keep(keep_points, keep_rule)           # push_raw: every frame thinned first
        self.seed, self.serial = int(seed), -1           # push_raw: frame f of the track is drawn under (serial, f)
        self.raw_err = torch.zeros(1, dtype=torch.int32, device=dev)     # set by a raw frame that could not be processed
        # window j starts at ring row (j * hop) % ring_rows, a sequence of period ring_rows / gcd: kept on the device
        # once, long enough that the windows of any one push are a contiguous slice of it (no upload per push)
        self._period = self.ring_rows // np.gcd(self.ring_rows, self.hop)
        self._max_win = frame_table.eager_window_count(self.T + self.max_push, self.T, self.hop)    # of one push
        self._starts = (np.arange(self._period + self._max_win, dtype=np.int64) * self.hop) % self.ring_rows
        self._starts_dev = torch.from_numpy(self._starts.astype(np.int32)).to(dev)
        self.reset()

    def reset(self):
        """forget the track: the next pushed frame is frame 0 of a new one (with a new serial: ``push_raw`` does not
        replay the previous track's draws)"""
        self.serial += 1
        self.n_frames = 0
        self.n_windows = 0
        self._preds, self._lik = [], []

    @torch.no_grad()
    def push(self, frames: torch.Tensor):
        """frames [n,N,C] fp32 on the device, the next n frames of the track -> (preds, sup_fv, likelihood) of the windows
        they complete (possibly none: empty tensors).  No ``dedup_points`` here: the host would have to read the number
        of distinct rows back before it launches the GEMMs, and a live tick must not wait for the device;
        ``push_raw`` with the constructor's ``dedup_points`` is the live route (its table is sized from the offsets)."""
        self._check_eval()
        frame_table.check_frames(frames, "StreamingScorer.push")
        return self._gather([self._push(frames[a:a + self.max_push]) for a in range(0, frames.shape[0], self.max_push)])

    def _gather(self, out):
        """the triples of a push's chunks (None: no window) -> one triple"""
        out = [o for o in out if o is not None]
        if not out:
            return _empty_triple(self._D, self.ring.device)
        if len(out) == 1:
            return out[0]
        return tuple(torch.cat([o[i] for o in out]) for i in range(3))

    @torch.no_grad()
    def push_raw(self, points: torch.Tensor, offsets: torch.Tensor, pick: torch.Tensor = None):
        """``push`` from the radar's detections: ``points`` [P,5] fp32 / fp64, ``offsets`` int32 [n + 1] on the device
        (``datasets.pack_raw_frames``), the next n frames of the track -> one ``ops.frames_from_raw`` launch per
        ``max_push`` frames (centred, padded to whole GEMM tiles by the same launch), then what ``push`` does.  ``pick``
        int32 [n, N]: host-drawn picks; None: drawn on the device, frame f of the track under the key ``(serial, f)`` and
        the constructor's ``seed``.  ``raw_err`` is set by a frame that could not be processed (its frame is zeros).
        With the constructor's ``dedup_points`` the padded frames are never written: ``ops.frames_from_raw_unique`` and
        ``functional.encoder_frame_features_ragged`` give the same frame features from the frames' distinct points.
        The constructor's ``keep_points`` / ``keep_rule`` thin every frame first (device-drawn picks only)."""
        self._check_eval()
        n = frame_table.check_raw(points, offsets, pick, self._N, "StreamingScorer.push_raw")
        q = F_hip.frame_pad_quantum(self._N)
        keys = frame_table.frame_keys(self.serial, self.n_frames, n, points.device) if pick is None and n else None
        raw = (points, offsets, self._N, self._C, pick, self.seed, keys, self.raw_err)
        out = []
        for a in range(0, n, self.max_push):
            b = min(a + self.max_push, n)
            if self.dedup_points:
                feats, self.last_pointnet_saves, _ = _ragged_features(self.encoder, *raw, a, b, prep=self.prep)
                out.append(self._push_features(feats, b - a))
            else:
                out.append(self._push_padded(frame_table.raw_frames(*raw, a, b, n_out=b - a + (a - b) % q, prep=self.prep),
                                             b - a))
        return self._gather(out)

    def _push(self, frames):
        n, q = frames.shape[0], F_hip.frame_pad_quantum(frames.shape[1])
        if n % q:                  # whole GEMM row tiles in bf16 mode; a push has no neighbours: zeros, features dropped
            frames = frame_table.pad_chunk(frames, 0, n, q)[0]
        return self._push_padded(frames, n)

    def _push_padded(self, frames, n):
        """``frames``: on the device, padded to whole tiles, the first ``n`` of them the track's next frames"""
        feats, self.last_pointnet_saves = F_hip.encoder_frame_features(self.encoder, frames)
        return self._push_features(feats, n)

    def _push_features(self, feats, n):
        """``feats``: the frame features of the track's next ``n`` frames in its first rows"""
        pos = self.n_frames % self.ring_rows
        first = min(n, self.ring_rows - pos)
        self.ring[pos:pos + first].copy_(feats[:first])
        if first < n:                               # the push wraps: second write from row 0
            self.ring[:n - first].copy_(feats[first:n])
        self.n_frames += n
        done = frame_table.eager_window_count(self.n_frames, self.T, self.hop)
        j0, nw = self.n_windows, done - self.n_windows
        if nw == 0:
            return None
        o = j0 % self._period
        plan = ops.WindowRows(self._starts[o:o + nw], self.T, self.ring_rows, self.ring_rows, dev=self._starts_dev[o:o + nw])
        logits, sup_fv, _ = F_hip.encoder_forward_windows(self.encoder, self.ring, plan, self.T)
        _, _, preds = ops.cross_entropy(logits, None, want_loss=False, want_preds=True)
        preds, lik = self._rule.score(sup_fv.contiguous(), preds)
        self.n_windows = done
        self._preds.append(preds)
        self._lik.append(lik)
        return preds, sup_fv, lik

    def votes(self) -> torch.Tensor:
        """``k_vote`` over the completed groups of k windows emitted since the last ``reset()`` -> [n_windows // k] int64"""
        if not self._preds:
            return torch.empty(0, dtype=torch.int64, device=self.ring.device)
        preds, lik = torch.cat(self._preds), torch.cat(self._lik)
        self._preds, self._lik = [preds], [lik]
        n = (preds.numel() // self.k) * self.k
        return self._rule.vote(lik[:n].contiguous(), preds[:n].contiguous(), self.threshold, self.k, self.n_labels)


class TickPlan:
    """What ``plan_tick`` returns: see there."""
    __slots__ = ("dst_row", "win_row", "win_stream", "win_j", "vote_pos", "run_start", "vote_stream", "vote_group",
                 "n_frames", "n_windows", "packed", "offsets", "frame_key")


def plan_tick(n_frames, n_windows, sids, counts, T, hop, k, ring_rows, pad_to=1, serials=None):
    """Host plan of one tick of ``MultiStreamScorer``: a pure function of the streams' counters, numpy only.

    ``n_frames`` / ``n_windows``: per SLOT, the frames pushed and the windows emitted so far; ``sids``: the distinct slots
    this tick feeds, ``counts[i]`` new frames of ``sids[i]`` (0 allowed), the frames concatenated in that order.  Slot s
    owns rows ``s * ring_rows .. (s + 1) * ring_rows - 1`` of the feature table, frame f of its track lives in row
    ``s * ring_rows + f % ring_rows``; a stream with n frames has ``frame_table.eager_window_count(n, T, hop)`` windows, window j
    starts at frame ``j * hop``; group ``j // k`` is voted on by the window with ``j % k == k - 1``.  Returns a TickPlan:

    * ``dst_row`` int32 [P]: the table row of every frame; P = the frames padded up to a multiple of ``pad_to``, the
      padding rows marked -1 (skip);
    * ``win_row`` / ``win_stream`` / ``win_j`` int32 [nw]: start row (absolute), slot and index within its stream of every
      window the tick completes, ordered by the position of the stream in ``sids``, ascending within a stream;
    * ``vote_pos`` int32 [nw]: where the group a window completes goes in the tick's votes, -1 if it completes none;
      ``vote_stream`` / ``vote_group`` int64 [g]: slot and group index of every vote;
    * ``run_start`` int32 [runs + 1]: the windows of one stream are ``run_start[r] .. run_start[r + 1]``;
    * ``n_frames`` / ``n_windows`` int64 [len(sids)]: the counters of ``sids`` after the tick;
    * ``packed`` int32: all six int32 arrays in one buffer (one upload), ``offsets[name] = (start, stop)`` in it.

    ``serials`` (optional, per SLOT: the serial number of the track in it): the plan also carries ``frame_key`` int32
    [frames, 2], the key ``(serial of its track, its index in its track)`` of every frame of the tick (no padding rows) --
    what ``MultiStreamScorer.push_raw`` draws a frame's points under -- appended to ``packed`` as
    ``offsets["frame_key"]`` (flattened); without ``serials`` it is None and ``packed`` is as before."""
    T, hop, k, ring_rows, pad_to = int(T), int(hop), int(k), int(ring_rows), int(pad_to)
    n_frames = np.asarray(n_frames, dtype=np.int64).reshape(-1)
    n_windows = np.asarray(n_windows, dtype=np.int64).reshape(-1)
    sids = np.asarray(sids, dtype=np.int64).reshape(-1)
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    n_slots, S = n_frames.size, sids.size
    if not 1 <= hop <= T or k < 1 or pad_to < 1 or ring_rows < T or n_slots != n_windows.size:
        raise ValueError("plan_tick: needs 1 <= hop <= T <= ring_rows, k >= 1, pad_to >= 1, one counter pair per slot")
    if S != counts.size:
        raise ValueError(f"plan_tick: {S} streams but {counts.size} counts")
    if n_slots * ring_rows >= 2 ** 31:
        raise ValueError("plan_tick: the table rows do not fit 32-bit indices")
    plan = TickPlan()
    plan.frame_key = None
    if serials is not None:
        serials = np.asarray(serials, dtype=np.int64).reshape(-1)
        if serials.size != n_slots:
            raise ValueError("plan_tick: one serial per slot")
        plan.frame_key = np.zeros((0, 2), np.int32)
    if S == 0:
        z = np.zeros(0, np.int64)
        nf1 = done = nwin = win_stream = j = z
        dst_row, complete, total, nw = np.zeros(0, np.int32), np.zeros(0, bool), 0, 0
    else:
        if sids.min() < 0 or sids.max() >= n_slots:
            raise ValueError(f"plan_tick: a stream id outside 0..{n_slots - 1}")
        seen = np.zeros(n_slots, bool)
        seen[sids] = True
        if np.count_nonzero(seen) != S:
            raise ValueError("plan_tick: a stream id appears twice in one tick")
        if counts.min() < 0 or counts.max() + T > ring_rows:
            raise ValueError(f"plan_tick: counts must lie in 0..ring_rows - T = {ring_rows - T} (a larger push would "
                             "overwrite frames its own windows still read)")
        nf0, w0 = n_frames[sids], n_windows[sids]
        nf1 = nf0 + counts
        done = frame_table.eager_window_count(nf1, T, hop)
        nwin = done - w0
        if nwin.min() < 0:
            raise ValueError("plan_tick: a stream has emitted more windows than its frames hold")
        if done.max() >= 2 ** 31:
            raise ValueError("plan_tick: a window index does not fit 32 bits")
        total, nw = int(counts.sum()), int(nwin.sum())
        # frame f of the tick: f - (frames of the streams before its own) + (frames its stream had) = its index in its track
        base = sids * ring_rows
        dst = np.arange(total, dtype=np.int64) + np.repeat(nf0 - (np.cumsum(counts) - counts), counts)
        if serials is not None:                                # here dst is still the frame's index in its track
            plan.frame_key = np.stack([np.repeat(serials[sids], counts), dst], axis=1).astype(np.int32)
        dst %= ring_rows
        dst += np.repeat(base, counts)
        pad = (-total) % pad_to
        dst_row = dst.astype(np.int32) if not pad else np.concatenate([dst, np.full(pad, -1, np.int64)]).astype(np.int32)
        wstart = np.cumsum(nwin) - nwin
        j = np.arange(nw, dtype=np.int64) + np.repeat(w0 - wstart, nwin)
        win_stream = np.repeat(sids, nwin)
        complete = j % k == k - 1
    plan.dst_row = dst_row
    plan.win_row = (win_stream * ring_rows + (j * hop) % ring_rows).astype(np.int32)
    plan.win_stream, plan.win_j = win_stream.astype(np.int32), j.astype(np.int32)
    plan.vote_pos = np.where(complete, np.cumsum(complete) - 1, -1).astype(np.int32)
    plan.vote_stream, plan.vote_group = win_stream[complete], j[complete] // k
    plan.run_start = np.append(wstart[nwin > 0], nw).astype(np.int32) if S else np.zeros(1, np.int32)
    plan.n_frames, plan.n_windows = nf1, done
    parts = (plan.dst_row, plan.win_row, plan.win_stream, plan.win_j, plan.vote_pos, plan.run_start)
    plan.offsets, a = {}, 0
    for name, arr in zip(("dst_row", "win_row", "win_stream", "win_j", "vote_pos", "run_start"), parts):
        plan.offsets[name] = (a, a + arr.size)
        a += arr.size
    if plan.frame_key is not None:
        parts += (plan.frame_key.reshape(-1),)
        plan.offsets["frame_key"] = (a, a + plan.frame_key.size)
    plan.packed = np.concatenate(parts)
    return plan


class Tick:
    """The result of one ``MultiStreamScorer.push``.  ``stream`` / ``window`` int64 [nw] and ``vote_stream`` /
    ``vote_group`` int64 [g]: host numpy arrays (known from the plan: no device sync); ``preds`` int64 [nw], ``sup_fv``
    fp32 [nw, 32], ``lik`` f64 [nw], ``votes`` int64 [g]: device tensors.  Windows are ordered by the position of their
    stream in ``sids``, ascending within a stream.  From a scorer with a gallery ``preds`` holds the extended labels
    (``n_labels + 1 + identity`` where an enrolled person's mode is the nearest) and ``lik`` counts the enrolled modes."""
    __slots__ = ("stream", "window", "vote_stream", "vote_group", "preds", "sup_fv", "lik", "votes")

    def __len__(self):
        return self.stream.size


def _tick(plan, preds, sup_fv, lik, votes):
    """a Tick: which windows and votes they are from the plan, what they scored from the device"""
    t = Tick()
    t.stream, t.window = plan.win_stream.astype(np.int64), plan.win_j.astype(np.int64)
    t.vote_stream, t.vote_group = plan.vote_stream, plan.vote_group
    t.preds, t.sup_fv, t.lik, t.votes = preds, sup_fv, lik, votes
    return t


def _host_ints(x):
    """a 1-D sequence of host ints -> int64 array; None for anything else"""
    try:
        arr = np.asarray(x)
    except (TypeError, ValueError):
        return None
    if arr.ndim != 1 or (arr.size and arr.dtype.kind not in "iu"):
        return None
    return arr.astype(np.int64)


class MultiStreamScorer(_LiveScorer):
    """Open-set scoring of up to ``max_streams`` live tracks in one batched tick.

    Every slot owns a ring of ``ring_rows >= NSTEPS + max_push`` rows in one ``[max_streams * ring_rows, 1024]`` feature
    table.  ``push(sids, counts, frames)`` takes the new frames of any subset of the open slots (ragged) and runs ONE eval
    PointNet pass over all of them, ONE scatter into the rings, ONE temporal block + heads pass over every window the tick
    completes (the segmented windowed form of the first temporal layer) and ONE scoring launch (argmax, likelihood, vote
    state, votes): the number of launches does not depend on the number of streams.  The window rule is
    ``StreamingScorer``'s (eager: window j comes back from the tick that brings its stream to ``NSTEPS + j * hop`` frames).
    ``push`` synchronises nothing and copies nothing to the host; the tick's plan (``plan_tick``) goes up as one pinned
    buffer.  The encoder's eval constants (``functional.encoder_eval_constants``) are folded once and rebuilt when a
    parameter, a buffer or the precision mode changes.  Per-stream state is O(k): the incomplete vote group.
    ``gallery`` (a ``gallery.Gallery``): the identities enrolled at run time are scored beside the prior's modes by the
    same single launch (``ops.stream_score_gallery``); ``history=H`` keeps every stream's last H embeddings on the device
    for ``enrol_stream``.  Without a gallery the tick is the one described above, launch for launch."""

    def __init__(self, encoder: CGEncoder, means: torch.Tensor, threshold: float, k: int, n_labels: int,
                 max_streams: int = 64, hop: int = constants.CROP_STEP, max_push: int = 64, ring_rows: int = None,
                 batch_size: int = 1024, seed: int = 0, dedup_points: bool = False, keep_points=0,
                 keep_rule: str = "first", gallery=None, history: int = 0):
        super().__init__(encoder, means, threshold, k, n_labels, hop, max_push, ring_rows, gallery)
        # run-time enrolment: the tick's scoring launch is ops.stream_score_gallery; ``history`` = H > 0 also keeps every
        # stream's last H embeddings on the device (fv_hist), from which ``enrol_stream`` enrols
        self.history = int(history)
        if self.history < 0 or (self.history and self.gallery is None):
            raise ValueError("MultiStreamScorer: history must be >= 0, and a history needs a gallery to enrol into")
        self.max_streams, self.batch_size = int(max_streams), int(batch_size)
        self.dedup_points = bool(dedup_points)           # push_raw: distinct points once, pooled with their multiplicities
        self._set_keep(keep_points, keep_rule)           # push_raw: every frame thinned first
        if self.max_streams < 1 or self.batch_size < 1:
            raise ValueError("MultiStreamScorer: needs max_streams >= 1, batch_size >= 1")
        dev = self.means.device
        if dev.type != "cuda":
            raise RuntimeError("MultiStreamScorer: the encoder must live on the HIP device; this package has no CPU path")
        self.ring = torch.zeros((self.max_streams * self.ring_rows, self._width), dtype=torch.float32, device=dev)
        self.hist_lik = torch.zeros((self.max_streams, self.k), dtype=torch.float64, device=dev)
        self.hist_pred = torch.zeros((self.max_streams, self.k), dtype=torch.int64, device=dev)
        self.fv_hist = (torch.zeros((self.max_streams * self.history, self._D), dtype=torch.float32, device=dev)
                        if self.history else None)
        self.scatter_err = torch.zeros(1, dtype=torch.int32, device=dev)     # set by a scatter destination out of range
        self.raw_err = torch.zeros(1, dtype=torch.int32, device=dev)         # set by a raw frame that could not be processed
        self.seed = int(seed)                                  # push_raw draws frame f of a track under (its serial, f)
        self.track_serial = np.zeros(self.max_streams, np.int64)             # per slot: bumped by open()
        self._next_serial = 0
        self.n_frames = np.zeros(self.max_streams, np.int64)
        self.n_windows = np.zeros(self.max_streams, np.int64)
        self._open = np.zeros(self.max_streams, bool)
        self._consts = None
        self._zeros = None

    def open(self) -> int:
        """-> the lowest free slot; its frame and window counters start at 0 (its ring rows are not cleared: a window only
        reads rows written since)"""
        free = np.flatnonzero(~self._open)
        if free.size == 0:
            raise ValueError(f"MultiStreamScorer.open: all {self.max_streams} slots are in use")
        sid = int(free[0])
        self._open[sid] = True
        self.n_frames[sid] = self.n_windows[sid] = 0
        self.track_serial[sid] = self._next_serial             # a reused slot does not replay its previous track's draws
        self._next_serial += 1
        return sid

    def close(self, sid: int):
        """end the track in slot ``sid``; the slot may be handed out again"""
        self._slots([sid], "close")
        self._open[int(sid)] = False

    def enrol_stream(self, sid: int, windows: int, ident=None) -> int:
        """Enrol the person in slot ``sid`` from the last ``windows <= min(history, windows so far)`` windows of the
        stream, oldest first -> the identity (``ident=None``: the lowest free one; a live one is refined).  The rows of
        ``fv_hist`` come from the host's own window counter and go up with the launch: nothing is read back and nothing
        waits for the device.  Labels already stored in the vote history stay as they are."""
        from .gallery import ring_rows
        if not self.history:
            raise RuntimeError("MultiStreamScorer.enrol_stream: built with history=0; there is nothing to enrol from")
        sid = int(self._slots([sid], "enrol_stream")[0])
        return self.gallery.enrol(self.fv_hist, ident, ring_rows(self.n_windows[sid], self.history, windows, sid))

    def _slots(self, sids, what):
        arr = _host_ints(sids)
        if arr is None:
            raise ValueError(f"MultiStreamScorer.{what}: stream ids must be a 1-D sequence of host ints")
        if arr.size and (arr.min() < 0 or arr.max() >= self.max_streams or not self._open[arr].all()):
            raise ValueError(f"MultiStreamScorer.{what}: unknown or closed stream id in {arr.tolist()}")
        return arr

    def _empty(self, plan, dev):
        return _tick(plan, *_empty_triple(self._D, dev), torch.empty(0, dtype=torch.int64, device=dev))

    @torch.no_grad()
    def push(self, sids, counts, frames: torch.Tensor) -> Tick:
        """``sids``: distinct open slots (host ints); ``counts[i]`` new frames of ``sids[i]`` (0 allowed, at most
        ``max_push``); ``frames`` [sum(counts), N, C] fp32 on the device, concatenated in that order -> the Tick of the
        windows these frames complete (possibly none: empty tensors, no temporal pass).  No ``dedup_points`` here: the
        host would have to read the number of distinct rows back before it launches the GEMMs, and a live tick must not
        wait for the device; ``push_raw`` with the constructor's ``dedup_points`` is the live route."""
        self._check_eval()
        frame_table.check_frames(frames, "MultiStreamScorer.push")
        n, N, C = frames.shape
        sids, plan, part, mode = self._begin_tick(sids, counts, n, N, "push", False)
        if n == 0:
            return self._empty(plan, self.ring.device)
        pad = plan.dst_row.size - n
        if pad:                                       # whole GEMM row tiles in bf16 mode, once per TICK; features dropped
            if self._zeros is None or tuple(self._zeros.shape[1:]) != (N, C) or self._zeros.shape[0] < pad:
                self._zeros = frames.new_zeros((max(pad, F_hip.frame_pad_quantum(N, mode)), N, C))
            frames = torch.cat([frames, self._zeros[:pad]])
        return self._finish_tick(sids, plan, part, mode, frames)

    @torch.no_grad()
    def push_raw(self, sids, counts, points: torch.Tensor, offsets: torch.Tensor, pick: torch.Tensor = None) -> Tick:
        """``push`` from the radar's detections: ``points`` [P,5] fp32 / fp64 and ``offsets`` int32 [sum(counts) + 1] on
        the device (``datasets.pack_raw_frames`` of the tick's frames, concatenated in the order of ``sids``) -> the same
        Tick, by ONE launch more than ``push`` (``ops.frames_from_raw``: the frames centred as ``process_track`` centres
        them and padded to whole GEMM tiles) and no host work per frame.  ``pick`` int32 [sum(counts), N]: host-drawn picks
        (``datasets.draw_picks``: the reference's draws); None: drawn on the device, frame f of a track under the key
        ``(track_serial[slot], f)`` and the constructor's ``seed`` -- the keys travel in the tick's one pinned upload.
        ``raw_err`` is set by a frame that could not be processed (it is encoded as zeros).
        With the constructor's ``dedup_points`` the padded frames are never written: the tick's distinct points go through
        the PointNet block once (``ops.frames_from_raw_unique``, ``functional.encoder_frame_features_ragged``: three
        launches in place of one, still none per stream) and give the same frame features up to fp32 summation order.
        The constructor's ``keep_points`` / ``keep_rule`` thin every frame first (device-drawn picks only): the same
        launches, fewer table rows."""
        self._check_eval()
        n = frame_table.check_raw(points, offsets, pick, self._N, "MultiStreamScorer.push_raw")
        sids, plan, part, mode = self._begin_tick(sids, counts, n, self._N, "push_raw", pick is None,
                                                  pad_to=1 if self.dedup_points else None)
        if n == 0:
            return self._empty(plan, self.ring.device)
        raw = (points, offsets, self._N, self._C, pick, self.seed, part["frame_key"].view(n, 2) if pick is None else None,
               self.raw_err)
        if self.dedup_points:
            feats, self.last_pointnet_saves, _ = _ragged_features(self.encoder, *raw, mode=mode, consts=self._consts,
                                                                  prep=self.prep)
            return self._finish_tick_features(sids, plan, part, mode, feats)
        return self._finish_tick(sids, plan, part, mode, frame_table.raw_frames(*raw, n_out=plan.dst_row.size, prep=self.prep))

    def _begin_tick(self, sids, counts, n, N, what, want_keys, pad_to=None):
        """the arguments of a tick checked, its plan made and (unless the tick is empty) uploaded -> (sids, plan, the
        plan's parts on the device, precision mode).  ``pad_to``: frames of the tick's PointNet pass are padded to a
        multiple of it (default: ``frame_pad_quantum``)."""
        sids = self._slots(sids, what)
        counts = _host_ints(counts)
        if counts is None or counts.size != sids.size:
            raise ValueError(f"MultiStreamScorer.{what}: counts must be host ints, one per stream id")
        if counts.size and (counts.min() < 0 or counts.max() > self.max_push):
            raise ValueError(f"MultiStreamScorer.{what}: counts must lie in 0..max_push = {self.max_push}")
        if int(counts.sum()) != n:
            raise ValueError(f"MultiStreamScorer.{what}: counts add up to {int(counts.sum())} frames, got {n}")
        dev = self.ring.device
        mode = F_hip.get_precision()
        q = F_hip.frame_pad_quantum(N, mode) if pad_to is None else pad_to
        plan = plan_tick(self.n_frames, self.n_windows, sids, counts, self.T, self.hop, self.k, self.ring_rows, q,
                         serials=self.track_serial if want_keys else None)
        if n == 0:
            return sids, plan, None, mode
        if self._consts is None or not self._consts.valid_for(self.encoder, mode):
            self._consts = F_hip.encoder_eval_constants(self.encoder, mode)
        # the whole plan in one pinned buffer, one asynchronous copy (the pinned block is recycled by torch's host
        # allocator only after the copy has run)
        host = torch.empty(plan.packed.size, dtype=torch.int32, pin_memory=True)
        host.numpy()[:] = plan.packed
        packed = host.to(dev, non_blocking=True)
        return sids, plan, {name: packed[a:b] for name, (a, b) in plan.offsets.items()}, mode

    def _finish_tick(self, sids, plan, part, mode, frames):
        """a tick from the point where its frames are on the device and padded to whole tiles"""
        feats, self.last_pointnet_saves = F_hip.encoder_frame_features(self.encoder, frames, mode, consts=self._consts)
        return self._finish_tick_features(sids, plan, part, mode, feats)

    def _finish_tick_features(self, sids, plan, part, mode, feats):
        """a tick from the point where its frames' features are on the device, one row per entry of the plan's dst_row"""
        dev = self.ring.device
        ops.scatter_rows(feats, part["dst_row"], self.ring, err_flag=self.scatter_err)
        self.n_frames[sids], self.n_windows[sids] = plan.n_frames, plan.n_windows
        nw = plan.win_row.size
        if nw == 0:
            return self._empty(plan, dev)
        rows = ops.WindowRows(plan.win_row, self.T, self.ring.shape[0], self.ring_rows, dev=part["win_row"],
                              segments=self.max_streams)
        out = [F_hip.encoder_forward_windows(self.encoder, self.ring, rows.slice(i, i + self.batch_size) if
                                             nw > self.batch_size else rows, self.T, mode, consts=self._consts)[:2]
               for i in range(0, nw, self.batch_size)]
        logits, sup_fv = (frame_table.join_rows(part).contiguous() for part in zip(*out))
        return _tick(plan, *self._rule.tick(logits, sup_fv, part, plan.vote_group.size, self.threshold, self.k, self.hist_lik,
                                            self.hist_pred, self.fv_hist))
