"""Run-time enrolment: identities that did not come from training, kept as modes beside the prior's.

The critic shapes ``sup_fv`` so that a trained class sits as ``N(mu_c, I)`` around its prior mean and an unknown person
falls between the modes.  A person seen for a few windows therefore gets a mode of their own -- the centroid of their
own embeddings under the same unit covariance -- and the rule that recognises the trained classes recognises them, with
no weight touched (kernels: ``csrc/gallery.hip``).

A ``Gallery`` is three device buffers (``sums`` fp64 and ``centroids`` fp32 ``[max_identities, D]``, ``counts`` int32
``[max_identities]``) and the host's bookkeeping of which slots are in use.  Slot e is identity e; the scorers report it
as label ``n_labels + 1 + e`` (``n_labels`` itself stays "unknown").  Every refusal is decided on the host from the
host's own records: nothing is read back from the device.
"""
import numpy as np
import torch

from . import ops


class Gallery:
    def __init__(self, D: int, max_identities: int, device):
        self.D, self.max_identities = int(D), int(max_identities)
        if self.D < 1 or self.max_identities < 1:
            raise ValueError("Gallery: needs D >= 1 and max_identities >= 1")
        self.device = torch.device(device)
        self.sums = torch.zeros((self.max_identities, self.D), dtype=torch.float64, device=self.device)
        self.counts = torch.zeros(self.max_identities, dtype=torch.int32, device=self.device)
        self.centroids = torch.zeros((self.max_identities, self.D), dtype=torch.float32, device=self.device)
        self.err = torch.zeros(1, dtype=torch.int32, device=self.device)    # set by an enrolment row out of range
        self._live = np.zeros(self.max_identities, bool)
        self.high_water = 0                                                 # the kernels scan slots 0 .. high_water - 1

    # ------------------------------------------------------------------ host bookkeeping (no device access)
    def _slot_for(self, ident, who):
        """the slot an enrolment goes to: the lowest free one, or ``ident`` itself (live: refined; free: taken)"""
        if ident is None:
            free = np.flatnonzero(~self._live)
            if free.size == 0:
                raise ValueError(f"Gallery.{who}: all {self.max_identities} identities are in use")
            return int(free[0])
        if isinstance(ident, bool) or not isinstance(ident, (int, np.integer)) or not 0 <= int(ident) < self.max_identities:
            raise ValueError(f"Gallery.{who}: identity must be an int in 0..{self.max_identities - 1}, got {ident!r}")
        return int(ident)

    def _took(self, slot):
        self._live[slot] = True
        self.high_water = max(self.high_water, slot + 1)

    def identities(self):
        """the live identities, ascending"""
        return [int(e) for e in np.flatnonzero(self._live)]

    def __len__(self):
        return int(self._live.sum())

    def __contains__(self, ident):
        return (not isinstance(ident, bool) and isinstance(ident, (int, np.integer))
                and 0 <= int(ident) < self.max_identities and bool(self._live[int(ident)]))

    def label_of(self, ident, n_labels):
        """the label the scorers give identity ``ident``: ``n_labels + 1 + ident``"""
        if ident not in self:
            raise ValueError(f"Gallery.label_of: unknown identity {ident!r}")
        return int(n_labels) + 1 + int(ident)

    def ident_of(self, label, n_labels):
        """the identity behind an extended label; None for a trained class or "unknown" (``label <= n_labels``)"""
        label, n_labels = int(label), int(n_labels)
        if label <= n_labels:
            return None
        ident = label - n_labels - 1
        if ident not in self:
            raise ValueError(f"Gallery.ident_of: label {label} names no live identity")
        return ident

    # ------------------------------------------------------------------ device side
    def enrol(self, sup_fv, ident=None, rows=None):
        """Add embeddings to an identity -> its id.  ``sup_fv`` fp32 [n, D] on the device; ``rows``: which of them, in
        this order (host ints or an int32 device tensor; None: all).  ``ident=None`` takes the lowest free slot; a live
        ``ident`` is refined (the running fp64 sum continues), a free one is taken.  One launch, nothing read back; a
        row index outside ``[0, n)`` is skipped on the device and sets ``err``."""
        slot = self._slot_for(ident, "enrol")
        if not isinstance(sup_fv, torch.Tensor) or sup_fv.dim() != 2 or sup_fv.shape[1] != self.D:
            raise ValueError(f"Gallery.enrol: needs embeddings [n, {self.D}], got "
                             f"{tuple(sup_fv.shape) if isinstance(sup_fv, torch.Tensor) else type(sup_fv)}")
        if rows is not None and not isinstance(rows, torch.Tensor):
            arr = np.asarray(rows)
            if arr.ndim != 1 or (arr.size and arr.dtype.kind not in "iu"):
                raise ValueError("Gallery.enrol: rows must be a 1-D sequence of ints or an int32 device tensor")
            if arr.size and (arr.min() < -2 ** 31 or arr.max() >= 2 ** 31):
                raise ValueError("Gallery.enrol: rows do not fit 32-bit indices")
            # one pinned buffer, one asynchronous copy (as MultiStreamScorer uploads a tick's plan): no wait for the device
            host = torch.empty(arr.size, dtype=torch.int32, pin_memory=self.device.type == "cuda")
            host.numpy()[:] = arr
            rows = host.to(self.device, non_blocking=True)
        m = sup_fv.shape[0] if rows is None else rows.numel()
        if m < 1:
            raise ValueError("Gallery.enrol: no rows to enrol")
        ops.gallery_accumulate(sup_fv, slot, self.sums, self.counts, self.centroids, rows, self.err)
        self._took(slot)
        return slot

    def remove(self, ident):
        """forget an identity: its count and sums are zeroed, the slot is free again"""
        if ident not in self:
            raise ValueError(f"Gallery.remove: unknown identity {ident!r}")
        e = int(ident)
        self.counts[e:e + 1].zero_()
        self.sums[e].zero_()
        self.centroids[e].zero_()
        self._live[e] = False

    def score(self, sup_fv, preds, means, n_labels):
        """``ops.gallery_score`` against this gallery -> (lik, labels, near)"""
        return ops.gallery_score(sup_fv, preds, means, self.centroids, self.counts, self.high_water, n_labels)

    def state_dict(self):
        return {"D": self.D, "max_identities": self.max_identities, "sums": self.sums.clone(), "counts": self.counts.clone(),
                "centroids": self.centroids.clone(), "live": self._live.copy(), "high_water": self.high_water}

    def load_state_dict(self, state):
        if int(state["D"]) != self.D or int(state["max_identities"]) != self.max_identities:
            raise ValueError(f"Gallery.load_state_dict: a gallery of [{state['max_identities']}, {state['D']}] does not fit "
                             f"one of [{self.max_identities}, {self.D}]")
        live = np.asarray(state["live"], bool)
        hw = int(state["high_water"])
        if live.shape != self._live.shape or not 0 <= hw <= self.max_identities or (
                live.any() and np.flatnonzero(live).max() >= hw):
            raise ValueError("Gallery.load_state_dict: inconsistent bookkeeping")
        for name in ("sums", "counts", "centroids"):
            src, dst = state[name], getattr(self, name)
            if tuple(src.shape) != tuple(dst.shape) or src.dtype != dst.dtype:
                raise ValueError(f"Gallery.load_state_dict: {name} must be {dst.dtype} {tuple(dst.shape)}")
        for name in ("sums", "counts", "centroids"):
            getattr(self, name).copy_(state[name])
        self._live, self.high_water = live.copy(), hw


def ring_rows(n_windows, H, m, stream=0):
    """The rows of ``fv_hist`` ([max_streams * H, D], window j of stream s in row ``s * H + j % H``) that hold the last ``m``
    windows of a stream that has emitted ``n_windows``, oldest first -> int32 [m].  A pure function of the host's window
    counter: an enrolment uploads it and never reads the device."""
    n_windows, H, m, stream = int(n_windows), int(H), int(m), int(stream)
    if H < 1 or not 1 <= m <= min(H, n_windows) or stream < 0:
        raise ValueError(f"ring_rows: needs 1 <= m <= min(H, windows so far) = {min(H, n_windows)}, got m = {m}")
    j = np.arange(n_windows - m, n_windows, dtype=np.int64)
    rows = stream * H + j % H
    if rows.size and rows.max() >= 2 ** 31:
        raise ValueError("ring_rows: the rows do not fit 32-bit indices")
    return rows.astype(np.int32)
