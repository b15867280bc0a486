"""The library calls of one step, in order: ``python tools/call_list.py fp32|bf16|fp16x3|train|eval|score|live|tracks``
prints, for every pcaa_* call, the entry point, its integer and float arguments and the ordinal (by first appearance) of the
stream it went to.  Pointers are not recorded, so two trees that launch the same work print the same list -- the check of
a refactor of the Python layer.  ``fp32`` / ``bf16`` / ``fp16x3``: one eager PCAATrainer step at B=4, N=32, C=4, K=4;
``eval``: one eval-mode encoder_forward(want_bwd=True) + encoder_backward(need_dx=True).

Between the calls stands the synchronisation skeleton, in program order and with the same stream ordinals:
``Stream.wait_stream`` / ``Stream.wait_event`` / ``Event.record`` / ``Tensor.record_stream`` (events by ordinal of first
appearance) and every collective (``all_reduce`` / ``all_gather_into_tensor`` / ``reduce_scatter_tensor`` of
torch.distributed and of an emulated exchange: element count, dtype, issuing stream) with the ``wait()`` of its work --
a dropped or moved wait is the difference a list of kernels alone cannot show.

``train``: every branch of ``PCAATrainer._step`` at the same shape (``train()``), each case under a ``--`` heading and
followed by the sha256 of the last step's losses and of ``flat_g.p`` / ``flat_d.p`` (two runs of one tree print the same
hashes; the one output that differed between two runs of a tree has a ``~out`` line).

``score`` / ``live`` / ``tracks``: the inference and track routes at N=32, C=4, K=4, in fp32 and then in bf16 mode, every
case under a ``--`` heading and followed by the sha256 of every tensor it returned (equal bits are part of the same diff;
gradients are not reproducible to the bit and get ``~out`` lines, see ``Recorder.case``).
``score``: ``OpenSetScorer.embed`` / ``embed_track`` / ``embed_raw_track`` at the track lengths where the window rule and
the padding of a chunk change branch; ``live``: ``StreamingScorer`` and ``MultiStreamScorer`` pushes, padded and raw;
``tracks``: ``cg_encoder_tracks`` / ``cg_encoder_raw_track`` forward and backward, ``adapt.finetune_frozen_bn_tracks``.
One process per list; no profiler."""
import ctypes
import hashlib
import os
import re
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opensetgaitrecognition_pcaa_amd import _lib, adapt, constants, datasets, functional as F, inference, models, ops  # noqa: E402
from opensetgaitrecognition_pcaa_amd import synthetic as syn  # noqa: E402
from opensetgaitrecognition_pcaa_amd.train import PCAATrainer  # noqa: E402
from oracle import pcaa_oracle as O  # noqa: E402

NUMBERS = (ctypes.c_int, ctypes.c_long, ctypes.c_size_t, ctypes.c_float, ctypes.c_double)
DEV = "cuda:0"
N, C, K, HOP = 32, 4, 4, 6


class Recorder:
    def __init__(self, lib):
        self.lib, self.calls, self.streams, self.exchanges = lib, [], {}, 0
        with open(_lib.HEADER) as f:           # the entry points whose last parameter is the stream
            self.streamed = set(re.findall(r"\b(pcaa_\w+)\s*\([^)]*\bstream\s*\)", f.read()))

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("pcaa_"):
            return fn

        def call(*args):
            nums = [a for a, t in zip(args, fn.argtypes) if t in NUMBERS]
            st = self.streams.setdefault(args[-1], len(self.streams)) if name in self.streamed else "-"
            self.calls.append(f"{name} {nums} stream {st}")
            return fn(*args)
        return call

    def stream(self, st=None):
        """the ordinal of a torch stream (default: the current one), shared with the library calls'"""
        return self.streams.setdefault(ops._s() if st is None else st.cuda_stream, len(self.streams))

    def hook_sync(self):
        """record the synchronisation skeleton from here on: wraps the Python-level stream / event / tensor methods and
        torch.distributed's collectives (an emulated exchange: ``hook_exchange``)"""
        import torch.distributed as dist
        events, nested = {}, []

        def ev(e):
            return events.setdefault(id(e), (len(events), e))[0]       # (the entry keeps the event, hence its id, alive)

        def wrap(cls, name, line):
            fn = getattr(cls, name)

            def method(obj, *a):
                if not nested:                 # torch implements wait_stream as record + wait_event: one line, not three
                    self.calls.append(line(obj, *a))
                nested.append(name)
                try:
                    return fn(obj, *a)
                finally:
                    nested.pop()
            setattr(cls, name, method)

        wrap(torch.cuda.Stream, "wait_stream", lambda s, o: f"Stream.wait_stream stream {self.stream(s)} for stream {self.stream(o)}")
        wrap(torch.cuda.Stream, "wait_event", lambda s, e: f"Stream.wait_event stream {self.stream(s)} event {ev(e)}")
        wrap(torch.cuda.Event, "record", lambda e, s=None: f"Event.record event {ev(e)} stream {self.stream(s)}")
        wrap(torch.Tensor, "record_stream", lambda t, s: f"Tensor.record_stream {t.numel()} {t.dtype} stream {self.stream(s)}")
        for name in ("all_reduce", "all_gather_into_tensor", "reduce_scatter_tensor"):
            setattr(dist, name, self._collective(name, getattr(dist, name)))

    def hook_exchange(self, xchg):
        """an emulated exchange issues no torch.distributed call: its two collectives are wrapped on the object"""
        if xchg is not None and xchg.emulated:
            for name in ("all_reduce", "all_gather_into_tensor"):
                setattr(xchg, name, self._collective(name, getattr(xchg, name)))

    def _collective(self, name, fn):
        rec = self

        class Work:
            def __init__(self, work, idx):
                self.work, self.idx = work, idx

            def wait(self, *a, **k):
                rec.calls.append(f"wait of exchange {self.idx} stream {rec.stream()}")
                return self.work.wait(*a, **k)

        def call(*a, **k):
            self.exchanges += 1
            tensors = [t for t in a if isinstance(t, torch.Tensor)]
            self.calls.append(f"{name} exchange {self.exchanges} {[t.numel() for t in tensors]} {tensors[0].dtype} "
                              f"async_op={bool(k.get('async_op', False))} stream {self.stream()}")
            work = fn(*a, **k)
            return None if work is None else Work(work, self.exchanges)
        return call

    def case(self, title, fn, exact=None, loose=()):
        """one case of the route modes: its heading, its calls, then the hashes of what it returned.  ``exact``: only the
        first so many outputs have reproducible bits; the others (weight gradients, which the GEMMs accumulate with
        floating-point atomics in an order that varies from run to run, and what is computed from them) get a ``~out``
        line with their norm instead -- ``grep -v '~out'`` leaves the part of a list that two runs must share.  ``loose``:
        single outputs, by index, that get a ``~out`` line"""
        self.calls.append(f"-- {title}")
        out = fn()
        for i, t in enumerate(out if isinstance(out, (tuple, list)) else (out,)):
            if isinstance(t, torch.Tensor):
                t = t.detach().cpu().numpy()
            arr = np.ascontiguousarray(t)
            if (exact is None or i < exact) and i not in loose:
                self.calls.append(f"   out[{i}] {arr.dtype} {list(arr.shape)} sha256 {hashlib.sha256(arr.tobytes()).hexdigest()}")
            else:
                self.calls.append(f"   ~out[{i}] {arr.dtype} {list(arr.shape)} l2 {np.linalg.norm(arr.astype(np.float64)):.6e}")


def _encoder():
    enc = models.CGEncoder(K, nmax_points=N, use_projection_head=True).float()
    syn.deterministic_fill_(enc, 0)
    return enc.to(DEV).eval()


def _track(n, seed):
    """a processed track [n, N, C] on the device whose frames carry padding: frame f repeats its first 1 + 3 * (f % 5)
    points at its end, bit for bit"""
    x = syn.synthetic_pcs(1, n, N, C, seed=seed)[0].clone()
    for f in range(n):
        r = 1 + 3 * (f % 5)
        x[f, N - r:] = x[f, :r]
    return x.contiguous().to(DEV)


def _raw(n, seed):
    """a raw track of n frames on the device -> (points, offsets, host-drawn picks)"""
    raw = syn.synthetic_raw_track(seed, n, max_points=40)
    points, offsets = datasets.pack_raw_frames(raw, torch.float32)
    np.random.seed(seed)
    pick = torch.from_numpy(datasets.draw_picks([len(fr["z_coord"]) for fr in raw], N))
    return points.to(DEV), offsets.to(DEV), pick.to(DEV)


def _flags(**kw):
    return " ".join(f"{k}={v}" for k, v in kw.items())


def score(rec, means):
    enc = _encoder()
    sc, sc1 = inference.OpenSetScorer(enc, means), inference.OpenSetScorer(enc, means, batch_size=1)
    T = constants.NSTEPS
    track = _track(61, 11)
    crops = torch.stack([track[j * HOP:j * HOP + T] for j in range(inference.window_count(61, T, HOP))]).permute(0, 3, 1, 2)
    for df in (False, True):
        for dp in (False, True):
            rec.case(f"embed {_flags(dedup_frames=df, dedup_points=dp)}",
                     lambda: sc.embed(crops, dedup_frames=df, hop=HOP, dedup_points=dp))
    for dp in (False, True):
        for n in (30, 31, 33, 36, 41, 61, 66):
            rec.case(f"embed_track F={n} {_flags(dedup_points=dp)}",
                     lambda: sc.embed_track(_track(n, n), HOP, dedup_points=dp))
        rec.case(f"embed_track F=61 batch_size=1 {_flags(dedup_points=dp)}",
                 lambda: sc1.embed_track(_track(61, 61), HOP, dedup_points=dp))
        for n in (30, 36, 66):
            rec.case(f"embed_track F={n} drop_last_aligned=False {_flags(dedup_points=dp)}",
                     lambda: sc.embed_track(_track(n, n), HOP, drop_last_aligned=False, dedup_points=dp))
        for who, s, n in (("", sc, 41), (" batch_size=1", sc1, 61)):
            points, offsets, pick = _raw(n, n)
            rec.case(f"embed_raw_track F={n}{who} host picks {_flags(dedup_points=dp)}",
                     lambda: s.embed_raw_track(points, offsets, pick, hop=HOP, dedup_points=dp))
            rec.case(f"embed_raw_track F={n}{who} device picks {_flags(dedup_points=dp)}",
                     lambda: s.embed_raw_track(points, offsets, None, seed=3, track_key=5, hop=HOP, dedup_points=dp))
    rec.case("raw_err", lambda: (sc.raw_err, sc1.raw_err))


def _tick_out(t):
    return t.stream, t.window, t.vote_stream, t.vote_group, t.preds, t.sup_fv, t.lik, t.votes


def live(rec, means):
    enc = _encoder()
    pushes = (7, 30, 5, 64, 70)
    total = 192                               # >= the frames of either sequence below
    track = _track(total, 21)
    points, offsets, pick = _raw(total, 22)
    off_host = offsets.cpu()

    def raw_slice(a, b, picks):
        p0, p1 = int(off_host[a]), int(off_host[b])
        return points[p0:p1].contiguous(), (offsets[a:b + 1] - p0).contiguous(), pick[a:b].contiguous() if picks else None

    def streaming(**kw):
        return inference.StreamingScorer(enc, means, 1e-30, 2, K, hop=HOP, max_push=64, seed=3, **kw)

    st, a = streaming(), 0
    for n in pushes:
        rec.case(f"StreamingScorer.push {n}", lambda: st.push(track[a:a + n]))
        a += n
    rec.case("StreamingScorer.votes", st.votes)
    for dp in (False, True):
        for picks in (True, False):
            st, a = streaming(dedup_points=dp), 0
            for n in pushes:
                rec.case(f"StreamingScorer.push_raw {n} {'host' if picks else 'device'} picks {_flags(dedup_points=dp)}",
                         lambda: st.push_raw(*raw_slice(a, a + n, picks)))
                a += n
            rec.case("StreamingScorer.votes, raw_err", lambda: (st.votes(), st.raw_err))

    ticks = (([0, 1, 2], [7, 30, 0]), ([0, 2], [30, 33]), ([], []), ([1, 0, 2], [5, 6, 12]), ([2, 1], [64, 1]))

    def multi(**kw):
        ms = inference.MultiStreamScorer(enc, means, 1e-30, 2, K, max_streams=3, hop=HOP, max_push=64, seed=3, **kw)
        for _ in range(3):
            ms.open()
        return ms

    ms, a = multi(), 0
    for sids, counts in ticks:
        n = sum(counts)
        rec.case(f"MultiStreamScorer.push {sids} {counts}", lambda: _tick_out(ms.push(sids, counts, track[a:a + n])))
        a += n
    rec.case("MultiStreamScorer.scatter_err", lambda: ms.scatter_err)
    for dp in (False, True):
        for picks in (True, False):
            ms, a = multi(dedup_points=dp), 0
            for sids, counts in ticks:
                n = sum(counts)
                rec.case(f"MultiStreamScorer.push_raw {sids} {counts} {'host' if picks else 'device'} picks "
                         f"{_flags(dedup_points=dp)}",
                         lambda: _tick_out(ms.push_raw(sids, counts, *raw_slice(a, a + n, picks))))
                a += n
            rec.case("MultiStreamScorer.scatter_err, raw_err", lambda: (ms.scatter_err, ms.raw_err))


def tracks(rec, means):
    lengths = (41, 61, 36)

    def walks():
        return [_track(n, 30 + n) for n in lengths]

    def backward(enc, out, extra=()):
        logits, fv = out
        r1 = syn.synthetic_pcs(1, 1, logits.shape[0], logits.shape[1], seed=41)[0, 0].to(DEV)
        r2 = syn.synthetic_pcs(1, 1, fv.shape[0], 1, seed=42)[0, 0].to(DEV)
        ((logits * r1).sum() + (fv * r2).sum()).backward()
        return [logits, fv] + [p.grad for p in enc.parameters()] + [t.grad for t in extra]

    for dp in (False, True):
        enc = _encoder()

        def forward():
            with torch.no_grad():
                return F.cg_encoder_tracks(enc, walks(), HOP, dedup_points=dp)
        rec.case(f"cg_encoder_tracks {list(lengths)} no_grad {_flags(dedup_points=dp)}", forward)
        rec.case(f"cg_encoder_tracks {list(lengths)} backward {_flags(dedup_points=dp)}",
                 lambda: backward(enc, F.cg_encoder_tracks(enc, walks(), HOP, dedup_points=dp)), exact=2)
    enc = _encoder()
    ws = walks()
    ws[1].requires_grad_(True)
    rec.case(f"cg_encoder_tracks {list(lengths)} backward, track 1 requires grad",
             lambda: backward(enc, F.cg_encoder_tracks(enc, ws, HOP), extra=(ws[1],)), exact=2)
    points, offsets, pick = _raw(41, 41)
    for dp in (False, True):
        for picks in (True, False):
            enc = _encoder()
            rec.case(f"cg_encoder_raw_track F=41 {'host' if picks else 'device'} picks backward {_flags(dedup_points=dp)}",
                     lambda: backward(enc, F.cg_encoder_raw_track(enc, points, offsets, pick if picks else None, seed=3,
                                                                  track_key=5, hop=HOP, dedup_points=dp)), exact=2)
    labels = syn.synthetic_labels(len(lengths), K, seed=43).to(DEV)
    for dp in (False, True):
        enc = _encoder()

        def finetune():
            losses = adapt.finetune_frozen_bn_tracks(enc, walks(), labels, 2, 1e-3, params="all", hop=HOP, dedup_points=dp)
            return [np.asarray(losses[:1], np.float64), np.asarray(losses[1:], np.float64)] + list(enc.parameters())
        rec.case(f"finetune_frozen_bn_tracks {list(lengths)} 2 steps params=all {_flags(dedup_points=dp)}", finetune, exact=1)


LOSSES = ("d_loss", "gp", "rec_loss", "loss_g", "sup_loss", "tot_loss")


def _train_inputs(n, seed=1):
    return (syn.synthetic_pcs(4, constants.NSTEPS, n, C, seed=seed).to(DEV).permute(0, 3, 1, 2),
            syn.synthetic_labels(4, K, seed=seed + 1).to(DEV), syn.synthetic_z0(4, 32, seed=seed + 2).to(DEV),
            syn.synthetic_alphas(4, seed=seed + 3).to(DEV))


def _train_case(rec, title, steps=(True,), n=N, precision="bf16", variant="v4", graphed=False, time_comm=False, loose=(), **kw):
    """``steps``: the ``supervise`` flag of each step of the case; ``loose``: see Recorder.case"""
    def run():
        cfg = dict(constants.CONFIG, NMAX=n, TRAIN_CLASSES=list(range(K)), BATCH_SIZE=4)
        tr = PCAATrainer(cfg, device=DEV, precision=precision, variant=variant, **kw)
        for i, m in enumerate(tr.modules().values()):
            syn.deterministic_fill_(m, 30 + i)
        if variant != "v1":
            tr.set_prior_means(O.sample_distant_points(32, K, 10, 10).float())
        tr.finalize()
        tr.train()
        tr.time_comm = time_comm
        rec.hook_exchange(tr._xchg)
        for i, supervise in enumerate(steps):
            rec.calls.append(f"   step {i} supervise={supervise}")
            if graphed:
                out = tr.step_graphed(*_train_inputs(n), supervise=supervise, warmup=1)
            else:
                out = tr.step(*_train_inputs(n), supervise=supervise)
        torch.cuda.synchronize()
        rec.calls.append(f"   dp_scheme {tr.dp_scheme} comm {sorted(tr.comm.items())} gradless {tr.gradless_ranges}")
        losses = torch.stack([torch.as_tensor(out[k] if out[k] is not None else 0.0).float().reshape(()).cpu() for k in LOSSES])
        return losses, tr.flat_g.p, tr.flat_d.p
    rec.case(title, run, loose=loose)


def train(rec):
    import torch.distributed as dist
    _train_case(rec, "v4 bf16: supervised, unsupervised, supervised", steps=(True, False, True))
    _train_case(rec, "v4 bf16 fused_decoder_update=False", fused_decoder_update=False)
    os.environ["PCAA_DEC_W16"] = "1"
    _train_case(rec, "v4 bf16 PCAA_DEC_W16=1, two steps", steps=(True, True))
    del os.environ["PCAA_DEC_W16"]
    _train_case(rec, "v4 bf16 step_graphed: eager warm-up, capture", steps=(True, True), graphed=True)
    _train_case(rec, "base bf16", variant="base")
    _train_case(rec, "v1 bf16", variant="v1")
    _train_case(rec, "v1 bf16 learn_centroids=True", variant="v1", learn_centroids=True)
    _train_case(rec, "v3 bf16", variant="v3")
    _train_case(rec, "v4 bf16 N=50: padded decoder", n=50)
    _train_case(rec, "emulate_world=2 all-reduce fp32 buckets", emulate_world=2)
    _train_case(rec, "emulate_world=2 all-reduce bf16 buckets", emulate_world=2, grad_compress="bf16")
    _train_case(rec, "emulate_world=2 dp_gather", emulate_world=2, dp_gather=True)
    _train_case(rec, "emulate_world=8 dp_gather", emulate_world=8, dp_gather=True)
    _train_case(rec, "emulate_world=8 dp_gather time_comm", emulate_world=8, dp_gather=True, time_comm=True)
    # every output of every case is hashed: two runs of one tree return the same bits, parameters after three steps included
    # -- but for flat_g.p of the one fp32-mode case, whose fp32 products accumulate with atomics in a varying order
    _train_case(rec, "emulate_world=2 dp_gather fp32: falls back to all-reduce", emulate_world=2, dp_gather=True,
                precision="fp32", loose=(1,))
    # the sharded optimizer wants a process group: one rank, the transport of tests/test_dp_rehearsal.py
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group("gloo", init_method=f"file://{tmp}/store", rank=0, world_size=1)
        for compress in (None, "bf16"):
            _train_case(rec, f"dp_zero one-rank group grad_compress={compress}", process_group=dist.group.WORLD,
                        force_collectives=True, dp_zero=True, grad_compress=compress)
            _train_case(rec, f"all-reduce one-rank group grad_compress={compress}", process_group=dist.group.WORLD,
                        force_collectives=True, grad_compress=compress)
        dist.destroy_process_group()


ROUTES = {"score": score, "live": live, "tracks": tracks}


def main(what):
    B, T = 4, constants.NSTEPS
    constants.NFEATURES = C
    rec = _lib._lib = Recorder(_lib.load())
    rec.hook_sync()
    if what == "train":
        train(rec)
        print("\n".join(rec.calls))
        return
    if what in ROUTES:
        means = O.sample_distant_points(32, K, 10, 10).float().to(DEV)
        for mode in ("fp32", "bf16"):
            rec.calls.append(f"==== {what} {mode}")
            F.set_precision(mode)
            ROUTES[what](rec, means)
        torch.cuda.synchronize()
        print("\n".join(rec.calls))
        return
    x = syn.synthetic_pcs(B, T, N, C, seed=1).to(DEV).permute(0, 3, 1, 2)
    if what == "eval":
        enc = _encoder()
        logits, fv, st = F.encoder_forward(enc, x, False, mode="fp32", want_bwd=True)
        F.encoder_backward(enc, st, torch.ones_like(logits), torch.ones_like(fv), need_dx=True)
    else:
        cfg = dict(constants.CONFIG, NMAX=N, TRAIN_CLASSES=list(range(K)), BATCH_SIZE=B)
        tr = PCAATrainer(cfg, device=DEV, precision=what)
        for i, m in enumerate((tr.encoder, tr.decoder, tr.discriminator, tr.decoder_projection_head,
                               tr.discriminator_projection_head)):
            syn.deterministic_fill_(m, 30 + i)
        tr.set_prior_means(O.sample_distant_points(32, K, 10, 10).float())
        tr.finalize()
        tr.train()
        tr.step(x, syn.synthetic_labels(B, K, seed=2).to(DEV), syn.synthetic_z0(B, 32, seed=3).to(DEV),
                syn.synthetic_alphas(B, seed=4).to(DEV))
    torch.cuda.synchronize()
    print("\n".join(rec.calls))


if __name__ == "__main__":
    main(sys.argv[1])
