"""Thin tensor-level wrappers over the C ABI (include/pcaa_hip.h).

Every function takes torch CUDA(=HIP) tensors, validates what the kernels
assume (device, dtype, contiguity, shapes) on the host BEFORE launching, and
launches on torch's current stream.  torch is used for allocation only.
"""
import ctypes
import os

import torch

from . import _lib
from ._lib import ACT_ELU, ACT_NONE, KC, PCAA_BF16, PCAA_F32, RC, check
from .datasets import RawPrep

PCAA_SPLIT_F16 = 2      # include/pcaa_hip.h

NREP = 16          # replicas of a BatchNorm statistics row (spreads fp64 atomics)
BN_EPS = 1e-5
BN_MOMENTUM = 0.1


def _p(t):
    return None if t is None else t.data_ptr()      # (ctypes takes the int for a void*: no c_void_p object per argument)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _s():
    """the current stream's handle.  Through torch's C entry points when it has them: torch.cuda.current_stream() walks
    ~10 Python frames (device-index resolution, an availability check that reads os.environ) -- 8 us a call, 86 calls a
    step = a sixth of the step's host time (cProfile, round 3)"""
    if _raw_stream is not None and _raw_device is not None:
        return _raw_stream(_raw_device())
    return torch.cuda.current_stream().cuda_stream


_get_cur_stream = getattr(torch._C, "_cuda_getCurrentStream", None)
_set_cur_stream = getattr(torch._C, "_cuda_setStream", None)


def current_stream():
    """torch.cuda.current_stream() of the current device without its ~8 us of Python (see _s)."""
    if _get_cur_stream is None or _raw_device is None:
        return torch.cuda.current_stream()
    sd = _get_cur_stream(_raw_device())
    return torch.cuda.Stream(stream_id=sd[0], device_index=sd[1], device_type=sd[2])


class on_stream:
    """``with on_stream(st):`` = ``with torch.cuda.stream(st):`` for a stream of the CURRENT device, through the same C
    entry points (torch._C._cuda_setStream) minus the Python around them: the step switches streams ~20 times."""
    __slots__ = ("st", "prev")

    def __init__(self, st):
        self.st = st
        self.prev = None

    def __enter__(self):
        # torch._C._cuda_getCurrentStream / _cuda_setStream / _cuda_getDevice are PRIVATE torch entry points (present in
        # the 2.x series this image ships): when any is missing, or the stream belongs to another device than the
        # current one (the raw path saves and restores the current device's stream only -- round-3 advisor finding),
        # the public context manager runs instead
        if (_set_cur_stream is None or _get_cur_stream is None or _raw_device is None
                or self.st.device_index != _raw_device()):
            self.prev = torch.cuda.stream(self.st)
            self.prev.__enter__()
            return self
        self.prev = _get_cur_stream(_raw_device())
        st = self.st
        _set_cur_stream(stream_id=st.stream_id, device_index=st.device_index, device_type=st.device_type)
        return self

    def __exit__(self, *exc):
        if isinstance(self.prev, tuple):
            _set_cur_stream(stream_id=self.prev[0], device_index=self.prev[1], device_type=self.prev[2])
        else:
            self.prev.__exit__(*exc)
        return False


def _dt(t):
    if t.dtype == torch.float32:
        return PCAA_F32
    if t.dtype == torch.bfloat16:
        return PCAA_BF16
    raise TypeError(f"unsupported dtype {t.dtype}")


def _chk(t, name, dtype=None, dim=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: expected a tensor on the HIP device, got "
                           f"{'cpu tensor' if isinstance(t, torch.Tensor) else type(t)} "
                           "(this package has no CPU path)")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if dim is not None and t.dim() != dim:
        raise ValueError(f"{name}: expected {dim}-D, got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous (shape {tuple(t.shape)}, strides {t.stride()})")
    return t


class LaunchTimer:
    """Optional per-launch HIP-event timing of pcaa_gemm calls (bench.py uses it
    to measure the dominant kernel's average duration inside the timed region;
    events are recorded on the stream the kernels are launched on)."""

    def __init__(self, only_prefix=None):
        self.records = []      # (key, flops, bytes, events)
        # every timed launch costs two event packets on the stream (~0.3 ms per step when all ~45
        # GEMM launches are timed); bench.py restricts the timing to the kernel it reports
        self.only_prefix = only_prefix

    def wants(self, key):
        return self.only_prefix is None or key.startswith(self.only_prefix)

    def summary(self):
        torch.cuda.synchronize()
        agg = {}
        for key, flops, nbytes, ev in self.records:
            if not ev.valid():
                continue
            a = agg.setdefault(key, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            a["launches"] += 1
            a["ms"] += ev.elapsed_ms()
            a["flops"] += flops
            a["bytes"] += nbytes
        return agg


class _TorchEvents:
    """two marker events around a call (each drains the queue: ~25 us on top of the kernel)"""

    def __init__(self):
        self.e0 = torch.cuda.Event(enable_timing=True)
        self.e1 = torch.cuda.Event(enable_timing=True)
        self.e0.record()

    def end(self):
        self.e1.record()
        return self

    def valid(self):
        return True

    def elapsed_ms(self):
        return self.e0.elapsed_time(self.e1)


class _KernelEvents:
    """start/stop events attached to the next LDS-DMA GEMM launch itself (pcaa_time_next_gemm): the
    kernel's own begin/end timestamps, as rocprofv3 reports them."""

    def __init__(self):
        lib = _lib.load()
        self.a, self.b = ctypes.c_void_p(), ctypes.c_void_p()
        check(lib.pcaa_timing_events_create(ctypes.byref(self.a), ctypes.byref(self.b)), "pcaa_timing_events_create")
        check(lib.pcaa_time_next_gemm(self.a, self.b), "pcaa_time_next_gemm")
        self.ok = False

    def end(self):
        lib = _lib.load()
        self.ok = not lib.pcaa_timing_pending()       # consumed by the launch?
        if not self.ok:
            lib.pcaa_time_next_gemm(None, None)
        return self

    def valid(self):
        return self.ok

    def elapsed_ms(self):
        ms = ctypes.c_float()
        check(_lib.load().pcaa_timing_elapsed_ms(self.a, self.b, ctypes.byref(ms)), "pcaa_timing_elapsed_ms")
        return float(ms.value)

    def __del__(self):
        try:
            _lib.load().pcaa_timing_events_destroy(self.a, self.b)
        except Exception:
            pass


def _begin_timing(key):
    return _KernelEvents() if key.startswith(("gemm_bf16_v2_kernel", "gemm_bf16_v2rc_kernel")) else _TorchEvents()


TIMER = None


def set_timer(timer):
    global TIMER
    TIMER = timer


def _timed(key, launch, flops, nbytes):
    """``launch()``, recorded under ``key`` when a LaunchTimer is installed and wants it.  ``key`` may be a callable
    (the route query of ops.gemm): it runs only with a timer installed.  Without one this is ``launch()`` and nothing
    else -- no ctypes call, no event (see _s for what host time per launch costs a step)."""
    timer = TIMER
    if timer is None:
        return launch()
    if callable(key):
        key = key()
    if not timer.wants(key):
        return launch()
    ev = _begin_timing(key)
    launch()
    ev.end()
    timer.records.append((key, flops, float(nbytes), ev))


class StatsPool:
    """One fp64 buffer for all BatchNorm statistics of a step, cleared by ONE
    fill at the start of the step instead of one per layer and direction."""

    def __init__(self, device, capacity_doubles=4 << 20):
        self.buf = torch.zeros(capacity_doubles, dtype=torch.float64, device=device)
        self.off = 0

    def begin(self):
        if self.off:
            self.buf[:self.off].zero_()
        self.off = 0

    def take_raw(self, n):
        """n zeroed doubles (16-B granular) from the pool, or None when it is full"""
        n = (n + 1) // 2 * 2
        if self.off + n > self.buf.numel():
            return None
        v = self.buf[self.off:self.off + n]
        self.off += n
        return v

    def take(self, ch):
        # + 2 doubles: the arrival counter of a finalize carried by the producer (BnTailFwd / BnTailBwd below), zeroed
        # with the statistics by begin(); 16-B granularity keeps every buffer aligned
        n = NREP * 2 * ch
        if self.off + n + 2 > self.buf.numel():
            return None
        v = self.buf[self.off:self.off + n].view(NREP, 2, ch)
        v._pcaa_counter = self.buf[self.off + n:self.off + n + 1].view(torch.int32)
        self.off += n + 2
        return v


STATS_POOL = None


def set_stats_pool(pool):
    global STATS_POOL
    STATS_POOL = pool


def new_stats(ch, device):
    if STATS_POOL is not None and STATS_POOL.buf.device == torch.device(device):
        v = STATS_POOL.take(ch)
        if v is not None:
            return v
    buf = torch.zeros(NREP * 2 * ch + 2, dtype=torch.float64, device=device)
    v = buf[:NREP * 2 * ch].view(NREP, 2, ch)
    v._pcaa_counter = buf[NREP * 2 * ch:NREP * 2 * ch + 1].view(torch.int32)
    return v


# ------------------------------------------------------------------ finalize carried by the producer (csrc/bn_tail.h)
# A BnTailFwd / BnTailBwd describes the BatchNorm finalize of the statistics a launch is about to accumulate.  The
# producer's wrapper calls arm(stats) right before its launch and resolve(stats) right after: if the launch could carry
# the tail (its last workgroup then writes the coefficients) resolve() has nothing to do, otherwise -- SyncBN (``sync``:
# the statistics are all-reduced first), a producer or shape that does not carry tails -- it runs the stand-alone kernel.
TAILS = {"enabled": os.environ.get("PCAA_BN_TAIL", "1") != "0", "taken": 0, "standalone": 0}


class BnTailFwd:
    def __init__(self, count, lin_bias, bn, ch, sync=None, update_running=True):
        self.count, self.lin_bias, self.bn, self.ch, self.sync, self.update_running = count, lin_bias, bn, ch, sync, update_running
        self.out = None
        self.armed = False
        self.count_out = count            # the count the statistics were averaged over (global under SyncBN)

    def arm(self, stats):
        counter = getattr(stats, "_pcaa_counter", None)
        if self.sync is not None or counter is None or not TAILS["enabled"]:
            return
        dev, bn, ch = stats.device, self.bn, self.ch
        scale = torch.empty(ch, dtype=torch.float32, device=dev)
        self.out = (scale, torch.empty_like(scale), torch.empty_like(scale), torch.empty_like(scale))
        rm = bn.running_mean if self.update_running else None
        rv = bn.running_var if self.update_running else None
        nbt = bn.num_batches_tracked if self.update_running else None
        check(_lib.load().pcaa_bn_tail_arm_fwd(_p(stats), NREP, int(self.count), _p(self.lin_bias), _p(bn.weight), _p(bn.bias),
                                               _p(rm), _p(rv), _p(nbt), BN_MOMENTUM if bn.momentum is None else bn.momentum,
                                               bn.eps, *(_p(t) for t in self.out), ch, _p(counter)), "pcaa_bn_tail_arm_fwd")
        self.armed = True

    def resolve(self, stats):
        """-> (scale, shift, mean, rstd)"""
        lib = _lib.load()
        if self.armed and not lib.pcaa_bn_tail_pending():
            TAILS["taken"] += 1
            return self.out
        if self.armed:
            lib.pcaa_bn_tail_disarm()
        count = self.sync(stats, self.count) if self.sync is not None else self.count
        self.count_out = count
        TAILS["standalone"] += 1
        self.out = bn_finalize(stats, count, self.lin_bias, self.bn, self.ch, self.update_running)
        return self.out


class BnTailBwd:
    def __init__(self, count, bn, mean, rstd, ch, dgamma=None, dbeta=None, sync=None):
        self.count, self.bn, self.mean, self.rstd, self.ch, self.sync = count, bn, mean, rstd, ch, sync
        self.dgamma, self.dbeta = dgamma, dbeta
        self.out = None
        self.armed = False

    def arm(self, stats):
        counter = getattr(stats, "_pcaa_counter", None)
        if self.sync is not None or counter is None or not TAILS["enabled"]:
            return
        dev, ch = stats.device, self.ch
        coef = torch.empty((3, ch), dtype=torch.float32, device=dev)
        dgamma = torch.empty(ch, dtype=torch.float32, device=dev) if self.dgamma is None else self.dgamma
        dbeta = torch.empty(ch, dtype=torch.float32, device=dev) if self.dbeta is None else self.dbeta
        self.out = (coef, dgamma, dbeta)
        check(_lib.load().pcaa_bn_tail_arm_bwd(_p(stats), NREP, int(self.count), _p(self.bn.weight), _p(self.mean),
                                               _p(self.rstd), _p(coef), _p(dgamma), _p(dbeta), ch, _p(counter)),
              "pcaa_bn_tail_arm_bwd")
        self.armed = True

    def resolve(self, stats):
        """-> (coef, dgamma, dbeta)"""
        lib = _lib.load()
        if self.armed and not lib.pcaa_bn_tail_pending():
            TAILS["taken"] += 1
            return self.out
        if self.armed:
            lib.pcaa_bn_tail_disarm()
        if self.sync is not None:
            self.sync(stats, 0)
        TAILS["standalone"] += 1
        self.out = bn_bwd_finalize(stats, self.count, self.bn, self.mean, self.rstd, self.ch, dgamma=self.dgamma,
                                   dbeta=self.dbeta)
        return self.out


# ------------------------------------------------------------------ GEMM
def gemm_v2_enable(on=True):
    """Lab switch (pcaa_gemm_v2_enable): with ``on=False`` the 4-wave tile loops (csrc/gemm_v2.h) decline every launch --
    plain products then take the register-staged 256 x 256 kernel, the fused entry points report their shapes unsupported.
    (Rounds 1-4 routed to the 8-wave loop here; round 5 removed it.)"""
    check(_lib.load().pcaa_gemm_v2_enable(int(bool(on))), "pcaa_gemm_v2_enable")


# LaunchTimer / PMC key of the kernel a product takes, by the PCAA_GEMM_KERNEL_* that pcaa_gemm_route answers (rocprofv3
# lists the instantiations as separate kernels; the 4-wave loops are timed kernel-exactly, the rest with stream events)
_GEMM_KEYS = {_lib.GEMM_KERNEL_F32_TILE128: "gemm_f32_kernel",
              _lib.GEMM_KERNEL_BF16_SMALL: "gemm_bf16_kernel",
              _lib.GEMM_KERNEL_BF16_STAGED: "gemm_bf16_big_kernel<{dt},{lay},{lay}>",
              _lib.GEMM_KERNEL_V2_KC: "gemm_bf16_v2_kernel<{dt},plain>",       # PointNet forward / plain dgrad
              _lib.GEMM_KERNEL_V2_RC: "gemm_bf16_v2rc_kernel<f32>"}            # the weight gradients


def _gemm_key(what, *args):
    """the key of the kernel the library would launch for the arguments of pcaa_gemm_route"""
    kernel = _lib.load().pcaa_gemm_route(*args)
    check(int(kernel < 0), what)          # a refusal: raised as the launch would raise it
    a_dtype, a_layout, b_dtype, b_layout, c_dtype = args[2], args[3], args[6], args[7], args[10]
    if kernel == _lib.GEMM_KERNEL_BF16_STAGED and not (a_dtype == b_dtype == PCAA_BF16 and a_layout == b_layout):
        return "gemm_bf16_big_kernel"
    return _GEMM_KEYS[kernel].format(dt="bf16" if c_dtype == PCAA_BF16 else "f32", lay="KC" if a_layout == KC else "RC")


def gemm(A, a_layout, B, b_layout, M, N, K, *, lda=None, ldb=None, out=None, out_dtype=torch.float32,
         bias=None, colstats=None, split_k=1, accumulate=False, math=PCAA_F32, tail=None):
    """out[M,N] (=|+=) A(M,K) . B(K,N) (+bias).  A/B are 2-D contiguous tensors
    whose storage order is given by the layout flag (see pcaa_hip.h).  ``tail``: the BatchNorm finalize of
    ``colstats`` (BnTailFwd), carried by this launch when it can be."""
    _chk(A, "gemm.A", dim=2)
    _chk(B, "gemm.B", dim=2)
    ea = (M, K) if a_layout == KC else (K, M)
    eb = (N, K) if b_layout == KC else (K, N)
    if tuple(A.shape) != ea or tuple(B.shape) != eb:
        raise ValueError(f"gemm: operand shapes {tuple(A.shape)} {tuple(B.shape)} do not match "
                         f"M={M} N={N} K={K} layouts {a_layout},{b_layout}")
    lda = A.stride(0) if lda is None else lda
    ldb = B.stride(0) if ldb is None else ldb
    atomic = split_k > 1 or accumulate
    if out is None:
        if atomic:
            out = torch.zeros((M, N), dtype=torch.float32, device=A.device)
        else:
            out = torch.empty((M, N), dtype=out_dtype, device=A.device)
    else:
        _chk(out, "gemm.out")
        if out.numel() != M * N:
            raise ValueError(f"gemm: out has {out.numel()} elements, need {M * N}")
    if bias is not None:
        _chk(bias, "gemm.bias", torch.float32)
        if bias.numel() != N:
            raise ValueError("gemm: bias length")
    if colstats is not None:
        _chk(colstats, "gemm.colstats", torch.float64)
        if tuple(colstats.shape) != (NREP, 2, N):
            raise ValueError("gemm: colstats shape")
    da, db, dc = _dt(A), _dt(B), _dt(out)
    args = (math, _p(A), da, a_layout, lda, _p(B), db, b_layout, ldb, _p(out), dc, N, M, N, K, _p(bias), _p(colstats), NREP,
            int(split_k), int(bool(accumulate)))
    if tail is not None:
        tail.arm(colstats)
    _timed(lambda: _gemm_key("pcaa_gemm", *args, 0), lambda: check(_lib.load().pcaa_gemm(*args, _s()), "pcaa_gemm"), 2.0 * M * N * K,
           (4 - 2 * da) * M * K + (4 - 2 * db) * N * K + (4 - 2 * dc) * M * N)          # (PCAA_BF16 = 1: 2 bytes, PCAA_F32 = 0: 4)
    if tail is not None:
        tail.resolve(colstats)
    return out


def gemm_group_rc_f32(products):
    """``products``: up to 8 tuples (A [K,M] fp32, B [K,N] fp32, C [M,N] fp32 -- accumulated into, the caller zeroes it --,
    split_k): all of them C += A^T . B on the exact-fp32 matrix pipe in ONE launch (pcaa_gemm_group_rc_f32_slabs), whose K
    ranges write slabs that pcaa_splitk_reduce then adds into C in a fixed order (no atomics: the same result every run)."""
    n = len(products)
    if not 1 <= n <= 8:
        raise ValueError("gemm_group_rc_f32: 1..8 products")
    ptr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    ints = lambda vs: (ctypes.c_int * n)(*[int(v) for v in vs])
    lib = _lib.load()
    splits = []
    for A, B, C, sk in products:
        _chk(A, "gemm_group.A", torch.float32, 2)
        _chk(B, "gemm_group.B", torch.float32, 2)
        _chk(C, "gemm_group.C", torch.float32)
        if A.shape[0] != B.shape[0] or C.numel() != A.shape[1] * B.shape[1] or A.stride(0) != A.shape[1] or B.stride(0) != B.shape[1]:
            raise ValueError("gemm_group_rc_f32: A [K,M], B [K,N] with contiguous rows, C [M,N]")
        splits.append(lib.pcaa_gemm_num_splits(PCAA_F32, A.shape[0], int(sk)))
    sizes = [ns * p[2].numel() for ns, p in zip(splits, products)]          # multiples of 4 floats: 16-B aligned slices
    slabs = torch.empty(sum(sizes), dtype=torch.float32, device=products[0][2].device).split(sizes)
    check(lib.pcaa_gemm_group_rc_f32_slabs(
        n, ptr([p[0] for p in products]), ptr([p[1] for p in products]), ptr(slabs),
        ints([p[0].shape[1] for p in products]), ints([p[1].shape[1] for p in products]), ints([p[0].shape[0] for p in products]),
        ints([p[3] for p in products]), _s()), "pcaa_gemm_group_rc_f32_slabs")
    for (_, _, C, _), sl, ns in zip(products, slabs, splits):
        check(lib.pcaa_splitk_reduce(_p(sl), ns, C.numel(), C.numel(), _p(C), 1, _s()), "pcaa_splitk_reduce")


def gemm_slabs(A, a_layout, B, b_layout, M, N, K, split_k, out=None, accumulate=False, math=PCAA_BF16,
               colstats=None, tail=None, reduce_ctx=None):
    """Split-K product without atomics: every split writes its partial [M,N] slab, a second
    launch sums the slabs into ``out`` (=|+=).  Used for the long-K weight gradients, where the
    atomic epilogue (256 KB of fp32 atomics per workgroup) cost as much as the MFMA loop."""
    _chk(A, "gemm_slabs.A", dim=2)
    _chk(B, "gemm_slabs.B", dim=2)
    if (M * N) % 4:
        raise ValueError("gemm_slabs: M*N must be a multiple of 4")
    lib = _lib.load()
    ns = lib.pcaa_gemm_num_splits(math, K, int(split_k))
    stride = M * N
    slabs = torch.empty(ns * stride, dtype=torch.float32, device=A.device)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    else:
        _chk(out, "gemm_slabs.out", torch.float32)
        if out.numel() != M * N:
            raise ValueError("gemm_slabs: out size")
    da, db = _dt(A), _dt(B)
    ab = (math, _p(A), da, a_layout, A.stride(0), _p(B), db, b_layout, B.stride(0))
    _timed(lambda: _gemm_key("pcaa_gemm_slabs", *ab, _p(slabs), PCAA_F32, N, M, N, K, None, None, 0, int(split_k), 0, stride),
           lambda: check(lib.pcaa_gemm_slabs(*ab, _p(slabs), stride, M, N, K, int(split_k), _s()), "pcaa_gemm_slabs"),
           2.0 * M * N * K, (4 - 2 * da) * M * K + (4 - 2 * db) * N * K + ns * stride * 4)
    if colstats is not None:
        # reduction fused with the BatchNorm column statistics of the result
        if accumulate:
            raise ValueError("gemm_slabs: colstats with accumulate is not supported")
        _chk(colstats, "gemm_slabs.colstats", torch.float64)
        check(lib.pcaa_splitk_reduce_stats(_p(slabs), ns, stride, _p(out), _p(colstats), NREP, M, N, _s()),
              "pcaa_splitk_reduce_stats")
        if tail is not None:
            tail.resolve(colstats)
        return out
    if reduce_ctx is not None:
        # ``reduce_ctx(slabs)``: a context manager under which the slab reduction is enqueued (functional's wgrad side
        # stream: the sum only feeds the optimizer, so it leaves the stream that carries the backward's chain)
        with reduce_ctx(slabs):
            check(lib.pcaa_splitk_reduce(_p(slabs), ns, stride, stride, _p(out), int(bool(accumulate)), _s()),
                  "pcaa_splitk_reduce")
        return out
    check(lib.pcaa_splitk_reduce(_p(slabs), ns, stride, stride, _p(out), int(bool(accumulate)), _s()),
          "pcaa_splitk_reduce")
    return out


def gemm_slabs_part(A, B, M, N, K, split_k, slabs, math=PCAA_BF16):
    """The weight-gradient form (RC x RC, contraction over the rows) over the rows the two views cover: writes the
    partial products of its splits into ``slabs`` (a float32 view with room for them, ``M*N`` apart) and returns their
    count.  Launch only -- the caller sums the slabs (``splitk_reduce``).  With this a long-K product can be cut in
    two launches on different streams (functional's overlapped weight gradients)."""
    _chk(A, "gemm_slabs_part.A", dim=2)
    _chk(B, "gemm_slabs_part.B", dim=2)
    if A.shape[0] != K or B.shape[0] != K or A.shape[1] != M or B.shape[1] != N:
        raise ValueError("gemm_slabs_part: operand views must be [K, M] and [K, N]")
    lib = _lib.load()
    ns = lib.pcaa_gemm_num_splits(math, K, int(split_k))
    stride = M * N
    _chk(slabs, "gemm_slabs_part.slabs", torch.float32)
    if slabs.numel() < ns * stride or not slabs.is_contiguous():
        raise ValueError("gemm_slabs_part: slab view too small")
    check(lib.pcaa_gemm_slabs(math, _p(A), _dt(A), RC, A.stride(0), _p(B), _dt(B), RC, B.stride(0),
                              _p(slabs), stride, M, N, K, int(split_k), _s()), "pcaa_gemm_slabs")
    return ns


def splitk_reduce(slabs, ns, M, N, out, accumulate=False):
    """out[M, N] (=|+=) the sum of ``ns`` slabs laid ``M*N`` apart"""
    _chk(out, "splitk_reduce.out", torch.float32)
    if out.numel() != M * N or slabs.numel() < ns * M * N:
        raise ValueError("splitk_reduce: sizes")
    check(_lib.load().pcaa_splitk_reduce(_p(slabs), int(ns), M * N, M * N, _p(out), int(bool(accumulate)), _s()),
          "pcaa_splitk_reduce")
    return out


def gemm_affine_elu(a, W16, scale, shift, pool_rows=0):
    """ELU(scale * (a[M,K] @ W16[N,K]^T) + shift) in one launch (eval-mode BatchNorm+ELU in the GEMM
    epilogue): bf16 [M,N], or with pool_rows in {32,64,128} its mean over groups of pool_rows consecutive
    rows, fp32 [M/pool_rows, N].  a, W16 bf16; shapes as gemm_dgrad_bn_supported."""
    _chk(a, "gemm_affine_elu.a", torch.bfloat16, 2)
    _chk(W16, "gemm_affine_elu.W16", torch.bfloat16, 2)
    _chk(scale, "gemm_affine_elu.scale", torch.float32)
    _chk(shift, "gemm_affine_elu.shift", torch.float32)
    M, K = a.shape
    N = W16.shape[0]
    if (W16.shape[1] != K or scale.numel() != N or shift.numel() != N or not gemm_dgrad_bn_supported(M, N, K)
            or pool_rows not in (0, 32, 64, 128)):
        raise ValueError(f"gemm_affine_elu: unsupported shapes a {tuple(a.shape)} W {tuple(W16.shape)} pool {pool_rows}")
    if pool_rows:
        out = torch.empty((M // pool_rows, N), dtype=torch.float32, device=a.device)
    else:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=a.device)
    # eval-mode epilogues (BatchNorm affine + ELU [+ mean-pool])
    _timed("gemm_bf16_v2_kernel<bf16,affine_elu>",
           lambda: check(_lib.load().pcaa_gemm_affine_elu(_p(a), a.stride(0), _p(W16), W16.stride(0), _p(out), N, _p(scale),
                                                          _p(shift), M, N, K, int(pool_rows), _s()), "pcaa_gemm_affine_elu"),
           2.0 * M * N * K, 2 * (M * K + N * K) + out.numel() * out.element_size())
    return out


def gemm_dgrad_bn_supported(M, N, K):
    return bool(_lib.load().pcaa_gemm_dgrad_bn_supported(int(M), int(N), int(K)))


# ---------------------------------------------------------------- eval-mode PointNet layers in fp8 (csrc/gemm_fp8.hip)
PCAA_FP8_E4M3 = 3
FP8 = torch.float8_e4m3fn      # OCP e4m3fn; the tensors only carry the bytes -- no ATen arithmetic runs on them


def quantize_weight_fp8(W2d):
    """fp32 W [R, C] -> (W8 e4m3 [R, C], s fp32 [R]): per row s = 2^(E-8) with absmax = f 2^E, f in [0.5, 1) (1 for a zero
    or non-finite row), W8 = e4m3fn_rne(W / s).  The caller folds s into the layer's BatchNorm scale."""
    _chk(W2d, "quantize_weight_fp8.W", torch.float32, 2)
    R, C = W2d.shape
    W8 = torch.empty((R, C), dtype=torch.uint8, device=W2d.device)
    s = torch.empty((R,), dtype=torch.float32, device=W2d.device)
    check(_lib.load().pcaa_quantize_weight_fp8(_p(W2d), _p(W8), _p(s), R, C, _s()), "pcaa_quantize_weight_fp8")
    return W8.view(FP8), s


def gemm_fp8_supported(M, N, K):
    return bool(_lib.load().pcaa_gemm_fp8_supported(int(M), int(N), int(K)))


def gemm_fp8_affine_elu(a8, W8, scale8, shift, pool_rows=0, out_dtype=None):
    """ELU(scale8 * (a8[M,K] @ W8[N,K]^T) + shift) on the block-scaled fp8 MFMA, e4m3 operands, fp32 accumulation:
    e4m3 (default) or bf16 [M, N]; with pool_rows in {32, 64, 128} the fp32 mean over groups of pool_rows rows
    [M / pool_rows, N].  scale8 = scale * s of quantize_weight_fp8; shapes as gemm_fp8_supported."""
    _chk(a8, "gemm_fp8_affine_elu.a8", FP8, 2)
    _chk(W8, "gemm_fp8_affine_elu.W8", FP8, 2)
    _chk(scale8, "gemm_fp8_affine_elu.scale8", torch.float32)
    _chk(shift, "gemm_fp8_affine_elu.shift", torch.float32)
    M, K = a8.shape
    N = W8.shape[0]
    if out_dtype is None:
        out_dtype = torch.float32 if pool_rows else FP8
    if (W8.shape[1] != K or scale8.numel() != N or shift.numel() != N or not gemm_fp8_supported(M, N, K)
            or pool_rows not in (0, 32, 64, 128) or (pool_rows and M % pool_rows)):
        raise ValueError(f"gemm_fp8_affine_elu: unsupported shapes a8 {tuple(a8.shape)} W8 {tuple(W8.shape)} pool {pool_rows}")
    if out_dtype not in ((torch.float32,) if pool_rows else (FP8, torch.bfloat16)):
        raise TypeError(f"gemm_fp8_affine_elu: out_dtype {out_dtype} with pool_rows {pool_rows}")
    out = torch.empty((M // pool_rows if pool_rows else M, N), dtype=out_dtype, device=a8.device)
    code = PCAA_FP8_E4M3 if out_dtype == FP8 else _dt(out)
    _timed("gemm_fp8_kernel<affine_elu>",
           lambda: check(_lib.load().pcaa_gemm_fp8_affine_elu(_p(a8), a8.stride(0), _p(W8), W8.stride(0), _p(out), code, N,
                                                              _p(scale8), _p(shift), M, N, K, int(pool_rows), _s()),
                         "pcaa_gemm_fp8_affine_elu"),
           2.0 * M * N * K, M * K + N * K + out.numel() * out.element_size())
    return out


def gemm_dgrad_bn(dy, Wt, y, scale, shift, mean, rstd, tail=None):
    """dz[M,N] = (dy[M,K] @ Wt[N,K]^T) * ELU'(y*scale+shift) plus the BatchNorm-backward statistics of
    the layer that owns y -- the dgrad of the layer above fused with the first half of this layer's
    backward.  Returns (dz bf16, stats).  (The variant that rebuilt y of the FIRST PointNet layer from the points in the
    epilogue -- measured slower than the separate statistics pass in round 1, never on -- left with the 8-wave kernel.)"""
    _chk(dy, "gemm_dgrad_bn.dy", torch.bfloat16, 2)
    _chk(Wt, "gemm_dgrad_bn.Wt", torch.bfloat16, 2)
    _chk(y, "gemm_dgrad_bn.y", torch.bfloat16, 2)
    M, K = dy.shape
    N = Wt.shape[0]
    if Wt.shape[1] != K or tuple(y.shape) != (M, N):
        raise ValueError("gemm_dgrad_bn: shape mismatch")
    dz = torch.empty_like(y)
    stats = new_stats(N, dy.device)
    if tail is not None:
        tail.arm(stats)
    # its own instantiation (epilogue carries ELU' + statistics)
    _timed("gemm_bf16_v2_kernel<bf16,dgrad_bn>",
           lambda: check(_lib.load().pcaa_gemm_dgrad_bn(_p(dy), dy.stride(0), _p(Wt), Wt.stride(0), _p(y), _p(dz), dz.stride(0),
                                                        _p(scale), _p(shift), _p(mean), _p(rstd), _p(stats), NREP, M, N, K,
                                                        None, 0, None, _s()), "pcaa_gemm_dgrad_bn"),
           2.0 * M * N * K, 2 * (M * K + N * K + 2 * M * N))
    if tail is not None:
        tail.resolve(stats)
    return dz, stats


# ------------------------------------------------------------------ split-operand parity mode (pcaa_gemm_split3)
# power-of-two image scales that keep each kind of tensor in fp16's normal range (|x| in 6e-5 .. 65504)
SPLIT_SCALE_ACT = 1.0            # activations after BatchNorm + ELU: O(1)
SPLIT_SCALE_WEIGHT = 256.0       # weights ~ 1/sqrt(fan_in): their lo halves would be fp16 subnormals unscaled
SPLIT_SCALE_GRAD = 65536.0       # gradients of a batch-mean loss: 1e-8 .. 1e-2


class SplitImage:
    """The [hi | lo] fp16 image of an fp32 [rows, ch] tensor times ``scale`` (hi = fp16(s v), lo = fp16(s v - hi)):
    ``img`` is fp16 [rows, 2 ch]; ``shape`` / ``device`` are those of the fp32 tensor it stands for."""
    __slots__ = ("img", "rows", "ch", "scale")
    dtype = "split_fp16"

    def __init__(self, img, rows, ch, scale):
        self.img, self.rows, self.ch, self.scale = img, rows, ch, float(scale)

    @property
    def shape(self):
        return (self.rows, self.ch)

    @property
    def device(self):
        return self.img.device

    def float(self):
        """the fp32 tensor the image stands for (tests)"""
        return (self.img[:, :self.ch].float() + self.img[:, self.ch:].float()) / self.scale


# Range guard (round 4, advisor finding): fp16 images hold |scale * v| <= 65504 while the reference's fp32 tensors have no
# limit.  The producers saturate what leaves the range and raise a per-device flag (csrc/common.h, split_guard); the
# flag is registered right before every producer launch (split_image_empty is on each producer's path) and read by
# range_check() -- PCAATrainer.check() calls it -- which raises: the caller reruns in "fp32" (exact, no range limit).
_RANGE_FLAGS = {}


def _range_flag(device):
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    t = _RANGE_FLAGS.get(idx)
    if t is None:
        t = _RANGE_FLAGS[idx] = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", idx))
    return t


def range_check(device=None, reset=True):
    """Raise FloatingPointError if an fp16x3-mode operand image saturated on ``device`` since the last check (one
    host sync).  The products of such a step are wrong; rerun it with precision "fp32"."""
    if device is None:
        idxs = list(_RANGE_FLAGS)
    else:
        dev = torch.device(device)       # an index-less "cuda" is the CURRENT device, as in _range_flag
        idxs = [dev.index if dev.index is not None else torch.cuda.current_device()]
    for idx in idxs:
        t = _RANGE_FLAGS.get(idx)
        if t is not None and int(t.item()):
            if reset:
                t.zero_()
            raise FloatingPointError(
                "fp16x3 mode: a value left the fp16 range of its [hi | lo] operand image (|scale * v| > 65504 or NaN; "
                f"scales: activations {SPLIT_SCALE_ACT:g}, weights {SPLIT_SCALE_WEIGHT:g}, gradients {SPLIT_SCALE_GRAD:g}); "
                "the image was saturated and this step's products are not fp32-grade -- use precision='fp32'")


def split_image_empty(rows, ch, device, scale):
    check(_lib.load().pcaa_set_range_flag(_p(_range_flag(device))), "pcaa_set_range_flag")
    return SplitImage(torch.empty((rows, 2 * ch), dtype=torch.float16, device=device), rows, ch, scale)


def split_f16(x2d, transpose=False, scale=SPLIT_SCALE_WEIGHT):
    """fp32 [rows, ch] -> SplitImage of x2d (``transpose``: of x2d^T, without materialising the transpose)"""
    _chk(x2d, "split_f16.x", torch.float32, 2)
    rows, ch = x2d.shape
    out = split_image_empty(ch, rows, x2d.device, scale) if transpose else split_image_empty(rows, ch, x2d.device, scale)
    check(_lib.load().pcaa_split_f16(_p(x2d), _p(out.img), rows, ch, int(bool(transpose)), float(scale), _s()),
          "pcaa_split_f16")
    return out


def gemm_split3_supported(M, N, K):
    return bool(_lib.load().pcaa_gemm_split3_supported(int(M), int(N), int(K)))


def gemm_split3(A, B, layout, M, N, K, colstats=None, tail=None, out=None):
    """out[M,N] fp32 = A . B^T (layout KC: A [M,K], B [N,K]) or A^T . B (RC: A [K,M], B [K,N]) from SplitImages:
    hi.hi + lo.hi + hi.lo on the f16 MFMA pipe, fp32 accumulate, rescaled by 1 / (A.scale B.scale)."""
    ea = (M, K) if layout == KC else (K, M)
    eb = (N, K) if layout == KC else (K, N)
    if tuple(A.shape) != ea or tuple(B.shape) != eb:
        raise ValueError(f"gemm_split3: operand shapes {A.shape} {B.shape} do not match M={M} N={N} K={K}")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    if tail is not None:
        tail.arm(colstats)
    _timed("gemm_bf16_v2_kernel<f32,split3>" if layout == KC else "gemm_bf16_v2rc_kernel<f32,split3>",
           lambda: check(_lib.load().pcaa_gemm_split3(_p(A.img), _p(B.img), layout, A.img.stride(0), B.img.stride(0), _p(out), N,
                                                      M, N, K, _p(colstats), NREP, 1.0 / (A.scale * B.scale), _s()), "pcaa_gemm_split3"),
           3 * 2.0 * M * N * K, 4 * (A.img.numel() // 2 + B.img.numel() // 2 + M * N))
    if tail is not None:
        tail.resolve(colstats)
    return out


def gemm_slabs_split3(A, B, M, N, K, split_k, out=None):
    """The weight-gradient form (RC x RC: A [K,M], B [K,N] SplitImages, contraction over the K rows) with slab split-K."""
    if tuple(A.shape) != (K, M) or tuple(B.shape) != (K, N):
        raise ValueError("gemm_slabs_split3: operand shapes")
    lib = _lib.load()
    ns = lib.pcaa_gemm_split3_num_splits(K, int(split_k))
    stride = M * N
    slabs = torch.empty(ns * stride, dtype=torch.float32, device=A.device)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    _timed("gemm_bf16_v2rc_kernel<f32,split3>",
           lambda: check(lib.pcaa_gemm_slabs_split3(_p(A.img), _p(B.img), RC, A.img.stride(0), B.img.stride(0), _p(slabs), stride,
                                                    M, N, K, int(split_k), 1.0 / (A.scale * B.scale), _s()), "pcaa_gemm_slabs_split3"),
           3 * 2.0 * M * N * K, 4 * (A.img.numel() // 2 + B.img.numel() // 2) + ns * stride * 4)
    check(lib.pcaa_splitk_reduce(_p(slabs), ns, stride, stride, _p(out), 0, _s()), "pcaa_splitk_reduce")
    return out


def bn_act_fwd_split(y, scale, shift):
    """a = ELU(y*scale+shift) as a SplitImage (fp32 y)"""
    _chk(y, "bn_act_fwd_split.y", torch.float32, 2)
    a = split_image_empty(y.shape[0], y.shape[1], y.device, SPLIT_SCALE_ACT)
    check(_lib.load().pcaa_bn_act_fwd_split(_p(y), _p(a.img), _p(scale), _p(shift), y.shape[0], y.shape[1], a.scale, _s()),
          "pcaa_bn_act_fwd_split")
    return a


def bn_bwd_dy_fused_split(y, scale, shift, coef, *, da=None, dpool=None, group_rows=0, pool_scale=1.0):
    """bn_bwd_dy_fused with dy written as a SplitImage (fp32 y / da)"""
    _chk(y, "bn_bwd_dy_fused_split.y", torch.float32, 2)
    rows, ch = y.shape
    dy = split_image_empty(rows, ch, y.device, SPLIT_SCALE_GRAD)
    check(_lib.load().pcaa_bn_bwd_dy_fused_split(_p(da), _p(dpool), int(group_rows), float(pool_scale), _p(y), _p(dy.img),
                                                 _p(scale), _p(shift), _p(coef), rows, ch, dy.scale, _s()),
          "pcaa_bn_bwd_dy_fused_split")
    return dy


def bn_bwd_dy_split(dz, y, coef):
    """dy = coef0*dz + coef1*y + coef2 as a SplitImage (fp32 dz, y): behind gemm_dgrad_bn_split3"""
    _chk(dz, "bn_bwd_dy_split.dz", torch.float32, 2)
    _chk(y, "bn_bwd_dy_split.y", torch.float32, 2)
    rows, ch = y.shape
    dy = split_image_empty(rows, ch, y.device, SPLIT_SCALE_GRAD)
    check(_lib.load().pcaa_bn_bwd_dy_split(_p(dz), _p(y), _p(dy.img), _p(coef), rows, ch, dy.scale, _s()),
          "pcaa_bn_bwd_dy_split")
    return dy


def gemm_dgrad_bn_split3_supported(M, N, K):
    return bool(_lib.load().pcaa_gemm_split3_supported(int(M), int(N), int(K)))


def gemm_dgrad_bn_split3(dy, wt, y, scale, shift, mean, rstd, tail=None):
    """dgrad of a PointNet layer on split-fp16 operands (dy [M, K], wt [N, K] SplitImages) fused with the first half of
    the BatchNorm + ELU backward of the layer below (fp32 y [M, N]): returns (dz fp32 [M, N], stats)."""
    M, K = dy.shape
    N = wt.shape[0]
    if wt.shape[1] != K or tuple(y.shape) != (M, N):
        raise ValueError("gemm_dgrad_bn_split3: operand shapes")
    _chk(y, "gemm_dgrad_bn_split3.y", torch.float32, 2)
    dz = torch.empty((M, N), dtype=torch.float32, device=y.device)
    stats = new_stats(N, y.device)
    if tail is not None:
        tail.arm(stats)
    check(_lib.load().pcaa_gemm_dgrad_bn_split3(_p(dy.img), dy.img.stride(0), _p(wt.img), wt.img.stride(0), _p(y), _p(dz), N,
                                                _p(scale), _p(shift), _p(mean), _p(rstd), _p(stats), NREP, M, N, K,
                                                1.0 / (dy.scale * wt.scale), _s()), "pcaa_gemm_dgrad_bn_split3")
    if tail is not None:
        tail.resolve(stats)
    return dz, stats


def pick_split_k(M, N, K, target_blocks=1024, bk=32, tile=128):
    tiles = ((M + tile - 1) // tile) * ((N + tile - 1) // tile)
    if tiles >= target_blocks:
        return 1
    s = max(1, target_blocks // tiles)
    return max(1, min(s, K // (4 * bk) if K >= 4 * bk else 1))


def cast_bf16(W2d, want_plain=True, want_transposed=True, out=None):
    """bf16 shadows of an fp32 weight matrix [R,C]: (W16 [R,C], W16t [C,R]).  ``out``: the plain image's destination."""
    _chk(W2d, "cast_bf16.W", torch.float32, 2)
    R, C = W2d.shape
    if out is not None:
        _chk(out, "cast_bf16.out", torch.bfloat16, 2)
        if tuple(out.shape) != (R, C):
            raise ValueError("cast_bf16: out shape")
    w = out if out is not None else (torch.empty((R, C), dtype=torch.bfloat16, device=W2d.device) if want_plain else None)
    wt = torch.empty((C, R), dtype=torch.bfloat16, device=W2d.device) if want_transposed else None
    check(_lib.load().pcaa_cast_bf16(_p(W2d), _p(w), _p(wt), R, C, _s()), "pcaa_cast_bf16")
    return w, wt


def pointnet_in_ok(C, cout):
    return 1 <= C <= 8 and cout % 4 == 0 and 4 <= cout <= 1024 and 256 % (cout // 4) == 0


def pointnet_in_fwd(x2d, W2d, bias, out_dtype, stats=None, tail=None):
    """y[P,cout] = x2d[P,C] . W2d[cout,C]^T + bias (+ BatchNorm statistics; ``tail``: their finalize, BnTailFwd)."""
    _chk(x2d, "pointnet_in.x", torch.float32, 2)
    _chk(W2d, "pointnet_in.W", torch.float32, 2)
    P, C = x2d.shape
    cout = W2d.shape[0]
    if W2d.shape[1] != C or not pointnet_in_ok(C, cout):
        raise ValueError(f"pointnet_in_fwd: unsupported shape C={C} cout={cout}")
    if out_dtype is None:                    # statistics only (recompute path): y is never stored
        if stats is None:
            raise ValueError("pointnet_in_fwd: statistics-only call needs stats")
        if tail is not None:
            tail.arm(stats)
        check(_lib.load().pcaa_pointnet_in_fwd(_p(x2d), C, _p(W2d), None, None, PCAA_F32, P, cout, _p(stats), NREP,
                                               _s()), "pcaa_pointnet_in_fwd(stats)")
        if tail is not None:
            tail.resolve(stats)
        return None
    y = torch.empty((P, cout), dtype=out_dtype, device=x2d.device)
    if tail is not None and stats is not None:
        tail.arm(stats)
    check(_lib.load().pcaa_pointnet_in_fwd(_p(x2d), C, _p(W2d), _p(bias), _p(y), _dt(y), P, cout, _p(stats), NREP, _s()),
          "pcaa_pointnet_in_fwd")
    if tail is not None and stats is not None:
        tail.resolve(stats)
    return y


def pointnet_in_apply(x2d, W2d, scale, shift, out_dtype):
    """a[P,cout] = ELU((x2d . W2d^T) * scale + shift): first PointNet layer, y recomputed, not read."""
    _chk(x2d, "pointnet_in_apply.x", torch.float32, 2)
    _chk(W2d, "pointnet_in_apply.W", torch.float32, 2)
    P, C = x2d.shape
    cout = W2d.shape[0]
    if W2d.shape[1] != C or not pointnet_in_ok(C, cout):
        raise ValueError(f"pointnet_in_apply: unsupported shape C={C} cout={cout}")
    if out_dtype == SplitImage.dtype:
        a = split_image_empty(P, cout, x2d.device, SPLIT_SCALE_ACT)
        check(_lib.load().pcaa_pointnet_in_apply(_p(x2d), C, _p(W2d), _p(scale), _p(shift), _p(a.img), PCAA_SPLIT_F16, P,
                                                 cout, _s()), "pcaa_pointnet_in_apply(split)")
        return a
    a = torch.empty((P, cout), dtype=out_dtype, device=x2d.device)
    code = PCAA_FP8_E4M3 if out_dtype == FP8 else _dt(a)      # (e4m3: the operand of gemm_fp8_affine_elu)
    check(_lib.load().pcaa_pointnet_in_apply(_p(x2d), C, _p(W2d), _p(scale), _p(shift), _p(a), code, P, cout, _s()),
          "pcaa_pointnet_in_apply")
    return a


def pointnet_in_bwd_stats(da, x2d, W2d, scale, shift, mean, rstd, tail=None):
    _chk(da, "pointnet_in_bwd_stats.da", dim=2)
    _chk(x2d, "pointnet_in_bwd_stats.x", torch.float32, 2)
    P, cout = da.shape
    C = x2d.shape[1]
    if x2d.shape[0] != P or tuple(W2d.shape) != (cout, C) or not pointnet_in_ok(C, cout):
        raise ValueError("pointnet_in_bwd_stats: unsupported shape")
    stats = new_stats(cout, da.device)
    if tail is not None:
        tail.arm(stats)
    check(_lib.load().pcaa_pointnet_in_bwd_stats(_p(da), _dt(da), _p(x2d), C, _p(W2d), _p(scale), _p(shift), _p(mean),
                                                 _p(rstd), _p(stats), NREP, P, cout, _s()),
          "pcaa_pointnet_in_bwd_stats")
    if tail is not None:
        tail.resolve(stats)
    return stats


def points_moments(x2d):
    """fp64 second moments and sums of the points (pcaa_points_moments) for pointnet_in_bwd_onepass."""
    _chk(x2d, "points_moments.x", torch.float32, 2)
    if not (1 <= x2d.shape[1] <= 8 and x2d.shape[0] >= 1):
        raise ValueError(f"points_moments: unsupported shape {tuple(x2d.shape)}")
    lib = _lib.load()
    n = lib.pcaa_points_moments_size()
    mom = STATS_POOL.take_raw(n) if (STATS_POOL is not None and STATS_POOL.buf.device == x2d.device) else None
    if mom is None:
        mom = torch.zeros(n, dtype=torch.float64, device=x2d.device)
    else:
        mom = mom[:n]
    check(lib.pcaa_points_moments(_p(x2d), x2d.shape[1], x2d.shape[0], _p(mom), _s()), "pcaa_points_moments")
    return mom


def pointnet_in_moment_coeffs(x2d, W2d, lin_bias, bn, mom=None, update_running=True):
    """Train-mode BatchNorm coefficients of the first PointNet layer from the points' moments (no pass over [P, cout]):
    -> (scale, shift, mean, rstd, mom)."""
    _chk(x2d, "pointnet_in_moment_coeffs.x", torch.float32, 2)
    _chk(W2d, "pointnet_in_moment_coeffs.W", torch.float32, 2)
    P, C = x2d.shape
    cout = W2d.shape[0]
    if W2d.shape[1] != C or not (1 <= C <= 8 and cout >= 1 and P >= 1):       # the kernel reads W as [cout, C]
        raise ValueError(f"pointnet_in_moment_coeffs: unsupported shape C={C} W {tuple(W2d.shape)}")
    if mom is None:
        mom = points_moments(x2d)
    tail = BnTailFwd(P, lin_bias, bn, cout, update_running=update_running)
    stats = mom                       # the armed finalize is matched by this pointer
    stats._pcaa_counter = mom         # (no arrival counter is used by this producer; any non-null word)
    tail.arm(stats)
    if not tail.armed:
        raise RuntimeError("pointnet_in_moment_coeffs: the carried finalize is switched off")
    check(_lib.load().pcaa_pointnet_in_moment_stats(_p(mom), _p(W2d), C, cout, _s()), "pcaa_pointnet_in_moment_stats")
    TAILS["taken"] += 1
    return tail.out + (mom,)


def pointnet_in_bwd_onepass(da, x2d, W2d, scale, shift, mean, rstd, tail, mom=None, out=None):
    """Backward of the recompute layer from ONE read of the incoming gradient: BatchNorm-backward statistics (their
    finalize: ``tail``, an ops.BnTailBwd) and G = dz^T.x in one launch, then dW = c0*G + c1*(W.x^T x) + c2*sum x.
    Returns dW [cout, C] (``out`` is overwritten)."""
    _chk(da, "pointnet_in_bwd_onepass.da", dim=2)
    _chk(x2d, "pointnet_in_bwd_onepass.x", torch.float32, 2)
    P, cout = da.shape
    C = x2d.shape[1]
    if x2d.shape[0] != P or tuple(W2d.shape) != (cout, C) or not pointnet_in_ok(C, cout):
        raise ValueError("pointnet_in_bwd_onepass: unsupported shape")
    lib = _lib.load()
    if mom is None:
        mom = points_moments(x2d)
    # G is accumulated against the points centred on their mean (csrc/pointnet_in.hip, MODE 3); under SyncBN the pivot is
    # the GLOBAL mean -- the same on every rank, so that the dropped term pivot (x) sum dy cancels in the all-reduce
    pivot_mom, pivot_count = mom, P
    if tail.sync is not None:
        pivot_mom = mom.clone()
        pivot_count = tail.sync(pivot_mom, P)
    stats = new_stats(cout, da.device)
    # one row per workgroup, stored (not accumulated): the combine sums the rows in a fixed order
    g_rows = lib.pcaa_pointnet_in_bwd_g_rows(P)
    G = torch.empty((g_rows, cout, C), dtype=torch.float32, device=da.device)
    tail.arm(stats)
    check(lib.pcaa_pointnet_in_bwd_onepass_rows(_p(da), _dt(da), _p(x2d), C, _p(W2d), _p(scale), _p(shift), _p(mean),
                                                _p(rstd), _p(stats), NREP, _p(G), P, cout, _p(pivot_mom), 1.0 / pivot_count,
                                                _s()), "pcaa_pointnet_in_bwd_onepass_rows")
    coef, _, _ = tail.resolve(stats)
    if out is None:
        out = torch.empty((cout, C), dtype=torch.float32, device=da.device)
    check(lib.pcaa_pointnet_in_bwd_combine(_p(G), g_rows, _p(W2d), _p(mom), _p(coef), _p(out), cout, C, P, _p(pivot_mom),
                                           1.0 / pivot_count, _s()), "pcaa_pointnet_in_bwd_combine")
    return out


def pointnet_in_bwd_wgrad(da, x2d, W2d, scale, shift, coef, out=None, out_is_zero=False, dz_is_pre=False):
    _chk(da, "pointnet_in_bwd_wgrad.da", dim=2)
    _chk(x2d, "pointnet_in_bwd_wgrad.x", torch.float32, 2)
    P, cout = da.shape
    C = x2d.shape[1]
    if x2d.shape[0] != P or tuple(W2d.shape) != (cout, C) or not pointnet_in_ok(C, cout):
        raise ValueError("pointnet_in_bwd_wgrad: unsupported shape")
    if out is None:
        out = torch.zeros((cout, C), dtype=torch.float32, device=da.device)
    elif not out_is_zero:
        out.zero_()
    check(_lib.load().pcaa_pointnet_in_bwd_wgrad(_p(da), _dt(da), _p(x2d), C, _p(W2d), _p(scale), _p(shift), _p(coef),
                                                 _p(out), P, cout, int(bool(dz_is_pre)), _s()),
          "pcaa_pointnet_in_bwd_wgrad")
    return out


def pointnet_in_wgrad(dy, x2d, out=None, out_is_zero=False):
    _chk(dy, "pointnet_in_wgrad.dy", dim=2)
    _chk(x2d, "pointnet_in_wgrad.x", torch.float32, 2)
    P, cout = dy.shape
    C = x2d.shape[1]
    if x2d.shape[0] != P or not pointnet_in_ok(C, cout):
        raise ValueError("pointnet_in_wgrad: unsupported shape")
    if out is None:
        out = torch.zeros((cout, C), dtype=torch.float32, device=dy.device)
    elif not out_is_zero:
        out.zero_()
    check(_lib.load().pcaa_pointnet_in_wgrad(_p(dy), _dt(dy), _p(x2d), C, _p(out), P, cout, _s()),
          "pcaa_pointnet_in_wgrad")
    return out


# ------------------------------------------------------------------ BatchNorm pieces
def bn_finalize(stats, count, lin_bias, bn, ch, update_running=True):
    dev = stats.device
    scale = torch.empty(ch, dtype=torch.float32, device=dev)
    shift = torch.empty_like(scale)
    mean = torch.empty_like(scale)
    rstd = torch.empty_like(scale)
    lib = _lib.load()
    rm = bn.running_mean if update_running else None
    rv = bn.running_var if update_running else None
    nbt = bn.num_batches_tracked if update_running else None
    check(lib.pcaa_bn_finalize(_p(stats), NREP, int(count), _p(lin_bias), _p(bn.weight), _p(bn.bias),
                               _p(rm), _p(rv), _p(nbt), BN_MOMENTUM if bn.momentum is None else bn.momentum,
                               bn.eps, _p(scale), _p(shift), _p(mean), _p(rstd), ch, _s()), "pcaa_bn_finalize")
    return scale, shift, mean, rstd


def bn_eval_coeffs(bn, ch, lin_bias=None):
    dev = bn.weight.device
    scale = torch.empty(ch, dtype=torch.float32, device=dev)
    shift = torch.empty_like(scale)
    check(_lib.load().pcaa_bn_eval_coeffs(_p(bn.weight), _p(bn.bias), _p(bn.running_mean), _p(bn.running_var),
                                          _p(lin_bias), bn.eps, _p(scale), _p(shift), ch, _s()),
          "pcaa_bn_eval_coeffs")
    return scale, shift


def bn_act_fwd(y, scale, shift):
    _chk(y, "bn_act_fwd.y", dim=2)
    a = torch.empty_like(y)
    check(_lib.load().pcaa_bn_act_fwd(_p(y), _p(a), _dt(y), _p(scale), _p(shift), y.shape[0], y.shape[1], _s()),
          "pcaa_bn_act_fwd")
    return a


def bn_act_meanpool_fwd(y, scale, shift, groups, group_rows, mean=None, rstd=None):
    """Mean over each group of rows of ELU(BN(y)).  With mean/rstd (training) also returns the
    per-(group, channel) sums (e1, e2) that bn_pool_bwd_stats turns into the backward statistics."""
    _chk(y, "bn_act_meanpool_fwd.y", dim=2)
    if y.shape[0] != groups * group_rows:
        raise ValueError("bn_act_meanpool_fwd: rows != groups*group_rows")
    out = torch.empty((groups, y.shape[1]), dtype=torch.float32, device=y.device)
    e = None
    if mean is not None:
        e = torch.empty((2, groups, y.shape[1]), dtype=torch.float32, device=y.device)
    check(_lib.load().pcaa_bn_act_meanpool_fwd(_p(y), _dt(y), _p(scale), _p(shift), _p(mean), _p(rstd), _p(out),
                                               _p(e[0]) if e is not None else None,
                                               _p(e[1]) if e is not None else None,
                                               groups, group_rows, y.shape[1], _s()), "pcaa_bn_act_meanpool_fwd")
    return out if e is None else (out, e)


def bn_pool_bwd_stats(dpool, e, pool_scale, tail=None):
    """BatchNorm-backward statistics of a mean-pooled layer from the forward's (e1, e2) sums."""
    _chk(dpool, "bn_pool_bwd_stats.dpool", torch.float32, 2)
    _chk(e, "bn_pool_bwd_stats.e", torch.float32, 3)
    groups, ch = dpool.shape
    if tuple(e.shape) != (2, groups, ch):
        raise ValueError("bn_pool_bwd_stats: e shape")
    stats = new_stats(ch, dpool.device)
    if tail is not None:
        tail.arm(stats)
    check(_lib.load().pcaa_bn_pool_bwd_stats(_p(dpool), _p(e[0]), _p(e[1]), float(pool_scale), _p(stats), NREP,
                                             groups, ch, _s()), "pcaa_bn_pool_bwd_stats")
    if tail is not None:
        tail.resolve(stats)
    return stats


def _grad_source(who, y, da, dpool, group_rows):
    """the checks of a [rows, ch] pass whose gradient comes dense (da, like y) or pooled (dpool fp32, one row per
    group_rows rows of y) -> (rows, ch)"""
    _chk(y, f"{who}.y", dim=2)
    rows, ch = y.shape
    if da is not None:
        _chk(da, f"{who}.da", y.dtype, 2)
        if da.shape != y.shape:
            raise ValueError(f"{who}: da shape")
    else:
        _chk(dpool, f"{who}.dpool", torch.float32, 2)
        if dpool.shape[0] * group_rows != rows or dpool.shape[1] != ch:
            raise ValueError(f"{who}: dpool shape")
    return rows, ch


def bn_act_bwd_dz(y, scale, shift, mean, rstd, *, da=None, dpool=None, group_rows=0, pool_scale=1.0, out=None):
    rows, ch = _grad_source("bn_act_bwd_dz", y, da, dpool, group_rows)
    dz = out if out is not None else torch.empty_like(y)
    stats = new_stats(ch, y.device)
    check(_lib.load().pcaa_bn_act_bwd_dz(_p(da), _p(dpool), int(group_rows), float(pool_scale), _p(y), _p(dz),
                                         _dt(y), _p(scale), _p(shift), _p(mean), _p(rstd), _p(stats), NREP,
                                         rows, ch, _s()), "pcaa_bn_act_bwd_dz")
    return dz, stats


def bn_act_bwd_stats(y, scale, shift, mean, rstd, *, da=None, dpool=None, group_rows=0, pool_scale=1.0, tail=None):
    """Statistics-only pass of the BatchNorm backward (sum dz, sum dz*yhat): reads, writes nothing."""
    _chk(y, "bn_act_bwd_stats.y", dim=2)
    rows, ch = y.shape
    stats = new_stats(ch, y.device)
    check(_lib.load().pcaa_bn_act_bwd_dz(_p(da), _p(dpool), int(group_rows), float(pool_scale), _p(y), None,
                                         _dt(y), _p(scale), _p(shift), _p(mean), _p(rstd), _p(stats), NREP,
                                         rows, ch, _s()), "pcaa_bn_act_bwd_dz(stats)")
    if tail is not None:
        tail.resolve(stats)
    return stats


def bn_bwd_dy_fused(y, scale, shift, coef, *, da=None, dpool=None, group_rows=0, pool_scale=1.0, out=None):
    """dy = coef0*(da*ELU'(BN(y))) + coef1*y + coef2 in one pass (dz never stored)."""
    _chk(y, "bn_bwd_dy_fused.y", dim=2)
    rows, ch = y.shape
    dy = out if out is not None else torch.empty_like(y)
    check(_lib.load().pcaa_bn_bwd_dy_fused(_p(da), _p(dpool), int(group_rows), float(pool_scale), _p(y), _p(dy),
                                           _dt(y), _p(scale), _p(shift), _p(coef), rows, ch, _s()),
          "pcaa_bn_bwd_dy_fused")
    return dy


def bn_bwd_finalize(stats, count, bn, mean, rstd, ch, dgamma=None, dbeta=None):
    dev = stats.device
    coef = torch.empty((3, ch), dtype=torch.float32, device=dev)
    dgamma = torch.empty(ch, dtype=torch.float32, device=dev) if dgamma is None else dgamma
    dbeta = torch.empty(ch, dtype=torch.float32, device=dev) if dbeta is None else dbeta
    check(_lib.load().pcaa_bn_bwd_finalize(_p(stats), NREP, int(count), _p(bn.weight), _p(mean), _p(rstd),
                                           _p(coef), _p(dgamma), _p(dbeta), ch, _s()), "pcaa_bn_bwd_finalize")
    return coef, dgamma, dbeta


def bn_eval_moments(bn, ch, lin_bias=None):
    """eval-mode (mean, rstd) of the bias-free y: running_mean - bias and 1/sqrt(running_var + eps)"""
    dev = bn.weight.device
    mean = torch.empty(ch, dtype=torch.float32, device=dev)
    rstd = torch.empty_like(mean)
    check(_lib.load().pcaa_bn_eval_moments(_p(bn.running_mean), _p(bn.running_var), _p(lin_bias), bn.eps, _p(mean),
                                           _p(rstd), ch, _s()), "pcaa_bn_eval_moments")
    return mean, rstd


def bn_eval_act_bwd(y, scale, shift, mean, rstd, *, da=None, dpool=None, group_rows=0, pool_scale=1.0, out=None):
    """Backward through eval-mode BatchNorm + ELU in one pass: dy = scale * (g * ELU'(scale*y + shift)) (``out`` may be
    ``da``) and the statistics {sum dz, sum dz*xhat} for bn_eval_bwd_finalize.  -> (dy, stats)"""
    rows, ch = _grad_source("bn_eval_act_bwd", y, da, dpool, group_rows)
    dy = out if out is not None else torch.empty_like(y)
    if dy.shape != y.shape or dy.dtype != y.dtype or not dy.is_contiguous():
        raise ValueError("bn_eval_act_bwd: out must be contiguous with y's shape and dtype")
    stats = new_stats(ch, y.device)
    check(_lib.load().pcaa_bn_eval_act_bwd(_p(da), _p(dpool), int(group_rows), float(pool_scale), _p(y), _p(dy),
                                           _dt(y), _p(scale), _p(shift), _p(mean), _p(rstd), _p(stats), NREP,
                                           rows, ch, _s()), "pcaa_bn_eval_act_bwd")
    return dy, stats


def bn_eval_bwd_finalize(stats, scale, ch, dgamma=None, dbeta=None, dbias=None):
    """-> (dgamma, dbeta, dbias), written into the given destinations where given"""
    dev = stats.device
    dgamma = torch.empty(ch, dtype=torch.float32, device=dev) if dgamma is None else dgamma
    dbeta = torch.empty(ch, dtype=torch.float32, device=dev) if dbeta is None else dbeta
    dbias = torch.empty(ch, dtype=torch.float32, device=dev) if dbias is None else dbias
    check(_lib.load().pcaa_bn_eval_bwd_finalize(_p(stats), NREP, _p(scale), _p(dgamma), _p(dbeta), _p(dbias), ch, _s()),
          "pcaa_bn_eval_bwd_finalize")
    return dgamma, dbeta, dbias


def bn_bwd_dy(dz, y, coef, out=None):
    dy = out if out is not None else torch.empty_like(dz)
    check(_lib.load().pcaa_bn_bwd_dy(_p(dz), _p(y), _p(dy), _dt(y), _p(coef), y.shape[0], y.shape[1], _s()),
          "pcaa_bn_bwd_dy")
    return dy


# ------------------------------------------------------------------ small helpers
def bias_act_(y, bias, act):
    _chk(y, "bias_act.y", torch.float32, 2)
    check(_lib.load().pcaa_bias_act(_p(y), _p(bias), act, y.shape[0], y.shape[1], _s()), "pcaa_bias_act")
    return y


def elu_bwd_from_out(da, a, out=None):
    _chk(da, "elu_bwd.da", torch.float32)
    _chk(a, "elu_bwd.a", torch.float32)
    dz = out if out is not None else torch.empty_like(da)
    check(_lib.load().pcaa_elu_bwd_from_out(_p(da), _p(a), _p(dz), da.numel(), _s()), "pcaa_elu_bwd_from_out")
    return dz


def colsum(x, out=None):
    _chk(x, "colsum.x", torch.float32, 2)
    out = torch.empty(x.shape[1], dtype=torch.float32, device=x.device) if out is None else out
    check(_lib.load().pcaa_colsum(_p(x), _p(out), x.shape[0], x.shape[1], _s()), "pcaa_colsum")
    return out


# ------------------------------------------------------------------ batch-skinny Linear layers (decoder)
def skinny_supported(M, N, K):
    return bool(_lib.load().pcaa_skinny_supported(int(M), int(N), int(K)))


def _w16_image(W16, W, what):
    """the bf16 image of weight W (pcaa_skinny_linear_*_w16): same shape, contiguous rows, bf16"""
    _chk(W16, what, torch.bfloat16, 2)
    if tuple(W16.shape) != tuple(W.shape) or W16.stride(1) != 1:
        raise ValueError(f"{what}: the bf16 image must have the weight's shape {tuple(W.shape)}, got {tuple(W16.shape)}")
    return W16


def skinny_linear_fwd(x, W, bias, act, exact=False, W16=None):
    """act(x[M,K] @ W[N,K]^T + bias) with M <= 64: one streaming pass over W.  ``exact``: fp32 products on the fp32
    matrix pipe (the parity modes) instead of bf16-rounded operands.  ``W16``: the bf16 image of W (every element the
    weight rounded to nearest even -- what the kernel's own conversion produces): streamed instead of W, same result."""
    _chk(x, "skinny_fwd.x", torch.float32, 2)
    _chk(W, "skinny_fwd.W", torch.float32, 2)
    M, K = x.shape
    N = W.shape[0]
    if W.shape[1] != K:
        raise ValueError("skinny_linear_fwd: shape mismatch")
    lib = _lib.load()
    ns = lib.pcaa_skinny_splits(2 if exact else 0, M, N, K)
    ws = torch.empty(ns * M * N, dtype=torch.float32, device=x.device)
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    if W16 is not None and not exact:
        Wsrc, fn, wb = _w16_image(W16, W, "skinny_fwd.W16"), lib.pcaa_skinny_linear_fwd_w16, 2
    else:
        Wsrc, fn, wb = W, (lib.pcaa_skinny_linear_fwd_exact if exact else lib.pcaa_skinny_linear_fwd), 4
    _timed("gemm_skinny_kernel", lambda: check(fn(_p(x), x.stride(0), _p(Wsrc), Wsrc.stride(0), _p(bias), act,
                                   _p(y), _p(ws), ws.numel(), M, N, K, ns, _s()),
                                "pcaa_skinny_linear_fwd"), 2.0 * M * N * K, wb * N * K + 4 * (M * K + M * N))
    return y


def skinny_linear_dgrad(dz, W, a_prev=None, out=None, accumulate=False, exact=False, W16=None):
    """dx[M,K] (=|+=) (dz[M,N] @ W[N,K]) * ELU'(a_prev) (a_prev: ELU OUTPUT of the layer below or None).
    ``W16``: the bf16 image of W, streamed instead of it (see skinny_linear_fwd)."""
    _chk(dz, "skinny_dgrad.dz", torch.float32, 2)
    _chk(W, "skinny_dgrad.W", torch.float32, 2)
    M, N = dz.shape
    K = W.shape[1]
    if W.shape[0] != N:
        raise ValueError("skinny_linear_dgrad: shape mismatch")
    if a_prev is not None:
        _chk(a_prev, "skinny_dgrad.a_prev", torch.float32)
        if a_prev.numel() != M * K:
            raise ValueError("skinny_linear_dgrad: a_prev size")
    if out is None:
        if accumulate:
            raise ValueError("skinny_linear_dgrad: accumulate needs out")
        out = torch.empty((M, K), dtype=torch.float32, device=dz.device)
    else:
        _chk(out, "skinny_dgrad.out", torch.float32)
        if out.numel() != M * K:
            raise ValueError("skinny_linear_dgrad: out size")
    lib = _lib.load()
    ns = lib.pcaa_skinny_splits(3 if exact else 1, M, N, K)
    ws = torch.empty(ns * M * K, dtype=torch.float32, device=dz.device)
    if W16 is not None and not exact:
        Wsrc, fn, wb = _w16_image(W16, W, "skinny_dgrad.W16"), lib.pcaa_skinny_linear_dgrad_w16, 2
    else:
        Wsrc, fn, wb = W, (lib.pcaa_skinny_linear_dgrad_exact if exact else lib.pcaa_skinny_linear_dgrad), 4
    _timed("gemm_skinny_kernel", lambda: check(fn(_p(dz), dz.stride(0), _p(Wsrc), Wsrc.stride(0), _p(out),
                                   _p(a_prev), int(bool(accumulate)), _p(ws), ws.numel(),
                                   M, N, K, ns, _s()),
                                "pcaa_skinny_linear_dgrad"), 2.0 * M * N * K, wb * N * K + 4 * (M * K + M * N))
    return out


def skinny_linear_wgrad(dz, x, out=None, exact=False):
    """dW[N,K] = dz[M,N]^T @ x[M,K] with M <= 64: one streaming store pass over dW."""
    _chk(dz, "skinny_wgrad.dz", torch.float32, 2)
    _chk(x, "skinny_wgrad.x", torch.float32, 2)
    M, N = dz.shape
    K = x.shape[1]
    if x.shape[0] != M:
        raise ValueError("skinny_linear_wgrad: shape mismatch")
    if out is None:
        out = torch.empty((N, K), dtype=torch.float32, device=dz.device)
    else:
        _chk(out, "skinny_wgrad.out")
        if out.numel() != N * K or out.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("skinny_linear_wgrad: out must hold N*K fp32 or bf16 elements")
    lib = _lib.load()
    if out.dtype == torch.bfloat16:       # the gradient as it crosses the wire (bf16 gradient buckets)
        if exact:
            raise ValueError("skinny_linear_wgrad: the exact variant writes fp32")
        _timed("gemm_skinny_kernel", lambda: check(lib.pcaa_skinny_linear_wgrad_bf16(_p(dz), dz.stride(0), _p(x), x.stride(0), _p(out), K,
                                                                      M, N, K, _s()),
                                    "pcaa_skinny_linear_wgrad_bf16"), 2.0 * M * N * K, 2 * N * K + 4 * (M * K + M * N))
        return out
    fn = lib.pcaa_skinny_linear_wgrad_exact if exact else lib.pcaa_skinny_linear_wgrad
    _timed("gemm_skinny_kernel", lambda: check(fn(_p(dz), dz.stride(0), _p(x), x.stride(0), _p(out), K, M, N, K, _s()),
                                "pcaa_skinny_linear_wgrad"), 2.0 * M * N * K, 4 * (N * K + M * K + M * N))
    return out


def _chk_adam_state(prefix, W, exp_avg, exp_avg_sq, N, K, dim=None, want=None):
    """The fused updates' (W, exp_avg, exp_avg_sq): contiguous fp32 device tensors of shape [N, K].  ``prefix`` names the
    wrapper ("skinny_wgrad_adam" for skinny_linear_wgrad_adam_); ``want``: the shape as the wrapper's message spells it."""
    fn = prefix.replace("skinny_", "skinny_linear_", 1) + "_"
    for t, nm in ((W, "W"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _chk(t, prefix + "." + nm, torch.float32, dim)
        if tuple(t.shape) != (N, K):
            raise ValueError(f"{fn}: {nm} must be {want or f'[{N},{K}]'}, got {tuple(t.shape)}")


def skinny_linear_wgrad_adam_(dz, x, W, exp_avg, exp_avg_sq, beta1, beta2, eps, coef_dev, grad_scale=1.0, exact=False):
    """W[N,K] <- Adam(W, dz[M,N]^T @ x[M,K]) in place, moments too (M <= 64): the weight gradient never reaches HBM.
    ``coef_dev``: the two step-dependent scalars of the optimizer step in progress (StepCount.coef_dev)."""
    _chk(dz, "skinny_wgrad_adam.dz", torch.float32, 2)
    _chk(x, "skinny_wgrad_adam.x", torch.float32, 2)
    M, N = dz.shape
    K = x.shape[1]
    if x.shape[0] != M:
        raise ValueError("skinny_linear_wgrad_adam_: shape mismatch")
    _chk_adam_state("skinny_wgrad_adam", W, exp_avg, exp_avg_sq, N, K)
    _chk(coef_dev, "skinny_wgrad_adam.coef", torch.float32)
    lib = _lib.load()
    fn = lib.pcaa_skinny_linear_wgrad_adam_exact if exact else lib.pcaa_skinny_linear_wgrad_adam
    _timed("gemm_skinny_kernel", lambda: check(fn(
        _p(dz), dz.stride(0), _p(x), x.stride(0), _p(W), _p(exp_avg), _p(exp_avg_sq), K, M, N, K, float(beta1),
        float(beta2), float(eps), float(grad_scale), _p(coef_dev), _s()), "pcaa_skinny_linear_wgrad_adam"),
        2.0 * M * N * K, 4 * (6 * N * K + M * K + M * N))
    return W


def gathered_rows_alloc(m):
    """rows a gathered operand of ``m`` valid rows must be allocated for (skinny_linear_wgrad_adam_rows_ reads whole
    64-row chunks: 64, 128, 256 or 512); None if m is beyond the kernel's 512"""
    for r in (64, 128, 256, 512):
        if m <= r:
            return r
    return None


def skinny_linear_wgrad_adam_rows_(dz_all, x_all, m, W, exp_avg, exp_avg_sq, beta1, beta2, eps, coef_dev, grad_scale=1.0):
    """The fused weight-gradient + Adam update from GATHERED rows (data parallel; pcaa_skinny_linear_wgrad_adam_rows):
    ``dz_all`` [R, N], ``x_all`` [R, K] hold the rows of all ranks stacked in their first ``m`` rows (R =
    gathered_rows_alloc(m); the rows behind m must be finite -- the buffers are zero-initialised once).
    W[N,K] <- Adam(W, grad_scale * dz_all[:m]^T @ x_all[:m]) in place, bf16 products."""
    _chk(dz_all, "skinny_wgrad_adam_rows.dz", torch.float32, 2)
    _chk(x_all, "skinny_wgrad_adam_rows.x", torch.float32, 2)
    R, N = dz_all.shape
    K = x_all.shape[1]
    need = gathered_rows_alloc(int(m))
    if need is None or x_all.shape[0] != R or R < need:
        raise ValueError(f"skinny_linear_wgrad_adam_rows_: {m} valid rows need buffers of {need} rows, got {R} / {x_all.shape[0]}")
    _chk_adam_state("skinny_wgrad_adam_rows", W, exp_avg, exp_avg_sq, N, K)
    _chk(coef_dev, "skinny_wgrad_adam_rows.coef", torch.float32)
    _timed("gemm_skinny_kernel", lambda: check(_lib.load().pcaa_skinny_linear_wgrad_adam_rows(
        _p(dz_all), dz_all.stride(0), _p(x_all), x_all.stride(0), _p(W), _p(exp_avg), _p(exp_avg_sq), K, int(m), N, K,
        float(beta1), float(beta2), float(eps), float(grad_scale), _p(coef_dev), R, _s()),
        "pcaa_skinny_linear_wgrad_adam_rows"), 2.0 * m * N * K, 4 * (6 * N * K + m * K + m * N))
    return W


PACK_ROWS = 64        # batch rows of one packed chunk (pcaa_pack_rows_t16)
PACK_MAX_CHUNKS = 8   # chunks one pcaa_skinny_linear_wgrad_adam_t16 launch contracts over


def packed_chunk_elems(N, K):
    """bf16 elements of one rank's packed weight-gradient operands of an [N, K] layer: (N + K) columns x 64 rows"""
    return int(_lib.load().pcaa_packed_chunk_elems(int(N), int(K)))


def pack_rows_t16(dz, x, out=None):
    """One rank's two weight-gradient operands of a batch-skinny layer -- dz [rows, N], x [rows, K], rows <= 64 -- as ONE
    packed chunk [(N + K) * 64] bf16 (transposed: a 128-B row per column of dz, then of x; rounded to nearest even; zero
    behind ``rows``): the form skinny_linear_wgrad_adam_t16_ contracts over and the data-parallel step all-gathers."""
    _chk(dz, "pack_rows_t16.dz", torch.float32, 2)
    _chk(x, "pack_rows_t16.x", torch.float32, 2)
    rows, N = dz.shape
    K = x.shape[1]
    if x.shape[0] != rows or rows > PACK_ROWS:
        raise ValueError(f"pack_rows_t16: dz {tuple(dz.shape)} / x {tuple(x.shape)}: equal row counts <= {PACK_ROWS}")
    n = packed_chunk_elems(N, K)
    if out is None:
        out = torch.empty(n, dtype=torch.bfloat16, device=dz.device)
    else:
        _chk(out, "pack_rows_t16.out", torch.bfloat16)
        if out.numel() != n:
            raise ValueError(f"pack_rows_t16: out must hold {n} bf16 elements, got {out.numel()}")
    check(_lib.load().pcaa_pack_rows_t16(_p(dz), dz.stride(0), N, _p(x), x.stride(0), K, rows, _p(out), _s()),
          "pcaa_pack_rows_t16")
    return out


def skinny_linear_wgrad_adam_t16_(packed, chunks, W, exp_avg, exp_avg_sq, beta1, beta2, eps, coef_dev, grad_scale=1.0):
    """The fused weight-gradient + Adam update from the ranks' PACKED operands (data parallel, round 6;
    pcaa_skinny_linear_wgrad_adam_t16): ``packed`` [>= chunks, (N + K) * 64] bf16, one pack_rows_t16 chunk per rank
    (a gathered buffer).  W[N,K] <- Adam(W, grad_scale * sum over the chunks of dz_c^T @ x_c) in place, bf16 products."""
    if (not isinstance(packed, torch.Tensor) or not packed.is_cuda or packed.dtype != torch.bfloat16 or packed.dim() != 2
            or packed.stride(1) != 1):
        raise TypeError("skinny_linear_wgrad_adam_t16_: packed must be a [chunks, >= (N + K) * 64] bf16 tensor on the HIP "
                        "device with contiguous rows")
    _chk(W, "skinny_wgrad_adam_t16.W", torch.float32, 2)
    N, K = W.shape
    _chk_adam_state("skinny_wgrad_adam_t16", W, exp_avg, exp_avg_sq, N, K, dim=2, want=tuple(W.shape))
    chunks = int(chunks)
    if not 1 <= chunks <= min(PACK_MAX_CHUNKS, packed.shape[0]) or packed.shape[1] < packed_chunk_elems(N, K):
        raise ValueError(f"skinny_linear_wgrad_adam_t16_: {chunks} chunks of an [{N},{K}] layer do not fit a packed buffer "
                         f"{tuple(packed.shape)} (at most {PACK_MAX_CHUNKS} chunks of {packed_chunk_elems(N, K)} elements)")
    _chk(coef_dev, "skinny_wgrad_adam_t16.coef", torch.float32)
    m = chunks * PACK_ROWS
    _timed("gemm_skinny_kernel", lambda: check(_lib.load().pcaa_skinny_linear_wgrad_adam_t16(
        _p(packed), packed.stride(0), chunks, _p(W), _p(exp_avg), _p(exp_avg_sq), K, N, K, float(beta1), float(beta2),
        float(eps), float(grad_scale), _p(coef_dev), _s()), "pcaa_skinny_linear_wgrad_adam_t16"),
        2.0 * m * N * K, 24 * N * K + 2 * m * (N + K))
    return W


def total(x, scale=1.0, out=None):
    _chk(x, "sum.x", torch.float32)
    out = torch.empty((), dtype=torch.float32, device=x.device) if out is None else _chk(out, "sum.out", torch.float32)
    if out.numel() != 1:
        raise ValueError("total: out must hold one float")
    check(_lib.load().pcaa_sum(_p(x), x.numel(), float(scale), _p(out), _s()), "pcaa_sum")
    return out


def rowsum(x, scale=1.0):
    _chk(x, "rowsum.x", torch.float32, 2)
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    check(_lib.load().pcaa_rowsum(_p(x), _p(out), x.shape[0], x.shape[1], float(scale), _s()), "pcaa_rowsum")
    return out


def scale_by_device_scalar(x, s):
    _chk(x, "scale.x", torch.float32)
    _chk(s, "scale.s", torch.float32)
    out = torch.empty_like(x)
    check(_lib.load().pcaa_scale_by_device_scalar(_p(x), _p(s), _p(out), x.numel(), _s()), "pcaa_scale_by_device_scalar")
    return out


def scale_rows(x, s):
    _chk(x, "scale_rows.x", torch.float32)
    _chk(s, "scale_rows.s", torch.float32)
    rows = s.numel()
    out = torch.empty_like(x)
    check(_lib.load().pcaa_scale_rows(_p(x), _p(s), _p(out), rows, x.numel() // rows, _s()), "pcaa_scale_rows")
    return out


def prior_sample(z0, means, gt, K):
    _chk(z0, "prior.z0", torch.float32, 2)
    _chk(means, "prior.means", torch.float32, 2)
    _chk(gt, "prior.gt", torch.int64, 1)
    B, D = z0.shape
    z = torch.empty_like(z0)
    oh = torch.empty((B, K), dtype=torch.float32, device=z0.device)
    check(_lib.load().pcaa_prior_sample(_p(z0), _p(means), _p(gt), B, K, D, _p(z), _p(oh), _s()), "pcaa_prior_sample")
    return z, oh


def pack_points(x):
    """logical [B,C,T,N] (any strides) -> contiguous point-major [B,T,N,C]."""
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
        raise RuntimeError("pack_points: expected a 4-D float32 tensor on the HIP device")
    B, C, T, N = x.shape
    out = torch.empty((B, T, N, C), dtype=torch.float32, device=x.device)
    sb, sc, st, sn = x.stride()
    check(_lib.load().pcaa_pack_points(_p(x), sb, sc, st, sn, _p(out), B, C, T, N, _s()), "pcaa_pack_points")
    return out


def _gather(who, unit, src, idx, out, err_flag):
    """the body of gather_rows (``unit`` = 16 bytes: pcaa_gather_rows takes the row size in bytes) and gather_rows_w4
    (4 bytes: pcaa_gather_rows_w4 takes it in 32-bit words)"""
    if not (isinstance(src, torch.Tensor) and src.is_cuda and src.is_contiguous() and src.dim() >= 1):
        raise RuntimeError(f"{who}: src must be a contiguous tensor on the HIP device (this package has no CPU path)")
    _chk(idx, who + ".idx", torch.int64, 1)
    row_bytes = src[0].numel() * src.element_size() if src.dim() > 1 else src.element_size()
    if row_bytes % unit or (unit == 4 and row_bytes == 0):
        raise ValueError(f"{who}: rows of {row_bytes} bytes are not a multiple of {unit}")
    n = idx.numel()
    if out is None:
        out = torch.empty((n,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    elif out.shape != (n,) + tuple(src.shape[1:]) or out.dtype != src.dtype or not out.is_contiguous():
        raise ValueError(f"{who}: out does not match")
    if err_flag is not None:
        _chk(err_flag, who + ".err_flag", torch.int32)
    if n:
        fn = getattr(_lib.load(), "pcaa_" + who)
        check(fn(_p(src), src.shape[0], row_bytes if unit == 16 else row_bytes // 4, _p(idx), _p(out), n, _p(err_flag), _s()),
              "pcaa_" + who)
    return out


def gather_rows(src, idx, out=None, err_flag=None):
    """out[r] = src[idx[r]] along dim 0 (device-side batch assembly; rows must be multiples of 16 bytes)."""
    return _gather("gather_rows", 16, src, idx, out, err_flag)


def gather_rows_w4(src, idx, out=None, err_flag=None):
    """``gather_rows`` for rows that are a multiple of 4 bytes only (pcaa_gather_rows_w4: a 3 000-byte frame of N = 150
    points x C = 5 features)."""
    return _gather("gather_rows_w4", 4, src, idx, out, err_flag)


def gather_frames(src, idx):
    """dst[r] = src[idx[r]] for rows of any whole number of 32-bit words: the 16-byte gather where a row allows it."""
    row_bytes = src[0].numel() * src.element_size()
    return gather_rows(src, idx) if row_bytes % 16 == 0 else gather_rows_w4(src, idx)


def gather_sum_rows(src, csr_off, csr_idx, out=None, err_flag=None):
    """The adjoint of ``gather_frames``: ``dst[u] = sum_{k in [csr_off[u], csr_off[u + 1])} src[csr_idx[k]]`` in ascending k,
    fp32, plain adds from +0 (pcaa_gather_sum_rows: no atomics, reproducible bit for bit on the host).  ``src`` fp32
    [n_src, ...] contiguous, ``csr_off`` int32 [n_dst + 1] and ``csr_idx`` int32 [nnz] on the device (``WindowRows.csr()``
    builds them on the host).  A row without contributors is zero; an index outside ``[0, n_src)`` is skipped and sets
    ``err_flag`` (int32 [1]).  -> fp32 [n_dst, ...]"""
    if not (isinstance(src, torch.Tensor) and src.is_cuda and src.is_contiguous() and src.dim() >= 2
            and src.dtype == torch.float32):
        raise RuntimeError("gather_sum_rows: src must be a contiguous float32 tensor of rows on the HIP device (this "
                           "package has no CPU path)")
    _chk(csr_off, "gather_sum_rows.csr_off", torch.int32, 1)
    _chk(csr_idx, "gather_sum_rows.csr_idx", torch.int32, 1)
    n_dst, nnz = csr_off.numel() - 1, csr_idx.numel()
    row_words = src[0].numel() if src.shape[0] else int(torch.Size(src.shape[1:]).numel())
    if n_dst < 0 or row_words < 1 or src.shape[0] < 1:
        raise ValueError(f"gather_sum_rows: needs csr_off [n_dst + 1] and at least one source row of at least one word; got "
                         f"csr_off {tuple(csr_off.shape)}, src {tuple(src.shape)}")
    shape = (n_dst,) + tuple(src.shape[1:])
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=src.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or not out.is_cuda:
        raise ValueError("gather_sum_rows: out does not match")
    if err_flag is not None:
        _chk(err_flag, "gather_sum_rows.err_flag", torch.int32)
    if n_dst:
        _timed("gather_sum_rows_kernel", lambda: check(_lib.load().pcaa_gather_sum_rows(
            _p(src), src.shape[0], row_words, _p(csr_off), _p(csr_idx) if nnz else None, nnz, _p(out), n_dst,
            _p(err_flag), _s()), "pcaa_gather_sum_rows"), float(nnz * row_words), (nnz + n_dst) * row_words * 4)
    return out


def crop_overlap_vec_bytes(crops):
    """16 or 4: the load width pcaa_crop_overlap takes for this tensor."""
    _chk(crops, "crop_overlap.crops", torch.float32, 4)
    M, T, N, C = crops.shape
    return int(_lib.load().pcaa_crop_overlap_vec_bytes(_p(crops), T * N * C, N * C))


def crop_overlap(crops, hop):
    """crops: point-major [M, T, N, C] fp32 -> int32 [M - 1]: 1 where the first T - hop frames of crop i + 1 equal the last
    T - hop frames of crop i bit for bit (pcaa_crop_overlap).  M == 1: empty, no launch."""
    _chk(crops, "crop_overlap.crops", torch.float32, 4)
    M, T, N, C = crops.shape
    hop = int(hop)
    if M < 1 or not 1 <= hop <= T:
        raise ValueError(f"crop_overlap: needs M >= 1 and 1 <= hop <= T, got M={M} T={T} hop={hop}")
    same = torch.empty(M - 1, dtype=torch.int32, device=crops.device)
    if M > 1:
        check(_lib.load().pcaa_crop_overlap(_p(crops), T * N * C, N * C, M, T, hop, _p(same), _s()), "pcaa_crop_overlap")
    return same


class WindowRows:
    """The start rows of B windows of T rows in a frame-feature table, range-checked on the HOST copy of the plan they
    come from (the kernels trust them: pcaa_dtc_conv_fwd_win).  ``ring_rows`` > 0: the table is a ring of that many rows
    and a window may wrap.  ``segments`` > 0 (needs ``ring_rows``): the table is that many rings of ``ring_rows`` rows back
    to back (``table_rows == segments * ring_rows``), a start is an absolute table row and the window wraps inside the
    ring it starts in (pcaa_dtc_conv_fwd_seg: the rings of many live streams).  ``dev``: the same values already on the
    device (int32), else they are uploaded here."""
    __slots__ = ("host", "dev", "T", "table_rows", "ring_rows", "segments")

    def __init__(self, host, T, table_rows, ring_rows=0, device=None, dev=None, segments=0):
        import numpy as np
        host = np.ascontiguousarray(host, dtype=np.int64).reshape(-1)
        T, table_rows, ring_rows, segments = int(T), int(table_rows), int(ring_rows), int(segments)
        if segments < 0 or (segments and (ring_rows < T or table_rows != segments * ring_rows)):
            raise ValueError(f"WindowRows: segments={segments} needs ring_rows={ring_rows} >= T={T} and table_rows="
                             f"{table_rows} == segments * ring_rows")
        if ring_rows and not T <= ring_rows <= table_rows:
            raise ValueError(f"WindowRows: ring_rows={ring_rows} must lie in [T={T}, table_rows={table_rows}]")
        if host.size:
            lo, hi = int(host.min()), int(host.max())
            if lo < 0 or (hi >= table_rows if segments else hi >= ring_rows if ring_rows else hi + T > table_rows):
                raise ValueError(f"WindowRows: window starts {lo}..{hi} (T={T}) leave the table of {table_rows} rows"
                                 + (f" (ring of {ring_rows})" if ring_rows else ""))
        if dev is None:
            dev = torch.from_numpy(host.astype(np.int32)).to(device)
        elif dev.dtype != torch.int32 or dev.numel() != host.size or not dev.is_cuda or not dev.is_contiguous():
            raise ValueError("WindowRows: dev must be a contiguous int32 device tensor with one entry per window")
        self.host, self.dev, self.T, self.table_rows, self.ring_rows = host, dev, T, table_rows, ring_rows
        self.segments = segments

    def __len__(self):
        return self.host.size

    def slice(self, a, b):
        return WindowRows(self.host[a:b], self.T, self.table_rows, self.ring_rows, dev=self.dev[a:b], segments=self.segments)

    def row_index(self):
        """int64 [B*T] device: the table row of every (window, step), for the one-gather fallback"""
        t = torch.arange(self.T, device=self.dev.device, dtype=torch.int64)
        start = self.dev.to(torch.int64)[:, None]
        # one rule: a window wraps inside the ring it starts in (a flat table is one ring that no window leaves, a single
        # ring is segment 0)
        ring = self.ring_rows or self.table_rows or 1
        off = start % ring
        return (start - off + (off + t[None, :]) % ring).reshape(-1).contiguous()

    def row_index_host(self):
        """``row_index()`` from the host copy of the plan: numpy int64 [B*T], no device work"""
        import numpy as np
        t = np.arange(self.T, dtype=np.int64)
        start = self.host[:, None]
        ring = self.ring_rows or self.table_rows or 1
        off = start % ring
        return (start - off + (off + t[None, :]) % ring).reshape(-1)

    def csr(self):
        """The plan transposed, for ``gather_sum_rows`` (the adjoint of ``gather_frames(table, row_index())``): numpy
        ``(csr_off int32 [table_rows + 1], csr_idx int32 [B*T])`` -- table row u receives the window rows
        ``csr_idx[csr_off[u] : csr_off[u + 1]]`` (row ``b * T + t`` of the materialised windows), in ascending order."""
        import numpy as np
        idx = self.row_index_host()
        order = np.argsort(idx, kind="stable")
        off = np.zeros(self.table_rows + 1, dtype=np.int64)
        np.cumsum(np.bincount(idx, minlength=self.table_rows), out=off[1:])
        return off.astype(np.int32), order.astype(np.int32)


def scatter_rows(src, dst_row, dst, err_flag=None):
    """dst[dst_row[r]] = src[r] along dim 0, one launch (pcaa_scatter_rows): ``dst_row`` int32 [n] on the device, negative =
    skip the row, >= dst.shape[0] = skip it and set ``err_flag`` (int32 [1]).  Duplicate destinations are the caller's
    error.  Rows of whole 32-bit words; 16-byte copies where the row size and the alignment allow."""
    for t, name in ((src, "src"), (dst, "dst")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dim() == 2):
            raise RuntimeError(f"scatter_rows: {name} must be a contiguous 2-D tensor on the HIP device (this package has no "
                               "CPU path)")
    _chk(dst_row, "scatter_rows.dst_row", torch.int32, 1)
    if src.dtype != dst.dtype or src.shape[1] != dst.shape[1]:
        raise ValueError(f"scatter_rows: rows of src {tuple(src.shape)} {src.dtype} and dst {tuple(dst.shape)} {dst.dtype} differ")
    row_bytes = src.shape[1] * src.element_size()
    if row_bytes % 4 or row_bytes == 0:
        raise ValueError(f"scatter_rows: rows of {row_bytes} bytes are not a multiple of 4")
    n = dst_row.numel()
    if n > src.shape[0]:
        raise ValueError(f"scatter_rows: {n} destinations for {src.shape[0]} source rows")
    if err_flag is not None:
        _chk(err_flag, "scatter_rows.err_flag", torch.int32)
    if n and dst.shape[0]:
        check(_lib.load().pcaa_scatter_rows(_p(src), _p(dst_row), n, row_bytes // 4, _p(dst), dst.shape[0], _p(err_flag),
                                            _s()), "pcaa_scatter_rows")
    return dst


RAW_MAX_CARD = 1024       # PCAA_RAW_MAX_CARD / PCAA_RAW_MAX_POINTS of include/pcaa_hip.h
RAW_MAX_POINTS = 1024


def _raw_entry(base, points, offsets, N, C, pick, seed, frame_key, standardize, divide_by_std, pick_out, err_flag, keep,
               keep_min, keep_rule, augment, prep):
    """What the raw routes share: the preparation decided (``datasets.RawPrep``: built from the keywords, or ``prep``) and
    checked against the call before any tensor is looked at, the inputs checked, the frames' keys required where the
    preparation reads them -> ``(prep, n, N, C, launch)``: ``n`` frames under ``offsets``, and ``launch(window, outs)`` =
    ``pcaa_<base><prep.suffix>(points .., n, *window, pick .., divide_by_std, *outs, err_flag, stream, *prep.tail)``."""
    prep = RawPrep.of(keep, keep_min, keep_rule, augment, base, prep)
    prep.check(base, pick, C)
    if not isinstance(points, torch.Tensor) or points.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{base}.points: expected a float32 or float64 tensor")
    _chk(points, base + ".points", None, 2)
    _chk(offsets, base + ".offsets", torch.int32, 1)
    N, C, seed = int(N), int(C), int(seed)
    n = offsets.numel() - 1
    if points.shape[1] != 5 or n < 0 or not 1 <= N <= RAW_MAX_POINTS or not 1 <= C <= 5:
        raise ValueError(f"{base}: needs points [P, 5], offsets [n + 1], 1 <= N <= {RAW_MAX_POINTS}, 1 <= C <= 5; got "
                         f"points {tuple(points.shape)}, n={n}, N={N}, C={C}")
    if not -2 ** 63 <= seed < 2 ** 63:
        raise ValueError(f"{base}: the seed must fit 64 bits")

    def per_frame(t, name, width):
        _chk(t, f"{base}.{name}", torch.int32, 2)
        if tuple(t.shape) != (n, width):
            raise ValueError(f"{base}: {name} must be [{n}, {width}], got {tuple(t.shape)}")

    if pick is not None:
        per_frame(pick, "pick", N)
    keyed = prep.needs_keys(pick)
    if keyed and n:
        if frame_key is None:
            raise ValueError(f"{base}: without picks, and to augment, every frame needs its key (frame_key int32 [n, 2])")
        per_frame(frame_key, "frame_key", 2)
    if pick_out is not None:
        per_frame(pick_out, "pick_out", N)
    if err_flag is not None:
        _chk(err_flag, base + ".err_flag", torch.int32)
    head = (_p(points), int(points.dtype == torch.float64), points.shape[0], _p(offsets), n)
    mid = (_p(pick), _p(frame_key) if keyed else None, seed, N, C, int(bool(standardize)), int(bool(divide_by_std)))
    name = "pcaa_" + base + prep.suffix

    def launch(window, outs):
        check(getattr(_lib.load(), name)(*head, *window, *mid, *outs, _p(err_flag), _s(), *prep.tail), name)

    return prep, n, N, C, launch


def frames_from_raw(points, offsets, N, C, *, pick=None, seed=0, frame_key=None, standardize=True, divide_by_std=False,
                    n_out=None, pick_out=None, err_flag=None, keep=0, keep_min=None, keep_rule="first", augment=None,
                    prep=None):
    """Raw radar detections -> processed frames in one launch (pcaa_frames_from_raw): ``points`` [P, 5] fp32 or fp64 (x,
    y, z, doppler, linear power), ``offsets`` int32 [n + 1] (frame f owns rows ``offsets[f] .. offsets[f + 1] - 1``) ->
    fp32 ``[n_out, N, C]``, rows ``n .. n_out - 1`` zero (``n_out`` defaults to n).  ``pick`` int32 [n, N]: output point p
    of frame f is raw point ``pick[f, p]`` of that frame (``datasets.draw_picks``: the reference's draws); None: the
    kernel draws them from ``frame_key`` int32 [n, 2] and ``seed`` (``datasets.device_picks_host`` restates the draw).
    ``pick_out`` int32 [n, N]: receives the picks used.  A frame that cannot be processed (cardinality < 1 or >
    RAW_MAX_CARD, offsets outside the points, a pick outside the frame) comes back as zeros and sets ``err_flag`` (int32
    [1]); nothing is checked on the host.  ``keep`` / ``keep_min`` / ``keep_rule`` / ``augment``, or ``prep`` built from
    them: the frames thinned and moved first, by the same launch (``datasets.RawPrep``: pcaa_frames_from_raw_thin,
    pcaa_frames_from_raw_aug); neutral: the plain call."""
    _, n, N, C, launch = _raw_entry("frames_from_raw", points, offsets, N, C, pick, seed, frame_key, standardize,
                                    divide_by_std, pick_out, err_flag, keep, keep_min, keep_rule, augment, prep)
    n_out = n if n_out is None else int(n_out)
    if n_out < n:
        raise ValueError(f"frames_from_raw: needs n_out >= n, got n={n}, n_out={n_out}")
    out = torch.empty((n_out, N, C), dtype=torch.float32, device=points.device)
    if n_out:
        launch((), (_p(out), n_out, _p(pick_out)))
    return out


def crops_from_raw(points, offsets, start, T, N, C, *, pick=None, seed=0, frame_key=None, standardize=True,
                   divide_by_std=False, out=None, err_flag=None, keep=0, keep_min=None, keep_rule="first",
                   augment=None, prep=None):
    """A batch of crops straight from the packed detections of a whole store, one launch (pcaa_crops_from_raw):
    ``points`` [P, 5] fp32 or fp64 and ``offsets`` int32 [F + 1] over ALL F frames of the store, ``start`` int32 [B] the
    store index of each crop's first frame -> fp32 ``[B, T, N, C]``, ``out[b, t]`` bit-equal to the frame
    ``frames_from_raw`` writes for store frame ``start[b] + t`` under the same ``pick`` row (int32 [F, N]) or, without
    picks, ``frame_key`` row (int32 [F, 2]) and ``seed``.  Crops may overlap and repeat.  A frame that cannot be processed
    (the rule of ``frames_from_raw``) and a crop that leaves the store (``start[b] < 0`` or ``start[b] + T > F``) come back
    as zeros and set ``err_flag`` (int32 [1]); nothing is checked on the host.  ``out``: a [B, T, N, C] buffer to fill.
    ``keep`` / ``keep_min`` / ``keep_rule`` / ``augment`` or ``prep``: as in ``frames_from_raw`` (pcaa_crops_from_raw_thin,
    pcaa_crops_from_raw_aug), the same frames -- a track's augmentation draws are shared by its windows."""
    _, F, N, C, launch = _raw_entry("crops_from_raw", points, offsets, N, C, pick, seed, frame_key, standardize,
                                    divide_by_std, None, err_flag, keep, keep_min, keep_rule, augment, prep)
    _chk(start, "crops_from_raw.start", torch.int32, 1)
    T, B = int(T), start.numel()
    if T < 1 or B * T >= 2 ** 31:
        raise ValueError(f"crops_from_raw: needs T >= 1, B T < 2^31; got B={B}, T={T}")
    if out is None:
        out = torch.empty((B, T, N, C), dtype=torch.float32, device=points.device)
    else:
        _chk(out, "crops_from_raw.out", torch.float32, 4)
        if tuple(out.shape) != (B, T, N, C):
            raise ValueError(f"crops_from_raw: out must be [{B}, {T}, {N}, {C}], got {tuple(out.shape)}")
    if B:
        _timed("crops_from_raw_kernel", lambda: launch((_p(start), B, T), (_p(out),)), 0.0, B * T * N * C * 4)
    return out


UNIQUE_ROW_QUANTUM = 256  # rows of the compact table: whole 256-row GEMM tiles (pcaa_gemm_affine_elu, pcaa_gemm_split3)


def unique_table_rows(P, n, N, keep=0):
    """M of ``frames_from_raw_unique``: frame f owns min(card_f, N) rows, a bad frame one, so for ascending offsets the
    frames own at most min(P + n, n N) rows; thinned to at most ``keep`` detections (0: not), min(P + n, n min(N, keep));
    rounded up to whole GEMM tiles (at least one)."""
    return unique_chunk_rows(min(int(P) + int(n), int(n) * min(int(N), int(keep) or int(N))))


def frames_from_raw_unique(points, offsets, N, C, *, pick=None, seed=0, frame_key=None, standardize=True,
                           divide_by_std=False, M=None, pick_out=None, err_flag=None, keep=0, keep_min=None,
                           keep_rule="first", augment=None, prep=None):
    """``frames_from_raw`` without the padding (pcaa_frames_from_raw_unique; arguments as there) -> ``(rows [M, C] fp32,
    weight [M] fp32, u_off [n + 1] int32)``: rows ``u_off[f] .. u_off[f + 1] - 1`` hold frame f's distinct picked
    detections in order of first occurrence, each bit-equal to the row ``frames_from_raw`` writes for that pick, ``weight``
    how often it was picked.  Unused rows of a frame's ``min(card, N)`` and the rows from ``u_off[n]`` on are zero with
    weight 0; a bad frame is one zero row of weight N and sets ``err_flag``.  ``M`` defaults to ``unique_table_rows``.
    Two launches (the scan of ``u_off``, the rows); nothing comes back to the host.  Thinned
    (pcaa_frames_from_raw_unique_thin), frame f owns ``min(card, k_f, N)`` rows and ``M`` defaults to
    ``unique_table_rows(P, n, N, keep)``.  Augmented (pcaa_frames_from_raw_unique_aug), the noise is keyed by the raw
    detection, so the distinct rows, their weights and ``u_off`` are those without it and every row is the padded route's."""
    prep, n, N, C, launch = _raw_entry("frames_from_raw_unique", points, offsets, N, C, pick, seed, frame_key, standardize,
                                       divide_by_std, pick_out, err_flag, keep, keep_min, keep_rule, augment, prep)
    M = unique_table_rows(points.shape[0], n, N, prep.keep) if M is None else int(M)
    if not 1 <= M < 2 ** 31 or n * RAW_MAX_POINTS >= 2 ** 31:
        raise ValueError(f"frames_from_raw_unique: needs 1 <= M < 2^31 and n * {RAW_MAX_POINTS} < 2^31, got M={M}, n={n}")
    dev = points.device
    rows = torch.empty((M, C), dtype=torch.float32, device=dev)
    weight = torch.empty(M, dtype=torch.float32, device=dev)
    u_off = torch.empty(n + 1, dtype=torch.int32, device=dev)
    _timed("frames_from_raw_unique_kernel", lambda: launch((), (_p(rows), _p(weight), _p(u_off), M, _p(pick_out))), 0.0,
           points.shape[0] * 5 * points.element_size() + M * (C + 1) * 4)
    return rows, weight, u_off


SCENE_MAX_CLUSTERS = 64   # PCAA_SCENE_MAX_CLUSTERS of include/pcaa_hip.h


def _chk_rows5(t, name):
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{name}: expected a float32 or float64 tensor")
    _chk(t, name, None, 2)
    if t.shape[1] != 5 or t.shape[0] >= 2 ** 31:
        raise ValueError(f"{name}: needs [P, 5] with P < 2^31, got {tuple(t.shape)}")


def scene_cluster(points, offsets, eps2, wz2, wv2, min_points, max_clusters, err, zero_fill=True):
    """Density clustering of n scene frames in one launch (pcaa_scene_cluster): ``points`` [P, 5] fp32 or fp64 (x, y, z,
    doppler, linear power: ``datasets.pack_raw_frames``' layout), ``offsets`` int32 [n + 1] -> ``(label int32 [P],
    n_clusters int32 [n], cluster_count int32 [n, Cmax], centroid fp32 [n, Cmax, 4], grouped [P, 5], seg_off int32
    [n, Cmax + 1])``.  Neighbours: ``dx*dx + dy*dy + wz2*dz*dz + wv2*dv*dv <= eps2`` in fp64; core: ``>= min_points``
    neighbours, self included; clusters: components of the core points, border points with their nearest core neighbour,
    ids by lowest core index; noise -1 (``scene.cluster_host`` restates the rule bit for bit).  ``grouped`` holds every
    frame's rows cluster by cluster, then the noise; cluster c of frame f owns ``grouped[seg_off[f, c] : seg_off[f, c +
    1]]``.  ``err`` int32 [1] (required): bit 0 is set by a frame of more than RAW_MAX_CARD detections or with offsets
    outside the points (zero clusters), bit 1 by a frame with more than ``max_clusters`` clusters (the rest is noise);
    nothing is checked on the host.  Rows that no frame owns are zero (``label``: -1); ``zero_fill=False`` leaves them
    unwritten and saves the two fills (the live front end: no ``seg_off`` entry ever points at such a row)."""
    _chk_rows5(points, "scene_cluster.points")
    _chk(offsets, "scene_cluster.offsets", torch.int32, 1)
    _chk(err, "scene_cluster.err", torch.int32)
    n, Cmax, min_points = offsets.numel() - 1, int(max_clusters), int(min_points)
    eps2, wz2, wv2 = float(eps2), float(wz2), float(wv2)
    if n < 0 or not 1 <= Cmax <= SCENE_MAX_CLUSTERS or min_points < 1 or err.numel() < 1:
        raise ValueError(f"scene_cluster: needs offsets [n + 1], 1 <= max_clusters <= {SCENE_MAX_CLUSTERS}, min_points >= 1; "
                         f"got n={n}, max_clusters={Cmax}, min_points={min_points}")
    if not all(0.0 <= v < float("inf") for v in (eps2, wz2, wv2)):
        raise ValueError(f"scene_cluster: eps2, wz2 and wv2 must be finite and >= 0, got {eps2}, {wz2}, {wv2}")
    dev, P = points.device, points.shape[0]
    if zero_fill:
        label, grouped = torch.full((P,), -1, dtype=torch.int32, device=dev), torch.zeros_like(points)
    else:
        label, grouped = torch.empty((P,), dtype=torch.int32, device=dev), torch.empty_like(points)
    n_clusters = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.empty((n, Cmax), dtype=torch.int32, device=dev)
    centroid = torch.empty((n, Cmax, 4), dtype=torch.float32, device=dev)
    seg_off = torch.empty((n, Cmax + 1), dtype=torch.int32, device=dev)
    if n:
        _timed("scene_cluster_kernel", lambda: check(_lib.load().pcaa_scene_cluster(
            _p(points), int(points.dtype == torch.float64), P, _p(offsets), n, eps2, wz2, wv2, min_points, Cmax, _p(label),
            _p(n_clusters), _p(count), _p(centroid), _p(grouped), _p(seg_off), _p(err), _s()), "pcaa_scene_cluster"),
            0.0, 2 * P * 5 * points.element_size())
    return label, n_clusters, count, centroid, grouped, seg_off


def gather_segments(src, seg_start, out_off, rows, err_flag=None, zero_fill=True):
    """``out[out_off[o] : out_off[o + 1]] = src[seg_start[o] : seg_start[o] + out_off[o + 1] - out_off[o]]`` for the M
    segments, one launch (pcaa_gather_segments): ``src`` [P, 5] fp32 or fp64, ``seg_start`` int32 [M] and ``out_off``
    int32 [M + 1] on the device, ``rows`` = ``out_off[M]`` as the host knows it -> ``out`` [rows, 5] in ``src``'s dtype:
    with ``offsets = out_off`` the layout ``frames_from_raw`` and ``push_raw`` take.  A segment that leaves the source or
    the output is skipped (its rows stay zero; unwritten with ``zero_fill=False``) and sets ``err_flag`` (int32 [1])."""
    _chk_rows5(src, "gather_segments.src")
    _chk(seg_start, "gather_segments.seg_start", torch.int32, 1)
    _chk(out_off, "gather_segments.out_off", torch.int32, 1)
    M, rows = seg_start.numel(), int(rows)
    if out_off.numel() != M + 1 or not 0 <= rows < 2 ** 31:
        raise ValueError(f"gather_segments: needs seg_start [M], out_off [M + 1] and 0 <= rows < 2^31; got M={M}, out_off "
                         f"{tuple(out_off.shape)}, rows={rows}")
    if err_flag is not None:
        _chk(err_flag, "gather_segments.err_flag", torch.int32)
    out = (torch.zeros if zero_fill else torch.empty)((rows, 5), dtype=src.dtype, device=src.device)
    if M:
        check(_lib.load().pcaa_gather_segments(_p(src), int(src.dtype == torch.float64), src.shape[0], _p(seg_start),
                                               _p(out_off), M, _p(out), rows, _p(err_flag), _s()), "pcaa_gather_segments")
    return out


def _chk_padded_frames(frames, who):
    """what frames_unique_offsets and frames_unique refuse before any launch -> (n, N, C)"""
    _chk(frames, who + ".frames", torch.float32, 3)
    n, N, C = frames.shape
    if not 1 <= N <= RAW_MAX_POINTS or not 1 <= C <= 5 or n * N >= 2 ** 31:
        raise ValueError(f"{who}: needs frames [n, N, C] with 1 <= N <= {RAW_MAX_POINTS}, 1 <= C <= 5, n N < 2^31; got "
                         f"{tuple(frames.shape)}")
    return n, N, C


def frames_unique_offsets(frames):
    """Padded frames -> where their distinct rows go (pcaa_frames_unique_offsets): ``frames`` fp32 contiguous point-major
    [n, N, C] -> ``u_off`` int32 [n + 1] on the device, the exclusive scan of the number of distinct rows per frame (rows
    are equal iff their C words are equal as bits).  Two launches whatever n is; nothing comes back to the host."""
    n, N, C = _chk_padded_frames(frames, "frames_unique_offsets")
    u_off = torch.empty(n + 1, dtype=torch.int32, device=frames.device)
    _timed("frames_unique_count_kernel", lambda: check(_lib.load().pcaa_frames_unique_offsets(
        _p(frames), n, N, C, _p(u_off), _s()), "pcaa_frames_unique_offsets"), 0.0, n * N * C * 4 + (n + 1) * 8)
    return u_off


def frames_unique(frames, u_off, a=0, b=None, M=None, out=None, err_flag=None):
    """The compact table of frames ``a .. b - 1`` (pcaa_frames_unique; ``u_off`` from ``frames_unique_offsets`` of the same
    frames) -> ``(rows [M, C] fp32, weight [M] fp32, seg_off [b - a + 1] int32)``, the contract of
    ``frames_from_raw_unique``: frame f owns rows ``seg_off[f - a] .. seg_off[f - a + 1] - 1``, its distinct rows in order
    of first occurrence, bit-equal to the source rows, ``weight`` the multiplicity (a frame's weights add up to N); the
    rows behind the last frame are zero with weight 0.  ``M`` defaults to the chunk's rows (``unique_chunk_rows``) and must
    be a multiple of UNIQUE_ROW_QUANTUM; without it (and without ``out``) two entries of ``u_off`` are read back, so a
    caller that must not wait passes it (``plan_unique_chunks`` gives it).  ``out=(rows, weight)``: the caller's buffers.  A frame whose given segment
    is not its own (a ``u_off`` of other frames, an ``M`` too small) writes nothing and sets ``err_flag`` (int32 [1])."""
    n, N, C = _chk_padded_frames(frames, "frames_unique")
    _chk(u_off, "frames_unique.u_off", torch.int32, 1)
    a, b = int(a), n if b is None else int(b)
    if u_off.numel() != n + 1 or not 0 <= a <= b <= n:
        raise ValueError(f"frames_unique: needs u_off [n + 1 = {n + 1}] and 0 <= a <= b <= n, got u_off "
                         f"{tuple(u_off.shape)}, a={a}, b={b}")
    if M is None and out is not None:
        M = out[0].shape[0]
    if M is None:
        lo, hi = u_off[[a, b]].tolist()
        M = unique_chunk_rows(hi - lo)
    M = int(M)
    if not 1 <= M < 2 ** 31 or M % UNIQUE_ROW_QUANTUM:
        raise ValueError(f"frames_unique: M must be a positive multiple of {UNIQUE_ROW_QUANTUM} below 2^31, got {M}")
    if err_flag is not None:
        _chk(err_flag, "frames_unique.err_flag", torch.int32)
    dev = frames.device
    if out is None:
        rows = torch.empty((M, C), dtype=torch.float32, device=dev)
        weight = torch.empty(M, dtype=torch.float32, device=dev)
    else:
        rows, weight = out
        _chk(rows, "frames_unique.out[0]", torch.float32, 2)
        _chk(weight, "frames_unique.out[1]", torch.float32, 1)
        if tuple(rows.shape) != (M, C) or weight.numel() != M:
            raise ValueError(f"frames_unique: out must be ([{M}, {C}], [{M}]), got {tuple(rows.shape)}, {tuple(weight.shape)}")
    seg_off = torch.empty(b - a + 1, dtype=torch.int32, device=dev)
    _timed("frames_unique_kernel", lambda: check(_lib.load().pcaa_frames_unique(
        _p(frames), n, N, C, _p(u_off), a, b, _p(rows), _p(weight), M, _p(seg_off), _p(err_flag), _s()),
        "pcaa_frames_unique"), 0.0, (b - a) * N * C * 4 + M * (C + 1) * 4)
    return rows, weight, seg_off


def unique_chunk_rows(need):
    """rows of a compact table that holds ``need`` distinct rows: whole GEMM tiles, at least one"""
    return max((int(need) + UNIQUE_ROW_QUANTUM - 1) // UNIQUE_ROW_QUANTUM, 1) * UNIQUE_ROW_QUANTUM


def plan_unique_chunks(u_off_host, budget_rows):
    """Host plan of the chunks of a padding-free pass: ``u_off_host`` [n + 1] (the host copy of ``frames_unique_offsets``),
    ``budget_rows`` >= the largest frame -> ``[(a, b, M)]``: consecutive frame ranges that cover 0 .. n, each as long as
    its distinct rows total at most ``budget_rows``; ``M = unique_chunk_rows`` of that total.  n == 0: no chunk."""
    import numpy as np
    u = np.asarray(u_off_host, dtype=np.int64).reshape(-1)
    n, budget = u.size - 1, int(budget_rows)
    if n < 0 or (n and (u[0] != 0 or (np.diff(u) < 0).any())):
        raise ValueError("plan_unique_chunks: needs ascending offsets [n + 1] that start at 0")
    if n and int(np.diff(u).max()) > budget:
        raise ValueError(f"plan_unique_chunks: a frame of {int(np.diff(u).max())} rows exceeds the budget of {budget}")
    chunks, a = [], 0
    while a < n:
        b = int(np.searchsorted(u, u[a] + budget, side="right")) - 1      # the last b with u[b] - u[a] <= budget
        b = min(max(b, a + 1), n)
        chunks.append((a, b, unique_chunk_rows(int(u[b] - u[a]))))
        a = b
    return chunks


def segment_weighted_mean(a, weight, u_off, N, scale=None, shift=None, err_flag=None):
    """``out[f] = (1 / N) sum_{r in [u_off[f], u_off[f + 1])} weight[r] * v(a[r])`` (pcaa_segment_weighted_mean): ``a``
    [M, ch] bf16 or fp32, ``weight`` fp32 [M], ``u_off`` int32 [n + 1] -> fp32 [n, ch].  ``v`` is the identity, or with
    ``scale`` / ``shift`` fp32 [ch] ``ELU(a * scale + shift)`` (``a`` a pre-BatchNorm y).  fp32 accumulation in a fixed
    order: a frame's result does not depend on n.  ``ch % 8 == 0``.  A segment outside ``[0, M]`` comes back as zeros and
    sets ``err_flag`` (int32 [1])."""
    _chk(a, "segment_weighted_mean.a", None, 2)
    if a.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"segment_weighted_mean.a: expected float32 or bfloat16, got {a.dtype}")
    _chk(weight, "segment_weighted_mean.weight", torch.float32, 1)
    _chk(u_off, "segment_weighted_mean.u_off", torch.int32, 1)
    M, ch = a.shape
    n, N = u_off.numel() - 1, int(N)
    if weight.numel() != M:
        raise ValueError(f"segment_weighted_mean: weight must be [{M}] (one per row of a), got {tuple(weight.shape)}")
    if ch < 8 or ch % 8 or n < 0 or N < 1:
        raise ValueError(f"segment_weighted_mean: needs ch % 8 == 0, u_off [n + 1], N >= 1; got ch={ch}, n={n}, N={N}")
    if (scale is None) != (shift is None):
        raise ValueError("segment_weighted_mean: scale and shift come together")
    if scale is not None:
        for t, name in ((scale, "scale"), (shift, "shift")):
            _chk(t, "segment_weighted_mean." + name, torch.float32, 1)
            if t.numel() != ch:
                raise ValueError(f"segment_weighted_mean: {name} must be [{ch}], got {tuple(t.shape)}")
    if err_flag is not None:
        _chk(err_flag, "segment_weighted_mean.err_flag", torch.int32)
    out = torch.empty((n, ch), dtype=torch.float32, device=a.device)
    if n:
        _timed("segment_weighted_mean_kernel", lambda: check(_lib.load().pcaa_segment_weighted_mean(
            _p(a), _dt(a), ch, _p(weight), _p(u_off), n, M, ch, N, _p(scale), _p(shift), _p(out), _p(err_flag), _s()),
            "pcaa_segment_weighted_mean"), 2.0 * M * ch, M * ch * a.element_size() + n * ch * 4)
    return out


def segment_weighted_mean_bwd(dpool, y, weight, u_off, N, scale, shift, mean, rstd, out=None, err_flag=None):
    """Backward of ``segment_weighted_mean(y, weight, u_off, N, scale, shift)`` w.r.t. the pre-BatchNorm ``y``
    (pcaa_segment_weighted_mean_bwd): for row r of segment f ``dy[r] = scale * dpool[f] * (weight[r] / N) * ELU'(y[r] *
    scale + shift)`` in y's dtype, and the statistics {sum dz, sum dz*xhat} for bn_eval_bwd_finalize (``mean``, ``rstd``
    from bn_eval_moments).  ``dpool`` fp32 [n, ch], ``y`` [M, ch] bf16 or fp32 (a column view with a leading dimension
    that is a multiple of 8 is taken as is; ``out`` then needs the same strides).  Rows that no valid segment owns come
    out as zeros; a segment outside ``[0, M]`` contributes nothing and sets ``err_flag`` (int32 [1]).  Valid segments must be
    disjoint (non-decreasing offsets are; an overlap needs a segment that runs backwards, which sets the flag: discard the
    result then).  -> (dy, stats)"""
    if not (isinstance(y, torch.Tensor) and y.is_cuda and y.dim() == 2 and y.stride(1) == 1):
        raise RuntimeError("segment_weighted_mean_bwd.y: must be a 2-D tensor on the HIP device with unit column stride "
                           "(this package has no CPU path)")
    if y.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"segment_weighted_mean_bwd.y: expected float32 or bfloat16, got {y.dtype}")
    M, ch = y.shape
    lda = y.stride(0) if M > 1 else ch
    _chk(dpool, "segment_weighted_mean_bwd.dpool", torch.float32, 2)
    _chk(weight, "segment_weighted_mean_bwd.weight", torch.float32, 1)
    _chk(u_off, "segment_weighted_mean_bwd.u_off", torch.int32, 1)
    n, N = u_off.numel() - 1, int(N)
    if weight.numel() != M:
        raise ValueError(f"segment_weighted_mean_bwd: weight must be [{M}] (one per row of y), got {tuple(weight.shape)}")
    if ch < 8 or ch % 8 or n < 0 or N < 1 or lda < ch or lda % 8:
        raise ValueError(f"segment_weighted_mean_bwd: needs ch % 8 == 0, a leading dimension >= ch that is a multiple of 8, "
                         f"u_off [n + 1], N >= 1; got ch={ch}, lda={lda}, n={n}, N={N}")
    if tuple(dpool.shape) != (n, ch):
        raise ValueError(f"segment_weighted_mean_bwd: dpool must be [{n}, {ch}], got {tuple(dpool.shape)}")
    for t, name in ((scale, "scale"), (shift, "shift"), (mean, "mean"), (rstd, "rstd")):
        _chk(t, "segment_weighted_mean_bwd." + name, torch.float32, 1)
        if t.numel() != ch:
            raise ValueError(f"segment_weighted_mean_bwd: {name} must be [{ch}], got {tuple(t.shape)}")
    if err_flag is not None:
        _chk(err_flag, "segment_weighted_mean_bwd.err_flag", torch.int32)
    if out is None:
        dy = torch.empty_like(y) if y.is_contiguous() else torch.empty_strided((M, ch), (lda, 1), dtype=y.dtype, device=y.device)
    else:
        dy = out
        if not (isinstance(dy, torch.Tensor) and dy.is_cuda and dy.shape == y.shape and dy.dtype == y.dtype
                and dy.stride(1) == 1 and (M <= 1 or dy.stride(0) == lda)):
            raise ValueError("segment_weighted_mean_bwd: out must have y's shape, dtype and strides")
    stats = new_stats(ch, y.device)
    if n:
        _timed("segment_weighted_mean_bwd_kernel", lambda: check(_lib.load().pcaa_segment_weighted_mean_bwd(
            _p(dpool), _p(y), _p(dy), _dt(y), lda, _p(weight), _p(u_off), n, M, ch, N, _p(scale), _p(shift), _p(mean),
            _p(rstd), _p(stats), NREP, _p(err_flag), _s()), "pcaa_segment_weighted_mean_bwd"),
            8.0 * M * ch, 3 * M * ch * y.element_size() + n * ch * 4)
    else:
        dy.zero_()
    return dy, stats


def _tick_io(who, logits, sup_fv, means, run_start, win_stream, win_j, vote_pos, n_votes, k, hist_lik, hist_lab, lab_name):
    """the tensors of one tick checked for ``who`` (``stream_score`` / ``stream_score_gallery``) and its outputs allocated
    -> (nw, K, D, k, n_votes, n_runs, labels [nw] int64, lik [nw] f64, votes [n_votes] int64)"""
    _chk(logits, who + ".logits", torch.float32, 2)
    _chk(sup_fv, who + ".sup_fv", torch.float32, 2)
    _chk(means, who + ".means", torch.float32, 2)
    _chk(hist_lik, who + ".hist_lik", torch.float64, 2)
    _chk(hist_lab, f"{who}.{lab_name}", torch.int64, 2)
    for t, name in ((run_start, "run_start"), (win_stream, "win_stream"), (win_j, "win_j"), (vote_pos, "vote_pos")):
        _chk(t, f"{who}.{name}", torch.int32, 1)
    nw, K = logits.shape
    D = sup_fv.shape[1]
    k, n_votes, n_runs = int(k), int(n_votes), run_start.numel() - 1
    if (sup_fv.shape[0] != nw or means.shape[1] != D or win_stream.numel() != nw or win_j.numel() != nw
            or vote_pos.numel() != nw or k < 1 or tuple(hist_lik.shape) != tuple(hist_lab.shape)
            or hist_lik.shape[1] != k or not 0 <= n_votes <= nw or not (1 <= n_runs <= nw or nw == 0)):
        raise ValueError(f"{who}: shapes do not describe one tick")
    dev = logits.device
    return (nw, K, D, k, n_votes, n_runs, torch.empty(nw, dtype=torch.int64, device=dev),
            torch.empty(nw, dtype=torch.float64, device=dev), torch.empty(n_votes, dtype=torch.int64, device=dev))


def stream_score(logits, sup_fv, means, run_start, win_stream, win_j, vote_pos, n_votes, threshold, k, n_labels,
                 n_classes, hist_lik, hist_pred):
    """One tick of many live streams in one launch (pcaa_stream_score) -> (preds [nw] int64, lik [nw] f64, votes [n_votes]
    int64).  ``run_start`` [n_runs + 1], ``win_stream`` / ``win_j`` / ``vote_pos`` [nw]: int32 on the device, from
    ``inference.plan_tick`` (a stream's windows are one contiguous ascending run).  ``hist_lik`` f64 / ``hist_pred`` int64
    [max_streams, k]: the streams' incomplete vote groups, read and updated in place."""
    nw, K, D, k, n_votes, n_runs, preds, lik, votes = _tick_io(
        "stream_score", logits, sup_fv, means, run_start, win_stream, win_j, vote_pos, n_votes, k, hist_lik, hist_pred,
        "hist_pred")
    if nw:
        check(_lib.load().pcaa_stream_score(
            _p(logits), _p(sup_fv), _p(means), _p(run_start), n_runs, _p(win_stream), _p(win_j), _p(vote_pos), nw, K, D,
            means.shape[0], ctypes.c_double(float(threshold)), k, int(n_labels), int(n_classes), _p(hist_lik),
            _p(hist_pred), hist_lik.shape[0], _p(preds), _p(lik), _p(votes) if n_votes else None, n_votes, _s()),
            "pcaa_stream_score")
    return preds, lik, votes


# ------------------------------------------------------------------ run-time enrolment (csrc/gallery.hip)
def _chk_gallery(who, sums, counts, centroids, E, D):
    """the three buffers of a gallery (``gallery.Gallery``) and its high-water mark against an embedding width"""
    _chk(centroids, who + ".centroids", torch.float32, 2)
    _chk(counts, who + ".counts", torch.int32, 1)
    if sums is not None:
        _chk(sums, who + ".sums", torch.float64, 2)
        if tuple(sums.shape) != tuple(centroids.shape):
            raise ValueError(f"{who}: sums {tuple(sums.shape)} and centroids {tuple(centroids.shape)} differ")
    E_max = centroids.shape[0]
    if E_max < 1 or counts.numel() != E_max or centroids.shape[1] != D or not 0 <= int(E) <= E_max:
        raise ValueError(f"{who}: needs centroids [E_max, {D}], counts [E_max] and 0 <= E <= E_max; got "
                         f"{tuple(centroids.shape)}, {tuple(counts.shape)}, E = {E}")
    return E_max


def gallery_accumulate(fv, slot, sums, counts, centroids, rows=None, err_flag=None):
    """Add rows of ``fv`` fp32 [n, D] to slot ``slot`` of a gallery in one launch (pcaa_gallery_accumulate): ``sums[slot] +=
    fv[rows[i]]`` in the order of ``rows`` (int32 [m] on the device; None: every row of ``fv`` in order) with plain fp64
    adds, then the slot's count and its centroid ``float32(sum / count)``.  An index outside ``[0, n)`` is skipped and
    sets ``err_flag`` (int32 [1]).  Nothing comes back to the host."""
    _chk(fv, "gallery_accumulate.fv", torch.float32, 2)
    n, D = fv.shape
    E_max = _chk_gallery("gallery_accumulate", sums, counts, centroids, 0, D)
    if rows is not None:
        _chk(rows, "gallery_accumulate.rows", torch.int32, 1)
    m = n if rows is None else rows.numel()
    if err_flag is not None:
        _chk(err_flag, "gallery_accumulate.err_flag", torch.int32, 1)
    if n < 1 or m < 1 or n >= 2 ** 31 or not 0 <= int(slot) < E_max:
        raise ValueError(f"gallery_accumulate: needs at least one row to add and a slot in 0..{E_max - 1}; got fv "
                         f"{tuple(fv.shape)}, {m} rows, slot {slot}")
    check(_lib.load().pcaa_gallery_accumulate(_p(fv), n, D, _p(rows), m, int(slot), E_max, _p(sums), _p(counts),
                                              _p(centroids), _p(err_flag), _s()), "pcaa_gallery_accumulate")


def gallery_score(sup_fv, preds, means, centroids, counts, E, n_labels):
    """Windows against the prior means AND a gallery (pcaa_gallery_score) -> (lik f64 [B], labels int64 [B], near int32
    [B]): ``lik = (sum over the Kc prior modes + sum over the live slots) / Kc``, ``near`` the closest mode (prior modes
    first), ``labels = preds`` where a prior mode is closest, else ``n_labels + 1 + slot``.  ``E``: slots ``0 .. E - 1`` are
    scanned.  With no live slot ``lik`` has the bits of ``inference.joint_likelihood``."""
    _chk(sup_fv, "gallery_score.sup_fv", torch.float32, 2)
    _chk(preds, "gallery_score.preds", torch.int64, 1)
    _chk(means, "gallery_score.means", torch.float32, 2)
    B, D = sup_fv.shape
    _chk_gallery("gallery_score", None, counts, centroids, E, D)
    if preds.numel() != B or means.shape[1] != D or means.shape[0] < 1 or int(n_labels) < 1:
        raise ValueError("gallery_score: needs one prediction per window, means [Kc, D] with Kc >= 1 and n_labels >= 1")
    dev = sup_fv.device
    lik = torch.empty(B, dtype=torch.float64, device=dev)
    labels = torch.empty(B, dtype=torch.int64, device=dev)
    near = torch.empty(B, dtype=torch.int32, device=dev)
    if B:
        check(_lib.load().pcaa_gallery_score(_p(sup_fv), _p(preds), _p(means), B, means.shape[0], D, _p(centroids),
                                             _p(counts), int(E), int(n_labels), _p(lik), _p(labels), _p(near), _s()),
              "pcaa_gallery_score")
    return lik, labels, near


def gallery_vote(lik, labels, threshold, k, n_labels):
    """``inference.k_vote`` over the extended labels of ``gallery_score`` (pcaa_gallery_kvote): groups of k consecutive
    windows (a trailing partial group is dropped) -> [n // k] int64, the most frequent label of a known group (lowest on
    ties), ``n_labels`` for the others."""
    _chk(lik, "gallery_vote.lik", torch.float64, 1)
    _chk(labels, "gallery_vote.labels", torch.int64, 1)
    k = int(k)
    if k < 1 or labels.numel() != lik.numel() or int(n_labels) < 1:
        raise ValueError("gallery_vote: needs k >= 1, n_labels >= 1 and one label per likelihood")
    nwin = lik.numel() // k
    out = torch.empty(nwin, dtype=torch.int64, device=lik.device)
    if nwin:
        check(_lib.load().pcaa_gallery_kvote(_p(lik), _p(labels), ctypes.c_double(float(threshold)), k, int(n_labels), nwin,
                                             _p(out), _s()), "pcaa_gallery_kvote")
    return out


def stream_score_gallery(logits, sup_fv, means, run_start, win_stream, win_j, vote_pos, n_votes, threshold, k, n_labels,
                         centroids, counts, E, hist_lik, hist_label, fv_hist=None):
    """``stream_score`` with the score of ``gallery_score`` and the vote of ``gallery_vote``, still one launch
    (pcaa_stream_score_gallery) -> (labels [nw] int64, lik [nw] f64, near [nw] int32, votes [n_votes] int64).
    ``hist_label`` int64 [max_streams, k] keeps the extended labels as they were stored.  ``fv_hist`` fp32
    [max_streams * H, D] (optional): window j of stream s also leaves its ``sup_fv`` in row ``s * H + j % H``."""
    nw, K, D, k, n_votes, n_runs, labels, lik, votes = _tick_io(
        "stream_score_gallery", logits, sup_fv, means, run_start, win_stream, win_j, vote_pos, n_votes, k, hist_lik,
        hist_label, "hist_label")
    _chk_gallery("stream_score_gallery", None, counts, centroids, E, D)
    H = 0
    if fv_hist is not None:
        _chk(fv_hist, "stream_score_gallery.fv_hist", torch.float32, 2)
        H = fv_hist.shape[0] // hist_lik.shape[0]
        if H < 1 or fv_hist.shape[0] != H * hist_lik.shape[0] or fv_hist.shape[1] != D:
            raise ValueError(f"stream_score_gallery: fv_hist must be [max_streams * H, {D}] with H >= 1, got "
                             f"{tuple(fv_hist.shape)} for {hist_lik.shape[0]} streams")
    near = torch.empty(nw, dtype=torch.int32, device=logits.device)
    if nw:
        check(_lib.load().pcaa_stream_score_gallery(
            _p(logits), _p(sup_fv), _p(means), _p(run_start), n_runs, _p(win_stream), _p(win_j), _p(vote_pos), nw, K, D,
            means.shape[0], ctypes.c_double(float(threshold)), k, int(n_labels), _p(centroids), _p(counts), int(E),
            _p(hist_lik), _p(hist_label), hist_lik.shape[0], _p(fv_hist), H, _p(labels), _p(lik), _p(near),
            _p(votes) if n_votes else None, n_votes, _s()), "pcaa_stream_score_gallery")
    return labels, lik, near, votes


def dtc_im2col(a, B, T, Cin, d):
    _chk(a, "im2col.a", torch.float32, 2)
    col = torch.empty((B * T, 3 * Cin), dtype=torch.float32, device=a.device)
    check(_lib.load().pcaa_dtc_im2col(_p(a), _p(col), B, T, Cin, d, _s()), "pcaa_dtc_im2col")
    return col


def dtc_col2im(dcol, B, T, Cin, d):
    _chk(dcol, "col2im.dcol", torch.float32, 2)
    da = torch.empty((B * T, Cin), dtype=torch.float32, device=dcol.device)
    check(_lib.load().pcaa_dtc_col2im(_p(dcol), _p(da), B, T, Cin, d, _s()), "pcaa_dtc_col2im")
    return da


# ------------------------------------------------------------------ losses
def chamfer(preds, gts, want_grad, grad_scale=1.0, grad_per_b=None):
    """preds/gts logical [B,C,T,N] fp32 with arbitrary strides.  Returns
    (frame_loss [B,T], dpreds contiguous [B,C,T,N] or None)."""
    for t, nm in ((preds, "preds"), (gts, "gts")):
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4:
            raise RuntimeError(f"chamfer: {nm} must be a 4-D float32 tensor on the HIP device")
    if preds.shape != gts.shape:
        raise ValueError("chamfer: shape mismatch")
    B, C, T, N = preds.shape
    fl = torch.empty((B, T), dtype=torch.float32, device=preds.device)
    dp = torch.empty((B, C, T, N), dtype=torch.float32, device=preds.device) if want_grad else None
    ds = dp.stride() if want_grad else (0, 0, 0, 0)
    ps, gs = preds.stride(), gts.stride()
    check(_lib.load().pcaa_chamfer_fwd_bwd(_p(preds), ps[0], ps[1], ps[2], ps[3], _p(gts), gs[0], gs[1], gs[2], gs[3],
                                           B, T, N, C, _p(fl), _p(dp), ds[0], ds[1], ds[2], ds[3],
                                           float(grad_scale), _p(grad_per_b), _s()), "pcaa_chamfer_fwd_bwd")
    return fl, dp


def cross_entropy(logits, target=None, want_loss=True, want_grad=False, grad_scale=1.0, want_preds=False,
                  err_flag=None):
    """``err_flag`` (device int32[1]): the kernel raises it when a target is outside [0,K) and the caller checks
    it when convenient (the trainer: once per epoch).  Without it the targets are range-checked here, on the
    host (one synchronisation) -- torch's CrossEntropyLoss raises on such a label, so must this."""
    _chk(logits, "ce.logits", torch.float32, 2)
    B, K = logits.shape
    if target is not None:
        _chk(target, "ce.target", torch.int64, 1)
        if target.shape[0] != B:
            raise ValueError(f"cross_entropy: {target.shape[0]} targets for {B} rows of logits")
        if err_flag is None:
            lo, hi = int(target.min().item()), int(target.max().item())
            if lo < 0 or hi >= K:
                raise IndexError(f"cross_entropy: target {lo if lo < 0 else hi} is out of bounds for {K} classes")
        else:
            _chk(err_flag, "ce.err_flag", torch.int32)
    dev = logits.device
    loss = torch.empty((), dtype=torch.float32, device=dev) if (want_loss and target is not None) else None
    dl = torch.empty_like(logits) if want_grad else None
    pr = torch.empty(B, dtype=torch.int64, device=dev) if want_preds else None
    check(_lib.load().pcaa_cross_entropy(_p(logits), _p(target), B, K, _p(loss), _p(dl), float(grad_scale), _p(pr),
                                         _p(err_flag) if target is not None else None, _s()),
          "pcaa_cross_entropy")
    return loss, dl, pr


# ------------------------------------------------------------------ OR-CED heads (csrc/orced.hip)
def orced_heads_fwd(x4, Wmu, bmu, Wlv, blv, eps, Wc, bc):
    """-> (logits [B,K], sup_fv, mu, logvar [B,L])"""
    for t, nm in ((x4, "x4"), (Wmu, "Wmu"), (Wlv, "Wlv"), (eps, "eps"), (Wc, "Wc")):
        _chk(t, f"orced_heads_fwd.{nm}", torch.float32, 2)
    B, d_in = x4.shape
    L, K = Wmu.shape[0], Wc.shape[0]
    lib = _lib.load()
    if (tuple(Wmu.shape) != (L, d_in) or tuple(Wlv.shape) != (L, d_in) or tuple(eps.shape) != (B, L)
            or tuple(Wc.shape) != (K, L) or not lib.pcaa_orced_heads_supported(B, K, d_in, L)):
        raise ValueError("orced_heads_fwd: unsupported shapes")
    mu = torch.empty((B, L), dtype=torch.float32, device=x4.device)
    logvar, sup = torch.empty_like(mu), torch.empty_like(mu)
    logits = torch.empty((B, K), dtype=torch.float32, device=x4.device)
    check(lib.pcaa_orced_heads_fwd(_p(x4), _p(Wmu), _p(bmu), _p(Wlv), _p(blv), _p(eps), _p(Wc), _p(bc), _p(mu), _p(logvar),
                                   _p(sup), _p(logits), B, K, d_in, L, _s()), "pcaa_orced_heads_fwd")
    return logits, sup, mu, logvar


def orced_heads_bwd(x4, eps, logvar, sup, Wmu, Wlv, Wc, d_logits, d_sup, d_mu, d_logvar, need_dx=True):
    """-> (dx4 or None, dWmu, dbmu, dWlv, dblv, dWc, dbc)"""
    B, d_in = x4.shape
    L, K = Wmu.shape[0], Wc.shape[0]
    dev = x4.device
    for t in (d_logits, d_sup, d_mu, d_logvar):
        if t is not None:
            _chk(t, "orced_heads_bwd.grad", torch.float32, 2)
    ws = torch.empty(2 * B * L, dtype=torch.float32, device=dev)
    dWmu, dWlv = torch.empty_like(Wmu), torch.empty_like(Wlv)
    dbmu = torch.empty(L, dtype=torch.float32, device=dev)
    dblv = torch.empty_like(dbmu)
    dWc = torch.empty_like(Wc)
    dbc = torch.empty(K, dtype=torch.float32, device=dev)
    dx4 = torch.empty_like(x4) if need_dx else None
    check(_lib.load().pcaa_orced_heads_bwd(_p(x4), _p(eps), _p(logvar), _p(sup), _p(Wmu), _p(Wlv), _p(Wc), _p(d_logits),
                                           _p(d_sup), _p(d_mu), _p(d_logvar), _p(ws), _p(dWmu), _p(dbmu), _p(dWlv), _p(dblv),
                                           _p(dWc), _p(dbc), _p(dx4), B, K, d_in, L, _s()), "pcaa_orced_heads_bwd")
    return dx4, dWmu, dbmu, dWlv, dblv, dWc, dbc


def orced_kl(mu, logvar, mu_k, want_loss=True, gscale=None):
    """CG_kl_divergence and (``gscale`` given: the upstream gradient) its gradients w.r.t. mu, logvar, mu_k."""
    for t in (mu, logvar, mu_k):
        _chk(t, "orced_kl", torch.float32, 2)
    B, L = mu.shape
    if tuple(logvar.shape) != (B, L) or tuple(mu_k.shape) != (B, L):
        raise ValueError("orced_kl: shape mismatch")
    loss = torch.empty((), dtype=torch.float32, device=mu.device) if want_loss else None
    grads = (torch.empty_like(mu), torch.empty_like(mu), torch.empty_like(mu)) if gscale is not None else (None, None, None)
    check(_lib.load().pcaa_orced_kl(_p(mu), _p(logvar), _p(mu_k), _p(loss), _p(grads[0]), _p(grads[1]), _p(grads[2]),
                                    float(gscale if gscale is not None else 0.0), B, L, _s()), "pcaa_orced_kl")
    return loss, grads


def orced_triplet(x, labels, epsilon, margin, gscale=None):
    """MultiSimilarityMiner(epsilon) + TripletMarginLoss(margin) of x [B,L] (non-zero rows) / labels [B] int64 in dense
    form -> (loss scalar, dx [B,L] = gscale * dloss/dx, or None without ``gscale``).  Three launches, no host read."""
    _chk(x, "orced_triplet.x", torch.float32, 2)
    _chk(labels, "orced_triplet.labels", torch.int64, 1)
    B, L = x.shape
    lib = _lib.load()
    if labels.shape[0] != B or labels.device != x.device:
        raise ValueError(f"orced_triplet: labels {tuple(labels.shape)} on {labels.device} for x {tuple(x.shape)} on {x.device}")
    if not lib.pcaa_orced_triplet_supported(B, L):
        raise ValueError(f"orced_triplet: unsupported shape B = {B}, L = {L} (pcaa_orced_triplet_supported)")
    ws = torch.empty((B * B + B * L + 4 * B + 1) // 2, dtype=torch.float64, device=x.device)      # (8-byte aligned)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x) if gscale is not None else None
    check(lib.pcaa_orced_triplet(_p(x), _p(labels), float(epsilon), float(margin),
                                 float(gscale if gscale is not None else 0.0), _p(ws), _p(loss), _p(dx), B, L, _s()),
          "pcaa_orced_triplet")
    return loss, dx


def orced_ood(z, re, pred, mean_z, sd_z, thr_re, thresholds_g, want_p=False):
    """The ensemble open-set rule after its statistics: z [n,L] fp32, re [n] fp32, pred [n] int64; mean_z, sd_z [K,L] and
    thr_re [K] fp64 (sd_z: the square root of the class's std) -> out [n] int64 (pred, or K = unknown), and with
    ``want_p`` the box probabilities p [K,n] fp64."""
    _chk(z, "orced_ood.z", torch.float32, 2)
    _chk(re, "orced_ood.re", torch.float32, 1)
    _chk(pred, "orced_ood.pred", torch.int64, 1)
    _chk(mean_z, "orced_ood.mean_z", torch.float64, 2)
    _chk(sd_z, "orced_ood.sd_z", torch.float64, 2)
    _chk(thr_re, "orced_ood.thr_re", torch.float64, 1)
    n, L = z.shape
    K = mean_z.shape[0]
    if (re.shape[0] != n or pred.shape[0] != n or tuple(mean_z.shape) != (K, L) or tuple(sd_z.shape) != (K, L)
            or thr_re.shape[0] != K or K < 1 or L < 1
            or any(t.device != z.device for t in (re, pred, mean_z, sd_z, thr_re))):
        raise ValueError("orced_ood: shape or device mismatch")
    out = torch.empty(n, dtype=torch.int64, device=z.device)
    p = torch.empty((K, n), dtype=torch.float64, device=z.device) if want_p else None
    if n:
        check(_lib.load().pcaa_orced_ood(_p(z), _p(re), _p(pred), _p(mean_z), _p(sd_z), _p(thr_re), float(thresholds_g),
                                         _p(out), _p(p), n, K, L, _s()), "pcaa_orced_ood")
    return (out, p) if want_p else out


# ------------------------------------------------------------------ discriminator
def _disc_params(m):
    lin = (m.model[0], m.model[2], m.model[4])
    return [lin[0].weight, lin[0].bias, lin[1].weight, lin[1].bias, lin[2].weight, lin[2].bias]


def disc_workspace(B, K, device):
    n = _lib.load().pcaa_disc_workspace_bytes(B, K)
    return torch.empty(n // 4, dtype=torch.float32, device=device)


def disc_forward(x, label, params):
    """x [B, 32], label [B, K] with 0 <= K <= 32 -> D [B, 1].  K = 0 (a [B, 0] label, W1 [64, 32]) is the critic without a
    label: accepted here and by the three entry points below, as the ABI accepts it."""
    _chk(x, "disc.x", torch.float32, 2)
    _chk(label, "disc.label", torch.float32, 2)
    B, K = label.shape
    if x.shape != (B, 32) or params[0].shape != (64, 32 + K):
        raise ValueError("disc_forward: shapes")
    out = torch.empty((B, 1), dtype=torch.float32, device=x.device)
    check(_lib.load().pcaa_disc_forward(_p(x), _p(label), B, K, *[_p(p) for p in params], _p(out), _s()),
          "pcaa_disc_forward")
    return out


def disc_backward(x, label, params, gout, want_dx=True, want_dlabel=False, want_params=True, grads_out=None, dx_out=None):
    B, K = label.shape
    _chk(gout, "disc.gout", torch.float32)
    if gout.numel() != B:
        raise ValueError("disc_backward: gout size")
    dev = x.device
    if dx_out is not None:
        _chk(dx_out, "disc.dx_out", torch.float32)
        if tuple(dx_out.shape) != tuple(x.shape):
            raise ValueError("disc_backward: dx_out must have x's shape")
    dx = (dx_out if dx_out is not None else torch.empty_like(x)) if want_dx else None
    dl = torch.empty_like(label) if want_dlabel else None
    if want_params:
        grads = grads_out if grads_out is not None else [torch.empty_like(p) for p in params]
        ws = disc_workspace(B, K, dev)
    else:
        grads = [None] * 6
        ws = None
    check(_lib.load().pcaa_disc_backward(_p(x), _p(label), B, K, *[_p(p) for p in params], _p(gout), _p(dx), _p(dl),
                                         *[_p(g) for g in grads], _p(ws), 0 if ws is None else ws.numel() * 4, _s()),
          "pcaa_disc_backward")
    return dx, dl, (grads if want_params else None)


def disc_backward_backward(x, label, params, gout, gbar, want_dx=True, want_dlabel=False, want_dgout=True,
                           want_params=True):
    """Backward of disc_backward's ``dx`` output: gradients of sum <gbar, dx> w.r.t. (x, label, gout, params)."""
    for t, nm in ((x, "x"), (label, "label"), (gout, "gout"), (gbar, "gbar")):
        _chk(t, f"disc_bb.{nm}", torch.float32)
    B, K = label.shape
    if x.shape != (B, 32) or gbar.shape != (B, 32) or gout.numel() != B:
        raise ValueError("disc_backward_backward: shapes")
    dev = x.device
    dx2 = torch.empty_like(x) if want_dx else None
    dl2 = torch.empty_like(label) if want_dlabel else None
    dgo = torch.empty(B, dtype=torch.float32, device=dev) if want_dgout else None
    grads = [torch.empty_like(p) for p in params] if want_params else [None] * 6
    ws = disc_workspace(B, K, dev)
    check(_lib.load().pcaa_disc_backward_backward(_p(x), _p(label), B, K, *[_p(p) for p in params], _p(gout), _p(gbar),
                                                  _p(dx2), _p(dl2), _p(dgo), *[_p(g) for g in grads], _p(ws),
                                                  ws.numel() * 4, _s()), "pcaa_disc_backward_backward")
    return dx2, dl2, dgo, (grads if want_params else None)


def disc_wgan_gp(z, fv, label, alphas, params, gp_weight, grads_out=None, want_dz=False, losses_out=None):
    for t, nm in ((z, "z"), (fv, "fv"), (label, "label"), (alphas, "alphas")):
        _chk(t, f"wgan.{nm}", torch.float32)
    B, K = label.shape
    if z.shape != (B, 32) or fv.shape != (B, 32) or alphas.numel() != B:
        raise ValueError("disc_wgan_gp: shapes")
    dev = z.device
    losses = torch.empty(2, dtype=torch.float32, device=dev) if losses_out is None else _chk(losses_out, "wgan.losses_out", torch.float32)
    if losses.numel() != 2:
        raise ValueError("disc_wgan_gp: losses_out must hold 2 floats")
    grads = grads_out if grads_out is not None else [torch.empty_like(p) for p in params]
    ws = disc_workspace(B, K, dev)
    dz = torch.empty_like(z) if want_dz else None
    check(_lib.load().pcaa_disc_wgan_gp(_p(z), _p(fv), _p(label), _p(alphas), B, K, *[_p(p) for p in params],
                                        float(gp_weight), _p(losses), *[_p(g) for g in grads], _p(dz), _p(ws),
                                        ws.numel() * 4, _s()), "pcaa_disc_wgan_gp")
    if want_dz:
        return losses, grads, dz          # dz = d(d_loss)/dz (variant 1: learned centroids)
    return losses, grads


# ------------------------------------------------------------------ optimizer
def adam_step_(p, g, m, v, lr, b1, b2, eps, step, grad_scale=1.0, max_blocks=0):
    for t, nm in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _chk(t, f"adam.{nm}", torch.float32)
    n = p.numel()
    if not (g.numel() == n and m.numel() == n and v.numel() == n):
        raise ValueError("adam_step_: size mismatch")
    check(_lib.load().pcaa_adam_step(_p(p), _p(g), _p(m), _p(v), n, float(lr), float(b1), float(b2), float(eps),
                                     int(step), float(grad_scale), int(max_blocks), _s()), "pcaa_adam_step")


def adam_advance_(step_dev, coef_dev, lr, b1, b2):
    """Device-side optimizer step count: ``step_dev`` int32[1] += 1 and ``coef_dev`` float32[2] =
    (lr / (1 - b1^step), 1 / sqrt(1 - b2^step)) -- see pcaa_adam_advance."""
    _chk(step_dev, "adam.step_dev", torch.int32)
    _chk(coef_dev, "adam.coef_dev", torch.float32)
    if step_dev.numel() != 1 or coef_dev.numel() != 2:
        raise ValueError("adam_advance_: step_dev is int32[1], coef_dev float32[2]")
    check(_lib.load().pcaa_adam_advance(_p(step_dev), _p(coef_dev), float(lr), float(b1), float(b2), _s()),
          "pcaa_adam_advance")


def adam_step_dev_(p, g, m, v, b1, b2, eps, coef_dev, grad_scale=1.0, max_blocks=0):
    """adam_step_ with the step-dependent scalars read from ``coef_dev`` (adam_advance_)."""
    for nm, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        _chk(t, f"adam.{nm}", torch.float32)
    _chk(coef_dev, "adam.coef_dev", torch.float32)
    n = p.numel()
    if not (g.numel() == m.numel() == v.numel() == n) or coef_dev.numel() != 2:
        raise ValueError("adam_step_dev_: size mismatch")
    check(_lib.load().pcaa_adam_step_dev(_p(p), _p(g), _p(m), _p(v), n, float(b1), float(b2), float(eps),
                                         _p(coef_dev), float(grad_scale), int(max_blocks), _s()),
          "pcaa_adam_step_dev")


def adam_step_dev_g16_(p, g16, m, v, b1, b2, eps, coef_dev, grad_scale=1.0, max_blocks=0):
    """adam_step_dev_ with a bf16 gradient (a reduced bf16 gradient bucket, consumed without widening it first)."""
    for nm, t in (("p", p), ("m", m), ("v", v)):
        _chk(t, f"adam_g16.{nm}", torch.float32)
    _chk(g16, "adam_g16.g", torch.bfloat16)
    _chk(coef_dev, "adam_g16.coef_dev", torch.float32)
    n = p.numel()
    if not (g16.numel() == m.numel() == v.numel() == n) or coef_dev.numel() != 2:
        raise ValueError("adam_step_dev_g16_: size mismatch")
    check(_lib.load().pcaa_adam_step_dev_g16(_p(p), _p(g16), _p(m), _p(v), n, float(b1), float(b2), float(eps),
                                             _p(coef_dev), float(grad_scale), int(max_blocks), _s()),
          "pcaa_adam_step_dev_g16")


# ------------------------------------------------------------------ fused MLP heads (heads.hip)
def heads_supported(B, K, d_in, d_sup, d_head, d_proj, backward):
    return bool(_lib.load().pcaa_heads_supported(int(B), int(K), int(d_in), int(d_sup), int(d_head), int(d_proj),
                                                 1 if backward else 0))


HEADS_D_IN, HEADS_D_SUP, HEADS_D_HEAD, HEADS_D_PROJ = 512, 32, 16, 64      # the widths heads.hip is written for


def _chk_heads_shapes(who, named):
    """every (name, tensor, shape) is a contiguous fp32 device tensor of exactly the shape the kernel addresses"""
    for nm, t, shape in named:
        _chk(t, f"{who}.{nm}", torch.float32)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{who}.{nm}: shape {tuple(t.shape)}, expected {tuple(shape)}")


def _heads_dims(who, x4, W2, Wh, Wg, backward):
    """-> (B, K, width of W2's rows); refuses what pcaa_heads_supported refuses, before anything else is looked at"""
    _chk(x4, f"{who}.x4", torch.float32, 2)
    _chk(W2, f"{who}.W2", torch.float32, 2)
    B, K = x4.shape[0], W2.shape[0]
    if not heads_supported(B, K, x4.shape[1], HEADS_D_SUP, HEADS_D_HEAD if Wh is not None else 0,
                           HEADS_D_PROJ if Wg is not None else 0, backward):
        raise ValueError(f"{who}: x4 {tuple(x4.shape)} / W2 {tuple(W2.shape)}: takes x4 [B >= 1, {HEADS_D_IN}] and W2 with "
                         "K >= 1 rows" + (", B <= 64 and K <= 8 in the backward" if backward else ""))
    return B, K, HEADS_D_HEAD if Wh is not None else HEADS_D_SUP


def heads_fwd(x4, W1, b1, Wh, bh, W2, b2, Wg=None, bg=None):
    """One launch for MLP_sup1 -> (MLP_head) -> MLP_sup2 and, if given, the decoder projection head.
    Returns (sup_fv [B,32], h [B,16] or None, logits [B,K], hproj [B,64] or None)."""
    if (Wh is None) != (bh is None):
        raise ValueError("heads_fwd: Wh and bh go together")
    if (Wg is None) != (bg is None):
        raise ValueError("heads_fwd: Wg and bg go together")
    B, K, din2 = _heads_dims("heads_fwd", x4, W2, Wh, Wg, False)
    d_head, d_proj = HEADS_D_HEAD, HEADS_D_PROJ
    named = [("W1", W1, (HEADS_D_SUP, HEADS_D_IN)), ("b1", b1, (HEADS_D_SUP,)), ("W2", W2, (K, din2)), ("b2", b2, (K,))]
    if Wh is not None:
        named += [("Wh", Wh, (d_head, HEADS_D_SUP)), ("bh", bh, (d_head,))]
    if Wg is not None:
        named += [("Wg", Wg, (d_proj, HEADS_D_SUP)), ("bg", bg, (d_proj,))]
    _chk_heads_shapes("heads_fwd", named)
    dev = x4.device
    sup = torch.empty((B, 32), dtype=torch.float32, device=dev)
    h = torch.empty((B, d_head), dtype=torch.float32, device=dev) if Wh is not None else None
    logits = torch.empty((B, K), dtype=torch.float32, device=dev)
    hproj = torch.empty((B, d_proj), dtype=torch.float32, device=dev) if Wg is not None else None
    check(_lib.load().pcaa_heads_fwd(_p(x4), _p(W1), _p(b1), _p(Wh), _p(bh), _p(W2), _p(b2), _p(Wg), _p(bg),
                                     _p(sup), _p(h), _p(logits), _p(hproj), B, K, _s()), "pcaa_heads_fwd")
    return sup, h, logits, hproj


def heads_bwd(x4, sup_fv, h, logits, hproj, W1, Wh, W2, Wg, d_logits, d_sup, d_hproj, outs=None):
    """One launch for the backward of heads_fwd.  ``outs``: optional dict of destination views
    (dW1, db1, dWh, dbh, dW2, db2, dWg, dbg) -- missing ones are allocated.  Returns (grads dict, dx4)."""
    if (Wh is None) != (h is None):
        raise ValueError("heads_bwd: Wh and h go together")
    if d_hproj is not None and (Wg is None or hproj is None):
        raise ValueError("heads_bwd: d_hproj needs Wg and hproj")
    B, K, din2 = _heads_dims("heads_bwd", x4, W2, Wh, Wg, True)
    d_sup_, d_head, d_proj = HEADS_D_SUP, HEADS_D_HEAD, HEADS_D_PROJ
    shapes = {"dW1": (d_sup_, HEADS_D_IN), "db1": (d_sup_,), "dW2": (K, din2), "db2": (K,), "dWh": (d_head, d_sup_),
              "dbh": (d_head,), "dWg": (d_proj, d_sup_), "dbg": (d_proj,)}
    named = [("sup_fv", sup_fv, (B, d_sup_)), ("h", h, (B, d_head)), ("logits", logits, (B, K)), ("hproj", hproj, (B, d_proj)),
             ("W1", W1, shapes["dW1"]), ("Wh", Wh, shapes["dWh"]), ("W2", W2, shapes["dW2"]), ("Wg", Wg, shapes["dWg"]),
             ("d_logits", d_logits, (B, K)), ("d_sup", d_sup, (B, d_sup_)), ("d_hproj", d_hproj, (B, d_proj))]
    _chk_heads_shapes("heads_bwd", [n for n in named if n[1] is not None or n[0] in ("sup_fv", "logits", "W1")])
    outs = dict(outs or {})
    dev = x4.device
    want = ["dW1", "db1", "dW2", "db2"] + (["dWh", "dbh"] if Wh is not None else []) + \
        (["dWg", "dbg"] if d_hproj is not None else [])
    for k in want:
        if outs.get(k) is None:
            outs[k] = torch.empty(shapes[k], dtype=torch.float32, device=dev)
    _chk_heads_shapes("heads_bwd", [(k, outs[k], shapes[k]) for k in shapes if outs.get(k) is not None])
    dx4 = torch.empty_like(x4)
    check(_lib.load().pcaa_heads_bwd(_p(x4), _p(sup_fv), _p(h), _p(logits), _p(hproj), _p(W1), _p(Wh), _p(W2),
                                     _p(Wg), _p(d_logits), _p(d_sup), _p(d_hproj), _p(outs["dW1"]), _p(outs["db1"]),
                                     _p(outs.get("dWh")), _p(outs.get("dbh")), _p(outs["dW2"]), _p(outs["db2"]),
                                     _p(outs.get("dWg")), _p(outs.get("dbg")), _p(dx4), B, K, _s()), "pcaa_heads_bwd")
    return outs, dx4


# ------------------------------------------------------------------ fused temporal-block forward (dtc_fused.hip)
def dtc_conv_supported(T, cin, cout):
    return bool(_lib.load().pcaa_dtc_conv_supported(int(T), int(cin), int(cout)))


def dtc_conv_dgrad_supported(T, cin, cout):
    """the shapes dtc_conv_dgrad takes (the first argument check of the launcher)"""
    return T <= 32 and cin % 4 == 0 and cout % 4 == 0


def dtc_conv_ksplit(adjoint, B, cin, cout):
    """the ksplit the library wants for a forward (pcaa_dtc_conv_ksplit) or an adjoint (pcaa_dtc_conv_dgrad_ksplit) call"""
    lib = _lib.load()
    return (lib.pcaa_dtc_conv_dgrad_ksplit if adjoint else lib.pcaa_dtc_conv_ksplit)(int(B), int(cin), int(cout))


DTC_ROUTES = ("one_f32", "one_bf16", "pair32_f32", "pair32_bf16", "pair64_f32", "pair64_bf16")     # PCAA_DTC_ROUTE_* 0 .. 5


def dtc_conv_route(adjoint, bf16, B, cin, cout, ksplit, windowed=False):
    """the kernel such a call takes, by the library's own dispatch (pcaa_dtc_conv_route) -> its name in DTC_ROUTES"""
    return DTC_ROUTES[_lib.load().pcaa_dtc_conv_route(int(adjoint), int(bf16), int(B), int(cin), int(cout), int(ksplit),
                                                      int(windowed))]


def dtc_conv_fwd(src, scale, shift, W2d, B, T, dilation, stats=None, want_col=False, tail=None, bf16=False, win_row=None,
                 ksplit=None):
    """One DilTempConv1d layer forward in one launch (see pcaa_dtc_conv_fwd): returns (y, col or None).
    ``win_row`` (a WindowRows of B windows): ``src`` is a frame-feature table [table_rows, cin] and sequence b reads its T
    rows from win_row[b] on (pcaa_dtc_conv_fwd_win, or pcaa_dtc_conv_fwd_seg for segmented rings; eval form: no
    statistics, no im2col).  ``ksplit``: pcaa_dtc_conv_ksplit's answer where the caller has it."""
    _chk(src, "dtc_conv_fwd.src", torch.float32, 2)
    _chk(W2d, "dtc_conv_fwd.W", torch.float32, 2)
    rows, cin = src.shape
    cout = W2d.shape[0]
    if win_row is not None:
        if not isinstance(win_row, WindowRows):
            raise TypeError("dtc_conv_fwd: win_row must be an ops.WindowRows (it carries the host-side range check)")
        if stats is not None or want_col or tail is not None:
            raise ValueError("dtc_conv_fwd: a windowed source is eval-only (no statistics, no im2col)")
        if len(win_row) != B or win_row.T != T or win_row.table_rows != rows:
            raise ValueError(f"dtc_conv_fwd: win_row describes {len(win_row)} windows of {win_row.T} rows in a table of "
                             f"{win_row.table_rows}, got B={B} T={T} table {tuple(src.shape)}")
        rows = B * T
    if rows != B * T or W2d.shape[1] != cin * 3 or not dtc_conv_supported(T, cin, cout):
        raise ValueError(f"dtc_conv_fwd: unsupported shapes src {tuple(src.shape)} W {tuple(W2d.shape)} B={B} T={T}")
    if scale is not None:
        _chk(scale, "dtc_conv_fwd.scale", torch.float32)
        _chk(shift, "dtc_conv_fwd.shift", torch.float32)
        if scale.numel() != cin or shift.numel() != cin:
            raise ValueError("dtc_conv_fwd: scale/shift length")
    if stats is not None:
        _chk(stats, "dtc_conv_fwd.stats", torch.float64)
        if tuple(stats.shape) != (NREP, 2, cout):
            raise ValueError("dtc_conv_fwd: stats shape")
    y = torch.empty((rows, cout), dtype=torch.float32, device=src.device)
    col = torch.empty((rows, cin * 3), dtype=torch.float32, device=src.device) if want_col else None
    lib = _lib.load()
    if ksplit is None:
        ksplit = dtc_conv_ksplit(False, B, cin, cout)
    if ksplit > 1:                 # split K: the partial products go to slabs, a reduction pass makes y (and the statistics)
        stride = rows * cout
        dst = torch.empty(ksplit * stride, dtype=torch.float32, device=src.device)
        dst_stats, split = None, (ksplit, stride)
    else:
        dst, dst_stats, split = y, stats, (1, 0)
        if tail is not None and stats is not None:
            tail.arm(stats)
    operands = (_p(src), _p(scale), _p(shift), _p(W2d), _p(dst))
    shape = (B, T, cin, cout, int(dilation))
    # one call per entry point (_bf16: the throughput mode's MFMA variant): plain, windowed, segmented
    if win_row is None:
        fwd = lib.pcaa_dtc_conv_fwd_bf16 if bf16 else lib.pcaa_dtc_conv_fwd
        rc = fwd(*operands, _p(col), _p(dst_stats), NREP, *shape, *split, _s())
    elif not win_row.segments:
        fwd = lib.pcaa_dtc_conv_fwd_win_bf16 if bf16 else lib.pcaa_dtc_conv_fwd_win
        rc = fwd(*operands, _p(col), _p(dst_stats), NREP, *shape, *split,
                 _p(win_row.dev), win_row.table_rows, win_row.ring_rows, _s())
    else:                          # eval only: the entry point takes neither col nor statistics
        fwd = lib.pcaa_dtc_conv_fwd_seg_bf16 if bf16 else lib.pcaa_dtc_conv_fwd_seg
        rc = fwd(*operands, *shape, *split, _p(win_row.dev), win_row.segments, win_row.ring_rows, _s())
    check(rc, "pcaa_dtc_conv_fwd")
    if ksplit > 1 and stats is not None:
        check(lib.pcaa_splitk_reduce_stats(_p(dst), ksplit, stride, _p(y), _p(stats), NREP, rows, cout, _s()),
              "pcaa_splitk_reduce_stats")
    elif ksplit > 1:
        check(lib.pcaa_splitk_reduce(_p(dst), ksplit, stride, stride, _p(y), 0, _s()), "pcaa_splitk_reduce")
    if tail is not None and stats is not None:
        tail.resolve(stats)
    return y, col


def dtc_conv_dgrad(dy, W2d, B, T, cin, dilation, dz=None, y=None, coef=None, want_dy=False, below=None, tail=None,
                   bf16=False, ksplit=None):
    """Adjoint of the causal dilated convolution w.r.t. its input in one launch (pcaa_dtc_conv_dgrad).
    ``dy`` [B*T,cout], or None with ``dz``, ``y``, ``coef``: dy is formed on load (``want_dy``: also returned).
    ``below`` = (y, scale, shift, mean, rstd) of the layer below: the result is that layer's dz and its
    BatchNorm-backward statistics come back too.  ``ksplit``: pcaa_dtc_conv_dgrad_ksplit's answer where the caller has it.
    Returns (out [B*T,cin], stats or None, dy or None)."""
    _chk(W2d, "dtc_conv_dgrad.W", torch.float32, 2)
    cout = W2d.shape[0]
    rows = B * T
    src = dy if dy is not None else dz
    _chk(src, "dtc_conv_dgrad.dy/dz", torch.float32, 2)
    if tuple(src.shape) != (rows, cout) or tuple(W2d.shape) != (cout, cin * 3) or not dtc_conv_dgrad_supported(T, cin, cout):
        raise ValueError(f"dtc_conv_dgrad: unsupported shapes {tuple(src.shape)} W {tuple(W2d.shape)} B={B} T={T}")
    if dy is None:
        _chk(y, "dtc_conv_dgrad.y", torch.float32, 2)
        _chk(coef, "dtc_conv_dgrad.coef", torch.float32, 2)
        if tuple(y.shape) != (rows, cout) or tuple(coef.shape) != (3, cout):
            raise ValueError("dtc_conv_dgrad: y / coef shapes")
    lib = _lib.load()
    dev = src.device
    out = torch.empty((rows, cin), dtype=torch.float32, device=dev)
    dy_out = torch.empty((rows, cout), dtype=torch.float32, device=dev) if (want_dy and dy is None) else None
    ks = dtc_conv_ksplit(True, B, cin, cout) if ksplit is None else ksplit
    dgrad = lib.pcaa_dtc_conv_dgrad_bf16 if bf16 else lib.pcaa_dtc_conv_dgrad
    stats = None
    ep = [None] * 5
    if below is not None:
        if ks > 1:
            raise ValueError("dtc_conv_dgrad: the fused epilogue needs cout <= 512")
        for t in below:
            _chk(t, "dtc_conv_dgrad.below", torch.float32)
        if tuple(below[0].shape) != (rows, cin) or any(t.numel() != cin for t in below[1:]):
            raise ValueError("dtc_conv_dgrad: below shapes")
        ep = list(below)
        stats = new_stats(cin, dev)
    if ks > 1:
        stride = rows * cin
        slabs = torch.empty(ks * stride, dtype=torch.float32, device=dev)
        check(dgrad(_p(dy), _p(dz), _p(y), _p(coef), _p(dy_out), _p(W2d), _p(slabs), None, None, None,
                                      None, None, None, NREP, B, T, cin, cout, int(dilation), ks, stride, _s()),
              "pcaa_dtc_conv_dgrad")
        check(lib.pcaa_splitk_reduce(_p(slabs), ks, stride, stride, _p(out), 0, _s()), "pcaa_splitk_reduce")
    else:
        if tail is not None and stats is not None:
            tail.arm(stats)
        check(dgrad(_p(dy), _p(dz), _p(y), _p(coef), _p(dy_out), _p(W2d), _p(out), *[_p(t) for t in ep],
                                      _p(stats), NREP, B, T, cin, cout, int(dilation), 1, 0, _s()),
              "pcaa_dtc_conv_dgrad")
        if tail is not None and stats is not None:
            tail.resolve(stats)
    return out, stats, (dy if dy is not None else dy_out)
