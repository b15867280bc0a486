"""Every dispatch branch of csrc/elementwise.hip against fp64 (references, gates and inputs: tests/elementwise_ref.py;
the gates themselves are shown reference-safe and defect-sensitive by tests/test_elementwise_gates_cpu.py).

Every comparison prints ``worst |err| / gate`` of its case (pytest -rP); the numbers are reported, the assertion is
``<= 1``.

    branch of the launcher                                          test
    --------------------------------------------------------------  ----------------------------------------------------
    bn_act_meanpool_fwd: streaming kernel (bf16, ch 1024,           test_meanpool_streaming_kernel
      group_rows % 4 == 0, groups >= 512), eval and train             [512-4] one batch, [513-12] odd batches, [1025-8]
                                                                      second trip of one group, [2049-36] three trips
    bn_act_meanpool_fwd: just outside the streaming condition       test_meanpool_generic_kernel_beside_the_streaming_one
      (groups 511, group_rows % 4 != 0, ch 512)
    bn_act_meanpool_fwd: generic kernel, fp32 / bf16, eval / train  test_meanpool_generic_kernel
    bn_act_bwd_dz: dense / pooled x fp32 / bf16 x dz / stats-only   test_bn_act_bwd_dz_dense, test_bn_act_bwd_dz_pooled
    bn_bwd_dy_fused: dense / pooled x fp32 / bf16, grid unit > 1    test_bn_bwd_dy_fused_dense, test_bn_bwd_dy_fused_pooled,
                                                                    test_bn_bwd_dy_fused_may_overwrite_da
    bn_bwd_dy_fused_split (dense / pooled), bn_act_fwd_split        test_split_twins
    bn_act_fwd, bn_bwd_dy: fp32 / bf16, one trip / several          test_bn_act_fwd_and_bn_bwd_dy
    bn_pool_bwd_stats: groups per block 1 / 3 / 32, channel loop    test_bn_pool_bwd_stats
    bn_finalize (bias, running stats on / off), bn_bwd_finalize,    test_bn_finalize_family
      bn_eval_coeffs
    the replica sum of the three finalizes and of the carried     test_finalize_replica_counts
      tail: nrep 1 / 11 / 16 (remainder only, trip + remainder,
      trips only), ch 260 (ragged second workgroup)
    splitk_reduce (accumulate on / off), splitk_reduce_stats        test_splitk_reduce
    adam: max_blocks <= 1024 (4 quads per thread) / above,          test_adam_against_fp64, test_adam_kernels_agree_bitwise,
      host step / device step, fp32 / bf16 gradient, n % 4 tail       test_adam_device_step_equals_host_step,
                                                                      test_adam_bf16_gradient_equals_widened_gradient,
                                                                      test_adam_subrange_leaves_the_rest_untouched
    colsum (8-deep trip / remainder), rowsum, total                 test_colsum, test_rowsum, test_total
    scale_rows, scale_by_device_scalar, bias_act_, elu_bwd_from_out test_scale_helpers, test_bias_act, test_elu_bwd_from_out
    gather_rows / gather_rows_w4 (valid, repeated, out-of-range)    test_gather_rows
    pack_points (strided source), prior_sample (K > D, K < D)       test_pack_points_strided, test_prior_sample
    host-side argument checks                                       test_rejected_arguments
"""
import pytest
import torch

import elementwise_ref as R
import eval_bwd_ref as E
from opensetgaitrecognition_pcaa_amd import _lib, ops
from opensetgaitrecognition_pcaa_amd._lib import ACT_ELU, ACT_NONE, PcaaError

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]


def check(name, got, want, gate):
    err = (got.double() - want).abs() / gate.clamp_min(1e-300)
    r = float(err.max())
    print(f"[elementwise] {name}: worst |err| / gate = {r:.3f}")
    if not r <= 1.0:
        at = [int(i) for i in torch.unravel_index(err.argmax(), err.shape)]
        over = (err > 1.0).nonzero()
        print(f"[elementwise] {name}: worst at {at}; {over.shape[0]} of {err.numel()} over the gate, first {over[:8].tolist()}")
    assert r <= 1.0, (name, r)
    return r


def bn_inputs(rows, ch, dtype, seed):
    return (R.activations(rows, ch, dtype, seed, DEV),) + R.bn_vectors(ch, seed, DEV)


# ===================================================================================================== Part A: mean-pool
def _meanpool(groups, Rr, ch, dtype, expect_stream):
    stream = dtype == BF16 and ch == 1024 and Rr % 4 == 0 and groups >= 512
    assert stream == expect_stream
    y, sc, sh, mu, rs = bn_inputs(groups * Rr, ch, dtype, R.seed_of(ch, Rr))
    ref = R.meanpool_ref(y, sc, sh, mu, rs, groups, Rr, lanes=1 if stream else R.row_lanes(ch))
    pooled_eval = ops.bn_act_meanpool_fwd(y, sc, sh, groups, Rr)
    pooled, e = ops.bn_act_meanpool_fwd(y, sc, sh, groups, Rr, mu, rs)
    tag = f"meanpool {'stream' if stream else 'generic'} {dtype} groups={groups} R={Rr} ch={ch}"
    check(tag + " pooled(eval)", pooled_eval, ref["pooled"], ref["pooled_gate"])
    check(tag + " pooled(train)", pooled, ref["pooled"], ref["pooled_gate"])
    check(tag + " e1", e[0], ref["e1"], ref["e1_gate"])
    check(tag + " e2", e[1], ref["e2"], ref["e2_gate"])
    assert torch.equal(pooled, pooled_eval)


@pytest.mark.parametrize("groups,Rr", [(512, 4), (513, 12), (1024, 32), (1025, 8), (1920, 128), (2049, 36)])
def test_meanpool_streaming_kernel(groups, Rr):
    _meanpool(groups, Rr, 1024, BF16, True)


@pytest.mark.parametrize("groups,Rr,ch", [(511, 128, 1024), (600, 150, 1024), (1920, 128, 512)])
def test_meanpool_generic_kernel_beside_the_streaming_one(groups, Rr, ch):
    _meanpool(groups, Rr, ch, BF16, False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Rr", [1, 3, 30, 150, 255])
@pytest.mark.parametrize("ch", [4, 16, 64, 512, 1024])
def test_meanpool_generic_kernel(ch, Rr, dtype):
    _meanpool(max(7, 4096 // ch), Rr, ch, dtype, False)


# ===================================================================================================== bn_act_bwd_dz
def _bwd_dz(rows, ch, dtype, gr):
    """gr: rows per group of the pooled gradient, 0: dense"""
    seed = R.seed_of(ch, rows)
    y, sc, sh, mu, rs = bn_inputs(rows, ch, dtype, seed)
    kw = ({"dpool": R.gradient(rows // gr, ch, F32, seed, DEV), "group_rows": gr, "pool_scale": 1.0 / gr} if gr
          else {"da": R.gradient(rows, ch, dtype, seed, DEV)})
    ref = R.bn_act_bwd_dz_ref(y, sc, sh, mu, rs, **kw)
    tag = f"bn_act_bwd_dz {'pooled gr=%d' % gr if gr else 'dense'} {dtype} rows={rows} ch={ch}"
    dz, stats = ops.bn_act_bwd_dz(y, sc, sh, mu, rs, **kw)
    check(tag + " dz", dz, ref["dz"], R.out_gate(ref["dz_gate"], ref["dz"], dtype))
    check(tag + " stats", stats.sum(0), ref["stats"], ref["stats_gate"])
    only = ops.bn_act_bwd_stats(y, sc, sh, mu, rs, **kw)
    check(tag + " stats(statistics-only pass)", only.sum(0), ref["stats"], ref["stats_gate"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ch", [4, 16, 512, 1024])
@pytest.mark.parametrize("rows", [1, 127, 128, 129, 3840 + 30])
def test_bn_act_bwd_dz_dense(rows, ch, dtype):
    _bwd_dz(rows, ch, dtype, 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ch", [4, 16, 512, 1024])
@pytest.mark.parametrize("rows,gr", [(1, 1), (127, 1), (128, 1), (129, 1), (126, 7), (133, 7), (3871, 7), (120, 30), (150, 30),
                                     (3840 + 30, 30), (150, 150), (300, 150), (3900, 150)])
def test_bn_act_bwd_dz_pooled(rows, gr, ch, dtype):
    _bwd_dz(rows, ch, dtype, gr)


# ===================================================================================================== column-invariant grid
def trip_rows(ch):
    """rows one grid-stride trip of the column-invariant grid covers when the grid is at its cap"""
    qpr = ch // 4
    g = qpr
    b = 256
    while b:
        g, b = b, g % b
    unit = qpr // g
    grid = -(-2048 // unit) * unit
    return grid * 256 // qpr


def multi_trip_rows(ch, multiple=1):
    """more than two full trips and a partial third"""
    rows = int(2.3 * trip_rows(ch)) + 1
    return -(-rows // multiple) * multiple


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ch", [4, 20, 96, 512, 1020, 1024])
@pytest.mark.parametrize("trips", ["one", "several"])
def test_bn_act_fwd_and_bn_bwd_dy(trips, ch, dtype):
    rows = 33 if trips == "one" else multi_trip_rows(ch)
    seed = R.seed_of(ch, 33)
    y, sc, sh, mu, rs = bn_inputs(rows, ch, dtype, seed)
    want, gate = R.bn_act_fwd_ref(y, sc, sh)
    check(f"bn_act_fwd {dtype} rows={rows} ch={ch}", ops.bn_act_fwd(y, sc, sh), want, R.out_gate(gate, want, dtype))
    coef = R.coef_vectors(ch, seed, DEV)
    dz = R.gradient(rows, ch, dtype, seed, DEV)
    want, gate = R.bn_bwd_dy_ref(dz, y, coef)
    check(f"bn_bwd_dy {dtype} rows={rows} ch={ch}", ops.bn_bwd_dy(dz, y, coef), want, R.out_gate(gate, want, dtype))


def _dy_fused(rows, ch, dtype, gr):
    seed = R.seed_of(ch, gr)
    y, sc, sh, mu, rs = bn_inputs(rows, ch, dtype, seed)
    coef = R.coef_vectors(ch, seed, DEV, grad_scale=1.0 / gr if gr else 1.0)
    kw = ({"dpool": R.gradient(rows // gr, ch, F32, seed, DEV), "group_rows": gr, "pool_scale": 1.0 / gr} if gr
          else {"da": R.gradient(rows, ch, dtype, seed, DEV)})
    want, gate = R.bn_bwd_dy_fused_ref(y, sc, sh, coef, **kw)
    tag = f"bn_bwd_dy_fused {'pooled gr=%d' % gr if gr else 'dense'} {dtype} rows={rows} ch={ch}"
    check(tag, ops.bn_bwd_dy_fused(y, sc, sh, coef, **kw), want, R.out_gate(gate, want, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ch", [4, 20, 96, 512, 1020, 1024])
def test_bn_bwd_dy_fused_dense(ch, dtype):
    _dy_fused(multi_trip_rows(ch), ch, dtype, 0)
    _dy_fused(33, ch, dtype, 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("gr", [1, 7, 30, 128, 150])
@pytest.mark.parametrize("ch", [4, 20, 96, 512, 1020, 1024])
def test_bn_bwd_dy_fused_pooled(ch, gr, dtype):
    """group_rows below and above the rows a trip advances (2 048 at ch = 1024, 524 288 at ch = 4); 6 300 rows at
    ch = 1024 is the issue's example of three trips"""
    _dy_fused(multi_trip_rows(ch, gr), ch, dtype, gr)
    _dy_fused(3 * gr, ch, dtype, gr)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bn_bwd_dy_fused_may_overwrite_da(dtype):
    """include/pcaa_hip.h: dy may alias da"""
    rows, ch = 6300, 1024
    seed = R.seed_of(ch, 0)
    y, sc, sh, mu, rs = bn_inputs(rows, ch, dtype, seed)
    coef = R.coef_vectors(ch, seed, DEV)
    da = R.gradient(rows, ch, dtype, seed, DEV)
    apart = ops.bn_bwd_dy_fused(y, sc, sh, coef, da=da)
    buf = da.clone()
    same = ops.bn_bwd_dy_fused(y, sc, sh, coef, da=buf, out=buf)
    assert same.data_ptr() == buf.data_ptr() and torch.equal(same, apart)
    want, gate = R.bn_bwd_dy_fused_ref(y, sc, sh, coef, da=da)
    check(f"bn_bwd_dy_fused dense {dtype} dy aliases da", same, want, R.out_gate(gate, want, dtype))


@pytest.mark.parametrize("gr", [30, 150])
def test_split_twins(gr):
    """the split-image producers against their fp32 twins (the assertions and the input scaling of
    test_hip_ops.py::test_split_image_producers) at a non-power-of-two ch, several trips, group_rows 30 and 150"""
    ch = 96
    rows = multi_trip_rows(ch, gr)
    seed = R.seed_of(ch, gr)
    y, sc, sh, mu, rs = bn_inputs(rows, ch, F32, seed)
    a32 = ops.bn_act_fwd(y, sc, sh)
    ai = ops.bn_act_fwd_split(y, sc, sh)
    hi = a32.to(torch.float16)
    assert torch.equal(ai.img[:, :ch], hi) and torch.equal(ai.img[:, ch:], (a32 - hi.float()).to(torch.float16))
    coef = R.coef_vectors(ch, seed, DEV) * 1e-4
    da = R.gradient(rows, ch, F32, seed, DEV) * 1e-4
    dy32 = ops.bn_bwd_dy_fused(y, sc, sh, coef, da=da.clone())
    dyi = ops.bn_bwd_dy_fused_split(y, sc, sh, coef, da=da)
    r = (dyi.float() - dy32).abs().max().item() / dy32.abs().max().item()
    print(f"[elementwise] bn_bwd_dy_fused_split dense rows={rows} ch={ch}: max |diff| / max |dy| = {r:.3e} (bound 2e-6)")
    assert r <= 2e-6
    dpool = R.gradient(rows // gr, ch, F32, seed, DEV) * 1e-3
    dy32p = ops.bn_bwd_dy_fused(y, sc, sh, coef, dpool=dpool, group_rows=gr, pool_scale=1 / gr)
    dyip = ops.bn_bwd_dy_fused_split(y, sc, sh, coef, dpool=dpool, group_rows=gr, pool_scale=1 / gr)
    r = (dyip.float() - dy32p).abs().max().item() / dy32p.abs().max().item()
    print(f"[elementwise] bn_bwd_dy_fused_split pooled gr={gr} rows={rows} ch={ch}: max |diff| / max |dy| = {r:.3e} (bound 2e-6)")
    assert r <= 2e-6
    ops.range_check(DEV)            # nothing left the fp16 range of the images


# ===================================================================================================== bn_pool_bwd_stats
@pytest.mark.parametrize("ch", [4, 512, 1024, 1028])
@pytest.mark.parametrize("groups", [1, 7, 255, 773, 8195])
def test_bn_pool_bwd_stats(groups, ch):
    """groups per block 1, 1, 1, 3, 32: partial last blocks, partial trips of eight; ch = 1028: the second trip of the
    channel loop"""
    seed = R.seed_of(ch, groups)
    dpool = R.gradient(groups, ch, F32, seed, DEV)
    e = torch.stack([R.uniform(groups * ch, seed + 8, DEV, 0.0, 128.0).view(groups, ch),
                     R.uniform(groups * ch, seed + 9, DEV, -100.0, 100.0).view(groups, ch)]).float().contiguous()
    want, gate = R.bn_pool_bwd_stats_ref(dpool, e, 1.0 / 128)
    stats = ops.bn_pool_bwd_stats(dpool, e, 1.0 / 128)
    check(f"bn_pool_bwd_stats groups={groups} ch={ch}", stats.sum(0), want, gate)


# ===================================================================================================== finalize kernels
class _BN:
    def __init__(self, case):
        self.weight, self.bias = case["gamma"], case["beta"]
        self.running_mean, self.running_var = case["rm"].clone(), case["rv"].clone()
        self.num_batches_tracked = torch.full((), 5, dtype=torch.int64, device=DEV)
        self.momentum, self.eps = 0.1, 1e-5


@pytest.mark.parametrize("update_running", [True, False])
@pytest.mark.parametrize("lin_bias", [True, False])
@pytest.mark.parametrize("ch", [4, 100, 1024])
def test_bn_finalize_family(ch, lin_bias, update_running):
    """column 0 of the case is constant: its variance clamps at 0 and rstd = 1 / sqrt(eps)"""
    case = R.finalize_case(ch, lin_bias, DEV)
    bn = _BN(case)
    eps = R.f32(bn.eps)
    ref = R.bn_finalize_ref(case["stats"], case["count"], case["lin_bias"], case["gamma"], case["beta"],
                            case["rm"] if update_running else None, case["rv"] if update_running else None, 0.1, eps)
    scale, shift, mean, rstd = ops.bn_finalize(case["stats"], case["count"], case["lin_bias"], bn, ch, update_running)
    tag = f"bn_finalize ch={ch} bias={lin_bias} running={update_running}"
    for k, got in (("scale", scale), ("shift", shift), ("mean", mean), ("rstd", rstd)):
        check(f"{tag} {k}", got, *ref[k])
    assert abs(float(rstd[0]) * eps ** 0.5 - 1.0) <= 1e-6
    if update_running:
        check(f"{tag} running_mean", bn.running_mean, *ref["running_mean"])
        check(f"{tag} running_var", bn.running_var, *ref["running_var"])
        assert int(bn.num_batches_tracked) == 6
    else:
        assert torch.equal(bn.running_mean, case["rm"]) and torch.equal(bn.running_var, case["rv"])
        assert int(bn.num_batches_tracked) == 5
    # backward finalize on the same statistics rows (any two sums will do), with the mean / rstd just produced
    refb = R.bn_bwd_finalize_ref(case["stats"], case["count"], case["gamma"], mean, rstd)
    coef, dgamma, dbeta = ops.bn_bwd_finalize(case["stats"], case["count"], bn, mean, rstd, ch)
    for k, got in (("coef0", coef[0]), ("coef1", coef[1]), ("coef2", coef[2]), ("dgamma", dgamma), ("dbeta", dbeta)):
        check(f"bn_bwd_finalize ch={ch} {k}", got, *refb[k])
    # eval coefficients: BatchNorm1d.eval() of (acc + bias), to fp32 rounding
    sc, sft = ops.bn_eval_coeffs(bn, ch, case["lin_bias"])
    wsc, gsc, wsft, gsft = R.bn_eval_coeffs_ref(case["gamma"], case["beta"], bn.running_mean, bn.running_var, case["lin_bias"], bn.eps)
    check(f"bn_eval_coeffs ch={ch} bias={lin_bias} scale", sc, wsc, gsc)
    check(f"bn_eval_coeffs ch={ch} bias={lin_bias} shift", sft, wsft, gsft)
    m = torch.nn.BatchNorm1d(ch, eps=eps).double().to(DEV).eval()
    with torch.no_grad():
        for dst, src in ((m.weight, case["gamma"]), (m.bias, case["beta"]), (m.running_mean, bn.running_mean),
                         (m.running_var, bn.running_var)):
            dst.copy_(src)
        acc = R.uniform(64 * ch, 3, DEV, -2.0, 2.0).view(64, ch)
        want = m(acc + (case["lin_bias"].double() if lin_bias else 0.0))
    check(f"bn_eval_coeffs ch={ch} bias={lin_bias} vs BatchNorm1d.eval()", acc * sc.double() + sft.double(), want,
          acc.abs() * gsc + gsft)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("ch", [4, 260])
@pytest.mark.parametrize("nrep", [1, 11, 16])
def test_finalize_replica_counts(nrep, ch):
    """ops always passes NREP = 16, i.e. two 8-deep trips of the replica sum and no remainder: through the C ABI,
    nrep = 1 (remainder only), 11 (one trip and three) and 16; ch = 260: the second workgroup of the stand-alone
    finalize has a ragged end.  The stand-alone finalizes against fp64, and bitwise against the finalize carried by a
    producer (bn_pool_bwd_stats, one group: one workgroup, which is then the last to arrive) on the same statistics."""
    lib, s = _lib.load(), ops._s()
    count = 176                                                    # a multiple of 11 and of 16
    case = R.finalize_case(ch, True, DEV, count=count, nrep=nrep)
    buf = torch.zeros(nrep * 2 * ch + 2, dtype=torch.float64, device=DEV)
    stats = buf[:nrep * 2 * ch].view(nrep, 2, ch)
    stats.copy_(case["stats"])
    counter = buf[nrep * 2 * ch:].view(torch.int32)
    # the producer adds a little to replica 0 (nothing to the constant column 0) before its last workgroup finalizes
    dpool = R.gradient(1, ch, F32, R.seed_of(ch, nrep), DEV)
    dpool[:, 0] = 0.0
    e = R.uniform(2 * ch, R.seed_of(nrep, ch), DEV, -1.0, 1.0).float().view(2, 1, ch).contiguous()

    def produce():
        _lib.check(lib.pcaa_bn_pool_bwd_stats(dpool.data_ptr(), e[0].data_ptr(), e[1].data_ptr(), 1.0 / 128, stats.data_ptr(),
                                              nrep, 1, ch, s), "pcaa_bn_pool_bwd_stats")
        assert lib.pcaa_bn_tail_pending() == 0, "the producer must have carried the finalize"
        assert int(counter[0]) == 0, "the finalizer leaves the arrival counter at zero"

    eps, mom = R.f32(1e-5), 0.1
    g, b, lb = case["gamma"], case["beta"], case["lin_bias"]
    tag = f"finalize nrep={nrep} ch={ch}"
    # ---- forward: carried, then stand-alone on the statistics the carried one saw
    run = {}
    for form in ("carried", "alone"):
        o = {k: torch.empty(ch, device=DEV) for k in ("scale", "shift", "mean", "rstd")}
        o["running_mean"], o["running_var"] = case["rm"].clone(), case["rv"].clone()
        o["nbt"] = torch.full((), 5, dtype=torch.int64, device=DEV)
        args = (stats.data_ptr(), nrep, count, lb.data_ptr(), g.data_ptr(), b.data_ptr(), o["running_mean"].data_ptr(),
                o["running_var"].data_ptr(), o["nbt"].data_ptr(), mom, eps, o["scale"].data_ptr(), o["shift"].data_ptr(),
                o["mean"].data_ptr(), o["rstd"].data_ptr(), ch)
        if form == "carried":
            _lib.check(lib.pcaa_bn_tail_arm_fwd(*args, counter.data_ptr()), "pcaa_bn_tail_arm_fwd")
            produce()
        else:
            _lib.check(lib.pcaa_bn_finalize(*args, s), "pcaa_bn_finalize")
        run[form] = o
    ref = R.bn_finalize_ref(stats, count, lb, g, b, case["rm"], case["rv"], mom, eps)
    for k in ("scale", "shift", "mean", "rstd", "running_mean", "running_var"):
        check(f"{tag} bn_finalize {k}", run["alone"][k], *ref[k])
        assert _same_bits(run["carried"][k], run["alone"][k]), (tag, k)
    assert int(run["alone"]["nbt"]) == 6 and int(run["carried"]["nbt"]) == 6
    assert abs(float(run["alone"]["rstd"][0]) * eps ** 0.5 - 1.0) <= 1e-6
    mean, rstd = run["alone"]["mean"], run["alone"]["rstd"]
    # ---- backward
    runb = {}
    for form in ("carried", "alone"):
        o = {"coef": torch.empty(3, ch, device=DEV), "dgamma": torch.empty(ch, device=DEV), "dbeta": torch.empty(ch, device=DEV)}
        args = (stats.data_ptr(), nrep, count, g.data_ptr(), mean.data_ptr(), rstd.data_ptr(), o["coef"].data_ptr(),
                o["dgamma"].data_ptr(), o["dbeta"].data_ptr(), ch)
        if form == "carried":
            _lib.check(lib.pcaa_bn_tail_arm_bwd(*args, counter.data_ptr()), "pcaa_bn_tail_arm_bwd")
            produce()
        else:
            _lib.check(lib.pcaa_bn_bwd_finalize(*args, s), "pcaa_bn_bwd_finalize")
        runb[form] = o
    refb = R.bn_bwd_finalize_ref(stats, count, g, mean, rstd)
    got = runb["alone"]
    for k, t in (("coef0", got["coef"][0]), ("coef1", got["coef"][1]), ("coef2", got["coef"][2]), ("dgamma", got["dgamma"]),
                 ("dbeta", got["dbeta"])):
        check(f"{tag} bn_bwd_finalize {k}", t, *refb[k])
    for k in ("coef", "dgamma", "dbeta"):
        assert _same_bits(runb["carried"][k], runb["alone"][k]), (tag, k)
    # ---- eval-mode backward finalize (never carried)
    sc = run["alone"]["scale"]
    oe = {k: torch.empty(ch, device=DEV) for k in ("dgamma", "dbeta", "dbias")}
    _lib.check(lib.pcaa_bn_eval_bwd_finalize(stats.data_ptr(), nrep, sc.data_ptr(), oe["dgamma"].data_ptr(),
                                             oe["dbeta"].data_ptr(), oe["dbias"].data_ptr(), ch, s), "pcaa_bn_eval_bwd_finalize")
    refe = E.bn_eval_bwd_finalize_ref(stats, sc)
    for k in ("dgamma", "dbeta", "dbias"):
        check(f"{tag} bn_eval_bwd_finalize {k}", oe[k], *refe[k])


# ===================================================================================================== split-K reduction
@pytest.mark.parametrize("ch", [4, 64, 1024])
@pytest.mark.parametrize("rows", [1, 31, 33, 900])
@pytest.mark.parametrize("nsplit", [1, 7, 8, 9, 64])
def test_splitk_reduce(nsplit, rows, ch):
    n = rows * ch
    slabs = R.uniform(nsplit * n, R.seed_of(nsplit, n), DEV, -1.0, 1.0).float()
    want, gate = R.splitk_reduce_ref(slabs, nsplit, n)
    out = torch.full((rows, ch), 7.0, device=DEV)
    ops.splitk_reduce(slabs, nsplit, rows, ch, out, accumulate=False)
    check(f"splitk_reduce nsplit={nsplit} rows={rows} ch={ch}", out.view(-1), want, gate)
    out0 = R.uniform(n, 5, DEV, -1.0, 1.0).float().view(rows, ch)
    want, gate = R.splitk_reduce_ref(slabs, nsplit, n, out0)
    acc = ops.splitk_reduce(slabs, nsplit, rows, ch, out0.clone(), accumulate=True)
    check(f"splitk_reduce(accumulate) nsplit={nsplit} rows={rows} ch={ch}", acc.view(-1), want, gate)
    # the form that also emits the column statistics: no ops wrapper of its own (ops.gemm_slabs calls it), so through the C ABI
    out2 = torch.full((rows, ch), 7.0, device=DEV)
    stats = ops.new_stats(ch, DEV)
    _lib.check(_lib.load().pcaa_splitk_reduce_stats(slabs.data_ptr(), nsplit, n, out2.data_ptr(), stats.data_ptr(), ops.NREP,
                                                    rows, ch, ops._s()), "pcaa_splitk_reduce_stats")
    want, gate = R.splitk_reduce_ref(slabs, nsplit, n)
    check(f"splitk_reduce_stats nsplit={nsplit} rows={rows} ch={ch} values", out2.view(-1), want, gate)
    sw, sg = R.colstats_of_ref(out2)
    check(f"splitk_reduce_stats nsplit={nsplit} rows={rows} ch={ch} statistics", stats.sum(0), sw, sg)


# ===================================================================================================== Part B: Adam
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
ADAM_N = [1, 3, 4, 5, 1003, 4 * 256 * 4 * 3 + 2, 3000001]


@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
@pytest.mark.parametrize("max_blocks", [0, 2048, 1024, 64, 1])
@pytest.mark.parametrize("n", ADAM_N)
@pytest.mark.parametrize("entry", ["host_step", "device_step", "device_step_bf16_grad"])
def test_adam_against_fp64(entry, n, max_blocks, grad_scale):
    """five consecutive steps from non-zero moments; every step is compared with one fp64 step from the state the
    kernel started that step with"""
    p, _, m, v = R.adam_state(n, 0, DEV)
    step_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    coef_dev = torch.zeros(2, device=DEV)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for step in range(1, 6):
        g = R.adam_gradient(n, step, DEV)
        if entry == "device_step_bf16_grad":
            g16 = g.bfloat16()
            g = g16.float()
        ref = R.adam_ref(p, g, m, v, LR, B1, B2, EPS, step, grad_scale)
        if entry == "host_step":
            ops.adam_step_(p, g, m, v, LR, B1, B2, EPS, step, grad_scale, max_blocks)
        else:
            ops.adam_advance_(step_dev, coef_dev, LR, B1, B2)
            if entry == "device_step":
                ops.adam_step_dev_(p, g, m, v, B1, B2, EPS, coef_dev, grad_scale, max_blocks)
            else:
                ops.adam_step_dev_g16_(p, g16, m, v, B1, B2, EPS, coef_dev, grad_scale, max_blocks)
        for k, t in (("p", p), ("m", m), ("v", v)):
            r = R.ratio(t, *ref[k])
            worst[k] = max(worst[k], r)
            assert r <= 1.0, (entry, n, max_blocks, grad_scale, step, k, r)
    print(f"[elementwise] adam {entry} n={n} max_blocks={max_blocks} grad_scale={grad_scale}: worst |err| / gate over 5 steps: "
          + ", ".join(f"{k} {x:.3f}" for k, x in worst.items()))


def _adam_run(n, steps, fn):
    p, _, m, v = R.adam_state(n, 0, DEV)
    for step in range(1, steps + 1):
        fn(p, R.adam_gradient(n, step, DEV), m, v, step)
    return p, m, v


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("n", ADAM_N)
def test_adam_kernels_agree_bitwise(n):
    """one arithmetic (common.h::adam_update): the one-quad kernel (default grid) and the four-quad kernel (max_blocks 64)"""
    a = _adam_run(n, 3, lambda p, g, m, v, t: ops.adam_step_(p, g, m, v, LR, B1, B2, EPS, t, 0.25, 0))
    b = _adam_run(n, 3, lambda p, g, m, v, t: ops.adam_step_(p, g, m, v, LR, B1, B2, EPS, t, 0.25, 64))
    assert _same(a, b)


@pytest.mark.parametrize("max_blocks", [0, 64])
@pytest.mark.parametrize("n", [5, 1003, 3000001])
def test_adam_device_step_equals_host_step(n, max_blocks):
    step_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    coef_dev = torch.zeros(2, device=DEV)

    def dev(p, g, m, v, t):
        ops.adam_advance_(step_dev, coef_dev, LR, B1, B2)
        assert int(step_dev) == t
        ops.adam_step_dev_(p, g, m, v, B1, B2, EPS, coef_dev, 1.0, max_blocks)

    a = _adam_run(n, 5, lambda p, g, m, v, t: ops.adam_step_(p, g, m, v, LR, B1, B2, EPS, t, 1.0, max_blocks))
    b = _adam_run(n, 5, dev)
    assert _same(a, b)


@pytest.mark.parametrize("max_blocks", [0, 64])
@pytest.mark.parametrize("n", [5, 1003, 3000001])
def test_adam_bf16_gradient_equals_widened_gradient(n, max_blocks):
    coef_dev = torch.zeros(2, device=DEV)
    step_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.adam_advance_(step_dev, coef_dev, LR, B1, B2)
    a = _adam_run(n, 3, lambda p, g, m, v, t: ops.adam_step_dev_g16_(p, g.bfloat16(), m, v, B1, B2, EPS, coef_dev, 0.25, max_blocks))
    b = _adam_run(n, 3, lambda p, g, m, v, t: ops.adam_step_dev_(p, g.bfloat16().float(), m, v, B1, B2, EPS, coef_dev, 0.25, max_blocks))
    assert _same(a, b)


@pytest.mark.parametrize("bf16_grad", [False, True])
@pytest.mark.parametrize("max_blocks", [0, 64])
@pytest.mark.parametrize("tail", [0, 1, 2, 3])
def test_adam_subrange_leaves_the_rest_untouched(tail, max_blocks, bf16_grad):
    """an update of [lo, hi) of larger buffers, lo a multiple of 4 and hi % 4 = tail: every element outside keeps its bits"""
    total, lo = 4 * 300, 16
    hi = lo + 1000 + tail
    canary = {"p": 0x4B1D0001, "m": 0x4B1D0002, "v": 0x4B1D0003}
    full = {k: t for k, t in zip("pgmv", R.adam_state(total, 1, DEV))}
    for k, bits in canary.items():
        iv = full[k].view(torch.int32)
        iv[:lo] = bits
        iv[hi:] = bits
    before = {k: full[k].clone() for k in "pmv"}
    coef_dev = torch.zeros(2, device=DEV)
    ops.adam_advance_(torch.zeros(1, dtype=torch.int32, device=DEV), coef_dev, LR, B1, B2)
    g = full["g"].bfloat16() if bf16_grad else full["g"]
    step = ops.adam_step_dev_g16_ if bf16_grad else ops.adam_step_dev_
    step(full["p"][lo:hi], g[lo:hi], full["m"][lo:hi], full["v"][lo:hi], B1, B2, EPS, coef_dev, 1.0, max_blocks)
    for k, bits in canary.items():
        iv = full[k].view(torch.int32)
        assert bool((iv[:lo] == bits).all()) and bool((iv[hi:] == bits).all()), k
    # ... and the range itself is the update of a buffer of its own
    own = {k: before[k][lo:hi].clone() for k in "pmv"}
    step(own["p"], g[lo:hi].clone(), own["m"], own["v"], B1, B2, EPS, coef_dev, 1.0, max_blocks)
    for k in "pmv":
        assert torch.equal(full[k][lo:hi], own[k]), k
        assert not torch.equal(full[k][lo:hi], before[k][lo:hi]), k


# ===================================================================================================== Part C: helpers
@pytest.mark.parametrize("cols", [1, 63, 64, 65, 333])
@pytest.mark.parametrize("rows", [1, 3, 28, 29, 32, 33, 1000])
def test_colsum(rows, cols):
    """four row lanes; the 8-deep trip runs while r + 28 < rows"""
    x = R.uniform(rows * cols, R.seed_of(rows, cols), DEV, -1.0, 1.0).float().view(rows, cols)
    xd = x.double().unsqueeze(0)
    check(f"colsum rows={rows} cols={cols}", ops.colsum(x), xd.sum(1)[0], R.sum_gate(xd, xd.abs(), 4)[0])


def _fp64_sum_gate(want, mags):
    """a sum accumulated in fp64 and rounded to fp32 once: the neighbouring fp32 value at most"""
    return 2.0 ** -23 * want.abs() + 2.0 ** -50 * mags + 1e-300


@pytest.mark.parametrize("scale", [1.0, 0.3])
@pytest.mark.parametrize("cols", [1, 63, 64, 65, 1000])
def test_rowsum(cols, scale):
    x = R.uniform(37 * cols, R.seed_of(37, cols), DEV, -1.0, 1.0).float().view(37, cols)
    s = R.f32(scale)
    check(f"rowsum cols={cols} scale={scale}", ops.rowsum(x, scale), x.double().sum(1) * s, _fp64_sum_gate(x.double().sum(1) * s, x.double().abs().sum(1) * s))


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 10 ** 6])
def test_total(n):
    x = R.uniform(n, R.seed_of(n, 1), DEV, -1.0, 1.0).float()
    s = R.f32(0.3)
    want = x.double().sum() * s
    check(f"total n={n}", ops.total(x, 0.3), want, _fp64_sum_gate(want, x.double().abs().sum() * s))


@pytest.mark.parametrize("rows,cols", [(1, 1), (5, 7), (1300, 1003)])
def test_scale_helpers(rows, cols):
    """exact fp32 products; 1 300 x 1 003 elements: three grid-stride trips of the 2 048-block grid"""
    x = R.uniform(rows * cols, 70, DEV, -2.0, 2.0).float().view(rows, cols)
    s = R.uniform(rows, 71, DEV, -2.0, 2.0).float()
    assert torch.equal(ops.scale_rows(x, s), x * s.view(rows, 1))
    assert torch.equal(ops.scale_by_device_scalar(x, s[:1]), x * s[0])


@pytest.mark.parametrize("rows,cols", [(1, 1), (70, 333), (1300, 1003)])
def test_bias_act(rows, cols):
    x = R.uniform(rows * cols, 72, DEV, -2.0, 2.0).float().view(rows, cols)
    b = R.uniform(cols, 73, DEV, -0.5, 0.5).float()
    assert torch.equal(ops.bias_act_(x.clone(), b, ACT_NONE), x + b)
    assert torch.equal(ops.bias_act_(x.clone(), None, ACT_NONE), x)
    want, gate = R.bn_act_fwd_ref(x, torch.ones(cols, device=DEV), b)
    check(f"bias_act_ ELU rows={rows} cols={cols}", ops.bias_act_(x.clone(), b, ACT_ELU), want, gate)
    want, gate = R.bn_act_fwd_ref(x, torch.ones(cols, device=DEV), torch.zeros(cols, device=DEV))
    check(f"bias_act_ ELU, no bias rows={rows} cols={cols}", ops.bias_act_(x.clone(), None, ACT_ELU), want, gate)


def test_elu_bwd_from_out():
    """ELU' from the output: 1 for a > 0, a + 1 otherwise (a = 0 included: the exponential branch's value at z = 0)"""
    n = 3 * 2048 * 256 + 5
    a = R.uniform(n, 74, DEV, -1.0, 1.0).float()
    a[::7] = 0.0
    a[1::7] = -0.0
    a[2] = -1.0
    da = R.uniform(n, 75, DEV, -2.0, 2.0).float()
    want = da * torch.where(a > 0, torch.ones_like(a), a + 1)
    assert torch.equal(ops.elu_bwd_from_out(da, a), want)
    assert torch.equal(ops.elu_bwd_from_out(da, a)[:14:7], da[:14:7])


@pytest.mark.parametrize("which,width", [("gather_rows", 4), ("gather_rows", 512), ("gather_rows_w4", 750), ("gather_rows_w4", 1),
                                         ("gather_rows_w4", 5)])
def test_gather_rows(which, width):
    """exact bytes for valid (and repeated) indices; an index of -1 or n_src zero-fills its row and raises the flag --
    defined behaviour: the kernel reads nothing out of range -- and the rows after it are still right"""
    fn = getattr(ops, which)
    n_src, n = 37, 5000
    src = R.uniform(n_src * width, 76, DEV, -1.0, 1.0).float().view(n_src, width)
    idx = (R.uniform(n, 77, DEV) * n_src).long().clamp_max(n_src - 1)
    idx[:3] = n_src - 1
    idx[3:6] = 0
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = fn(src, idx, err_flag=flag)
    assert torch.equal(out.view(torch.int32), src[idx].view(torch.int32)) and int(flag) == 0
    for bad in (-1, n_src):
        idx2 = idx.clone()
        where = [0, 17, n - 1]
        idx2[where] = bad
        flag.zero_()
        out = fn(src, idx2, err_flag=flag)
        want = src[idx2.clamp(0, n_src - 1)].clone()
        want[where] = 0.0
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), bad
        assert int(flag) == 1, bad
        out = fn(src, idx2)                 # no flag given: the rows are zero-filled all the same
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), bad


def test_pack_points_strided():
    base = R.uniform(3 * 17 * 30 * 10, 78, DEV, -1.0, 1.0).float().view(3, 17, 30, 10)
    for x in (base.permute(0, 3, 2, 1), base[:, 2:9, ::2, 1::3], base.permute(0, 2, 1, 3)[:, :, :5]):
        assert not x.is_contiguous()
        assert torch.equal(ops.pack_points(x), x.permute(0, 2, 3, 1).contiguous())


@pytest.mark.parametrize("B,K,D", [(6, 20, 8), (6, 4, 32), (300, 9, 7), (300, 7, 9)])
def test_prior_sample(B, K, D):
    """one launch sized by the larger of K and D writes both outputs"""
    z0 = R.uniform(B * D, 79, DEV, -1.0, 1.0).float().view(B, D)
    means = R.uniform(K * D, 80, DEV, -1.0, 1.0).float().view(K, D)
    gt = (R.uniform(B, 81, DEV) * K).long().clamp_max(K - 1)
    z, oh = ops.prior_sample(z0, means, gt, K)
    assert torch.equal(z, z0 + means[gt])
    assert torch.equal(oh, torch.nn.functional.one_hot(gt, K).float())


def test_rejected_arguments():
    """the host checks refuse these before any launch: the outputs keep their contents"""
    sc, sh, mu, rs = R.bn_vectors(24, 1, DEV)
    with pytest.raises(PcaaError, match="multiple of 4"):
        ops.bn_act_fwd(torch.zeros(8, 6, device=DEV), sc[:6].contiguous(), sh[:6].contiguous())
    with pytest.raises(PcaaError, match="ch=20"):
        ops.bn_act_meanpool_fwd(torch.zeros(8, 20, device=DEV), sc[:20].contiguous(), sh[:20].contiguous(), 2, 4)
    buf = {k: t for k, t in zip("pgmv", R.adam_state(65, 2, DEV))}
    before = {k: t.clone() for k, t in buf.items()}
    with pytest.raises(PcaaError, match="aligned"):
        ops.adam_step_(buf["p"][1:], buf["g"][1:], buf["m"][1:], buf["v"][1:], LR, B1, B2, EPS, 1)
    with pytest.raises(PcaaError, match="aligned"):
        ops.adam_step_(buf["p"][4:], buf["g"][4:], buf["m"][4:], buf["v"][3:-1], LR, B1, B2, EPS, 1)
    assert all(torch.equal(buf[k], before[k]) for k in "pgmv")
    src = torch.ones(5, 6, device=DEV)                 # 24-byte rows
    idx = torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="multiple of 16"):
        ops.gather_rows(src, idx)
    out = torch.full((2, 6), 3.0, device=DEV)
    rc = _lib.load().pcaa_gather_rows(src.data_ptr(), 5, 24, idx.data_ptr(), out.data_ptr(), 2, None, ops._s())
    assert rc == 1 and b"16 bytes" in _lib.load().pcaa_last_error()
    assert bool((out == 3.0).all())
