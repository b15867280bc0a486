"""The eval-mode BatchNorm + ELU backward kernels (csrc/elementwise.hip: pcaa_bn_eval_act_bwd, pcaa_bn_eval_bwd_finalize,
pcaa_bn_eval_moments) through the C ABI against their fp64 restatement (tests/eval_bwd_ref.py; its gates are shown
reference-safe and defect-sensitive on the CPU by tests/test_eval_bwd_gates_cpu.py, at these very inputs).

    branch                                                              where
    ------------------------------------------------------------------  -------------------------------------------
    rows 1 / 127 / 129 / 300: below, astride, beyond one 128-row        every test_eval_act_bwd case
      workgroup (a lane's four-row trip cut short, a second workgroup)
    ch 4 / 64 / 512 / 1024: 256 row lanes per workgroup ... 1           every test_eval_act_bwd case
    fp32 / bf16 storage                                                 the dtype parameter
    da form, out of place and in place over da                          forms "da", "da in place"
    pooled form, group_rows 1 / 30 / 32 / 150: groups that end          forms "pool 1" ... "pool 150"
      inside, at and across workgroup boundaries
    finalize: fresh destinations / caller-given ones, no dbias          test_eval_bwd_finalize
    host-side argument checks                                           test_rejected_arguments

Every output element is compared (dy whole, both statistics of every channel), and the rows behind the tensor's end
are checked to be untouched.  Every comparison prints ``worst |err| / gate``; the assertion is ``<= 1``.
"""
import pytest
import torch

import elementwise_ref as R
import eval_bwd_ref as E
from opensetgaitrecognition_pcaa_amd import _lib, ops
from opensetgaitrecognition_pcaa_amd.ops import NREP, _p, _s

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
GUARD = 3          # rows behind dy's end that must stay as they were


def check(name, got, want, gate):
    err = (got.double() - want).abs() / gate.clamp_min(1e-300)
    r = float(err.max())
    print(f"[eval-bwd] {name}: worst |err| / gate = {r:.3f}")
    assert r <= 1.0, (name, r)


def case_inputs(rows, ch, gr, dtype, pooled):
    """as tests/test_eval_bwd_gates_cpu.py::case_inputs, on the device (the hash generator gives the same bits)"""
    seed = R.seed_of(ch, rows * 1009 + gr)
    y = R.activations(rows, ch, dtype, seed, DEV)
    sc, sh, mu, rs = R.bn_vectors(ch, seed, DEV)
    kw = ({"dpool": R.gradient(E.pooled_groups(rows, gr), ch, F32, seed, DEV), "group_rows": gr, "pool_scale": 1.0 / gr}
          if pooled else {"da": R.gradient(rows, ch, dtype, seed, DEV)})
    return y, sc, sh, mu, rs, kw


def launch(y, sc, sh, mu, rs, dy, da=None, dpool=None, group_rows=0, pool_scale=1.0):
    rows, ch = y.shape
    stats = torch.zeros((NREP, 2, ch), dtype=torch.float64, device=DEV)
    ops.check(_lib.load().pcaa_bn_eval_act_bwd(_p(da), _p(dpool), int(group_rows), float(pool_scale), _p(y), _p(dy),
                                               ops._dt(y), _p(sc), _p(sh), _p(mu), _p(rs), _p(stats), NREP, rows, ch, _s()),
              "pcaa_bn_eval_act_bwd")
    return stats


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("ch", [4, 64, 512, 1024])
@pytest.mark.parametrize("rows", [1, 127, 129, 300])
def test_eval_act_bwd(rows, ch, dtype):
    for form in ("da", "da in place", "pool 1", "pool 30", "pool 32", "pool 150"):
        pooled = form.startswith("pool")
        gr = int(form.split()[1]) if pooled else 0
        y, sc, sh, mu, rs, kw = case_inputs(rows, ch, gr, dtype, pooled)
        z = y.double() * sc.double() + sh.double()
        assert bool((z > 0).any()) and bool((z <= 0).any()), "both ELU branches must be populated"
        ref = E.bn_eval_act_bwd_ref(y, sc, sh, mu, rs, **kw)
        buf = torch.full((rows + GUARD, ch), 7.0, dtype=dtype, device=DEV)
        if form == "da in place":
            buf[:rows] = kw["da"]
            stats = launch(y, sc, sh, mu, rs, buf, da=buf)
        else:
            stats = launch(y, sc, sh, mu, rs, buf, **kw)
        tag = f"{form} {dtype} rows={rows} ch={ch}"
        check(tag + " dy", buf[:rows], ref["dy"], R.out_gate(ref["dy_gate"], ref["dy"], dtype))
        assert bool((buf[rows:] == 7.0).all()), tag + ": wrote behind the last row"
        check(tag + " stats", stats.sum(0), ref["stats"], ref["stats_gate"])
        if not pooled and form == "da":
            # the module-facing wrapper: same launch, same bits
            dy2, stats2 = ops.bn_eval_act_bwd(y, sc, sh, mu, rs, da=kw["da"])
            assert torch.equal(dy2, buf[:rows])
            check(tag + " stats (ops)", stats2.sum(0), ref["stats"], ref["stats_gate"])


@pytest.mark.parametrize("ch", [4, 64, 512, 1024])
def test_eval_bwd_finalize(ch):
    rows = 300
    y, sc, sh, mu, rs, kw = case_inputs(rows, ch, 0, F32, False)
    _, stats = ops.bn_eval_act_bwd(y, sc, sh, mu, rs, **kw)
    ref = E.bn_eval_bwd_finalize_ref(stats, sc)          # from the kernel's own fp64 sums: same stored values
    dg, db, dbias = ops.bn_eval_bwd_finalize(stats, sc, ch)
    for k, v in (("dgamma", dg), ("dbeta", db), ("dbias", dbias)):
        check(f"finalize ch={ch} {k}", v, *ref[k])
    # caller-given destinations (views of a flat gradient buffer); what lies between them is left alone
    flat = torch.full((3 * ch + 2,), 5.0, dtype=F32, device=DEV)
    o = [flat[0:ch], flat[ch + 1:2 * ch + 1], flat[2 * ch + 2:3 * ch + 2]]
    out = ops.bn_eval_bwd_finalize(stats, sc, ch, dgamma=o[0], dbeta=o[1], dbias=o[2])
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(out, o))
    assert torch.equal(o[0], dg) and torch.equal(o[1], db) and torch.equal(o[2], dbias)
    assert float(flat[ch]) == 5.0 and float(flat[2 * ch + 1]) == 5.0
    # no dbias wanted (a BatchNorm without a bias in front of it): the other two as before
    dg2, db2 = torch.empty_like(dg), torch.empty_like(db)
    ops.check(_lib.load().pcaa_bn_eval_bwd_finalize(_p(stats), NREP, None, _p(dg2), _p(db2), None, ch, _s()), "finalize")
    assert torch.equal(dg2, dg) and torch.equal(db2, db)


@pytest.mark.parametrize("lin_bias", [False, True])
def test_eval_moments(lin_bias):
    case = R.finalize_case(100, lin_bias, DEV)
    bn = torch.nn.BatchNorm1d(100).to(DEV)
    with torch.no_grad():
        bn.running_mean.copy_(case["rm"]); bn.running_var.copy_(case["rv"])
    mean, rstd = ops.bn_eval_moments(bn, 100, case["lin_bias"])
    want_m = case["rm"].double() - (case["lin_bias"].double() if lin_bias else 0.0)
    want_r = 1.0 / torch.sqrt(case["rv"].double() + R.f32(bn.eps))
    check("bn_eval_moments mean", mean, want_m, R.U * (case["rm"].abs().double() + 0.3) + 1e-300)      # one fp32 difference
    check("bn_eval_moments rstd", rstd, want_r, 8 * R.U * want_r)          # sum, root, quotient (bn_eval_coeffs' gate)


def test_rejected_arguments():
    lib = _lib.load()
    y = torch.zeros((8, 8), device=DEV)
    v = torch.zeros(8, device=DEV)
    st = torch.zeros((NREP, 2, 8), dtype=torch.float64, device=DEV)
    dp = torch.zeros((1, 8), device=DEV)

    def call(da, dpool, yy, dy, ch=8, gr=8):
        return lib.pcaa_bn_eval_act_bwd(_p(da), _p(dpool), gr, 1.0, _p(yy), _p(dy), 0, _p(v), _p(v), _p(v), _p(v), _p(st),
                                        NREP, 8, ch, _s())
    assert call(y, dp, y, torch.empty_like(y)) == 1 and b"exactly one" in lib.pcaa_last_error()
    assert call(None, None, y, torch.empty_like(y)) == 1
    assert call(y.clone(), None, y, y) == 1 and b"alias" in lib.pcaa_last_error()
    assert call(y.clone(), None, y, torch.empty_like(y), ch=12) == 1          # 3 quads do not tile 256 threads
    assert call(None, dp, y, torch.empty_like(y), gr=0) == 1
    assert lib.pcaa_bn_eval_bwd_finalize(_p(st), NREP, None, None, None, _p(v), 8, _s()) == 1          # dbias needs scale
