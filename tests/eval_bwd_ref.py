"""fp64 restatement of the eval-mode BatchNorm + ELU backward (csrc/elementwise.hip: pcaa_bn_eval_act_bwd and
pcaa_bn_eval_bwd_finalize), the gate of each output, and planted defects.  Built from tests/elementwise_ref.py: the
inputs, the "same stored values on both sides" rule and every gate are that file's.

    z = scale*y + shift;  dz = g ELU'(z)  (g = da, or dpool[group]*pool_scale);  dy = scale*dz
    stats = {sum_rows dz, sum_rows dz*xhat},  xhat = (y - mean)*rstd  with the RUNNING moments of the bias-free y
    dbeta = stats[0];  dgamma = stats[1];  dbias = scale*dbeta

The gates (derivations in elementwise_ref's docstring):

* dy: the ``bn_bwd_dy_fused`` gate with k0 = scale and k1 = k2 = 0 -- |dy| (rel_e + 2u) + 8u |dy| -- plus 2^-8 |want|
  for a bf16 output.
* both statistics: ``sum_gate`` over the per-workgroup partials (128 rows each, row r on lane r % lanes, fp32), which
  meet in fp64 -- the statistics gate of ``bn_act_bwd_dz``, taken with the running moments.
* the finalize: the ``bn_bwd_finalize`` gate -- fp64 arithmetic on the fp64 sums, one rounding: 2^-23 |want|.

Planted defects: elementwise_ref's "drop_last_row", "swap_quads", "next_group_grad", and two of this kernel's own:
"batch_stats" (xhat formed with the batch's own mean and rstd of y, as a train-mode kernel would, instead of the
running ones) and "zero_bias_grad" (the finalize returns dbias = 0, the train-mode value).
"""
import torch

import elementwise_ref as R

BN_EPS = 1e-5


def pooled_groups(rows, group_rows):
    """groups a pooled gradient needs for ``rows`` rows (the last group may be cut short by the tensor's end)"""
    return -(-rows // group_rows)


def bn_eval_act_bwd_ref(y, scale, shift, mean, rstd, *, da=None, dpool=None, group_rows=0, pool_scale=1.0, defect=None,
                        block_rows=128):
    """-> dict(dy, dy_gate32, stats [2, ch], stats_gate [2, ch])"""
    kw = dict(da=da, dpool=dpool, group_rows=group_rows, pool_scale=pool_scale)
    ch = y.shape[1]
    coef = torch.stack([scale, torch.zeros_like(scale), torch.zeros_like(scale)])
    el_defect = defect if defect in ("swap_quads", "next_group_grad") else None
    dy, dy_gate = R.bn_bwd_dy_fused_ref(y, scale, shift, coef, defect=el_defect, **kw)
    if defect == "batch_stats":
        yd = y.double()
        mean = yd.mean(0).float()
        rstd = (1.0 / torch.sqrt(yd.var(0, unbiased=False) + BN_EPS)).float()
    st = R.bn_act_bwd_dz_ref(y, scale, shift, mean, rstd, defect=None if defect == "batch_stats" else defect,
                             block_rows=block_rows, **kw)
    assert st["stats"].shape == (2, ch)
    return {"dy": dy, "dy_gate": dy_gate, "stats": st["stats"], "stats_gate": st["stats_gate"]}


def bn_eval_bwd_finalize_ref(stats, scale, defect=None):
    """stats fp64 [nrep, 2, ch] -> {"dbeta" | "dgamma" | "dbias": (want, gate)}"""
    s = stats.double().sum(0)
    r32 = 2.0 ** -23
    dbias = scale.double() * s[0]
    if defect == "zero_bias_grad":
        dbias = torch.zeros_like(dbias)
    return {"dbeta": (s[0], r32 * s[0].abs() + 1e-300), "dgamma": (s[1], r32 * s[1].abs() + 1e-300),
            "dbias": (dbias, r32 * (scale.double() * s[0]).abs() + 1e-300)}


def spread_stats(stats, nrep=16, seed=0):
    """[2, ch] fp64 sums -> [nrep, 2, ch] replicas that add up to them (the layout the kernels accumulate into)"""
    ch = stats.shape[1]
    w = R.uniform(nrep * 2 * ch, 900 + seed, stats.device, 0.5, 1.5).view(nrep, 2, ch)
    return (stats.unsqueeze(0) * w / w.sum(0, keepdim=True)).contiguous()
