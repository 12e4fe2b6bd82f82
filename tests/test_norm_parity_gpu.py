"""GPU parity of ops.norm_act (csrc/norm.hip: statistics, forward apply, training and frozen backward) with the float64 reference
tests/norm_ref.py, one test per row of tests/norm_cases.py and storage type.  Every row asserts the launch plans it is there for
(ops.norm_plan, with the real tensors' alignment) before anything is launched.

Bounds.  u = 2^-24 is the unit roundoff of fp32; every magnitude comes from the float64 reference, never from the kernel.  The
factors count the fp32 roundings of the kernel's expression (each at most u relative to the quantity rounded); no factor is fitted.

  y      |y - y64| <= 8 u M max(1, |alpha|),   M = |gamma| invstd (|x| + |mean|) + |beta|.
         The kernel forms sc = gamma*invstd, sh = beta - mean*sc, y = act(fma(x, sc, sh)).  Roundings that reach the term x*sc:
         invstd's representation, the product sc, the fma (3); that reach mean*sc: mean's and invstd's representations, sc, the
         product mean*sc, the difference sh, the fma (6); beta's share: the difference sh and the fma (2).  At most 6 on any term,
         2 more for the activation's product alpha*u and as head room for invstd of the running mode, which is an fp32 rsqrt of
         an fp32 sum rather than a rounded float64 value: 8.  alpha*u scales the whole error by |alpha|.
  dx     |dx - dx64| <= 8 u (|k0 du| + |k1| + |k2| (|x| + |mean|) invstd),  dx = k0 du - k1 - xhat k2.
         k0 du: invstd, the product k0, du = dy*alpha, the fma (4).  k1 = k0 * S0 * (1/N): invstd, k0, the fp32 store of S0, 1/N, two
         products, the fma (7).  xhat k2 with xhat = (x - mean) * invstd: mean's representation and the difference act on
         (|x| + |mean|) invstd (2), invstd and the product (2), k2 as k1 without the fma (6) — the terms of k2 and of xhat do not
         add on one quantity: at most 8 on |k2| (|x| + |mean|) invstd with the two final roundings.  Frozen statistics: k1 = k2 = 0.
  bf16   y and dx add 2^-8 |y64| (|dx64|): one bf16 ulp — half an ulp of storage rounding, and the case where the fp32 result lies
         on the other side of a rounding boundary.  The reference is evaluated on the bf16-rounded inputs.
  dbeta  |dbeta - ref| <= 4 u sum|du|: du = dy*alpha (1), float64 accumulation, the fp32 store of the per-group sum (1) and of the
         result (1): 3, bounded by 4.
  dgamma |dgamma - ref| <= 8 u sum(|du| (|x| + |mean|) invstd): xhat carries mean's representation, the difference, invstd and the
         product (4), du (1), the two fp32 stores (2): 7, bounded by 8.
  dalpha |dalpha - ref| <= 8 u sum over the negative side of |dy| M (over all channels for one shared slope): the pre-activation
         of the backward, fma(gamma, xhat, beta), carries xhat's 4 and the fma (5), the two fp32 stores (2): 7, bounded by 8.
  running statistics: <= 4 u relative — float64 sums rounded once, then one float64 update rounded to fp32.

The sums S0, S1 inside dx and the parameter gradients are sums of terms of both signs: their bounds are relative to the L1 sum
of the terms (what the rounding errors scale with), not to the value.  The gradient bounds need the kink margin of
norm_ref.condition: forward and backward kernels form the pre-activation by different expressions, each within 8 u M of float64, so
an input within that distance of the kink may be given different sides; the rows' inputs keep 64 u M, and no element is excluded.

Printed per tensor, not asserted: the kernel's max-norm error and torch-CPU-fp32's against the same reference (DESIGN.md quotes
the worst ratios)."""
import pytest
import torch

import norm_cases as nc
import norm_ref as nr
from util import rel_err

U = nr.U
BF16_ULP = 2.0 ** -8
DIAG_MAX_ELEMENTS = 1 << 20      # the torch-CPU-fp32 diagnostic is skipped above this size (it would dominate the test's time)


def bounds(row, dtype, ref):
    """{tensor: (reference, elementwise bound)} of the row's results, all float64."""
    bf = BF16_ULP if dtype == "bf16" else 0.0
    c = row.c
    if row.act == "prelu":
        amax = nr._bc(ref["alpha"], c).abs().clamp_min(1.0)
    else:
        amax = 1.0
    out = {"y": (ref["y"], bf * ref["y"].abs() + 8.0 * U * ref["M"] * amax),
           "dx": (ref["dx"], bf * ref["dx"].abs() + 8.0 * U * ref["dx_bound_scale"])}
    if row.grads and row.affine:
        out["dbeta"] = (ref["dbeta"], 4.0 * U * ref["l1_du"])
        out["dgamma"] = (ref["dgamma"], 8.0 * U * ref["l1_dgamma"])
    if row.grads and row.act == "prelu":
        out["dalpha"] = (ref["dalpha"], 8.0 * U * ref["l1_dalpha"])
    if "running_mean" in ref:
        out["running_mean"] = (ref["running_mean"], 4.0 * U * ref["running_mean"].abs())
        out["running_var"] = (ref["running_var"], 4.0 * U * ref["running_var"].abs())
    return out


def compare(row, dtype, ref, got):
    """[(tensor, worst error / bound, elements over the bound)] of `got` (name -> float64 CPU tensor) against the reference."""
    report = []
    for name, (want, bound) in bounds(row, dtype, ref).items():
        g = got[name].reshape(want.shape)
        err = (g - want).abs()
        over = err > bound
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.inf, 0.0))
        report.append((name, float(ratio.max()), int(over.sum())))
    return report


def to64(t):
    return None if t is None else t.detach().double().cpu().contiguous()


def reference_of(row, dtype, inp):
    ref = nc.reference(row, dtype, inp)
    ref["alpha"] = inp["alpha"]
    return ref


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row,dtype", nc.PAIRS, ids=nc.PAIR_IDS)
def test_norm_act_matches_float64_reference(row, dtype):
    inp = nc.make_inputs(row, dtype)
    ref = reference_of(row, dtype, inp)
    res, ss = nc.run_row(row, dtype, inp)
    torch.cuda.synchronize()
    got = {k: to64(v) for k, v in res.items() if v is not None}
    if ss is not None:
        ss.assert_outside_intact("%s %s: out= slice" % (row.id, dtype))
    # determinism: the same bits from a second run on fresh tensors
    res2, ss2 = nc.run_row(row, dtype, inp, plan_check=False)
    for k, v in res.items():
        if v is not None:
            assert torch.equal(v, res2[k]), "%s %s: %s differs between two runs" % (row.id, dtype, k)
    if ss2 is not None:
        ss2.assert_outside_intact("%s %s: out= slice, second run" % (row.id, dtype))
    report = compare(row, dtype, ref, got)
    for name, ratio, over in report:
        print("%s %s %-12s worst error / bound = %.3f" % (row.id, dtype, name, ratio))
    if inp["x"].numel() <= DIAG_MAX_ELEMENTS:
        cpu = nc.cpu_fp32(row, inp)
        for name in ("y", "dx", "dgamma", "dbeta", "dalpha"):
            if name in got and cpu.get(name) is not None:
                ek, ec = rel_err(got[name].reshape(ref[name].shape), ref[name]), rel_err(cpu[name].reshape(ref[name].shape), ref[name])
                print("%s %s %-12s max-norm error: kernel %.3e, torch CPU fp32 %.3e" % (row.id, dtype, name, ek, ec))
    bad = ["%s: %d elements over the bound, worst error / bound = %.3f" % (name, over, ratio) for name, ratio, over in report if over]
    assert not bad, "%s %s (%s)\n  " % (row.id, dtype, row.why) + "\n  ".join(bad)

