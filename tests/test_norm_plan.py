"""CPU suite for the norm-activation family's launch plans and for the float64 parity net built on them (tests/norm_cases.py,
tests/norm_ref.py, tests/test_norm_parity_gpu.py); nothing here needs a device.

  * every row of the case table gets the plan it declares from the host query (ops.norm_plan);
  * a sweep of the query finds no corner of the plan space (norm_cases.corner) without a row, and every geometry of the sweep
    keeps the plan's invariants, the workspace size among them;
  * the kink conditioning terminates on every row within 4 rounds and moves fewer than 1 % of the elements;
  * the bounds of the GPU test accept an fp32 emulation of the kernels' expressions and reject three small defects that the older
    1e-3 max-norm bar lets through."""
import ctypes

import numpy as np
import pytest
import torch

import norm_cases as nc
import norm_ref as nr
import test_norm_parity_gpu as parity
from mri_epilepsy_diagnosis_amd import _lib
from util import rel_err

@pytest.mark.parametrize("row,dtype", nc.PAIRS, ids=nc.PAIR_IDS)
def test_row_gets_its_declared_plan(row, dtype):
    got = nc.check(row, dtype)
    assert sorted(got) == sorted(row.passes())
    if dtype == "bf16":      # only the forward moves 8 channels per lane
        assert all(got[p][0] <= 4 for p in got if p != "fwd")


def test_table_covers_both_dtypes_of_the_listed_corners():
    assert sorted(nc.PLANS) == sorted((r.id, dt) for r, dt in nc.PAIRS)
    assert all(r in nc.BY_ID for r in nc.WS_ROWS)


SWEEP_C = list(range(1, 71)) + [128, 256, 260, 1024, 1028]
SWEEP_GROUPS = (1, 3, 40, 1030)


def _sweep():
    """Yields (pass name, dtype name, geometry, plan) over the geometries of the completeness sweep."""
    L = _lib.lib()
    info = _lib.NormPlanInfo()
    for c in SWEEP_C:
        for pad in range(10):
            for groups in SWEEP_GROUPS:
                for dt in ("f32", "bf16"):
                    g = _lib.NormGeom(groups, 1, c, c + pad, c + pad, 1 if groups > 1 else 0, _lib.ACT_NONE, 1, 0.0, 1e-5, 0, nc.DTYPES[dt])
                    for align in (2, 4, 8, 16):
                        for pname, pcode in nc.PASSES.items():
                            g.vox = 1
                            assert L.mri3d_norm_plan_query(ctypes.byref(g), pcode, align, ctypes.byref(info)) == 0
                            row = 8 * info.VT
                            cap = max(1, nc.MAX_BLOCKS // (info.groups * info.cy))
                            for gvox in sorted({1, row, row + 1, row * cap - 1, row * cap, row * cap + 1}):
                                if gvox < 1:
                                    continue
                                g.vox = gvox
                                assert L.mri3d_norm_plan_query(ctypes.byref(g), pcode, align, ctypes.byref(info)) == 0
                                yield pname, dt, g, (info.vec, info.CL, info.VT, info.cy, info.nblk, info.groups), info.gvox


def test_sweep_invariants_and_every_corner_has_a_row():
    L = _lib.lib()
    found = {}
    count = 0
    for pname, dt, g, plan, gvox in _sweep():
        vec, cl, vt, cy, nblk, groups = plan
        count += 1
        assert gvox == g.vox and groups == g.n
        assert cl * vt <= 256 and cy * cl * vec >= g.c and g.c % vec == 0, (pname, dt, g.c, g.x_ld, plan)
        assert vec in ((1, 4, 8) if (pname == "fwd" and dt == "bf16") else (1, 4))
        need = groups * nblk * g.c * 3 * 8 + groups * g.c * 3 * 4
        assert need <= L.mri3d_norm_workspace_bytes(ctypes.byref(g)), (pname, dt, g.n, g.c, g.vox, plan)
        found.setdefault(nc.corner(pname, dt, g.c, plan, gvox), (g.n, g.c, g.x_ld, g.vox))
    assert count > 100000
    claimed = set()
    for row, dt in nc.PAIRS:
        claimed |= nc.corners(row, dt)
    missing = sorted(k for k in found if k not in claimed)
    assert not missing, "corners (pass, dtype, vec, CL == lanes, 256 %% CL == 0, cy > 1, block class) without a row:\n  " + \
        "\n  ".join("%s e.g. (n, c, pitch, vox) = %s" % (k, found[k]) for k in missing)
    # and the table holds the block classes the issue names, in both statistics layouts
    classes = {k[6] for k in claimed}
    assert classes == {"1", "between", "capped", "clamped"}


@pytest.mark.parametrize("row,dtype", nc.PAIRS, ids=nc.PAIR_IDS)
def test_conditioning_terminates(row, dtype):
    inp = nc.make_inputs(row, dtype)            # raises when 4 rounds do not suffice
    rounds, changed = inp["conditioning"]
    assert rounds <= 4
    assert changed < 0.01 * inp["x"].numel(), (changed, inp["x"].numel())
    if row.act is not None:
        running = (inp["rm"], inp["rv"]) if row.mode == "running" else None
        u, m, _, _ = nr.pre_activation(inp["x"].double(), inp["gamma"], inp["beta"], row.mode, nc.EPS, row.group_c, running)
        assert bool((u.abs() >= nr.KINK_MARGIN * nr.U * m).all())      # no element is left out: the margin holds everywhere


# ------------------------------------------------------------------------------------------------ the bounds themselves
def _f32(t):
    return t.to(torch.float32)


def _fma32(a, b, c):
    """fp32 fma of fp32 tensors: the product of two floats is exact in float64."""
    return (a.double() * b.double() + c.double()).to(torch.float32)


def emulate(row, dtype, inp):
    """The kernels' arithmetic on the CPU, expression for expression in fp32 with float64 sums (csrc/norm.hip): what a correct
    kernel returns, up to the order of the float64 additions."""
    bf16 = dtype == "bf16"
    x, dy = inp["x"].float(), inp["dy"].float()
    n, c = x.shape[:2]
    running = (inp["rm"], inp["rv"]) if row.mode == "running" else None
    mean64, var64, invstd64, cnt = nr.statistics(x.double(), row.mode, nc.EPS, row.group_c, running)
    mu = _f32(mean64)
    is_ = torch.rsqrt(inp["rv"].reshape(1, c, 1, 1, 1) + np.float32(nc.EPS)) if row.mode == "running" else _f32(invstd64)
    one = torch.ones(1, c, 1, 1, 1)
    gm = inp["gamma"].reshape(1, c, 1, 1, 1) if inp["gamma"] is not None else one
    bt = inp["beta"].reshape(1, c, 1, 1, 1) if inp["beta"] is not None else 0 * one
    al = nr.slopes(row.act, inp["alpha"], nc.SLOPE, c)
    al = one if al is None else _f32(al)
    store = (lambda t: t.to(torch.bfloat16).double()) if bf16 else (lambda t: t.double())
    # forward
    sc = gm * is_
    sh = bt - mu * sc
    u = _fma32(x, sc.expand_as(x), sh.expand_as(x))
    y = u if row.act is None else torch.where(u > 0, u, u * al)
    # backward
    xh = (x - mu) * is_
    ub = _fma32(gm.expand_as(x), xh, bt.expand_as(x))
    pos = ub > 0 if row.act is not None else torch.ones_like(ub, dtype=torch.bool)
    du = torch.where(pos, dy, dy * al)
    per = (2, 3, 4) if row.mode in ("instance", "group") else (0, 2, 3, 4)
    s0 = _f32(du.double().sum(per, keepdim=True))
    s1 = _f32((du.double() * xh.double()).sum(per, keepdim=True))
    s2 = _f32(torch.where(pos, torch.zeros_like(ub).double(), dy.double() * ub.double()).sum(per, keepdim=True))
    out = dict(y=store(y))
    out["dbeta"] = _f32(s0.double().sum(0).reshape(-1)).double()
    out["dgamma"] = _f32(s1.double().sum(0).reshape(-1)).double()
    if row.act == "prelu":
        ta = s2.double().sum(0).reshape(-1)
        out["dalpha"] = _f32(ta.sum().reshape(1) if inp["alpha"].numel() == 1 else ta).double()
    k0 = gm * is_
    if row.mode in nc.TRAINING:
        gc = row.group_c if row.mode == "group" else 1
        inv_m = np.float32(1.0) / (np.float32(x[0, 0].numel() if row.mode != "batch" else n * x[0, 0].numel()) * np.float32(gc))
        if row.mode == "group":
            comb = lambda s: _f32((gm.double() * s.double()).reshape(n, c // gc, gc).sum(2, keepdim=True).expand(-1, -1, gc).reshape(n, c, 1, 1, 1))
            s0, s1, kk = comb(s0), comb(s1), is_
        else:
            kk = k0
        k1, k2 = kk * s0 * inv_m, kk * s1 * inv_m
        dx = _fma32(k0.expand_as(x), du, (-k1).expand_as(x)) - xh * k2
    else:
        dx = k0 * du
    out["dx"] = store(dx)
    if row.mode == "batch":
        mo = float(np.float32(nc.MOMENTUM))
        unb = var64.reshape(-1) * (cnt / (cnt - 1.0))
        out["running_mean"] = _f32((1.0 - mo) * inp["rm"].double() + mo * mean64.reshape(-1)).double()
        out["running_var"] = _f32((1.0 - mo) * inp["rv"].double() + mo * unb).double()
    return out


EMULATED = [(r, dt) for r, dt in nc.PAIRS if r.n * r.c * r.vox <= 5_000_000]


@pytest.mark.parametrize("row,dtype", EMULATED, ids=["%s-%s" % (r.id, dt) for r, dt in EMULATED])
def test_bounds_accept_an_fp32_emulation_of_the_kernels(row, dtype):
    """The rounding counts of the bounds hold for the kernels' own expressions evaluated in fp32 on the CPU, and the two
    pre-activation expressions agree on the side of every element once the inputs are conditioned."""
    inp = nc.make_inputs(row, dtype)
    ref = parity.reference_of(row, dtype, inp)
    got = emulate(row, dtype, inp)
    report = parity.compare(row, dtype, ref, got)
    print(" ".join("%s %.2f" % (name, ratio) for name, ratio, over in report))
    bad = [(name, ratio, over) for name, ratio, over in report if over]
    assert not bad, (row.id, dtype, bad)


def _small_case():
    row = nc.BY_ID["blk_between"]      # batch statistics, one shared PReLU slope, 2 x 16 x 8x8x10
    inp = nc.make_inputs(row, "f32")
    return row, inp, parity.reference_of(row, "f32", inp)


def _reference_results(ref):
    return {k: ref[k].clone() for k in ("y", "dx", "dgamma", "dbeta", "dalpha", "running_mean", "running_var")}


def _rejected(row, ref, got):
    return {name for name, ratio, over in parity.compare(row, "f32", ref, got) if over}


def test_bounds_accept_the_reference_itself():
    row, inp, ref = _small_case()
    assert _rejected(row, ref, _reference_results(ref)) == set()


def test_bounds_reject_a_mean_off_by_64_fp32_ulps():
    row, inp, ref = _small_case()
    x, dy = inp["x"].double(), inp["dy"].double()
    c = row.c
    mean = ref["mean"].clone()
    mean[0, 0] += 64.0 * float(np.spacing(np.float32(abs(float(mean[0, 0, 0, 0, 0])))))
    g, b, al = nr._bc(inp["gamma"], c), nr._bc(inp["beta"], c), nr._bc(inp["alpha"], c)
    u = g * (x - mean) * ref["invstd"] + b
    got = _reference_results(ref)
    got["y"] = torch.where(u > 0, u, al * u)
    assert "y" in _rejected(row, ref, got)
    assert rel_err(got["y"], ref["y"]) < 1e-3          # the max-norm bar of the older tests lets it through


def test_bounds_reject_a_voxel_row_dropped_from_the_sums():
    row, inp, ref = _small_case()
    du, xhat = ref["du"], ref["xhat"]
    d0, d1 = du[1, :, 3, 4, 5], (du * xhat)[1, :, 3, 4, 5]          # the dropped row's terms, per channel
    got = _reference_results(ref)
    got["dbeta"] = ref["dbeta"] - d0
    got["dgamma"] = ref["dgamma"] - d1
    s0 = ref["S0"].reshape(1, -1, 1, 1, 1) - d0.reshape(1, -1, 1, 1, 1)
    s1 = ref["S1"].reshape(1, -1, 1, 1, 1) - d1.reshape(1, -1, 1, 1, 1)
    got["dx"] = ref["k0"] * du - ref["k0"] * s0 / ref["count"] - xhat * (ref["k0"] * s1 / ref["count"])
    assert {"dbeta", "dgamma", "dx"} <= _rejected(row, ref, got)
    # in dx the defect is one part in the number of voxels per channel: the max-norm bar of the older tests, 1e-3 of the largest
    # element, sees it at this size (1280 voxels) only just, and not at all in a volume a few times larger
    assert rel_err(got["dx"], ref["dx"]) < 5.0 / (row.n * row.vox)


def test_bounds_reject_the_other_side_of_the_kink():
    """An element at the kink (pre-activation -1e-9 * M, far inside what either kernel expression resolves) that the backward puts on
    the positive side, as the forward expression may: its term dy * u is too small to show in dalpha — the reason a tight gradient bar
    cannot exist without the kink margin — but du changes by dy * (1 - alpha), which the bounds of dx and dbeta reject."""
    row = nc.BY_ID["blk_between"]
    inp = nc.make_inputs(row, "f32")
    x = inp["x"].double().clone()
    c = row.c
    g = nr._bc(inp["gamma"], c)
    i = (1, 2, 3, 4, 5)
    for _ in range(8):      # the statistics move with the element: a few Newton steps
        u, m, mean, invstd = nr.pre_activation(x, inp["gamma"], inp["beta"], row.mode, nc.EPS)
        x[i] -= (u[i] + 1e-9 * m[i]) / (g[0, i[1], 0, 0, 0] * invstd[0, i[1], 0, 0, 0])
    ref = nr.norm_act_ref(x, inp["dy"].double(), inp["gamma"], inp["beta"], inp["alpha"], row.mode, row.act, nc.SLOPE, nc.EPS, 0,
                          (inp["rm"], inp["rv"]), nc.MOMENTUM)
    ref["alpha"] = inp["alpha"]
    assert -1e-6 < float(ref["u"][i]) < 0 and not bool(ref["pos"][i])
    al = float(inp["alpha"])
    delta = float(inp["dy"][i]) * (1.0 - al)              # du with the element on the positive side, minus du
    got = _reference_results(ref)
    got["dalpha"] = ref["dalpha"] - float(inp["dy"][i]) * float(ref["u"][i])
    got["dbeta"] = ref["dbeta"].clone()
    got["dbeta"][i[1]] += delta
    got["dx"] = ref["dx"].clone()
    got["dx"][i] += float(ref["k0"][0, i[1], 0, 0, 0]) * delta
    rejected = _rejected(row, ref, got)
    assert "dalpha" not in rejected and {"dbeta", "dx"} <= rejected
    assert rel_err(got["dalpha"], ref["dalpha"]) < 1e-3
