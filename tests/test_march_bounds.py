"""CPU suite that keeps the bounds of the marching-kernel parity suite honest (tests/march_ref.py; tests/test_march_parity_gpu.py):
the float64 reference agrees with the definition and with torch's other float64 operators; an fp32 emulation in the kernel's order
of summation (tests/march_emu.py) stays inside the bounds for every row, type and pass; and each of ten deliberate errors — the
ones the kernel's corners can make — leaves the bounds on the rows named here."""
import pytest
import torch
import torch.nn.functional as F

import march_cases as mc
import march_emu as emu
import march_ref as mr
import march_run as run

ROWS = {r.id: r for r in mc.ROWS}


def _by_definition(x, w, b):
    """y and A of Conv3d(k = 3, padding 1) as 27 shifted sums in float64: no convolution operator"""
    n, ci, D, H, W = x.shape
    xp = torch.zeros((n, ci, D + 2, H + 2, W + 2), dtype=torch.float64)
    xp[:, :, 1:-1, 1:-1, 1:-1] = x
    y = torch.zeros((n, w.shape[0], D, H, W), dtype=torch.float64)
    A = torch.zeros_like(y)
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                xs = xp[:, :, kd:kd + D, kh:kh + H, kw:kw + W]
                y += torch.einsum("ncdhw,oc->nodhw", xs, w[:, :, kd, kh, kw])
                A += torch.einsum("ncdhw,oc->nodhw", xs.abs(), w[:, :, kd, kh, kw].abs())
    if b is not None:
        y, A = y + b.view(1, -1, 1, 1, 1), A + b.abs().view(1, -1, 1, 1, 1)
    return y, A


@pytest.mark.parametrize("rid,dtype", [("tmpl-bias", "f32"), ("decode-n2-2blocks-2seg", "bf16"), ("d1", "bf16"), ("tmpl-plain", "f32")])
def test_reference_agrees_with_the_definition_and_torchs_float64_operators(rid, dtype):
    row = ROWS[rid]
    inp = run.make_inputs(row, dtype)
    x, dy, w = inp["x"].double(), inp["dy"].double(), mr.stored_weights(inp["w"], dtype)
    b = inp["b"].double() if inp["b"] is not None else None
    y, A, a, A0 = mr.forward(x, w, b)
    yd, Ad = _by_definition(x, w, b)
    assert (y - yd).abs().max() <= 1e-12 * Ad.max() and (A - Ad).abs().max() <= 1e-12 * Ad.max()
    assert torch.equal(a, F.conv3d(x, w, None, padding=1)) and torch.equal(A0, F.conv3d(x.abs(), w.abs(), None, padding=1))
    dx, L1 = mr.dgrad(dy, w, x.shape)
    assert (dx - F.conv_transpose3d(dy, w, None, padding=1)).abs().max() <= 1e-12 * L1.max()
    assert (L1 - F.conv_transpose3d(dy.abs(), w.abs(), None, padding=1)).abs().max() <= 1e-12 * L1.max()
    # the data gradient is the forward of the transposed, flipped weights: the definition again
    dxd, L1d = _by_definition(dy, w.transpose(0, 1).flip(2, 3, 4), None)
    assert (dx - dxd).abs().max() <= 1e-12 * L1d.max() and (L1 - L1d).abs().max() <= 1e-12 * L1d.max()
    if dtype == "bf16":
        assert torch.equal(w, inp["w"].to(torch.bfloat16).double()) and not torch.equal(w, inp["w"].double())
    val, bound = mr.stats(a, A0, row.ci, 8, 4)
    assert torch.equal(val[:, 0], a.sum((0, 2, 3, 4))) and torch.equal(val[:, 1], (a * a).sum((0, 2, 3, 4))) and bool((bound > 0).all())


def _emulated(row, dtype, fault=None, passes=None):
    pl = run.plans(row, dtype)
    inp = run.make_inputs(row, dtype)
    bnd = run.bounds(row, dtype, inp, pl)
    got = {}
    for p in passes or row.passes:
        if mc.runs(row, dtype, p):
            got.update(emu.emulate(row, dtype, inp, pl[p], p, fault=fault))
    return run.report({k: bnd[k] for k in got}, got)


@pytest.mark.parametrize("row,dtype", mc.PAIRS, ids=mc.IDS)
def test_fp32_emulation_in_the_kernels_order_stays_inside_the_bounds(row, dtype):
    rep = _emulated(row, dtype)
    assert {name for name, _, _ in rep} == ({"y"} if mc.runs(row, dtype, "fwd") else set()) | ({"dx"} if mc.runs(row, dtype, "dgrad") else set()) \
        | ({"stats"} if row.stats and mc.runs(row, dtype, "fwd") else set())
    for name, ratio, over in rep:
        print("%s %s %-5s emulation: worst error / bound = %.3g" % (row.id, dtype, name, ratio))
        assert over == 0 and ratio <= 1, (row.id, dtype, name, ratio, over)


# fault -> [(row, type, pass, the result that must leave its bound)]
MUST_FAIL = {
    "tap-dropped-on-a-border-voxel": [("d1", "f32", "fwd", "y"), ("d1", "bf16", "dgrad", "dx"), ("tmpl-bias", "bf16", "fwd", "y")],
    "halo-plane-missing-at-a-segment-start": [("seg-d16-2x8", "f32", "fwd", "y"), ("seg-d40-5x8", "bf16", "dgrad", "dx"),
                                              ("decode-n2-2blocks-2seg", "bf16", "fwd", "y")],
    "rotation-not-offset-by-the-first-plane": [("seg-d16-2x8", "bf16", "fwd", "y"), ("seg-d25-3x9-last7", "f32", "dgrad", "dx"),
                                               ("seg-d40-5x8", "f32", "fwd", "y")],
    "sigma-permutation-left-out": [("one-column-d5", "bf16", "fwd", "y"), ("nc12-f32", "f32", "fwd", "y"), ("nc8", "bf16", "fwd", "y"),
                                   ("nc24", "f32", "dgrad", "dx")],
    "slot-not-restarted": [("one-column-d5", "f32", "fwd", "y"), ("d3", "bf16", "dgrad", "dx"), ("wait-one-chunk-h8", "bf16", "fwd", "y")],
    "bias-added-twice": [("tmpl-bias", "f32", "fwd", "y"), ("tmpl-stats-bias", "bf16", "fwd", "y")],
    "ragged-row-in-the-statistics": [("tmpl-stats", "f32", "fwd", "stats"), ("decode-n3-stats", "bf16", "fwd", "stats"),
                                     ("split-16+16-stats", "f32", "fwd", "stats")],
    "inactive-voxel-lane-in-the-statistics": [("tmpl-stats", "bf16", "fwd", "stats"), ("decode-n3-stats", "f32", "fwd", "stats"),
                                              ("split-16+16-stats", "bf16", "fwd", "stats")],
    "half-chunk-not-zero-filled": [("half-chunk-x-pitched", "bf16", "fwd", "y"), ("kc24-x-and-y-pitched", "bf16", "dgrad", "dx"),
                                   ("split-16+8-second-pitched", "bf16", "fwd", "y")],
    "neighbouring-slice-read": [("x-pitch+8-from-ch8", "f32", "fwd", "y"), ("y-pitch+8-from-ch8", "bf16", "dgrad", "dx"),
                                ("split-16+16", "bf16", "fwd", "y"), ("one-column-d5", "f32", "dgrad", "dx")],
}


def test_every_deliberate_error_is_listed():
    assert set(MUST_FAIL) == set(emu.FAULTS) and len(emu.FAULTS) == 10


@pytest.mark.parametrize("fault", emu.FAULTS)
def test_deliberate_error_leaves_the_bounds(fault):
    for rid, dtype, p, name in MUST_FAIL[fault]:
        rep = {k: (ratio, over) for k, ratio, over in _emulated(ROWS[rid], dtype, fault=fault, passes=(p,))}
        ratio, over = rep[name]
        print("%s on %s %s %s: %s worst error / bound = %.3g, %d elements over" % (fault, rid, dtype, p, name, ratio, over))
        assert over > 0 and ratio > 1, (fault, rid, dtype, p, name, ratio)
        # and nothing but the fault does it: the same row without it is inside (test above); a statistics fault leaves y alone
        if name == "stats":
            assert rep["y"][1] == 0
