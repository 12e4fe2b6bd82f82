"""Two places where the fp32 3x3x3 MFMA kernels carry work that is easy to get subtly wrong when it is packed tighter, each against
torch's CPU conv in float64 on the same inputs, at the project's fp32 bar (2e-5 of the reference's max-norm, tests/test_fuzz_gpu.py).

A. The SINGLE tap group of the tiled forward / data-gradient kernel (conv_mfma.hip: tap (2,2,2) of the image the kernel reads, i.e.
   tap (0,0,0) of the weights in the data gradient): its eight channels sit in other k-slots than those of every other group, its
   voxel fragment is two floats at the far corner of the halo tile.  Weight sets that have ONLY that tap give every
   (co, ci) a value of its own, so a wrong channel-to-k-slot map or chunk offset is a wrong number, not noise; weight sets that lack
   only that tap show that nothing else moved.  The volumes are ragged in d, h and w (zero fill at the halo's far corner), inputs and
   gradients are channel slices whose neighbours hold junk.
B. dbias of wgrad6 / wgrad3<float> (conv_mfma_wgrad.hip), one more accumulator next to the tap groups (DESIGN.md §4.13 says why it
   still rides on the MFMA): dy that lives only on the volume's faces (a halo voxel or a zero-filled piece leaking into the sum
   changes it), and random dy next to junk pad channels; db and dw, and for eight output channels (duplicate columns) that db is
   not doubled.

Every case is a pinned case of tests/conv_cases.py; its routes are asserted with the real pointers before anything is launched."""
import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc
from mri_epilepsy_diagnosis_amd import ops

pytestmark = pytest.mark.gpu

TOL = 2e-5     # fp32 bar of the project: |a - ref| <= TOL * max|ref|
JUNK = 1.0e4   # what the neighbouring channels of a slice hold


def _by_id(table, cid):
    (case,) = [c for c in table.cases if table.ids(c) == cid]
    return case


def _buffers(case, x, dy):
    """x and dy as the channel slices of `_run_conv_case` (tests/test_fuzz_gpu.py), the other channels of both buffers junk."""
    nb, ci, co, d, h, w, pad_in, pad_out, _ = case
    xbuf = torch.full((nb, ci + pad_in, d, h, w), JUNK, device="cuda").contiguous(memory_format=torch.channels_last_3d)
    xbuf[:, pad_in:] = x.cuda()
    dybuf = torch.full((nb, co + pad_out, d, h, w), -JUNK, device="cuda").contiguous(memory_format=torch.channels_last_3d)
    dybuf[:, :co] = dy.cuda()
    return xbuf[:, pad_in:].detach().requires_grad_(True), dybuf[:, :co]


def _close(a, ref, what):
    a, ref = a.detach().double().cpu(), ref.double()
    err, scale = (a - ref).abs().max().item(), ref.abs().max().item()
    print("%s: max err %.3e, scale %.3e, ratio %.3e" % (what, err, scale, err / (scale + 1e-30)))
    assert scale > 0, "%s: the reference is all zeros, the case checks nothing" % what
    assert err <= TOL * scale, "%s: %.3e vs scale %.3e" % (what, err, scale)


# ------------------------------------------------------------------ A. the single tap group
# (table, case id, {pass: exact route}); 48 -> 16: six chunks forward, three N-blocks backward; 16 -> 8: the row-paired kernel forward
SINGLE_TAP = [
    (cc.TILED_F32, "n64_16-16_5x9x19_p0_0", {"fwd": "tiled nt1", "dgrad": "tiled nt1"}),
    (cc.TILED_F32, "n64_48-16_5x9x21_p0_8", {"fwd": "tiled nt1", "dgrad": "tiled nt1"}),
    (cc.TILED_F32, "n64_32-32_5x9x17_p8_8", {"fwd": "tiled nt2", "dgrad": "tiled nt2"}),
    (cc.TILED_F32, "n72_8-32_5x9x17_p8_0", {"fwd": "tiled nt2", "dgrad": "tiled_n8"}),
    (cc.N8_TILED, "n64_16-8_5x9x17_p8_8", {"fwd": "tiled_n8", "dgrad": "tiled nt1"}),
]
WEIGHT_SETS = ["only_tap26", "only_tap0", "all_but_tap26", "all_but_tap0"]


def _weights(kind, co, ci, g):
    w = torch.zeros(co, ci, 27)
    if kind.startswith("only"):
        distinct = 1.0 + torch.arange(ci).float()[None, :] + 0.01 * torch.arange(co).float()[:, None]
        w[:, :, 26 if kind == "only_tap26" else 0] = distinct
    else:
        w = torch.randn(co, ci, 27, generator=g) * (1.0 / (27 * ci) ** 0.5)
        w[:, :, 26 if kind == "all_but_tap26" else 0] = 0.0
    return w.reshape(co, ci, 3, 3, 3)


@pytest.mark.parametrize("kind", WEIGHT_SETS)
@pytest.mark.parametrize("table,cid,routes", SINGLE_TAP, ids=[c[1] for c in SINGLE_TAP])
def test_single_tap_group_forward_and_data_gradient(table, cid, routes, kind):
    case = _by_id(table, cid)
    nb, ci, co, d, h, w, pad_in, pad_out, seed = case
    assert cc.is_ragged(nb, d, h, w)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(nb, ci, d, h, w, generator=g)
    dy = torch.randn(nb, co, d, h, w, generator=g)
    wt = _weights(kind, co, ci, g)
    b = torch.randn(co, generator=g)
    xg, dyg = _buffers(case, x, dy)
    got = table.check(case, "f32", x=xg, dy=dyg)
    for p, name in routes.items():
        assert got[p] == name, "%s %s: routed to '%s', this test is there for '%s'" % (cid, p, got[p], name)
    wg, bg = wt.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    yg = ops.conv3d(xg, wg, bg, stride=1, padding=1)
    yg.backward(dyg)
    yr = F.conv3d(x.double(), wt.double(), b.double(), padding=1)
    dxr = F.conv_transpose3d(dy.double(), wt.double(), padding=1)
    _close(yg, yr, "y")
    _close(xg.grad, dxr, "dx")


# ------------------------------------------------------------------ B. dbias of the fp32 weight-gradient kernels
# (table, case id, exact wgrad route, eight output channels); with a bias, as every table here is
DBIAS = [
    (cc.TILED_F32, "n64_48-16_5x9x21_p0_8", "wgrad6", False),        # three ci-tiles: only the first one's bias slot is read
    (cc.TILED_F32, "n64_16-16_5x9x19_p0_0", "wgrad6", False),        # one ci-tile
    (cc.RANDOM, "n1_16-24_9x9x12_p16_0", "wgrad6", False),           # the second co-block is half empty
    (cc.RANDOM, "n1_64-8_2x13x4_p0_8", "wgrad6 co8", True),
    (cc.N8_TILED, "n64_8-8_5x9x17_p8_8", "wgrad6 ci8 co8", True),
    (cc.N8_TILED, "n64_8-16_5x9x17_p0_8", "wgrad3", False),
]
DY_PATTERNS = ["faces", "random"]


@pytest.mark.parametrize("pattern", DY_PATTERNS)
@pytest.mark.parametrize("table,cid,route,co8", DBIAS, ids=[c[1] for c in DBIAS])
def test_dbias_and_weight_gradient(table, cid, route, co8, pattern):
    case = _by_id(table, cid)
    nb, ci, co, d, h, w, pad_in, pad_out, seed = case
    assert table.bias
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(nb, ci, d, h, w, generator=g)
    dy = torch.randn(nb, co, d, h, w, generator=g)
    if pattern == "faces":   # the first and the last w column and the last h row of the volume, nothing else
        keep = torch.zeros(d, h, w, dtype=torch.bool)
        keep[:, :, 0] = keep[:, :, w - 1] = keep[:, h - 1, :] = True
        dy = dy * keep
    wt = torch.randn(co, ci, 3, 3, 3, generator=g) * (1.0 / (27 * ci) ** 0.5)
    b = torch.randn(co, generator=g)
    xg, dyg = _buffers(case, x, dy)
    got = table.check(case, "f32", x=xg, dy=dyg)
    assert got["wgrad"] == route, "%s: routed to '%s', this test is there for '%s'" % (cid, got["wgrad"], route)
    wg, bg = wt.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    ops.conv3d(xg, wg, bg, stride=1, padding=1).backward(dyg)
    dbr = dy.double().sum(dim=(0, 2, 3, 4))
    dwr = torch.nn.grad.conv3d_weight(x.double(), wt.shape, dy.double(), padding=1)
    _close(bg.grad, dbr, "db")
    _close(wg.grad, dwr, "dw")
    if co8:   # columns 8..15 of the accumulator repeat the eight channels: one copy, not the sum of both
        twice = (bg.grad.detach().double().cpu() - 2.0 * dbr).abs().max().item()
        assert twice > 0.5 * dbr.abs().max().item(), "db looks doubled"
