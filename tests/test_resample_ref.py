"""CPU suite: the float64 restatement tests/resample_ref.py against torch itself, wherever both compute the same thing exactly —
F.max_pool3d(return_indices=True) and its autograd for the pool, F.interpolate in float64 and its autograd where the source
coordinates are exact in both (x2, x4, align_corners with a dyadic ratio), and F.interpolate's nearest index on CPU fp32 bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resample_ref as rr

POOLS = [  # spatial, k, s, p
    ((8, 6, 4), (2, 2, 2), (2, 2, 2), (0, 0, 0)),
    ((7, 9, 11), (3, 3, 3), (2, 2, 2), (1, 1, 1)),
    ((5, 8, 6), (1, 2, 2), (1, 2, 2), (0, 0, 0)),
    ((8, 9, 10), (2, 2, 2), (3, 3, 3), (0, 0, 0)),
    ((8, 16, 16), (4, 8, 8), (4, 8, 8), (0, 0, 0)),
    ((9, 8, 7), (4, 4, 4), (2, 2, 2), (2, 2, 2)),
]


def _values(kind, shape, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "ties":
        return torch.randint(0, 8, shape, generator=g).double() * 0.5 - 2.0
    x = torch.randn(shape, generator=g).float().double()
    if kind == "nan":
        x[torch.rand(shape, generator=g) < 0.05] = float("nan")
    if kind == "neginf":
        x[:, :, : shape[2] // 2] = -np.inf
    if kind == "negative":
        x = -x.abs() - 1.0
    return x


@pytest.mark.parametrize("kind", ["normal", "ties", "nan", "neginf", "negative"])
@pytest.mark.parametrize("sp,k,s,p", POOLS)
def test_pool_is_torch_max_pool3d_in_float64(sp, k, s, p, kind):
    x = _values(kind, (2, 3) + sp, 1)
    y, tap = rr.pool_fwd(x, k, s, p)
    xt = x.clone().requires_grad_(True)
    yt, it = F.max_pool3d(xt, k, s, p, return_indices=True)
    assert torch.equal(y.view(torch.int64), yt.detach().view(torch.int64))
    assert torch.equal(rr.pool_input_index(tap, x.shape, k, s, p), it)
    assert int(tap.max()) < k[0] * k[1] * k[2]
    dy = _values("normal", tuple(y.shape), 2)
    addend = _values("normal", tuple(x.shape), 3)
    dx, l1, t = rr.pool_bwd(dy, tap, x.shape, k, s, p)
    yt.backward(dy)
    assert torch.allclose(dx, xt.grad, rtol=0, atol=1e-13)
    assert torch.equal(t, rr.pool_bwd(torch.ones_like(dy), tap, x.shape, k, s, p)[0])
    assert bool((l1 >= dx.abs() - 1e-13).all())
    dxa, l1a, ta = rr.pool_bwd(dy, tap, x.shape, k, s, p, addend)
    assert torch.equal(dxa, dx + addend) and torch.equal(ta, t + 1) and torch.equal(l1a, l1 + addend.abs())


EXACT = [  # in, out, scale_factor or None (size given), align_corners
    ((3, 4, 5), (6, 8, 10), 2.0, False),
    ((1, 4, 5), (2, 8, 10), 2.0, False),
    ((3, 2, 5), (12, 8, 20), 4.0, False),
    ((5, 3, 9), (9, 9, 17), None, True),      # (in - 1) / (out - 1) = 1/2, 1/4, 1/2
    ((5, 3, 1), (1, 9, 4), None, True),       # an output extent of 1, an input extent of 1
]


def _ratios(in_sz, out_sz, sf, ac):
    if ac:
        return [(i - 1) / (o - 1) if o > 1 else 0.0 for i, o in zip(in_sz, out_sz)]
    return [1.0 / sf if sf else i / o for i, o in zip(in_sz, out_sz)]


@pytest.mark.parametrize("in_sz,out_sz,sf,ac", EXACT)
def test_trilinear_is_torch_interpolate_in_float64(in_sz, out_sz, sf, ac):
    x = _values("normal", (2, 3) + in_sz, 4)
    ratios = _ratios(in_sz, out_sz, sf, ac)
    y, a, g = rr.trilinear_fwd(x, out_sz, ratios, ac)
    xt = x.clone().requires_grad_(True)
    yt = F.interpolate(xt, size=out_sz, mode="trilinear", align_corners=ac) if sf is None else \
        F.interpolate(xt, scale_factor=sf, mode="trilinear", align_corners=ac)
    assert torch.allclose(y, yt.detach(), rtol=0, atol=1e-13)
    assert bool((a >= y.abs() - 1e-13).all()) and all(tuple(v.shape) == tuple(y.shape) and bool((v >= 0).all()) for v in g)
    dy = _values("normal", tuple(y.shape), 5)
    dx, l1, t, gb = rr.trilinear_bwd(dy, in_sz, ratios, ac)
    yt.backward(dy)
    assert torch.allclose(dx, xt.grad, rtol=0, atol=1e-12)
    if (in_sz, sf) == ((3, 4, 5), 2.0):     # x2: a coarse voxel gathers fine 2i-1 .. 2i+2 per axis, one fewer at either border
        assert t[0, 0, 1, 1, 1] == 64 and t[0, 0, 0, 0, 0] == 27 and t[0, 0, 2, 3, 4] == 27 and t[0, 0, 1, 0, 2] == 48
    assert bool(((t >= 1) | (dx == 0)).all()) and bool((l1 >= dx.abs() - 1e-12).all()) and all(bool((v >= 0).all()) for v in gb)


@pytest.mark.parametrize("in_sz,out_sz,sf", [((3, 4, 5), (6, 8, 10), 2.0), ((3, 2, 5), (12, 8, 20), 4.0), ((4, 5, 6), (9, 11, 13), None),
                                             ((7, 3, 9), (7, 7, 7), None)])
def test_nearest_is_torch_interpolate(in_sz, out_sz, sf):
    x = _values("normal", (2, 3) + in_sz, 6)
    ratios = _ratios(in_sz, out_sz, sf, False)
    xt = x.float().requires_grad_(True)
    yt = F.interpolate(xt, size=out_sz, mode="nearest") if sf is None else F.interpolate(xt, scale_factor=sf, mode="nearest")
    y = rr.nearest_fwd(x, out_sz, ratios)
    assert torch.equal(y, yt.detach().double())
    dy = _values("ties", tuple(y.shape), 7)            # small dyadic values: the fp32 sums of autograd are exact
    dx, l1, t = rr.nearest_bwd(dy, in_sz, ratios)
    yt.backward(dy.float())
    assert torch.equal(dx, xt.grad.double())
    assert torch.equal(t, rr.nearest_bwd(torch.ones_like(dy), in_sz, ratios)[0]) and bool((l1 >= dx.abs()).all())


def test_nearest_index_is_atens_bit_for_bit_over_all_extents_to_40():
    for i in range(1, 41):
        x = torch.arange(i, dtype=torch.float32).view(1, 1, i, 1, 1)
        for o in range(1, 41):
            want = F.interpolate(x, size=(o, 1, 1), mode="nearest").flatten().long()
            assert torch.equal(rr.nearest_index(i, o, i / o), want), (i, o)


def test_trilinear_transpose_is_the_adjoint_of_the_forward_at_inexact_coordinates():
    """<fwd(x), dy> = <x, bwd(dy)> in float64 for a scale of 1.5, a down-sizing and corners, where torch's own double coordinate
    differs from the one made from the fp32 ratio"""
    for in_sz, out_sz, sf, ac in (((4, 5, 6), (6, 7, 9), 1.5, False), ((9, 11, 13), (4, 5, 6), None, False), ((5, 6, 4), (10, 12, 8), None, True)):
        x, dy = _values("normal", (1, 2) + in_sz, 8), _values("normal", (1, 2) + out_sz, 9)
        ratios = _ratios(in_sz, out_sz, sf, ac)
        y = rr.trilinear_fwd(x, out_sz, ratios, ac)[0]
        dx = rr.trilinear_bwd(dy, in_sz, ratios, ac)[0]
        assert abs(float((y * dy).sum() - (x * dx).sum())) < 1e-11
        kw = dict(size=out_sz) if sf is None else dict(scale_factor=sf)
        yt = F.interpolate(x, mode="trilinear", align_corners=ac, **kw)
        assert torch.allclose(y, yt, rtol=0, atol=1e-5)       # torch's double ratio against the fp32 one: close, not equal
