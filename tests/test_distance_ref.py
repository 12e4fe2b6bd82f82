"""CPU suite: tests/distance_ref.py (the definitions the GPU suite compares csrc/distance.hip with) held to scipy.ndimage and to
torch float64 autograd, and the GPU suite's comparisons shown to see planted mistakes in the reference's own output."""
import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

import distance_cases as cases
import distance_ref as R

SHAPES = [(5, 7, 9), (12, 10, 17), (1, 20, 33)]
RADII = [1, 1.5, 2, 3]


def _masks(shape):
    rng = np.random.default_rng(sum(shape))
    out = [(rng.random(shape) < p).astype(np.uint8) for p in (0.05, 0.5, 0.95)]
    out.append(cases.pattern("ball", shape, 3))
    out.append(cases.pattern("corner_zero", shape, 4))
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_squared_edt_is_scipys(shape):
    for m in _masks(shape):
        want = np.rint(ndi.distance_transform_edt(m) ** 2).astype(np.int32)
        R.compare_exact(R.edt_sq(m[None])[0], want, "edt_sq")
        # distances inside `value`, and with the outside as zeros (one voxel of padding all round)
        R.compare_exact(R.edt_sq(m[None] * 7, value=7)[0], want, "edt_sq value")
        padded = np.rint(ndi.distance_transform_edt(np.pad(m, 1)) ** 2).astype(np.int32)[1:-1, 1:-1, 1:-1]
        R.compare_exact(R.edt_sq(m[None], outside_zero=True)[0], padded, "edt_sq outside_zero")
    assert (R.edt_sq(np.ones((1,) + shape, np.uint8)) == R.EDT_INF).all()
    assert (R.edt_sq(np.zeros((1,) + shape, np.uint8)) == 0).all()


def test_float32_root_is_the_rounded_float64_root():
    s = np.arange(1 << 20, dtype=np.int64)
    assert np.array_equal(np.sqrt(s.astype(np.float32)), np.sqrt(s.astype(np.float64)).astype(np.float32))


@pytest.mark.parametrize("radius", RADII + [6])
@pytest.mark.parametrize("shape", SHAPES)
def test_morphology_is_scipys_with_the_ball(shape, radius):
    b = R.ball(radius)
    for m in _masks(shape):
        mb = m[None]
        R.compare_exact(R.dilate(mb, radius)[0], ndi.binary_dilation(m, b).astype(np.uint8), "dilate")
        R.compare_exact(R.erode(mb, radius, 0)[0], ndi.binary_erosion(m, b, border_value=0).astype(np.uint8), "erode 0")
        R.compare_exact(R.erode(mb, radius, 1)[0], ndi.binary_erosion(m, b, border_value=1).astype(np.uint8), "erode 1")
        R.compare_exact(R.opening(mb, radius)[0], ndi.binary_opening(m, b).astype(np.uint8), "opening")
        R.compare_exact(R.closing(mb, radius)[0], ndi.binary_closing(m, b).astype(np.uint8), "closing")


def test_fill_holes_is_scipys():
    for name, m in cases.hole_masks().items():
        R.compare_exact(R.fill_holes(m), ndi.binary_fill_holes(m).astype(np.uint8), name)
    for shape in SHAPES:
        for m in _masks(shape):
            R.compare_exact(R.fill_holes(m), ndi.binary_fill_holes(m).astype(np.uint8), "fill_holes")


def _one_hot2dist(seg):
    """The paper's code (Kervadec et al., utils.py::one_hot2dist) for one volume, (K, d, h, w) booleans -> float64."""
    res = np.zeros(seg.shape, dtype=np.float64)
    for k in range(len(seg)):
        pos = seg[k].astype(bool)
        if pos.any():
            neg = ~pos
            res[k] = ndi.distance_transform_edt(neg) * neg - (ndi.distance_transform_edt(pos) - 1) * pos
    return res


@pytest.mark.parametrize("C,ids", [(2, (1,)), (3, (0, 1)), (9, (1, 2, 5)), (4, (0, 1, 2, 3))])
def test_signed_map_is_one_hot2dist(C, ids):
    rng = np.random.default_rng(C)
    y = rng.integers(0, C, (2, 6, 7, 8)).astype(np.uint8)
    y[1][y[1] == ids[-1]] = (ids[-1] + 1) % C                  # the last class is absent from the second volume
    s = R.signed_sqdist(y, C, ids)
    for n in range(2):
        want = _one_hot2dist(np.stack([y[n] == c for c in ids]))
        assert np.array_equal(R.phi(s[n]), want)
    assert (s[1, -1] == 0).all()
    # a class filling a volume has no boundary; ignored voxels are marked and count as "not the class"
    full = np.full((1, 4, 5, 6), ids[0], np.uint8)
    assert (R.signed_sqdist(full, C, ids)[0, 0] == 0).all()
    y[0, 2, 3, 4] = 255
    y[0, 2, 3, 5] = ids[0]
    s = R.signed_sqdist(y, C, ids)
    assert (s[0, :, 2, 3, 4] == R.INT32_MIN).all() and s[0, 0, 2, 3, 5] == -1
    assert (R.signed_sqdist(np.full((1, 3, 3, 3), 255, np.uint8), C, ids) == R.INT32_MIN).all()
    almost = np.full((1, 4, 5, 6), ids[0], np.uint8)
    almost[0, 0, 0, 0] = 255                                   # the class fills every counted voxel
    s = R.signed_sqdist(almost, C, ids)
    assert s[0, 0, 0, 0, 0] == R.INT32_MIN and (s[0, 0].ravel()[1:] == 0).all()


@pytest.mark.parametrize("C,ids", [(2, (1,)), (3, (0, 1)), (9, (1, 2, 5))])
def test_loss_and_gradient_are_torch_float64_autograd(C, ids):
    z, y = cases.loss_inputs(C, (5, 6, 7), 1.0, seed=C)
    s = R.signed_sqdist(y, C, ids)
    loss, grad = R.boundary_loss(z, s, ids)
    tl, tg = R.torch_loss(z, s, ids, torch.float64)
    assert abs(loss - tl) <= 1e-13 * max(1.0, abs(tl)) and np.abs(grad - tg).max() <= 1e-15
    none = np.full_like(s, R.INT32_MIN)
    loss, grad = R.boundary_loss(z, none, ids)
    assert loss == 0.0 and not grad.any()


# ------------------------------------------------------------------ the comparisons see planted mistakes
def _sees(compare, *args):
    with pytest.raises(AssertionError):
        compare(*args)


def test_comparisons_see_planted_mistakes(capsys):
    C, ids = 3, (1, 2)
    z, y = cases.loss_inputs(C, (5, 6, 7), 1.0, seed=11)
    y[0, 0, 0, :3] = 255
    s = R.signed_sqdist(y, C, ids)
    loss, grad = R.boundary_loss(z, s, ids)
    a = R.mean_abs_term(z, s, ids)
    l32, g32 = R.torch_loss(z, s, ids, torch.float32)
    e32l, e32g = abs(l32 - loss), float(np.abs(g32 - grad).max())
    R.compare_loss(l32, loss, e32l, a, "torch float32")                     # the honest float32 evaluation passes
    R.compare_grad(g32, grad, e32g, False, "torch float32")

    def loss_with(phi_of=R.phi, smap=s, denom=None, counted=None):
        e = np.exp(z - z.max(axis=1, keepdims=True))
        p = (e / e.sum(axis=1, keepdims=True))[:, list(ids)]
        counted = (smap != R.INT32_MIN) if counted is None else counted
        f = phi_of(smap)
        return float((p * f * counted).sum() / (counted.sum() if denom is None else denom))

    assert abs(loss_with() - loss) < 1e-15
    # the -1 inside dropped
    no_minus_one = lambda q: np.where(q < 0, -np.sqrt(np.abs(q.astype(np.float64))), R.phi(q)) * (q != R.INT32_MIN)  # noqa: E731
    _sees(R.compare_loss, loss_with(phi_of=no_minus_one), loss, e32l, a)
    # the sign flipped
    _sees(R.compare_loss, loss_with(phi_of=lambda q: -R.phi(q)), loss, e32l, a)
    _sees(R.compare_grad, -grad, grad, e32g, False)
    # the mean taken over C instead of K
    counted = s != R.INT32_MIN
    _sees(R.compare_loss, loss_with(denom=counted.sum() * C / len(ids)), loss, e32l, a)
    _sees(R.compare_grad, grad * len(ids) / C, grad, e32g, False)
    # ignored voxels counted (their terms taken as if the voxel were background)
    y_counted = np.where(y >= C, 0, y).astype(np.uint8)
    s_counted = R.signed_sqdist(y_counted, C, ids)
    _sees(R.compare_exact, s_counted, s)
    _sees(R.compare_loss, R.boundary_loss(z, s_counted, ids)[0], loss, e32l, a)
    _sees(R.compare_loss, loss_with(denom=s.size), loss, e32l, a)
    # the integer maps: < for <= at r^2, outside_zero swapped, distances crossing the volumes of a batch
    m = np.stack([cases.pattern("ball", (9, 10, 11), 1), cases.pattern("corner_zero", (9, 10, 11), 2)])
    for radius in RADII:
        r2 = R.r2_of(radius)
        _sees(R.compare_exact, (R.edt_sq(m, value=0) < r2).astype(np.uint8), R.dilate(m, radius))
        _sees(R.compare_exact, (R.edt_sq(m, outside_zero=True) >= r2).astype(np.uint8), R.erode(m, radius, 0))
    _sees(R.compare_exact, R.edt_sq(m, outside_zero=True), R.edt_sq(m, outside_zero=False))
    _sees(R.compare_exact, R.erode(m, 2, 1), R.erode(m, 2, 0))
    crossing = R.edt_sq(m.reshape((1, 18, 10, 11))).reshape(m.shape)       # the batch read as one tall volume
    _sees(R.compare_exact, crossing, R.edt_sq(m))
    capsys.readouterr()
