"""Shapes and inputs of the tissue-pass parity tests (tests/test_tissue_gpu.py) and the plan corners they have to reach
(tests/test_tissue_host.py asserts that they do).  Volumes stay below 10^5 voxels.

Every case has more than `order` voxels along every axis: with fewer the powers of a coordinate repeat (xh^3 == xh on three
points) and the normal equations of the reference's M-step are singular.  The W == 1 case therefore runs at order 0, and the
second trip of the row loop, which needs more than 32768 rows, is taken at order 2 on rows of three voxels."""
import functools

import numpy as np

import tissue_ref as R

# name: (shape, classes, order, mask kind)
CASES = {
    "w37_odd_rows": ((5, 7, 37), 3, 3, "blob"),          # one partial wave step; 35 rows: the last block has 3
    "w64_full_step": ((6, 6, 64), 2, 2, None),          # exactly one full wave step, no mask
    "w65_one_lane": ((5, 5, 65), 4, 1, "rows"),         # a second step of one lane; whole rows masked out
    "w130_specials": ((7, 6, 130), 3, 3, "specials"),   # three steps; NaN, inf, 0 and negative voxels inside the mask
    "w1_two_trips": ((182, 181, 1), 3, 0, None),        # one voxel per row, 32942 rows: more than 8192 blocks x 4 rows
    "two_trips_quadratic": ((130, 253, 3), 2, 2, "blob"),   # the row loop's second trip with a field that varies along the row
    "order0_four": ((4, 9, 40), 4, 0, "blob"),
    "empty_mask": ((5, 7, 37), 3, 3, "empty"),
}
ITERATIONS = (0, 1, 5)


def volume(shape, seed):
    """A three-tissue image times a smooth field, float32, every voxel > 0."""
    xh, yh, zh = R.coordinates(shape)
    d, h, w = np.meshgrid(xh, yh, zh, indexing="ij")
    s = np.sin(5 * d + 1) * np.cos(4 * h + 0.5) + np.sin(6 * w + 2 + 3 * d) + 0.5 * np.sin(7 * h * w + 2 * d)
    q = np.quantile(s, [0.3, 0.65])
    img = np.asarray(R.CLASS_INTENSITY)[(s > q[0]).astype(int) + (s > q[1])] + 0.04 * np.random.default_rng(seed).standard_normal(shape)
    coef = np.random.default_rng(50 + seed).uniform(-0.3, 0.3, 20)
    coef[0] = 0.0
    return (np.maximum(img, 1e-3) * np.exp(R.field_log(shape, coef, 3))).astype(np.float32), s


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(x float32, mask uint8 or None) of a case."""
    shape, _classes, _order, kind = CASES[name]
    seed = sorted(CASES).index(name)
    x, s = volume(shape, seed)
    if kind is None:
        return x, None
    mask = (s > np.quantile(s, 0.15)).astype(np.uint8)
    if kind == "empty":
        mask[:] = 0
    if kind == "rows":
        mask.reshape(-1, shape[2])[::3] = 0
        mask[mask != 0] = 7            # any non-zero byte selects
    if kind == "specials":
        flat, inside = x.reshape(-1), np.flatnonzero(mask.reshape(-1))
        pick = np.random.default_rng(9).choice(inside, 40, replace=False)
        flat[pick[:10]] = np.nan
        flat[pick[10:20]] = np.inf
        flat[pick[20:30]] = 0.0
        flat[pick[30:]] = -0.5
    return x, mask


@functools.lru_cache(maxsize=None)
def reference(name):
    """{iteration: (params, sums, magnitudes)} for the parameters after 0, 1 and 5 reference iterations, computed once."""
    shape, K, order, kind = CASES[name]
    x, mask = inputs(name)
    if kind == "empty":
        p = np.concatenate([[0.2, 0.3, 0.5], [-1.2, -0.5, 0.0], [0.05, 0.04, 0.03], np.linspace(-0.2, 0.2, R.ncoef(order))])
        return {0: (p,) + R.em_sums(x, mask, K, order, p)}
    sel = R.selected(x, mask)
    params, v_floor = R.initial(np.log(x[sel].astype(np.float64)), K, order)
    out = {}
    for it in range(max(ITERATIONS) + 1):
        sums, mag = R.em_sums(x, mask, K, order, params)
        if it in ITERATIONS:
            out[it] = (params, sums, mag)
        params = R.update(params, sums, K, order, v_floor)
    return out


def bound(n, mag):
    """Per entry: two float64 summations of n terms in different orders, and a few ulp on an exp argument of at most 745 (4x)."""
    return (n * 2.0 ** -52 + 2.0 ** -40) * mag
