"""float64 numpy restatement of the two augmentation kernels (include/mri3d.h, "Augmentation"), for the tests only.

TorchIO is absent ("parity unpinned"): these are the project's own definitions, written independently of the HIP code —
whole-volume array arithmetic in float64 with no per-row factoring."""
import numpy as np


def bspline_axis(n, g):
    """Control-point index (n,) and the four weights (n, 4) of every voxel of an axis of extent n under g control points."""
    m = g - 3
    p = (np.arange(n, dtype=np.float64) + 0.5) * m / n
    i = np.clip(np.floor(p), 0, m - 1).astype(np.int64)
    f = p - i
    w = np.stack([(1 - f) ** 3 / 6, (3 * f ** 3 - 6 * f ** 2 + 4) / 6, (-3 * f ** 3 + 3 * f ** 2 + 3 * f + 1) / 6, f ** 3 / 6], 1)
    return i, w


def displacement(grid, shape):
    """u (3, D, H, W) float64 of one subject's control grid (3, gd, gh, gw)."""
    grid = np.asarray(grid, dtype=np.float64)
    (i_d, w_d), (i_h, w_h), (i_w, w_w) = (bspline_axis(n, g) for n, g in zip(shape, grid.shape[1:]))
    u = np.zeros((3,) + tuple(shape))
    for a in range(4):
        for b in range(4):
            for c in range(4):
                cp = grid[:, (i_d + a)[:, None, None], (i_h + b)[None, :, None], (i_w + c)[None, None, :]]
                u += cp * (w_d[:, a][:, None, None] * w_h[:, b][None, :, None] * w_w[:, c][None, None, :])
    return u


def source_coords(affine, grid, shape):
    """s (3, D, H, W) float64 for one subject: A[:, :3] o + A[:, 3] + u(o).  `affine` is used as given (pass the fp32-rounded
    matrix the device received)."""
    A = np.asarray(affine, dtype=np.float64)
    o = np.stack(np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij"))
    s = np.einsum("ab,bdhw->adhw", A[:, :3], o) + A[:, 3][:, None, None, None]
    if grid is not None:
        s = s + displacement(grid, shape)
    return s


def warp(image, label, affine, grid, pad):
    """One subject.  Returns (image_out float64 or None, label_out or None, compare_image mask, compare_label mask): the
    masks leave out voxels whose source lies within 1e-3 of the inside/outside boundary on any axis and, for the label, also
    within 1e-3 of a half-integer."""
    shape = (image if image is not None else label).shape
    s = source_coords(affine, grid, shape)
    n = np.asarray(shape, dtype=np.float64)[:, None, None, None]
    inside = np.all((s >= -0.5) & (s <= n - 0.5), axis=0)
    near_edge = np.any((np.abs(s + 0.5) < 1e-3) | (np.abs(s - (n - 0.5)) < 1e-3), axis=0)
    near_half = np.any(np.abs(s - np.floor(s) - 0.5) < 1e-3, axis=0)
    img_out = lab_out = None
    if image is not None:
        x = np.asarray(image, dtype=np.float64)
        fl = np.floor(s)
        f = s - fl
        fl = fl.astype(np.int64)
        acc = np.zeros(shape)
        for a in (0, 1):
            for b in (0, 1):
                for c in (0, 1):
                    idx = [np.clip(fl[k] + t, 0, shape[k] - 1) for k, t in enumerate((a, b, c))]
                    wgt = (f[0] if a else 1 - f[0]) * (f[1] if b else 1 - f[1]) * (f[2] if c else 1 - f[2])
                    acc += wgt * x[idx[0], idx[1], idx[2]]
        img_out = np.where(inside, acc, float(pad))
    if label is not None:
        near = np.floor(s + 0.5).astype(np.int64)
        idx = [np.clip(near[k], 0, shape[k] - 1) for k in range(3)]
        lab_out = np.where(inside, label[idx[0], idx[1], idx[2]], np.zeros((), dtype=label.dtype))
    return img_out, lab_out, ~near_edge, ~(near_edge | near_half)


def bias_field(x, coef, order):
    """x (D, H, W) * exp(P) in float64; coefficients in the nesting order i, j, k."""
    xh, yh, zh = (np.linspace(-1, 1, n) if n > 1 else np.zeros(1) for n in x.shape)
    P = np.zeros(x.shape)
    n = 0
    for i in range(order + 1):
        for j in range(order + 1 - i):
            for k in range(order + 1 - i - j):
                P += float(coef[n]) * (xh ** i)[:, None, None] * (yh ** j)[None, :, None] * (zh ** k)[None, None, :]
                n += 1
    assert n == len(coef)
    return np.asarray(x, dtype=np.float64) * np.exp(P)
