"""Plain float64 restatement of the pool and upsample family (csrc/resample.hip) on the CPU: torch / numpy only, nothing of the
package is imported.  Tensors are logical (N, C, D, H, W) float64; k, s, p, sizes and ratios are triples.  Besides each result the
functions return the magnitudes the bounds of tests/test_resample_parity_gpu.py are made of (L1 sums, term counts, coordinate
sensitivities), so that every bound comes from here and none from a kernel.

Selection rule of the pool (torch's): taps are visited in raster order (kd, kh, kw); a tap takes the window when it is the first
valid one, larger than the best so far, or NaN — so the first maximum wins, a NaN wins and the last NaN's index is kept, and
padding (which is never visited) never wins.  Inputs are fp32- or bf16-representable, so every comparison is exact in float64."""
import numpy as np
import torch

U = 2.0 ** -24


def pool_out(i, k, s, p):
    return (i + 2 * p - k) // s + 1


def _axis_taps(out, in_size, k, s, p):
    """(clamped source index, valid) of tap k for every output index of one axis"""
    i = torch.arange(out) * s - p + k
    return i.clamp(0, in_size - 1), (i >= 0) & (i < in_size)


def pool_fwd(x, k, s, p):
    """(y, tap): the window maximum and the window-local raster index (kd*KH + kh)*KW + kw of the element that gave it"""
    n, c, d, h, w = x.shape
    do, ho, wo = (pool_out(i, kk, ss, pp) for i, kk, ss, pp in zip((d, h, w), k, s, p))
    best = torch.full((n, c, do, ho, wo), -np.inf, dtype=torch.float64)
    tap = torch.zeros((n, c, do, ho, wo), dtype=torch.int64)
    seen = torch.zeros((do, ho, wo), dtype=torch.bool)
    for kd in range(k[0]):
        idd, vd = _axis_taps(do, d, kd, s[0], p[0])
        for kh in range(k[1]):
            ihh, vh = _axis_taps(ho, h, kh, s[1], p[1])
            for kw in range(k[2]):
                iww, vw = _axis_taps(wo, w, kw, s[2], p[2])
                valid = vd[:, None, None] & vh[None, :, None] & vw[None, None, :]
                if not bool(valid.any()):
                    continue
                v = x.index_select(2, idd).index_select(3, ihh).index_select(4, iww)
                take = valid & (~seen | (v > best) | torch.isnan(v))
                best = torch.where(take, v, best)
                tap = torch.where(take, torch.full_like(tap, (kd * k[1] + kh) * k[2] + kw), tap)
                seen = seen | valid
    assert bool(seen.all()), "a window without a valid tap"
    return best, tap


def pool_input_index(tap, xshape, k, s, p):
    """flat (d, h, w) index of the input element behind every tap: what F.max_pool3d(return_indices=True) returns"""
    d, h, w = xshape[2:]
    do, ho, wo = tap.shape[2:]
    kd, kh, kw = tap // (k[1] * k[2]), (tap // k[2]) % k[1], tap % k[2]
    i_d = torch.arange(do).view(do, 1, 1) * s[0] - p[0] + kd
    i_h = torch.arange(ho).view(1, ho, 1) * s[1] - p[1] + kh
    i_w = torch.arange(wo).view(1, 1, wo) * s[2] - p[2] + kw
    assert bool(((i_d >= 0) & (i_d < d) & (i_h >= 0) & (i_h < h) & (i_w >= 0) & (i_w < w)).all())
    return (i_d * h + i_h) * w + i_w


def pool_bwd(dy, tap, xshape, k, s, p, addend=None):
    """(dx, L1, T): dx = addend + the sum of dy over the windows whose tap is this voxel; L1 the sum of the terms' magnitudes and T
    their number (the addend counts as a term)."""
    n, c, d, h, w = xshape
    flat = pool_input_index(tap, xshape, k, s, p).reshape(n * c, -1)

    def scatter(v):
        return torch.zeros(n * c, d * h * w, dtype=torch.float64).scatter_add_(1, flat, v.reshape(n * c, -1)).view(n, c, d, h, w)
    dx, l1, t = scatter(dy), scatter(dy.abs()), scatter(torch.ones_like(dy))
    if addend is not None:
        dx, l1, t = dx + addend, l1 + addend.abs(), t + 1
    return dx, l1, t


# ---------------------------------------------------------------------------------------------- nearest
def nearest_index(in_size, out_size, r):
    """ATen's nearest source index in float32 arithmetic: min(floor(float32(o) * float32(r)), in - 1)"""
    o = np.arange(out_size, dtype=np.float32)
    i = np.floor(o * np.float32(r)).astype(np.int64)
    return torch.from_numpy(np.minimum(i, in_size - 1))


def nearest_fwd(x, out_size, ratios):
    idx = [nearest_index(i, o, r) for i, o, r in zip(x.shape[2:], out_size, ratios)]
    return x.index_select(2, idx[0]).index_select(3, idx[1]).index_select(4, idx[2])


def nearest_bwd(dy, in_size, ratios):
    """(dx, L1, T): the float64 sum of the fine voxels of every coarse voxel, the sum of their magnitudes, their number"""
    idx = [nearest_index(i, o, r) for i, o, r in zip(in_size, dy.shape[2:], ratios)]

    def fold(v):
        for dim in (4, 3, 2):
            shape = list(v.shape)
            shape[dim] = in_size[dim - 2]
            v = torch.zeros(shape, dtype=torch.float64).index_add_(dim, idx[dim - 2], v)
        return v
    cnt = [torch.bincount(i, minlength=m).double() for i, m in zip(idx, in_size)]
    t = (cnt[0][:, None, None] * cnt[1][None, :, None] * cnt[2][None, None, :]).expand(dy.shape[0], dy.shape[1], *in_size)
    return fold(dy), fold(dy.abs()), t


# ---------------------------------------------------------------------------------------------- trilinear
def linear_axis(in_size, out_size, r, align_corners):
    """(i0, i1, l0, l1) of one axis: the source coordinate in float64 from the fp32 ratio, r (o + 0.5) - 0.5 clamped at 0, or r o
    with corners; i0 = floor clamped to the last index, i1 the next index clamped, l1 the fraction in [0, 1]."""
    r = float(np.float32(r))
    o = np.arange(out_size, dtype=np.float64)
    src = r * o if align_corners else np.maximum(r * (o + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), in_size - 1)
    i1 = np.minimum(i0 + 1, in_size - 1)
    l1 = np.clip(src - i0, 0.0, 1.0)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(1.0 - l1), torch.from_numpy(l1)


def _bc(v, dim):
    shape = [1] * 5
    shape[dim] = -1
    return v.view(shape)


def _interp(x, dim, ax, weighted=True):
    i0, i1, l0, l1 = ax
    a, b = x.index_select(dim, i0), x.index_select(dim, i1)
    return _bc(l0, dim) * a + _bc(l1, dim) * b if weighted else (b - a).abs()


def trilinear_fwd(x, out_size, ratios, align_corners, sensitivity=True):
    """(y, A, (G_d, G_h, G_w)): the 8-tap sum with float64 weights; A = sum |w_i| |x_i|; G_a = sum over the taps of the two other axes
    of |w_other| |x(i1_a) - x(i0_a)|: the magnitude of dy / d(source coordinate of axis a) (None where it is not asked for)."""
    axes = [linear_axis(i, o, r, align_corners) for i, o, r in zip(x.shape[2:], out_size, ratios)]

    def all_axes(v, skip=None):
        for dim in (2, 3, 4):
            if dim != skip:
                v = _interp(v, dim, axes[dim - 2])
        return v
    g = tuple(all_axes(_interp(x, dim, axes[dim - 2], weighted=False), skip=dim) for dim in (2, 3, 4)) if sensitivity else None
    return all_axes(x), all_axes(x.abs()), g


def _interp_t(v, dim, in_size, ax, weighted=True):
    i0, i1, l0, l1 = ax
    shape = list(v.shape)
    shape[dim] = in_size
    out = torch.zeros(shape, dtype=torch.float64)
    if weighted:
        return out.index_add_(dim, i0, _bc(l0, dim) * v).index_add_(dim, i1, _bc(l1, dim) * v)
    # |d weight / d coordinate| = 1 on both taps of an output index whose taps differ (a clamped pair has the constant weight 1)
    live = _bc((i0 != i1).double(), dim) * v
    return out.index_add_(dim, i0, live).index_add_(dim, i1, live)


def trilinear_bwd(dy, in_size, ratios, align_corners, sensitivity=True):
    """(dx, L1, T, (G_d, G_h, G_w)): the exact transpose of trilinear_fwd as a float64 scatter-add; L1 = sum |w| |dy| and T the
    number of fine voxels with a non-zero weight on the coarse voxel; G_a the magnitude of d dx / d(source coordinates of axis a)."""
    axes = [linear_axis(i, o, r, align_corners) for i, o, r in zip(in_size, dy.shape[2:], ratios)]

    def all_axes(v, skip=None):
        for dim in (4, 3, 2):
            v = _interp_t(v, dim, in_size[dim - 2], axes[dim - 2], weighted=dim != skip)
        return v
    cnt = []
    for (i0, i1, l0, l1), m in zip(axes, in_size):
        second = (l1 > 0) & ~((i0 == i1) & (l0 > 0))     # an output index with both taps on one source index counts once
        cnt.append((torch.bincount(i0[l0 > 0], minlength=m) + torch.bincount(i1[second], minlength=m)).double())
    t = (cnt[0][:, None, None] * cnt[1][None, :, None] * cnt[2][None, None, :]).expand(dy.shape[0], dy.shape[1], *in_size)
    g = tuple(all_axes(dy.abs(), skip=dim) for dim in (2, 3, 4)) if sensitivity else None
    return all_axes(dy), all_axes(dy.abs()), t, g
