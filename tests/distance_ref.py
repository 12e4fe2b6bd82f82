"""The definitions behind csrc/distance.hip restated with numpy, in integers and float64: the squared Euclidean distance
transform, ball morphology as its thresholds, hole filling, the signed squared-distance map of a class map, and the boundary loss
with its gradient.  tests/test_distance_ref.py holds every function here to scipy / torch float64 autograd; the GPU suite compares
the kernels with these functions (and `compare_*` are the comparisons it uses, so their power is tested on the CPU too)."""
import numpy as np

EDT_INF = 0x3f000000
INT32_MIN = -2 ** 31


def _minplus(f, axis, outside_zero):
    """out[x] = min_q f[q] + (x - q)^2 along `axis` (int64), with zeros at q = -1 and q = len when outside_zero."""
    n = f.shape[axis]
    shape = [1] * f.ndim
    shape[axis] = n
    x = np.arange(n, dtype=np.int64).reshape(shape)
    out = np.full(f.shape, np.iinfo(np.int64).max, dtype=np.int64)
    for q in range(n):
        out = np.minimum(out, np.take(f, [q], axis=axis) + (x - q) ** 2)
    if outside_zero:
        out = np.minimum(out, np.minimum((x + 1) ** 2, (n - x) ** 2))
    return out


def edt_sq(vol, value=None, outside_zero=False):
    """vol: uint8 (n, d, h, w).  int32 squared distance to the nearest zero voxel of the same volume (inside: != 0, or == value);
    EDT_INF everywhere in a volume without a zero voxel (outside_zero False)."""
    vol = np.asarray(vol)
    assert vol.ndim == 4
    inside = vol != 0 if value is None else vol == value
    f = np.where(inside, np.int64(EDT_INF), np.int64(0))
    for axis in (3, 2, 1):
        f = _minplus(f, axis, outside_zero)
    return np.minimum(f, EDT_INF).astype(np.int32)


def r2_of(radius):
    return int(np.floor(float(radius) ** 2 + 1e-9))


def ball(radius):
    """The structuring element: offsets with i^2 + j^2 + k^2 <= floor(radius^2), as a boolean cube."""
    r2 = r2_of(radius)
    k = int(np.floor(np.sqrt(r2)))
    g = np.arange(-k, k + 1)
    return (g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2) <= r2


def dilate(mask, radius):
    """mask: uint8 (n, d, h, w) -> uint8: a voxel within `radius` of a non-zero voxel."""
    return (edt_sq(mask, value=0) <= r2_of(radius)).astype(np.uint8)


def erode(mask, radius, outside=0):
    """A voxel further than `radius` from every zero voxel; outside = 0: the outside of the volume counts as zero voxels."""
    return (edt_sq(mask, outside_zero=not outside) > r2_of(radius)).astype(np.uint8)


def opening(mask, radius):
    return dilate(erode(mask, radius, 0), radius)


def closing(mask, radius):
    return erode(dilate(mask, radius), radius, 0)


def fill_holes(mask):
    """mask: uint8 (d, h, w) or (h, w).  The mask plus every background voxel not connected (6-neighbourhood) to the volume's border."""
    bg = np.asarray(mask) == 0
    reach = np.zeros_like(bg)
    nd = bg.ndim
    for axis in range(nd):
        for side in (0, -1):
            idx = [slice(None)] * nd
            idx[axis] = side
            reach[tuple(idx)] = bg[tuple(idx)]
    while True:
        grown = reach.copy()
        for axis in range(nd):
            a = [slice(None)] * nd
            b = [slice(None)] * nd
            a[axis], b[axis] = slice(1, None), slice(None, -1)
            grown[tuple(a)] |= reach[tuple(b)]
            grown[tuple(b)] |= reach[tuple(a)]
        grown &= bg
        if (grown == reach).all():
            break
        reach = grown
    return (~reach).astype(np.uint8)


def signed_sqdist(class_map, classes, ids):
    """class_map: uint8 (n, d, h, w) -> int32 (n, K, d, h, w), the table of the issue: INT32_MIN at an ignored voxel; 0 where the
    class is absent from the volume or fills all its counted voxels; + squared distance to the class outside it; - squared
    distance to what is not the class (ignored voxels included) inside it."""
    y = np.asarray(class_map)
    n = y.shape[0]
    out = np.zeros((n, len(ids)) + y.shape[1:], dtype=np.int32)
    counted = y < classes
    for k, c in enumerate(ids):
        pos = y == c
        to_class = edt_sq(np.where(pos, 0, 1).astype(np.uint8))            # zeros: the voxels of the class
        to_other = edt_sq(pos.astype(np.uint8))                            # zeros: everything else
        for i in range(n):
            if pos[i].any() and (counted[i] & ~pos[i]).any():
                out[i, k] = np.where(pos[i], -to_other[i], to_class[i])
            out[i, k][~counted[i]] = INT32_MIN
    return out


def phi(s):
    """The distance the loss uses, float64: sqrt(s), -(sqrt(-s) - 1), 0; 0 where the term is left out (INT32_MIN)."""
    s = np.asarray(s).astype(np.int64)
    out = np.zeros(s.shape, dtype=np.float64)
    pos, neg = s > 0, (s < 0) & (s != INT32_MIN)
    out[pos] = np.sqrt(s[pos].astype(np.float64))
    out[neg] = -(np.sqrt((-s[neg]).astype(np.float64)) - 1.0)
    return out


def boundary_loss(logits, smap, ids):
    """logits: float64 (n, C, d, h, w); smap: int32 (n, K, d, h, w).  (loss, dloss/dlogits) in float64: the mean over the terms with
    s != INT32_MIN of softmax(logits)[:, ids] * phi(s); 0 and zeros when no term counts."""
    z = np.asarray(logits, dtype=np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    counted = np.asarray(smap) != INT32_MIN
    cnt = int(counted.sum())
    f = phi(smap)
    grad = np.zeros_like(z)
    if cnt == 0:
        return 0.0, grad
    ids = list(ids)
    loss = float((p[:, ids] * f).sum() / cnt)
    full = np.zeros_like(z)
    full[:, ids] = f
    dot = (p[:, ids] * f).sum(axis=1, keepdims=True)
    grad = p * (full - dot) / cnt
    return loss, grad


def mean_abs_term(logits, smap, ids):
    """A of the loss bound: the float64 mean of |p * phi| over the counted terms (0 when there is none)."""
    z = np.asarray(logits, dtype=np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    counted = np.asarray(smap) != INT32_MIN
    cnt = int(counted.sum())
    return float(np.abs(p[:, list(ids)] * phi(smap)).sum() / cnt) if cnt else 0.0


def torch_loss(z, s, ids, dtype):
    """(softmax * phi)[counted terms].mean() by torch's CPU autograd in `dtype` -> (loss, grad) as float64: in float64 what
    boundary_loss is held to, in float32 the yardstick e32 of the bounds."""
    import torch
    zt = torch.from_numpy(np.asarray(z)).to(dtype).requires_grad_(True)
    f = torch.from_numpy(phi(s)).to(dtype)
    counted = torch.from_numpy(np.asarray(s) != INT32_MIN)
    p = torch.softmax(zt, dim=1)[:, list(ids)]
    loss = (p * f)[counted].mean() if counted.any() else (zt * 0).sum()
    loss.backward()
    return float(loss.detach().double()), zt.grad.double().numpy()


# ------------------------------------------------------------------ the comparisons of the GPU suite
def compare_exact(got, want, what=""):
    """Integer or byte volumes, bit for bit."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d of %d elements differ, first at %s: got %s, want %s" % (
        what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def loss_bound(e32, a):
    return 8.0 * max(e32, 2.0 ** -23 * a)


def compare_loss(got, want, e32, a, what=""):
    err = abs(float(got) - float(want))
    print("%s: loss %.9g, float64 %.9g, error %.3g, bound %.3g (e32 %.3g, A %.3g)" % (what, got, want, err, loss_bound(e32, a), e32, a))
    assert err <= loss_bound(e32, a), (what, got, want, err, loss_bound(e32, a))


def grad_bound(g64, e32, bf16):
    g64 = np.asarray(g64, dtype=np.float64)
    b = np.full(g64.shape, 8.0 * max(e32, 2.0 ** -23 * float(np.abs(g64).max(initial=0.0))))
    return b + (2.0 ** -8 * np.abs(g64) if bf16 else 0.0)


def compare_grad(got, g64, e32, bf16, what=""):
    got, g64 = np.asarray(got, dtype=np.float64), np.asarray(g64, dtype=np.float64)
    assert got.shape == g64.shape, (what, got.shape, g64.shape)
    err, bound = np.abs(got - g64), grad_bound(g64, e32, bf16)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print("%s: max gradient error %.3g, bound there %.3g (e32 %.3g, max |g| %.3g)" % (what, err[worst], bound[worst], e32,
                                                                                      np.abs(g64).max(initial=0.0)))
    assert (err <= bound).all(), (what, worst, got[worst], g64[worst], err[worst], bound[worst])
