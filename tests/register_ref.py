"""numpy restatement of csrc/register.hip: quantisation, the joint histogram under candidate affines, the histogram costs, the
resampler between two grids and the 2x mean pyramid.  Every function computes in float64 by default; `fp32=True` repeats the
kernel's arithmetic operation by operation in float32, in the order include/mri3d.h documents (numpy rounds every float32
operation once, the file is compiled without contraction).

For the histogram and the resampler the float64 pass also COUNTS how far the kernel's float32 result may lie from it, so that a
test never compares a float32 bin decision with a float64 one:

  d_c  coordinates.  s_a = A2*w + ((A0*d + A1*h) + A3) takes five roundings, each at most u = 2^-24 times the magnitude of its
       result, which never exceeds M = |A0| d + |A1| h + |A2| w + |A3| by more than (1 + u)^4:  d_c = 5 u M (1 + 2^-20) + 2^-50 M
       (the last term covers the float64 evaluation itself).
  d_v  sampled value.  Trilinear interpolation with clamped indices is continuous and piecewise linear; along axis a its slope
       never exceeds L_a = the largest difference of two neighbours along a in the whole volume.  So moving the coordinate by d_c
       moves the value by at most sum_a L_a d_c.  The seven lerps x = v0 + f*(v1 - v0) sit three deep; a lerp passes on at most the
       larger error of its inputs (a convex combination) and adds the roundings of its subtraction and product (each at most
       u * 2 V) and of its sum (u * V), V = max |v|: 5 u V per level, 16 u V with the slack for three levels.
       d_v = sum_a L_a d_c + 16 u V.
  d_t  bin coordinate t = (v - lo) * scale:  |scale| d_v + 2 u (|t| + |lo scale|) (1 + 2^-20)  (one subtraction, one product).

A sample is CERTAIN when its inside test clears d_c on every axis and floor(t - d_t) == floor(t + d_t) after clamping; else it is
UNCERTAIN and the reference lists every bin it could reach (or that it may not count at all)."""
import numpy as np

U32 = 2.0 ** -24
SKIP = 255


# ---------------------------------------------------------------------------------------------- quantisation
def quantize(x, lo, scale, bins, mask=None, fp32=True):
    dt = np.float32 if fp32 else np.float64
    xv = np.asarray(x, dtype=np.float32).astype(dt)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.floor((xv - dt(np.float32(lo))) * dt(np.float32(scale)))
    t = np.minimum(np.maximum(np.nan_to_num(t, nan=0.0, posinf=1e30, neginf=-1e30), 0), bins - 1)
    out = t.astype(np.uint8)
    bad = ~np.isfinite(np.asarray(x, dtype=np.float32))
    if mask is not None:
        bad |= np.asarray(mask).astype(np.uint8) == 0
    out[bad] = SKIP
    return out


# ---------------------------------------------------------------------------------------------- coordinates and sampling
def _grid(shape, dt):
    d, h, w = shape
    return (np.arange(d, dtype=dt)[:, None, None], np.arange(h, dtype=dt)[None, :, None], np.arange(w, dtype=dt)[None, None, :])


def coords(affine, fixed_shape, fp32=False):
    """s_a for every fixed voxel, a list of three (d, h, w) arrays, in the documented order."""
    dt = np.float32 if fp32 else np.float64
    A = np.asarray(affine, dtype=np.float32).reshape(3, 4).astype(dt)
    gd, gh, gw = _grid(fixed_shape, dt)
    out = []
    for a in range(3):
        r = (A[a, 0] * gd + A[a, 1] * gh) + A[a, 3]
        out.append(np.broadcast_to(A[a, 2] * gw + r, fixed_shape).astype(dt))
    return out


def coord_error(affine, fixed_shape):
    """d_c per axis, three (d, h, w) float64 arrays."""
    A = np.abs(np.asarray(affine, dtype=np.float32).reshape(3, 4).astype(np.float64))
    gd, gh, gw = _grid(fixed_shape, np.float64)
    out = []
    for a in range(3):
        M = np.broadcast_to(A[a, 0] * gd + A[a, 1] * gh + A[a, 2] * gw + A[a, 3], fixed_shape)
        out.append(5 * U32 * M * (1 + 2.0 ** -20) + 2.0 ** -50 * M)
    return out


def inside(s, shape, lo=-0.5, hi=-0.5):
    """warp3d's rule: -0.5 <= s_a <= N_a - 0.5 (lo and hi exist for the planted mistakes of the tests)."""
    dt = s[0].dtype.type
    ok = np.ones(s[0].shape, dtype=bool)
    for a in range(3):
        ok &= (s[a] >= dt(lo)) & (s[a] <= dt(shape[a]) + dt(hi))
    return ok


def trilinear(vol, s):
    """The kernel's trilinear sample at coordinates s (their dtype sets the arithmetic), indices clamped."""
    dt = s[0].dtype.type
    v = np.asarray(vol, dtype=np.float32).astype(dt)
    N = v.shape
    q = [np.minimum(np.maximum(s[a], dt(-1)), dt(N[a])) for a in range(3)]
    e = [np.floor(x) for x in q]
    f = [q[a] - e[a] for a in range(3)]
    i = [e[a].astype(np.int64) for a in range(3)]
    lo = [np.clip(i[a], 0, N[a] - 1) for a in range(3)]
    hi = [np.clip(i[a] + 1, 0, N[a] - 1) for a in range(3)]

    def lerp(a, b, t):
        return a + t * (b - a)
    x00 = lerp(v[lo[0], lo[1], lo[2]], v[lo[0], lo[1], hi[2]], f[2])
    x01 = lerp(v[lo[0], hi[1], lo[2]], v[lo[0], hi[1], hi[2]], f[2])
    x10 = lerp(v[hi[0], lo[1], lo[2]], v[hi[0], lo[1], hi[2]], f[2])
    x11 = lerp(v[hi[0], hi[1], lo[2]], v[hi[0], hi[1], hi[2]], f[2])
    y0 = lerp(x00, x01, f[1])
    y1 = lerp(x10, x11, f[1])
    return lerp(y0, y1, f[0])


def nearest_index(s, shape):
    dt = s[0].dtype.type
    q = [np.minimum(np.maximum(s[a], dt(-1)), dt(shape[a])) for a in range(3)]
    return [np.clip(np.floor(q[a] + dt(0.5)).astype(np.int64), 0, shape[a] - 1) for a in range(3)]


def bin_coordinate(v, m_lo, m_scale):
    dt = v.dtype.type
    return (v - dt(np.float32(m_lo))) * dt(np.float32(m_scale))


def _clamp_bin(t, bins):
    return np.clip(np.floor(np.nan_to_num(t, nan=0.0)), 0, bins - 1).astype(np.int64)


def lipschitz(vol):
    v = np.asarray(vol, dtype=np.float64)
    return [float(np.abs(np.diff(v, axis=a)).max()) if v.shape[a] > 1 else 0.0 for a in range(3)]


def value_error(vol, dc):
    """d_v for every sample, from the coordinate errors dc."""
    L = lipschitz(vol)
    V = float(np.abs(np.asarray(vol, dtype=np.float64)).max())
    return L[0] * dc[0] + L[1] * dc[1] + L[2] * dc[2] + 16 * U32 * V


# ---------------------------------------------------------------------------------------------- joint histogram
def joint_hist(fixed_bins, moving, affines, m_lo, m_scale, bins, fp32=False, inside_lo=-0.5, inside_hi=-0.5):
    """(k, bins, bins) int64: hist[c][bf][bm]."""
    fb = np.asarray(fixed_bins, dtype=np.uint8)
    affines = np.asarray(affines, dtype=np.float32).reshape(-1, 3, 4)
    out = np.zeros((len(affines), bins, bins), dtype=np.int64)
    counted = fb < bins
    for c, A in enumerate(affines):
        s = coords(A, fb.shape, fp32)
        ok = counted & inside(s, moving.shape, inside_lo, inside_hi)
        bm = _clamp_bin(bin_coordinate(trilinear(moving, s), m_lo, m_scale), bins)
        np.add.at(out[c], (fb[ok].astype(np.int64), bm[ok]), 1)
    return out


def joint_hist_bounds(fixed_bins, moving, affines, m_lo, m_scale, bins):
    """Per candidate: (H_certain, H_possible, n_certain, n_uncertain).  H_certain counts the certain samples; H_possible has a 1
    for every bin an uncertain sample could reach.  The kernel's histogram H obeys H_certain <= H <= H_certain + H_possible and
    n_certain <= H.sum() <= n_certain + n_uncertain."""
    fb = np.asarray(fixed_bins, dtype=np.uint8)
    affines = np.asarray(affines, dtype=np.float32).reshape(-1, 3, 4)
    k = len(affines)
    Hc, Hp = np.zeros((k, bins, bins), dtype=np.int64), np.zeros((k, bins, bins), dtype=np.int64)
    nc, nu = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64)
    counted = fb < bins
    lo_s = float(np.float32(m_lo)) * float(np.float32(m_scale))
    for c, A in enumerate(affines):
        s = coords(A, fb.shape)
        dc = coord_error(A, fb.shape)
        sure_in, maybe_in = np.ones(fb.shape, dtype=bool), np.ones(fb.shape, dtype=bool)
        for a in range(3):
            hi = moving.shape[a] - 0.5
            sure_in &= (s[a] >= -0.5 + dc[a]) & (s[a] <= hi - dc[a])
            maybe_in &= (s[a] >= -0.5 - dc[a]) & (s[a] <= hi + dc[a])
        t = bin_coordinate(trilinear(moving, s), m_lo, m_scale)
        dt_ = abs(float(np.float32(m_scale))) * value_error(moving, dc) + 2 * U32 * (np.abs(t) + abs(lo_s)) * (1 + 2.0 ** -20)
        b_lo, b_hi = _clamp_bin(t - dt_, bins), _clamp_bin(t + dt_, bins)
        certain = counted & sure_in & (b_lo == b_hi)
        uncertain = counted & maybe_in & ~certain
        bf = fb.astype(np.int64)
        np.add.at(Hc[c], (bf[certain], b_lo[certain]), 1)
        for b in range(int((b_hi - b_lo)[uncertain].max()) + 1 if uncertain.any() else 0):
            sel = uncertain & (b_lo + b <= b_hi)
            np.add.at(Hp[c], (bf[sel], (b_lo + b)[sel]), 1)
        nc[c], nu[c] = int(certain.sum()), int(uncertain.sum())
    return Hc, Hp, nc, nu


# ---------------------------------------------------------------------------------------------- costs
def hist_costs(hist, kind, min_count=0):
    """(k, 2) float64 {cost, n} by the definitions of the header: 0 correlation ratio, 1 -MI, 2 -(H_f + H_m) / H_fm."""
    hist = np.asarray(hist, dtype=np.float64)
    out = np.zeros((hist.shape[0], 2))
    bins = hist.shape[1]
    y = np.arange(bins) + 0.5
    for c, H in enumerate(hist):
        n = H.sum()
        out[c] = (np.inf, n)
        if n < min_count or n <= 0:
            continue
        p = H / n
        pi, pj = p.sum(1), p.sum(0)
        if kind == 0:
            var = (pj * (y - (pj * y).sum()) ** 2).sum()
            rows = pi > 0
            mean_i = (p[rows] * y).sum(1) / pi[rows]
            var_i = (p[rows] * (y[None, :] - mean_i[:, None]) ** 2).sum(1) / pi[rows]
            if var > 0:
                out[c, 0] = (pi[rows] * var_i).sum() / var
        else:
            def ent(q):
                q = q[q > 0]
                return -(q * np.log(q)).sum()
            hf, hm, hfm = ent(pi), ent(pj), ent(p.ravel())
            if kind == 1:
                out[c, 0] = -(hf + hm - hfm)
            elif hfm > 0:
                out[c, 0] = -(hf + hm) / hfm
    return out


# ---------------------------------------------------------------------------------------------- resampling
def resample_affine(image, label, affine, out_shape, pad=0.0, fp32=False):
    """(image_out, label_out), None where the input is None."""
    src_shape = (image if image is not None else label).shape
    s = coords(affine, out_shape, fp32)
    ok = inside(s, src_shape)
    img_out = lab_out = None
    if image is not None:
        v = trilinear(image, s)
        img_out = np.where(ok, v, v.dtype.type(np.float32(pad)))
    if label is not None:
        n = nearest_index(s, src_shape)
        lab = np.asarray(label)
        lab_out = np.where(ok, lab[n[0], n[1], n[2]], np.zeros((), dtype=lab.dtype)).astype(lab.dtype)
    return img_out, lab_out


def resample_bounds(image, affine, out_shape, src_shape=None):
    """(sure_in, sure_out, d_v, tie): voxels certainly inside / outside the source, the bound on |kernel - float64| of an inside
    image sample, and the voxels whose nearest label index the float32 coordinate may round the other way (floor(q + 0.5) within
    d_c + u |q + 0.5| of an integer, on any axis)."""
    src_shape = image.shape if image is not None else src_shape
    s = coords(affine, out_shape)
    dc = coord_error(affine, out_shape)
    sure_in, maybe_in = np.ones(out_shape, dtype=bool), np.ones(out_shape, dtype=bool)
    tie = np.zeros(out_shape, dtype=bool)
    for a in range(3):
        hi = src_shape[a] - 0.5
        sure_in &= (s[a] >= -0.5 + dc[a]) & (s[a] <= hi - dc[a])
        maybe_in &= (s[a] >= -0.5 - dc[a]) & (s[a] <= hi + dc[a])
        z = np.clip(s[a], -1, src_shape[a]) + 0.5
        tie |= np.abs(z - np.round(z)) <= dc[a] + U32 * np.abs(z) * (1 + 2.0 ** -20)
    dv = value_error(image, dc) if image is not None else None
    return sure_in, ~maybe_in, dv, tie


# ---------------------------------------------------------------------------------------------- pyramid
def downsample2(x, fp32=False):
    dt = np.float32 if fp32 else np.float64
    x = np.asarray(x, dtype=np.float32).astype(dt)
    d, h, w = x.shape
    do, ho, wo = (d + 1) // 2, (h + 1) // 2, (w + 1) // 2
    pad = np.zeros((2 * do, 2 * ho, 2 * wo), dtype=dt)
    pad[:d, :h, :w] = x
    exists = np.zeros(pad.shape, dtype=bool)
    exists[:d, :h, :w] = True
    total = None
    for a in range(2):
        for b in range(2):
            for c in range(2):
                term = pad[a::2, b::2, c::2]
                total = term.copy() if total is None else total + term     # a missing voxel adds an exact 0
    cnt = exists.reshape(do, 2, ho, 2, wo, 2).sum((1, 3, 5)).astype(dt)
    return total * (dt(1) / cnt)
