"""fp32 emulation of the kernels of csrc/upconv.hip and csrc/sepconv.hip in THEIR summation order (numpy float32; an fma is the
exact product and sum in float64 rounded once to fp32), driven by the launch plan the library answers.  tests/test_fusedconv_bounds.py
uses it twice: the emulation must stay inside the counted bounds, and each deliberate error `err` below must leave them.

Arrays are logical NCDHW numpy float32 holding the stored values; results are fp32 (the storage rounding of y / dx is the caller's).

    err (upconv_fwd)    "coarse_pad"   the zero padding decided on the coarse index (fine index / S, truncating) instead of the fine one
                        "drop_slab"    the last slab of the second grid trip never written
    err (upconv_dgrad)  "tap_sign"     input voxel u reads output u + off instead of u - off
                        "skip_xor"     the butterfly's last step (lane bit 1) left out
                        "c0_stuck"     the first halving step does not advance c0: two channel groups land on the same channels
                        "no_live"      the lanes past wc in a row's last pass store as well (onto the next row's first voxels)
    err (upconv_wgrad)  "drop_slab"    the last slab of the second grid trip skipped
                        "drop_ragged"  the ragged last H chunk of every plane skipped
    err (pair)          "kh0"          a row's tap list starts at kh = 0 instead of (h + p2) mod s2
                        "x_plane"      the x plane outside [0, D) read (plane 0, as the clamped load does) instead of zeroed"""
import numpy as np

import fusedconv_ref as fr

F32 = np.float32


def fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _tap_list(k):
    return [tp for _, tp in fr.taps(k)]


def _slab(plan, slab, n_dout, ho):
    """(nd, h0, hn) of a slab index"""
    hchunks = -(-ho // plan["hch"])
    hk, nd = slab % hchunks, slab // hchunks
    h0 = hk * plan["hch"]
    return nd, h0, min(plan["hch"], ho - h0)


def upconv_fwd(x, w, b, S, pad, plan=None, err=None):
    n, ci, dc, hc, wc = x.shape
    co, k = w.shape[0], w.shape[2:]
    fine = (S * dc, S * hc, S * wc)
    do, ho, wo = fr.out_extents(fine, k, pad)
    od, oh, ow = np.meshgrid(np.arange(do), np.arange(ho), np.arange(wo), indexing="ij")
    acc = np.zeros((n, co, do, ho, wo), F32)
    if b is not None:
        acc += b.astype(F32).reshape(1, co, 1, 1, 1)
    wt = w.reshape(co, ci, -1)
    for t, tp in enumerate(_tap_list(k)):
        idx = [o + tp[a] - pad[a] for a, o in enumerate((od, oh, ow))]
        if err == "coarse_pad":
            cidx = [np.trunc(i / S).astype(np.int64) for i in idx]
            ok = np.logical_and.reduce([(c >= 0) & (c < e) for c, e in zip(cidx, (dc, hc, wc))])
        else:
            ok = np.logical_and.reduce([(i >= 0) & (i < f) for i, f in zip(idx, fine)])
            cidx = [i // S for i in idx]
        cidx = [np.clip(c, 0, e - 1) for c, e in zip(cidx, (dc, hc, wc))]
        q = x[:, :, cidx[0], cidx[1], cidx[2]] * ok.astype(F32)                      # (n, ci, do, ho, wo)
        for c in range(ci):
            for j in range(co):
                acc[:, j] = fma(q[:, c], wt[j, c, t], acc[:, j])
    if err == "drop_slab":
        nd, h0, hn = _slab(plan, min(2 * plan["grid"], plan["slabs"]) - 1, n * do, ho)
        acc[nd // do, :, nd % do, h0:h0 + hn] = 0
    return acc


def upconv_dgrad(dy, w, S, pad, coarse, plan, err=None):
    n, co, do, ho, wo = dy.shape
    ci, k = w.shape[1], w.shape[2:]
    dc, hc, wc = coarse
    fine = (S * dc, S * hc, S * wc)
    SV = S ** 3
    idd, ihh, iww = np.meshgrid(np.arange(fine[0]), np.arange(fine[1]), np.arange(fine[2]), indexing="ij")
    a = np.zeros((n, ci) + fine, F32)
    wt = w.reshape(co, ci, -1)
    sign = 1 if err == "tap_sign" else -1
    for t, tp in enumerate(_tap_list(k)):
        o = [i + sign * (tp[ax] - pad[ax]) for ax, i in enumerate((idd, ihh, iww))]
        ok = np.logical_and.reduce([(i >= 0) & (i < e) for i, e in zip(o, (do, ho, wo))])
        o = [np.clip(i, 0, e - 1) for i, e in zip(o, (do, ho, wo))]
        d = dy[:, :, o[0], o[1], o[2]] * ok.astype(F32)                              # (n, co) + fine
        for j in range(co):
            for c in range(ci):
                a[:, c] = fma(d[:, j], wt[j, c, t], a[:, c])
    # lanes of a coarse voxel: sub = (sd * S + sh) * S + sw
    v = a.reshape(n, ci, dc, S, hc, S, wc, S).transpose(0, 2, 4, 6, 3, 5, 7, 1).reshape(n, dc, hc, wc, SV, ci).copy()
    sub = np.arange(SV)
    c0 = np.zeros(SV, np.int64)
    N, bit, first = ci, SV // 2, True
    while N >= 2 and bit >= 1:
        hi = (sub & bit) != 0
        lo_half, hi_half = v[..., : N // 2], v[..., N // 2: N]
        send = np.where(hi[:, None], lo_half, hi_half)
        keep = np.where(hi[:, None], hi_half, lo_half)
        recv = send[..., sub ^ bit, :]
        nv = keep if (err == "skip_xor" and bit == 1) else (keep + recv).astype(F32)
        v = nv
        if not (err == "c0_stuck" and first):
            c0 = c0 + np.where(hi, N // 2, 0)
        first = False
        N //= 2
        bit //= 2
    rem = 2 * bit if bit >= 1 else 1                                                 # lanes still holding partial sums of the same channels
    o = rem // 2
    while o >= 1:
        if not (err == "skip_xor" and o == 1):
            v = (v + v[..., sub ^ o, :]).astype(F32)
        o //= 2
    # stores: lanes with (sub & (rem - 1)) == 0 write their N channels at c0; rows (n, cd, ch) in `per` coarse voxels a pass
    rows = n * dc * hc
    dx = np.zeros((rows, wc, ci), F32)
    vr = v.reshape(rows, wc, SV, N)
    for s in sub[(sub & (rem - 1)) == 0]:                                            # in lane order: with c0_stuck a later lane overwrites
        dx[:, :, c0[s]: c0[s] + N] = vr[:, :, s]
    if err == "no_live":
        # the passes x per - wc dead lanes of a row's last pass hold zeros (their dy loads stay masked) and store them past the row's
        # end: onto the first voxels of the next row, taken to land after that row's own stores
        dx[1:, : plan["passes"] * plan["per"] - wc] = 0
    return dx.reshape(n, dc, hc, wc, ci).transpose(0, 4, 1, 2, 3)


def _tree(v):
    """the block sum of v (blocks, 256, items): xor-shuffle tree in each wave, the four waves in a fixed order"""
    nb, _, items = v.shape
    v = v.reshape(nb, 4, 64, items)
    lane = np.arange(64)
    o = 32
    while o >= 1:
        v = (v + v[:, :, lane ^ o, :]).astype(F32)
        o //= 2
    wsum = v[:, :, 0, :]
    return ((wsum[:, 0] + wsum[:, 1]).astype(F32) + (wsum[:, 2] + wsum[:, 3]).astype(F32)).astype(F32)


def _final(part):
    """the reduce kernel: partials summed in double, rounded to fp32"""
    return part.astype(np.float64).sum(axis=0).astype(F32)


def upconv_wgrad(x, dy, S, pad, k, plan, err=None):
    """(dw (Co, Ci) + k, dbias (Co))"""
    n, ci, dc, hc, wc = x.shape
    co, do, ho, wo = dy.shape[1:]
    fine = (S * dc, S * hc, S * wc)
    tl = _tap_list(k)
    nt, grid, hch = len(tl), plan["grid"], plan["hch"]
    hchunks = -(-ho // hch)
    slabs = n * do * hchunks
    assert slabs == plan["slabs"]
    acc = np.zeros((grid, 256, nt * ci * co), F32)
    bacc = np.zeros((grid, 256, co), F32)
    blk = np.arange(grid)
    for gt in range(plan["gtrips"]):
        slab = gt * grid + blk
        live_b = slab < slabs
        if err == "drop_slab":
            live_b &= slab != (min(2 * grid, slabs) - 1)
        slab = np.minimum(slab, slabs - 1)
        hk, nd = slab % hchunks, slab // hchunks
        nn, od = nd // do, nd % do
        h0 = hk * hch
        hn = np.minimum(hch, ho - h0)
        if err == "drop_ragged":
            live_b &= hn == hch
        inner = hn * wo
        for lt in range(plan["trips"]):
            e = lt * 256 + np.arange(256)[None, :]                                   # (1, 256)
            live = live_b[:, None] & (e < inner[:, None])
            e = np.minimum(e, inner[:, None] - 1)
            ow, oh = e % wo, h0[:, None] + e // wo
            d = dy[nn[:, None], :, od[:, None], oh, ow] * live[..., None].astype(F32)       # (grid, 256, co)
            bacc = (bacc + d).astype(F32)
            for t, tp in enumerate(tl):
                idx = (od[:, None] + tp[0] - pad[0] + 0 * oh, oh + tp[1] - pad[1], ow + tp[2] - pad[2])
                ok = np.logical_and.reduce([(i >= 0) & (i < f) for i, f in zip(idx, fine)]) & live
                c = [np.clip(i, 0, f - 1) // S for i, f in zip(idx, fine)]
                q = x[nn[:, None], :, c[0], c[1], c[2]] * ok[..., None].astype(F32)        # (grid, 256, ci)
                for cc in range(ci):
                    for j in range(co):
                        i = (t * ci + cc) * co + j
                        acc[:, :, i] = fma(q[:, :, cc], d[:, :, j], acc[:, :, i])
    dwp, dbp = _final(_tree(acc)), _final(_tree(bacc))
    dw = dwp.reshape(nt, ci, co).transpose(2, 1, 0).reshape((co, ci) + tuple(k))
    return dw, dbp


def pair_wgrad_first(x, dy2, w2, s1, p1, s2, p2, plan, err=None, K1=6, MT=3):
    """(dw1 (C, 1, K1, 1, 1), dbias1 (C)) from x (N, 1, D, H, W), dy2 (N, C2, D1, H2, W), w2 (C2, C, 1, K2, 1)"""
    n, _, D, H, W = x.shape
    c2n, d1n, h2n = dy2.shape[1:4]
    cn, k2 = w2.shape[1], w2.shape[3]
    grid, rows = plan["grid"], n * d1n * H
    assert rows == plan["rows"]
    acc = np.zeros((grid, 4, 64, cn * K1), F32)
    bacc = np.zeros((grid, 4, 64, cn), F32)
    lane = np.arange(64)
    for gt in range(plan["gtrips"]):
        row = (gt * grid + np.arange(grid))[:, None] * 4 + np.arange(4)[None, :]     # (grid, 4): wave-uniform
        live_r = row < rows
        row = np.minimum(row, rows - 1)
        h, r2 = row % H, row // H
        d1, nn = r2 % d1n, r2 // d1n
        kh0 = np.zeros_like(h) if err == "kh0" else (h + p2) % s2
        for ck in range(plan["chunks"]):
            wv = ck * 64 + lane                                                      # (64,)
            live = live_r[..., None] & (wv < W)[None, None, :]
            wcl = np.minimum(wv, W - 1)
            g = np.zeros((grid, 4, 64, cn), F32)
            for t in range(MT):
                kh = kh0 + t * s2
                u = h + p2 - kh
                ok = (kh < k2) & (u >= 0) & (np.floor_divide(np.maximum(u, 0), s2) < h2n)
                h2 = np.where(ok, np.maximum(u, 0) // s2, 0)
                khc = np.where(ok, kh, 0)
                q = dy2[nn[..., None], :, d1[..., None], h2[..., None], wcl[None, None, :]]       # (grid, 4, 64, c2)
                q = q * ok[..., None, None].astype(F32)
                wk = w2[:, :, 0, :, 0][:, :, khc]                                    # (c2, c, grid, 4)
                for kk in range(c2n):
                    for c in range(cn):
                        g[..., c] = fma(q[..., kk], wk[kk, c][..., None], g[..., c])
            g = g * live[..., None].astype(F32)
            bacc = (bacc + g).astype(F32)
            for kd in range(K1):
                pid = d1 * s1 + kd - p1
                inr = (pid >= 0) & (pid < D)
                xv = x[nn[..., None], 0, np.where(inr, pid, 0)[..., None], h[..., None], wcl[None, None, :]]
                if err != "x_plane":
                    xv = xv * inr[..., None].astype(F32)
                for c in range(cn):
                    acc[..., c * K1 + kd] = fma(xv, g[..., c], acc[..., c * K1 + kd])
    dw = _final(_tree(acc.reshape(grid, 256, -1))).reshape(cn, 1, K1, 1, 1)
    return dw, _final(_tree(bacc.reshape(grid, 256, -1)))
