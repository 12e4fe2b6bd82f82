"""float64 reference of the two fused convolution operators (csrc/upconv.hip, csrc/sepconv.hip), written from the definition: index
arithmetic and sums over taps, no F.interpolate and no F.conv3d.  Tensors are logical NCDHW torch.float64; evaluate on the STORED
values (bf16-rounded where the storage type is bf16).  Every result comes with the magnitudes its error bound is counted from:
    value, L1 = sum |term|, T = number of terms          (per output element, same shape as the value)

upconv   y[n, o, v]   = b[o] + sum_t sum_ci w[o, ci, t] x[n, ci, (v + off_t) // S]      off_t = tap - padding, per axis; the term is
                        zero where the FINE index v + off_t lies outside the fine grid S * coarse (zero padding at the fine level)
         dx[n, ci, c] = sum over the S^3 fine voxels u of coarse voxel c, sum_t sum_o w[o, ci, t] dy[n, o, u - off_t]
         dw[o, ci, t] = sum_n sum_v dy[n, o, v] x[n, ci, (v + off_t) // S],   dbias[o] = sum_n sum_v dy[n, o, v]
pair     first = Conv3d(1, C, (K1,1,1), stride (s1,1,1), padding (p1,0,0)), second = Conv3d(C, C2, (1,K2,1), stride (1,s2,1),
         padding (0,p2,0)) on its output:
         da1[n, c, d1, h, w] = sum over kh = (h + p2) mod s2, + s2, .. < K2 with h2 = (h + p2 - kh) / s2 in [0, H2):
                               sum_c2 dy2[n, c2, d1, h2, w] w2[c2, c, kh]
         dw1[c, kd] = sum_n sum_(d1,h,w) x[n, s1 d1 + kd - p1, h, w] da1[n, c, d1, h, w]   (planes outside [0, D) are zero)
         dbias1[c]  = sum da1[n, c]"""
import itertools

import torch

U = 2.0 ** -24
F64 = torch.float64


def taps(k):
    """[(tap index, (a, b, c))] in the weight's memory order (kd slowest)"""
    return list(enumerate(itertools.product(range(k[0]), range(k[1]), range(k[2]))))


def out_extents(fine, k, pad):
    return tuple(f + 2 * p - kk + 1 for f, kk, p in zip(fine, k, pad))


def _axis(out, off, fine, S):
    """coarse index (clamped) and validity of the fine input index o + off for o in range(out)"""
    i = torch.arange(out) + off
    ok = (i >= 0) & (i < fine)
    return torch.div(i.clamp(0, fine - 1), S, rounding_mode="floor"), ok


def _gather(x, S, k, pad, tap, out):
    """x read through the index map at one tap: (N, Ci, Do, Ho, Wo), zero where the fine index is outside; and the (Do, Ho, Wo) mask"""
    fine = tuple(S * e for e in x.shape[2:])
    (cd, okd), (ch, okh), (cw, okw) = (_axis(out[a], tap[a] - pad[a], fine[a], S) for a in range(3))
    ok = okd[:, None, None] & okh[None, :, None] & okw[None, None, :]
    xs = x[:, :, cd][:, :, :, ch][:, :, :, :, cw]
    return xs * ok.to(x.dtype), ok


def upconv_fwd(x, w, b, S, pad):
    """(y, A, T): A = |b| + sum |w| |x| over the in-range terms, T their number (the bias included)"""
    k = tuple(w.shape[2:])
    out = out_extents(tuple(S * e for e in x.shape[2:]), k, pad)
    n, co = x.shape[0], w.shape[0]
    y = torch.zeros((n, co) + out, dtype=F64)
    A, T = torch.zeros_like(y), torch.zeros_like(y)
    if b is not None:
        y += b.view(1, -1, 1, 1, 1)
        A += b.abs().view(1, -1, 1, 1, 1)
        T += 1
    for _, tp in taps(k):
        xs, ok = _gather(x, S, k, pad, tp, out)
        wt = w[:, :, tp[0], tp[1], tp[2]]
        y += torch.einsum("ncdhw,oc->nodhw", xs, wt)
        A += torch.einsum("ncdhw,oc->nodhw", xs.abs(), wt.abs())
        T += ok.to(F64) * x.shape[1]
    return y, A, T


def upconv_dgrad(dy, w, S, pad, coarse):
    """(dx, L1, T) on the coarse grid (N, Ci) + coarse"""
    k = tuple(w.shape[2:])
    fine = tuple(S * e for e in coarse)
    out = tuple(dy.shape[2:])
    n, ci = dy.shape[0], w.shape[1]
    g = torch.zeros((n, ci) + fine, dtype=F64)
    L1, T = torch.zeros_like(g), torch.zeros_like(g)
    for _, tp in taps(k):
        idx, oks = [], []
        for a in range(3):
            o = torch.arange(fine[a]) - (tp[a] - pad[a])          # input voxel u feeds output o = u - off
            oks.append((o >= 0) & (o < out[a]))
            idx.append(o.clamp(0, out[a] - 1))
        ok = (oks[0][:, None, None] & oks[1][None, :, None] & oks[2][None, None, :]).to(F64)
        ds = dy[:, :, idx[0]][:, :, :, idx[1]][:, :, :, :, idx[2]] * ok
        wt = w[:, :, tp[0], tp[1], tp[2]]
        g += torch.einsum("nodhw,oc->ncdhw", ds, wt)
        L1 += torch.einsum("nodhw,oc->ncdhw", ds.abs(), wt.abs())
        T += ok * w.shape[0]

    def blocks(t):
        return t.view(n, ci, coarse[0], S, coarse[1], S, coarse[2], S).sum(dim=(3, 5, 7))
    return blocks(g), blocks(L1), blocks(T)


def upconv_wgrad(x, dy, S, pad, k):
    """{"dw": (dw, L1, T), "dbias": (dbias, L1, T)}: dw in the torch layout (Co, Ci, kd, kh, kw)"""
    out = tuple(dy.shape[2:])
    co, ci = dy.shape[1], x.shape[1]
    dw = torch.zeros((co, ci) + tuple(k), dtype=F64)
    L1, T = torch.zeros_like(dw), torch.zeros_like(dw)
    for _, tp in taps(k):
        xs, ok = _gather(x, S, k, pad, tp, out)
        dw[:, :, tp[0], tp[1], tp[2]] = torch.einsum("nodhw,ncdhw->oc", dy, xs)
        L1[:, :, tp[0], tp[1], tp[2]] = torch.einsum("nodhw,ncdhw->oc", dy.abs(), xs.abs())
        T[:, :, tp[0], tp[1], tp[2]] = float(ok.sum()) * x.shape[0]
    nvox = float(dy.shape[0] * out[0] * out[1] * out[2])
    return {"dw": (dw, L1, T), "dbias": (dy.sum(dim=(0, 2, 3, 4)), dy.abs().sum(dim=(0, 2, 3, 4)), torch.full((co,), nvox, dtype=F64))}


def pair_extents(sp, k1, s1, p1, k2, s2, p2):
    """(D1, H2)"""
    return (sp[0] + 2 * p1 - k1) // s1 + 1, (sp[1] + 2 * p2 - k2) // s2 + 1


def pair_da1(dy2, w2, H, s2, p2):
    """(da1, A1, T1): (N, C, D1, H, W); A1 = sum |dy2| |w2|, T1 the number of terms"""
    n, c2n, d1, h2n, wn = dy2.shape
    cn, k2 = w2.shape[1], w2.shape[3]
    da1 = torch.zeros((n, cn, d1, H, wn), dtype=F64)
    A1, T1 = torch.zeros_like(da1), torch.zeros_like(da1)
    for kh in range(k2):
        hs = [h for h in range(H) if (h + p2 - kh) >= 0 and (h + p2 - kh) % s2 == 0 and (h + p2 - kh) // s2 < h2n]
        if not hs:
            continue
        h2 = [(h + p2 - kh) // s2 for h in hs]
        wk = w2[:, :, 0, kh, 0]
        da1[:, :, :, hs, :] += torch.einsum("nkdhw,kc->ncdhw", dy2[:, :, :, h2, :], wk)
        A1[:, :, :, hs, :] += torch.einsum("nkdhw,kc->ncdhw", dy2[:, :, :, h2, :].abs(), wk.abs())
        T1[:, :, :, hs, :] += c2n
    return da1, A1, T1


def pair_wgrad_first(x, dy2, w2, k1, s1, p1, s2, p2):
    """{"dw1": (dw1 (C, 1, K1, 1, 1), L1, T), "dbias1": (dbias1 (C), L1, T)} from x (N, 1, D, H, W), dy2 (N, C2, D1, H2, W), w2 (C2, C, 1, K2, 1)"""
    n, _, D, H, W = x.shape
    da1, A1, T1 = pair_da1(dy2, w2, H, s2, p2)
    cn, d1n = da1.shape[1], da1.shape[2]
    dw, L1, T = (torch.zeros((cn, 1, k1, 1, 1), dtype=F64) for _ in range(3))
    for kd in range(k1):
        i = s1 * torch.arange(d1n) + kd - p1
        ok = ((i >= 0) & (i < D)).to(F64)
        xs = x[:, 0, i.clamp(0, D - 1)] * ok.view(1, -1, 1, 1)                      # (N, D1, H, W)
        dw[:, 0, kd, 0, 0] = torch.einsum("ndhw,ncdhw->c", xs, da1)
        L1[:, 0, kd, 0, 0] = torch.einsum("ndhw,ncdhw->c", xs.abs(), A1)
        T[:, 0, kd, 0, 0] = torch.einsum("d,ncdhw->c", ok, T1)
    s = (0, 2, 3, 4)
    return {"dw1": (dw, L1, T), "dbias1": (da1.sum(dim=s), A1.sum(dim=s), T1.sum(dim=s))}
