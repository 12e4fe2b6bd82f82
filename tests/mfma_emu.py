"""fp32 emulation of the 3x3x3 MFMA convolution kernels on the CPU, in the kernels' order of summation, for tests/test_mfma_bounds.py:
it shows that the bounds of tests/mfma_ref.py hold for an honest fp32 evaluation and that the errors these kernels' corners can
make leave them.  Every accumulation step is one fused multiply-add in fp32 (the exact product added in float64, rounded to fp32);
the k order inside one MFMA instruction is taken as ascending k, which is what csrc/conv_mfma.hip states for the fp32 instruction.

  tiled (conv_mfma_fwd2_kernel; the data gradient is the forward of the transposed, flipped weights on dy): chunk by chunk of 8 fp32 /
      16 bf16 channels, tap group by tap group (pair_tap: two taps share a K step), per group k-step by k-step: fp32 k-step s adds
      (tap a, ch s), (tap a, ch 4 + s), (tap b, ch s), (tap b, ch 4 + s); the single group 13 of the fp32 image adds tap 26's channels
      in single_chan's order 0, 4, 1, 5 | 2, 6, 3, 7; the bf16 K = 32 step adds tap a's 16 channels, then tap b's.  Then the bias, then
      the rounding to the storage type.  (tiled_n8 adds the same products in its own row-paired order, which is not restated.)
      Statistics: per lane over the 8 rows of a tile in fp32 (s1 += a, s2 = fma(a, a, s2), rows outside the volume add 0), the four
      additions of row_sum16 over the 16 voxel lanes, float64 from there.
  direct (conv_mfma_direct_kernel, mode 0: forward at stride 1, 2, 3 and the stride-1 data gradient): (kd, kh) pair by pair, 16-channel
      chunk by chunk, kw by kw, four K = 4 steps s4 that add channels s4, 4 + s4, 8 + s4, 12 + s4 of the chunk; the split form gives
      pair i to wave i mod 4 and adds waves 1, 2, 3 to wave 0 in that order.  fp32 weights in both storage types.
  weight gradient: per workgroup its tiles in the order of its walk (tile_walk, restated here; cin1: a contiguous range), per tile
      every wave its quarter of the rows, per row the voxels in the kernel's k order, one accumulator element per (tap, ci, co); the
      transposed-tile kernels (wgrad6, bf16, bf16t) attribute a product to the tile of its X voxel and read dY one voxel to the
      left / right; then wave 0 + wave 1 + wave 2 + wave 3 in fp32, the workgroups' partials in float64, the result in fp32.

FAULTS: the deliberate errors, by name."""
import torch

import mfma_run as run

FAULTS = ("product-dropped-at-the-last-voxel", "single-group-channels-swapped", "neighbouring-channel-read", "bf16-weights-unrounded",
          "voxel-dropped-from-dw", "w-halo-counted-into-dw", "db-doubled", "statistics-include-the-bias", "partial-dropped",
          "last-ragged-row-unwritten")
F32 = torch.float32


def _fma(acc, a, b):
    return (acc.double() + a.double() * b.double()).float()


def pair_tap(tg, half):
    if tg < 9:
        return tg * 3 + half
    if tg < 12:
        return (half * 3 + (tg - 9)) * 3 + 2
    return (6 + half) * 3 + 2 if tg == 12 else (26 if half == 0 else 27)


def _tiled_order(kc, bf):
    """[(tap, channel)] in the order one accumulator element receives its products"""
    ck = 16 if bf else 8
    seq = []
    for c in range(-(-kc // ck)):
        for tg in range(14):
            ta, tb = pair_tap(tg, 0), pair_tap(tg, 1)
            if bf:
                seq += [(t, c * 16 + j) for t in (ta, tb) for j in range(16)]
            elif tg == 13:
                seq += [(26, c * 8 + 2 * s + (g >> 1) + 4 * (g & 1)) for s in range(2) for g in range(4)]
            else:
                seq += [(t, c * 8 + h * 4 + s) for s in range(4) for t in (ta, tb) for h in range(2)]
    return [(t, ch) for t, ch in seq if t < 27 and ch < kc]


def _direct_order(kc):
    """[(pair index, tap, channel)]"""
    seq = []
    for pair in range(9):
        for c in range(-(-kc // 16)):
            for kw in range(3):
                seq += [(pair, pair * 3 + kw, c * 16 + 4 * kq + s4) for s4 in range(4) for kq in range(4)]
    return [(p, t, ch) for p, t, ch in seq if ch < kc]


def _tree16(v):
    v = v.reshape(v.shape[:-1] + (v.shape[-1] // 16, 16))
    for h in (8, 4, 2, 1):
        v = v[..., :h] + v[..., h:2 * h]
    return v[..., 0]


def conv(row, dtype, inp, pl, p, fault=None, sub=None):
    """the forward (p = "fwd") or the stride-1 data gradient (p = "dgrad") of a tiled or direct (mode 0) plan `pl` ->
    {"y" | "dx": the stored result, "stats": (Co, 2) float64 where the row asks for them}; sub: only the first `sub` output channels
    (every output channel receives its products in the same order)"""
    bf = dtype == "bf16"
    kernel = pl["kernel"]
    assert kernel in ("tiled", "tiled_n8", "direct") and pl["mode"] == 0 and (p == "fwd" or row.stride == 1)
    w = inp["w"].float()
    if bf and kernel != "direct" and fault != "bf16-weights-unrounded":
        w = w.to(torch.bfloat16).float()
    src = inp["x"].float() if p == "fwd" else inp["dy"].float()
    if p == "dgrad":
        w = w.transpose(0, 1).flip(2, 3, 4).contiguous()
    w = w[:sub]
    nc, kc = w.shape[:2]
    w = w.reshape(nc, kc, 27)
    s = row.stride
    N, _, D, H, W = src.shape
    Do, Ho, Wo = run.out_sp(row) if p == "fwd" else (D, H, W)
    xp = torch.zeros((N, kc, D + 2, H + 2, W + 2), dtype=F32)
    xp[:, :, 1:-1, 1:-1, 1:-1] = src

    def xs(tap, ch):
        kd, kh, kw = tap // 9, (tap // 3) % 3, tap % 3
        return xp[:, ch:ch + 1, kd:kd + s * (Do - 1) + 1:s, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s]

    def wv(tap, ch):
        return w[:, ch, tap].view(1, nc, 1, 1, 1)
    if kernel == "direct":
        accs = [torch.zeros((N, nc, Do, Ho, Wo), dtype=F32) for _ in range(4 if pl["split"] else 1)]
        for pair, tap, ch in _direct_order(kc):
            i = pair & 3 if pl["split"] else 0
            accs[i] = _fma(accs[i], wv(tap, ch), xs(tap, ch))
        acc = accs[0]
        for a in accs[1:]:
            acc = acc + a
    else:
        acc = torch.zeros((N, nc, Do, Ho, Wo), dtype=F32)
        for tap, ch in _tiled_order(kc, bf):
            a, b = wv(tap, ch), xs(tap, ch)
            if fault == "single-group-channels-swapped" and not bf and tap == 26 and ch % 8 in (1, 4):
                b = xs(tap, ch - ch % 8 + (5 - ch % 8))          # channel 1's voxels against channel 4's weights and back
            acc = _fma(acc, a, b)
    if fault == "neighbouring-channel-read":                   # the channel behind the slice holds ones
        acc = _fma(acc, torch.full((1,), 1e-3), torch.ones_like(acc))
    if fault == "product-dropped-at-the-last-voxel":
        tap, ch = 13, kc - 1
        acc[-1, :, -1, -1, -1] = (acc[-1, :, -1, -1, -1].double() - w[:, ch, tap].double() * xs(tap, ch)[-1, 0, -1, -1, -1].double()).float()
    bias = inp["b"][:sub].float().view(1, -1, 1, 1, 1) if (p == "fwd" and inp["b"] is not None) else None
    out = (acc + bias if bias is not None else acc).to(run.TORCH[dtype])
    if fault == "last-ragged-row-unwritten":
        out[:, :, :, -1, :] = float("nan")
    res = {"y" if p == "fwd" else "dx": out}
    if row.stats and p == "fwd":
        a = acc + bias if (fault == "statistics-include-the-bias" and bias is not None) else acc
        Hp, Wp = -(-Ho // 8) * 8, -(-Wo // 16) * 16
        ap = torch.zeros((N, nc, Do, Hp, Wp), dtype=F32)
        ap[:, :, :, :Ho, :Wo] = a
        ap = ap.view(N, nc, Do, Hp // 8, 8, Wp)
        s1 = torch.zeros((N, nc, Do, Hp // 8, Wp), dtype=F32)
        s2 = torch.zeros_like(s1)
        for m in range(8):
            s1 = s1 + ap[:, :, :, :, m]
            s2 = _fma(s2, ap[:, :, :, :, m], ap[:, :, :, :, m])
        t1, t2 = _tree16(s1).double(), _tree16(s2).double()              # (N, nc, Do, tiles h, tiles w): one per wave and tile
        if fault == "partial-dropped":                                   # the first tile's four waves: its workgroup's partial
            t1[0, :, :4, 0, 0] = 0
            t2[0, :, :4, 0, 0] = 0
        res["stats"] = torch.stack((t1.sum((0, 2, 3, 4)), t2.sum((0, 2, 3, 4))), 1)
    return res


# ---------------------------------------------------------------------------------------------- weight gradient
def tile_walk(P, bx, row_yz, ntiles):
    """(first, stride, count) of workgroup bx of the (ci-tile, output block) row `row_yz`: tile_walk of conv_mfma_wgrad.hip"""
    NX = min(P, 8)
    off = (P * row_yz) % NX
    grp = (bx + off) % NX
    p0 = (grp - off + NX) % NX
    slot, members = (bx - p0) // NX, (P - p0 + NX - 1) // NX
    r_lo, r_hi = ntiles * grp // NX, ntiles * (grp + 1) // NX
    first = r_lo + slot
    return first, members, ((r_hi - first + members - 1) // members if first < r_hi else 0)


def workgroup_tiles(pl, bx, row_yz=0):
    if pl["kernel"] == "cin1":
        return list(range(pl["ntiles"] * bx // pl["p"], pl["ntiles"] * (bx + 1) // pl["p"]))
    first, stride, count = tile_walk(pl["p"], bx, row_yz, pl["ntiles"])
    return [first + k * stride for k in range(count)]


def _w_order(kernel):
    if kernel == "wgrad6":
        return [j + 4 * kq for j in range(4) for kq in range(4)]
    if kernel == "bf16t":
        return [o + 4 * kq + i for kq in range(4) for o in (0, 16) for i in range(4)]
    return list(range(32 if kernel == "bf16" else 16))


def _wave_rows(pl, tile, wv, D):
    """[(n, d, h)] rows of wave wv in a tile / task, in order, and the tile's w0"""
    k = pl["kernel"]
    tw = tile % pl["tiles_w"]
    t = tile // pl["tiles_w"]
    if k in ("cin1", "wgrad3", "wgrad4"):
        th, t = t % pl["tiles_h"], t // pl["tiles_h"]
        td, n = t % pl["tiles_d"], t // pl["tiles_d"]
        half = pl["tile_h"] // 2
        rows = [(n, td * 2 + (wv >> 1), th * pl["tile_h"] + (wv & 1) * half + hr) for hr in range(half)]
    elif k in ("wgrad6", "bf16"):
        td, t = t % pl["tiles_d"], t // pl["tiles_d"]
        th, n = t % pl["tiles_h"], t // pl["tiles_h"]
        rows = [(n, td * 2 + (wv * 3 + r) // 6, th * 6 + (wv * 3 + r) % 6) for r in range(3)]
    else:
        th, t = t % pl["tiles_h"], t // pl["tiles_h"]
        seg, n = t % pl["tiles_d"], t // pl["tiles_d"]
        rows = [(n, d, th * 8 + 2 * wv + r) for d in range(seg * pl["segl"], min(D, (seg + 1) * pl["segl"])) for r in range(2)]
    return rows, tw * pl["tile_w"]


def wgrad(row, dtype, inp, pl, fault=None, sub=None):
    """{"dw": (Co, Ci, 3, 3, 3) fp32, "db": (Co) fp32 where the row asks for it}; sub: only the first `sub` input and output channels
    (every element of dw has the same sequence of voxels)"""
    k = pl["kernel"]
    transposed = k in ("wgrad6", "bf16", "bf16t")
    x, dy = inp["x"][:, :sub].float(), inp["dy"][:, :sub].float()
    N, ci, D, H, W = x.shape
    co = dy.shape[1]
    xp = torch.zeros((N + 1, D + 2, H + 2, W + 2, ci), dtype=F32)          # sample N: zeros, for padding and out-of-volume positions
    xp[:N, 1:-1, 1:-1, 1:-1] = x.permute(0, 2, 3, 4, 1)
    dp = torch.zeros((N + 1, D + 2, H + 2, W + 2, co), dtype=F32)
    dp[:N, 1:-1, 1:-1, 1:-1] = dy.permute(0, 2, 3, 4, 1)
    if fault == "w-halo-counted-into-dw":          # the voxel beyond the W edge repeats the last one: of X (tap kw = 2), of dY (the
        xp[:, :, :, W + 1] = xp[:, :, :, W]        # transposed tiles' left-shifted dY, tap kw = 0)
        dp[:, :, :, W + 1] = dp[:, :, :, W]
    P = pl["p"]
    lists = []
    for bx in range(P):
        tiles = workgroup_tiles(pl, bx)
        for wv in range(4):
            pos = []
            for t in tiles:
                rows, w0 = _wave_rows(pl, t, wv, D)
                for (n, d, h) in rows:
                    for u in _w_order(k):
                        ok = d < D and h < H and w0 + u < W
                        pos.append((n, d, h, w0 + u) if ok else (N, 0, 0, 0))
            lists.append(pos)
    L = max(len(p_) for p_ in lists)
    # the plan's chain is this emulation's longest sequence (bf16t: of whole segments, the plan counts segl planes for each)
    assert L == pl["chain"] or (k == "bf16t" and L <= pl["chain"]), (L, pl["chain"])
    if fault == "voxel-dropped-from-dw":
        lists[0][[i for i, q in enumerate(lists[0]) if q[0] < N][0]] = (N, 0, 0, 0)
    idx = torch.tensor([p_ + [(N, 0, 0, 0)] * (L - len(p_)) for p_ in lists]).view(P, 4, L, 4)
    acc = torch.zeros((P, 4, 27, ci, co), dtype=F32)
    accb = torch.zeros((P, 4, co), dtype=F32)
    taps = torch.arange(27)
    kd, kh, kw = (taps // 9).view(1, 1, 27), ((taps // 3) % 3).view(1, 1, 27), (taps % 3).view(1, 1, 27)
    for l in range(L):
        n, d, h, u = (idx[:, :, l, j].unsqueeze(-1) for j in range(4))          # (P, 4, 1)
        if transposed:
            xv = xp[n, d + kd, h + kh, u + 1]                                   # (P, 4, 27, ci)
            dv = dp[n, d + 1, h + 1, (u + 2 - kw).clamp(0, W + 1)]              # (P, 4, 27, co)
        else:
            xv = xp[n, d + kd, h + kh, u + kw]
            dv = dp[n, d + 1, h + 1, u + 1].expand(P, 4, 27, co)
        acc = _fma(acc, xv.unsqueeze(-1), dv.unsqueeze(-2))
        accb = accb + dp[n[..., 0], d[..., 0] + 1, h[..., 0] + 1, u[..., 0] + 1]
    part, partb = acc[:, 0], accb[:, 0]
    for wv in range(1, 4):
        part, partb = part + acc[:, wv], partb + accb[:, wv]
    if fault == "partial-dropped":
        part, partb = part[1:], partb[1:]
    res = {"dw": part.double().sum(0).float().permute(2, 1, 0).reshape(co, ci, 3, 3, 3)}
    if row.dbias:
        db = partb.double().sum(0).float()
        res["db"] = 2 * db if fault == "db-doubled" else db
    return res
