"""fp32 emulation of csrc/conv_march.hip on the CPU, in the kernel's order of summation, for tests/test_march_bounds.py: it shows that
the bounds of tests/march_ref.py hold for an honest fp32 evaluation and that the errors the kernel's corners can make leave them.

What is modelled, per d segment of the launch plan (tests/march_run.plans): the input planes max(dlo - 1, 0) .. min(dhi, D - 1) are
consumed in order; output plane o lives in accumulator slot o mod 3, slot s receives tap plane kd(s) of the input plane p with
(kd(0), kd(1), kd(2)) rotating by one per plane from 2 - ((s - plo + 1) mod 3); a slot restarts from zero with the kd = 0 group of
the plane's first chunk; per plane the chunks of 8 fp32 / 16 bf16 input channels in turn, per chunk phase A (kh = 0, 1, 2 on the
kw = 0 | 1 pair), phase B (kw = 2, kh = 0 | 1), phase C (the tap (2, 2)): one fp32 dot product per group (the matrix unit's order
inside an instruction is not modelled), added to the slot in fp32.  Rows h0 .. h0 + 7 and voxels w0 .. w0 + 15 of every column
are accumulated, also those outside the volume (from the zero-filled halo); output plane p - 2 is stored when plane p arrives: the
statistics lanes add the stored accumulators (rows inside the volume) in fp32, then the bias, the rounding to the storage type.
The input is read from a flat NDHWC buffer whose unread channels hold NaN, as the device run lays it out (tests/march_run.py); the
output channels of a 16-block are permuted as pack_w_march_kernel and the epilogue permute them (twice = not at all).

FAULTS: the deliberate errors, by name."""
import torch

import march_run as run

FAULTS = ("tap-dropped-on-a-border-voxel", "halo-plane-missing-at-a-segment-start", "rotation-not-offset-by-the-first-plane",
          "sigma-permutation-left-out", "slot-not-restarted", "bias-added-twice", "ragged-row-in-the-statistics",
          "inactive-voxel-lane-in-the-statistics", "half-chunk-not-zero-filled", "neighbouring-slice-read")
F32 = torch.float32
GROUPS = ([[(kh, 0), (kh, 1)] for kh in range(3)] + [[(0, 2), (1, 2)]] + [[(2, 2)]])      # phase A x 3, phase B, phase C: (kh, kw)


class _Source:
    """channel kc of the pass's input as fp32 planes, read out of the flat buffers the entry point is handed"""

    def __init__(self, row, dtype, inp, p):
        st = run.TORCH[dtype]
        c1 = row.split or row.ci
        if p == "fwd":
            parts = [(inp["x"][:, :c1], "x")] + ([(inp["x"][:, c1:], "x2")] if row.split else [])
        else:
            parts = [(inp["dy"], "y")]
        self.parts, self.first = [], c1
        for t, name in parts:
            ld, o = run.width(row, name), run.off(row, name)
            buf = torch.full((t.shape[0],) + tuple(t.shape[2:]) + (ld,), run.NAN, dtype=st)
            buf[..., o:o + t.shape[1]] = t.to(st).permute(0, 2, 3, 4, 1)
            wider = torch.cat((buf.flatten(), torch.full((64,), run.NAN, dtype=st)))
            self.parts.append((wider.float(), run.width(row, name), run.off(row, name), t.shape[1]))
        self.shape = (inp["x"].shape[0],) + tuple(inp["x"].shape[2:])
        self.nvox = self.shape[0] * self.shape[1] * self.shape[2] * self.shape[3]

    def holder(self, kc):
        """(part index, channel inside the part) of input channel kc: the second tensor holds the channels from the split on"""
        return (1, kc - self.first) if len(self.parts) > 1 and kc >= self.first else (0, kc)

    def channel(self, part, k):
        """channel slot k of a part (k past its channels: whatever lies there in memory) -> (N, D, H, W) fp32"""
        flat, ld, off, _ = self.parts[part]
        idx = torch.arange(self.nvox) * ld + off + k
        return flat[idx].view(self.shape)


def _tree16(v):
    """the four additions of row_sum16 over groups of 16 lanes (last axis), fp32"""
    v = v.reshape(v.shape[:-1] + (v.shape[-1] // 16, 16))
    for h in (8, 4, 2, 1):
        v = v[..., :h] + v[..., h:2 * h]
    return v[..., 0]


def emulate(row, dtype, inp, pl, p, fault=None):
    """{"y" | "dx": the stored result (N, Nc, D, H, W) in the storage type, "stats": (Nc, 2) float64 where the row asks for them}"""
    assert fault is None or fault in FAULTS
    bf = dtype == "bf16"
    CK = 16 if bf else 8
    N, (D, H, W) = row.n, row.sp
    w = inp["w"].to(torch.bfloat16).float() if bf else inp["w"].float()
    if p == "dgrad":
        w = w.transpose(0, 1).flip(2, 3, 4).contiguous()          # dx = conv(dy, W[kc][nc][26 - tap])
    Nc, Kc = w.shape[:2]
    nch, nbl = pl["chunks"], pl["blocks"]
    wp = torch.zeros((nbl * 16, nch * CK, 3, 3, 3), dtype=F32)
    wp[:Nc, :Kc] = w
    bias = torch.zeros(nbl * 16, dtype=F32)
    if p == "fwd" and inp["b"] is not None:
        bias[:Nc] = inp["b"].float()
    stats = row.stats and p == "fwd"
    src = _Source(row, dtype, inp, p)
    colsH, colsW = -(-H // 8), -(-W // 16)
    Hp, Wp = colsH * 8, colsW * 16
    out = torch.zeros((N, Nc, D, H, W), dtype=run.TORCH[dtype])
    total = torch.zeros((nbl * 16, 2), dtype=torch.float64)

    def planes_of(pz):
        """[chunk][slot in chunk] -> zero-padded halo plane (N, Hp + 2, Wp + 2) of input plane pz"""
        res = []
        for c in range(nch):
            chans = []
            for j in range(CK):
                kc = c * CK + j
                part, k = src.holder(min(kc, Kc - 1))
                k += kc - min(kc, Kc - 1)
                if fault == "neighbouring-slice-read" and kc >= Kc - 8:
                    k += 8
                if kc >= Kc and fault != "half-chunk-not-zero-filled":
                    chans.append(None)
                    continue
                halo = torch.zeros((N, Hp + 2, Wp + 2), dtype=F32)
                halo[:, 1:H + 1, 1:W + 1] = src.channel(part, k)[:, pz]
                chans.append(halo)
            res.append(chans)
        return res

    for seg in range(pl["nseg"]):
        dlo = seg * pl["seglen"]
        dhi = min(dlo + pl["seglen"], D)
        if dlo >= D:
            continue
        plo, phi = max(dlo - 1, 0), min(dhi, D - 1)
        first = plo + 1 if (fault == "halo-plane-missing-at-a-segment-start" and seg > 0) else plo
        slots = torch.zeros((3, N, nbl * 16, Hp, Wp), dtype=F32)
        s1 = torch.zeros((N, nbl * 16, colsH, Wp), dtype=F32)
        s2 = torch.zeros_like(s1)
        rot = 0 if fault == "rotation-not-offset-by-the-first-plane" else first
        kds = [2 - (s - rot + 1) % 3 for s in range(3)]

        def store(o):
            nonlocal s1, s2
            acc = slots[o % 3]
            if stats:
                for ch in range(colsH):
                    rows = 8 if fault == "ragged-row-in-the-statistics" else min(8, H - ch * 8)
                    for m in range(rows):
                        v = acc[:, :, ch * 8 + m]
                        s1[:, :, ch] = s1[:, :, ch] + v
                        s2[:, :, ch] = v * v + s2[:, :, ch]
            vals = acc + bias.view(1, -1, 1, 1)
            if fault == "bias-added-twice":
                vals = vals + bias.view(1, -1, 1, 1)
            if fault == "sigma-permutation-left-out":          # the weight rows of quads 1 and 2 change places, the epilogue's do not
                q = vals.view(N, nbl, 4, 4, Hp, Wp)
                vals = q[:, :, [0, 2, 1, 3]].reshape(N, nbl * 16, Hp, Wp)
            out[:, :, o] = vals[:, :Nc, :H, :W].to(out.dtype)

        for pz in range(first, phi + 1):
            if pz - 2 >= dlo:
                store(pz - 2)
            halos = planes_of(pz)
            for c in range(nch):
                live = [j for j in range(CK) if halos[c][j] is not None]
                for s in range(3):
                    kd = kds[s]
                    acc = slots[s]
                    if kd == 0 and c == 0 and fault != "slot-not-restarted":
                        acc = torch.zeros_like(acc)
                    for grp in GROUPS:
                        xs = torch.stack([halos[c][j][:, kh:kh + Hp, kw:kw + Wp] for kh, kw in grp for j in live], 1)
                        wg = torch.stack([wp[:, c * CK + j, kd, kh, kw] for kh, kw in grp for j in live], 1)
                        prod = torch.einsum("nkhw,ok->nohw", xs, wg)
                        if fault == "half-chunk-not-zero-filled" or fault == "neighbouring-slice-read":
                            prod = (xs[:, None] * wg[None, :, :, None, None]).sum(2)      # 0 x NaN must stay NaN
                        acc = acc + prod
                    slots[s] = acc
            kds = [0 if k == 2 else k + 1 for k in kds]
        if phi - 1 >= dlo:
            store(phi - 1)
        if phi < dhi:
            store(phi)
        if stats:
            ok = (torch.arange(Wp) < W).float()
            if fault == "inactive-voxel-lane-in-the-statistics":
                ok = torch.ones(Wp)
            total[:, 0] += _tree16(s1 * ok).double().sum((0, 2, 3))
            total[:, 1] += _tree16(s2 * ok).double().sum((0, 2, 3))
    if fault == "tap-dropped-on-a-border-voxel":              # the tap (1, 1, 2) of the first voxel of the volume
        xs = torch.stack([src.channel(*src.holder(kc))[0, 0, 0, 1] for kc in range(Kc)])
        out[0, :, 0, 0, 0] = (out[0, :, 0, 0, 0].float() - (wp[:Nc, :Kc, 1, 1, 2] * xs).sum(1)).to(out.dtype)
    res = {"y" if p == "fwd" else "dx": out}
    if stats:
        res["stats"] = total[:Nc]
    return res
