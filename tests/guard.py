"""Guard bands around kernel-written buffers, and a float64 reference of a convolution at chosen output voxels.

A kernel that writes past the memory it was handed does not fault while the bytes still belong to some torch allocation; it
silently corrupts a neighbouring tensor.  `guarded` puts the region handed to the kernel between two sentinel-filled guards in
ONE allocation, so an overrun lands in the test's own memory and `assert_guards_intact` names the first overwritten element.
Sentinels are NaN payloads compared bit for bit through an integer view (a kernel that writes a NaN of its own is still seen)."""
import numpy as np
import torch

CL3D = torch.channels_last_3d

# dtype -> (integer view of the same width, sentinel bits)
SENTINELS = {
    torch.float32: (torch.int32, 0x7FC0DEAD),
    torch.bfloat16: (torch.int16, 0x7FDE),
    torch.float64: (torch.int64, 0x7FF8DEADBEEF0001),
    torch.uint8: (torch.uint8, 0xA5),
}

GUARD_FRONT = 64 << 10   # bytes; a multiple of 256, so the region keeps the allocation's alignment
GUARD_BACK = 4 << 20     # bytes; more than 512 statistics blocks of 128 channels (1 MiB) or a 16-channel voxel row past the end


def _bits(t):
    return t.view(SENTINELS[t.dtype][0])


def _first_mismatch(bits, value):
    bad = (bits != value).nonzero()
    return None if bad.numel() == 0 else int(bad[0, 0])


class Guarded:
    """One allocation = front guard | region | back guard, all filled with the dtype's sentinel."""

    def __init__(self, numel_or_shape, dtype, device="cuda", front=GUARD_FRONT, back=GUARD_BACK):
        shape = (int(numel_or_shape),) if isinstance(numel_or_shape, (int, np.integer)) else tuple(int(s) for s in numel_or_shape)
        esz = torch.empty((), dtype=dtype).element_size()
        assert front % 256 == 0 and front % esz == 0 and back % esz == 0
        self.shape, self.dtype, self.esz = shape, dtype, esz
        self.numel = int(np.prod(shape, dtype=np.int64))
        self.nf, self.nb = front // esz, back // esz
        self.storage = torch.empty(self.nf + self.numel + self.nb, dtype=dtype, device=device)
        self.sentinel = SENTINELS[dtype][1]
        _bits(self.storage).fill_(self.sentinel)
        self.flat = self.storage[self.nf:self.nf + self.numel]
        self.region = self.flat.view(shape)

    def assert_guards_intact(self, what="buffer"):
        bits = _bits(self.storage)
        i = _first_mismatch(bits[:self.nf], self.sentinel)
        if i is not None:
            raise AssertionError("%s: front guard overwritten, first at %d bytes before the region (%d-element region of %s)"
                                 % (what, (self.nf - i) * self.esz, self.numel, self.dtype))
        i = _first_mismatch(bits[self.nf + self.numel:], self.sentinel)
        if i is not None:
            last = int((bits[self.nf + self.numel:] != self.sentinel).nonzero()[-1, 0])
            raise AssertionError("%s: back guard overwritten, first at element %d past the end (byte %d), last at element %d "
                                 "(%d-element region of %s)" % (what, i, i * self.esz, last, self.numel, self.dtype))

    def untouched(self):
        """Boolean mask (region shape) of the elements that still hold the sentinel bits."""
        return (_bits(self.flat) == self.sentinel).view(self.shape)


def guarded(numel_or_shape, dtype, front=GUARD_FRONT, back=GUARD_BACK, device="cuda"):
    return Guarded(numel_or_shape, dtype, device=device, front=front, back=back)


class SentinelSlice:
    """An NDHWC buffer of `channels` channels (itself inside guard bands), every element holding the sentinel, and its channel
    slice [off, off + c) as a logical (N, c, D, H, W) view for a producer to write.  `assert_outside_intact` checks that every
    channel outside the slice, and both guards, kept their bits."""

    def __init__(self, n, channels, spatial, dtype, off, c, device="cuda"):
        d, h, w = spatial
        self.g = Guarded((n, d, h, w, channels), dtype, device=device)
        self.buf = self.g.region.permute(0, 4, 1, 2, 3)          # logical NCDHW over NDHWC memory
        assert self.buf.is_contiguous(memory_format=CL3D)
        self.off, self.c, self.channels = off, c, channels
        self.slice = self.buf.narrow(1, off, c)

    def assert_outside_intact(self, what="pitched destination"):
        self.g.assert_guards_intact(what)
        bits = _bits(self.g.region)
        outside = torch.ones(self.channels, dtype=torch.bool, device=bits.device)
        outside[self.off:self.off + self.c] = False
        bad = (bits[..., outside] != self.g.sentinel)
        if bool(bad.any()):
            idx = bad.nonzero()[0].tolist()
            ch = outside.nonzero()[idx[4], 0].item()
            raise AssertionError("%s: channel %d outside the slice [%d, %d) overwritten at (n, d, h, w) = %s (%d elements)"
                                 % (what, ch, self.off, self.off + self.c, tuple(idx[:4]), int(bad.sum())))

    def slice_untouched(self):
        return _bits(self.g.region)[..., self.off:self.off + self.c] == self.g.sentinel


def sample_voxels(n, d, h, w, count=4000, seed=0):
    """(V, 4) int64 output coordinates (sample, d, h, w): the 8 corners of the first and the last sample, points on all 6 faces and
    12 edges, and `count` random voxels (interior ones where the volume has an interior)."""
    g = torch.Generator().manual_seed(seed)

    def r(hi, k):
        return torch.randint(0, hi, (k,), generator=g)
    pts = []
    for s in sorted({0, n - 1}):
        for cd in (0, d - 1):
            for ch in (0, h - 1):
                for cw in (0, w - 1):
                    pts.append(torch.tensor([[s, cd, ch, cw]]))
    k = 16
    ns = r(n, k)
    for axis, ext in ((1, d), (2, h), (3, w)):       # faces: one coordinate pinned to 0 or ext - 1
        for v in (0, ext - 1):
            p = torch.stack((ns, r(d, k), r(h, k), r(w, k)), 1)
            p[:, axis] = v
            pts.append(p)
    for free, ext in ((1, d), (2, h), (3, w)):       # edges: the two other coordinates pinned
        pinned = [a for a in (1, 2, 3) if a != free]
        exts = {1: d, 2: h, 3: w}
        for v0 in (0, exts[pinned[0]] - 1):
            for v1 in (0, exts[pinned[1]] - 1):
                p = torch.stack((ns, r(d, k), r(h, k), r(w, k)), 1)
                p[:, pinned[0]], p[:, pinned[1]] = v0, v1
                pts.append(p)
    lo = [1 if e > 2 else 0 for e in (d, h, w)]
    interior = torch.stack((r(n, count),) + tuple(lo[i] + r(max(1, e - 2 * lo[i]), count) for i, e in enumerate((d, h, w))), 1)
    pts.append(interior)
    return torch.unique(torch.cat(pts, 0), dim=0)


def gather_voxels(t, vox):
    """t[n, :, d, h, w] at the (V, 4) coordinates -> (V, C) on the host (t is a logical NCDHW device tensor)."""
    v = vox.to(t.device)
    return t[v[:, 0], :, v[:, 1], v[:, 2], v[:, 3]].detach().cpu()


def conv3d_ref_at(x, w, b, stride, pad, dil, voxels):
    """float64 reference of conv3d(x, w, b, stride, pad, dil) at the output voxels (V, 4) -> (V, Co).  x may live on the device
    (only the V x taps input vectors the voxels need are gathered); w, b are used as given (round them first for bf16)."""
    stride, pad, dil = (tuple(v) if isinstance(v, (tuple, list)) else (v,) * 3 for v in (stride, pad, dil))
    n, ci, di, hi, wi = x.shape
    co, _, kd, kh, kw = w.shape
    v = voxels.to(x.device)
    cols = []
    for a in range(kd):
        for bb in range(kh):
            for c in range(kw):
                zd = v[:, 1] * stride[0] - pad[0] + a * dil[0]
                zh = v[:, 2] * stride[1] - pad[1] + bb * dil[1]
                zw = v[:, 3] * stride[2] - pad[2] + c * dil[2]
                ok = (zd >= 0) & (zd < di) & (zh >= 0) & (zh < hi) & (zw >= 0) & (zw < wi)
                vals = x[v[:, 0], :, zd.clamp(0, di - 1), zh.clamp(0, hi - 1), zw.clamp(0, wi - 1)].double()
                cols.append(torch.where(ok[:, None], vals, torch.zeros_like(vals)).cpu())
    xs = torch.stack(cols, 2)                                   # (V, Ci, taps)
    wm = w.detach().double().cpu().reshape(co, ci, kd * kh * kw)
    y = torch.einsum("vct,oct->vo", xs, wm)
    if b is not None:
        y = y + b.detach().double().cpu()[None, :]
    return y


def kernels_launched(fn):
    """Run fn() under the torch profiler; returns (fn's result, the set of device kernel names it launched)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    names = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}
    return out, names
