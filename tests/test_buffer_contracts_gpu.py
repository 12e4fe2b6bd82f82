"""Buffer contracts of the kernel-written memory: every buffer a host query sizes and a separately dispatched kernel fills is
checked for writes OUTSIDE it, not only for the values inside it (tests/guard.py).

  * BatchNorm statistics partials stat_partials[blocks][co][2] of the fused forward (plain and split operand), per dispatcher
    route: exactly the queried blocks inside sentinel guards; all of them written; their sums equal float64 sums over the returned
    y; y itself against a float64 reference at sampled voxels (corners, faces, edges, ~4000 random ones) of full volumes.
  * Workspaces: every operator gets exactly the bytes it asked for, poisoned (0xA5 bytes, then fp32 NaN) and guarded; its
    results must be bit-identical to a run with the normal grow-only workspace (a kernel that reads workspace it did not write
    first, or writes past it, shows up).
  * Pitched / sliced destinations: channels outside the slice keep their sentinel bits; inside, the values match a reference.

Every route is checked to be the one actually taken by the names of the kernels it launches (torch profiler), so a dispatcher
change that moves a shape to another kernel fails here instead of silently dropping that route's coverage."""
import ctypes
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc
import norm_cases as nc
from guard import SentinelSlice, conv3d_ref_at, gather_voxels, guarded, kernels_launched, sample_voxels
from mri_epilepsy_diagnosis_amd import _lib, ops

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32 = torch.float32
CL = torch.channels_last_3d
DT = {"f32": F32, "bf16": BF}


def _rand(seed, shape, dtype):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, generator=g, device="cuda").to(dtype).contiguous(memory_format=CL)


def _route(names, pattern, what):
    assert any(re.search(pattern, n) for n in names), "%s: expected a kernel matching %r, launched %s" % (what, pattern, sorted(names))


def _ref_close(got, ref, dtype, what):
    """fp32: 1e-3 max-norm relative; bf16: 2 bf16 ulp + 2e-3 of the scale (inputs and weights bf16-rounded in the reference)."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs()
    if dtype == BF:
        bad = err > 2.0 * 2.0 ** -8 * ref.abs() + 2e-3 * scale
        assert not bool(bad.any()), "%s: %d/%d outside tolerance, max err %.3e (scale %.3e)" % (what, int(bad.sum()), bad.numel(),
                                                                                                 err.max().item(), scale)
    else:
        assert err.max().item() <= 1e-3 * scale, "%s: max-norm relative error %.3e" % (what, err.max().item() / scale)


def _wq(w, dtype):
    return w.to(BF).double() if dtype == BF else w.double()   # the MFMA kernels round the weights to the tensor dtype


# ------------------------------------------------------------------------------------------------ a. statistics partials


def _fwd_stats_capi(xa, w, b, xb=None):
    """conv(cat((xa, xb)), w) + b with fused statistics through the C ABI; the partials are EXACTLY the queried blocks inside a
    guarded float64 buffer.  -> (y, Guarded partials, blocks, kernel names)."""
    L = _lib.lib()
    n, ca = xa.shape[:2]
    cb = 0 if xb is None else xb.shape[1]
    co = w.shape[0]
    sp = tuple(xa.shape[2:])
    g = ops._conv_geom((n, ca + cb) + sp, w.shape, (1, 1, 1), (1, 1, 1), (1, 1, 1), x_ld=ops._pitch_of(xa), y_ld=co, dtype=ops._dt(xa))
    b_ld = None if xb is None else ops._pitch_of(xb)
    if xb is None:
        blocks = L.mri3d_conv3d_fwd_stats_blocks(ctypes.byref(g))
    else:
        assert L.mri3d_conv3d_cat_supported(ctypes.byref(g), ca, b_ld, _lib.PASS_FWD) == 1
        blocks = L.mri3d_conv3d_fwd_cat_stats_blocks(ctypes.byref(g), ca, b_ld)
    assert blocks > 0
    part = guarded((blocks, co, 2), torch.float64)
    y = torch.empty((n, co) + sp, dtype=xa.dtype, device="cuda", memory_format=CL)
    ws = ops._workspace(L.mri3d_conv3d_workspace_bytes(ctypes.byref(g), _lib.PASS_FWD), xa.device)

    def call():
        if xb is None:
            rc = L.mri3d_conv3d_fwd_stats(ctypes.byref(g), ops._ptr(xa), ops._ptr(w), ops._ptr(b), ops._ptr(y), ops._ptr(part.region),
                                          ops._ptr(ws), ws.numel(), ops._stream())
        else:
            rc = L.mri3d_conv3d_fwd_cat(ctypes.byref(g), ops._ptr(xa), ops._ptr(xb), ca, b_ld, ops._ptr(w), ops._ptr(b), ops._ptr(y),
                                        ops._ptr(part.region), ops._ptr(ws), ws.numel(), ops._stream())
        _lib.check(rc, "conv3d_fwd_stats")
    _, names = kernels_launched(call)
    return y, part, blocks, names


def _check_stats(y, b, part, dtype, what):
    """Every queried block written; sum(a), sum(a^2) of a = y - bias equal float64 sums over the returned y."""
    untouched = part.untouched()
    assert not bool(untouched.any()), "%s: %d of %d partial blocks never written" % (what, int(untouched.any(2).any(1).sum()),
                                                                                   untouched.shape[0])
    sums = part.region.sum(0)                                       # (co, 2) float64
    a = y.double() - (b.double().view(1, -1, 1, 1, 1) if b is not None else 0.0)
    s1, s2 = a.sum((0, 2, 3, 4)), (a * a).sum((0, 2, 3, 4))
    abs1 = a.abs().sum((0, 2, 3, 4))
    del a
    # the statistics are taken from the fp32 accumulators, before the result is rounded for storage
    tol = 1e-4 if dtype == BF else 1e-6
    e1 = ((sums[:, 0] - s1).abs() / abs1).max().item()
    e2 = ((sums[:, 1] - s2).abs() / s2).max().item()
    assert e1 <= tol and e2 <= tol, "%s: statistics sums off by %.3e (sum a, relative to sum |a|) / %.3e (sum a^2)" % (what, e1, e2)


# the cases (id, dtype, n, ca, cb, second-tensor pitch, co, volume, kernel the dispatcher must pick): cc.CAPI_STATS
@pytest.mark.parametrize("case", cc.CAPI_STATS.cases, ids=cc.CAPI_STATS.ids)
def test_statistics_partials_stay_inside_the_queried_blocks(case):
    cid, dtype_id, n, ca, cb, ld2, co, sp, route = case
    dtype = DT[dtype_id]
    seed = 100 + sum(sp) + ca + cb + ld2 + co
    xa = _rand(seed, (n, ca) + sp, dtype)
    xb = None
    if cb:
        bbuf = _rand(seed + 1, (n, ld2) + sp, dtype)
        xb = bbuf[:, ld2 - cb:]                                        # a channel slice of a wider buffer when ld2 > cb
        assert ops._pitch_of(xb) == ld2
    g = torch.Generator().manual_seed(seed + 2)
    w = (torch.randn(co, ca + cb, 3, 3, 3, generator=g) / np.sqrt(27 * (ca + cb))).cuda()
    b = (torch.randn(co, generator=g) * 0.1).cuda()
    cc.CAPI_STATS.check(case, dtype_id, x=xa if xb is None else xb)
    y, part, blocks, names = _fwd_stats_capi(xa, w, b, xb)
    _route(names, route, cid)
    part.assert_guards_intact("%s: statistics partials (%d blocks x %d channels)" % (cid, blocks, co))
    _check_stats(y, b, part, dtype, cid)
    vox = sample_voxels(n, *sp, seed=seed)
    ref = conv3d_ref_at(xa, _wq(w[:, :ca], dtype), b, 1, 1, 1, vox)
    if xb is not None:
        ref += conv3d_ref_at(xb, _wq(w[:, ca:], dtype), None, 1, 1, 1, vox)
    _ref_close(gather_voxels(y, vox), ref, dtype, cid + ": y at %d sampled voxels" % vox.shape[0])
    if cid.startswith("f32_cat_ld"):
        # the same layer through ops.conv3d_cat: the partials it allocates have the launched kernel's block count
        L = _lib.lib()
        ys = ops.conv3d_cat(xa, xb, w.requires_grad_(True), b, padding=1, bn_stats=True)
        assert "Conv3dCatFn" in type(ys.grad_fn).__name__
        st = ys._mri3d_bn_stats
        gw = ops._conv_geom((n, ca + cb) + sp, w.shape, (1, 1, 1), (1, 1, 1), (1, 1, 1), dtype=ops._dt(xa))
        assert st[1] == blocks and blocks != L.mri3d_conv3d_fwd_stats_blocks(ctypes.byref(gw)), (st[1], blocks)
        assert torch.equal(ys, y)
        assert torch.equal(st[0].view(blocks, co, 2), part.region)


def test_no_fused_statistics_on_the_narrow_kernel():
    """Volumes at most 8 voxels wide (fp32) run on the LDS-free kernel, which has no statistics epilogue: the query answers 0, the
    entry point refuses a partials pointer without writing it, and ops.conv3d(bn_stats=True) falls back to the plain forward."""
    L = _lib.lib()
    torch.manual_seed(7)
    x = _rand(7, (64, 16, 8, 8, 8), F32)
    w = torch.randn(16, 16, 3, 3, 3, device="cuda") * 0.1
    b = torch.randn(16, device="cuda")
    g = ops._conv_geom(tuple(x.shape), w.shape, (1, 1, 1), (1, 1, 1), (1, 1, 1), dtype=_lib.F32)
    assert L.mri3d_conv3d_fwd_stats_blocks(ctypes.byref(g)) == 0
    part = guarded((64, 16, 2), torch.float64)
    y = torch.empty_like(x)
    ws = ops._workspace(L.mri3d_conv3d_workspace_bytes(ctypes.byref(g), _lib.PASS_FWD), x.device)
    rc = L.mri3d_conv3d_fwd_stats(ctypes.byref(g), ops._ptr(x), ops._ptr(w), ops._ptr(b), ops._ptr(y), ops._ptr(part.region),
                                  ops._ptr(ws), ws.numel(), ops._stream())
    torch.cuda.synchronize()
    assert rc == -2, rc                                                # MRI3D_ENOTSUP
    part.assert_guards_intact("refused partials")
    assert bool(part.untouched().all())
    ys, names = kernels_launched(lambda: ops.conv3d(x, w, b, padding=1, bn_stats=True))
    _route(names, r"conv_mfma_direct_kernel", "narrow forward")
    assert getattr(ys, "_mri3d_bn_stats", None) is None
    assert torch.equal(ys, ops.conv3d(x, w, b, padding=1))


# ------------------------------------------------------------------------------------------------ b. workspaces


class _ExactWorkspaces:
    """Stands in for ops._workspace: each call gets a fresh region of exactly `nbytes` (no 1 MiB minimum) between 0xA5 guards,
    poisoned with 0xA5 bytes ("a5") or fp32 NaN bits ("nan")."""

    def __init__(self, fill):
        self.fill, self.bufs = fill, []

    def __call__(self, nbytes, device):
        gb = guarded(int(nbytes), torch.uint8, device=device)
        if self.fill == "nan" and nbytes >= 4:
            gb.flat[:int(nbytes) // 4 * 4].view(torch.int32).fill_(0x7FC0DEAD)
        self.bufs.append(gb)
        return gb.region

    def assert_intact(self, what):
        for i, gb in enumerate(self.bufs):
            gb.assert_guards_intact("%s: workspace #%d (%d bytes)" % (what, i, gb.numel))


def _same_bits(a, b):
    if a.dtype.is_floating_point:
        iv = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}[a.dtype]
        a, b = a.contiguous().view(iv), b.contiguous().view(iv)
    return a.shape == b.shape and torch.equal(a, b)


def _conv_case(n, ci, co, sp, dtype, k=3, pad=1, dil=1, seed=0):
    def run():
        x = _rand(seed, (n, ci) + sp, dtype).requires_grad_(True)
        g = torch.Generator().manual_seed(seed + 1)
        w = (torch.randn(co, ci, k, k, k, generator=g) / np.sqrt(k ** 3 * ci)).cuda().requires_grad_(True)
        b = torch.randn(co, generator=g).cuda().requires_grad_(True)
        y = ops.conv3d(x, w, b, 1, pad, dil)
        y.backward(_rand(seed + 2, tuple(y.shape), dtype))
        return [y.detach(), x.grad, w.grad, b.grad]
    return run


def _convt_case():
    def run():
        x = _rand(11, (2, 16, 6, 7, 8), F32).requires_grad_(True)
        g = torch.Generator().manual_seed(12)
        w = (torch.randn(16, 8, 2, 2, 2, generator=g) * 0.2).cuda().requires_grad_(True)
        b = torch.randn(8, generator=g).cuda().requires_grad_(True)
        y = ops.conv_transpose3d(x, w, b, stride=2)
        y.backward(_rand(12, tuple(y.shape), F32))
        return [y.detach(), x.grad, w.grad, b.grad]
    return run


def _upconv_case():
    def run():
        x = _rand(13, (2, 8, 3, 4, 5), F32).requires_grad_(True)
        g = torch.Generator().manual_seed(14)
        w = (torch.randn(1, 8, 3, 1, 1, generator=g) * 0.3).cuda().requires_grad_(True)
        b = torch.randn(1, generator=g).cuda().requires_grad_(True)
        assert ops.upsample_conv3d_supported(x, w, 4, 1, (1, 0, 0), 1)
        y = ops.upsample_conv3d(x, 4, w, b, padding=(1, 0, 0))
        y.backward(_rand(15, tuple(y.shape), F32))
        return [y.detach(), x.grad, w.grad, b.grad]
    return run


def _pair_case():
    class Conv:   # what ops.conv3d_pair reads of an nn.Conv3d
        def __init__(self, w, b, stride, padding):
            self.weight, self.bias, self.stride, self.padding, self.dilation = w, b, stride, padding, (1, 1, 1)

    def run():
        x = _rand(16, (2, 1, 12, 10, 9), F32)
        g = torch.Generator().manual_seed(17)
        ps = [t.cuda().requires_grad_(True) for t in (torch.randn(8, 1, 6, 1, 1, generator=g) * 0.4, torch.randn(8, generator=g),
                                                      torch.randn(8, 8, 1, 6, 1, generator=g) * 0.2, torch.randn(8, generator=g))]
        c1, c2 = Conv(ps[0], ps[1], (2, 1, 1), (2, 0, 0)), Conv(ps[2], ps[3], (1, 2, 1), (0, 2, 0))
        assert ops.conv3d_pair_supported(x, c1, c2)
        y = ops.conv3d_pair(x, c1, c2)
        y.backward(_rand(18, tuple(y.shape), F32))
        return [y.detach()] + [p.grad for p in ps]
    return run


def _norm_case(mode, dtype=F32):
    def run():
        x = _rand(19, (2, 16, 9, 10, 11), dtype).requires_grad_(True)
        g = torch.Generator().manual_seed(20)
        gamma, beta = (1 + 0.1 * torch.randn(16, generator=g)).cuda().requires_grad_(True), (0.1 * torch.randn(16, generator=g)).cuda().requires_grad_(True)
        alpha = torch.full((1,), 0.25, device="cuda").requires_grad_(True)
        rm, rv = torch.zeros(16, device="cuda"), torch.ones(16, device="cuda")
        y = ops.norm_act(x, gamma, beta, alpha, rm if mode == "batch" else None, rv if mode == "batch" else None, stats_mode=mode,
                         act="prelu", group_c=4 if mode == "group" else 0)
        y.backward(_rand(21, tuple(y.shape), dtype))
        return [y.detach(), x.grad, gamma.grad, beta.grad, alpha.grad, rm, rv]
    return run


def _norm_row_case(row_id, dtype_id):
    """A row of tests/norm_cases.py (its plans are asserted before the launch): the geometries whose block count the workspace
    formula treats apart, groups * nblk > kNormMaxBlocks."""
    row = nc.BY_ID[row_id]

    def run():
        res, _ = nc.run_row(row, dtype_id, nc.make_inputs(row, dtype_id))
        return [res[k] for k in ("y", "dx", "dgamma", "dbeta", "dalpha") if res[k] is not None]
    return run


def _upsample_case(mode):
    def run():
        x = _rand(22, (2, 16, 6, 7, 8), F32).requires_grad_(True)
        y = ops.upsample3d(x, scale_factor=2, mode=mode, align_corners=False if mode == "trilinear" else None)
        y.backward(_rand(23, tuple(y.shape), F32))
        return [y.detach(), x.grad]
    return run


def _dice_case():
    def run():
        logits = _rand(24, (2, 3, 9, 10, 11), F32).requires_grad_(True)
        g = torch.Generator(device="cuda").manual_seed(25)
        t = (torch.rand(2, 1, 9, 10, 11, generator=g, device="cuda") < 0.3).float()
        loss = ops.softmax_dice_loss(logits, t)
        loss.backward()
        return [loss.detach(), logits.grad]
    return run


def _overlap_case():
    def run():
        g = torch.Generator(device="cuda").manual_seed(26)
        p = (torch.rand(2, 30, 31, 33, generator=g, device="cuda") < 0.4).to(torch.uint8)
        q = (torch.rand(2, 30, 31, 33, generator=g, device="cuda") < 0.4).to(torch.uint8)
        return [ops.mask_overlap_counts(p, q)]
    return run


def _ws_conv(case):
    """A row of cc.WS_CONV as (id, run, kernel pattern); the route the row declares is asserted when the case runs."""
    cid, dtype_id, n, ci, co, sp, k, pad, dil, seed, pattern = case
    run = _conv_case(n, ci, co, sp, DT[dtype_id], k=k, pad=pad, dil=dil, seed=seed)

    def checked():
        cc.WS_CONV.check(case, dtype_id)
        return run()
    return cid, checked, pattern


def _ws_wgrad(case):
    """A row of cc.WS_WGRAD as (id, run, kernel pattern): x and the incoming gradient are channel slices of wider buffers; the routes
    the row declares are asserted with the real tensors before the passes run."""
    cid, dtype_id, (n, ci, co, sp, k, s, p, dil, bias, pad_in, pad_out), dy_off, seed, pattern = case
    dtype = DT[dtype_id]

    def run():
        x = _rand(seed, (n, ci + pad_in) + sp, dtype)[:, pad_in:].detach().requires_grad_(True)
        g = torch.Generator().manual_seed(seed + 1)
        w = (torch.randn(co, ci, *k, generator=g) / np.sqrt(k[0] * k[1] * k[2] * ci)).cuda().requires_grad_(True)
        b = torch.randn(co, generator=g).cuda().requires_grad_(True)
        geom = ops._conv_geom(tuple(x.shape), w.shape, s, p, dil)
        dy = _rand(seed + 2, (n, co + pad_out, geom.dout, geom.ho, geom.wo), dtype)[:, dy_off:dy_off + co]
        cc.WS_WGRAD.check(case, dtype_id, x=x, dy=dy)
        y = ops.conv3d(x, w, b, s, p, dil)
        y.backward(dy)
        return [y.detach(), x.grad, w.grad, b.grad]
    return cid, run, pattern


# (id, case, kernel that must be among the launched ones, or None); the convolutions: cc.WS_CONV, cc.WS_WGRAD
WS_CASES = [_ws_conv(c) for c in cc.WS_CONV.cases] + [_ws_wgrad(c) for c in cc.WS_WGRAD.cases] + [
    ("conv_transpose3d", _convt_case(), None),
    ("upsample_conv3d", _upconv_case(), r"upconv"),
    ("conv3d_pair", _pair_case(), r"convpair|sepconv|pair"),
    ("norm_act_batch", _norm_case("batch"), None),
    ("norm_act_instance", _norm_case("instance"), None),
    ("norm_act_group", _norm_case("group"), None),
    ("norm_act_batch_bf16", _norm_case("batch", BF), None),
] + [("norm_act_row_%s_%s" % (rid, dt), _norm_row_case(rid, dt), None) for rid in nc.WS_ROWS for dt in nc.BY_ID[rid].dtypes] + [
    ("upsample3d_nearest", _upsample_case("nearest"), None),
    ("upsample3d_trilinear", _upsample_case("trilinear"), None),
    ("softmax_dice_loss", _dice_case(), None),
    ("mask_overlap_counts", _overlap_case(), None),
]


@pytest.mark.parametrize("case", WS_CASES, ids=lambda c: c[0])
def test_workspaces_exact_size_poisoned_and_guarded(case, monkeypatch):
    cid, run, route = case
    ref, names = kernels_launched(run)
    if route is not None:
        _route(names, route, cid)
    for fill in ("a5", "nan"):
        exact = _ExactWorkspaces(fill)
        with monkeypatch.context() as m:
            m.setattr(ops, "_workspace", exact)
            got = run()
            torch.cuda.synchronize()
        assert exact.bufs, "%s: no workspace was requested" % cid
        exact.assert_intact("%s (%s)" % (cid, fill))
        for i, (a, b) in enumerate(zip(got, ref)):
            assert _same_bits(a, b), "%s: result #%d differs from the run with the grow-only workspace (poison %s)" % (cid, i, fill)


# ------------------------------------------------------------------------------------------------ c. pitched destinations


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("co", [4, 8, 24, 40])
@pytest.mark.parametrize("off", [0, 8])
def test_conv_forward_into_a_pitched_slice(co, off, dtype):
    """mri3d_conv3d_fwd with y_ld > co: channels [off, off + co) of a wider buffer; the last quad / octet of co = 4, 24, 40 is
    partly filled, so a vector store past co lands in the neighbouring channels."""
    L = _lib.lib()
    n, ci, sp = 2, 16, (5, 9, 19)
    torch.manual_seed(40 + co + off)
    x = _rand(40 + co + off, (n, ci) + sp, dtype)
    w = torch.randn(co, ci, 3, 3, 3, device="cuda") / np.sqrt(27 * ci)
    b = torch.randn(co, device="cuda")
    dst = SentinelSlice(n, off + co + 8, sp, dtype, off, co)
    g = ops._conv_geom(tuple(x.shape), w.shape, (1, 1, 1), (1, 1, 1), (1, 1, 1), y_ld=dst.channels, dtype=ops._dt(x))
    ws = ops._workspace(L.mri3d_conv3d_workspace_bytes(ctypes.byref(g), _lib.PASS_FWD), x.device)
    _lib.check(L.mri3d_conv3d_fwd(ctypes.byref(g), ops._ptr(x), ops._ptr(w), ops._ptr(b), ops._ptr(dst.slice), ops._ptr(ws), ws.numel(),
                                  ops._stream()), "conv3d_fwd")
    torch.cuda.synchronize()
    dst.assert_outside_intact("conv forward into channels [%d, %d) of %d" % (off, off + co, dst.channels))
    assert not bool(dst.slice_untouched().any()), "slice not completely written"
    vox = sample_voxels(n, *sp, seed=co)
    _ref_close(gather_voxels(dst.slice, vox), conv3d_ref_at(x, _wq(w, dtype), b, 1, 1, 1, vox), dtype, "pitched forward")


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("ci", [4, 8, 24, 40])
@pytest.mark.parametrize("off", [0, 8])
def test_conv_data_gradient_into_a_pitched_slice(ci, off, dtype):
    """mri3d_conv3d_dgrad with x_ld > ci: dx written into channels [off, off + ci) of a wider buffer."""
    L = _lib.lib()
    n, co, sp = 2, 16, (6, 7, 21)
    torch.manual_seed(60 + ci + off)
    dy = _rand(60 + ci + off, (n, co) + sp, dtype)
    w = torch.randn(co, ci, 3, 3, 3, device="cuda") / np.sqrt(27 * co)
    dst = SentinelSlice(n, off + ci + 8, sp, dtype, off, ci)
    g = ops._conv_geom((n, ci) + sp, w.shape, (1, 1, 1), (1, 1, 1), (1, 1, 1), x_ld=dst.channels, y_ld=co, dtype=ops._dt(dy))
    ws = ops._workspace(L.mri3d_conv3d_workspace_bytes(ctypes.byref(g), _lib.PASS_DGRAD), dy.device)
    _lib.check(L.mri3d_conv3d_dgrad(ctypes.byref(g), ops._ptr(dy), ops._ptr(w), None, ops._ptr(dst.slice), ops._ptr(ws), ws.numel(),
                                    ops._stream()), "conv3d_dgrad")
    torch.cuda.synchronize()
    dst.assert_outside_intact("conv data gradient into channels [%d, %d) of %d" % (off, off + ci, dst.channels))
    assert not bool(dst.slice_untouched().any()), "slice not completely written"
    vox = sample_voxels(n, *sp, seed=ci)
    # stride 1, padding 1: dx = conv3d(dy, w^T with the taps mirrored, padding 1)
    wt = w.transpose(0, 1).flip(2, 3, 4)
    _ref_close(gather_voxels(dst.slice, vox), conv3d_ref_at(dy, _wq(wt, dtype), None, 1, 1, 1, vox), dtype, "pitched data gradient")


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", ["nearest", "trilinear"])
def test_upsample_into_a_channel_slice(mode, dtype):
    n, c, sp = 2, 16, (5, 6, 7)
    x = _rand(70, (n, c) + sp, dtype)
    out_sp = tuple(2 * s for s in sp)
    dst = SentinelSlice(n, 16 + c + 8, out_sp, dtype, 16, c)
    ac = False if mode == "trilinear" else None
    y = ops.upsample3d(x, scale_factor=2, mode=mode, align_corners=ac, out=(dst.buf, 16))
    torch.cuda.synchronize()
    assert y.data_ptr() == dst.slice.data_ptr()
    dst.assert_outside_intact("upsample3d(out=) %s" % mode)
    ref = F.interpolate(x.double().cpu(), scale_factor=2, mode=mode, align_corners=ac)
    _ref_close(dst.slice.cpu(), ref, dtype, "upsample3d(out=) %s" % mode)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_norm_act_into_a_channel_slice(dtype):
    n, c, sp = 2, 24, (7, 9, 11)
    torch.manual_seed(71)
    x = _rand(71, (n, c) + sp, dtype)
    gamma, beta = torch.rand(c, device="cuda") + 0.5, torch.randn(c, device="cuda") * 0.1
    dst = SentinelSlice(n, 8 + c + 8, sp, dtype, 8, c)
    ops.norm_act(x, gamma, beta, None, None, None, stats_mode="batch", act="relu", out=(dst.buf, 8))
    torch.cuda.synchronize()
    dst.assert_outside_intact("norm_act(out=)")
    xd = x.double().cpu()
    mean, var = xd.mean((0, 2, 3, 4), keepdim=True), xd.var((0, 2, 3, 4), unbiased=False, keepdim=True)
    ref = torch.relu((xd - mean) / torch.sqrt(var + 1e-5) * gamma.double().cpu().view(1, -1, 1, 1, 1) + beta.double().cpu().view(1, -1, 1, 1, 1))
    got = dst.slice.cpu().double()
    tol = 2e-2 if dtype == BF else 1e-4
    assert (got - ref).abs().max().item() <= tol * ref.abs().max().item(), (got - ref).abs().max().item()


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_decoder_concat_buffer_filled_slice_by_slice(dtype):
    """unet.UNet's shared concat buffer (unet/unet.py:130-135): the encoder's norm_act writes the skip into channels [0, C), the
    pool reads it, the decoder's upsample writes [C, 3C); each producer leaves the other one's channels bit-unchanged, and
    join_channels hands out exactly the buffer."""
    n, c, sp = 2, 8, (8, 10, 12)
    torch.manual_seed(72)
    x = _rand(72, (n, c) + sp, dtype)
    low = _rand(73, (n, 2 * c) + tuple(s // 2 for s in sp), dtype)
    dst = SentinelSlice(n, 3 * c, sp, dtype, 0, c)
    gamma, beta = torch.rand(c, device="cuda") + 0.5, torch.randn(c, device="cuda") * 0.1
    skip = ops.norm_act(x, gamma, beta, None, None, None, stats_mode="instance", act="relu", out=(dst.buf, 0))
    torch.cuda.synchronize()
    dst.assert_outside_intact("skip producer")
    before = dst.g.storage.clone()
    pooled, skip2 = ops.max_pool3d_skip(skip, 2)
    torch.cuda.synchronize()
    assert _same_bits(dst.g.storage, before), "max_pool3d_skip wrote into the concat buffer"
    assert skip2.data_ptr() == skip.data_ptr()
    ref_pool = F.max_pool3d(skip.double().cpu(), 2)
    assert torch.equal(pooled.double().cpu(), ref_pool)
    skip_bits = dst.buf[:, :c].clone()
    up = ops.upsample3d(low, scale_factor=2, mode="nearest", out=(dst.buf, c))
    torch.cuda.synchronize()
    dst.g.assert_guards_intact("upsample producer")
    assert _same_bits(dst.buf[:, :c].contiguous(), skip_bits.contiguous()), "the upsample producer changed the skip channels"
    assert torch.equal(dst.buf[:, c:].double().cpu(), F.interpolate(low.double().cpu(), scale_factor=2, mode="nearest"))
    joined = ops.join_channels(dst.buf, [skip, up])
    assert joined.data_ptr() == dst.buf.data_ptr() and joined.shape == dst.buf.shape
