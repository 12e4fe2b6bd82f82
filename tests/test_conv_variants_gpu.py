"""Every kernel and instantiation of conv_generic.hip and conv_pointwise.hip against the same operation in float64 on the CPU.

The case tables (tests/conv_cases.py: GENERIC_DENSE, GENERIC_PITCHED, TRANSPOSE) cover every route name of the two files per storage
type and pass, which tests/test_conv_routes.py proves on the CPU; each test here asserts its three routes with the real tensors
before it launches.  Per case:

  parity       y, dx, dw, db against F.conv3d / F.conv_transpose3d on .double() tensors and autograd.  fp32: max-norm relative error
               <= util.REL_TOL.  bf16: test_bf16_gpu._close (2 bf16 ulp + 2e-3 of the scale; ulp 0 for the parameter gradients), inputs
               and incoming gradient rounded to bf16 first, weights rounded iff the forward runs on an MFMA kernel (those round their
               weight operand; the kernels of the two files here keep fp32 weights).
  sentinel     x and the incoming gradient are channel slices of wider NDHWC buffers whose other channels hold a sentinel; both
               buffers are bit-identical after the passes, and a kernel that read a neighbouring channel fails parity.
  determinism  the whole forward and backward run twice: y, dx, dw and db are bit-identical (every weight gradient reduces its
               partials in a fixed order)."""
import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc
from mri_epilepsy_diagnosis_amd import ops
from test_bf16_gpu import _close
from util import assert_close, to_ncdhw

pytestmark = pytest.mark.gpu

SENTINEL = -1024.0      # exact in bf16; next to inputs of order one it ruins any sum it leaks into
_TORCH = {"f32": torch.float32, "bf16": torch.bfloat16}
_DTYPES = dict(argnames="dn", argvalues=["f32", "bf16"])
CL3D = torch.channels_last_3d


def _seed(table, case):
    return 1000 * sorted(cc.TABLES).index(table.name) + table.cases.index(case)


def _slice_of_wide_buffer(t, pad, dtype):
    """`t` (N, C, D, H, W) as channels [pad, pad + C) of an NDHWC buffer of pitch C + pad on the device; the rest is the sentinel."""
    n, c = t.shape[:2]
    buf = torch.full((n, c + pad) + tuple(t.shape[2:]), SENTINEL, device="cuda", dtype=dtype).contiguous(memory_format=CL3D)
    buf[:, pad:] = t.cuda().to(dtype)
    return buf, buf[:, pad:]


def _mfma(route):
    return route.split(" ")[0] not in ("generic", "pointwise")


def _compare(dn, got, ref):
    """got / ref: (y, dx, dw, db) with db None where there is no bias."""
    for what, g, r in zip(("y", "dx", "dw", "db"), got, ref):
        if r is None:
            continue
        g = to_ncdhw(g) if g.dim() == 5 and what in ("y", "dx") else g
        if dn == "f32":
            assert_close(g.float().cpu(), r, what=what)
        elif what in ("y", "dx"):
            _close(g, r, what)
        else:
            _close(g, r, what, ulp=0.0, abs_frac=2e-3)


def _assert_deterministic(a, b):
    for what, u, v in zip(("y", "dx", "dw", "db"), a, b):
        if u is not None:
            assert torch.equal(u, v), "%s differs between two runs of the same passes" % what


def _run_geom(table, case, dn):
    n, ci, co, sp, k, s, p, dil, bias, pad_in, pad_out = case
    dtype = _TORCH[dn]
    gen = torch.Generator().manual_seed(_seed(table, case))
    taps = k[0] * k[1] * k[2]
    x = torch.randn(n, ci, *sp, generator=gen)
    w = torch.randn(co, ci, *k, generator=gen) * (1.0 / (taps * ci) ** 0.5)
    b = torch.randn(co, generator=gen) if bias else None
    if dn == "bf16":
        x = x.to(dtype).float()
    oshape = F.conv3d(x[:1, :, :, :, :], w, None, s, p, dil).shape[2:]
    dy = torch.randn(n, co, *oshape, generator=gen)
    if dn == "bf16":
        dy = dy.to(dtype).float()

    xbuf, xs = _slice_of_wide_buffer(x, pad_in, dtype)
    dybuf, dys = _slice_of_wide_buffer(dy, pad_out, dtype)
    xbuf0, dybuf0 = xbuf.clone(), dybuf.clone()
    routes = table.check(case, dn, x=xs, dy=dys)

    def run():
        xg = xs.detach().requires_grad_(True)
        wg, bg = w.cuda().requires_grad_(True), (b.cuda().requires_grad_(True) if bias else None)
        y = ops.conv3d(xg, wg, bg, s, p, dil)
        y.backward(dys)
        return y.detach(), xg.grad, wg.grad, (bg.grad if bias else None)

    got, again = run(), run()
    assert got[0].dtype == dtype and got[1].dtype == dtype and got[2].dtype == torch.float32
    assert torch.equal(xbuf, xbuf0) and torch.equal(dybuf, dybuf0), "a pass wrote into one of its input buffers"
    _assert_deterministic(got, again)

    wref = w.to(dtype).float() if (dn == "bf16" and _mfma(routes["fwd"])) else w
    xr, wr = x.double().requires_grad_(True), wref.double().requires_grad_(True)
    br = b.double().requires_grad_(True) if bias else None
    yr = F.conv3d(xr, wr, br, s, p, dil)
    yr.backward(dy.double())
    _compare(dn, got, (yr.detach(), xr.grad, wr.grad, br.grad if bias else None))


@pytest.mark.parametrize(**_DTYPES)
@pytest.mark.parametrize("case", cc.GENERIC_DENSE.cases, ids=cc.GENERIC_DENSE.ids)
def test_generic_and_pointwise_kernels_dense(case, dn):
    _run_geom(cc.GENERIC_DENSE, case, dn)


@pytest.mark.parametrize(**_DTYPES)
@pytest.mark.parametrize("case", cc.GENERIC_PITCHED.cases, ids=cc.GENERIC_PITCHED.ids)
def test_generic_and_pointwise_kernels_on_pitched_channel_slices(case, dn):
    _run_geom(cc.GENERIC_PITCHED, case, dn)


@pytest.mark.parametrize(**_DTYPES)
@pytest.mark.parametrize("case", cc.TRANSPOSE.cases, ids=cc.TRANSPOSE.ids)
def test_conv_transpose3d_on_every_data_gradient_kernel_with_a_bias(case, dn):
    table = cc.TRANSPOSE
    n, ci, co, sp, k, s, p, op, bias = case
    dtype = _TORCH[dn]
    gen = torch.Generator().manual_seed(_seed(table, case))
    taps = k[0] * k[1] * k[2]
    x = torch.randn(n, ci, *sp, generator=gen)
    w = torch.randn(ci, co, *k, generator=gen) * (1.0 / (taps * ci) ** 0.5)
    b = torch.randn(co, generator=gen) if bias else None
    dy = torch.randn(n, co, *cc.transpose_out(case), generator=gen)
    if dn == "bf16":
        x, dy = x.to(dtype).float(), dy.to(dtype).float()
    xd = x.cuda().to(dtype).contiguous(memory_format=CL3D)
    dyd = dy.cuda().to(dtype).contiguous(memory_format=CL3D)
    routes = table.check(case, dn, x=xd, dy=dyd)

    def run():
        xg = xd.detach().requires_grad_(True)
        wg, bg = w.cuda().requires_grad_(True), (b.cuda().requires_grad_(True) if bias else None)
        y = ops.conv_transpose3d(xg, wg, bg, s, p, op, 1)
        assert tuple(y.shape) == tuple(dy.shape)
        y.backward(dyd)
        return y.detach(), xg.grad, wg.grad, (bg.grad if bias else None)

    got, again = run(), run()
    _assert_deterministic(got, again)
    # the forward is the mirrored convolution's data gradient: its route is the one that decides the weight rounding
    wref = w.to(dtype).float() if (dn == "bf16" and _mfma(routes["fwd"])) else w
    xr, wr = x.double().requires_grad_(True), wref.double().requires_grad_(True)
    br = b.double().requires_grad_(True) if bias else None
    yr = F.conv_transpose3d(xr, wr, br, s, p, op, 1, 1)
    yr.backward(dy.double())
    _compare(dn, got, (yr.detach(), xr.grad, wr.grad, br.grad if bias else None))
