"""Seeded random-geometry sweep of the 3x3x3 MFMA conv kernels (fp32 and bf16 storage): ragged spatial sizes around the tile
edges (4x8x16 forward tile, 2x6x16 / 2x6x32 weight-gradient tiles), every channel count the dispatcher routes to an MFMA
kernel, pitched (channel-slice) inputs and outputs — against torch's CPU conv on the same (rounded) inputs.

The case tables live in tests/conv_cases.py, each with the kernel route it is there for; tests/test_conv_routes.py checks those
routes on the CPU, and every test here asserts them again with its real pointers before it launches."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc
from mri_epilepsy_diagnosis_amd import ops

pytestmark = pytest.mark.gpu


def _params(table):
    """parametrize arguments of a table of tests/conv_cases.py (the comments on what each table is there for are next to it)."""
    return dict(argnames="case", argvalues=table.cases, ids=table.ids)


_BOTH = dict(argnames="dtype", argvalues=[torch.float32, torch.bfloat16], ids=["f32", "bf16"])


@pytest.mark.parametrize(**_BOTH)
@pytest.mark.parametrize(**_params(cc.RANDOM))
def test_conv3x3x3_random_geometry(case, dtype):
    _run_conv_case(case, dtype, cc.RANDOM)


@pytest.mark.parametrize(**_BOTH)
@pytest.mark.parametrize(**_params(cc.MISALIGNED))
def test_conv3x3x3_misaligned_channel_slices_fall_back_to_generic_kernels(case, dtype):
    _run_conv_case(case, dtype, cc.MISALIGNED)


@pytest.mark.parametrize(**_params(cc.TILED_F32))
def test_conv3x3x3_ragged_tiles_with_large_batch_stay_on_the_tiled_kernel(case):
    _run_conv_case(case, torch.float32, cc.TILED_F32)


@pytest.mark.parametrize(**_params(cc.DIRECT_F32_BATCH))
def test_conv3x3x3_ragged_volumes_under_512_work_units_take_the_lds_free_kernel(case):
    _run_conv_case(case, torch.float32, cc.DIRECT_F32_BATCH)


@pytest.mark.parametrize(**_params(cc.SMALL))
def test_conv3x3x3_small_volumes(case):
    _run_conv_case(case, torch.float32, cc.SMALL)


@pytest.mark.parametrize(**_params(cc.DIRECT_WIDE))
def test_conv3x3x3_lds_free_kernel_with_two_and_four_n_tiles_per_wave(case):
    _run_conv_case(case, torch.float32, cc.DIRECT_WIDE)


@pytest.mark.parametrize(**_BOTH)
@pytest.mark.parametrize(**_params(cc.LARGE_BATCH))
def test_conv3x3x3_many_small_volumes(case, dtype):
    _run_conv_case(case, dtype, cc.LARGE_BATCH)


@pytest.mark.parametrize(**_params(cc.MARCH_WGRAD))
def test_bf16_weight_gradient_marching_along_d(case):
    _run_conv_case(case, torch.bfloat16, cc.MARCH_WGRAD)


@pytest.mark.parametrize(**_BOTH)
@pytest.mark.parametrize(**_params(cc.N8))
def test_conv3x3x3_eight_output_channels(case, dtype):
    _run_conv_case(case, dtype, cc.N8)


@pytest.mark.parametrize(**_BOTH)
@pytest.mark.parametrize(**_params(cc.N8_TILED))
def test_conv3x3x3_eight_output_channels_on_the_row_paired_tiled_kernel(case, dtype):
    _run_conv_case(case, dtype, cc.N8_TILED)


@pytest.mark.parametrize(**_BOTH)
@pytest.mark.parametrize(**_params(cc.STRIDED))
def test_conv3x3x3_stride2(case, dtype):
    _run_conv_case(case, dtype, cc.STRIDED)


@pytest.mark.parametrize(**_BOTH)
@pytest.mark.parametrize(**_params(cc.STRIDED_WIDE))
def test_conv3x3x3_stride2_wave_per_tile_and_wide_n_blocks(case, dtype):
    _run_conv_case(case, dtype, cc.STRIDED_WIDE)


@pytest.mark.parametrize(**_params(cc.STRIDE3))
def test_conv3x3x3_stride3(case):
    _run_conv_case(case, torch.float32, cc.STRIDE3)


@pytest.mark.parametrize(**_params(cc.BF16_WGRAD_QUADS))
def test_bf16_weight_gradient_with_channel_counts_the_bf16_kernels_cannot_take(case):
    _run_conv_case(case, torch.bfloat16, cc.BF16_WGRAD_QUADS)


@pytest.mark.parametrize(**_params(cc.MARCH_BF16))
def test_bf16_marching_kernel_where_the_dispatcher_chooses_it(case):
    _run_conv_case(case, torch.bfloat16, cc.MARCH_BF16)


@pytest.mark.parametrize(**_params(cc.MARCH_BF16_NOBIAS))
def test_bf16_marching_kernel_by_choice_without_a_bias(case):
    _run_conv_case(case, torch.bfloat16, cc.MARCH_BF16_NOBIAS)


@pytest.mark.parametrize(**_BOTH)
@pytest.mark.parametrize(**_params(cc.WGRAD_NOBIAS))
def test_weight_gradient_kernels_without_a_bias(case, dtype):
    _run_conv_case(case, dtype, cc.WGRAD_NOBIAS)


def _dtype_id(dtype):
    return "f32" if dtype == torch.float32 else "bf16"


def _run_conv_case(case, dtype, table):
    """One case of a "slice" table against torch's CPU conv on the same (rounded) inputs; the routes the table declares are asserted
    with the real pointers before anything is launched."""
    nb, ci, co, d, h, w, pad_in, pad_out, seed = case
    stride = table.stride
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(nb, ci, d, h, w, generator=g)
    wt = torch.randn(co, ci, 3, 3, 3, generator=g) * (1.0 / np.sqrt(27 * ci))
    b = torch.randn(co, generator=g)
    if not table.bias:
        b = None
    do, ho, wo = [(e - 1) // stride + 1 for e in (d, h, w)]     # k 3, pad 1
    dy = torch.randn(nb, co, do, ho, wo, generator=g)
    if dtype == torch.bfloat16:
        x, dy = x.to(dtype).float(), dy.to(dtype).float()
    # input as a channel slice of a wider NDHWC buffer (voxel pitch ci + pad_in), as the decoder's concat buffers are
    xbuf = torch.zeros(nb, ci + pad_in, d, h, w, device="cuda", dtype=dtype).contiguous(memory_format=torch.channels_last_3d)
    xbuf[:, pad_in:] = x.cuda().to(dtype)
    xg = xbuf[:, pad_in:].detach().requires_grad_(True)
    wg, bg = wt.cuda().requires_grad_(True), (b.cuda().requires_grad_(True) if b is not None else None)
    dybuf = torch.zeros(nb, co + pad_out, do, ho, wo, device="cuda", dtype=dtype).contiguous(memory_format=torch.channels_last_3d)
    dybuf[:, :co] = dy.cuda().to(dtype)
    table.check(case, _dtype_id(dtype), x=xg, dy=dybuf[:, :co])
    yg = ops.conv3d(xg, wg, bg, stride=stride, padding=1)
    yg.backward(dybuf[:, :co])

    def ref(wref):
        xr = x.clone().requires_grad_(True)
        wr, br = wref.clone().requires_grad_(True), (b.clone().requires_grad_(True) if b is not None else None)
        yr = F.conv3d(xr, wr, br, stride=stride, padding=1)
        yr.backward(dy)
        return yr.detach(), xr.grad, wr.grad, (br.grad if b is not None else None)

    if dtype == torch.float32:
        yr, dxr, dwr, dbr = ref(wt)
        tol_act = tol_par = 2e-5
    else:
        # forward / data-gradient round the weights to bf16 for the MFMA operands; the weight gradient does not involve them
        yr, dxr, _, _ = ref(wt.to(dtype).float())
        _, _, dwr, dbr = ref(wt)
        tol_act, tol_par = 1.2e-2, 2e-3

    def close(a, r, tol, what):
        a, r = a.detach().float().cpu(), r.float()
        err = (a - r).abs().max().item()
        assert err <= tol * (r.abs().max().item() + 1e-6), "%s: %.3e vs scale %.3e" % (what, err, r.abs().max().item())

    close(yg, yr, tol_act, "y")
    close(xg.grad, dxr, tol_act, "dx")
    close(wg.grad, dwr, tol_par, "dw")
    if b is not None:
        close(bg.grad, dbr, tol_par, "db")


def _sum_bounds(tol, amax, count):
    """Bounds on |sum a - sum r| and |sum a^2 - sum r^2| over `count` values that each obey |a - r| <= tol * amax, |r| <= amax."""
    return tol * amax * count, tol * amax * (2.0 + tol) * amax * count


@pytest.mark.parametrize(**_BOTH)
@pytest.mark.parametrize(**_params(cc.STATS_ORACLE))
def test_conv3x3x3_fused_statistics_against_the_cpu_reference(case, dtype):
    """conv3d(bn_stats=True): y AND the per-channel statistics partials of the epilogue (sum a, sum a^2 of a = y - bias, float64 per
    workgroup) against torch's CPU conv on the same (rounded) inputs — the tiled kernel's STATS instantiations and the marching
    kernel's, which the other statistics tests only compare with a second device pass.  y: the tolerances of `_run_conv_case`.
    Statistics: they are sums of the fp32 accumulators BEFORE the result is rounded for storage, and a bf16 product is exact in
    fp32, so in both storage types every accumulator obeys the fp32 bound of 2e-5 of the reference's max-norm; the sums over the
    N x D x H x W voxels of a channel are then within `_sum_bounds` of the reference's float64 sums."""
    nb, ci, co, d, h, w, has_bias = case
    g = torch.Generator().manual_seed(ci * 1000 + co * 10 + d)
    x = torch.randn(nb, ci, d, h, w, generator=g) * 1.5 + 0.3
    wt = torch.randn(co, ci, 3, 3, 3, generator=g) * (1.0 / np.sqrt(27 * ci))
    b = torch.randn(co, generator=g) if has_bias else None
    if dtype == torch.bfloat16:
        x = x.to(dtype).float()
    xg = x.cuda().to(dtype).contiguous(memory_format=torch.channels_last_3d)
    cc.STATS_ORACLE.check(case, _dtype_id(dtype), x=xg)
    yg = ops.conv3d(xg, wt.cuda(), b.cuda() if has_bias else None, padding=1, bn_stats=True)
    part, blocks, _ = yg._mri3d_bn_stats
    sums = part.view(blocks, co, 2).sum(0).cpu()                       # (co, 2) float64
    wref = wt if dtype == torch.float32 else wt.to(dtype).float()      # the MFMA operands are the weights rounded to bf16
    ar = F.conv3d(x, wref, None, padding=1).double()                    # a = y - bias
    amax = ar.abs().max().item()
    yr = ar + (b.double().view(1, -1, 1, 1, 1) if has_bias else 0.0)
    tol_act = 2e-5 if dtype == torch.float32 else 1.2e-2
    err = (yg.double().cpu() - yr).abs().max().item()
    assert err <= tol_act * (yr.abs().max().item() + 1e-6), "y: %.3e vs scale %.3e" % (err, yr.abs().max().item())
    b1, b2 = _sum_bounds(2e-5, amax, nb * d * h * w)
    e1 = (sums[:, 0] - ar.sum((0, 2, 3, 4))).abs().max().item()
    e2 = (sums[:, 1] - (ar * ar).sum((0, 2, 3, 4))).abs().max().item()
    print("statistics: |d sum a| %.3e (bound %.3e), |d sum a^2| %.3e (bound %.3e)" % (e1, b1, e2, b2))
    assert e1 <= b1 and e2 <= b2, "statistics sums off by %.3e (bound %.3e) / %.3e (bound %.3e)" % (e1, b1, e2, b2)


@pytest.mark.parametrize(**_BOTH)
@pytest.mark.parametrize(**_params(cc.FIRST))
def test_first_layer_conv_one_input_channel(case, dtype):
    """Conv3d(1, 8|16, 3, padding=1): the direct first-layer kernels (conv_cin1_{fwd,wgrad}_kernel), ragged tiles, outputs
    written into / gradients read from a pitched channel slice."""
    nb, co, d, h, w, bias, pad_out = case
    g = torch.Generator().manual_seed(co * 1000 + d * 100 + h * 10 + w)
    x = torch.randn(nb, 1, d, h, w, generator=g)
    wt = torch.randn(co, 1, 3, 3, 3, generator=g) * 0.2
    b = torch.randn(co, generator=g) if bias else None
    dy = torch.randn(nb, co, d, h, w, generator=g)
    if dtype == torch.bfloat16:
        x, dy = x.to(dtype).float(), dy.to(dtype).float()
    xg = x.cuda().to(dtype).requires_grad_(True)
    wg = wt.cuda().requires_grad_(True)
    bg = b.cuda().requires_grad_(True) if bias else None
    dybuf = torch.zeros(nb, co + pad_out, d, h, w, device="cuda", dtype=dtype).contiguous(memory_format=torch.channels_last_3d)
    dybuf[:, pad_out:] = dy.cuda().to(dtype)
    cc.FIRST.check(case, _dtype_id(dtype), x=xg, dy=dybuf[:, pad_out:])
    yg = ops.conv3d(xg, wg, bg, padding=1)
    yg.backward(dybuf[:, pad_out:])
    x64, w64 = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True) if bias else None
    r = F.conv3d(x64, w64, b64, padding=1)
    r.backward(dy.double())
    tol_act = 2e-5 if dtype == torch.float32 else 1.2e-2       # bf16: y / dx are rounded to bf16 on store
    tol_par = 2e-5 if dtype == torch.float32 else 2e-5         # parameter gradients accumulate in fp32 from exact inputs

    def close(a, ref, tol, what):
        err = (a.detach().double().cpu() - ref).abs().max().item()
        assert err <= tol * (ref.abs().max().item() + 1e-6), "%s: %.3e vs scale %.3e" % (what, err, ref.abs().max().item())

    close(yg, r.detach(), tol_act, "y")
    close(xg.grad, x64.grad, tol_act, "dx")
    close(wg.grad, w64.grad, tol_par, "dw")
    if bias:
        close(bg.grad, b64.grad, tol_par, "db")


@pytest.mark.parametrize(**_params(cc.ONE_OUT))
def test_single_output_channel_convs(case):
    """The autoencoder's single-channel tail (AE_model.py:110-160): few-tap convs ending in one channel (co1 weight-gradient
    kernel) and the 1 -> 1 3x3x3 `vox` stencil (forward, data gradient, weight gradient)."""
    nb, ci, k, pad, stride, shape, bias = case
    g = torch.Generator().manual_seed(ci * 100 + sum(shape))
    x = torch.randn((nb, ci) + shape, generator=g)
    wt = torch.randn((1, ci) + k, generator=g) * 0.3
    b = torch.randn(1, generator=g) if bias else None
    xg = x.cuda().contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)
    wg = wt.cuda().requires_grad_(True)
    bg = b.cuda().requires_grad_(True) if bias else None
    cc.ONE_OUT.check(case, "f32", x=xg)
    yg = ops.conv3d(xg, wg, bg, stride=stride, padding=pad)
    x64, w64 = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True) if bias else None
    r = F.conv3d(x64, w64, b64, stride=stride, padding=pad)
    dy = torch.randn(r.shape, generator=g)
    yg.backward(dy.cuda())
    r.backward(dy.double())

    def close(a, ref, what):
        err = (a.detach().double().cpu() - ref).abs().max().item()
        assert err <= 2e-5 * (ref.abs().max().item() + 1e-6), "%s: %.3e vs scale %.3e" % (what, err, ref.abs().max().item())

    close(yg, r.detach(), "y")
    close(xg.grad, x64.grad, "dx")
    close(wg.grad, w64.grad, "dw")
    if bias:
        close(bg.grad, b64.grad, "db")


def test_conv_tensors_with_more_than_2_31_elements():
    """288 GB of HBM invite batches whose activation tensors exceed 2^31 ELEMENTS (12 x 48 x 160x192x160 = 2.83e9, 11.3 GB in fp32):
    every voxel index in the kernels must be 64-bit (or relative to a per-item origin).  Size-independent property: the kernels are
    deterministic per output voxel, so the last volume of the big batch must equal — bit for bit — the same volume convolved alone
    (forward and data gradient), and the weight gradient of the batch must equal the sum of the per-volume weight gradients."""
    nb, ci, co, shape = 12, 48, 16, (160, 192, 160)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.empty((nb, ci) + shape, device="cuda", memory_format=torch.channels_last_3d)
    assert x.numel() > 2 ** 31
    for i in range(nb):                       # generated volume by volume (a single randn of 11 GB is its own stress test)
        x[i].copy_(torch.randn((ci,) + shape, device="cuda", generator=g).unsqueeze(0).contiguous(memory_format=torch.channels_last_3d)[0])
    wt = (torch.randn(co, ci, 3, 3, 3, device="cuda", generator=g) / np.sqrt(27 * ci))
    b = torch.randn(co, device="cuda", generator=g)
    dy = torch.randn((nb, co) + shape, device="cuda", generator=g).contiguous(memory_format=torch.channels_last_3d)

    def run(xs, dys):
        xs = xs.detach().requires_grad_(True)
        w, bb = wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
        y = ops.conv3d(xs, w, bb, padding=1)
        y.backward(dys)
        return y.detach(), xs.grad, w.grad, bb.grad

    y_all, dx_all, dw_all, db_all = run(x, dy)
    dw_sum, db_sum = torch.zeros_like(dw_all, dtype=torch.float64), torch.zeros_like(db_all, dtype=torch.float64)
    for i in (0, nb // 2, nb - 1):
        y_i, dx_i, _, _ = run(x[i:i + 1], dy[i:i + 1])
        assert torch.equal(y_all[i:i + 1], y_i), "forward of volume %d differs inside the big batch" % i
        assert torch.equal(dx_all[i:i + 1], dx_i), "data gradient of volume %d differs inside the big batch" % i
    del y_all, dx_all
    for i in range(nb):
        _, _, dw_i, db_i = run(x[i:i + 1], dy[i:i + 1])
        dw_sum += dw_i.double()
        db_sum += db_i.double()
    assert torch.allclose(dw_all.double(), dw_sum, rtol=2e-5, atol=2e-5 * float(dw_sum.abs().max()))
    assert torch.allclose(db_all.double(), db_sum, rtol=2e-5, atol=2e-5 * float(db_sum.abs().max()))


def test_streaming_ops_on_tensors_with_more_than_2_31_elements():
    """Same property for the per-sample streaming operators (InstanceNorm + LeakyReLU, MaxPool3d, trilinear x2 on the pooled
    tensor) on a 2.83e9-element activation tensor: volume i of the batch result equals the operator on volume i alone, forward
    and backward, bit for bit."""
    nb, c, shape = 12, 48, (160, 192, 160)
    g = torch.Generator(device="cuda").manual_seed(6)
    x = torch.empty((nb, c) + shape, device="cuda", memory_format=torch.channels_last_3d)
    for i in range(nb):
        x[i].copy_(torch.randn((c,) + shape, device="cuda", generator=g).unsqueeze(0).contiguous(memory_format=torch.channels_last_3d)[0])
    assert x.numel() > 2 ** 31

    def run(xs):
        xs = xs.detach().requires_grad_(True)
        z = ops.norm_act(xs, None, None, None, None, None, "instance", 0.1, 1e-5, "leaky_relu", 0.01)
        p = ops.max_pool3d(z, 2)
        u = ops.upsample3d(p, scale_factor=2, mode="trilinear", align_corners=False)
        (u * u).sum().backward()
        return z.detach(), p.detach(), u.detach(), xs.grad

    big = run(x)
    for i in (0, nb - 1):
        one = run(x[i:i + 1])
        for name, a, r in zip(("norm_act", "max_pool", "upsample", "dx"), big, one):
            assert torch.equal(a[i:i + 1], r), "%s of volume %d differs inside the big batch" % (name, i)
