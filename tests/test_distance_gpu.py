"""GPU suite of csrc/distance.hip: the squared distance transform, ball morphology, hole filling and the signed map bit for bit
against tests/distance_ref.py and scipy.ndimage, the boundary loss and its gradient against float64, all outputs inside guard
bands, and DiceBoundaryLoss through routine.run_epoch.

An int32 map is guarded as float32 storage viewed as int32: the sentinel's bits (0x7FC0DEAD) exceed every legal value
(at most MRI3D_EDT_INF = 0x3f000000; INT32_MIN and the signed values are negative)."""
import ctypes

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

import distance_cases as cases
import distance_ref as R
from guard import guarded
from mri_epilepsy_diagnosis_amd import _lib, ops, parallel
from mri_epilepsy_diagnosis_amd.segmentation import distance, labels as label_maps, losses, routine
from mri_epilepsy_diagnosis_amd.unet import UNet
from util import seeded_randn

pytestmark = pytest.mark.gpu

CL = torch.channels_last_3d
F32, BF = torch.float32, torch.bfloat16


def _i32_out(shape):
    g = guarded(shape, torch.float32)
    return g, g.region.view(torch.int32)


def _finish(g, what):
    g.assert_guards_intact(what)
    assert not bool(g.untouched().any()), "%s: elements left unwritten" % what


def _scipy_sq(m, outside_zero):
    """One volume by scipy itself (used where the numpy restatement would walk thousands of candidates per line)."""
    if outside_zero:
        return np.rint(ndi.distance_transform_edt(np.pad(m != 0, 1)) ** 2).astype(np.int32)[1:-1, 1:-1, 1:-1]
    if (m != 0).all():
        return np.full(m.shape, R.EDT_INF, np.int32)
    return np.rint(ndi.distance_transform_edt(m != 0) ** 2).astype(np.int32)


def _want_sq(batch, outside_zero):
    if max(batch.shape[1:]) > 400:
        return np.stack([_scipy_sq(m, outside_zero) for m in batch])
    return R.edt_sq(batch, outside_zero=outside_zero)


@pytest.mark.parametrize("outside_zero", [False, True], ids=["inside_only", "outside_zero"])
@pytest.mark.parametrize("c", cases.EDT_CASES, ids=lambda c: c.name)
def test_squared_edt_is_exact(c, outside_zero):
    for j, name in enumerate(c.patterns):
        # the volumes of a batch hold different patterns: nothing may cross from one to the next
        batch = np.stack([cases.pattern(c.patterns[(j + 3 * i) % len(c.patterns)], c.shape, seed=j + i) for i in range(c.n)])
        g, out = _i32_out(batch.shape)
        got = ops.edt_sq(torch.from_numpy(batch).cuda(), outside_zero=outside_zero, out=out)
        assert got.data_ptr() == out.data_ptr()
        what = "%s %s" % (c.name, name)
        _finish(g, what)
        R.compare_exact(got.cpu().numpy(), _want_sq(batch, outside_zero), what)


def test_shapes_values_and_saturation():
    m = cases.pattern("rand50", (6, 9, 40), 1)
    dev = torch.from_numpy(m).cuda()
    want = R.edt_sq(m[None])[0]
    R.compare_exact(ops.edt_sq(dev).cpu().numpy(), want, "3-D")
    R.compare_exact(ops.edt_sq(dev[0]).cpu().numpy(), R.edt_sq(m[None, :1])[0, 0], "2-D")
    R.compare_exact(ops.edt_sq(dev != 0).cpu().numpy(), want, "bool")
    y = cases.class_map(5, (6, 9, 40), 2, n=1)
    R.compare_exact(ops.edt_sq(torch.from_numpy(y).cuda(), value=3).cpu().numpy(), R.edt_sq(y, value=3), "value")
    ones = torch.ones((2, 3, 4, 5), dtype=torch.uint8, device="cuda")
    ones[1, 1, 2, 3] = 0
    sq = ops.edt_sq(ones)
    assert bool((sq[0] == ops.EDT_INF).all()) and int(sq[1].max()) < 64 and ops.EDT_INF == R.EDT_INF
    assert torch.equal(distance.distance_transform_edt(dev), torch.sqrt(torch.from_numpy(want).float()).cuda())
    with pytest.raises(RuntimeError):
        ops.edt_sq(torch.from_numpy(m))                                    # a CPU tensor: no fallback


def test_full_size_mask_against_scipy_and_twice_the_same_bits():
    shape = (160, 192, 160)
    rng = np.random.default_rng(3)
    g = np.ogrid[:160, :192, :160]
    m = ((g[0] - 80) ** 2 + (g[1] - 96) ** 2 + (g[2] - 80) ** 2 <= 60 ** 2) ^ (rng.random(shape) < 0.001)
    m = m.astype(np.uint8)
    dev = torch.from_numpy(m).cuda()
    gd, out = _i32_out(shape)
    got = ops.edt_sq(dev, out=out)
    _finish(gd, "full size")
    again = ops.edt_sq(dev)
    assert torch.equal(got, again)
    want = ndi.distance_transform_edt(m)
    R.compare_exact(got.cpu().numpy(), np.rint(want ** 2).astype(np.int32), "full size")
    assert np.array_equal(distance.distance_transform_edt(dev).cpu().numpy(), want.astype(np.float32))


MORPH_SHAPES = [(17, 19, 23), (1, 37, 70), (3, 5, 300)]


@pytest.mark.parametrize("radius", [1, 1.5, 2, 3, 6])
@pytest.mark.parametrize("shape", MORPH_SHAPES, ids=str)
def test_morphology_is_scipys(shape, radius):
    ball = R.ball(radius)
    batch = np.stack([cases.pattern(p, shape, 5) for p in ("ball", "rand50", "rand99", "rand01")])
    batch[0] |= cases.pattern("rand01", shape, 6) & 1
    dev = torch.from_numpy(batch).cuda()
    g = guarded(batch.shape, torch.uint8)
    got = {"dilate": distance.dilate(dev, radius, out=g.region).clone()}
    g.assert_guards_intact("dilate")
    got["erode 0"] = distance.erode(dev, radius, out=g.region).clone()
    g.assert_guards_intact("erode")
    got["erode 1"] = distance.erode(dev, radius, outside=1)
    got["opening"] = distance.opening(dev, radius)
    got["closing"] = distance.closing(dev, radius)
    for i, m in enumerate(batch):
        want = {"dilate": ndi.binary_dilation(m, ball), "erode 0": ndi.binary_erosion(m, ball, border_value=0),
                "erode 1": ndi.binary_erosion(m, ball, border_value=1), "opening": ndi.binary_opening(m, ball),
                "closing": ndi.binary_closing(m, ball)}
        for k, w in want.items():
            R.compare_exact(got[k][i].cpu().numpy(), w.astype(np.uint8), "%s r=%s volume %d" % (k, radius, i))
    # one volume alone gives what it gives in the batch
    assert torch.equal(distance.dilate(dev[1], radius), got["dilate"][1])


def test_fill_holes_is_scipys():
    for name, m in cases.hole_masks().items():
        got = distance.fill_holes(torch.from_numpy(m).cuda())
        R.compare_exact(got.cpu().numpy(), ndi.binary_fill_holes(m).astype(np.uint8), name)
    full = torch.ones((3, 4, 5), dtype=torch.uint8, device="cuda")
    assert torch.equal(distance.fill_holes(full), full)


def _signed(y, C, ids, what):
    g, out = _i32_out((y.shape[0], len(ids)) + y.shape[1:])
    got = ops.signed_sqdist(torch.from_numpy(y).cuda(), C, ids, out=out)
    _finish(g, what)
    R.compare_exact(got.cpu().numpy(), R.signed_sqdist(y, C, ids), what)
    return got


@pytest.mark.parametrize("C,ids", cases.LOSS_CLASSES, ids=lambda v: str(v) if isinstance(v, int) else "k%d" % len(v))
def test_signed_map_is_exact(C, ids):
    y = cases.class_map(C, (7, 9, 10), C)
    got = _signed(y, C, ids, "blobs")
    again = ops.signed_sqdist(torch.from_numpy(y).cuda()[:, None], C, ids)       # (n, 1, d, h, w) is accepted
    assert torch.equal(got, again)


def test_signed_map_special_volumes():
    ids_of = {2: (1,), 3: (1, 2), 9: (1, 2, 5)}
    for name, (y, C) in cases.signed_map_cases().items():
        got = _signed(y, C, ids_of[C], name)
        if name == "all_ignored":
            assert bool((got == ops.INT32_MIN).all())
        if name == "absent_from_one_volume":
            assert bool((got[1, 0] == 0).all()) and bool((got[0, 0] != 0).any())
        if name == "filling_a_volume":
            assert bool((got[0] == 0).all())


# ------------------------------------------------------------------------------------------------ loss and gradient
def _layouts(z, dtype):
    """name -> a device leaf tensor holding z (n, C, d, h, w) in `dtype`: dense NDHWC, and channel slices of a wider buffer."""
    n, C = z.shape[:2]
    zt = torch.from_numpy(z).to(dtype)
    out = {"dense": zt.cuda().contiguous(memory_format=CL)}
    for name, off in (("padded", 0), ("padded_offset", 1)):
        buf = torch.zeros((n, C + 4) + z.shape[2:], dtype=dtype, device="cuda").contiguous(memory_format=CL)
        buf[:, off:off + C] = zt.cuda()
        out[name] = buf.narrow(1, off, C)
    return {k: v.detach().requires_grad_(True) for k, v in out.items()}


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("spatial", cases.LOSS_SPATIAL, ids=str)
@pytest.mark.parametrize("C,ids", cases.LOSS_CLASSES, ids=lambda v: str(v) if isinstance(v, int) else "k%d" % len(v))
def test_loss_and_gradient_against_float64(C, ids, spatial, dtype):
    """Loss: |error| <= 8 max(e32, 2^-23 A), A the float64 mean of |p phi|; gradient: 8 max(e32, 2^-23 max|g64|) per element plus
    2^-8 |g64| for bf16 storage; e32 is torch's CPU float32 evaluation against float64 on the same (rounded) logits."""
    for scale in (1.0, 32.0):
        z, y = cases.loss_inputs(C, spatial, scale, seed=C)
        y[0, 0, 0, :2] = 255                                                  # two ignored voxels
        z = torch.from_numpy(z).to(dtype).double().numpy()                    # the reference sees the stored logits
        s = R.signed_sqdist(y, C, ids)
        l64, g64 = R.boundary_loss(z, s, ids)
        l32, g32 = R.torch_loss(z, s, ids, torch.float32)
        e32l, e32g, a = abs(l32 - l64), float(np.abs(g32 - g64).max()), R.mean_abs_term(z, s, ids)
        smap = ops.signed_sqdist(torch.from_numpy(y).cuda(), C, ids)
        R.compare_exact(smap.cpu().numpy(), s, "map")
        for name, x in _layouts(z, dtype).items():
            what = "C=%d K=%d %s %s scale %g %s" % (C, len(ids), spatial, dtype, scale, name)
            loss = ops.softmax_boundary_loss(x, smap, ids)
            loss.backward()
            assert loss.dtype == F32 and loss.shape == () and x.grad.dtype == dtype and x.grad.shape == x.shape
            R.compare_loss(loss.item(), l64, e32l, a, what)
            R.compare_grad(x.grad.float().cpu().numpy(), g64, e32g, dtype == BF, what)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("C,ids", [(3, (1, 2)), (32, tuple(range(32)))], ids=["c3", "c32"])
def test_pitched_gradient_stays_inside_guard_bands(C, ids, dtype):
    """The raw entry points with a pitched gradient buffer between guards: the padding channels keep their sentinel."""
    n, spatial, ld = 2, (5, 6, 7), C + 4
    vox = int(np.prod(spatial))
    z, y = cases.loss_inputs(C, spatial, 1.0, seed=3)
    smap = ops.signed_sqdist(torch.from_numpy(y).cuda(), C, ids)
    gx, gd = guarded((n, vox, ld), dtype), guarded((n, vox, ld), dtype)
    gx.region[:, :, :C] = torch.from_numpy(z).to(dtype).cuda().permute(0, 2, 3, 4, 1).reshape(n, vox, C)
    L = _lib.lib()
    g = _lib.BoundaryGeom(n, vox, C, ld, _lib.BF16 if dtype == BF else _lib.F32, len(ids), (ctypes.c_int32 * 32)(*ids))
    loss, stats = torch.empty((), device="cuda"), torch.empty(4, device="cuda")
    one = torch.ones((), device="cuda")
    ws = torch.empty(L.mri3d_softmax_boundary_workspace_bytes(), dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.mri3d_softmax_boundary_fwd(ctypes.byref(g), p(gx.region), p(smap), p(loss), p(stats), p(ws), ws.numel(), stream) == 0
    assert L.mri3d_softmax_boundary_bwd(ctypes.byref(g), p(gx.region), p(smap), p(stats), p(one), p(gd.region), ld, stream) == 0
    torch.cuda.synchronize()
    gd.assert_guards_intact("pitched gradient")
    untouched = gd.untouched()
    assert bool(untouched[:, :, C:].all()) and not bool(untouched[:, :, :C].any())
    x = torch.from_numpy(z).to(dtype).cuda().contiguous(memory_format=CL).requires_grad_(True)
    ref = ops.softmax_boundary_loss(x, smap, ids)
    ref.backward()
    assert loss.item() == ref.item()
    assert torch.equal(gd.region[:, :, :C], x.grad.permute(0, 2, 3, 4, 1).reshape(n, vox, C))


def test_all_voxels_ignored_and_same_bits_run_to_run():
    C, ids = 3, (0, 2)
    z, y = cases.loss_inputs(C, (8, 16, 33), 1.0, seed=9)
    x = torch.from_numpy(z).float().cuda().contiguous(memory_format=CL).requires_grad_(True)
    none = ops.signed_sqdist(torch.full(y.shape, 255, dtype=torch.uint8, device="cuda"), C, ids)
    loss = ops.softmax_boundary_loss(x, none, ids)
    loss.backward()
    assert loss.item() == 0.0 and not bool(x.grad.any())
    runs = []
    for _ in range(2):
        x.grad = None
        smap = ops.signed_sqdist(torch.from_numpy(y).cuda(), C, ids)
        loss = ops.softmax_boundary_loss(x, smap, ids)
        loss.backward()
        runs.append((smap.clone(), loss.clone(), x.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_python_refusals():
    x = torch.zeros((1, 3, 4, 4, 4), device="cuda").contiguous(memory_format=CL)
    y = torch.zeros((1, 4, 4, 4), dtype=torch.uint8, device="cuda")
    smap = ops.signed_sqdist(y, 3, (1,))
    with pytest.raises(ValueError):
        ops.signed_sqdist(y, 3, (3,))
    with pytest.raises(ValueError):
        ops.softmax_boundary_loss(x, smap, (1, 1))
    with pytest.raises(RuntimeError):
        ops.softmax_boundary_loss(x, smap, (1, 2))                            # one plane, two ids
    with pytest.raises(RuntimeError):
        ops.softmax_boundary_loss(x, smap.float(), (1,))
    with pytest.raises(ValueError):
        distance.dilate(y, -1)
    with pytest.raises(RuntimeError):
        losses.BoundaryLoss(ids=(1,), classes=2)(x, y)                        # built for 2 classes, 3 in the logits


# ------------------------------------------------------------------------------------------------ through the loop
IDS = [17, 53]        # -> classes 1, 2; background 0


def _batches(count):
    out = []
    for i in range(count):
        g = torch.Generator().manual_seed(80 + i)
        pick = torch.kron(torch.randint(0, 4, (1, 1, 4, 4, 4), generator=g), torch.ones((1, 1, 4, 4, 4), dtype=torch.int64))
        raw = torch.tensor(IDS + [4, 3000])[pick].to(torch.int16)
        out.append({routine.MRI: {routine.DATA: seeded_randn(70 + i, (1, 1, 16, 16, 16))}, routine.LABEL: {routine.DATA: raw}})
    return out


def _train(batches, capture, make_loss):
    lm = label_maps.LabelMap.from_ids(IDS)
    torch.manual_seed(0)
    model = UNet(in_channels=1, out_classes=3, dimensions=3, num_encoding_blocks=3, out_channels_first_layer=8, normalization="batch",
                 upsampling_type="linear", padding=True, activation="PReLU").cuda()
    cache = parallel.StepCache.of(model)
    cache.disabled = not capture
    opt = torch.optim.AdamW(model.parameters())
    got = []
    for b in batches:
        got += routine.run_epoch(1, routine.Action.TRAIN, [b], model, opt, loss_fn=make_loss(),
                                 prepare=lambda batch, dev: label_maps.prepare_batch_index(batch, dev, lm)).tolist()
    return got, cache


def test_dice_boundary_training_is_captured_once_and_equals_the_eager_run():
    batches = _batches(2)
    make = lambda: losses.DiceBoundaryLoss(1.0, 0.5, ids=(1, 2), classes=3)  # noqa: E731  (a new, equal object per epoch)
    eager, ecache = _train(batches, False, make)
    captured, cache = _train(batches, True, make)
    print("DiceBoundaryLoss trajectory", captured, "eager", eager)
    assert (ecache.captures, ecache.eager_runs) == (0, 2)
    assert (cache.captures, cache.eager_runs, cache.replays) == (1, 0, 2) and not cache.disabled
    assert captured == eager and all(np.isfinite(captured))
    assert losses.DiceBoundaryLoss(1.0, 0.5, (1, 2), 3) == make() and hash(losses.DiceBoundaryLoss(1.0, 0.5, (1, 2), 3)) == hash(make())
    assert losses.DiceBoundaryLoss(1.0, 0.25, (1, 2), 3) != make()
