"""The first layer's activation folded into its convolution kernels (ops.conv3d_act, mri3d_conv_cin1_act_*).

Bars.  The two kernels keep the FMA chains and every summation order of the four launches they replace (ops.conv3d +
ops.norm_act without statistics), so z, a, dW and db are BIT-EQUAL to theirs, and within REL_TOL of a float64 CPU evaluation —
the bar of the existing cin1 and norm_act parity cases.  dalpha is the same float64 sum of exact products over another partition
of the voxels, rounded to fp32 per channel at the end: held to the same bit-equality.  With sixteen output channels the backward
is not offered (the layer's plain weight gradient is an MFMA kernel): the operator then runs the two backward launches itself."""
import copy
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from guard import SentinelSlice, guarded, kernels_launched
from util import REL_TOL, rel_err, to_ncdhw

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL3D = torch.channels_last_3d
F32 = torch.float32
SLOPE = 0.01

# N, (D, H, W): exactly one tile of Co = 8 (4 x 8 x 32); one voxel over the tile in every dimension; smaller than a tile; several
# tiles with ragged ends along H and W
SHAPES = [(2, (4, 8, 32)), (2, (5, 9, 33)), (2, (3, 3, 3)), (1, (9, 17, 70))]
# activation, alpha: one slope > 0, = 0, < 0, one per channel (both signs)
ACTS = [("prelu", "pos"), ("prelu", "zero"), ("prelu", "neg"), ("prelu", "each"), ("relu", None), ("leaky_relu", None)]
CASES = [(s, co, a) for s in SHAPES for co in (8, 16) for a in ACTS]
IDS = ["n%d_%s_co%d_%s%s" % (s[0], "x".join(map(str, s[1])), co, a[0], "" if a[1] is None else "_" + a[1]) for s, co, a in CASES]


def _dev(t):
    return t.to(DEV).contiguous(memory_format=CL3D) if t.dim() == 5 else t.to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _alpha(kind, co, g):
    if kind is None:
        return None
    if kind == "each":
        a = 0.25 + 0.1 * torch.rand(co, generator=g)
        a[::2] = -a[::2]
        return a
    return torch.full((1,), {"pos": 0.25, "zero": 0.0, "neg": -0.3}[kind])


@functools.lru_cache(maxsize=None)
def _inputs(i):
    (n, sp), co, (act, al) = CASES[i]
    g = torch.Generator().manual_seed(4000 + i)
    return {"x": torch.randn(n, 1, *sp, generator=g), "w": 0.3 * torch.randn(co, 1, 3, 3, 3, generator=g),
            "b": 0.2 * torch.randn(co, generator=g), "alpha": _alpha(al, co, g), "da": torch.randn(n, co, *sp, generator=g)}


def _reference(p, act):
    """float64 CPU: z, a and the gradients of sum(a * da)."""
    leaf = {k: (v.double().requires_grad_(True) if v is not None and k in ("w", "b", "alpha") else v) for k, v in p.items()}
    z = F.conv3d(p["x"].double(), leaf["w"], leaf["b"], padding=1)
    if act == "prelu":
        a_ = leaf["alpha"]
        a = torch.where(z > 0, z, z * (a_[None, :, None, None, None] if a_.numel() > 1 else a_))
    elif act == "relu":
        a = torch.relu(z)
    else:
        a = torch.where(z > 0, z, z * SLOPE)
    (a * p["da"].double()).sum().backward()
    return {"z": z.detach(), "a": a.detach(), "dw": leaf["w"].grad, "db": leaf["b"].grad if leaf["b"] is not None else None,
            "dalpha": leaf["alpha"].grad if leaf["alpha"] is not None else None}


def _run(p, act, fused):
    """One forward + backward on the device: the fused operator, or ops.conv3d + ops.norm_act without statistics."""
    from mri_epilepsy_diagnosis_amd import ops
    t = {k: (_dev(v) if v is not None else None) for k, v in p.items()}
    for k in ("w", "b", "alpha"):
        if t[k] is not None:
            t[k] = t[k].detach().requires_grad_(True)
    co = t["w"].shape[0]
    if fused:
        assert ops.conv3d_act_supported(t["x"], t["w"], act, t["alpha"]), "the predicate declined a listed case"
        z = torch.empty_like(t["da"])
        fn = lambda: ops.conv3d_act(t["x"], t["w"], t["b"], t["alpha"], act, SLOPE, out=(z, torch.empty_like(t["da"])))
    else:
        def fn():
            fn.z = ops.conv3d(t["x"], t["w"], t["b"], 1, 1, 1)
            return ops.norm_act(fn.z, None, None, t["alpha"], None, None, "none", 0.1, 0.0, act, SLOPE)
    a, names = kernels_launched(fn)
    assert any("conv_cin1_act_fwd_kernel" in k for k in names) == fused, names
    assert any("norm_act_fwd_kernel" in k or "conv_cin1_fwd_kernel" in k for k in names) != fused, names
    _, names = kernels_launched(lambda: a.backward(t["da"]))
    assert any("conv_cin1_act_bwd_kernel" in k for k in names) == (fused and co == 8), names
    if fused and co == 8:
        assert not any(key in k for k in names for key in ("norm_act_bwd", "conv_cin1_wgrad_kernel", "conv_mfma_wgrad")), names
    res = {"z": to_ncdhw(z if fused else fn.z), "a": to_ncdhw(a), "dw": t["w"].grad.detach().cpu(),
           "db": t["b"].grad.detach().cpu() if t["b"] is not None else None,
           "dalpha": t["alpha"].grad.detach().cpu() if t["alpha"] is not None else None}
    return res


def _compare(fu, un, ref):
    for k in ("z", "a", "dw", "db", "dalpha"):
        assert (fu[k] is None) == (un[k] is None) == (ref[k] is None), k
        if ref[k] is None:
            continue
        ef, eu = rel_err(fu[k], ref[k]), rel_err(un[k], ref[k])
        print("%-7s fused %.3e  four launches %.3e  tolerance %.3e" % (k, ef, eu, REL_TOL))
        assert torch.equal(_bits(fu[k]), _bits(un[k])), "%s moved: max |diff| %.3e" % (k, (fu[k] - un[k]).abs().max().item())
        assert ef <= REL_TOL, "%s: %.3e > %.3e" % (k, ef, REL_TOL)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_operator_against_four_launches_and_float64(i):
    _, _, (act, _) = CASES[i]
    p = _inputs(i)
    _compare(_run(p, act, True), _run(p, act, False), _reference(p, act))


@pytest.mark.parametrize("co", [8, 16])
def test_signed_zeros_and_a_gradient_on_the_faces(co):
    """z holds exact zeros of both signs (a constant-zero block of x holding +0 and -0, a bias of -0, one channel's weights all
    negative and one's all positive), alpha < 0 makes the sign of a's zeros depend on them; da is non-zero on the volume's faces
    only, where the tiles' halos and ragged ends are."""
    n, sp = 2, (6, 10, 37)
    g = torch.Generator().manual_seed(91)
    x = torch.randn(n, 1, *sp, generator=g)
    x[:, :, :, :, 4:12] = 0.0
    x[:, :, :, :, 12:20] = -0.0
    w = 0.3 * torch.randn(co, 1, 3, 3, 3, generator=g)
    w[1], w[3] = -w[1].abs() - 0.1, w[3].abs() + 0.1
    b = torch.zeros(co)
    b[1], b[3] = -0.0, -0.0
    da = torch.zeros(n, co, *sp)
    face = torch.randn(n, co, *sp, generator=g)
    for sl in ((slice(None), slice(None), 0), (slice(None), slice(None), -1), (slice(None), slice(None), slice(None), 0),
               (slice(None), slice(None), slice(None), -1), (Ellipsis, 0), (Ellipsis, -1)):
        da[sl] = face[sl]
    p = {"x": x, "w": w, "b": b, "alpha": torch.full((1,), -0.3), "da": da}
    fu, un = _run(p, "prelu", True), _run(p, "prelu", False)
    zb = _bits(fu["z"])
    assert bool((zb == 0).any()) and bool((zb == -2 ** 31).any()), "the test's own precondition: zeros of both signs in z"
    _compare(fu, un, _reference(p, "prelu"))


def _geom(n, sp, co, x_ld=1, z_ld=None):
    from mri_epilepsy_diagnosis_amd import _lib
    d, h, w = sp
    return _lib.ConvGeom(n, d, h, w, 1, d, h, w, co, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, x_ld, co if z_ld is None else z_ld, _lib.F32)


@pytest.mark.parametrize("co", [8, 16])
def test_pitched_tensors_guards_and_exact_workspace(co):
    """x as channel 2 of a 4-channel buffer, z, a and da as channels [4, 4 + Co) of wider buffers inside guard bands; dW, db,
    dalpha and the workspaces (at exactly the queried size, poisoned with NaN) inside guard bands too.  Same bits as the dense
    four launches; one byte less of workspace is refused before anything is written."""
    from mri_epilepsy_diagnosis_amd import _lib
    L = _lib.lib()
    n, sp = 2, (5, 9, 33)
    gen = torch.Generator().manual_seed(17)
    p = {"x": torch.randn(n, 1, *sp, generator=gen), "w": 0.3 * torch.randn(co, 1, 3, 3, 3, generator=gen),
         "b": 0.2 * torch.randn(co, generator=gen), "alpha": _alpha("each", co, gen), "da": torch.randn(n, co, *sp, generator=gen)}
    un = _run(p, "prelu", False)
    wide = torch.zeros(n, 4, *sp, device=DEV).contiguous(memory_format=CL3D)
    wide[:, 2:3] = p["x"].to(DEV)
    x = wide[:, 2:3]
    w, b, alpha = p["w"].to(DEV), p["b"].to(DEV), p["alpha"].to(DEV)
    P = lambda v: None if v is None else ctypes.c_void_p(v.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ld = co + 8
    g = _geom(n, sp, co, x_ld=4, z_ld=ld)
    act = _lib.ACT_PRELU
    assert L.mri3d_conv_cin1_act_supported(ctypes.byref(g), ld, act, co, _lib.PASS_FWD, 16) == 1
    need = L.mri3d_conv_cin1_act_workspace_bytes(ctypes.byref(g), _lib.PASS_FWD)
    assert need > 0

    def poisoned(nbytes):
        ws = guarded(nbytes, torch.uint8)
        ws.flat[:nbytes // 8 * 8].view(torch.float64).fill_(float("nan"))
        return ws

    def forward(ws_bytes, expect=0):
        z, a = (SentinelSlice(n, ld, sp, F32, 4, co) for _ in range(2))
        ws = poisoned(ws_bytes)
        rc = L.mri3d_conv_cin1_act_fwd(ctypes.byref(g), ld, act, co, 0.0, P(x), P(w), P(b), P(alpha), P(z.slice), P(a.slice), P(ws.flat),
                                       ws_bytes, s)
        torch.cuda.synchronize()
        assert rc == expect, (rc, L.mri3d_last_error())
        ws.assert_guards_intact("forward workspace")
        for t, what in ((z, "z"), (a, "a")):
            t.assert_outside_intact(what)
            assert bool(t.slice_untouched().all() if expect else not t.slice_untouched().any()), what
        return z, a

    forward(need - 1, expect=-4)
    z, a = forward(need)
    assert torch.equal(_bits(to_ncdhw(z.slice)), _bits(un["z"])) and torch.equal(_bits(to_ncdhw(a.slice)), _bits(un["a"]))

    bwd_ok = L.mri3d_conv_cin1_act_supported(ctypes.byref(g), ld, act, co, _lib.PASS_WGRAD, 16)
    assert bwd_ok == (1 if co == 8 else 0)
    name = ctypes.create_string_buffer(64)
    _lib.check(L.mri3d_conv_cin1_act_route(ctypes.byref(g), ld, act, co, _lib.PASS_WGRAD, 16, name, 64), "route")
    assert name.value.decode() == ("cin1 act bwd co8" if co == 8 else "none")
    da = SentinelSlice(n, ld, sp, F32, 4, co)
    da.slice.copy_(p["da"].to(DEV))
    need = L.mri3d_conv_cin1_act_workspace_bytes(ctypes.byref(g), _lib.PASS_WGRAD)

    def backward(ws_bytes, expect=0):
        dw, db, dal = guarded((co, 1, 3, 3, 3), F32), guarded(co, F32), guarded(co, F32)
        ws = poisoned(ws_bytes)
        rc = L.mri3d_conv_cin1_act_bwd(ctypes.byref(g), ld, act, co, 0.0, P(x), P(z.slice), P(da.slice), P(alpha), P(dw.region),
                                       P(db.region), P(dal.region), P(ws.flat), ws_bytes, s)
        torch.cuda.synchronize()
        assert rc == expect, (rc, L.mri3d_last_error())
        for t, what in ((dw, "dW"), (db, "db"), (dal, "dalpha"), (ws, "backward workspace")):
            t.assert_guards_intact(what)
        z.assert_outside_intact("z after the backward"), da.assert_outside_intact("da")
        if expect:
            assert all(bool(t.untouched().all()) for t in (dw, db, dal))
            return None
        assert not any(bool(t.untouched().any()) for t in (dw, db, dal))
        return dw.region.cpu(), db.region.cpu(), dal.region.cpu()

    if co != 8:
        assert backward(need, expect=-2) is None     # MRI3D_ENOTSUP, as the predicate said
        return
    assert backward(need - 1, expect=-4) is None
    for got, k in zip(backward(need), ("dw", "db", "dalpha")):
        assert torch.equal(_bits(got), _bits(un[k])), k


def _model(seed=0):
    from mri_epilepsy_diagnosis_amd.unet import UNet
    torch.manual_seed(seed)
    return UNet(in_channels=1, out_classes=2, dimensions=3, num_encoding_blocks=3, out_channels_first_layer=8,
                normalization="batch", upsampling_type="linear", padding=True, activation="PReLU")


@pytest.mark.parametrize("shape", [(1, 1, 16, 16, 32), (2, 1, 8, 24, 40)])
def test_model_fused_first_equals_four_launches(shape):
    """Loss, every gradient and the BatchNorm running statistics after one step and after three FlatAdam steps."""
    from mri_epilepsy_diagnosis_amd import ops, parallel
    base = _model()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(*shape, generator=g).to(DEV)
    t = (torch.rand(*shape, generator=g) < 0.2).float().to(DEV)
    runs = {}
    for fused in (True, False):
        net = copy.deepcopy(base).to(DEV)
        assert net.fused_first            # the default
        net.fused_first = fused
        flat = parallel.FlatParams(net)
        opt = parallel.FlatAdam(flat, lr=1e-3)
        snaps = []
        for it in range(3):
            flat.zero_grad()
            if it == 0:
                loss, names = kernels_launched(lambda: ops.softmax_dice_loss(net(x), t))
                _, nb = kernels_launched(loss.backward)
                names = list(names) + list(nb)
            else:
                loss = ops.softmax_dice_loss(net(x), t)
                loss.backward()
            snaps.append((loss.detach().clone(), flat.grad.clone(), {k: v.clone() for k, v in net.named_buffers()}))
            opt.step(flat.all_reduce())
        runs[fused] = (snaps, names)
    count = lambda names, key: sum(1 for k in names if key in k)
    nf, nu = runs[True][1], runs[False][1]
    assert count(nf, "conv_cin1_act_fwd_kernel") == 1 and count(nf, "conv_cin1_act_bwd_kernel") == 1, nf
    assert count(nf, "conv_cin1_fwd_kernel") == 0 and count(nf, "conv_cin1_wgrad_kernel") == 0 and count(nf, "norm_act_bwd_frozen_kernel") == 0
    assert count(nu, "conv_cin1_act") == 0 and count(nu, "conv_cin1_fwd_kernel") == 1 and count(nu, "conv_cin1_wgrad_kernel") == 1
    for it, ((lf, gf, bf), (lu, gu, bu)) in enumerate(zip(runs[True][0], runs[False][0])):
        assert torch.equal(_bits(lf), _bits(lu)), "loss of step %d" % it
        assert torch.equal(_bits(gf), _bits(gu)) and gf.abs().max().item() > 0, "gradients of step %d" % it
        assert bf.keys() == bu.keys()
        for k in bf:
            assert torch.equal(bf[k], bu[k]), "%s after step %d" % (k, it)


def test_captured_step_with_fused_first_replays_eager_bit_exactly():
    from mri_epilepsy_diagnosis_amd import ops, parallel
    net = _model(3).to(DEV)
    assert net.fused_first
    flat = parallel.FlatParams(net)
    x = torch.randn(1, 1, 16, 16, 32, device=DEV)
    t = (torch.rand(1, 1, 16, 16, 32, device=DEV) < 0.2).float()
    cap = parallel.CapturedStep(flat, lambda: ops.softmax_dice_loss(net(x), t)).capture()
    state = {k: v.clone() for k, v in net.state_dict().items()}
    net.load_state_dict(state)
    l_g, g_g = cap.run().clone(), flat.grad.clone()
    net.load_state_dict(state)
    l_e = cap._eager().clone()
    assert torch.equal(l_g, l_e) and torch.equal(g_g, flat.grad) and g_g.abs().max().item() > 0
    cap.release()
